"""The sampling denoiser's attention kernels at N <= 64 under a PEAKED softmax: the case table of tests/test_gpu_denoiser_attn_peaked.py, whose
preconditions tests/test_denoiser_attn_cases_cpu.py asserts on the CPU.  Importable without a GPU.

Freshly initialised weights give an almost uniform softmax (median largest probability 0.03 .. 0.11): an absolute logit error of 1e-5
disappears.  A trained network is peaked; there exp(s - max) underflows for most keys, the 1 / sqrt(dh) folded into Q, the operand bits of
the in_proj product and the order of the score sum decide the result.  The networks here are the suite's seeded ones with the W_q and W_k
rows of every in_proj_weight multiplied by f (every logit f^2 larger):

  two_f4     train_long_checks.make_two(4.0): the default shape with 2 layers; fp64 median largest probability of every layer >= 0.8
  eight_f3   the 8-layer seeded_diffuser weights, f = 3; every layer >= 0.5 (at f = 4 the fp32 CPU oracle itself is 1.4 .. 4.7e-5 from fp64,
             so 4 x its distance is no bound under 1e-4: unusable)
  gen_hd8_f4 / gen_hd68_f4   EDGE_CFGS[0] / EDGE_CFGS[3] of tests/denoiser_cfgs.py (head dim 8 and 68), f = 4, on the shape-generic path;
             every layer >= 0.8 as for two_f4

The thresholds apply at N >= 7 (N = 1 is trivially 1, and 1 / N bounds the figure from below at 2 and 5 frames).

A case names the kernel it is about; ``kernel_of`` derives that name from engine_history_cases.den_plan, the Python restatement of
pd_den_step_plan that tests/test_engine_history_cpu.py holds to the header.  Shapes are the smallest at which each kernel's edges exist;
every large-batch case is just over 1 024 token rows."""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

import engine_history_cases as H
import train_checks as TC
import train_long_checks as TLC
from conftest import pose_err
from vit_checks import one_thread

TOL = 2e-5              # the suite's standing teacher-forced tolerance
MARGIN = 4.0            # x the fp32 CPU oracle's own distance from fp64 (test_long_denoiser_with_peaked_attention, vit_checks)
CEIL = 1e-4             # BASELINE.json north_star
PMAX_MIN_N = 7          # the peakedness thresholds apply from this many frames on
BENIGN_PMAX = 0.2       # what the same cases reach under f = 1


class Case(NamedTuple):
    kernel: str          # the attention kernel the case is about
    net: str
    B: int
    N: int
    t: int = 31
    split: int = 2       # PD_OPT_DENOISER_SPLIT (the small path ignores it; engines below 1 024 rows of capacity stay at 0)
    fused: int = 0       # PD_OPT_DENOISER_FUSED_ATTN
    long: int = 0        # PD_OPT_DENOISER_LONG_ATTN
    cap: Tuple[int, int] = (69, 64)       # (max_B, max_N) of the engine that runs it: one engine per (net, cap) serves several shapes

    @property
    def id(self) -> str:
        return f"{self.kernel}-{self.net}-b{self.B}n{self.N}-t{self.t}-s{self.split}f{self.fused}l{self.long}"

    @property
    def generic(self) -> bool:
        return self.kernel.startswith("pd_gen_")


SMALL_CAP, LARGE_CAP, N1_CAP = (7, 64), (69, 64), (1024, 1)
SMALL, SEQ0, SEQ1, SEQ2, MMA, QKV, GEN = ("pd_attn_kernel<false>", "pd_attn_seq_kernel<0>", "pd_attn_seq_kernel<1>", "pd_attn_seq_kernel<2>",
                                           "pd_attn_mma_kernel<2>", "pd_qkv_attn_kernel", "pd_gen_attn_kernel")
LONG0, LONG1, LONG2, GEN_LONG = "pd_attn_long_kernel<0>", "pd_attn_long_kernel<1>", "pd_attn_long_kernel<2>", "pd_gen_attn_long_kernel"

SMALL_SHAPES = [(3, 1), (3, 2), (5, 5), (2, 63), (2, 64), (7, 20)]          # 4 query rows per workgroup, lane = key
SEQ0_SHAPES = [(52, 20), (49, 21), (25, 41), (16, 64)]                      # rounds of 20 rows
MMA_SHAPES = [(1024, 1), (69, 15), (64, 16), (61, 17), (34, 31), (32, 32)]  # 16-row and 16-key tiles, zero row N
QKV_SHAPES = MMA_SHAPES + [(54, 19), (53, 20)]                              # G N = 95: the fullest image; a ragged last group
SEQ2_SHAPES = [(32, 33), (21, 50), (16, 64)]
LONG_SHAPES = [(52, 20), (32, 33), (16, 64)]


def _cap(B, N):
    return N1_CAP if B > LARGE_CAP[0] else LARGE_CAP


def _table() -> List[Case]:
    c: List[Case] = []
    two, eight = "two_f4", "eight_f3"
    c += [Case(SMALL, two, B, N, split=0, cap=SMALL_CAP) for B, N in SMALL_SHAPES]
    c += [Case(SEQ0, two, B, N, split=0) for B, N in SEQ0_SHAPES]
    c += [Case(MMA, two, B, N, cap=_cap(B, N)) for B, N in MMA_SHAPES]
    c += [Case(QKV, two, B, N, fused=2, cap=_cap(B, N)) for B, N in QKV_SHAPES]
    c += [Case(SEQ2, two, B, N) for B, N in SEQ2_SHAPES]
    c += [Case(LONG0, two, B, N, split=0, long=1) for B, N in LONG_SHAPES]
    c += [Case(LONG2, two, B, N, long=1) for B, N in LONG_SHAPES]
    c += [Case(LONG0, two, 7, 20, split=0, long=1, cap=SMALL_CAP)]
    # the other timesteps, one case per kernel
    for t in (99, 0):
        c += [Case(SMALL, two, 7, 20, t, split=0, cap=SMALL_CAP), Case(SEQ0, two, 52, 20, t, split=0), Case(MMA, two, 61, 17, t),
              Case(QKV, two, 61, 17, t, fused=2), Case(SEQ2, two, 21, 50, t), Case(LONG2, two, 52, 20, t, long=1)]
    # the 8-layer network, one case per kernel
    c += [Case(SMALL, eight, 7, 20, split=0, cap=SMALL_CAP), Case(SEQ0, eight, 52, 20, split=0), Case(MMA, eight, 61, 17),
          Case(QKV, eight, 61, 17, fused=2), Case(QKV, eight, 53, 20, fused=2), Case(SEQ2, eight, 21, 50), Case(LONG2, eight, 52, 20, long=1)]
    # the shape-generic path: the default shape forced onto it, and head dims 8 and 68
    c += [Case(GEN, two, B, N, split=0, cap=(5, 64)) for B, N in ((5, 13), (2, 64))]
    for net in ("gen_hd8_f4", "gen_hd68_f4"):
        c += [Case(GEN, net, B, N, split=0, cap=(3, 64)) for B, N in ((3, 33), (2, 64))]
    c += [Case(GEN, "gen_hd8_f4", 3, 33, t, split=0, cap=(3, 64)) for t in (99, 0)]
    return c


CASES = _table()
# mode 1 (bf16 planes) is a separately reported mode: finiteness and bitwise long-attn equality only, its distance from fp64 printed
MODE1_CASES = [Case(SEQ1, "two_f4", 52, 20, split=1), Case(SEQ1, "two_f4", 16, 64, split=1)]
# cases dropped because 4 x the fp32 oracle's own distance from fp64 reaches 1e-4 on the CPU (never run with a looser bound): none
DROPPED: List[str] = []


def kernel_of(case: Case) -> str:
    """The attention kernel one denoiser evaluation of ``case`` launches."""
    long = case.N > 64 or case.long != 0
    if case.generic or case.net.startswith("gen_"):                                # pd_denoiser_generic.hip:415-423
        return GEN_LONG if long else GEN
    has_streamed = case.cap[0] * case.cap[1] >= H.PD_STREAM_MIN_ROWS
    p = H.den_plan(case.B, case.N, case.split if has_streamed else 0, case.fused, case.long, False, has_streamed)
    if p["fused_attn"]:
        return QKV
    split_out = {H.SMALL: 0, H.STREAMED: 0, H.BF16_PLANES: 1, H.F16_PLANES: 2}[p["path"]]  # den_layer_small / _streamed / _bf16 / _f16
    if p["long_attn"]:
        return f"pd_attn_long_kernel<{split_out}>"
    if p["path"] == H.SMALL:
        return SMALL
    if p["attn_mma"]:
        return MMA
    return f"pd_attn_seq_kernel<{split_out}>"


def bitwise_twin(case: Case) -> Optional[Case]:
    """The case whose result ``case``'s must equal bit for bit (include/pd_engine.h): the two-launch form of a fused case; the kernel a forced
    key-tiled kernel replaces, except pd_attn_mma_kernel (MFMA-ordered sums: rounding-level, held to the fp64 rule alone)."""
    if case.kernel == QKV:
        return case._replace(kernel=MMA, fused=0)
    if case.long:
        twin = case._replace(long=0)
        twin = twin._replace(kernel=kernel_of(twin))
        return None if twin.kernel == MMA else twin
    return None


# ---- networks ------------------------------------------------------------------------------------------------------------------------
GEN_CFG_INDEX = {"gen_hd8_f4": 0, "gen_hd68_f4": 3}          # denoiser_cfgs.EDGE_CFGS: head dim 8 (d = 32); head dim 68 (d = 544, no pivot)
QK_FACTOR = {"two_f4": 4.0, "eight_f3": 3.0, "gen_hd8_f4": 4.0, "gen_hd68_f4": 4.0}
PMAX_THRESHOLD = {"two_f4": 0.8, "eight_f3": 0.5, "gen_hd8_f4": 0.8, "gen_hd68_f4": 0.8}   # per layer, by f: 0.8 at f = 4, 0.5 at f = 3


def _scaled(sd: Dict[str, torch.Tensor], f: float) -> Dict[str, torch.Tensor]:
    sd = {k: v.detach().clone() for k, v in sd.items()}
    for k, v in sd.items():
        if k.endswith("in_proj_weight"):
            v[: 2 * v.shape[1]] *= f
    return sd


@functools.lru_cache(maxsize=None)
def network(name: str, benign: bool = False):
    """-> (fp32 state dict on the CPU, train_checks.Net, engine keyword arguments, z_dim); ``benign``: the same network at f = 1."""
    f = 1.0 if benign else QK_FACTOR[name]
    if name == "two_f4":
        return _scaled(TLC.make_two().state_dict(), f), TC.Net(2, 4, True), dict(num_layers=2), 384
    if name == "eight_f3":
        from posediffusion_amd import synth
        diff = synth.make_diffuser(seed=0)
        synth.randomize_norm_and_bias_(diff.model)                # conftest.seeded_diffuser's construction
        return _scaled(diff.model.state_dict(), f), TC.DEFAULT_NET, dict(num_layers=8), 384
    from denoiser_cfgs import EDGE_CFGS, build_dropin
    cfg = EDGE_CFGS[GEN_CFG_INDEX[name]]
    kw = dict(num_layers=cfg.layers, nhead=cfg.heads, norm_first=cfg.norm_first, pivot=cfg.pivot)
    return _scaled(build_dropin(cfg, seed=40 + cfg.d).state_dict(), f), TC.Net.of_cfg(cfg), kw, cfg.z


def inputs(case: Case):
    """randn x and z of a (network, B, N), from their seed alone."""
    z_dim = network(case.net)[3]
    g = torch.Generator().manual_seed(7000 + 100 * case.B + case.N)
    return torch.randn(case.B, case.N, 9, generator=g), torch.randn(case.B, case.N, z_dim, generator=g)


# ---- oracle --------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def oracle(sd, net: TC.Net, x, t: int, z, dtype):
    """train_checks.denoiser_forward in ``dtype`` -> (out [B, N, 9], pmax: per layer [B, nhead, N])."""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    out, info = TC.denoiser_forward(sd, net, x.to(dtype), torch.full((x.shape[0],), t, dtype=torch.long), z.to(dtype))
    return out, info["pmax"]


@torch.no_grad()
def argmax_keys(sd64, net: TC.Net, x, t: int, z) -> List[int]:
    """The sorted key indices that hold the maximum of some softmax row, over all layers, heads and sequences (float64)."""
    sd64 = {k: v.double() for k, v in sd64.items() if v.is_floating_point()}
    lgs = TLC._log_probs(sd64, net, x.double(), torch.full((x.shape[0],), t, dtype=torch.long), z.double())
    return sorted(set(torch.cat([lg.argmax(dim=-1).flatten() for lg in lgs]).tolist()))


def median_pmax(pmax) -> List[float]:
    return [p.flatten().median().item() for p in pmax]


@functools.lru_cache(maxsize=None)
def reference(net: str, B: int, N: int, t: int) -> Dict:
    """Computed once per (network, shape, t) and shared, never modified: the fp64 output, the fp32 CPU oracle's own distance from it (on
    one thread: its sums do not depend on the host), the bound of the GPU test and the fp64 median largest probability per layer."""
    case = Case("", net, B, N, t)
    sd, nt, _, _ = network(net)
    x, z = inputs(case)
    out64, pmax = oracle(sd, nt, x, t, z, torch.float64)
    with one_thread():
        out32, _ = oracle(sd, nt, x, t, z, torch.float32)
    e32 = pose_err(out32, out64)
    return {"out64": out64, "e32": e32, "bound": max(TOL, MARGIN * e32), "pmax": median_pmax(pmax)}


def reference_of(case: Case) -> Dict:
    return reference(case.net, case.B, case.N, case.t)


def worst_row(out, ref64) -> Tuple[int, int, float]:
    """(sequence, frame, error) of the row with the largest error, each pose column group relative to its own largest reference magnitude."""
    from conftest import POSE_GROUPS
    out, ref64 = out.detach().cpu().double(), ref64.double()
    rel = torch.zeros(out.shape[:2], dtype=torch.float64)
    for sl in POSE_GROUPS.values():
        rel = torch.maximum(rel, (out[..., sl] - ref64[..., sl]).abs().amax(dim=-1) / ref64[..., sl].abs().max().clamp_min(1e-30))
    i = int(rel.argmax())
    return i // out.shape[1], i % out.shape[1], rel.flatten()[i].item()
