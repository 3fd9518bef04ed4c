"""No GPU: the trainer at 65 ... 256 frames (PD_TR_OPT_MAX_FRAMES, include/pd_engine_train.h) as far as it can be pinned without
a device -- the float64 mirror of the key-tiled two-phase attention (tests/train_long_checks.py) against autograd of plain softmax
attention, the dynamic-LDS size functions compiled into a stand-alone host program, the C-ABI of the two option functions, the drop-in's
``engine_grad_max_frames`` rules, the keep rate of every dropout mask tests/test_gpu_train_long.py uses, and the precondition of its
sharp-softmax case."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import train_checks as TC
import train_dropout_checks as D
import train_long_checks as L
from posediffusion_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")
CU_LDS_BYTES = 163840                                        # 160 KB of LDS per compute unit (gfx950)


# ------------------------------------------------------------------------------------------------ the tiled scheme against plain attention
def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "site0-mask"])
@pytest.mark.parametrize("N,hd", [(1, 16), (64, 16), (65, 24), (130, 16), (256, 8)], ids=lambda v: str(v))
def test_tiled_two_phase_mirror_is_softmax_attention_and_its_gradient(N, hd, masked):
    g = torch.Generator().manual_seed(600 + N)
    q, k, v, dO = (torch.randn(N, hd, generator=g, dtype=torch.float64) for _ in range(4))
    q = q * 3.0                                              # scores of a few units: probabilities spread over decades
    scale = 1.0 / math.sqrt(hd)
    keep, ks = None, 1.0
    if masked:
        keep, ks = torch.from_numpy(D.keep_mask(N, N, 1, 0, 77, 2, 0.3)), D.scale_of(0.3)
        if N == 1:
            keep = torch.ones(1, 1, dtype=torch.bool)        # (a dropped single key makes every gradient zero: nothing to compare)
    ctx, stats = L.tiled_forward(q, k, v, scale, keep, ks)
    dq, dk, dv = L.tiled_backward(q, k, v, dO, scale, stats, keep, ks)
    want = L.plain_attention_grads(q, k, v, dO, scale, keep, ks)
    for name, got, ref in zip(("ctx", "dq", "dk", "dv"), (ctx, dq, dk, dv), want):
        e = _rel(got, ref)
        print(f"N {N} hd {hd} masked {masked} {name}: {e:.3e}")
        if N == 1 and name in ("dq", "dk"):
            assert got.abs().max().item() == 0.0, name       # one key: P = 1, dS = 1 (dP - dP) = 0 exactly
        else:
            assert e <= 1e-12, (name, e)


# ------------------------------------------------------------------------------------------------ LDS sizes, on the host
_LDS_PROGRAM = r"""
#define PD_TR_LATTN_HOST_ONLY
#include "pd_train_lattn.h"
#include <stdio.h>
int main() {
    const int shapes[][2] = {{256, 128}, {65, 128}, {64, 128}, {256, 8}, {130, 24}, {1, 12}};
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i)
        printf("%d %d %zu %zu %zu\n", shapes[i][0], shapes[i][1], pd_tr_lattn_lds(shapes[i][0], shapes[i][1]),
               pd_tr_lattn_bwd_rows_lds(shapes[i][0], shapes[i][1]), pd_tr_lattn_bwd_keys_lds(shapes[i][0], shapes[i][1]));
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None, reason="no host C++ compiler")
def test_lds_size_functions_are_host_includable_and_fit_a_compute_unit(tmp_path):
    src, exe = tmp_path / "lds.cpp", tmp_path / "lds"
    src.write_text(_LDS_PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++")
    out = subprocess.run([cxx, "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert len(rows) == 6
    for N, hd, fwd, a, b in rows:
        nt, ld = -(-N // 64), hd + 4
        assert fwd == 4 * ((64 + 16) * ld + 16 * 64 * nt), (N, hd, fwd)             # tile, 16 scaled query rows, their probabilities
        assert a == 4 * ((64 + 32) * ld + 16 * 64 * nt), (N, hd, a)                 # ... and the dO rows
        assert b == 4 * ((128 + 32) * ld + 2 * 16 * 65), (N, hd, b)                 # K and V tile, 16 + 16 rows, two [16][65] blocks
    N, hd, fwd, a, b = rows[0]
    print(f"dynamic LDS at 256 frames, head dim 128: forward {fwd} B, backward rows {a} B, backward keys {b} B")
    assert (N, hd) == (256, 128) and max(fwd, a, b) <= CU_LDS_BYTES


# ------------------------------------------------------------------------------------------------ ABI
def _header():
    with open(os.path.join(ROOT, "include", "pd_engine_train.h")) as fh:
        return fh.read()


def test_option_functions_are_bound_and_refuse_a_null_handle():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    for name in ("pd_trainer_set_option", "pd_trainer_get_option"):
        assert name in _lib.TRAIN_SIGNATURES and getattr(lib, name).argtypes == _lib.TRAIN_SIGNATURES[name][1]
    assert lib.pd_trainer_set_option(None, _lib.PD_TR_OPT_MAX_FRAMES, 256) == -1
    assert "pd_trainer_set_option" in _lib.last_error()
    v = C.c_int(7)
    assert lib.pd_trainer_get_option(None, _lib.PD_TR_OPT_MAX_FRAMES, C.byref(v)) == -1 and v.value == 7
    assert "pd_trainer_get_option" in _lib.last_error()


def test_option_constants_equal_the_headers():
    hdr = _header()
    for name in ("PD_TR_OPT_MAX_FRAMES", "PD_TR_OPT_LONG_ATTN"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert "N <= 64 frames by default, up to 256 with PD_TR_OPT_MAX_FRAMES" in hdr


# ------------------------------------------------------------------------------------------------ drop-in
def test_engine_grad_max_frames_defaults_to_64_and_is_range_checked_without_a_device():
    diff = synth.make_diffuser(seed=0, num_layers=1)
    assert diff.engine_grad_max_frames == 64
    x = torch.zeros(1, 2, 9)
    for bad in (63, 257):
        diff.engine_grad_max_frames = bad
        for grad in (False, True):
            diff.engine_grad = grad
            with pytest.raises(ValueError, match=f"engine_grad_max_frames = {bad}"):
                diff.p_losses(x, torch.tensor([3]), z=torch.zeros(1, 2, 384), noise=x)
    diff.engine_grad, diff.engine_grad_max_frames = True, 64
    diff.eval()
    x = torch.zeros(1, 65, 9)
    with pytest.raises(RuntimeError, match=r"limit of 64 frames.*engine_grad_max_frames = 65"):     # before any device check
        diff.p_losses(x, torch.tensor([3]), z=torch.zeros(1, 65, 384), noise=x)
    diff.engine_grad_max_frames = 256
    with pytest.raises(RuntimeError, match="AMD GPU"):       # admitted: the next thing in the way is the missing device
        diff.p_losses(x, torch.tensor([3]), z=torch.zeros(1, 65, 384), noise=x)


# ------------------------------------------------------------------------------------------------ the masks of the GPU cases
def _case_masks(case):
    _, cfg, B, N, p, sites, seed, step, _, _ = case
    d, nhead, ff, layers = D.CONFIGS[cfg]
    for l in range(layers):
        for s, (rows, cols) in enumerate(D.site_shapes(B, N, nhead, d, ff)):
            if sites & (1 << s):
                yield l, s, D.keep_mask(rows, cols, l, s, seed, step, p)


@pytest.mark.parametrize("case", L.MASKED_CASES, ids=[c[0] for c in L.MASKED_CASES])
def test_keep_rate_of_every_mask_the_long_gpu_suite_uses(case):
    p = float(np.float32(case[4]))
    for l, s, m in _case_masks(case):
        n, rate = m.size, m.mean()
        assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (l, s, rate, n)      # the bound of tests/test_train_dropout_cpu.py


def test_cases_cover_what_they_are_meant_to():
    assert sorted({n for _, n, _, _ in L.EDGE_CASES}) == [65, 128, 129, 192, 193, 255, 256]
    assert {(c[2], c[3], c[4], c[5]) for c in L.DROPOUT_CASES} == {(1, 65, 0.1, D.ATTN), (1, 65, 0.5, D.ATTN), (1, 65, 0.1, D.ALL), (1, 65, 0.5, D.ALL),
                                                                   (2, 256, 0.1, D.ALL), (1, 130, 0.1, D.ALL)}
    assert [c[7] for c in L.DROPOUT_CASES if c[3] == 130] == [3]
    assert L.BITWISE_NS == (1, 5, 63, 64) and L.CAPACITY_BATCHES == [(2, 256), (3, 7), (1, 65), (2, 130), (3, 7)]


def test_sharp_case_meets_its_precondition_on_float64():
    from test_gpu_train_grad import _inputs
    den = L.make_two(L.SHARP_QK)
    sd = {k: v.detach().clone() for k, v in den.state_dict().items() if v.is_floating_point()}
    net = TC.Net(2, 4, True)
    drawn = _inputs(L.SHARP_B, L.SHARP_N, 384, L.SHARP_SEED)
    med, shares = L.sharp_precondition(L.attention_probs(sd, net, drawn))
    print(f"as drawn: median {med:.3f}, shares {[f'{s:.3f}' for s in shares]}")
    assert shares[2] < 0.10                                  # why the last tile's two frames are fitted: 2 keys of 130 hold 1.5 % of the maxima
    L.check_sharp_precondition(sd, net, L.fit_last_tile(sd, net, drawn))
