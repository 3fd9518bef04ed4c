"""Same-box A / B of one denoiser step between engine libraries, over a list of (engine size, batch, GEMM mode, attention option) entries:
per entry the sha256 of one step's output (bitwise comparison between libraries; parity is the tests' business) and the step-alone time
(pd_time_kernel).  One fresh child process per library; the child takes its library from PD_ENGINE_LIB.

    python tools/den_ab.py [--rounds R] [--reps K] [libA.so libB.so ...]
    PD_ENGINE_LIB=lib.so python tools/den_ab.py --child [--reps K]          (what the parent starts; also the program to put behind a profiler)

The default list covers every decision of a step's launch plan (csrc/pd_denoiser_plan.h) on both of its sides, for a chip of 256 CUs."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PD_OPT_DENOISER_SPLIT, PD_OPT_DENOISER_FUSED_ATTN = 2, 5
DFLT = None   # split / fused: leave the engine's default (an engine of fewer than 1 024 token rows has no split modes)
# (max_B, max_N, B, N, split mode, fused option)
ENTRIES = (
    # small path
    [(13, 50, B, N, DFLT, DFLT) for B, N in ((1, 1), (1, 20), (8, 20), (2, 33), (1, 50))]
    # ... its 32- / 16-wide tile switch at gemm_wide_min_tiles = 200: MT = 4 / 5 (1 536 wide), 6 / 7 (1 024 wide), 12 / 13 (512 wide)
    + [(13, 50, B, 32, DFLT, DFLT) for B in (4, 5, 6, 7, 12, 13)]
    # 1 020 and 1 040 token rows on a streamed-capable engine: small path against streamed path
    + [(257, 20, B, 20, DFLT, DFLT) for B in (51, 52)]
    # every GEMM mode under every attention option
    + [(257, 20, B, 20, split, fused) for B in (52, 256) for split in (0, 1, 2) for fused in (0, 1, 2)]
    # the fused kernel's fill rule: 192 workgroups are 3 / 4 of 256 CUs (B = 189), 260 need a second round (B = 257); 103: the +2 % case
    + [(257, 20, B, 20, 2, 1) for B in (103, 188, 189, 256, 257)]
    # 96-row tiles of the 512-wide strip GEMMs: 4 096 rows no, 4 128 and 6 144 yes, 6 176 no
    + [(193, 32, B, 32, 2, DFLT) for B in (128, 129, 192, 193)]
    # N > 32: two launches with pd_attn_seq_kernel whatever the option
    + [(32, 33, 32, 33, 2, 2)]
)


def child(reps):
    import torch
    from posediffusion_amd import synth
    from posediffusion_amd.engine import PoseEngine
    from posediffusion_amd.host import denoiser_state
    dev = torch.device("cuda:0")
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(dev)
    eng, size = None, None
    for max_B, max_N, B, N, split, fused in ENTRIES:
        if size != (max_B, max_N):
            if eng is not None:
                eng.close()
            eng = PoseEngine(denoiser_state(diff.model), {n: v for n, v in diff.named_buffers(recurse=False)}, device=dev, max_B=max_B, max_N=max_N)
            size = (max_B, max_N)
            defaults = None
            if max_B * max_N >= 1024:
                defaults = (eng.get_option(PD_OPT_DENOISER_SPLIT), eng.get_option(PD_OPT_DENOISER_FUSED_ATTN))
        if defaults is not None:
            eng.set_option(PD_OPT_DENOISER_SPLIT, defaults[0] if split is None else split)
            eng.set_option(PD_OPT_DENOISER_FUSED_ATTN, defaults[1] if fused is None else fused)
        z = synth.make_z(B, N).to(dev)
        x = torch.randn(B, N, 9, generator=torch.Generator().manual_seed(3))
        out = eng.denoise(x.to(dev), z, 40).cpu().contiguous()
        h = hashlib.sha256(out.numpy().tobytes()).hexdigest()[:16]
        ts = [eng.time_kernel(0, B, N, reps=reps) * 1e3 for _ in range(3)]
        mode = "-" if split is None else split
        opt = "-" if fused is None else fused
        print(f"  engine {max_B:3d} x {max_N:2d}  B={B:3d} N={N:2d} ({B * N:4d} rows) split {mode} fused {opt}: sha256 {h}  finite {int(bool(torch.isfinite(out).all()))}"
              f"  step alone {min(ts):7.1f} us (of {[round(t, 1) for t in ts]})", flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rounds", type=int, default=2, help="passes over the libraries, alternating")
    ap.add_argument("--reps", type=int, default=30, help="steps per timing (three timings per entry, the fastest counts)")
    ap.add_argument("libs", nargs="*")
    args = ap.parse_args()
    if args.child:
        child(args.reps)
    else:
        libs = args.libs or [os.path.join(ROOT, "posediffusion_amd", "lib", "libpd_engine.so")]
        for rnd in range(args.rounds):
            for lib in libs:
                print(f"{os.path.relpath(lib, ROOT)} (round {rnd}):", flush=True)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)],
                                     env=dict(os.environ, PD_ENGINE_LIB=os.path.abspath(lib)), check=False)
                if res.returncode != 0:       # a child that failed may have faulted the GPU: start nothing after it
                    sys.exit(f"child exited with {res.returncode}: stopping")
