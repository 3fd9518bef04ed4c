"""Same-box A / B of the two trainers (include/pd_engine_train.h, include/pd_engine_vit_train.h) between engine libraries: the sha256 of
every output of a fixed list of forward + backward calls (bitwise comparison between libraries; parity is the tests' business), and the
comparison of two rocprofv3 kernel traces of that list.  One fresh child process per library; the child takes its library from
PD_ENGINE_LIB.

    python tools/trainer_ab.py libA.so libB.so [...]                      hashes of every library, equal or not (exit status 1 if not)
    PD_ENGINE_LIB=lib.so python tools/trainer_ab.py --child               what the parent starts; also the program to put behind a profiler
    python tools/trainer_ab.py --traces dirA dirB                         the ordered launches of two `rocprofv3 --kernel-trace` outputs

The list: the denoiser trainer at 20 frames (one reduction chunk at 60 and 240 rows, two at 400) and at 65 frames (key-tiled attention),
each with and without dropout at all four sites; the backbone trainer with one scale, with three scales whose reductions stay in one
chunk (accumulation through the GEMM's resid = C) and with three scales of which one takes two chunks (accumulating reduce), with a
resampled trained grid, and with a ``want`` subset that leaves out fc1 / qkv weights (their LayerNorm recompute is then not launched)."""
import csv
import glob
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DROP = dict(dropout_p=0.1, dropout_sites=15, seed=51, step=2)
# (label, B, N, dropout)
DENOISER = [("n20 60 rows", 3, 20, False), ("n20 60 rows dropout", 3, 20, True), ("n20 240 rows (1 chunk)", 12, 20, False),
            ("n20 400 rows (2 chunks)", 20, 20, False), ("n20 400 rows dropout", 20, 20, True), ("n65 tiled", 1, 65, False),
            ("n65 tiled dropout", 1, 65, True), ("n65 x 5 tiled dropout (2 chunks)", 5, 65, True)]
# (label, images, H, W, scales, depth, leave out fc1 / qkv weights)
BACKBONE = [("one scale", 2, 48, 32, (1,), 1, False), ("three scales <= 256 rows", 3, 96, 96, (1, 1 / 2, 1 / 3), 2, False),
            ("three scales 394 rows", 2, 224, 224, (1, 1 / 2, 1 / 3), 2, False), ("resampled trained grid", 1, 224, 232, (1,), 1, False),
            ("want subset", 3, 96, 96, (1, 1 / 2, 1 / 3), 2, True)]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def child():
    import torch
    import vit_train_checks as VC
    from posediffusion_amd import synth
    from posediffusion_amd.schedule import diffusion_buffers
    from posediffusion_amd.train import PoseTrainer, shape_from_modules
    from posediffusion_amd.vit_train import VitTrainer, shape_from_module, token_rows
    dev = torch.device("cuda:0")
    two = synth.make_diffuser(seed=0, num_layers=2)
    synth.randomize_norm_and_bias_(two.model)
    params = {k: v.detach().to(dev).contiguous() for k, v in two.model.state_dict().items() if v.is_floating_point()}
    shape = dict(shape_from_modules(two.model), objective="pred_noise")
    for label, B, N, drop in DENOISER:
        g = torch.Generator().manual_seed(100 * B + N)
        x0, noise, z = torch.randn(B, N, 9, generator=g), torch.randn(B, N, 9, generator=g), torch.randn(B, N, shape["z_dim"], generator=g)
        t = torch.randint(0, 100, (B,), generator=g)
        tr = PoseTrainer(shape, diffusion_buffers(), B, N, device=dev, max_frames=256)
        out = tr.forward(params, x0.to(dev), z.to(dev), t.to(dev), noise.to(dev), "l1", **(DROP if drop else {}))
        grads = tr.backward(params, torch.full((B, N, 9), 1.0 / (B * N * 9), device=dev))
        tr.check_async()
        for k in ("loss", "model_out"):
            print(f"denoiser | {label} | out.{k} | {_sha(out[k])}")
        for k in sorted(grads):
            print(f"denoiser | {label} | {k} | {_sha(grads[k])}")
        tr.close()
    for label, n, H, W, scales, depth, subset in BACKBONE:
        case = VC.Case(n, H, W, scales, depth)
        net = VC.make_net(depth)
        vparams = {k: v.detach().to(dev).contiguous() for k, v in net.named_parameters()}
        images, g_z = VC.inputs(case)
        want = [k for k in vparams if not k.endswith(("mlp.fc1.weight", "attn.qkv.weight"))] if subset else None
        tr = VitTrainer(shape_from_module(net), n, n * token_rows(H, W, scales), len(scales), device=dev)
        zf = tr.forward(vparams, images.to(dev), scales)
        grads = tr.backward(vparams, g_z.to(dev), want)
        torch.cuda.synchronize()
        print(f"backbone | {label} | z | {_sha(zf)}")
        for k in sorted(grads):
            print(f"backbone | {label} | {k} | {_sha(grads[k])}")
        tr.close()


def _launches(trace_dir):
    """the launches of a rocprofv3 --kernel-trace output in start order: (kernel name without its arguments, every grid / workgroup / LDS column)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (trace_dir, files)
    with open(files[0]) as fh:
        rows = list(csv.DictReader(fh))
    cols = [c for c in rows[0] if re.search(r"Grid_Size|Workgroup_Size|LDS|Group_Segment", c)]
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    return cols, [(r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0],) + tuple(r[c] for c in cols) for r in rows]


# the kernels this comparison admits under another name: (old, new)
RENAMED = [("pd_vt_ln_kernel", "pd_tr_ln_kernel"), ("pd_vt_reduce_acc_kernel<float>", "pd_tr_reduce_kernel<float, true>"),
           ("pd_vt_reduce_acc_kernel<double>", "pd_tr_reduce_kernel<double, true>"), ("pd_tr_reduce_kernel<float>", "pd_tr_reduce_kernel<float, false>"),
           ("pd_tr_reduce_kernel<double>", "pd_tr_reduce_kernel<double, false>")]


def _short(name):
    """template arguments that only some libraries' sources have: the strip GEMM as <EPI, RT>, the fused attention kernel as <BARE>"""
    name = re.sub(r"(pd_gemm_strip_kernel<\d+, \d+), true, 1, 0, true>", r"\1>", name.replace("void ", ""))
    return re.sub(r"(pd_qkv_attn_kernel<\d+), false>", r"\1>", name)


def traces(dir_a, dir_b):
    (cols, a), (cols_b, b) = _launches(dir_a), _launches(dir_b)
    assert cols == cols_b
    ren = dict(RENAMED)
    mapped = [(ren.get(_short(r[0]), _short(r[0])),) + r[1:] for r in a]
    b = [(_short(r[0]),) + r[1:] for r in b]
    names_raw = sum(1 for x, y in zip(a, b) if _short(x[0]) != y[0])
    shape_diff = [i for i, (x, y) in enumerate(zip(mapped, b)) if x[1:] != y[1:]]
    name_diff = [i for i, (x, y) in enumerate(zip(mapped, b)) if x[0] != y[0]]
    digest = lambda rows: hashlib.sha256(repr(rows).encode()).hexdigest()[:16]       # noqa: E731
    print(f"columns compared: Kernel_Name {' '.join(cols)}")
    print(f"launches: {len(a)} / {len(b)}; engine kernels (pd_tr_ / pd_vt_): {sum('pd_tr_' in r[0] or 'pd_vt_' in r[0] for r in a)} / "
          f"{sum('pd_tr_' in r[0] or 'pd_vt_' in r[0] for r in b)}")
    print(f"launches whose (grid, workgroup, LDS) columns differ: {len(shape_diff)}; sha256 of the ordered lists {digest([r[1:] for r in a])} / {digest([r[1:] for r in b])}")
    print(f"launches whose names differ as recorded: {names_raw}; after mapping the renamed kernels: {len(name_diff)}; "
          f"sha256 of the mapped (name, shape) lists {digest(mapped)} / {digest(b)}")
    kinds = {}
    for i in shape_diff:                                 # which kernel, which columns, from what to what
        key = (b[i][0],) + tuple(f"{c} {x} -> {y}" for c, x, y in zip(cols, mapped[i][1:], b[i][1:]) if x != y and not c.startswith("Grid"))
        kinds[key] = kinds.get(key, 0) + 1
    for key, n in sorted(kinds.items()):
        print(f"   {n} launches of {key[0]}: {'; '.join(key[1:]) or 'grid'}")
    for i in name_diff[:10]:
        print("  ", i, mapped[i], b[i])
    return 0 if len(a) == len(b) and not shape_diff and not name_diff else 1


def main(argv):
    if argv[:1] == ["--child"]:
        child()
        return 0
    if argv[:1] == ["--traces"]:
        return traces(argv[1], argv[2])
    results = []
    for lib in argv:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, PD_ENGINE_LIB=os.path.abspath(lib)),
                             capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            print(out.stdout[-2000:], out.stderr[-4000:])
            return out.returncode or 1
        results.append([l for l in out.stdout.splitlines() if " | " in l])
    keys = [l.rsplit(" | ", 1)[0] for l in results[0]]
    assert all([l.rsplit(" | ", 1)[0] for l in r] == keys for r in results)
    differing = 0
    for i, k in enumerate(keys):
        hashes = [r[i].rsplit(" | ", 1)[1] for r in results]
        differing += len(set(hashes)) > 1
        print(f"{k:90s} {' '.join(hashes)}{'   DIFFER' if len(set(hashes)) > 1 else ''}")
    print(f"{len(keys)} outputs, {len(set(l.rsplit(' | ', 1)[1] for l in results[0]))} distinct hashes, {differing} differ between {len(argv)} libraries")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
