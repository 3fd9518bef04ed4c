"""GPU: pd_train_images (include/pd_engine_images.h) through its C-ABI against the fp64 yardstick of
tests/train_images_checks.py -- the resize at every kind of source side and crop box, the colour stage in all 24 orders, the per-frame
statuses with canaries around the output, and the host-side argument refusals.  The worst figures are printed when the module is done
and written to $PD_PARITY_DIR/train_images_parity.txt where that variable names a directory (kept as profiles/train_images_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_images_checks as IC
from posediffusion_amd import _lib
from posediffusion_amd.images import colour_entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 123456.0
_FIGURES = {}     # line name -> text
_ALONE = {}       # (case name, fill) -> the frame's output when launched alone


def launch(frames, boxes, S=32, fill=0, colours=(), seq=None, pads=None, canary=False):
    """frames: uint8 [H, W, 3] arrays; boxes: (x0, y0, side); pads: bytes in front of each frame.  -> (out [F, 3, S, S], status [F])
    (with canary=True also the guard words before and after ``out``)."""
    dev = torch.device("cuda:0")
    Fn = len(frames)
    pads = pads or [0] * Fn
    seq = seq if seq is not None else [-1] * Fn
    ftab = (_lib.pd_img_frame * max(Fn, 1))()
    chunks, off = [], 0
    for k, (fr, b) in enumerate(zip(frames, boxes)):
        chunks.append(np.zeros(pads[k], np.uint8))
        off += pads[k]
        h, w = (fr.shape[0], fr.shape[1]) if fr is not None else b[3:]
        ftab[k] = _lib.pd_img_frame(off, h, w, b[0], b[1], b[2], seq[k])
        if fr is not None:
            chunks.append(np.ascontiguousarray(fr).reshape(-1))
            off += fr.size
    chunks.append(np.zeros(16, np.uint8))
    pixels = torch.from_numpy(np.concatenate(chunks)).to(dev)
    ftab_d = torch.from_numpy(np.frombuffer(ftab, dtype=np.uint8).copy()).to(dev)
    ctab = (_lib.pd_img_colour * max(len(colours), 1))(*[colour_entry(c) if isinstance(c, dict) else c for c in colours])
    ctab_d = torch.from_numpy(np.frombuffer(ctab, dtype=np.uint8).copy()).to(dev)
    guard = 64
    buf = torch.full((guard + Fn * 3 * S * S + guard,), CANARY, device=dev)
    status = torch.full((Fn + 2,), -7, dtype=torch.int32, device=dev)
    lib = _lib.load()
    need = lib.pd_train_images_workspace_bytes(Fn, S)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    _lib.check(lib.pd_train_images(pixels.data_ptr(), ftab_d.data_ptr(), Fn, ctab_d.data_ptr() if colours else None, len(colours), S, fill,
                                   buf.data_ptr() + 4 * guard, status.data_ptr() + 4, ws.data_ptr(), ws.numel() * 8,
                                   torch.cuda.current_stream().cuda_stream), "pd_train_images")
    torch.cuda.synchronize()
    out, st = buf[guard:guard + Fn * 3 * S * S].view(Fn, 3, S, S).cpu(), status[1:1 + Fn].cpu()
    if canary:
        ok = bool((buf[:guard] == CANARY).all()) and bool((buf[-guard:] == CANARY).all()) and int(status[0]) == -7 and int(status[-1]) == -7
        return out, st, ok
    return out, st


def record(name, text):
    _FIGURES[name] = text


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    if not _FIGURES:
        return
    text = "pd_train_images against the fp64 yardstick (tests/train_images_checks.py): worst absolute error, its bound\n"
    text += "".join(f"{k:28s} {_FIGURES[k]}\n" for k in sorted(_FIGURES))
    print(text)
    out = os.environ.get("PD_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "train_images_parity.txt"), "w") as fh:
            fh.write(text)


def alone(name, H, W, box, fill):
    key = (name, fill)
    if key not in _ALONE:
        out, st = launch([IC.case_picture(name, H, W)], [box], fill=fill, pads=[1 if "odd" in name else 0])
        assert st.tolist() == [0]
        _ALONE[key] = out[0]
    return _ALONE[key]


CASES_FILL = [(c, 0) for c in IC.ALL_CASES] + [(c, 255) for c in IC.BORDER_CASES]


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fill", CASES_FILL, ids=[f"{c[0]}-fill{f}" for c, f in CASES_FILL])
def test_resize_against_the_fp64_yardstick(case, fill):
    name, H, W, box = case
    img = IC.case_picture(name, H, W)
    got = alone(name, H, W, box, fill)
    ref, (tx, ty) = IC.yardstick(img, box, 32, fill)
    err, bound = (got.double() - ref).abs().max().item(), IC.resize_bound(tx, ty)
    print(f"{name} fill {fill}: err {err:.3e} bound {bound:.3e} taps {tx}")
    record(f"resize {name} fill {fill}", f"err {err:.3e}  bound {bound:.3e}  taps {tx}")
    assert err <= bound
    if name == "side32":                                    # an identity crop inside the picture: the bits of u8 / 255
        assert torch.equal(got, torch.from_numpy(img).permute(2, 0, 1).float().div(255))
    if name == "side33":                                    # ATen's fp32 path misplaces near-zero edge taps; this kernel must not
        x = torch.from_numpy(img).permute(2, 0, 1).float()[None] / 255
        aten = (F.interpolate(x, size=(32, 32), mode="bilinear", antialias=True)[0].double() - ref).abs().max().item()
        print(f"ATen fp32 distance {aten:.3e}")
        record("resize side33 ATen-fp32", f"err {aten:.3e}")
        assert err < aten
    if name.startswith("outside"):
        assert torch.equal(got, torch.full_like(got, fill / 255))


def test_resize_500_to_224():
    img = IC.picture(500, 500, seed=500)
    out, st = launch([img], [(0, 0, 500)], S=224)
    ref, (tx, ty) = IC.yardstick(img, (0, 0, 500), 224)
    err, bound = (out[0].double() - ref).abs().max().item(), IC.resize_bound(tx, ty)
    x = torch.from_numpy(img).permute(2, 0, 1).float()[None] / 255
    aten = (F.interpolate(x, size=(224, 224), mode="bilinear", antialias=True)[0].double() - ref).abs().max().item()
    print(f"500 -> 224: err {err:.3e} bound {bound:.3e} taps {tx}; ATen fp32 {aten:.3e}")
    record("resize 500->224", f"err {err:.3e}  bound {bound:.3e}  taps {tx}  (ATen-fp32 {aten:.3e})")
    assert st.tolist() == [0] and err <= bound


def test_largest_image_sizes():
    """S = PD_IMG_MAX_SIZE and 1023: the largest pixel indices the kernels split into (row, column), in the resize's horizontal pass and
    epilogue and in the colour kernel; one band of output rows per workgroup."""
    up, e = IC.picture(40, 40, seed=40), dict(jitter=1, order=(1, 3, 0, 2), brightness=1.2, contrast=0.8, saturation=1.1, hue=-0.04)
    S = _lib.PD_IMG_MAX_SIZE
    out, st = launch([up], [(0, 0, 40)], S=S, colours=[e], seq=[0])
    bound, (ref,) = IC.own_error_bound([(up, (0, 0, 40), e)], S=S)
    err = (out[0].double() - ref).abs().max().item()
    print(f"40 -> {S} with colour: err {err:.3e} bound {bound:.3e}")
    record(f"colour 40->{S}", f"err {err:.3e}  bound {bound:.3e}")
    assert st.tolist() == [0] and err <= bound
    down = IC.picture(1100, 1100, seed=11)
    out, st = launch([down], [(0, 0, 1100)], S=1023)
    ref, (tx, ty) = IC.yardstick(down, (0, 0, 1100), 1023)
    err, bound = (out[0].double() - ref).abs().max().item(), IC.resize_bound(tx, ty)
    print(f"1100 -> 1023: err {err:.3e} bound {bound:.3e} taps {tx}")
    record("resize 1100->1023", f"err {err:.3e}  bound {bound:.3e}  taps {tx}")
    assert st.tolist() == [0] and err <= bound


@pytest.mark.parametrize("fill", [0, 255])
def test_one_launch_of_every_kind_is_bitwise_each_frame_alone_and_repeatable(fill):
    cases = IC.ALL_CASES if fill == 0 else IC.BORDER_CASES
    frames = [IC.case_picture(n, H, W) for n, H, W, _ in cases]
    pads = [3 if "odd" in n else (k % 2) for k, (n, _, _, _) in enumerate(cases)]
    a, st = launch(frames, [c[3] for c in cases], fill=fill, pads=pads)
    b, _ = launch(frames, [c[3] for c in cases], fill=fill, pads=pads)
    assert st.tolist() == [0] * len(cases) and torch.equal(a, b)
    for k, (n, H, W, box) in enumerate(cases):
        assert torch.equal(a[k], alone(n, H, W, box, fill)), n


# ---- colour ---------------------------------------------------------------------------------------------------------------------------
_colour_sources = IC.colour_sources


@pytest.fixture(scope="module")
def colour_bound():
    """4 x the largest distance, over the whole table, of an fp32 run of the yardstick from the fp64 yardstick"""
    return IC.colour_table_bound()


def test_all_orders_and_factor_sets_in_one_launch(colour_bound):
    bound, refs = colour_bound
    table = IC.colour_table()
    srcs = _colour_sources()
    frames = [img for img, _ in srcs for _ in table]
    boxes = [box for _, box in srcs for _ in table]
    seq = list(range(len(table))) * len(srcs)
    out, st = launch(frames, boxes, colours=table, seq=seq)
    assert st.tolist() == [0] * len(frames)
    errs = [(out[k].double() - refs[k]).abs().max().item() for k in range(len(frames))]
    k = int(np.argmax(errs))
    print(f"colour: worst err {max(errs):.3e} (order {table[k % len(table)]['order']}, factors {IC.FACTOR_SETS[k % 4]}), bound {bound:.3e}")
    record("colour 24 orders x 4 sets", f"err {max(errs):.3e}  bound {bound:.3e}  (4 x the fp32 yardstick's own {bound / 4:.3e})")
    assert max(errs) <= bound
    again, _ = launch(frames, boxes, colours=table, seq=seq)
    assert torch.equal(out, again)
    one, _ = launch([frames[k]], [boxes[k]], colours=[table[seq[k]]], seq=[0])      # the worst frame alone: the same bits
    assert torch.equal(one[0], out[k])


def test_contrast_mean_of_a_frame_with_one_bright_pixel(colour_bound):
    img = np.zeros((32, 32, 3), np.uint8)
    img[17, 5] = (255, 200, 90)
    e = dict(jitter=1, order=(1, 0, 2, 3), brightness=1.0, contrast=0.6, saturation=1.0, hue=0.0)
    out, st = launch([img], [(0, 0, 32)], colours=[e], seq=[0])
    ref, _ = IC.yardstick(img, (0, 0, 32), 32, colour=e)
    err = (out[0].double() - ref).abs().max().item()
    mean = (0.2989 * 255 + 0.587 * 200 + 0.114 * 90) / 255 / 1024
    print(f"one bright pixel: err {err:.3e}; background {out[0, 0, 0, 0].item():.6e} (0.4 mean = {0.4 * mean:.6e})")
    record("colour contrast one pixel", f"err {err:.3e}  bound {colour_bound[0]:.3e}")
    assert st.tolist() == [0] and err <= colour_bound[0] and abs(out[0, 0, 0, 0].item() - 0.4 * mean) <= 1e-9


def test_grayscale_erase_identity_and_two_sequences(colour_bound):
    bound, _ = colour_bound
    img_a, img_b = IC.picture(64, 64, seed=1), IC.picture(33, 33, seed=2)
    jit = dict(jitter=1, order=(3, 1, 0, 2), brightness=1.3, contrast=0.7, saturation=1.15, hue=-0.07)
    entries = [dict(jitter=0, grayscale=1), dict(jitter=0, erase=(0, 0, 5, 7)), dict(jitter=0, erase=(0, 0, 32, 32)),
               dict(jitter=0, erase=(3, 4, 0, 9)), dict(jitter=0), jit, dict(jit, grayscale=1, erase=(27, 25, 5, 7), order=(0, 2, 1, 3))]
    frames = [img_a] * len(entries) + [img_b, img_b, img_a]
    boxes = [(0, 0, 64)] * len(entries) + [(0, 0, 33), (0, 0, 33), (0, 0, 64)]
    seq = list(range(len(entries))) + [5, 6, -1]
    out, st = launch(frames, boxes, colours=entries, seq=seq)
    assert st.tolist() == [0] * len(frames)
    plain, _ = launch([img_a, img_b], [(0, 0, 64), (0, 0, 33)])
    for k in (3, 4, 9):                                    # erase_h == 0, nothing to do, no colour entry: the resize's bits
        assert torch.equal(out[k], plain[0]), k
    assert torch.equal(out[0][0], out[0][1]) and torch.equal(out[0][0], out[0][2])
    assert float(out[1][:, :5, :7].abs().max()) == 0.0 and torch.equal(out[1][:, 5:], plain[0][:, 5:]) and torch.equal(out[1][:, :, 7:], plain[0][:, :, 7:])
    assert float(out[2].abs().max()) == 0.0
    assert float(out[6][:, 27:, 25:].abs().max()) == 0.0
    worst = 0.0
    for k in range(len(frames)):
        ref, _ = IC.yardstick(frames[k], boxes[k], 32, colour=entries[seq[k]] if seq[k] >= 0 else None)
        worst = max(worst, (out[k].double() - ref).abs().max().item())
    print(f"grayscale / erase / two sequences: worst err {worst:.3e}, bound {bound:.3e}")
    record("colour gray/erase/2 seqs", f"err {worst:.3e}  bound {bound:.3e}")
    assert worst <= bound
    assert not torch.equal(out[5], out[7][:, :, :]) and not torch.equal(out[7], out[8])      # different draws, different frames


# ---- status and arguments -------------------------------------------------------------------------------------------------------------------
def test_every_device_side_status_zeroes_its_frame_and_spares_its_neighbours():
    img = IC.picture(40, 50, seed=4)
    good = dict(jitter=1, order=(0, 1, 2, 3), brightness=1.1, contrast=0.9, saturation=1.1, hue=0.02)
    entries = [good, dict(good, order=(0, 1, 1, 3)), dict(good, order=(0, 1, 2, 4)), dict(jitter=0, erase=(30, 0, 5, 4)),
               dict(jitter=0, erase=(0, 29, 1, 4)), dict(jitter=0, erase=(-1, 0, 2, 2)), dict(jitter=0, erase=(0, 0, 2, -2))]
    bad = [((0, 0, 0), 40, 50, 0, _lib.PD_IMG_BAD_SIDE), ((0, 0, -5), 40, 50, 0, _lib.PD_IMG_BAD_SIDE),
           ((0, 0, _lib.PD_IMG_MAX_SIDE + 1), 40, 50, 0, _lib.PD_IMG_BAD_SIDE), ((0, 0, 20), 0, 50, 0, _lib.PD_IMG_BAD_SIZE),
           ((0, 0, 20), 40, -1, 0, _lib.PD_IMG_BAD_SIZE), ((0, 0, 20), 40, 50, 7, _lib.PD_IMG_BAD_COLOUR),
           ((0, 0, 20), 40, 50, -2, _lib.PD_IMG_BAD_COLOUR), ((0, 0, 20), 40, 50, 1, _lib.PD_IMG_BAD_ORDER),
           ((0, 0, 20), 40, 50, 2, _lib.PD_IMG_BAD_ORDER), ((0, 0, 20), 40, 50, 3, _lib.PD_IMG_BAD_ERASE),
           ((0, 0, 20), 40, 50, 4, _lib.PD_IMG_BAD_ERASE), ((0, 0, 20), 40, 50, 5, _lib.PD_IMG_BAD_ERASE),
           ((0, 0, 20), 40, 50, 6, _lib.PD_IMG_BAD_ERASE)]
    ref_good, _ = launch([img], [(5, 3, 30)], colours=[good], seq=[0])
    frames, boxes, seq, want = [img], [(5, 3, 30)], [0], [0]
    for box, h, w, c, code in bad:
        frames += [None, img]
        boxes += [box + (h, w), (5, 3, 30)]
        seq += [c, 0]
        want += [code, 0]
    out, st, guards_ok = launch(frames, boxes, colours=entries, seq=seq, canary=True)
    assert guards_ok and st.tolist() == want
    for k, code in enumerate(want):
        if code:
            assert float(out[k].abs().max()) == 0.0 and not bool(torch.signbit(out[k]).any()), k
        else:
            assert torch.equal(out[k], ref_good[0]), k


def test_host_side_refusals_and_the_empty_call():
    lib = _lib.load()
    p = 0x1000                                                 # never dereferenced: every call below is refused on the host
    need = lib.pd_train_images_workspace_bytes(2, 32)

    def call(pixels=p, frames=p, n=2, colours=p, nc=1, S=32, fill=0, out=p, status=p, ws=p, wsb=need):
        return lib.pd_train_images(pixels, frames, n, colours, nc, S, fill, out, status, ws, wsb, None)

    for kw, word in ((dict(pixels=None), "pixels is NULL"), (dict(frames=None), "frames is NULL"), (dict(out=None), "out is NULL"),
                     (dict(status=None), "status_out is NULL"), (dict(ws=None), "workspace is NULL"), (dict(colours=None), "colours is NULL"),
                     (dict(n=-1), "n_frames = -1"), (dict(n=_lib.PD_IMG_MAX_FRAMES + 1, wsb=1 << 40), "n_frames = 65536"), (dict(nc=-1), "n_colours = -1"), (dict(S=0), "image_size = 0"),
                     (dict(S=_lib.PD_IMG_MAX_SIZE + 1), "image_size"), (dict(fill=-1), "fill = -1"), (dict(fill=256), "fill = 256"),
                     (dict(wsb=need - 1), "workspace"), (dict(ws=p + 4), "workspace")):
        assert call(**kw) == -1, kw
        assert "pd_train_images" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
    assert call(n=0, wsb=0) == 0 and call(n=0, colours=None, nc=0) == 0
    out, st, guards_ok = launch([], [], canary=True)
    assert guards_ok and out.numel() == 0
