"""Every token row of the image feature extractor against the fp64 network (a plain helper module, imported by the tests).

The ViT's product output is the CLS feature after the final LayerNorm, and with `make_vit`'s weights the attention is close to uniform
(mean largest probability 0.015 at 197 tokens): a fault in one non-CLS row reaches that output divided by roughly the token count.  A 1e-3
error confined to one edge row (a wrong tile edge, a wrong `min(.., T - 1)` clamp, a row that keeps 11 bits instead of 22) moves the CLS
feature by 5e-6 and passes its 2e-5 bound.  These helpers compare the residual stream itself (`VitEngine.tokens` / `vit_oracle.token_rows`:
all rows after the last block, before the final LayerNorm), row by row, each row against its own largest reference magnitude.

The bound rule (never the engine's exact mode: that is code under test):
    err <= max(K x e32, floor)   and   err < 1e-4
with e32 the CPU fp32 oracle's own distance from the fp64 oracle on the same inputs and weights, measured with the same helper.  K = 4: the
engine and the fp32 oracle are two fp32 evaluations of one function that differ in summation order (split-K over four waves, MFMA
accumulation, fused LayerNorm) and, on fp16 planes, in 22-bit operands; the denoiser's adversarial test allows 2 x between two fp32-grade
modes of one engine, a second factor 2 covers the CPU's different order.  A (family, depth) pair is only usable when K x e32 < 1e-4.
"""
import contextlib

import torch

from oracle import vit_oracle as VO

TILE = 32
K_E32 = 4.0
CONTRACT = 1e-4                 # the project's parity contract
CLS_FLOOR = 2e-6                # what test_vit_large_batch_gemm_paths_vs_oracle already holds the default mode to against fp64
# Largest worst-token-row e32 (fp32 oracle on one CPU thread against the fp64 oracle, no GPU involved) over the benign token-count sweep below (SWEEP, one image,
# depth 2, make_vit(seed=0), images(1, H, W, 100 + T)): 1.77e-6 (96 and 273 tokens); the other shapes 5.5e-7 .. 1.74e-6.
# tests/test_vit_checks_cpu.py recomputes three of the shapes and asserts that they do not exceed it.
E32_BENIGN_MAX = 1.8e-6
TOKEN_FLOOR = K_E32 * E32_BENIGN_MAX

# (H, W) -> tokens per image T = 1 + (H // 16)(W // 16): on and around the 32-key tile, the 8-key chunk and the 256-key change of the PV loop,
# the streamed threshold (1 024 rows) and VT_MAX = 1 056
SWEEP = (((16, 16), 2), ((16, 112), 8), ((32, 64), 9), ((64, 64), 17), ((16, 496), 32), ((23, 503), 32), ((64, 128), 33), ((112, 144), 64),
         ((128, 128), 65), ((80, 304), 96), ((128, 192), 97), ((128, 256), 129), ((224, 224), 197), ((240, 272), 256), ((256, 256), 257),
         ((263, 279), 273), ((256, 512), 513), ((512, 512), 1025), ((80, 3376), 1056))


@contextlib.contextmanager
def one_thread():
    """the fp32 oracle, whose rounding IS the yardstick, runs on one CPU thread: its sums do not depend on how many the host has"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def tokens_of(H, W):
    return 1 + (H // 16) * (W // 16)


def token_row_errs(got, ref64, skip_channels=()):
    """got, ref64 [n, T, C] -> dict(worst, where=(image, token), tile_pos=(token % 32, flat row % 32), per_token_pos[32], per_row_pos[32],
    rows[n, T]): per row max_c |got - ref| / max_c |ref| in fp64, the worst row and the worst row per position inside a 32-row tile -- of
    the image's own token index (the attention's query blocks) and of the flat row index image * T + token (the GEMMs' row tiles) -- so
    that a failure names the edge.  `skip_channels` are left out of both maxima: a massive channel dominates the plain row norm and hides
    the rest."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref64).detach().cpu().double()
    assert got.shape == ref.shape and got.dim() == 3, (got.shape, ref.shape)
    n, T, Cn = ref.shape
    keep = torch.ones(Cn, dtype=torch.bool)
    keep[list(skip_channels)] = False
    d = (got - ref).abs()[..., keep].amax(dim=-1)
    s = ref.abs()[..., keep].amax(dim=-1).clamp_min(1e-30)
    rows = d / s
    rows = torch.where(torch.isnan(rows), torch.full_like(rows, float("inf")), rows)          # a NaN row is a failing row, not a skipped one
    flat = rows.reshape(-1)
    w = int(flat.argmax())
    tok = torch.arange(T).repeat(n)
    row = torch.arange(n * T)
    per_tok = torch.zeros(TILE, dtype=torch.float64).scatter_reduce(0, tok % TILE, flat, "amax", include_self=True)
    per_row = torch.zeros(TILE, dtype=torch.float64).scatter_reduce(0, row % TILE, flat, "amax", include_self=True)
    return {"worst": flat[w].item(), "where": (w // T, w % T), "tile_pos": ((w % T) % TILE, w % TILE), "per_token_pos": per_tok,
            "per_row_pos": per_row, "rows": rows}


def describe(e):
    """one line: worst row error, its (image, token) and position inside the 32-row tiles"""
    (im, tk), (tp, rp) = e["where"], e["tile_pos"]
    return f"{e['worst']:.2e} at (image {im}, token {tk}; tile pos {tp} of its query block, {rp} of its row tile)"


def bound(e32, floor):
    """max(K x e32, floor); the caller also asserts the contract (err < 1e-4) and the usability condition K x e32 < 1e-4"""
    return max(K_E32 * e32, floor)


def usable(e32):
    return K_E32 * e32 < CONTRACT


def cls_feature(net, tokens):
    """final LayerNorm of the CLS rows of `tokens` [n, T, C] (what DinoViT.forward returns)"""
    with torch.no_grad():
        return net.norm(tokens.to(net.cls_token.dtype))[:, 0]


def images(n, H, W, seed):
    return torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(seed))


@torch.no_grad()
def attention_stats(net64, x):
    """(mean over blocks, heads and query rows of the largest attention probability, largest logit range of a row) of the fp64 network"""
    dt = net64.cls_token.dtype
    mean = torch.tensor(VO.RESNET_MEAN, dtype=dt).view(1, 3, 1, 1)
    std = torch.tensor(VO.RESNET_STD, dtype=dt).view(1, 3, 1, 1)
    img = (x.to(dt) - mean) / std
    B, _, w, h = img.shape
    t = net64.patch_embed(img)
    t = torch.cat((net64.cls_token.expand(B, -1, -1), t), dim=1)
    t = t + net64.interpolate_pos_encoding(t, w, h)
    pmax, span = [], 0.0
    for blk in net64.blocks:
        a = blk.attn
        Bn, N, Cn = t.shape
        qkv = a.qkv(blk.norm1(t)).reshape(Bn, N, 3, a.num_heads, Cn // a.num_heads).permute(2, 0, 3, 1, 4)
        logits = (qkv[0] @ qkv[1].transpose(-2, -1)) * a.scale
        pmax.append(logits.softmax(dim=-1).amax(dim=-1).mean().item())
        span = max(span, (logits.amax(dim=-1) - logits.amin(dim=-1)).max().item())
        t = blk(t)
    return sum(pmax) / len(pmax), span


# ---- weight families: (seed, depth, dtype) -> DinoViT truncated to `depth` blocks -------------------------------------------------------
# Every change is made to the fp32 parameters and the network cast afterwards, so the fp32 and the fp64 network of one (family, seed, depth)
# hold the same values (as make_vit's do) and the engine, which reads fp32, runs the same network.
MASSIVE = 137                    # the channel the massive-activation families load


def _base(seed, depth):
    net = VO.make_vit(seed)
    assert 1 <= depth <= len(net.blocks)
    net.blocks = net.blocks[:depth]
    return net


def _signs(shape, g):
    return torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def benign(seed, depth, dtype):
    return _base(seed, depth).to(dtype).eval()


def deep(seed, depth, dtype):
    """make_vit's family beyond 12 blocks (VDEPTH_MAX = 16): blocks 12 .. depth - 1 are those of make_vit(seed + 1)"""
    net = VO.make_vit(seed)
    if depth > len(net.blocks):
        net.blocks.extend(VO.make_vit(seed + 1).blocks[:depth - len(net.blocks)])
    net.blocks = net.blocks[:depth]
    return net.to(dtype).eval()


def grid15(seed, depth, dtype):
    """a network trained on a 15 x 15 position grid (DinoViT(img_size=240)): make_vit's parameters, its own 226-row position table"""
    src = _base(seed, depth)
    net = VO.DinoViT(img_size=240, depth=depth)
    with torch.no_grad():
        own = net.state_dict()
        for k, v in src.state_dict().items():
            if k != "pos_embed":
                own[k].copy_(v)
    return net.to(dtype).eval()


def grid1(seed, depth, dtype):
    """a network trained on a 1 x 1 position grid (DinoViT(img_size=16)): make_vit's parameters, its own 2-row position table -- every
    other grid is a resampling of ONE cell, whose four taps per axis all clamp to it"""
    src = _base(seed, depth)
    net = VO.DinoViT(img_size=16, depth=depth)
    with torch.no_grad():
        own = net.state_dict()
        for k, v in src.state_dict().items():
            if k != "pos_embed":
                own[k].copy_(v)
    return net.to(dtype).eval()


def _peaked(seed, depth, dtype, factor):
    net = _base(seed, depth)
    with torch.no_grad():
        for blk in net.blocks:
            d = blk.attn.qkv.weight.shape[1]
            blk.attn.qkv.weight[:2 * d] *= factor          # q and k rows: logits x factor^2
            blk.attn.qkv.bias[:2 * d] *= factor
    return net.to(dtype).eval()


def peaked_attention_x3(seed, depth, dtype):
    """trained-like peaked attention: mean largest probability 0.54 - 0.57, logit range about 40 (depth 2)"""
    return _peaked(seed, depth, dtype, 3.0)


def peaked_attention_x6(seed, depth, dtype):
    """mean largest probability 0.89, logit range about 160: expf(row - max) underflows for most keys"""
    return _peaked(seed, depth, dtype, 6.0)


def massive_channel(seed, depth, dtype):
    """one residual channel at about 300 from the first MLP on: LayerNorm rows close to +- sqrt(384) e_137"""
    net = _base(seed, depth)
    with torch.no_grad():
        net.blocks[0].mlp.fc2.bias[MASSIVE] = 300.0
    return net.to(dtype).eval()


def outlier_weight_per_row(seed, depth, dtype):
    """one entry of +- 2.0 per row in the four Linear weights of every block: max|w| pushes the bulk 2^-6 down the weight scale"""
    net = _base(seed, depth)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for blk in net.blocks:
            for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
                w = lin.weight
                col = torch.randint(0, w.shape[1], (w.shape[0],), generator=g)
                w[torch.arange(w.shape[0]), col] = 2.0 * _signs((w.shape[0],), g)
    return net.to(dtype).eval()


def bias_30x(seed, depth, dtype):
    """every second q / k / v and FC1 bias at +- 30: loose `ctx` / `hid` bounds, the values low in their range"""
    net = _base(seed, depth)
    g = torch.Generator().manual_seed(2000 + seed)
    with torch.no_grad():
        for blk in net.blocks:
            for b in (blk.attn.qkv.bias, blk.mlp.fc1.bias):
                b[::2] = 30.0 * _signs(b[::2].shape, g)
    return net.to(dtype).eval()


def _gamma(seed, depth, dtype, sigma):
    net = _base(seed, depth)
    g = torch.Generator().manual_seed(3000 + seed)
    with torch.no_grad():
        for blk in net.blocks:
            for ln in (blk.norm1, blk.norm2):
                ln.weight.copy_(torch.exp(sigma * torch.randn(ln.weight.shape, generator=g)))
    return net.to(dtype).eval()


def wide_gamma(seed, depth, dtype):
    """LayerNorm gains exp(1.5 N(0, 1)): about 0.01 .. 90, folded into the weight planes.  NOT in FAMILIES: the reference's own fp32 is
    chaotic under it (fp64 mean largest attention probability 0.91, logit range 417 in block 0).  e32 of the worst token row, 6 images of
    224 x 224, seed 0: 3.4e-5 at depth 1 and 5.6e-5 at depth 2, so 4 x e32 >= 1e-4 at every depth and the bound rule has no room for an
    engine (tests/test_vit_checks_cpu.py asserts this at depth 2).  `wide_gamma_1p0` is the widest spread that passes the condition."""
    return _gamma(seed, depth, dtype, 1.5)


def wide_gamma_1p0(seed, depth, dtype):
    """LayerNorm gains exp(N(0, 1)): about 0.04 .. 25 folded into the weight planes; e32 3.6e-6 at depth 2, 7.3e-6 at depth 4"""
    return _gamma(seed, depth, dtype, 1.0)


def wide_gamma_0p75(seed, depth, dtype):
    """the narrower spread exp(0.75 N(0, 1)) for depth 4"""
    return _gamma(seed, depth, dtype, 0.75)


def tiny_gelu_outputs(seed, depth, dtype):
    """The ViT counterpart of the denoiser's `tiny_relu_outputs`.  Channel 137 of every token is 1e6 from the embedding on (patch bias and CLS
    token), so LayerNorm rows are sqrt(384) e_137 plus (x_k - mean) / std with std ~ 5e4.  norm2 is the identity affine, FC1 rows are
    +- 0.02 of alternating sign over 382 channels (137 and its pair 136 are zero: 191 of each sign, the common -mean / std term cancels
    exactly) and the FC1 bias is 1e-7: pre-activations ~ 1e-6 .. 1e-5 where the `hid` bound sqrt(384) ||w||_2 + |b| is 7.7, so GELU
    outputs sit near 2^-20 of the bound (their fp16 lo halves subnormal or lost)."""
    net = _base(seed, depth)
    g = torch.Generator().manual_seed(4000 + seed)
    with torch.no_grad():
        net.patch_embed.proj.bias[MASSIVE] = 1.0e6
        net.cls_token[..., MASSIVE] = 1.0e6
        for blk in net.blocks:
            w = blk.mlp.fc1.weight
            alt = torch.where(torch.arange(w.shape[1]) % 2 == 0, 0.02, -0.02)
            w.copy_(alt[None, :] * _signs((w.shape[0], 1), g))
            w[:, MASSIVE] = 0.0
            w[:, MASSIVE - 1] = 0.0
            blk.mlp.fc1.bias.fill_(1e-7)
            blk.norm2.weight.fill_(1.0)
            blk.norm2.bias.zero_()
    return net.to(dtype).eval()


# family -> (builder, depths it runs at, channels skipped in the row norms: () = none)
FAMILIES = {
    "peaked_attention_x3": (peaked_attention_x3, (2, 4), ()),
    "peaked_attention_x6": (peaked_attention_x6, (2,), ()),
    "massive_channel": (massive_channel, (2, 4), (MASSIVE,)),
    "outlier_weight_per_row": (outlier_weight_per_row, (2, 4), ()),
    "bias_30x": (bias_30x, (2, 4), ()),
    "wide_gamma_1p0": (wide_gamma_1p0, (2, 4), ()),
    "wide_gamma_0p75": (wide_gamma_0p75, (4,), ()),
    "tiny_gelu_outputs": (tiny_gelu_outputs, (2, 4), (MASSIVE,)),
}
PEAKEDNESS = {"peaked_attention_x3": 0.4, "peaked_attention_x6": 0.8}      # least fp64 mean largest attention probability the family relies on


def oracle_pair(family, seed, depth):
    """(fp32 network, fp64 network) of one family with identical parameter values"""
    return family(seed, depth, torch.float32), family(seed, depth, torch.float64)


@torch.no_grad()
def oracle_errs(net32, net64, x, scale_factor=1, skip_channels=()):
    """(fp64 token rows, e32 dict of the token rows, e32 of the CLS feature): the yardstick of the bound rule"""
    from conftest import rel_err
    ref64 = VO.token_rows(net64, x.double(), scale_factor)
    with one_thread():
        ref32 = VO.token_rows(net32, x, scale_factor)
    return ref64, token_row_errs(ref32, ref64, skip_channels), rel_err(cls_feature(net32, ref32), cls_feature(net64, ref64))

