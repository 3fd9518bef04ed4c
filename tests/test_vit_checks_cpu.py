"""CPU: the token-row checks of tests/vit_checks.py against the oracle itself -- the record of why the token view exists.

Faults of the kind a kernel edge produces are injected into the fp64 oracle (a patched forward here, not in oracle/): the worst token row
moves far beyond the bound the GPU tests use, while the first fault moves the CLS feature -- all the earlier ViT tests compared -- by less
than their 2e-5 bound.  The weight families are checked for what the GPU tests rely on: the bound rule's condition 4 x e32 < 1e-4, the
peakedness of the peaked families, finite and non-constant rows of `tiny_gelu_outputs` with GELU outputs near 2^-20 of the `hid` bound."""
import pytest
import torch
import torch.nn.functional as F

import vit_checks as V
from conftest import rel_err
from oracle import vit_oracle as VO

FAULTS = ("last_query_row_x1.001", "rows_160_on_x1.001", "fc2_last_row_tile_bias_99_percent", "tanh_gelu", "last_key_masked")


@torch.no_grad()
def _faulty_token_rows(net, x, fault):
    """vit_oracle.token_rows at scale 1 with `fault` in every block (None: the oracle itself, bit for bit)"""
    dt = net.cls_token.dtype
    img = (x.to(dt) - torch.tensor(VO.RESNET_MEAN, dtype=dt).view(1, 3, 1, 1)) / torch.tensor(VO.RESNET_STD, dtype=dt).view(1, 3, 1, 1)
    B, _, w, h = img.shape
    t = net.patch_embed(img)
    t = torch.cat((net.cls_token.expand(B, -1, -1), t), dim=1)
    t = t + net.interpolate_pos_encoding(t, w, h)
    for blk in net.blocks:
        a = blk.attn
        _, N, Cn = t.shape
        qkv = a.qkv(blk.norm1(t)).reshape(B, N, 3, a.num_heads, Cn // a.num_heads).permute(2, 0, 3, 1, 4)
        logits = (qkv[0] @ qkv[1].transpose(-2, -1)) * a.scale
        if fault == "last_key_masked":
            logits[..., -1] = float("-inf")
        o = (logits.softmax(dim=-1) @ qkv[2]).transpose(1, 2).reshape(B, N, Cn)
        if fault == "last_query_row_x1.001":              # the last row of the ragged 32-row query block (token 196 of 197)
            o[:, -1] *= 1.001
        if fault == "rows_160_on_x1.001":
            o[:, 160:] *= 1.001
        t = t + a.proj(o)
        u = blk.mlp.fc1(blk.norm2(t))
        u = F.gelu(u, approximate="tanh") if fault == "tanh_gelu" else F.gelu(u)
        y = blk.mlp.fc2(u)
        if fault == "fc2_last_row_tile_bias_99_percent":  # tokens 192 .. 196: the last 32-row tile of an image
            y[:, 192:] -= 0.01 * blk.mlp.fc2.bias
        t = t + y
    return t


@pytest.fixture(scope="module")
def full_depth():
    net32, net64 = V.oracle_pair(V.benign, 0, 12)
    x = V.images(3, 224, 224, 1)
    ref64, e32, c32 = V.oracle_errs(net32, net64, x)
    assert torch.equal(_faulty_token_rows(net64, x, None), ref64)
    return net64, x, ref64, e32, c32


def test_fp32_oracle_passes_its_own_bound(full_depth):
    _, _, _, e32, c32 = full_depth
    print("12 blocks, 3 x 224 x 224, fp32 oracle vs fp64: worst token row", V.describe(e32), f"CLS {c32:.2e}")
    assert V.usable(e32["worst"]) and e32["worst"] <= V.bound(e32["worst"], V.TOKEN_FLOOR) and c32 <= V.CLS_FLOOR


@pytest.mark.parametrize("fault", FAULTS)
def test_token_row_check_sees_each_injected_fault(full_depth, fault):
    net64, x, ref64, e32, _ = full_depth
    bad = _faulty_token_rows(net64, x, fault)
    e = V.token_row_errs(bad.float(), ref64)                       # stored in fp32, as an engine's result would be
    cls = rel_err(V.cls_feature(net64, bad), V.cls_feature(net64, ref64))
    bnd = V.bound(e32["worst"], V.TOKEN_FLOOR)
    print(f"{fault}: CLS feature moves {cls:.2e}, worst token row {V.describe(e)}; bound {bnd:.2e}")
    assert e["worst"] > 10 * bnd, (fault, e["worst"], bnd)        # the token view sees it, with room
    if fault == "last_query_row_x1.001":
        assert cls < 2e-5, cls                                     # ... the CLS-only bound of the earlier tests does not
        assert e["where"][1] == 196 and e["tile_pos"][0] == 4     # and the helper names the edge
    if fault == "fc2_last_row_tile_bias_99_percent":
        assert e["where"][1] >= 192
        # tile positions 0 .. 4 (of the last query block) carry it; attention spreads a 20 x smaller share to every other row
        assert e["per_token_pos"][:5].min() > 10 * e["per_token_pos"][5:].max()


def test_helper_skips_channels_and_counts_nan_rows():
    ref = torch.randn(2, 40, 384, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    ref[..., V.MASSIVE] = 300.0
    got = ref.clone()
    got[1, 33, 5] += 1e-3
    plain, skipped = V.token_row_errs(got, ref), V.token_row_errs(got, ref, (V.MASSIVE,))
    assert plain["where"] == skipped["where"] == (1, 33) and plain["tile_pos"] == (1, (40 + 33) % 32)
    assert plain["worst"] < 4e-6 < 1e-4 < skipped["worst"]          # the massive channel hides a 1e-3 error in the plain row norm
    got[0, 7, V.MASSIVE] = 301.0                                    # an error IN the skipped channel is only seen without the skip
    assert V.token_row_errs(got, ref, (V.MASSIVE,))["where"] == (1, 33) and V.token_row_errs(got, ref)["where"] == (0, 7)
    got[0, 2, 0] = float("nan")
    assert V.token_row_errs(got, ref)["worst"] == float("inf") and V.token_row_errs(got, ref)["where"] == (0, 2)


@pytest.mark.parametrize("hw", [(64, 64), (224, 224), (512, 512)])
def test_benign_e32_constant_is_not_exceeded(hw):
    """TOKEN_FLOOR = 4 x E32_BENIGN_MAX comes from a CPU run of the whole sweep; three of its shapes recomputed"""
    assert hw in dict(V.SWEEP) and all(V.tokens_of(*s) == T for s, T in V.SWEEP)
    net32, net64 = V.oracle_pair(V.benign, 0, 2)
    _, e32, c32 = V.oracle_errs(net32, net64, V.images(1, *hw, 100 + V.tokens_of(*hw)))
    print(hw, "fp32 oracle vs fp64:", V.describe(e32), f"CLS {c32:.2e}")
    assert e32["worst"] <= V.E32_BENIGN_MAX and c32 <= V.CLS_FLOOR


@pytest.mark.parametrize("name,depth", [(n, d) for n, (_, ds, _) in sorted(V.FAMILIES.items()) for d in ds])
def test_family_is_usable_and_is_what_it_claims(name, depth):
    fam, _, skip = V.FAMILIES[name]
    net32, net64 = V.oracle_pair(fam, 0, depth)
    for (k, a), b in zip(net32.state_dict().items(), net64.state_dict().values()):
        assert torch.equal(a.double(), b), k                        # one network in two precisions
    x = V.images(2, 224, 224, 31)
    ref64, e32, c32 = V.oracle_errs(net32, net64, x, 1, skip)
    print(f"{name} depth {depth}: e32 worst token row {V.describe(e32)}, CLS {c32:.2e}")
    assert torch.isfinite(ref64).all()
    assert V.usable(e32["worst"]) and V.usable(c32), (name, depth, e32["worst"], c32)
    if name in V.PEAKEDNESS:
        pmax, span = V.attention_stats(net64, x)
        print(f"  mean largest attention probability {pmax:.3f}, largest logit range {span:.0f}")
        assert pmax >= V.PEAKEDNESS[name]
    if name == "massive_channel":
        assert ref64[..., V.MASSIVE].abs().min() > 250
    if name == "tiny_gelu_outputs":
        other = [c for c in range(384) if c != V.MASSIVE]
        assert ref64[:, :, other].std(dim=1).max() > 0.1            # rows differ from token to token
        hid = []
        hooks = [blk.mlp.fc1.register_forward_hook(lambda m, i, o: hid.append(F.gelu(o))) for blk in net64.blocks]
        VO.token_rows(net64, x.double())
        for hk in hooks:
            hk.remove()
        for blk, g in zip(net64.blocks, hid):
            hid_bound = 384 ** 0.5 * blk.mlp.fc1.weight.norm(dim=1).max() + blk.mlp.fc1.bias.abs().max()
            assert 2.0 ** -24 < g.abs().median() / hid_bound < 2.0 ** -19, (g.abs().median() / hid_bound).log2()


def test_wide_gamma_1p5_leaves_the_bound_rule_no_room():
    """exp(1.5 N) gains make the reference's own fp32 chaotic already at depth 2 (4 x e32 >= 1e-4): the reason FAMILIES carries the spread
    exp(1.0 N) instead.  Should this start to fail, the family has become usable and belongs in FAMILIES."""
    net32, net64 = V.oracle_pair(V.wide_gamma, 0, 2)
    _, e32, _ = V.oracle_errs(net32, net64, V.images(6, 224, 224, 31))
    print("wide_gamma (sigma 1.5) depth 2: e32", V.describe(e32))
    assert not V.usable(e32["worst"])
