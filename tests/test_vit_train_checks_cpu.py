"""No GPU: the yardstick of the backbone trainer's tests (tests/vit_train_checks.py) is the oracle's function, and its block split is
what the GPU test needs."""
import pytest
import torch

from oracle import vit_oracle as VO
import vit_train_checks as VC

CASE = VC.Case(2, 48, 32, (1, 1 / 2), 2)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_forward_is_the_oracles_bit_for_bit(dtype):
    net = VC.make_net(CASE.depth).to(dtype)
    images, _ = VC.inputs(CASE)
    with torch.no_grad():
        z = VC.multiscale(net, images.to(dtype), CASE.scales)
    assert torch.equal(z, VO.multiscale_features(net, images.to(dtype), CASE.scales))
    assert VC.multiscale(net, images.to(dtype), CASE.scales).requires_grad


def test_reference_gradients_cover_every_parameter_and_the_k_bias_is_rounding_only():
    net = VC.make_net(CASE.depth)
    images, g_z = VC.inputs(CASE)
    z64, g64 = VC.reference(net, images, g_z, CASE.scales, torch.float64)
    z32, g32 = VC.reference(net, images, g_z, CASE.scales, torch.float32)
    assert sorted(g64) == sorted(n for n, _ in net.named_parameters()) and z64.dtype == torch.float64 and z32.dtype == torch.float32
    assert all(p.grad is None for p in net.parameters())                      # the helper differentiates a copy
    print(f"z own distance {VC.grad_dist(z32, z64):.3e}")
    assert VC.grad_dist(z32, z64) < 1e-5
    for name in g64:
        assert g64[name].abs().max() > 0 and torch.isfinite(g64[name]).all(), name
        assert not VC.misses(name, g32[name], g32[name], g64[name]), name      # own against 4 x own: the rule is self-consistent
        for blk, e, own, zero in VC.block_dists(name, g32[name], g32[name], g64[name]):
            if VC.is_k_bias(name, blk):                                         # mathematically zero: float64 holds its own rounding only
                b = VC.grad_blocks(name, g64[name])
                ratio = (b["k"].abs().max() / b["v"].abs().max()).item()
                print(f"{name}[k]: float64 max is {ratio:.1e} of the v rows' (fp32 distance from it {own:.1e})")
                assert ratio < 1e-12
    blocks = VC.grad_blocks("pos_embed", g64["pos_embed"])
    assert blocks["cls"].shape == (1, 384) and blocks["patch"].shape == (196, 384)
    print(f"pos_embed: CLS row max {blocks['cls'].abs().max():.3e}, patch rows max {blocks['patch'].abs().max():.3e}")
    assert blocks["cls"].abs().max() > blocks["patch"].abs().max()


def test_bound_has_the_four_ulp_floor():
    assert VC.bound(0.0) == 8 * 2.0 ** -24 and VC.bound(1e-6) == 4e-6 and VC.bound(1e-6, 16.0) == 1.6e-5
