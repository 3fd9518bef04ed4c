"""No GPU: the trainer's dropout (pd_train_forward_dropout, include/pd_engine_train.h) as far as it can be pinned without a device --
the generator against its published known answers, the threshold, the placement of the four sites against torch's own
nn.TransformerEncoderLayer with injected masks, the statistics of every mask the GPU suite uses, the C-ABI entry and the drop-in's rules."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from denoiser_cfgs import Cfg, build_dropin
import train_checks as TC
import train_dropout_checks as D
from posediffusion_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONDEFAULT = Cfg(96, 4, 200, 2, 50, 40, True, False)


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32_10 (counter; key -> output)."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(v):08x}" for v in D.philox4x32_10(ctr, key)) == want
    # vectorised over a counter word = one call per element
    many = D.philox4x32_10((np.arange(5), 7, 2, 1), (3, 4))
    for i in range(5):
        assert [int(w[i]) for w in many] == [int(w) for w in D.philox4x32_10((i, 7, 2, 1), (3, 4))]


def test_threshold_and_scale():
    below_one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert D.threshold(0.0) == 0
    assert D.threshold(0.1) == 429496736                      # float32(0.1) = 13421773 x 2^-27, times 2^32
    assert D.threshold(0.5) == 2 ** 31
    assert D.threshold(below_one) == 2 ** 32 - 256            # 1 - 2^-24: still a uint32
    assert D.scale_of(0.5) == 2.0 and D.scale_of(0.0) == 1.0 and D.scale_of(0.1) == float(np.float32(1) / np.float32(0.9))
    assert D.keep_mask(8, 8, 0, 0, 1, 0, 0.0).all()           # thr 0 keeps everything


def test_keep_mask_uses_row_groups_of_four_and_the_words_in_order():
    m = D.keep_mask(9, 6, 3, 2, (5 << 32) | 9, 4, 0.5)
    for r in range(9):
        for c in range(6):
            w = D.philox4x32_10((r >> 2, c, 4 * 3 + 2, 4), (9, 5))[r & 3]
            assert bool(m[r, c]) == (int(w) >= 2 ** 31), (r, c)


def _small_inputs(B, N, zdim, seed=0):
    g = torch.Generator().manual_seed(4200 + 100 * B + N + seed)
    return {"x_start": torch.randn(B, N, 9, generator=g), "noise": torch.randn(B, N, 9, generator=g),
            "z": torch.randn(B, N, zdim, generator=g), "t": torch.linspace(0, 99, B).round().long()}


def test_without_sites_the_helper_is_train_checks_exactly():
    den = build_dropin(NONDEFAULT, seed=31)
    sd = {k: v.detach().clone() for k, v in den.state_dict().items()}
    net, inp = TC.Net.of_cfg(NONDEFAULT), _small_inputs(3, 7, NONDEFAULT.z)
    ref = TC.loss_and_grads(sd, net, inp, "pred_noise", "l1")
    for p, sites in ((0.3, 0), (0.0, D.ALL)):
        got = D.loss_and_grads_dropout(sd, net, inp, "pred_noise", "l1", p, sites, 5, 0)
        assert torch.equal(got["loss"], ref["loss"]) and torch.equal(got["model_out"], ref["model_out"])
        for n, g in ref["grads"].items():
            assert torch.equal(got["grads"][n], g), n
    drop = D.loss_and_grads_dropout(sd, net, inp, "pred_noise", "l1", 0.3, D.ALL, 5, 0)
    assert not torch.equal(drop["model_out"], ref["model_out"])


class _Masked(torch.nn.Module):
    def __init__(self, factor):
        super().__init__()
        self.factor = factor

    def forward(self, x):
        return x * self.factor.reshape(x.shape)


def test_residual_and_ff_sites_are_torchs_dropout1_dropout_dropout2():
    """A real nn.TransformerEncoderLayer(norm_first=True) in .train() whose three Dropout modules apply keep_mask x scale."""
    d, nhead, ff, B, N, l, p, seed, step = 32, 4, 72, 3, 5, 1, 0.3, 77, 2
    torch.manual_seed(3)
    layer = torch.nn.TransformerEncoderLayer(d, nhead, ff, dropout=p, batch_first=True, norm_first=True).double().train()
    layer.self_attn.dropout = 0.0
    f = lambda site, cols: torch.from_numpy(D.keep_mask(B * N, cols, l, site, seed, step, p)).double() * D.scale_of(p)      # noqa: E731
    layer.dropout1, layer.dropout, layer.dropout2 = _Masked(f(1, d)), _Masked(f(2, ff)), _Masked(f(3, d))
    x = torch.randn(B, N, d, dtype=torch.float64)
    want = layer(x)
    sd = {k: v.detach() for k, v in layer.state_dict().items()}
    got = D.encoder_layer(sd, "", x, nhead, l, D.RESID1 | D.FF | D.RESID2, (p, seed, step))
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    for sites in (D.RESID1, D.FF, D.RESID2, 0):                # each site matters, and none is the eval function
        other = D.encoder_layer(sd, "", x, nhead, l, sites, (p, seed, step))
        assert (other - want).abs().max().item() > 1e-3 * want.abs().max().item(), sites


def test_attention_site_is_torchs_dropout_on_the_probabilities(monkeypatch):
    """``self_attn(x, x, x, need_weights=True)`` takes torch's explicit softmax -> dropout -> bmm path, whose dropout is
    ``torch.nn.functional.dropout`` on the [B nhead, N, N] probabilities: with that function replaced by keep_mask x scale the module's
    output is the helper's attention (the installed torch routes through it: the test asserts that the replacement was called)."""
    d, nhead, B, N, l, p, seed, step = 32, 4, 3, 5, 2, 0.4, 91, 0
    torch.manual_seed(4)
    mha = torch.nn.MultiheadAttention(d, nhead, dropout=p, batch_first=True).double().train()
    factor = torch.from_numpy(D.keep_mask(B * nhead * N, N, l, 0, seed, step, p)).double() * D.scale_of(p)
    calls = []

    def fake_dropout(inp, p=0.5, training=True, inplace=False):
        calls.append((tuple(inp.shape), p, training))
        return inp * factor.reshape(inp.shape)

    monkeypatch.setattr(torch.nn.functional, "dropout", fake_dropout)
    x = torch.randn(B, N, d, dtype=torch.float64)
    want, weights = mha(x, x, x, need_weights=True)
    assert calls == [((B * nhead, N, N), p, True)], calls
    sd = {"self_attn." + k: v.detach() for k, v in mha.state_dict().items()}
    got = D.attention(sd, "", x, nhead, l, D.ATTN, (p, seed, step))
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert (D.attention(sd, "", x, nhead, l, 0, (p, seed, step)) - want).abs().max().item() > 1e-3 * want.abs().max().item()


def _case_masks(case):
    _, cfg, B, N, p, sites, seed, step, _, _ = case
    d, nhead, ff, layers = D.CONFIGS[cfg]
    for l in range(layers):
        for s, (rows, cols) in enumerate(D.site_shapes(B, N, nhead, d, ff)):
            if sites & (1 << s):
                yield l, s, D.keep_mask(rows, cols, l, s, seed, step, p)


@pytest.mark.parametrize("case", D.GPU_CASES, ids=[c[0] for c in D.GPU_CASES])
def test_keep_rate_of_every_mask_the_gpu_suite_uses(case):
    p = float(np.float32(case[4]))
    seen = []
    for l, s, m in _case_masks(case):
        n = m.size
        rate = m.mean()
        assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (l, s, rate, n)
        for l2, s2, m2 in seen:
            if m2.shape == m.shape and m.size >= 64:
                assert not np.array_equal(m, m2), ((l, s), (l2, s2))
        seen.append((l, s, m))


def test_masks_differ_by_layer_site_seed_and_step():
    base = D.keep_mask(15, 512, 0, 1, 11, 0, 0.1)
    assert np.array_equal(base, D.keep_mask(15, 512, 0, 1, 11, 0, 0.1))
    for other in (D.keep_mask(15, 512, 1, 1, 11, 0, 0.1), D.keep_mask(15, 512, 0, 3, 11, 0, 0.1), D.keep_mask(15, 512, 0, 1, 12, 0, 0.1),
                  D.keep_mask(15, 512, 0, 1, 11 + (1 << 32), 0, 0.1), D.keep_mask(15, 512, 0, 1, 11, 1, 0.1)):
        assert not np.array_equal(base, other)
        assert 0.7 < (base == other).mean() < 0.9             # independent masks at p = 0.1 agree on 0.82 of the elements
    # a prefix of a larger mask: the mapping depends on (row, column) alone, never on the extent
    assert np.array_equal(base, D.keep_mask(64, 1024, 0, 1, 11, 0, 0.1)[:15, :512])


def test_symbol_is_exported_bound_and_refuses_bad_arguments():
    assert "pd_train_forward_dropout" in _lib.TRAIN_SIGNATURES
    with open(os.path.join(ROOT, "include", "pd_engine_train.h")) as fh:
        hdr = fh.read()
    for name, val in (("PD_DROP_ATTN", 1), ("PD_DROP_RESID1", 2), ("PD_DROP_FF", 4), ("PD_DROP_RESID2", 8), ("PD_DROP_ALL", 15)):
        assert f"#define {name} {val}u" in hdr and getattr(_lib, name) == val
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    fn = lib.pd_train_forward_dropout
    assert fn.argtypes == _lib.TRAIN_SIGNATURES["pd_train_forward_dropout"][1]
    tail = (None, None, None, None, None)
    assert fn(None, None, None, None, None, None, 1, 1, 1, 0.1, 15, 0, 0, *tail) == -1
    assert "pd_train_forward_dropout: NULL trainer" in _lib.last_error()
    # argument checks come before anything is read or launched: a handle that is never dereferenced is enough
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert fn(fake, None, None, None, None, None, 1, 1, 1, p, 15, 0, 0, *tail) == -1
        assert "argument p=" in _lib.last_error() and "[0, 1)" in _lib.last_error()
    assert fn(fake, None, None, None, None, None, 1, 1, 1, 0.1, 16, 0, 0, *tail) == -1
    assert "argument sites=0x10" in _lib.last_error()


def test_dropin_rules_without_a_device():
    diff = synth.make_diffuser(seed=0, num_layers=1)
    assert diff.engine_dropout is False and diff.engine_grad is False
    diff.engine_grad = True
    diff.train()
    x, z = torch.zeros(1, 2, 9), torch.zeros(1, 2, 384)
    with pytest.raises(RuntimeError) as off:                   # off: today's refusal, word for word
        diff.p_losses(x, torch.tensor([3]), z=z, noise=x)
    assert str(off.value) == ("engine_grad: the diffuser is in .train() mode and its encoder layers have dropout p = 0.1: the reference "
                              "would apply dropout there and the engine does not (no-dropout rule). Set TRANSFORMER.dropout = 0 or call .eval()")
    diff.engine_dropout = True
    assert diff._dropout_p() == 0.1
    with pytest.raises(RuntimeError, match="AMD GPU"):         # on: the rule lets it through to the device check
        diff.p_losses(x, torch.tensor([3]), z=z, noise=x)
    diff.model._trunk.layers[0].dropout2.p = 0.25
    with pytest.raises(RuntimeError, match=r"engine_dropout.*different probabilities \(0\.1 and 0\.25\)"):
        diff.p_losses(x, torch.tensor([3]), z=z, noise=x)
    diff.model._trunk.layers[0].dropout2.p = 0.1
    diff.model._trunk.layers[0].self_attn.dropout = 0.0
    with pytest.raises(RuntimeError, match=r"different probabilities \(0\.0 and 0\.1\)"):
        diff.p_losses(x, torch.tensor([3]), z=z, noise=x)
