"""No GPU: the frame-count yardstick (tests/train_ragged_checks.py) IS the definition of pd_trainer_set_frame_counts
(include/pd_engine_train.h):

  (a) without dropout its loss and every gradient are the sum over the sequences of ``train_checks.loss_and_grads`` on the sliced
      sequence alone (masks, signs and g_loss sliced as well; dz in the padded layout, zero at padding), to 1e-12 relative in float64;
  (b) with all counts = N it returns, bit for bit, what ``loss_and_grads`` / ``loss_and_grads_dropout`` return in float64;
  (c) changing the padding rows of every input to other finite values (and to NaN) changes no output bit."""
import pytest
import torch

from denoiser_cfgs import Cfg, build_dropin
import train_checks as TC
import train_dropout_checks as TD
import train_ragged_checks as TR

NONDEFAULT = Cfg(96, 4, 200, 2, 50, 40, True, False)        # the GPU suite's non-default configuration (no pivot)
PIVOT = Cfg(96, 4, 200, 2, 50, 40, True, True)


def _case(cfg, seed, B, N, t):
    den = build_dropin(cfg, seed=seed)
    sd = {k: v.detach().clone() for k, v in den.state_dict().items() if v.is_floating_point()}
    g = torch.Generator().manual_seed(100 * B + N)
    inp = {"x_start": torch.randn(B, N, 9, generator=g), "noise": torch.randn(B, N, 9, generator=g),
           "z": torch.randn(B, N, cfg.z, generator=g), "t": torch.tensor(t)}
    return sd, TC.Net.of_cfg(cfg), inp


def _same(a, b, what):
    assert a.dtype == b.dtype and torch.equal(a, b), what


def _assert_results_bitwise(r, q, what):
    for k in ("loss", "model_out", "x_t"):
        _same(r[k], q[k], (what, k))
    assert set(r["grads"]) == set(q["grads"])
    for n in q["grads"]:
        _same(r["grads"][n], q["grads"][n], (what, n))
    for a, b in zip(r["pre"], q["pre"]):
        _same(a, b, (what, "pre"))
    _same(r["signs"], q["signs"], (what, "signs"))


@pytest.mark.parametrize("cfg,counts,N,objective,loss_type", [(NONDEFAULT, (7, 1, 4), 7, "pred_noise", "l1"), (PIVOT, (5, 2, 3), 5, "pred_x0", "l2"),
                                                               (PIVOT, (5, 2, 3), 5, "pred_noise", "l1")],
                         ids=["n7-nopivot-l1", "n5-pivot-x0-l2", "n5-pivot-l1"])
def test_a_ragged_yardstick_is_the_sum_over_the_sequences_alone(cfg, counts, N, objective, loss_type):
    B = len(counts)
    sd, net, inp = _case(cfg, 31, B, N, [99, 0, 41])
    g_loss = TC.draw_g_loss(B, N, seed=1) + 0.01 / (B * N * 9)           # no all-zero sequence: every slot has a gradient to compare
    for g in (None, g_loss):
        r = TR.loss_and_grads(sd, net, inp, counts, objective, loss_type, g_loss=g)
        gl = TR.default_g_loss(counts, N) if g is None else g.double()
        total = {n: torch.zeros_like(v) for n, v in r["grads"].items()}
        for b, n in enumerate(counts):
            alone = TC.loss_and_grads(sd, net, TR.slice_sequence(inp, b, n), objective, loss_type, g_loss=gl[b:b + 1, :n],
                                      masks=[m[b:b + 1, :n] for m in r["masks"]], signs=r["signs"][b:b + 1, :n])
            for k in ("loss", "model_out", "x_t"):
                ref = alone[k]
                assert (r[k][b:b + 1, :n] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item(), (b, k)
                assert (r[k][b, n:] == 0).all() and not torch.signbit(r[k][b, n:]).any(), (b, k, "padding rows are +0")
            for a, m in zip(alone["pre"], r["masks"]):                    # the forced masks are the sliced sequence's own: nothing was bent
                assert torch.equal(a > 0, m[b:b + 1, :n])
            for name, v in alone["grads"].items():
                if name == "z":
                    total["z"][b:b + 1, :n] += v
                else:
                    total[name] += v
        for name, v in total.items():
            assert TC.grad_dist(r["grads"][name], v) <= 1e-12, (name, TC.grad_dist(r["grads"][name], v))
        for b, n in enumerate(counts):
            assert (r["grads"]["z"][b, n:] == 0).all(), ("dz at padding", b)


@pytest.mark.parametrize("cfg", [NONDEFAULT, PIVOT], ids=["nopivot", "pivot"])
def test_b_all_counts_equal_to_n_is_the_uniform_yardstick_bit_for_bit(cfg):
    B, N = 3, 7
    sd, net, inp = _case(cfg, 31, B, N, [99, 0, 41])
    counts = (N,) * B
    for objective, loss_type in (("pred_noise", "l1"), ("pred_x0", "l2")):
        for g in (None, TC.draw_g_loss(B, N)):
            q = TC.loss_and_grads(sd, net, inp, objective, loss_type, g_loss=g)
            _assert_results_bitwise(TR.loss_and_grads(sd, net, inp, counts, objective, loss_type, g_loss=g), q, (objective, loss_type, "plain"))
            forced = {"masks": q["masks"], "signs": q["signs"]}
            q = TC.loss_and_grads(sd, net, inp, objective, loss_type, g_loss=g, **forced)
            _assert_results_bitwise(TR.loss_and_grads(sd, net, inp, counts, objective, loss_type, g_loss=g, **forced), q, (objective, loss_type, "forced"))
        drop = dict(p=0.1, sites=TD.ALL, seed=11, step=3)
        q = TD.loss_and_grads_dropout(sd, net, inp, objective, loss_type, drop["p"], drop["sites"], drop["seed"], drop["step"])
        _assert_results_bitwise(TR.loss_and_grads(sd, net, inp, counts, objective, loss_type, **drop), q, (objective, loss_type, "dropout"))


@pytest.mark.parametrize("drop", [{}, dict(p=0.1, sites=TD.ALL, seed=11, step=0)], ids=["plain", "dropout"])
def test_c_padding_rows_of_the_inputs_are_not_read(drop):
    counts, N = (7, 1, 4), 7
    B = len(counts)
    sd, net, inp = _case(NONDEFAULT, 31, B, N, [99, 0, 41])
    g_loss = TC.draw_g_loss(B, N, seed=1) + 0.01 / (B * N * 9)
    valid = TR.valid_rows(counts, N)
    base = TR.loss_and_grads(sd, net, inp, counts, "pred_noise", "l1", g_loss=g_loss, **drop)
    for fill in (3.25, -1e30, float("nan")):
        other = {k: (torch.where(valid[..., None], v, torch.full((), fill)) if k != "t" else v) for k, v in inp.items()}
        g_other = torch.where(valid[..., None], g_loss, torch.full((), fill))
        assert not torch.equal(torch.nan_to_num(other["z"]), inp["z"])
        _assert_results_bitwise(TR.loss_and_grads(sd, net, other, counts, "pred_noise", "l1", g_loss=g_other, **drop), base, fill)


def test_dropout_masks_are_those_of_the_padded_layout():
    """A mask row computed with the count instead of the stride is another mask for every head >= 1 of the first sequence already."""
    counts, N, nhead = (4, 7), 7, 4
    full = TD.keep_mask(len(counts) * nhead * N, N, 0, 0, 11, 0, 0.5)
    packed = TD.keep_mask(nhead * counts[0], N, 0, 0, 11, 0, 0.5)
    assert (full[:counts[0]] == packed[:counts[0]]).all()                                     # head 0 of sequence 0: rows 0 .. agree
    assert (full[N:N + counts[0]] != packed[counts[0]:2 * counts[0]]).any()                   # head 1: the padded row is N + i, not n + i
