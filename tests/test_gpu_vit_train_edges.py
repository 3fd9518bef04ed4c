"""GPU (-m gpu): the backbone trainer (include/pd_engine_vit_train.h) at the workload's row counts, at image sizes that are no multiple
of the patch, on the key-tile edges of its attention, at the limits of its shape family and under trained-like weights.  The cases and
what each one reaches are in tests/vit_train_edge_cases.py; tests/test_vit_train_edges_cpu.py shows from the reference alone that the
checks below see what each case is there for.

The rule is tests/test_gpu_vit_train.py's, through its own ``_assert_parity`` and ``RECORDED_MARGIN``: z, every gradient tensor and every
q / k / v and cls / patch block at most max(4 x own, 8 x 2^-24) from float64 autograd; zero in float64 is exactly zero; the k rows of
attn.qkv.bias are printed only.  No other tolerance.
  1. PARITY at every case of vit_train_edge_cases.EDGES; the worst distance / bound of the case is printed (profiles/vit_train_parity.txt).
     trained_grid_wide / _tall (224 x 232, 232 x 224: the trained 14 x 14 grid under unequal pixel sizes, which DINO resamples) missed
     before the fix -- z 4.650e-4 and 5.822e-4 from float64 against bounds of 1.5e-6 and 1.9e-6 -- for two reasons: pd_vit_train_forward
     took pos_embed for every 14 x 14 grid, and torch's GPU bicubic kernel, which VitTrainer resampled with, copies at equal sizes.  The
     yardstick there is vit_train_checks.reference's adjoint of the oracle's own forward (torch's CPU bicubic backward copies too).
     massive_channel missed while data-gradient reductions ran as chains of 384 terms: blocks.1.norm1.weight was 5.539e-07 from float64
     against the floor of 4.768e-07 (own 1.805e-08).  Its maximum is channel 137, a cancelling column sum behind qkv's data gradient;
     cut into chains of 96 the entry's error halves over seven inputs and the tensor is at 1.967e-07 (profiles/vit_train_parity.txt
     section 5).
  2. STATE, bitwise: one trainer runs rows_2758, five_images, rows_2758; the second and third results are those of fresh trainers of
     exactly fitting capacity (stale stash rows, the stride of the final LayerNorm's statistics).
  3. VIEWS, bitwise: channels-last images and a slice of a wider tensor give the bits of the contiguous call.
  4. REFUSAL: a NULL table at 224 x 232 is PD_ERR_INVALID_ARG naming pos[0], and the trainer stays usable.
Every figure is printed before it is asserted."""
import pytest
import torch

import vit_train_checks as VC
import vit_train_edge_cases as EC
from posediffusion_amd.vit_train import VitTrainer, shape_from_module, token_rows
from test_gpu_vit_train import DEV, _Net, _assert_parity, _engine_pass

pytestmark = pytest.mark.gpu


class _EdgeNet(_Net):
    """``_Net`` around a network of vit_train_edge_cases.net_of instead of make_net"""

    def __init__(self, family, depth):
        self.cpu = EC.net_of(family, depth)
        self.gpu = {k: v.detach().to(DEV).contiguous() for k, v in self.cpu.named_parameters()}
        self.shape = shape_from_module(self.cpu)
        self._trainers, self._refs = {}, {}


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(family, depth):
        if (family, depth) not in made:
            made[family, depth] = _EdgeNet(family, depth)
        return made[family, depth]
    yield get
    for n in made.values():
        n.close()


def _fresh(net, case):
    return VitTrainer(net.shape, case.n, case.n * token_rows(case.H, case.W, case.scales), len(case.scales), device=torch.device(DEV))


@pytest.mark.parametrize("name", list(EC.EDGES))
def test_forward_and_every_gradient_against_float64(nets, name):
    edge = EC.EDGES[name]
    case = edge.case
    net = nets(edge.family, case.depth)
    images, g_z, ref64, ref32 = net.reference(case)
    tr = _fresh(net, case)                                               # of exactly fitting capacity, freed with the test
    try:
        z, grads = _engine_pass(tr, net.gpu, images, g_z, case.scales)
    finally:
        tr.close()
    ratio, where = VC.worst_ratio(z, grads, ref64, ref32)
    print(f"[{name}] worst distance / bound {ratio:.3f} at {where}")
    _assert_parity(name, z, grads, ref64, ref32)


def test_a_missing_table_is_refused_where_dino_resamples_the_trained_grid(nets):
    case = EC.EDGES["trained_grid_wide"].case
    net = nets("make_net", 1)
    images, g_z, ref64, ref32 = net.reference(case)
    tr = _fresh(net, case)
    try:
        pos_for = tr._pos_for
        tr._pos_for = lambda *a: None                                    # what a caller does that takes every 14 x 14 grid for the trained table
        with pytest.raises(RuntimeError, match=r"code -1.*pos\[0\]: NULL.*needs the resampled position table"):
            tr.forward(net.gpu, images.to(DEV), case.scales)
        tr._pos_for = pos_for
        z, grads = _engine_pass(tr, net.gpu, images, g_z, case.scales)   # the refused call left the trainer usable
    finally:
        tr.close()
    _assert_parity("after the refusal", z, grads, ref64, ref32)


def _same_bits(a, b):
    (za, ga), (zb, gb) = a, b
    return ([] if torch.equal(za, zb) else ["z"]) + [k for k in ga if not torch.equal(ga[k], gb[k])]


def test_a_reused_trainer_gives_the_bits_of_fresh_ones(nets):
    big, small = EC.EDGES["rows_2758"].case, EC.EDGES["five_images"].case
    net = nets("make_net", 1)
    fresh = {}
    for case in (big, small):
        tr = _fresh(net, case)
        images, g_z, _, _ = net.reference(case)
        fresh[case] = _engine_pass(tr, net.gpu, images, g_z, case.scales)
        tr.close()
    # capacity beyond both cases in every unit: images (the stride of the final LayerNorm's statistics), rows, scales
    shared = VitTrainer(net.shape, big.n + 2, big.n * token_rows(big.H, big.W, big.scales) + 100, 4, device=torch.device(DEV))
    try:
        for step, case in enumerate((big, small, big)):
            images, g_z, _, _ = net.reference(case)
            differ = _same_bits(_engine_pass(shared, net.gpu, images, g_z, case.scales), fresh[case])
            print(f"call {step} ({case.label}) on the shared trainer: {len(differ)} tensors differ from a fresh trainer's {differ[:4]}")
            assert differ == []
    finally:
        shared.close()


def test_non_contiguous_images_give_the_bits_of_the_contiguous_call(nets):
    case = EC.EDGES["ragged_pixels"].case
    net = nets("make_net", 1)
    images, g_z, _, _ = net.reference(case)
    tr = _fresh(net, case)
    try:
        plain = _engine_pass(tr, net.gpu, images, g_z, case.scales)
        cl = images.to(DEV).contiguous(memory_format=torch.channels_last)
        wide = torch.rand(case.n, 3, case.H + 3, case.W + 9, device=DEV)
        wide[:, :, 2:2 + case.H, 5:5 + case.W] = images.to(DEV)
        view = wide[:, :, 2:2 + case.H, 5:5 + case.W]
        assert not cl.is_contiguous() and not view.is_contiguous() and torch.equal(cl.cpu(), images) and torch.equal(view.cpu(), images)
        for label, x in (("channels_last", cl), ("slice of a wider tensor", view)):
            differ = _same_bits(_engine_pass(tr, net.gpu, x, g_z, case.scales), plain)
            print(f"{label}: {len(differ)} tensors differ from the contiguous call's")
            assert differ == []
    finally:
        tr.close()
