"""No GPU: pd_trainer_set_frame_counts (include/pd_engine_train.h) is exported and bound, refuses a NULL trainer, and the Python layers
validate ``n_frames`` -- one count per sequence, each in [1, N] -- before they need a device."""
import os

import pytest
import torch

from posediffusion_amd import _lib, synth
from posediffusion_amd.train import PoseTrainer, check_frame_counts, p_losses_with_grad


def test_symbol_is_exported_bound_and_refuses_a_null_trainer():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    assert "pd_trainer_set_frame_counts" in _lib.TRAIN_SIGNATURES
    lib = _lib.load()
    assert lib.pd_trainer_set_frame_counts.argtypes == _lib.TRAIN_SIGNATURES["pd_trainer_set_frame_counts"][1]
    counts = (_lib.C.c_int32 * 2)(3, 2)
    assert lib.pd_trainer_set_frame_counts(None, 2, counts, None) == -1
    assert "pd_trainer_set_frame_counts" in _lib.last_error() and "NULL trainer" in _lib.last_error()
    assert lib.pd_trainer_set_frame_counts(None, 0, None, None) == -1


def test_check_frame_counts_names_the_rule():
    assert check_frame_counts(torch.tensor([5, 1, 3]), 3, 5) == [5, 1, 3]
    assert check_frame_counts((2, 2), 2, 2) == [2, 2]
    with pytest.raises(ValueError, match=r"one frame count per sequence \(3\), got 2"):
        check_frame_counts([5, 1], 3, 5)
    with pytest.raises(ValueError, match=r"every count must lie in \[1, N\] \(N=5\)"):
        check_frame_counts([5, 0, 3], 3, 5)
    with pytest.raises(ValueError, match=r"every count must lie in \[1, N\] \(N=5\)"):
        check_frame_counts([5, 6, 3], 3, 5)


def test_trainer_forward_validates_n_frames_before_it_needs_a_device():
    tr = PoseTrainer.__new__(PoseTrainer)                    # no pd_trainer behind it: validation comes first
    tr._h = None
    x = torch.zeros(3, 5, 9)
    for bad, msg in (([5, 1], "one frame count per sequence"), ([5, 0, 3], r"\[1, N\]"), ([5, 1, 6], r"\[1, N\]")):
        with pytest.raises(ValueError, match=msg):
            tr.forward({}, x, torch.zeros(3, 5, 4), torch.zeros(3, dtype=torch.long), x, "l1", n_frames=bad)
        with pytest.raises(ValueError, match=msg):
            p_losses_with_grad(tr, torch.nn.Linear(1, 1), x, torch.zeros(3, 5, 4), torch.zeros(3, dtype=torch.long), x, n_frames=bad)


def test_dropin_p_losses_validates_n_frames_before_it_needs_a_device():
    diff = synth.make_diffuser(seed=0, num_layers=1)
    x, z, t = torch.zeros(2, 3, 9), torch.zeros(2, 3, 384), torch.tensor([3, 4])
    for grad in (False, True):
        diff.engine_grad = grad
        diff.eval()
        with pytest.raises(ValueError, match="one frame count per sequence"):
            diff.p_losses(x, t, z=z, noise=x, n_frames=[3])
        with pytest.raises(ValueError, match=r"every count must lie in \[1, N\] \(N=3\)"):
            diff.p_losses(x, t, z=z, noise=x, n_frames=[3, 4])
        with pytest.raises(ValueError, match=r"every count must lie in \[1, N\]"):
            diff(x, z=z, n_frames=[0, 3])
        with pytest.raises(RuntimeError, match="AMD GPU"):       # valid counts reach the device check: the trainer, in either grad mode
            diff.p_losses(x, t, z=z, noise=x, n_frames=[3, 1])
    with pytest.raises(NotImplementedError, match="needs the image features z"):
        diff.p_losses(x, t, noise=x, n_frames=[3, 1])
