"""Register / scratch budget of the trainer kernels that frame counts per sequence touch (pd_trainer_set_frame_counts; pd_train_lattn.h
and pd_train_kernels.h, compiled in pd_train.hip), read from hipcc's resource remarks like tests/test_kernel_resources_train.py
(cross-compiled for gfx950, no GPU needed): the key-tiled attention forward and both phases of its backward, which now take the count
pointer, in their DROP = false and DROP = true instantiations; the first and last kernels of the pass, which treat padding rows as
absent; and the two small kernels that carry the counts.  None spills, none touches scratch; the count pointer is a run-time argument,
so every templated kernel keeps one instantiation per DROP value."""
import shutil

import pytest

from test_kernel_resources_train import _kernel_resources

TEMPLATED = ("pd_tr_lattn_kernel", "pd_tr_lattn_bwd_rows_kernel", "pd_tr_lattn_bwd_keys_kernel")
PLAIN = ("pd_tr_q_sample_kernel", "pd_tr_embed_kernel", "pd_tr_tail_kernel", "pd_tr_tail_bwd_kernel", "pd_tr_set_counts_kernel",
         "pd_tr_copy_counts_kernel")


def _clean(name, r):
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_with_frame_counts_do_not_spill_and_keep_their_instantiations(tmp_path):
    kernels = _kernel_resources("pd_train.hip", tmp_path)
    for stem in TEMPLATED:
        for variant in ("ILb0E", "ILb1E"):
            match = [k for k in kernels if stem + variant in k]
            assert len(match) == 1, (stem + variant, sorted(kernels))
            _clean(match[0], kernels[match[0]])
        assert len([k for k in kernels if stem in k]) == 2, (stem, sorted(kernels))
    for stem in PLAIN:
        match = [k for k in kernels if stem in k]
        assert len(match) == 1 and "pd_tr_" in match[0], (stem, sorted(kernels))
        _clean(match[0], kernels[match[0]])
