"""Register / scratch budget of the trainer's key-tiled attention kernels (posediffusion_amd/csrc/pd_train_lattn.h, launched from
pd_train.hip), read from hipcc's resource remarks like tests/test_kernel_resources_train.py (cross-compiled for gfx950, no GPU needed):
the forward and both phases of the backward exist in their DROP = false and DROP = true instantiations, carry the pd_tr_ prefix, neither
spill nor touch scratch, and their names do not collide with the stems the short kernels are pinned under."""
import shutil

import pytest

from test_kernel_resources_train import _kernel_resources

# (substring of the mangled name): template <bool DROP> mangles as ILb1E / ILb0E
LONG = ("pd_tr_lattn_kernel", "pd_tr_lattn_bwd_rows_kernel", "pd_tr_lattn_bwd_keys_kernel")
SHORT = ("pd_tr_attn_kernelILb0E", "pd_tr_attn_kernelILb1E", "pd_tr_attn_bwd_kernelILb0E", "pd_tr_attn_bwd_kernelILb1E")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_key_tiled_attention_kernels_exist_in_both_variants_and_do_not_spill(tmp_path):
    kernels = _kernel_resources("pd_train.hip", tmp_path)
    for stem in LONG:
        for variant in ("ILb0E", "ILb1E"):
            match = [k for k in kernels if stem + variant in k]
            assert len(match) == 1, (stem + variant, sorted(kernels))
            assert "pd_tr_" in match[0]
            r = kernels[match[0]]
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (match[0], r)
    for stem in SHORT:                                   # the short kernels keep their one instantiation each
        assert len([k for k in kernels if stem in k]) == 1, (stem, sorted(kernels))
    assert not [k for k in kernels if "pd_attn_long" in k], sorted(kernels)
