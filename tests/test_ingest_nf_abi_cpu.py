"""No GPU: the C-ABI of device-side match ingestion with one frame count per sequence (pd_ggs_set_matches_csr_async_nf) -- declared in
include/pd_engine_ingest.h (the extension header: the function list of pd_engine.h is pinned), exported by the built library, bound in
posediffusion_amd._lib (EXT_SIGNATURES) with the header's argument list -- and the host-side
packing that feeds it (host.pack_matches_ragged)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from posediffusion_amd import _lib, host
from posediffusion_amd.engine import PoseEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, OLD = "pd_ggs_set_matches_csr_async_nf", "pd_ggs_set_matches_csr_async"


def _args(name, header="pd_engine_ingest.h"):
    with open(os.path.join(ROOT, "include", header)) as fh:
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", fh.read())
    assert m, f"{name} is not declared in include/{header}"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_symbol_is_declared_in_the_header_with_the_documented_signature():
    assert _args(NAME) == ["pd_engine *eng", "int seq_first", "int n_seqs", "const int64_t *seq_offsets", "const double *kp1",
                           "const double *kp2", "const int64_t *i12", "const int *n_frames", "int height", "int width",
                           "const pd_match_hints *hints", "void *stream"]
    # the old export is untouched: the same list with one frame count for the call
    assert _args(OLD, "pd_engine.h") == [a if a != "const int *n_frames" else "int n_frames" for a in _args(NAME)]


def test_extension_header_and_ext_signatures_list_the_same_functions():
    with open(os.path.join(ROOT, "include", "pd_engine_ingest.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert set(re.findall(r"\b(pd_\w+)\s*\(", hdr)) == set(_lib.EXT_SIGNATURES) == {NAME}
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)


def test_symbol_is_bound_in_lib_with_the_headers_argument_list():
    res, args = _lib.EXT_SIGNATURES[NAME]
    old = _lib.SIGNATURES[OLD][1]
    assert res is C.c_int and len(args) == len(_args(NAME)) == 12
    assert args[7] == C.POINTER(C.c_int)
    assert [a for i, a in enumerate(args) if i != 7] == [a for i, a in enumerate(old) if i != 7] and old[7] is C.c_int


@pytest.fixture(scope="module")
def lib():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    return _lib.load()


def test_symbol_is_exported_and_refuses_a_null_engine_and_null_counts(lib):
    assert getattr(lib, NAME).argtypes == _lib.EXT_SIGNATURES[NAME][1]
    off = (C.c_int64 * 2)(0, 4)
    counts = (C.c_int * 1)(8)
    assert getattr(lib, NAME)(None, 0, 1, off, None, None, None, counts, 224, 224, None, None) == -1      # PD_ERR_INVALID_ARG
    assert NAME in _lib.last_error()


def test_set_matches_async_takes_n_frames_and_upload_matches_device_side():
    p = inspect.signature(PoseEngine.set_matches_async).parameters
    assert "n_frames" in p and p["n_frames"].default is None
    p = inspect.signature(host.upload_matches).parameters
    assert "device_side" in p and p["device_side"].default is False


def _md(n_frames, m, hw=(224, 224), seed=0):
    rng = np.random.default_rng(seed)
    return {"kp1": rng.uniform(0, 200, (m, 2)), "kp2": rng.uniform(0, 200, (m, 2)),
            "i12": rng.integers(0, n_frames, (m, 2)).astype(np.int64), "img_shape": (n_frames, 3, *hw)}


def test_pack_matches_ragged_offsets_counts_and_rows():
    mds = [_md(8, 5, seed=1), _md(20, 11, seed=2), _md(13, 1, seed=3)]
    kp1, kp2, i12, off, shape, counts = host.pack_matches_ragged(mds, pin=False)
    assert off.tolist() == [0, 5, 16, 17] and counts == [8, 20, 13] and tuple(shape) == (20, 3, 224, 224)
    assert kp1.shape == kp2.shape == i12.shape == (17, 2)
    for b, md in enumerate(mds):
        a, e = int(off[b]), int(off[b + 1])
        assert np.array_equal(kp1[a:e].numpy(), md["kp1"]) and np.array_equal(kp2[a:e].numpy(), md["kp2"])
        assert np.array_equal(i12[a:e].numpy(), md["i12"])
    assert mds[0]["img_shape"] == (8, 3, 224, 224)                # the callers' dicts are not touched


def test_pack_matches_ragged_refuses_differing_image_sizes():
    with pytest.raises(ValueError, match="image size"):
        host.pack_matches_ragged([_md(8, 5), _md(20, 5, hw=(192, 320))], pin=False)


def test_pack_matches_still_refuses_differing_frame_counts():
    with pytest.raises(ValueError, match="must share img_shape"):
        host.pack_matches([_md(8, 5), _md(20, 5)], pin=False)
    assert len(host.pack_matches([_md(8, 5), _md(8, 7)], pin=False)) == 5
