"""CPU: the public surface of GGS above 64 frames -- the engine option PD_OPT_GGS_MAX_FRAMES and the cfg flag PD_GGS_CFG_LONG_FRAMES in
include/pd_engine.h and posediffusion_amd/_lib.py; no new export; the drop-in's default limit."""
import os
import re

from posediffusion_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "pd_engine.h")) as fh:
        return fh.read()


def test_lib_constants_match_the_header():
    hdr = _header()
    for name, want in (("PD_OPT_GGS_MAX_FRAMES", 7), ("PD_GGS_CFG_LONG_FRAMES", 64)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert m, name
        assert int(m.group(1)) == want == getattr(_lib, name), name
    # a flag of its own among the pd_ggs_cfg.reserved bits, an id of its own among the options
    flags = {n: int(v) for n, v in re.findall(r"#define\s+(PD_GGS_CFG_\w+)\s+(\d+)", hdr)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values()), flags
    opts = {n: int(v) for n, v in re.findall(r"#define\s+(PD_OPT_\w+)\s+(\d+)", hdr)}
    assert len(set(opts.values())) == len(opts), opts


def test_no_new_export():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = set(re.findall(r"\b(pd_\w+)\s*\(", hdr))
    assert len(protos) == 43, sorted(protos)
    assert protos == set(_lib.SIGNATURES), protos ^ set(_lib.SIGNATURES)


def test_the_dropins_default_limit_is_unchanged():
    assert host.GGS_MAX_FRAMES == 64
    from posediffusion_amd import synth
    assert synth.make_diffuser(seed=0).ggs_max_frames == 64
