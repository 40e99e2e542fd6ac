"""The library's translation units (lam_slide_amd/_lib.py UNITS): k_linear1_ts is compiled in csrc/unit_lin1.hip with options of its own, so
that hipcc keeps its hidden-512 instances in the register file.  Read from the code-object notes of the built library (no GPU needed):

  * k_linear1_ts<32, 512, 8, true> (the kernel bench.py spends half a step in) and <32, 512, 8, false> use no scratch and at most 256 VGPRs;
  * no instance of k_linear1_ts has more scratch than it had as part of the single translation unit (the table below: that build's notes);
  * every instance host_launch.hip.h can dispatch is in the library exactly once;
  * lsl_build_info() names each unit's options."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402
import isa_scan  # noqa: E402

# (head width, hidden, waves, LNF) -> private_segment_fixed_size [bytes per lane] of the single-unit build (-O3, clang 22 / roc-7.2.0)
SCRATCH_BEFORE = {
    (16, 128, 8, 0): 0, (16, 128, 8, 1): 0, (16, 256, 8, 0): 0, (16, 256, 8, 1): 0, (16, 384, 8, 0): 0, (16, 384, 8, 1): 0,
    (16, 512, 4, 0): 0, (16, 512, 8, 0): 0, (16, 512, 8, 1): 24,
    (32, 128, 8, 0): 0, (32, 128, 8, 1): 0, (32, 256, 8, 0): 0, (32, 256, 8, 1): 0, (32, 384, 8, 0): 0, (32, 384, 8, 1): 20,
    (32, 512, 4, 0): 0, (32, 512, 8, 0): 76, (32, 512, 8, 1): 112,
}


@pytest.fixture(scope="module")
def lin1_notes():
    assert os.path.exists(isa_scan.LLVM + "/llvm-readelf"), "the ROCm LLVM tools that build() compiles with"
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    out = {}
    for sym, fields in isa_diff.notes(_lib.LIB_PATH).items():
        m = re.match(r"_Z12k_linear1_tsILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EEv8Lin1Args\.kd$", sym)
        if m:
            key = tuple(int(v) for v in m.groups())
            assert key not in out, sym  # (one definition: the kernel is not also left in the main unit)
            out[key] = {k: int(v) for k, v in fields.items() if v is not None and v.isdigit()}
    return out


def test_every_dispatched_instance_is_built_once(lin1_notes):
    assert set(lin1_notes) == set(SCRATCH_BEFORE), set(lin1_notes) ^ set(SCRATCH_BEFORE)


def test_hidden_512_instances_use_no_scratch(lin1_notes):
    for key in ((32, 512, 8, 1), (32, 512, 8, 0)):
        n = lin1_notes[key]
        print(f"k_linear1_ts<{key}>: {n}")
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
        assert n["vgpr_count"] <= 256, (key, n)  # (8 waves of 64 lanes: two waves per SIMD, half the 512-register file each)


def test_no_instance_has_more_scratch_than_in_the_single_unit(lin1_notes):
    for key, before in SCRATCH_BEFORE.items():
        assert lin1_notes[key]["private_segment_fixed_size"] <= before, (key, lin1_notes[key], before)


def test_build_info_names_the_unit_options():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    lib.lsl_build_info.restype = C.c_char_p
    info = lib.lsl_build_info().decode()
    assert "gfx950" in info
    for name, extra in _lib.UNITS:
        assert f"{name}: {_lib.unit_options(extra)}" in info, (name, info)
    assert dict(_lib.UNITS)["unit_lin1.hip"], "unit_lin1.hip exists for the sake of its own options"
