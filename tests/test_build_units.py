"""The library's translation units (lam_slide_amd/_lib.py UNITS): k_linear1_ts is compiled in csrc/unit_lin1.hip with options of its own, so
that hipcc keeps its hidden-512 instances in the register file.  Read from the code-object notes of the built library (no GPU needed):

  * k_linear1_ts<32, 512, 8, true> (the kernel bench.py spends half a step in) and <32, 512, 8, false> use no scratch and at most 256 VGPRs;
  * no instance of k_linear1_ts has more scratch than it had as part of the single translation unit (the table below: that build's notes);
  * every instance host_launch.hip.h can dispatch is in the library exactly once;
  * lsl_build_info() names each unit's options.

The other units hold one family of entry points each (the sampling path, the losses, the evaluation statistics, the frozen stage 1), with
the kernels those launch: every kernel is in exactly one code object, each unit's code object holds its family's, and a refused call of any
unit leaves its message where lsl_last_error() reads it."""
import collections
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


@pytest.fixture(scope="module")
def unit_kernels():
    """{unit: the kernel symbols of its code object} - the library holds one code object per unit, in link order"""
    assert os.path.exists(isa_scan.LLVM + "/llvm-readelf"), "the ROCm LLVM tools that build() compiles with"
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    objects = isa_diff.notes_by_object(_lib.LIB_PATH)
    assert len(objects) == len(_lib.UNITS), (len(objects), _lib.UNITS)
    return {name: [sym for sym, _ in obj] for (name, _), obj in zip(_lib.UNITS, objects)}


def test_every_kernel_is_in_exactly_one_code_object(unit_kernels):
    count = collections.Counter(sym for syms in unit_kernels.values() for sym in syms)
    assert len(count) > 200 and all(sym.endswith(".kd") for sym in count), len(count)
    assert [sym for sym, n in count.items() if n != 1] == []


def test_each_unit_owns_its_kernels(unit_kernels):
    def units_of(kernel):  # the units whose code object holds an instance of `kernel`, and how many
        return {unit: n for unit, syms in unit_kernels.items() if (n := sum(kernel in sym for sym in syms))}

    for kernel in ("k_geom_loss_frame", "k_class_loss_frame", "k_loss_final"):
        assert set(units_of(kernel)) == {"unit_loss.hip"}, (kernel, units_of(kernel))
    finals = {tuple(int(v) for v in re.match(r"_Z12k_loss_finalILi(\d+)ELi(\d+)ELi(\d+)EE", sym).groups())
              for sym in unit_kernels["unit_loss.hip"] if "k_loss_final" in sym}
    assert finals == {(5, 0, 3), (5, 4, 5), (2, 0, 1)}, finals  # the geometry, peptide and class finals: every instance there is
    for kernel in ("k_msm_step", "k_dihedral", "k_wmom_tiles"):
        assert set(units_of(kernel)) == {"unit_stat.hip"}, (kernel, units_of(kernel))
    assert set(units_of("k_dec_attn")) == {"unit_stage1.hip"}, units_of("k_dec_attn")
    assert units_of("k_linear1_ts") == {"unit_lin1.hip": len(SCRATCH_BEFORE)}, units_of("k_linear1_ts")
    assert all("k_linear1_ts" in sym for sym in unit_kernels["unit_lin1.hip"])  # (and nothing else: the unit's options are that kernel's)


def test_one_error_buffer_across_units():
    """One refused call per unit, refused by its shape check before any launch (the pointers are never dereferenced): each leaves its own
    message in the one buffer lsl_last_error() reads."""
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    calls = {
        "unit_stat.hip": (lambda: lib.lsl_msm_active_set(p, 0, 4, p, p, None), -3, "S = 0, ns = 4: S outside 1..65535 series"),
        "unit_loss.hip": (lambda: lib.lsl_geom_loss_sums(p, p, p, 1, 0, 3, p, None), -3, "A = 0 outside the native form (1..2048 entities)"),
        "unit_stage1.hip": (lambda: lib.lsl_decoder_create(None, None, None), -1, "null decoder argument"),
        "lsl_api.hip": (lambda: lib.lsl_model_create(None, None), -1, "null argument"),
    }
    assert set(calls) == {name for name, _ in _lib.UNITS} - {"unit_lin1.hip"}  # (unit_lin1.hip has no entry point)
    for order in (list(calls), list(calls)[::-1]):  # (each message replaces the one before it, whichever unit wrote that)
        for unit in order:
            fn, code, message = calls[unit]
            assert fn() == code, unit
            assert lib.lsl_last_error().decode() == message, (unit, lib.lsl_last_error())
