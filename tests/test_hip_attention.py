"""The attention kernels of the second stage (csrc/k_attn.hip.h: k_attention_stream short / grouped / long / chunked / chunked with the
denominator column, k_attention_rows<4,4,1> .. <16,1,0>, k_attention_tiny, k_attention_linear), row by row against an fp64 softmax of
the very bf16 q | k | v the kernel read (lsl_debug_taps), at the case table of attention_cases.py: every form at its tile, chunk and
group edges, both head layouts, packed launches with a partial last tile, the persistent loop with more than three units per
workgroup, the three softmax regimes, the knob-selected fallback forms.

Every token, head and real channel d must satisfy (derivation: attention_cases.py)
  * MFMA forms:         |z[d] - o[d]| <= 2^-6 A[d]        (u = 2^-8: p rounded once: u A + u A, o rounded once: u A; bar 4 u A)
  * k_attention_tiny:   |z[d] - o[d]| <= 2^-8 |o[d]| + (S + head_dim + 16) 2^-23 A[d]
  * k_attention_linear: the same with A_lin = q_s (k_s^T |v|)   (fp32 throughout, one bf16 rounding on the way out)
with o = p v, A = p |v| of the fp64 reference.  conftest.parity prints the worst element of each (case, sub-block, form, arm) in units
of u A; measured on MI355X (profiles/attention_rowwise_parity.txt): MFMA forms 0.66 .. 2.26 u A against the bar of 4, worst on the packed tiny
axes and rows<4,1,4> at the sharp gain; tiny and linear up to 0.995 of their element bar (one rounding of o).

A comparison counts only under its conditions, asserted on the tapped values: the library reports the intended kernel class
(lsl_profile_kernel_name; the finer form follows from plan_attention's rule, restated and tested in attention_cases.py); at the sharp
gain every key position carries p_j >= 0.25 for some query, so that a dropped, doubled or wrongly masked key would move an element far
beyond the bar; the kernel's own softmax-regime predicate, recomputed from the tapped q / k and the norm scales, gives the regime the
arm intends.  Padded output channels (channel >= head_dim of a head) must be finite: linear2 multiplies them by zero columns."""
import os
import subprocess
import sys

import pytest
import torch

import attention_cases as ac
from conftest import parity
from test_hip_parity import _hip_taps, build_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_NETS = {}


def _net(model, arm, linear, dev):
    key = (model, arm, linear)
    if key not in _NETS:
        sh, p = ac.params(model, arm, linear)
        net = build_net(sh, p, dev)
        net.ensure_packed(dev)
        _NETS[key] = net
    return _NETS[key]


def tap_case(case, arm, dev, linear=False):
    """{bi: (qkv [n, 3, H, hdp], z [n, H, hdp], kernel class)} of both sub-blocks, profile class 2 (attention) armed around each tap."""
    from lam_slide_amd import _lib
    model, B, T, L = case[:4]
    lib = _lib.load()
    net = _net(model, arm, linear, dev)
    h, mods = ac.inputs(model, B, T, L)
    h, mods = h.to(dev), mods.to(dev)
    out = {}
    for bi in (0, 1):
        _lib.check(lib.lsl_profile_enable(net._handle, 2, 4))
        qkv, z = _hip_taps(net, lib, bi, h, mods, B, T, L, dev)
        name = lib.lsl_profile_kernel_name(net._handle).decode()
        lib.lsl_profile_enable(net._handle, -1, 0)
        out[bi] = (qkv, z[:, :net.dims.hhd].reshape(-1, net.dims.heads, net.dims.head_dim_pad), name)
    return out


def check_axis(tag, case, arm, bi, tapped, linear=False, flags=None, regime=False):
    """One sub-block of one case: form, per-row bound, padded channels; sharp arm: key coverage; regime=True (or sharp): the softmax regime."""
    qkv, z, name = tapped
    model = case[0]
    hd = ac.head_dims(model)[0]
    pl = ac.case_plans(case, linear, **(flags or {}))[bi]
    assert name == pl.kernel, (tag, name, pl)
    assert torch.isfinite(z).all(), tag  # (the padded channels included)
    q, k, v = ac.axis_qkv(qkv, pl, hd)
    ref = ac.linear_reference(q, k, v) if linear else ac.softmax_reference(q, k, v)
    if arm == "sharp" and not linear:
        assert float(ref.cover.min()) >= 0.25, (tag, "key coverage", float(ref.cover.min()), int(ref.cover.argmin()))
    if (regime or arm == "sharp") and not linear:
        sh, p = ac.params(model, arm)
        pre = "blocks.0." + ("temporal_block" if bi else "spatial_block") + ".norm."
        got = ac.regime(pl, q, k, p[pre + "query_norm.scale"], p[pre + "key_norm.scale"], ac.premul_of(sh), hd)
        assert got == ac.intended_regime(pl, arm), (tag, "regime", got)
    ua, of_bar = ac.worst(ac.axis_view(z[..., :hd], pl), ref, pl.form, pl.S, hd)
    name = f"attn.{tag}.{bi}.{pl.form}.{arm}[uA]"
    # (tiny, linear: the element bar in units of u A is |o| / A + (S + head_dim + 16) 2^-15, at most the figure given to parity)
    parity(name, ua, ac.MFMA_BAR_UA if ac.is_mfma(pl.form) else 1.0 + (pl.S + hd + 16) * 2.0 ** -15)
    assert of_bar <= 1.0, (name, ua, of_bar)


def check_case(case, dev, arms=("unit", "sharp"), linear=False):
    for arm in arms:
        tapped = tap_case(case, arm, dev, linear)
        for bi in (0, 1):
            check_axis(ac.case_id(case), case, arm, bi, tapped[bi], linear)


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_attention_rows_against_fp64_softmax(case, dev):
    check_case(case, dev)


@pytest.mark.parametrize("case", ac.PERSISTENT_CASES, ids=ac.case_id)
def test_stream_persistent_loop_three_units_per_workgroup(case, dev):
    """More units than three times the grid of two workgroups per CU: every workgroup walks at least three units - both K | V images
    and the wrap-around back to the first."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert ac.PERSISTENT_UNITS[case] >= 3 * 2 * cus + 1, (cus, ac.PERSISTENT_UNITS[case])
    check_case(case, dev)


@pytest.mark.parametrize("case", ac.LINEAR_CASES, ids=ac.case_id)
def test_linear_attention_rows_against_fp64(case, dev):
    check_case(case, dev, arms=("unit",), linear=True)


@pytest.mark.parametrize("case,bi,mixed", ac.REGIME_CASES, ids=lambda x: ac.case_id(x) if isinstance(x, tuple) else str(x))
def test_softmax_regimes(case, bi, mixed, dev):
    """No shift at all (launch-wide bound), the per-tile decision with tiles on either side, the exact max pass."""
    for arm in ac.regime_arms(mixed):
        check_axis(ac.case_id(case), case, arm, bi, tap_case(case, arm, dev)[bi], regime=True)


# ---- fallback forms: the knobs are read once per process, so each arm taps its cases in a child ------------------------------------------

def child_main(arm, path):
    """(in the child) tap every case of the arm at both gains and save the tapped tensors and kernel classes"""
    dev = torch.device("cuda:0")
    out = {}
    for case in ac.FALLBACK_ARMS[arm][1]:
        for gain in ("unit", "sharp"):
            for bi, (qkv, z, name) in tap_case(case, gain, dev).items():
                out[ac.case_id(case), gain, bi] = (qkv.to(torch.bfloat16), z.to(torch.bfloat16), name)
    torch.save(out, path)


def _run_child(arm):
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_hip_attention\n"
            "test_hip_attention.child_main(sys.argv[1], sys.argv[2])\n") % (os.path.dirname(here), here)
    path = f"/tmp/lsl_attn_rows_{arm}_{os.getpid()}.pt"
    env = {k: v for k, v in os.environ.items() if k not in ac.FALLBACK_KNOBS}
    env.update(ac.FALLBACK_ARMS[arm][0])
    subprocess.run([sys.executable, "-c", code, arm, path], check=True, env=env, timeout=300)
    res = torch.load(path)
    os.remove(path)
    return {k: (qkv.float(), z.float(), name) for k, (qkv, z, name) in res.items()}


@pytest.mark.parametrize("arm", ["stream_off", "group_off"])
def test_fallback_forms_against_fp64_softmax(arm, dev):
    """LSL_ATTN_STREAM=0: k_attention_rows<4,1,6>, <4,1,8> and <16,1,0> up to the LDS limit, k_attention_tiny where the packed form ran;
    LSL_ATTN_GROUP=0: k_attention_tiny at L = 2, 4, 8."""
    res = _run_child(arm)
    for case in ac.FALLBACK_ARMS[arm][1]:
        for gain in ("unit", "sharp"):
            for bi in (0, 1):
                check_axis(f"{arm}.{ac.case_id(case)}", case, gain, bi, res[ac.case_id(case), gain, bi], flags=ac.arm_flags(arm))


def test_token_major_rows_equal_planes_bit_for_bit(dev):
    """LSL_QKV_PLANES=0: the LONG stream kernel reads q / k / v as token-major rows; same q / k / v bits, same attention output bits as
    the plane layout, and the per-row bound holds for it."""
    rows, planes = _run_child("planes_off"), _run_child("planes_on")
    case = ac.PLANES_CASE
    assert ac.case_plans(case)[0].planes and not ac.case_plans(case, planes_on=False)[0].planes
    for key in planes:
        assert torch.equal(rows[key][0], planes[key][0]) and torch.equal(rows[key][1], planes[key][1]), key
        assert rows[key][2] == planes[key][2]
    for gain in ("unit", "sharp"):
        check_axis(f"planes_off.{ac.case_id(case)}", case, gain, 0, rows[ac.case_id(case), gain, 0], flags=ac.arm_flags("planes_off"))
