"""The machinery of the per-row attention tests (attention_cases.py), on the CPU, before test_hip_attention.py relies on it on the
MI355X: the case table reaches every form by plan_attention's rule; the fp64 reference on token-major rows equals the oracle's own
attention output (axis geometry, pre-multiplier, padded heads, linear mode); a torch emulation of each form's roundings stays within
that form's bar; a dropped, doubled or wrongly masked key and a misplaced query row do not; and the key-coverage and softmax-regime
conditions hold on the oracle's values for every case, so that the GPU run is not their first evaluation."""
import functools

import pytest
import torch

import attention_cases as ac

ALL_SOFTMAX = ac.CASES + ac.PERSISTENT_CASES
FALLBACK = tuple((arm, case) for arm, (_, cases) in ac.FALLBACK_ARMS.items() if arm != "planes_on" for case in cases)


@functools.lru_cache(maxsize=4)
def _axis(case, arm, bi, linear=False, flags=()):
    """plan, tapped-like q, k, v of the axis in fp64 and the fp64 reference, from the oracle's bf16-rounded taps."""
    hd = ac.head_dims(case[0])[0]
    pl = ac.case_plans(case, linear, **dict(flags))[bi]
    qkv, _ = ac.oracle_rows(case, arm, bi, linear)
    q, k, v = ac.axis_qkv(qkv, pl, hd)
    ref = ac.linear_reference(q, k, v) if linear else ac.softmax_reference(q, k, v)
    return pl, q, k, v, ref


def test_table_forms_follow_plan_attention_and_every_form_is_reached():
    seen = set()
    lists = [(ac.CASES + ac.PERSISTENT_CASES + tuple(c for c, _, _ in ac.REGIME_CASES), {}, False), (ac.LINEAR_CASES, {}, True)]
    lists += [(cases, ac.arm_flags(arm), False) for arm, (_, cases) in ac.FALLBACK_ARMS.items()]
    for cases, flags, linear in lists:
        for case in cases:
            sp, tm = ac.case_plans(case, linear, **flags)
            assert (sp.form, tm.form) == case[4:], (case, sp.form, tm.form)
            seen.update((pl.form, ac.head_dims(case[0])[1], pl.planes) for pl in (sp, tm))
    forms = {f for f, _, _ in seen}
    assert forms == {"tiny", "grouped", "short", "long", "chunked", "chunked_den", "linear", "rows<4,4,1>", "rows<4,2,2>", "rows<4,1,4>",
                     "rows<4,1,6>", "rows<4,1,8>", "rows<16,1,0>"}
    for f in forms - {"chunked_den", "rows<4,4,1>"}:  # (the denominator column needs 24 of 32; rows<4,4,1> by default only with 2 or 4 heads)
        assert {w for g, w, _ in seen if g == f} == {16, 32}, f
    assert ("long", 32, True) in seen and ("long", 32, False) in seen and ("long", 16, True) in seen and ("long", 16, False) in seen
    assert ac.rows_max_s(32) == 1248 and ac.rows_max_s(16) == 2528
    # the required lengths, per form
    lengths = {}
    for cases, flags, linear in lists:
        for case in cases:
            for pl in ac.case_plans(case, linear, **flags):
                lengths.setdefault(pl.form, set()).add(pl.S)
    need = {"tiny": {1, 2, 3, 4, 5, 6, 7, 8}, "grouped": {2, 4, 8}, "short": {9, 16, 31, 32}, "rows<4,4,1>": {9, 31, 32}, "rows<4,2,2>": {33, 63, 64},
            "rows<4,1,4>": {65, 96, 97, 127, 128}, "long": {129, 160, 255, 256}, "chunked": {257, 288, 511, 512, 513},
            "chunked_den": {257, 513, 1000}, "linear": {1, 2, 33, 257}, "rows<4,1,6>": {129, 192}, "rows<4,1,8>": {193, 256},
            "rows<16,1,0>": {257, 1248, 2528}}
    for f, s in need.items():
        assert s <= lengths[f], (f, s - lengths[f])
    # packed launches of 12 (one partial tile), 44 (ragged last tile) and 64 tokens at every block size that divides them
    packed = {(c[3], c[1] * c[2] * c[3]) for c in ac.CASES if c[4] == "grouped" and c[2] <= 8}
    assert {(2, 12), (2, 44), (2, 64), (4, 12), (4, 44), (4, 64), (8, 64)} <= packed
    # rows<4,4,1> with a partial last workgroup: n_seq H not a multiple of 4
    assert any(pl.form == "rows<4,4,1>" and (pl.n_seq * ac.MODELS[c[0]][1]) % 4 for c in ac.CASES for pl in ac.case_plans(c))
    for case, units in ac.PERSISTENT_UNITS.items():
        assert units >= 3 * 512 + 1


def test_every_softmax_axis_has_16_sequence_head_pairs():
    for case in ALL_SOFTMAX + tuple(c for c, _, _ in ac.REGIME_CASES) + tuple(c for _, c in FALLBACK):
        for pl in ac.case_plans(case):
            assert pl.n_seq * ac.MODELS[case[0]][1] >= 16, (case, pl)


@pytest.mark.parametrize("case", ALL_SOFTMAX + ac.LINEAR_CASES, ids=ac.case_id)
def test_reference_equals_the_oracles_attention_in_fp64(case):
    """Unrounded fp64 oracle taps, laid out as lsl_debug_taps lays them out (token-major, padded heads, q times the pre-multiplier),
    through axis_qkv and the fp64 reference: the oracle's own attention output, to fp64 rounding."""
    linear = case in ac.LINEAR_CASES
    hd = ac.head_dims(case[0])[0]
    for bi in (0, 1):
        pl = ac.case_plans(case, linear)[bi]
        qkv, attn = ac.oracle_rows(case, "sharp", bi, linear, dtype=torch.float64, rounded=False)
        q, k, v = ac.axis_qkv(qkv, pl, hd)
        ref = ac.linear_reference(q, k, v) if linear else ac.softmax_reference(q, k, v)
        want = ac.axis_view(attn, pl)
        err = float((ref.o - want).abs().max() / want.abs().max())
        assert err < 1e-11, (case, bi, err)


def _check_emulation(case, arm, bi, flags=()):
    hd = ac.head_dims(case[0])[0]
    pl, q, k, v, ref = _axis(case, arm, bi, False, flags)
    ua, of_bar = ac.worst(ac.emulate(q, k, v, pl.form), ref, pl.form, pl.S, hd)
    print(f"EMULATED {ac.case_id(case)}.{bi}.{pl.form}.{arm} worst {ua:.2f} uA, {of_bar:.2f} of the bar")
    assert of_bar <= 1.0, (case, arm, bi, ua, of_bar)
    return pl, q, k, v, ref


def _check_sharp(case, bi, flags=()):
    """coverage, regime, and every mutation beyond the bar"""
    hd = ac.head_dims(case[0])[0]
    pl, q, k, v, ref = _check_emulation(case, "sharp", bi, flags)
    assert float(ref.cover.min()) >= 0.25, (case, bi, float(ref.cover.min()), int(ref.cover.argmin()))
    sh, p = ac.params(case[0], "sharp")
    pre = "blocks.0." + ("temporal_block" if bi else "spatial_block") + ".norm."
    got = ac.regime(pl, q, k, p[pre + "query_norm.scale"], p[pre + "key_norm.scale"], ac.premul_of(sh), hd)
    assert got == ac.intended_regime(pl, "sharp"), (case, bi, got)
    for name, kw in ac.mutations(pl).items():
        _, of_bar = ac.worst(ac.emulate(q, k, v, pl.form, **kw), ref, pl.form, pl.S, hd)
        assert of_bar > 1.0, (case, bi, name, of_bar)
    return pl


@pytest.mark.parametrize("case", ALL_SOFTMAX, ids=ac.case_id)
def test_emulated_roundings_within_the_bar_and_mutations_beyond_it(case):
    for bi in (0, 1):
        _check_emulation(case, "unit", bi)
        pl = _check_sharp(case, bi)
        assert "neighbour_row" in ac.mutations(pl) or pl.S == 1
        assert ("key_256_dropped" in ac.mutations(pl)) == (pl.S > 256) and ("mask_shifted_one_block" in ac.mutations(pl)) == (pl.form == "grouped")


@pytest.mark.parametrize("arm,case", FALLBACK, ids=lambda x: x if isinstance(x, str) else ac.case_id(x))
def test_fallback_arm_cases_on_the_cpu(arm, case):
    flags = tuple(sorted(ac.arm_flags(arm).items()))
    for bi in (0, 1):
        _check_emulation(case, "unit", bi, flags)
        _check_sharp(case, bi, flags)


@pytest.mark.parametrize("case", ac.LINEAR_CASES, ids=ac.case_id)
def test_linear_mode_emulation_within_the_bar(case):
    hd = ac.head_dims(case[0])[0]
    for bi in (0, 1):
        pl, q, k, v, ref = _axis(case, "unit", bi, True)
        ua, of_bar = ac.worst(ac.emulate_linear(q, k, v), ref, "linear", pl.S, hd)
        print(f"EMULATED {ac.case_id(case)}.{bi}.linear worst {ua:.2f} uA, {of_bar:.2f} of the bar")
        assert of_bar <= 1.0, (case, bi, ua, of_bar)
        # a position left out of the context moves the result beyond the bar
        if pl.S >= 2:
            cut = ac.linear_reference(q, k[:, :, :-1], v[:, :, :-1])
            assert ac.worst(cut.o, ref, "linear", pl.S, hd)[1] > 1.0


@pytest.mark.parametrize("case,bi,mixed", ac.REGIME_CASES, ids=lambda x: ac.case_id(x) if isinstance(x, tuple) else str(x))
def test_regime_arms_reach_the_intended_softmax_path(case, bi, mixed):
    hd = ac.head_dims(case[0])[0]
    for arm in ac.regime_arms(mixed):
        pl, q, k, v, ref = _check_emulation(case, arm, bi)
        sh, p = ac.params(case[0], arm)
        pre = "blocks.0." + ("temporal_block" if bi else "spatial_block") + ".norm."
        got = ac.regime(pl, q, k, p[pre + "query_norm.scale"], p[pre + "key_norm.scale"], ac.premul_of(sh), hd)
        assert got == ac.intended_regime(pl, arm), (case, bi, arm, got)
