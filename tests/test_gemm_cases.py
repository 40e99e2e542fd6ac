"""The machinery of the per-element GEMM tests (gemm_cases.py), on the CPU, before test_hip_gemm.py relies on it on the MI355X: the case
table's forms follow the restated launch rules at 256 CUs and reach every form, tile, range, segment and table edge; the tilings the
product rule can answer are enumerated; the fp64 references, fed the oracle's own intermediates, reproduce the oracle's taps to fp64
rounding (geometry, padding, positions on both axes, the pre-multiplier); a torch emulation of each kernel family's roundings stays
inside the bars; and each mutation of that emulation - a dropped k-step, a missing bias tile, the neighbour's gate row or residual row,
a rotation one position on, swapped norm scales, a missing pre-multiplier, a dropped mlp block of the tail, an unwritten last tile -
lands outside them.  The k-step, gate and unwritten-tile mutations sit in the last block of 32 tokens (the one a ragged launch gets wrong);
the residual mutation moves every row by one token, the rotation one token only.  Every one of them moves its elements by 16 / K of S, a
bias, a gate row or a whole update - three orders of magnitude above the bars - so a single row of the same slip is caught as well."""
import functools

import pytest
import torch

import attention_cases as ac
import gemm_cases as gc
from oracle import latent_net

EMULATE_MAX_N = 1400  # cases up to this many tokens are emulated; the larger ones repeat their forms' arithmetic on more rows
MUTATE_MAX_N = 700


def _plans():
    return [(c, gc.plan(c)) for c in gc.CASES]


def test_table_forms_follow_the_restated_rules_and_every_form_is_reached():
    plans = _plans()
    for c, p in plans:
        assert (p.lin1, p.lin2[0]) == c[5:], (gc.case_id(c), p.lin1, p.lin2)
        assert gc.handle_flags(c[4])[0] in ("plain", "tail", "lnf")
    n_of, tpt_of = gc.n_tokens, lambda c: c[2] * c[3]
    shared = lambda c: gc.handle_flags(c[4])[1]  # noqa: E731

    # LayerNorm + modulate: both kernels at every hidden size, n = 1, 3, 4, 5, one n above the persistent grid, trajectories of 1 and 3
    # tokens (3: a boundary inside a workgroup's four tokens), both strides
    ln = {}
    for c, _ in plans:
        kern, grid = gc.ln_form(gc.dims(c[0]).D, n_of(c))
        ln.setdefault(kern, []).append((gc.dims(c[0]).D, n_of(c), tpt_of(c), shared(c), grid))
    assert {D for D, *_ in ln["k_ln_modulate_v4"]} == {256, 512} and {D for D, *_ in ln["k_ln_modulate"]} == {64, 128, 192, 320, 384, 448}
    for kern, rows in ln.items():
        assert {1, 3, 4, 5} <= {n for _, n, *_ in rows}, kern
        assert {1, 3} <= {t for _, n, t, _, _ in rows if n > t}, kern
        assert {s for _, _, _, s, _ in rows} == {False, True}, kern
    assert any(4 * g < n for _, n, _, _, g in ln["k_ln_modulate_v4"])  # a wave walks more than one token

    # k_linear1_ts: the eight instances at 8 waves, hidden 512 at 4 waves on either side of 10 240 tokens, the q | k | v launch
    labels = {p.lin1 for _, p in plans}
    assert {"k_linear1_ts<%d, %d, 8>" % (w, D) for w in (16, 32) for D in (128, 256, 384, 512)} <= labels
    assert {"k_linear1_ts<32, 256, 8> (q | k | v)", "k_linear1_ts<16, 256, 8> (q | k | v)", "k_linear1_ts<32, 512, 4>", "k_linear1_ts<16, 512, 4>"} <= labels
    n512 = {(n_of(c), p.waves) for c, p in plans if p.lin1_ts and gc.dims(c[0]).D == 512}
    assert {(10240, 4), (10241, 8)} <= n512
    ts = [(c, p) for c, p in plans if p.lin1_ts]
    for TT in (256, 128):
        assert {1, TT - 1, TT, TT + 1} <= {n_of(c) for c, p in ts if p.split.TT == TT}, TT
        assert any(n_of(c) > TT and n_of(c) % TT not in (0, 1, TT - 1) for c, p in ts if p.split.TT == TT)  # a ragged last tile
    assert any(p.split.ntile == 1 and p.split.wpt == p.split.NB // 2 for _, p in ts)  # wpt at its cap
    starts = set()
    for c, p in ts:
        if 2 <= p.split.wpt < p.split.NB // 2:
            starts |= {min(3, 32 * (i0 % p.split.NB) // gc.dims(c[0]).HHD) for i0, _ in p.split.ranges}
    assert starts == {0, 1, 2, 3}  # a segment starts inside each of q, k, v, mlp
    even = [(c, p) for c, p in ts if p.split.wpt == 0]
    assert {gc.dims(c[0]).D for c, _ in even} >= {128, 512}
    for c, p in even:
        assert n_of(c) > 32768 and any(i0 // p.split.NB != (i1 - 1) // p.split.NB for i0, i1 in p.split.ranges), gc.case_id(c)
    assert {p.planes for _, p in ts} == {False, True}

    # linear1 on the tile GEMM: hidden 64, 192, 320, 448; tilings 5, 10, 11; n = 1 and either side of the token tile
    g1 = [(c, p) for c, p in plans if not p.lin1_ts]
    assert {gc.dims(c[0]).D for c, _ in g1} == {64, 192, 320, 448} and {p.gemm1 for _, p in g1} == {5, 10, 11}
    for t in (10, 11):
        assert {1, 127, 128, 129} <= {n_of(c) for c, p in g1 if p.gemm1 == t}, t
    assert {0, 1, 255} <= {n_of(c) % 256 for c, p in g1 if p.gemm1 == 5}
    assert {gc.dims(c[0]).D for c, p in g1 if p.gemm1 == 5} == {64, 192, 320, 448}  # K = 64: one k-tile for two slots; 448: seven
    assert any(gc.dims(c[0]).F1 % gc.GEMM_TILE[p.gemm1][0] for c, p in g1 if p.gemm1 == 5) and any(gc.dims(c[0]).F1 % 128 for c, p in g1 if p.gemm1 == 11)

    # k_linear2_ws: every instance with its slice count, the block counts, the token-range shapes, the gate rows
    ws = [(c, p) for c, p in plans if p.lin2_kind == "ws"]
    assert {(gc.dims(c[0]).K2, p.grid2.slices) for c, p in ws} == {(384, 1), (768, 2), (1280, 3), (1536, 4)}
    for K2 in (384, 768, 1280, 1536):
        assert {1, 31, 32, 33} <= {n_of(c) for c, _ in ws if gc.dims(c[0]).K2 == K2}, K2
    assert {7, 8, 9} <= {(n_of(c) + 31) // 32 for c, _ in ws}
    sizes = [set(p.grid2.ranges) for _, p in ws]
    assert {0, 1} in sizes and {1} in sizes and {2} in sizes and {3} in sizes and {2, 3} in sizes and {1, 2} in sizes
    assert any(n_of(c) % 32 for c, _ in ws) and any(n_of(c) % 32 == 0 for c, _ in ws)
    assert {1, 3} <= {tpt_of(c) for c, _ in ws if not shared(c) and n_of(c) > tpt_of(c)} and any(tpt_of(c) >= 4096 for c, _ in ws)
    assert {shared(c) for c, _ in ws} == {False, True}
    assert any(p.grid2.gate_rows == 1 for _, p in ws) and any(p.grid2.gate_rows > 64 for _, p in ws)
    # both sides of the gate-table limit: the same model, the same tokens per trajectory, the tile GEMM beyond
    over = {(c[0], tpt_of(c)) for c, p in plans if p.lin2_kind == "gemm" and gc.linear2_ws_shape_ok(gc.dims(c[0]).D, gc.dims(c[0]).K2) and c[4] == "plain"}
    under = {(c[0], tpt_of(c)) for c, p in ws if c[4] == "plain"}
    assert {("d256h8r2", 1), ("d512h16r2", 3)} <= over & under
    assert {p.lin2[0] for c, p in plans if c[4].startswith("lnf")} == {"k_linear2_ws<%d> (+ row statistics)" % k for k in (384, 768, 1280, 1536)}
    assert all(p.lin2[1] == "k_linear2_ws<%d>" % gc.dims(c[0]).K2 for c, p in plans if c[4].startswith("lnf"))

    # linear2 on the tile GEMM: 7, 11, 15, 28, each threshold from both sides, 28 on 192- and 384-wide models
    g2 = [(c, p) for c, p in plans if p.lin2_kind == "gemm"]
    assert {p.gemm2 for _, p in g2} == {7, 11, 15, 28}
    by = {(c[0], n_of(c)): p.gemm2 for c, p in g2}
    for model, n, t in (("d512h16r1", 16384, 7), ("d448h16r1", 16384, 15), ("d192h8r1", 16256, 28), ("d384h16r1", 8064, 28)):
        assert by[model, n] == 11 and by[model, n + 1] == t, (model, n)
    assert {127, 128, 129} <= {n_of(c) for c, _ in g2}

    # k_tail: M = 64, 128, 512, 1024; n = 1, 31, 32, 33; more than one wave tile per workgroup; both strides
    tl = [(c, p) for c, p in plans if p.lin2_kind == "tail"]
    assert {gc.dims(c[0]).Mp for c, _ in tl} == {64, 128, 512, 1024} and {1, 31, 32, 33} <= {n_of(c) for c, _ in tl}
    assert any((n_of(c) + 31) // 32 > gc.tail_grid(n_of(c)) for c, _ in tl) and {shared(c) for c, _ in tl} == {False, True}
    assert all(p.lin1.endswith("(q | k | v)") for _, p in tl)


def test_gate_rows_and_lds_needs_of_the_restated_configs():
    assert [gc.linear2_ws_max_gate_rows(k) for k in (1536, 1280, 768, 384)] == [28, 59, 124, 172]
    assert gc.lin1_lds(512, 3584) <= gc.LDS_BUDGET < gc.lin1_lds(512, 3584) + 32768
    assert gc.tail_shape_ok(256, 256, 64) and gc.tail_shape_ok(256, 256, 1024) and not gc.tail_shape_ok(256, 256, 96) and not gc.tail_shape_ok(512, 512, 1024)
    assert gc.linear2_ws_grid(256, 7 * 32, 3, False).rpx == 1 and gc.linear2_ws_grid(256, 16 * 32, 3, False).rpx == 2
    assert gc.linear2_ws_grid(512, 10 ** 6, 3, False).rpx == 8 and gc.linear2_ws_grid(128, 10 ** 6, 3, True).gate_rows == 1


def test_tilings_the_product_rule_can_answer():
    """Every model make_dims can produce at hidden 64 .. 512 (16- or 32-wide padded heads, mlp widths up to 5 x hidden) at every token count
    that matters to the rule: linear1 on the tile GEMM answers 5, 10 and 11 - never 12, whose K % 128 == 0 models are all token-stationary
    instances - and linear2 on it 7, 11, 15 and 28."""
    lin1, lin2, ts_hidden = set(), set(), set()
    counts = sorted({1, 128, 129} | {256 * t + r for t in (32, 40, 64, 80, 128, 160, 320, 400) for r in (0, 1)})
    for D in range(64, 513, 64):
        for H in (h for h in range(1, 65) if D % h == 0 and D // h <= 32 and (D // h) % 2 == 0):
            hdp = 16 if D // H <= 16 else 32
            for M in range(32, 5 * D + 1, 32):
                Mp = M + 32 if (H * hdp + M) % 64 else M
                F1, K2 = 3 * H * hdp + Mp, H * hdp + Mp
                for n in counts:
                    if gc.linear1_ts_ok(hdp, D, F1, H * hdp, n):
                        ts_hidden.add(D)
                    else:
                        assert D % 128 != 0 or (H * hdp) % 64 != 0 or gc.lin1_lds(D, F1) > gc.LDS_BUDGET, (D, H, M)
                        lin1.add(gc.gemm_variant(False, F1, D, n))
                    lin2.add(gc.gemm_variant(True, D, K2, n))
    assert ts_hidden == {128, 256, 384, 512}
    assert lin1 == {5, 10, 11} and lin2 == {7, 11, 15, 28}
    for m in gc.MODELS:
        d = gc.dims(m)
        assert d.D % 128 != 0 or gc.linear1_ts_ok(d.hdp, d.D, d.F1, d.HHD, 1), m


# ---- the references against the oracle ----------------------------------------------------------------------------------------------------
def _rows(x, B, T, L, temporal):
    """[G, S, F] of the oracle's axis layout -> token-major [n, F]"""
    if not temporal:
        return x.reshape(B * T * L, -1)
    return x.reshape(B, L, T, -1).permute(0, 2, 1, 3).reshape(B * T * L, -1)


def _qk_formulas_in_fp64(x, scale, cos, sin):
    """latent_net.head_rms and rotate_pairs without their casts to fp32 (the oracle forms the statistics and the rotation in fp32
    whatever dtype it runs in, as the reference does): x [G, H, S, hd] fp64."""
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * scale
    y0, y1 = y[..., 0::2], y[..., 1::2]
    return torch.stack([cos * y0 - sin * y1, sin * y0 + cos * y1], -1).reshape(x.shape)


ORACLE_CASES = tuple({c[:4]: c for c in gc.CASES if gc.n_tokens(c) <= 300 and c[4] in ("plain", "tail")}.values())


@pytest.mark.parametrize("case", ORACLE_CASES, ids=gc.case_id)
def test_references_reproduce_the_oracles_taps_in_fp64(case):
    model, B, T, L = case[:4]
    d = gc.dims(model)
    sh, p = gc.params(model)
    p64 = latent_net.cast_params(p, torch.float64)
    h, mods = gc.inputs(model, B, T, L)
    h64 = h.double()
    D = d.D
    for bi in (0, 1):
        traj, pos = gc.token_geometry(B, T, L, bi)
        shift, scale, gate = gc.mod_rows(mods, bi, D, traj)
        n_pos = T if bi else L
        u = latent_net.layer_norm(h64, 1e-6) * (1 + scale.reshape(B, T, L, D)) + shift.reshape(B, T, L, D)
        cs, sn = latent_net.rope_cos_sin(n_pos, sh.head_dim, sh.theta)
        taps = {}
        seq = u.permute(0, 2, 1, 3).reshape(B * L, T, D) if bi else u.reshape(B * T, L, D)
        latent_net.attn_mlp_block(p64, gc.BLOCK_NAMES[bi], seq, cs.double(), sn.double(), sh, taps)
        want_out = h64.reshape(-1, D) + gate * _rows(taps["out"], B, T, L, bi)
        pk = gc.packed(model, bi)

        def close(got, want, what, bar=1e-12):
            err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
            assert err < bar, (gc.case_id(case), bi, what, err)

        a = gc.a_reference(h64.reshape(-1, D), shift, scale)["a"][0]
        close(a, u.reshape(-1, D), "a")
        cos, sin = gc.rope_table(model, n_pos)
        ref = gc.linear1_reference(a, pk, model, pos, cos, sin)
        zt = _rows(taps["z"], B, T, L, bi)
        # q_rope, k_rope: the oracle's taps have passed through fp32 inside head_rms and rotate_pairs (four roundings of 2^-24 and the
        # cancellation of the rotation: 1e-6 of the largest element); the same two formulas kept in fp64 on the oracle's z: 1e-12
        G, S = taps["z"].shape[:2]
        for i, (name, tap) in enumerate((("q", "q_rope"), ("k", "k_rope"))):
            pre = gc.premul_of(model) if i == 0 else 1.0
            x = taps["z"][..., i * D:(i + 1) * D].reshape(G, S, d.H, d.hd).permute(0, 2, 1, 3)
            sc = p64[gc.BLOCK_NAMES[bi] + (".norm.query_norm.scale" if i == 0 else ".norm.key_norm.scale")]
            close(ref[name][0], ac.token_rows(_qk_formulas_in_fp64(x, sc, cs.double(), sn.double()), B, T, L, bi) * pre, name)
            close(ref[name][0], ac.token_rows(taps[tap], B, T, L, bi) * pre, name + " (the tap)", 1e-6)
        close(ref["v"][0], zt[:, 2 * D:3 * D].reshape(-1, d.H, d.hd), "v")
        close(ref["gelu"][0][:, :d.M], latent_net.gelu_erf(zt[:, 3 * D:]), "gelu")
        assert float(ref["gelu"][0][:, d.M:].abs().max()) == 0.0 if d.Mp > d.M else True
        z_attn = gc.pad_heads(_rows(taps["attn"], B, T, L, bi).reshape(-1, d.H, d.hd), model)
        z = torch.cat([z_attn, ref["gelu"][0]], -1)
        close(gc.linear2_reference(h64.reshape(-1, D), z, gate, pk, model)["h_out"][0], want_out, "h_out")
        if case[4] == "tail":
            close(gc.tail_reference(h64.reshape(-1, D), a, z_attn, gate, pk, model)["h_out"][0], want_out, "h_out (tail)")


# ---- the emulated roundings inside the bars, the mutations outside ---------------------------------------------------------------------------
EMULATED = tuple(c for c in gc.CASES if gc.n_tokens(c) <= EMULATE_MAX_N and not c[4].startswith("lnf"))


def _inside(tag, got, ref_bar):
    w, i = gc.worst(got, ref_bar)
    assert w <= 1.0, (tag, w, i)
    return w


def _outside(tag, got, ref_bar):
    w, _ = gc.worst(got, ref_bar)
    assert w > 1.0, (tag, "the mutation stays inside the bar", w)


@functools.lru_cache(maxsize=2)
def _operands(case, bi):
    model, B, T, L, handle = case[:5]
    d = gc.dims(model)
    h, mods = gc.inputs(model, B, T, L, gc.handle_flags(handle)[1])
    traj, pos = gc.token_geometry(B, T, L, bi)
    shift, scale, gate = gc.mod_rows(mods, bi, d.D, traj)
    cos, sin = gc.rope_table(model, T if bi else L)
    return h.reshape(-1, d.D), shift, scale, gate, pos, cos, sin, gc.packed(model, bi)


@pytest.mark.parametrize("case", EMULATED, ids=gc.case_id)
def test_emulated_roundings_inside_the_bars_and_mutations_outside(case):
    model, B, T, L, handle = case[:5]
    d = gc.dims(model)
    kind, shared = gc.handle_flags(handle)
    n, tpt = B * T * L, T * L
    mutate = n <= MUTATE_MAX_N
    last = (n - 1) // 32  # the last block of 32 tokens
    for bi in (0, 1):
        tag = f"{gc.case_id(case)}.{bi}"
        h, shift, scale, gate, pos, cos, sin, pk = _operands(case, bi)
        a = gc.emulate_a(h, shift, scale)
        worst = {"a": _inside(tag + ".a", a, gc.a_reference(h.double(), shift, scale)["a"])}
        ref1 = gc.linear1_reference(a.double(), pk, model, pos, cos, sin)
        emu1 = gc.emulate_linear1(a, pk, model, pos, cos, sin)
        for k in ("q", "k", "v", "gelu"):
            worst[k] = _inside(f"{tag}.{k}", emu1[k], ref1[k])
        z_attn = gc.pad_heads(emu1["v"], model)  # (any bf16 rows serve as the tapped attention output)
        z = torch.cat([z_attn, emu1["gelu"]], -1)
        if kind == "tail":
            ref2 = gc.tail_reference(h.double(), a.double(), z_attn.double(), gate, pk, model, with_linear2_bar=True)
            emu2 = lambda **kw: gc.emulate_tail(h, a, z_attn, gate, pk, model, **kw)  # noqa: E731
            ratio = float((ref2["h_out"][1] / ref2["linear2_bar"][1]).median())
            print(f"TAIL BAR {tag} M = {d.Mp}: median of the tail bar / the linear2 bar = {ratio:.1f}")
        else:
            ref2 = gc.linear2_reference(h.double(), z.double(), gate, pk, model)
            emu2 = lambda **kw: gc.emulate_linear2(h, z, gate, pk, model, **kw)  # noqa: E731
        worst["h_out"] = _inside(tag + ".h_out", emu2(), ref2["h_out"])
        print("EMULATED " + tag + " " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " of the bar")
        if not mutate:
            continue
        # one 16-deep k-step dropped in one 32 x 32 tile, the bias omitted on one feature tile: a tile inside every section
        ks1, ks2 = d.D // 16 - 1, d.K2 // 16 // 2
        for k, ft in (("q", 0), ("k", d.HHD // 32), ("v", 2 * d.HHD // 32 + (d.HHD // 32 - 1)), ("gelu", 3 * d.HHD // 32)):
            _outside(f"{tag}.{k}.k_step_dropped", gc.emulate_linear1(a, pk, model, pos, cos, sin, drop=(last, ft, ks1))[k], ref1[k])
            _outside(f"{tag}.{k}.bias_omitted", gc.emulate_linear1(a, pk, model, pos, cos, sin, no_bias_tile=ft)[k], ref1[k])
        _outside(tag + ".h_out.k_step_dropped", emu2(drop=(last, d.D // 32 - 1, ks2)), ref2["h_out"])
        _outside(tag + ".h_out.bias_omitted", emu2(no_bias_tile=0), ref2["h_out"])
        if not shared and B > 1:
            _outside(tag + ".h_out.gate_of_the_next_trajectory", emu2(gate_block=(last if n - 32 * last > 0 else 0, tpt)), ref2["h_out"])
        if n > 1:
            _outside(tag + ".h_out.residual_of_the_next_token", emu2(residual_next=True), ref2["h_out"])
        if cos.shape[0] > 1:
            for k in ("q", "k"):
                _outside(f"{tag}.{k}.position_plus_one", gc.emulate_linear1(a, pk, model, pos, cos, sin, pos_shift_token=n - 1)[k], ref1[k])
        sw = gc.emulate_linear1(a, pk, model, pos, cos, sin, swap_scales=True)
        _outside(tag + ".q.scales_swapped", sw["q"], ref1["q"])
        _outside(tag + ".k.scales_swapped", sw["k"], ref1["k"])
        _outside(tag + ".q.premul_omitted", gc.emulate_linear1(a, pk, model, pos, cos, sin, premul=False)["q"], ref1["q"])
        un = gc.emulate_linear1(a, pk, model, pos, cos, sin, untouched_from=32 * last)
        for k in ("q", "k", "v", "gelu"):
            _outside(f"{tag}.{k}.last_tile_untouched", un[k], ref1[k])
        _outside(tag + ".h_out.last_tile_untouched", emu2(untouched_from=32 * last), ref2["h_out"])
        if kind == "tail":
            _outside(tag + ".h_out.mlp_block_dropped", emu2(drop_mlp_block=d.Mp // 32 - 1), ref2["h_out"])


def test_every_family_is_emulated_and_mutated_at_its_smallest_and_at_a_mid_sized_case():
    fam = {}
    for c in EMULATED:
        p = gc.plan(c)
        for f in (p.lin1.split("<")[0] + ("" if p.lin1_ts else "<EpiLinear1>"), p.lin2[0].split(" ")[0].split("<")[0] + ("<EpiLinear2>" if p.lin2_kind == "gemm" else "")):
            fam.setdefault(f, []).append(gc.n_tokens(c))
    assert set(fam) == {"k_linear1_ts", "k_gemm_glds<EpiLinear1>", "k_linear2_ws", "k_gemm_glds<EpiLinear2>", "k_tail"}
    for f, ns in fam.items():
        assert min(ns) == 1 and any(64 < n <= MUTATE_MAX_N for n in ns), (f, sorted(ns))
