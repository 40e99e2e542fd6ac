"""The machinery of the per-element tests of the fp32 frame (frame_cases.py), on the CPU, before test_hip_frame.py relies on it on the
MI355X: the case tables reach every launch form, tile edge, route and record variant the restated rules can produce at 256 CUs; the
workgroup-to-tile maps of the multi-tile head cases give the sequences the table names; the fp64 references, fed the oracle's inputs,
reproduce the oracle's own taps; one fp32 emulation of each kernel family's summation order stays inside the bars; and every mutation of
those emulations - a dropped k-step, a missing bias, the neighbour's modulation row in a straddling tile, a stale shift / scale after a
trajectory change, an unwritten last slab at 33 channels, the other mask_emb row, the add row taken modulo the wrong count, a stale staged
input tile for features >= 256 (the defect k_embed had at hidden 320 / 384 / 448 with 97 - 127 inputs no multiple of 8) - lands outside
them, each placed in the last ragged tile or at the edge it belongs to.  The emulations run the launch rules at a small CU count, so that
a few hundred tokens give a workgroup several tiles."""
import pytest
import torch

import frame_cases as fc
from oracle import latent_net


# ---- reach --------------------------------------------------------------------------------------------------------------------------------
def test_dense_table_reaches_every_route_pair_and_edge():
    mods = [c for c in fc.DENSE_CASES if c[0] == "mods"]
    seen = {}
    for _, D, V, rows, single in mods:
        for name, (form, pre, post, I) in fc.mods_chain(D, rows, single, V).items():
            seen.setdefault((form.kernel, pre, post), []).append((I, rows, single, name))
    # every route with every PRE / POST pair the chain uses: the single row and the MFMA and tiled routes all three; the rows route away
    # from the single row is reached by vec_in's first layer only (an input width that is no multiple of 4)
    for kern in ("k_dense_rows", "k_dense_mfma", "k_dense_tiled"):
        assert {(kern, 0, 1), (kern, 0, 0), (kern, 1, 0)} <= set(seen), kern
    assert all(s for _, _, s, _ in seen["k_dense_rows", 0, 0]) and any(not s and I in (3, 5) for I, _, s, _ in seen["k_dense_rows", 0, 1])
    assert {D for _, D, _, r, s in mods if s and r == 1} == set(fc.HIDDEN)
    for kern in ("k_dense_mfma", "k_dense_tiled"):
        for pair in ((0, 0), (1, 0)):
            assert {1, 2, 31, 32, 33, 64, 65} <= {r for _, r, _, _ in seen[(kern,) + pair]}, (kern, pair)
    assert {I for I, *_ in seen["k_dense_mfma", 0, 0]} == {128, 256} and {I for I, *_ in seen["k_dense_mfma", 1, 0]} == {128, 256}
    assert {I for I, *_ in seen["k_dense_mfma", 0, 1]} == {128, 256}  # (first layer: 256; vec_in at 128 and 256 inputs)
    assert {I for I, *_ in seen["k_dense_tiled", 0, 0]} == {64, 192, 320, 384, 448, 512}
    assert {I for I, *_ in seen["k_dense_tiled", 0, 1]} == {12, 24}
    assert {V for _, _, V, _, _ in mods if V} == {128, 256, 12, 24, 3, 5}
    steps = [c for c in fc.DENSE_CASES if c[0] == "steps"]
    assert {1, 7, 8, 9, 16, 17, 48, 49, 50} <= {c[2] for c in steps}
    launches = {fc.steps_ranges(c[2])[0] for c in steps}
    assert launches == {1, 2}  # the 48-step chunk of k_time_features_steps and one behind it
    assert fc.steps_ranges(17) == (1, [6, 6, 5], [9, 8]) and fc.steps_ranges(50)[1] == [8] * 6 + [2] and fc.steps_ranges(8)[1:] == ([8], [8])
    for c in fc.DENSE_CASES:  # the labels are the restated rule's
        if c[0] == "mods":
            assert fc.mods_label(c[1], c[3], c[4], c[2]).count(" > ") == (4 if c[2] else 3)


def test_embed_table_reaches_every_form_tile_size_and_dq_class():
    forms = {}
    for C, D, n, handle in fc.EMBED_CASES:
        for mode in (0, 1):
            f = fc.embed_form(mode, C, D, n, handle == "lnf")
            key = ("mfma", f.ck) if f.kind == "mfma" else ("reg", f.cmax, f.nd, "lds" if f.w_lds else "scalar" if C & 3 else "vec")
            forms.setdefault(key, []).append((C, D, n, handle, mode, f))
    want = {("mfma", ck) for ck in range(5, 17)} | {("reg", 32, 4, k) for k in ("scalar", "vec", "lds")} | {("reg", 64, 2, "vec"), ("reg", 96, 2, "vec"),
                                                                                                         ("reg", 128, 1, "vec")}
    assert want <= set(forms), want - set(forms)
    for key, rows in forms.items():
        assert {1, 31, 32, 33} <= {n for _, _, n, *_ in rows}, key
        assert {0, 1} == {m for *_, m, _ in rows}, key
    ins = {C for C, *_ in fc.EMBED_CASES}
    assert {1, 3, 6, 4, 8, 28, 32, 36, 60, 68, 92, 100, 124} <= ins
    assert {D for C, D, *_ in fc.EMBED_CASES if C in (100, 124)} >= {64, 256, 320, 384, 448, 512}
    for ck in range(5, 17):  # a feature-tile count the three-tile groups do not divide, on more than one token tile
        assert any(D // 32 % 3 and n > 32 for _, D, n, *_ in forms["mfma", ck]), ck
    # the LDS form: 16 -> 32 -> 64-token tiles, n on either side of each change; a workgroup that walks two tiles with a ragged last one
    lds = {n: f for _, _, n, _, m, f in forms["reg", 32, 4, "lds"] if m == 1}
    assert (lds[fc.EMB_T16_MAX].tok, lds[fc.EMB_T16_MAX + 1].tok, lds[fc.EMB_T32_MAX].tok, lds[fc.EMB_T32_MAX + 1].tok) == (16, 32, 32, 64)
    assert lds[fc.EMB_MULTI].tok == 64 and lds[fc.EMB_MULTI].tiles_per_wg == 2 and fc.EMB_MULTI % 64 not in (0, 63)
    assert fc.EMB_MULTI > 64 * 2 * fc.CUS
    # every register form at every DQ class it has, with more tiles than workgroups
    classes = {}
    for key, rows in forms.items():
        if key[0] == "reg":
            for _, D, n, _, _, f in rows:
                if f.tiles > f.grid:
                    classes.setdefault(key[1:3], set()).add(fc.dq_class(f.dq))
    assert classes[32, 4] >= {"div", "nodiv"} and classes[64, 2] >= {"div", "nodiv", "eq"} and classes[96, 2] >= {"div", "nodiv", "eq"}
    assert classes[128, 1] == {"div", "nodiv", "eq", "between", "two"}
    between = {D for C, D, n, *_ in fc.EMBED_CASES if C in (100, 124) and n == fc.EMB_MULTI and fc.dq_class(D) == "between"}
    assert between == {320, 384, 448}
    # normalize at every <NE, VEC>, with a partial workgroup of four waves; ln_fuse at 256 and 512 with and without the LDS path
    assert {D for _, D, _, h in fc.EMBED_CASES if h == "norm"} == set(fc.HIDDEN)
    assert {1, 3, 4, 5} <= {n for _, _, n, h in fc.EMBED_CASES if h == "norm"}
    lnf = {(C == 32, D) for C, D, _, h in fc.EMBED_CASES if h == "lnf"}
    assert lnf == {(False, 256), (True, 256), (True, 512), (False, 512)}
    assert all(C <= 32 and D in (256, 512) for C, D, _, h in fc.EMBED_CASES if h == "lnf")
    assert any(n == fc.EMB_MULTI for *_, n, h in fc.EMBED_CASES if h == "lnf")
    m = fc.mask_of(200)
    assert set(m.tolist()) == {0, 1} and m[63] != m[74] and int(m[32]) == 0 and int(m[37]) == 1  # runs of 37 cross the 16 / 32 / 64-token edges


def test_head_table_reaches_every_form_slab_count_and_sequence():
    forms = [(c, fc.head_form(c[0], c[1], fc.head_n(c))) for c in fc.HEAD_CASES]
    assert {(f.ne, f.vec) for _, f in forms} == {(1, 1), (2, 2), (3, 1), (4, 2), (5, 1), (6, 2), (7, 1), (8, 2)}
    assert {c[1] for c, _ in forms} == set(fc.HEAD_CHANNELS) == {1, 3, 4, 31, 32, 33, 64, 96, 100}
    for D in fc.HIDDEN:
        assert {1, 31, 32, 33} <= {fc.head_n(c) for c, _ in forms if c[0] == D}, D
    assert {f.per_cu for _, f in forms} == {1, 2} and {f.one_slab for _, f in forms} == {True, False}
    assert {c[4] for c, _ in forms} == {"B", "1"}
    assert any(f.ne == 1 and f.one_slab for _, f in forms)  # hidden 64: the partial products are larger than the rows they overlay
    kinds = set()
    for name, (case, wg, want) in fc.HEAD_SEQ.items():
        assert case in fc.HEAD_CASES
        f = fc.head_form(case[0], case[1], fc.head_n(case))
        assert f.tiles > 2 * f.grid and fc.head_n(case) > 2 * 32 * f.grid, name  # three tiles per workgroup
        walk = fc.head_walk(f, wg, fc.head_n(case), case[3], case[4] == "1")
        assert walk == want, (name, walk)
        kinds.add((f.one_slab, f.per_cu))
        assert fc.head_n(case) % 32, name  # a ragged last tile
        assert 30000 < fc.head_n(case) * max(1, 3 - f.per_cu) < 70000, name
    assert kinds == {(True, 2), (False, 1), (False, 2)}
    # single, straddling, single of another trajectory: the reload; single, single of the same: none; then a straddling tile and a reload behind it
    assert fc.HEAD_SEQ["reload"][2] == [("single", 0, True), ("straddle", 40, 41), ("single", 81, True)]
    assert fc.HEAD_SEQ["noreload"][2][:4] == [("single", 0, True), ("single", 0, False), ("straddle", 0, 1), ("single", 1, True)]
    # (the sequence the kernel cannot meet: a third tile in the first tile's trajectory behind a straddling one - in no workgroup of any case)
    for case, f in forms:
        n, tpt = fc.head_n(case), case[3]
        for wg in range(min(f.grid, 64)):
            w = fc.head_walk(f, wg, n, tpt, case[4] == "1")
            for i in range(2, len(w)):
                assert not (w[i - 1][0] == "straddle" and w[i][0] == "single" and w[i - 2][0] == "single" and w[i][1] == w[i - 2][1]), (case, wg)
    assert set(fc.HEAD_VARIANTS) == {"out", "aw0", "noise", "devnoise", "saved", "trace"} and fc.HEAD_RECORDS["aw0"][2] == 0.0
    assert fc.HEAD_RECORDS["saved"][3] != 0.0 and fc.HEAD_OFFSET != 0


def test_no_case_is_large():
    for c in fc.EMBED_CASES:
        assert c[2] <= 50000
    for c in fc.HEAD_CASES:
        assert fc.head_n(c) * c[0] * 4 <= 80 << 20
    assert 0 < fc.K_TRIG <= 16 and 0 < fc.K_EXP <= 16 and 0 < fc.K_RSQ <= 16


# ---- the references against the oracle ----------------------------------------------------------------------------------------------------
def test_references_reproduce_the_oracle():
    for V, normalize in ((None, False), (5, True)):
        sh, p = fc.params(6, 128, V, normalize)
        w = fc.frame_weights(p)
        g = torch.Generator().manual_seed(1)
        B, T, L = 3, 2, 5
        x, xc = torch.randn(B, T, L, 6, generator=g), torch.randn(B, T, L, 6, generator=g)
        mask = (torch.rand(B, T, L, generator=g) < 0.5).long()
        t = torch.rand(B, generator=g)
        y = torch.randn(B, V, generator=g) if V else None
        taps = {}
        p64 = latent_net.cast_params(p, torch.float64)
        out = latent_net.forward(p64, sh, x.double(), t.double(), xc.double(), mask, y.double() if V else None, taps)
        n = B * T * L
        cond, _ = fc.embed_reference(0, xc.reshape(n, 6).double(), w, mask.reshape(n))
        h, _ = fc.embed_reference(1, x.reshape(n, 6).double(), w, base=cond)
        hn = fc.ln_reference(h)[0] if normalize else h
        assert torch.allclose(hn, taps["h0"].reshape(n, 128), rtol=0, atol=1e-12)
        # the conditioning chain, each layer from the layer before
        tf, _ = fc.tfeat_reference(t.float())
        assert torch.allclose(tf, latent_net.time_features(t.float()).double(), atol=2e-6)  # (fp32 cos / sin of the same fp32 arguments)
        add = None
        if V:
            yh, _ = fc.dense_reference(y.double(), w["vec_w1"], w["vec_b1"], None, False, True)
            add, _ = fc.dense_reference(yh, w["vec_w2"], w["vec_b2"], None, False, False)
        hid, _ = fc.dense_reference(tf, w["time_w1"], w["time_b1"], None, False, True)
        vec, _ = fc.dense_reference(hid, w["time_w2"], w["time_b2"], add, False, False)
        assert torch.allclose(vec, taps["vec"], atol=2e-5)  # (the oracle's arguments are the exact products: 1e-4 of argument, attenuated)
        mods, _ = fc.dense_reference(taps["vec"], w["mod_w"], w["mod_b"], None, True, False)
        assert torch.allclose(mods[:, :6 * 128], taps["l0.mod"], atol=1e-12) and torch.allclose(mods[:, 6 * 128:], taps["final_mod"].reshape(B, -1), atol=1e-12)
        # the head on the oracle's last residual stream
        traj = torch.arange(n) // (T * L)
        shift, scale = fc.final_rows(mods, 128, traj)
        m, _ = fc.head_reference(taps["l0.h"].reshape(n, 128), shift, scale, w)
        assert torch.allclose(m, out.reshape(n, 6), atol=1e-11)
        stats, _ = fc.stats_reference(taps["l0.h"].reshape(n, 128), gsz=64)
        mean = taps["l0.h"].reshape(n, 128).mean(-1)
        assert torch.allclose(stats[:, 1], -mean * stats[:, 0], atol=1e-13)


def test_the_time_argument_is_the_two_fp32_products_not_the_exact_one():
    t = torch.rand(64, generator=torch.Generator().manual_seed(2))
    a = fc.time_args(t)
    exact = 1000.0 * t.double()[:, None] * fc.time_freqs().double()[None]
    assert float((a - exact).abs().max()) > 2e-5  # far above the bar of K_TRIG u: the reference must round as the kernel does
    assert torch.equal(a.float().double(), a)


# ---- emulations inside the bars, mutations outside ---------------------------------------------------------------------------------------
def _inside(got, ref_bar, tag):
    w, i = fc.worst(got, ref_bar)
    assert w < 1.0, (tag, w, i)
    return w


def _outside(got, ref_bar, tag):
    w, i = fc.worst(got, ref_bar)
    assert w > 4.0, (tag, w, i)


DENSE_EMU = [(I, rows, single, pre, post) for I, rows, single in ((256, 65, False), (128, 33, False), (192, 65, False), (320, 33, False), (24, 65, False),
                                                                  (12, 31, False), (5, 33, False), (3, 2, False), (256, 1, True), (448, 1, True))
             for pre, post in ((0, 1), (0, 0), (1, 0))]


@pytest.mark.parametrize("I,rows,single,pre,post", DENSE_EMU)
def test_dense_emulation_and_mutations(I, rows, single, pre, post):
    g = torch.Generator().manual_seed(7)
    O = 96
    x = torch.randn(rows, I, generator=g) * (2.0 if pre else 1.0)
    W, b = torch.randn(O, I, generator=g) / I ** 0.5, torch.randn(O, generator=g)
    add = torch.randn(rows, O, generator=g) if not (pre or post) else None
    form = fc.dense_form(I, rows, single)
    ref = fc.dense_reference(x.double(), W.double(), b.double(), add.double() if add is not None else None, pre, post)
    tag = (form, pre, post, rows)
    _inside(fc.emulate_dense(form, x, W, b, add, pre, post), ref, tag)
    tile = form.row_tile or rows
    last = (rows - 1) // tile  # the last (ragged) row tile
    _outside(fc.emulate_dense(form, x, W, b, add, pre, post, drop=(last, (I - 1) // 16)), ref, tag + ("dropped k-step",))
    _outside(fc.emulate_dense(form, x, W, b, add, pre, post, no_bias=last), ref, tag + ("missing bias",))
    if add is not None and rows > 2:
        _outside(fc.emulate_dense(form, x, W, b, add, pre, post, add_rows_wrong=rows - 1), ref, tag + ("add row % add_mod",))
        # (only the last row moves: it takes row 0's)
        got = fc.emulate_dense(form, x, W, b, add, pre, post, add_rows_wrong=rows - 1)
        assert fc.worst(got[:-1], (ref[0][:-1], ref[1][:-1]))[0] < 1.0


def test_time_feature_and_silu_bars_hold_for_torch_fp32():
    t = torch.rand(50, generator=torch.Generator().manual_seed(3))
    a = ((t * 1000.0)[:, None] * fc.time_freqs()[None])
    _inside(torch.cat([torch.cos(a), torch.sin(a)], -1), fc.tfeat_reference(t), "tfeat")
    x = torch.linspace(-30, 30, 4001)
    w, _ = fc.worst(fc._silu32(x), (fc.silu64(x.double()), fc.silu_bar(x.double())))
    assert w < 1.0, w
    # a coarser exponential (relative 2^-18) is outside
    w, _ = fc.worst(x / (1.0 + torch.exp(-x) * (1 + 2.0 ** -18)), (fc.silu64(x.double()), fc.silu_bar(x.double())))
    assert w > 1.0, w


EMBED_EMU = [(C, D, n, cus) for C, D, n, cus in ((3, 64, 150, 1), (8, 192, 150, 1), (32, 256, 70, 1), (36, 64, 150, 1), (92, 320, 150, 1), (100, 64, 150, 1),
                                               (124, 256, 150, 1), (100, 320, 200, 1), (124, 384, 330, 2), (100, 448, 200, 1), (100, 512, 150, 1),
                                               (40, 128, 97, 1), (128, 256, 130, 1), (72, 320, 33, 1))]


@pytest.mark.parametrize("C,D,n,cus", EMBED_EMU)
def test_embed_emulation_and_mutations(C, D, n, cus):
    sh, p = fc.params(C, D)
    w = fc.frame_weights(p)
    g = torch.Generator().manual_seed(7)
    x, xc, mask = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g), fc.mask_of(n)
    ref0 = fc.embed_reference(0, xc.double(), w, mask)
    f0, f1 = fc.embed_form(0, C, D, n, False, cus), fc.embed_form(1, C, D, n, False, cus)
    cond = fc.emulate_embed(0, xc, w, mask, None, f0, cus)
    _inside(cond, ref0, (C, D, "cond"))
    ref1 = fc.embed_reference(1, x.double(), w, base=cond.double())
    _inside(fc.emulate_embed(1, x, w, None, cond, f1, cus), ref1, (C, D, "state"))
    last = f0.tiles - 1
    assert n % f0.tok  # the last tile is ragged
    _outside(fc.emulate_embed(0, xc, w, mask, None, f0, cus, drop_c=(last, C - 1)), ref0, (C, D, "dropped input"))
    _outside(fc.emulate_embed(1, x, w, None, cond, f1, cus, drop_c=(last, C - 1)), ref1, (C, D, "dropped input, state"))
    _outside(fc.emulate_embed(0, xc, w, mask, None, f0, cus, no_bias=True), ref0, (C, D, "missing bias"))
    _outside(fc.emulate_embed(0, xc, w, mask, None, f0, cus, other_mask_row=last), ref0, (C, D, "other mask_emb row"))
    if f1.kind == "reg" and fc.dq_class(f1.dq) == "between":
        assert f1.tiles_per_wg >= 2
        for mode, xx, ff, rr, base in ((0, xc, f0, ref0, None), (1, x, f1, ref1, cond)):
            got = fc.emulate_embed(mode, xx, w, mask, base, ff, cus, stale_xs=True)
            _outside(got, rr, (C, D, "stale xs tile"))
            r = ((got.double() - rr[0]).abs() / rr[1]) >= 1.0
            assert not r[:, :256].any() and r[:, 256:].any()  # features below 256 are right
            lastwg = [t for wg in range(ff.grid) for t in list(range(wg, ff.tiles, ff.grid))[-1:]]
            for t in lastwg:  # a workgroup's last tile is right: a launch of one tile per workgroup never showed the defect
                assert not r[ff.tok * t:ff.tok * t + ff.tok].any()


def test_ln_and_stats_emulations_and_mutations():
    g = torch.Generator().manual_seed(7)
    for D in (64, 192, 256, 512):
        h = torch.randn(37, D, generator=g) * (0.5 + torch.rand(37, 1, generator=g)) + torch.randn(37, 1, generator=g)
        _inside(fc.emulate_ln(h, 1e-5), fc.ln_reference(h.double()), ("ln", D))
        _outside(fc.emulate_ln(h, 1e-3), fc.ln_reference(h.double()), ("ln with another eps", D))
        _outside(fc.emulate_ln(h.roll(1, 0), 1e-5), fc.ln_reference(h.double()), ("ln row", D))
        if D % 256 == 0:
            ref = fc.stats_reference(h.double())
            _inside(fc.emulate_stats(h), ref, ("stats", D))
            bad = fc.emulate_stats(h)
            bad[-1] = fc.emulate_stats(h[:, :256].repeat(1, D // 256))[-1] if D > 256 else bad[-2]
            _outside(bad, ref, ("stats of one part only", D))


HEAD_EMU = [(64, 3, 3, 23, "B", 1), (128, 33, 3, 23, "B", 1), (256, 32, 7, 40, "B", 1), (192, 100, 5, 13, "B", 1), (512, 64, 4, 50, "B", 1), (320, 4, 3, 23, "1", 1)]


@pytest.mark.parametrize("D,C,B,tpt,rows,cus", HEAD_EMU)
def test_head_emulation_and_mutations(D, C, B, tpt, rows, cus):
    case = (D, C, B, tpt, rows)
    sh, p = fc.params(C, D)
    w = fc.frame_weights(p)
    h, mods, x, noise, saved = fc.head_inputs(case)
    n = B * tpt
    shared = rows == "1"
    form = fc.head_form(D, C, n, cus)
    traj = torch.zeros(n, dtype=torch.long) if shared else torch.arange(n) // tpt
    shift, scale = fc.final_rows(mods, D, traj)
    mref = fc.head_reference(h.double(), shift, scale, w)
    tag = (D, C, n)
    _inside(fc.emulate_head(h, mods, w, C, tpt, shared, form), mref, tag + ("out",))
    last = form.tiles - 1
    assert n % 32
    _outside(fc.emulate_head(h, mods, w, C, tpt, shared, form, drop=(last, D // 8 - 1)), mref, tag + ("dropped k-step",))
    _outside(fc.emulate_head(h, mods, w, C, tpt, shared, form, no_bias=True), mref, tag + ("missing bias",))
    walks = [fc.head_walk(form, wg, n, tpt, shared) for wg in range(form.grid)]
    if not shared:
        if any(k[0] == "straddle" for wk in walks for k in wk):
            _outside(fc.emulate_head(h, mods, w, C, tpt, shared, form, neighbour_row=True), mref, tag + ("neighbour's row in a straddling tile",))
        if any(a[0] == "single" and b[0] == "single" and b[2] and a[1] != b[1] for wk in walks for a, b in zip(wk, wk[1:])) or \
                any(len(wk) > 2 and wk[-1][0] == "single" and wk[-1][2] and wk[0][0] == "single" for wk in walks):
            _outside(fc.emulate_head(h, mods, w, C, tpt, shared, form, stale=True), mref, tag + ("stale shift / scale",))
    for name, rec in fc.HEAD_RECORDS.items():
        ref = fc.step_reference(mref, x.double(), rec, noise.double(), saved.double())
        _inside(fc.emulate_head(h, mods, w, C, tpt, shared, form, rec, x, noise, saved), ref, tag + (name,))
        if C > 32:
            _outside(fc.emulate_head(h, mods, w, C, tpt, shared, form, rec, x, noise, saved, unwritten_last_slab=True), ref, tag + (name, "unwritten last slab"))
    if C == 33:  # the single channel of the second slab
        got = fc.emulate_head(h, mods, w, C, tpt, shared, form, unwritten_last_slab=True)
        r = ((got.double() - mref[0]).abs() / mref[1]) >= 1.0
        assert r[:, 32].all() and not r[:, :32].any()


def test_stale_and_neighbour_mutations_fire_on_the_table_sequence():
    """The two multi-tile mutations at a shape the GPU runs, with the workgroup map of 256 CUs: the emulation is inside the bars, a stale
    shift / scale moves the third tile of workgroup 0 (and nothing in its first), the neighbour's row moves its straddling tile."""
    case, wg, want = fc.HEAD_SEQ["reload"]
    D, C, B, tpt, _ = case
    n = fc.head_n(case)
    f = fc.head_form(D, C, n)
    sh, p = fc.params(C, D)
    w = fc.frame_weights(p)
    h, mods, *_ = fc.head_inputs(case)
    shift, scale = fc.final_rows(mods, D, torch.arange(n) // tpt)
    mref = fc.head_reference(h.double(), shift, scale, w)
    _inside(fc.emulate_head(h, mods, w, C, tpt, False, f), mref, "reload")
    t1, t2, t3 = (slice(32 * t, 32 * t + 32) for t in range(wg, f.tiles, f.grid))
    for kw, hit, clean in (({"stale": True}, t3, (t1, t2)), ({"neighbour_row": True}, t2, (t1, t3))):
        got = fc.emulate_head(h, mods, w, C, tpt, False, f, **kw)
        r = ((got.double() - mref[0]).abs() / mref[1]) >= 1.0
        assert r[hit].any() and not any(r[c].any() for c in clean), kw
