"""``lam_slide_amd.kmeans`` without a GPU: the C ABI (symbols, header, limits, every refusal before anything touches a GPU, the workspace
formula), the torch float64 restatement against the numpy oracle of tests/kmeans_oracle.py, the three ``init`` forms, and the
``post_process`` branch of ``displacement_errors`` against a line-by-line restatement of second_stage/nba.py:228-238 - with the defaults
leaving every existing result bit for bit as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kmeans_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsl_kmeans_workspace_bytes", "lsl_kmeans_step", "lsl_kmeans_nearest_rows")


# ---- the C ABI ----
def test_library_exports_header_and_limits():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib, kmeans
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s) and getattr(lib, s).argtypes is not None
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6 and "lsl_kmeans_workspace_bytes, lsl_kmeans_step, lsl_kmeans_nearest_rows added" in header
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_kmeans.hip.h")).read()
    asg = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_tica.hip.h")).read()
    macro = lambda name, text=src: int(re.search(r"#define " + name + r" (\d+)", text).group(1))  # noqa: E731
    # the centres' limits are k_assign's: k_kmeans.hip.h names them and k_tica.hip.h alone holds the numbers
    for km, own in (("LSL_KM_MAX_K", "LSL_ASG_MAX_K"), ("LSL_KM_MAX_D", "LSL_ASG_MAX_D"), ("LSL_KM_CELLS", "LSL_ASG_CELLS"), ("LSL_KM_TILE", "LSL_ASG_TILE")):
        assert re.search(r"^#define " + km + " " + own + r"\b", src, re.M), km
    assert macro("LSL_ASG_MAX_K", asg) == kmeans.MAX_K == 1024 and macro("LSL_ASG_MAX_D", asg) == kmeans.MAX_D == 64
    assert macro("LSL_ASG_CELLS", asg) == kmeans.CELLS == 8192 and macro("LSL_KM_SEG") == kmeans.SEG == orc.SEG
    assert re.search(r"^#define LSL_KM_MAX_Q \(LSL_KM_CELLS / 256\)", src, re.M) and kmeans.CELLS // 256 == 32  # the fp64 register accumulators of a thread
    assert kmeans.segments(1) == 1 and kmeans.segments(kmeans.SEG) == 1 and kmeans.segments(kmeans.SEG + 1) == 2
    # the limits live in the binding beside the others; the module's names are aliases of them
    assert (kmeans.MAX_K, kmeans.MAX_D, kmeans.CELLS, kmeans.SEG, kmeans.MAX_S) == (_lib.ASG_MAX_K, _lib.ASG_MAX_D, _lib.ASG_CELLS, _lib.KM_SEG, _lib.KM_MAX_S)
    assert macro("LSL_KM_MAX_S") == _lib.KM_MAX_S == 65535
    assert not re.search(r"atomic\w*\([^;]*(float|double)", src)  # integer atomics only


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib, kmeans
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    names = ("y", "centers", "labels", "counts", "state", "done", "ws")

    def step(S=1, n=1000, d=4, k=100, update=1, rel_tol=1e-5, center_tol=0.0, nbytes=1 << 40, **ptr):
        p = {name: ptr.get(name, one) for name in names}
        return lib.lsl_kmeans_step(p["y"], S, n, d, p["centers"], k, p["labels"], p["counts"], p["state"], p["done"], update, rel_tol, center_tol,
                                   p["ws"], nbytes, None)

    near = lambda y=one, S=1, n=60, d=2, c=one, k=20, rows=one: lib.lsl_kmeans_nearest_rows(y, S, n, d, c, k, rows, None)  # noqa: E731
    for name in names:
        assert step(**{name: None}) == -1, name
    assert near(y=None) == -1 and near(c=None) == -1 and near(rows=None) == -1 and b"null" in lib.lsl_last_error()
    refused = (dict(k=0), dict(k=1025, d=1), dict(d=0), dict(d=65), dict(k=1024, d=9), dict(k=129, d=64), dict(n=0), dict(n=-5), dict(S=0), dict(S=65536))
    for kw in refused:
        assert step(**kw) == -3, kw
        assert near(**kw) == -3, kw
    assert step(k=1025, d=1) == -3 and b"k = 1025" in lib.lsl_last_error() and b"centres" in lib.lsl_last_error()
    assert step(d=65) == -3 and b"d = 65" in lib.lsl_last_error()
    assert step(S=65536) == -3 and b"S = 65536" in lib.lsl_last_error()
    assert step(n=0) == -3 and b"n = 0" in lib.lsl_last_error()
    assert step(rel_tol=-1e-3) == -3 and b"rel_tol" in lib.lsl_last_error()
    assert step(center_tol=-1.0) == -3 and step(rel_tol=float("nan")) == -3
    assert step(nbytes=8) == -4 and b"workspace" in lib.lsl_last_error()
    assert step(k=128, d=64, nbytes=0) == -4 and step(k=1024, d=8, nbytes=0) == -4  # the cell limit itself is native
    # the workspace: per (series, segment) fp64 sums [k, d] and inertia, int32 counts [k] and the changed-label count; 0 when refused
    need = lib.lsl_kmeans_workspace_bytes
    unit = lambda d, k: 8 * (k * d + 1) + 4 * (k + 1)  # noqa: E731
    seg = kmeans.SEG
    assert need(1, seg, 4, 100) == unit(4, 100) and need(1, seg + 1, 4, 100) == 2 * unit(4, 100)
    assert need(3, 2 * seg + 17, 2, 20) == 3 * 3 * unit(2, 20) and need(11264, 60, 2, 20) == 11264 * unit(2, 20)
    assert need(1, 1, 1, 1) == unit(1, 1) and need(1, 2 ** 31 - 1, 1, 1) == kmeans.segments(2 ** 31 - 1) * unit(1, 1)
    for kw in refused:
        a = dict(S=1, n=1000, d=4, k=100)
        a.update(kw)
        assert need(a["S"], a["n"], a["d"], a["k"]) == 0, kw
    assert step(nbytes=need(1, 1000, 4, 100) - 1) == -4


# ---- the restatement against the oracle ----
CASES = ((700, 5, 3, 0), (2 * orc.SEG + 17, 8, 2, 1), (300, 12, 1, 2), (60, 20, 2, 3))  # (n, k, d, seed)


def check_fit(res, want, y, allow_ties=0):
    lab = res.labels.cpu().numpy()
    assert int((lab != want["labels"]).sum()) <= allow_ties
    assert np.array_equal(res.counts.cpu().numpy(), np.bincount(lab[lab >= 0], minlength=len(want["counts"])))
    assert int(res.n_iter) == want["n_iter"] and bool(res.converged) == want["converged"]
    c = res.centers.cpu().numpy()
    bar = orc.center_bar(y, want["labels"], want["centers"], want["counts"])
    assert (np.abs(c.astype(np.float64) - want["centers"].astype(np.float64)) <= 2 * bar).all()
    assert abs(float(res.inertia) - want["inertia"]) <= (orc.SEG + 8) * 2.0 ** -53 * want["inertia"] * 4


@pytest.mark.parametrize("n,k,d,seed", CASES)
def test_torch_restatement_matches_the_oracle(n, k, d, seed):
    from lam_slide_amd import kmeans
    y = orc.blobs(n, k, d, seed=seed, spread=1.0, sep=2.0)  # overlapping components: several iterations
    yt = torch.from_numpy(y)
    for init, tol in (("stride", 1e-5), ("stride", 0.0)):
        c0 = kmeans.initial_centers(yt[None], k, init)[0].numpy()
        assert np.array_equal(c0, y[(np.arange(k) * n) // k])
        want = orc.fit(y, c0, max_iter=100, rel_tol=tol)
        assert want["min_gap"] > 1e-9  # no near tie: another float64 evaluation has the same labels
        res = kmeans.kmeans_fit(yt, k, init=init, max_iter=100, rel_tol=tol)
        assert res.path == "torch" == kmeans.last_path["kmeans_fit"] and res.centers.shape == (k, d) and res.labels.dtype == torch.int32
        assert res.counts.dtype == torch.int64 and res.inertia.dtype == torch.float64 and res.n_iter.dtype == torch.int32 and res.converged.dtype == torch.bool
        check_fit(res, want, y)
        assert want["n_iter"] >= 2
    # max_iter cuts the iteration: not converged, the same centres as the oracle's
    want = orc.fit(y, c0, max_iter=1, rel_tol=0.0)
    res = kmeans.kmeans_fit(yt, k, init=torch.from_numpy(c0), max_iter=1, rel_tol=0.0)
    check_fit(res, want, y)
    assert not bool(res.converged) and int(res.n_iter) == 1


def test_batch_nan_rows_empty_clusters_and_center_tol():
    from lam_slide_amd import kmeans
    ys = [orc.blobs(200, 4, 2, seed=10 + i, spread=0.3 + 0.4 * i, sep=3.0) for i in range(3)]
    ys[1][17] = np.nan
    ys[1][150, 1] = np.nan
    y = torch.from_numpy(np.stack(ys))
    init = y[:, :6].clone()
    init[2, 5] = 1e6  # a centre no row is nearest to: an empty cluster
    res = kmeans.kmeans_fit(y, 6, init=init, rel_tol=0.0)
    assert res.centers.shape == (3, 6, 2) and res.labels.shape == (3, 200) and res.counts.shape == (3, 6) and res.n_iter.shape == (3,)
    for s in range(3):
        want = orc.fit(ys[s], init[s].numpy(), rel_tol=0.0)
        one = kmeans.KMeansResult(*(r[s] for r in res[:6]), res.path)
        check_fit(one, want, ys[s])
    lab = res.labels.numpy()
    assert lab[1, 17] == -1 and lab[1, 150] == -1 and (lab[1] == -1).sum() == 2 and int(res.counts[1].sum()) == 198
    assert int(res.counts[2, 5]) == 0 and torch.equal(res.centers[2, 5], init[2, 5])  # kept bit for bit
    assert len(set(res.n_iter.tolist())) > 1  # the series stop at different iterations: a finished one is left alone
    # center_tol: stops no later, by the oracle's rule
    want = orc.fit(ys[0], init[0].numpy(), rel_tol=0.0, center_tol=0.05)
    res = kmeans.kmeans_fit(y[0], 6, init=init[0], rel_tol=0.0, center_tol=0.05)
    check_fit(res, want, ys[0])
    with pytest.raises(ValueError):
        kmeans.kmeans_fit(y, 6, init=init, rel_tol=-1.0)
    with pytest.raises(ValueError):
        kmeans.kmeans_fit(y, 6, init=init[:, :5])
    with pytest.raises(ValueError):
        kmeans.kmeans_fit(y, 6, init="random")
    with pytest.raises(ValueError):
        kmeans.kmeans_fit(y[0, 0], 6)


def test_kmeanspp_indices_equal_the_numpy_restatement():
    from lam_slide_amd import kmeans
    S, n, k, d = 5, 400, 9, 3
    y = np.stack([orc.blobs(n, k, d, seed=20 + s) for s in range(S)])
    y[3, 11] = np.nan
    g = torch.Generator().manual_seed(137)
    u = torch.rand(S, k, generator=g, dtype=torch.float64)
    idx = kmeans.kmeanspp_indices(torch.from_numpy(y), u).numpy()
    for s in range(S):
        assert np.array_equal(idx[s], orc.kmeanspp_indices(y[s], u[s].numpy())), s
        assert idx[s, 0] == int(np.floor(float(u[s, 0]) * n)) and len(set(idx[s].tolist())) == k
    # the module draws exactly these numbers from the seed: the same centres; another seed gives others
    c = kmeans.initial_centers(torch.from_numpy(y), k, "kmeans++", seed=137)
    assert torch.equal(c.nan_to_num(7.0), torch.from_numpy(y)[torch.arange(S)[:, None], torch.from_numpy(idx)].nan_to_num(7.0))
    assert torch.equal(c.nan_to_num(7.0), kmeans.initial_centers(torch.from_numpy(y), k, "kmeans++", seed=137).nan_to_num(7.0))
    assert not torch.equal(c.nan_to_num(7.0), kmeans.initial_centers(torch.from_numpy(y), k, "kmeans++", seed=138).nan_to_num(7.0))
    res = kmeans.kmeans_fit(torch.from_numpy(y[0]), k, seed=137)
    want = orc.fit(y[0], y[0][idx[0]])
    check_fit(res, want, y[0])


def test_nearest_rows_restatement():
    from lam_slide_amd import kmeans
    y = np.stack([orc.blobs(60, 20, 2, seed=30 + s) for s in range(4)])
    y[1, 5] = y[1, 40]  # a duplicate: the lowest index wins
    y[2, 3] = np.nan
    y[3] = np.nan
    c = y[:, ::3][:, :20].copy()
    c[1, 0] = y[1, 40]
    c[3] = 0.0
    rows = kmeans.nearest_rows(torch.from_numpy(y), torch.from_numpy(c))
    assert rows.dtype == torch.int32 and rows.shape == (4, 20) and kmeans.last_path["nearest_rows"] == "torch"
    for s in range(4):
        want, gap = orc.nearest(y[s], c[s])
        assert np.array_equal(rows[s].numpy(), want), s
    assert int(rows[1, 0]) == 5 and (rows[3] == -1).all() and 3 not in rows[2].tolist()
    assert torch.equal(kmeans.nearest_rows(torch.from_numpy(y[0]), torch.from_numpy(c[0])), rows[0])


def test_fit_microstates_gives_centres_for_assign_centers():
    from lam_slide_amd import assign_centers, fit_microstates, kmeans, tica
    y = torch.from_numpy(orc.blobs(3000, 10, 3, seed=40))
    centers = fit_microstates(y, k=10, max_iter=50)
    again = kmeans.kmeans_fit(y, 10, max_iter=50, seed=137)
    assert centers.shape == (10, 3) and torch.equal(centers, again.centers) and tica.last_path["fit_microstates"] == "torch"
    labels, counts = assign_centers(y, centers)
    assert torch.equal(labels, again.labels) and torch.equal(counts, again.counts)


# ---- displacement_errors ----
def today(pred, target, mask, c1, R):
    """displacement_errors' torch path as it was before post_process existed."""
    from lam_slide_amd import metrics
    pred5, t0t, Tf = metrics._layout(pred, target, c1)
    rows, traj = metrics._rows_torch(pred5, target, c1, t0t, Tf)
    B, A = pred5.shape[1], pred5.shape[3]
    agents = rows[:R].min(dim=0).values
    real = torch.ones(B, A, dtype=torch.bool) if mask is None else (mask if mask.dtype == torch.bool else mask != 0)
    agents = torch.where(real[..., None], agents, torch.full((), float("nan"), dtype=agents.dtype))
    kept = torch.where(real[..., None], agents, torch.zeros((), dtype=agents.dtype)).double()
    totals = torch.cat((kept.sum(dim=(0, 1)), real.sum().double()[None], traj[:R].double().sum(dim=(0, 1))))
    return agents[..., 0], agents[..., 1], traj[..., 0], traj[..., 1], totals


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def test_defaults_leave_displacement_errors_bit_identical(golden):
    from lam_slide_amd import DisplacementMeter, displacement_errors
    f11, f14 = golden("f11_pedestrian_k.npz"), golden("f14_compute_errors.npz")
    c1 = f11["positions"].shape[2] - f11["true_future"].shape[1]
    p14, t14 = f14["traj"].permute(1, 2, 0, 3)[:, None].contiguous(), f14["target"].permute(1, 0, 2)[None].contiguous()
    for pred, target, mask, first, R in ((f11["positions"], f11["true_future"], f11["attention_mask"][:, -1], c1, None),
                                         (f11["positions"], f11["true_future"], f11["attention_mask"][:, -1], c1, 7), (p14, t14, None, 0, None)):
        want = today(pred, target, mask, first, pred.shape[0] if R is None else R)
        for kw in ({}, {"post_process": False}, {"post_process": False, "post_kmeans": {"seed": 3}}):
            r = displacement_errors(pred, target, mask, first_frame=first, num_runs=R, **kw)
            for got, w in zip((r.ade, r.fde, r.traj_ade, r.traj_fde, r.totals), want):
                assert got.dtype == w.dtype and torch.equal(bits(got), bits(w))
            assert r.ade_post is None and r.fde_post is None and r.totals_post is None and r.path == "torch"
            m = DisplacementMeter(2.0)
            m.update(r)
            assert sorted(m.compute()) == ["ade", "fde", "traj_ade", "traj_fde"]
            with pytest.raises(ValueError):
                r.real_post()


def nba_post_process(all_final_frames, all_traj, all_target, res_centers):
    """second_stage/nba.py:190-196 and 230-236 line by line, with the fitted centres handed in."""
    def _compute_errors(selected_traj, all_target):
        error = torch.norm(selected_traj - all_target[:, None], dim=-1)  # [B, K, T]
        error_ave = error.mean(dim=-1)  # [B, K]
        error_final = error[..., -1]  # [B, K]
        return error_ave.min(dim=1).values, error_final.min(dim=1).values

    dis = torch.norm(all_final_frames[:, :, None, :] - res_centers[:, None, :, :], dim=-1)  # [B, K, C]
    index = dis.argmin(dim=1)
    selected_traj = all_traj[torch.arange(all_traj.size(0))[:, None], index]
    return _compute_errors(selected_traj, all_target)


def test_post_process_torch_path_is_the_reference_lines():
    from lam_slide_amd import DisplacementMeter, best_of_k_errors, displacement_errors
    g = torch.Generator().manual_seed(5)
    K, R, B, T, A, D, c1 = 12, 4, 3, 9, 11, 2, 3
    target = torch.randn(B, T, A, D, generator=g)
    pred = target[None] + 0.5 * torch.randn(K, B, T, A, D, generator=g)
    mask = torch.ones(B, A, dtype=torch.bool)
    mask[0, 3] = mask[2, 10] = False
    r = displacement_errors(pred, target, mask, first_frame=c1, num_runs=R, post_process=True, post_kmeans={"seed": 11})
    assert r.path == "torch" and r.post_fit.path == "torch" and r.post_fit.centers.shape == (B * A, R, D) and r.post_rows.shape == (B, A, R)
    assert r.ade_post.shape == (B, A) and r.totals_post.dtype == torch.float64 and r.totals_post.shape == (2,)
    keep = mask.reshape(-1)
    fut = pred[:, :, c1:]
    all_traj = fut.permute(1, 3, 0, 2, 4).reshape(B * A, K, T - c1, D)[keep]  # "(B L) K T D"
    all_final = fut[:, :, -1].permute(1, 2, 0, 3).reshape(B * A, K, D)[keep]
    all_target = target[:, c1:].permute(0, 2, 1, 3).reshape(B * A, T - c1, D)[keep]
    ades, fdes = nba_post_process(all_final, all_traj, all_target, r.post_fit.centers[keep])
    ade_post, fde_post = r.real_post()
    assert ade_post.shape == ades.shape == (B * A - 2,)
    # The centre of a cluster of two samples is their midpoint: both are equally near in exact arithmetic, and rounding picks one.  The
    # reference's lines evaluate the distances in float32 (relative error of a squared distance <= 4 * 2^-24 ~ 2.4e-7), the module in
    # float64: an agent is compared only where the float64 gap between the nearest and the second-nearest sample of every centre is
    # above 1e-6, where the two evaluations must select the same samples.
    cen = r.post_fit.centers[keep].numpy()
    clear = torch.tensor([float(orc.nearest(all_final[i].numpy(), cen[i])[1].min()) > 1e-6 for i in range(len(cen))])
    print(f"post_process: {int(clear.sum())} of {len(clear)} agents without a near tie")
    assert int(clear.sum()) >= 12
    assert float((ade_post - ades)[clear].abs().max()) <= 4e-6 * float(ades.abs().max()) and float((fde_post - fdes)[clear].abs().max()) <= 4e-6 * float(fdes.abs().max())
    assert torch.isnan(r.ade_post[0, 3]) and torch.isnan(r.fde_post[2, 10]) and int(torch.isnan(r.ade_post).sum()) == 2
    assert abs(float(r.totals_post[0]) - float(ade_post.double().sum())) <= 1e-12 * float(r.totals_post[0])
    # best-of-num_runs over the first samples is untouched by the branch; the selection is over all K samples
    plain = displacement_errors(pred, target, mask, first_frame=c1, num_runs=R)
    assert torch.equal(bits(plain.ade), bits(r.ade)) and torch.equal(plain.totals, r.totals)
    assert (ade_post >= displacement_errors(pred, target, mask, first_frame=c1).real()[0] - 1e-6).all()
    m = DisplacementMeter(3.0)
    m.update(r)
    m.update(r)
    out = m.compute()
    assert abs(out["ade_post"] - 3.0 * float(ade_post.double().mean())) <= 1e-12 * out["ade_post"] and sorted(out) == ["ade", "ade_post", "fde", "fde_post", "traj_ade", "traj_fde"]
    assert abs(out["fde_post"] - 3.0 * float(fde_post.double().mean())) <= 1e-12 * out["fde_post"]

    class Drv:  # the two members best_of_k_errors reads
        cond_idx = (0, c1)

        def sample_latents_k(self, latents, K, y=None, inits=None):
            return pred.reshape(K, B, T, A * D, 1)

    four = best_of_k_errors(Drv(), torch.zeros(B, T, A * D, 1), target[:, c1:], K, lambda z: z.reshape(K * B, T, A, D), mask, num_runs=R, fused=True,
                            post_process=True, post_kmeans={"seed": 11})
    assert len(four) == 4 and torch.equal(four[2], ade_post) and torch.equal(four[3], fde_post) and torch.equal(four[0], r.real()[0])
    two = best_of_k_errors(Drv(), torch.zeros(B, T, A * D, 1), target[:, c1:], K, lambda z: z.reshape(K * B, T, A, D), mask, num_runs=R, fused=True)
    assert len(two) == 2 and torch.equal(two[0], four[0])
    with pytest.raises(ValueError):
        best_of_k_errors(Drv(), torch.zeros(B, T, A * D, 1), target[:, c1:], K, lambda z: z.reshape(K * B, T, A, D), mask, post_process=True)
