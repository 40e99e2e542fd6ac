"""GPU tests of the contracts BETWEEN entry points of the statistics kernels: what two kernels must do alike because users rely on it, which no
single-kernel test states.  Each holds by construction - both sides call one fragment of csrc/k_stat_frag.hip.h - and is pinned here.

  kmeans_fit / assign_centers   the labels and counts of an assignment against given centres are the same integers (nearest_centre)
  nearest_rows / assign_centers the reverse lookup is the assignment with rows and centres swapped: (a - b)^2 and (b - a)^2 are one float64
                                value, so the fused chains (sq_dist_chain) agree bit for bit and ties go to the lowest index on both sides
  narrow / wide projection      lsl_project and lsl_project_wide run one float64 chain: a table padded with a zero column, whose term
                                is fma(0, 0, acc) = acc, projects to the same bits and the same limits
Every assertion is an equality of integers or of bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _table(rng, n, d):
    """float32 [n, d] on a coarse grid (multiples of 1/4 in [-2, 2]): equal distances happen, and ties are part of what is compared."""
    return (rng.integers(-8, 9, size=(n, d)) / 4.0).astype(np.float32)


@pytest.mark.parametrize("S,n,d,k", ((1, 1, 1, 1), (1, 257, 3, 7), (1, 300, 64, 128), (5, 60, 2, 20)))
def test_kmeans_fit_labels_are_assign_centers_labels(dev, S, n, d, k):
    from lam_slide_amd import assign_centers, kmeans, tica
    rng = np.random.default_rng(1000 + n)
    y, c = np.stack([_table(rng, n, d) for _ in range(S)]), np.stack([_table(rng, k, d) for _ in range(S)])
    if (n, d, k) == (257, 3, 7):
        c[0, 5] = c[0, 2]  # two identical centres: the tie goes to the lowest index
        y[0, 100] = c[0, 2]
        y[0, 3, 1] = y[0, 256, 0] = np.nan  # two rows that hold a NaN: -1, not counted
    yt, ct = torch.from_numpy(y).to(dev), torch.from_numpy(c).to(dev)
    fit = kmeans.kmeans_fit(yt, k, init=ct, max_iter=0)
    assert fit.path == "fused" and fit.labels.shape == (S, n) and fit.counts.shape == (S, k)
    for s in range(S):
        labels, counts = assign_centers(yt[s], ct[s])
        assert tica.last_path["assign_centers"] == "fused"
        assert torch.equal(fit.labels[s], labels) and torch.equal(fit.counts[s], counts), s
    if (n, d, k) == (257, 3, 7):
        lab = fit.labels[0].cpu()
        assert lab[100] == 2 and lab[3] == -1 and lab[256] == -1 and int((lab == 5).sum()) == 0 and int(fit.counts[0].sum()) == n - 2


@pytest.mark.parametrize("n,d,k", ((64, 2, 20), (65, 8, 1024)))  # one lane per (series, centre) up to 64 rows, 64 lanes above
def test_nearest_rows_is_assign_centers_with_the_roles_swapped(dev, n, d, k):
    from lam_slide_amd import assign_centers, kmeans, tica
    rng = np.random.default_rng(2000 + n)
    y, c = _table(rng, n, d), _table(rng, k, d)
    y[n - 1] = y[0]  # a duplicate row: the lowest row wins on both sides
    c[0] = y[0]
    yt, ct = torch.from_numpy(y).to(dev), torch.from_numpy(c).to(dev)
    rows = kmeans.nearest_rows(yt, ct)
    labels, _ = assign_centers(ct, yt)
    assert kmeans.last_path["nearest_rows"] == "fused" and tica.last_path["assign_centers"] == "fused"
    assert torch.equal(rows, labels) and int(rows[0]) == 0


def test_narrow_and_wide_projection_agree_on_a_padded_table(dev):
    from lam_slide_amd import TicaModel, WideTicaModel, koopman_tica, tica
    n, F, d = 65, 128, 16  # a full tile of rows and a tile of one row; the widest narrow table, one column short of the narrowest wide one
    rng = np.random.default_rng(3000)
    x = rng.standard_normal((n, F)).astype(np.float32)
    mean, W = rng.standard_normal(F), rng.standard_normal((F, d))
    narrow = TicaModel(mean, W, np.ones(d), d, kinetic_map=False)
    wide = WideTicaModel(np.append(mean, 0.0), np.vstack([W, np.zeros((1, d))]), np.ones(d), d, kinetic_map=False)
    xn = torch.from_numpy(x).to(dev)
    xw = torch.from_numpy(np.hstack([x, np.zeros((n, 1), dtype=np.float32)])).to(dev)
    out = []
    for model, table in ((narrow, xn), (wide, xw)):
        lim = torch.empty(2, d, dtype=torch.float32, device=dev)
        lim[0], lim[1] = float("inf"), float("-inf")
        out.append((model.transform(table, lim), lim))
        assert tica.last_path["transform"] == "fused"
    assert koopman_tica.last_path["transform"] == "fused"
    (yn, ln), (yw, lw) = out
    assert yn.shape == (n, d) and torch.equal(yn, yw) and torch.equal(ln, lw)
    assert torch.equal(ln[0], yn.amin(dim=0)) and torch.equal(ln[1], yn.amax(dim=0))
