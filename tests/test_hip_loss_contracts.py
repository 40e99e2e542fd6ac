"""GPU tests of the contracts BETWEEN entry points of the loss kernels: what two kernels must do alike because users concatenate per-frame
sums of shards and finish them by ``sums=``, which no single-kernel test states.  Each holds by construction - both sides call one
fragment of csrc/k_loss_frag.hip.h - and is pinned here.

  the finals are one function    geom_losses, peptide_losses and class_losses finish their sums by one kernel (k_loss_final): a quotient
                                 of the same two columns has the same bits whichever entry point forms it, and they are the bits of the
                                 documented order - fp64 lane sums over rows l, l + 64, ..., the lanes added in lane order, one division,
                                 one rounding to float32
  the two team forms agree       a frame of 64 entities (a wave per frame) and the same frame padded to 65 with a masked-out entity (the
                                 workgroup per frame) give the same five sums: wave 0 owns the same entities in the same order and the
                                 other three waves add exact zeros
Every assertion is an equality of bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _bits(x) -> list:
    """The float32 bit patterns of a tensor, a list of tensors or an array of float32."""
    if isinstance(x, (list, tuple)):
        x = torch.stack(list(x))
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    assert x.dtype == np.float32
    return np.ascontiguousarray(x).reshape(-1).view(np.uint32).tolist()


def _column_total(table: np.ndarray, k: int) -> float:
    """The documented order in plain loops (Python floats are fp64): lane l adds rows l, l + 64, ...; the lanes are added in lane order."""
    lanes = []
    for lane in range(64):
        s = 0.0
        for f in range(lane, table.shape[0], 64):
            s += float(table[f, k])
        lanes.append(s)
    tot = 0.0
    for s in lanes:
        tot += s
    return tot


def _quotient(num: float, den: float) -> np.ndarray:
    return np.array([num / den], dtype=np.float64).astype(np.float32)  # one division, one rounding


@pytest.mark.parametrize("F", (1, 63, 64, 65, 130))
def test_the_finals_are_one_function(dev, F):
    from lam_slide_amd import class_losses, geom_losses, peptide_losses
    rng = np.random.default_rng(4000 + F)
    g = (rng.random((F, 5)) * 100.0 + 0.5).astype(np.float32)
    p = (rng.random((F, 4)) * 100.0 + 0.5).astype(np.float32)
    gt, pt = torch.from_numpy(g).to(dev), torch.from_numpy(p).to(dev)
    geo, pep = geom_losses(sums=gt), peptide_losses(sums=(gt, pt))
    cls = class_losses(sums=gt[:, [0, 2]].contiguous())
    for a, b in (("pos_loss", "pos_loss"), ("dist", "norm_loss"), ("inter_dist_loss", "inter_distance_loss")):
        assert _bits(geo[a]) == _bits(pep[b]), (a, b)
    assert _bits(cls) == _bits(geo["pos_loss"])
    G, P = [_column_total(g, k) for k in range(5)], [_column_total(p, k) for k in range(4)]
    assert _bits([geo["pos_loss"], geo["dist"], geo["inter_dist_loss"]]) == _bits(np.concatenate(
        [_quotient(G[0], G[2]), _quotient(G[1], G[2]), _quotient(G[3], G[4])]))
    assert _bits([pep["pos_frame_loss"], pep["torsion_loss"]]) == _bits(np.concatenate([_quotient(P[0], P[1]), _quotient(P[2], P[3])]))


@pytest.mark.parametrize("D", (2, 3))
def test_the_two_team_forms_agree(dev, D):
    from lam_slide_amd import geom_loss_sums
    F, A = 5, 64  # F = 5: the last workgroup of the 64-thread form holds a single live team
    rng = np.random.default_rng(5000 + D)
    pred, target = (rng.standard_normal((F, A + 1, D)).astype(np.float32) for _ in range(2))  # (entity 64: finite, masked out below)
    mask = rng.random((F, A + 1)) < 0.8
    mask[:, A] = False
    mask[0, :A] = True  # one frame with every entity real
    pt, tt, mt = (torch.from_numpy(x).to(dev) for x in (pred, target, mask))
    wave = geom_loss_sums(pt[:, :A], tt[:, :A], mt[:, :A])
    group = geom_loss_sums(pt, tt, mt)
    assert wave.shape == group.shape == (F, 5) and int(wave[0, 2]) == A
    assert _bits(wave) == _bits(group)
