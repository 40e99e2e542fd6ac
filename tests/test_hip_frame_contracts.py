"""GPU tests of the contracts BETWEEN the kernels of the fp32 frame: what the head, the no-network record and the trajectory-resident kernel
must do alike because a sampler mixes them and a sharded run concatenates their states, which no single-kernel test states.  The general
path holds them by construction - k_head_step_mfma and k_state_affine call one fragment of csrc/k_small_frag.hip.h (step_apply) - and
k_resident restates that fragment four wide; both are pinned here.

  one noise stream              the value w a record draws for element e of the state is element elem_offset + e of the documented stream under
                                the record's step index, whichever kernel applies the record: the no-network record x <- 0 x + 1 w, the network
                                record (ax, am, aw) = (0, 0, 1) through the general head, and the same two records on the resident path (0 x and
                                0 m are zeros for finite x and m, and 1 w + 0 = w, so the equality is exact)
  one update, three destinations  a record with a trace slice and LSL_STEP_SAVE leaves the same values in x, in the trace and in the saved state,
                                applied by the head or as a no-network record
Every assertion is torch.equal on values."""
import ctypes as C

import pytest
import torch

from test_hip_frame import _lib, _stream, head, lib_noise

pytestmark = pytest.mark.gpu

SEED = 0x1_0000_0007  # both key words of the stream non-zero
OFFSET = 5            # not on a Philox block boundary
STEPS = (0, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _model(D, H, mlp_ratio, Cc, dev):
    from lam_slide_amd import LatentSIV3
    from lam_slide_amd.synthetic import seeded_state_dict
    net = LatentSIV3(reset_parameters=False, depth=1, in_dim=Cc, hidden_size=D, num_heads=H, mlp_ratio=mlp_ratio)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net.to(dev)
    net.ensure_packed(dev)
    return net


@pytest.fixture(scope="module")
def head_case(dev):
    """The general head at hidden 64, 4 heads, in_dim 3 on 33 tokens (B = 1, T = 1, L = 33): two head tiles, the second ragged, C no multiple
    of 4.  -> (net, h [33, 64], mods [1, MODW], x [33, 3])"""
    D, Cc, n = 64, 3, 33
    net = _model(D, 4, 1, Cc, dev)
    g = torch.Generator().manual_seed(7)
    h = torch.randn(n, D, generator=g).to(dev)
    mods = (0.5 * torch.randn(1, 8 * D, generator=g)).to(dev)  # depth 1: six rows of the sub-blocks, then the head's shift | scale
    x = torch.randn(n, Cc, generator=g).to(dev)
    return net, h, mods, x


def test_one_noise_stream_head(dev, head_case):
    net, h, mods, x = head_case
    n = x.shape[0]
    for step in STEPS:
        w = lib_noise(net, n, SEED, step, OFFSET, dev)
        assert torch.isfinite(w).all() and float(w.abs().max()) > 0
        got, *_ = head(net, h, mods, 1, 1, n, dev, rec=(0.0, 0.0, 1.0, 0.0), x=x, seed=SEED, offset=OFFSET, step=step)
        assert torch.equal(got, w), (step, int((got != w).sum()), "elements differ")
    assert not torch.equal(lib_noise(net, n, SEED, 0, OFFSET, dev), lib_noise(net, n, SEED, 1, OFFSET, dev))  # (the step index is looked at)


@pytest.mark.parametrize("T,L", ((2, 2), (3, 16)), ids=("one_token_tile", "three_token_tiles"))
def test_one_noise_stream_resident(dev, T, L):
    L_, lib = _lib()
    B, Cc = 2, 32
    net = _model(128, 4, 2, Cc, dev)
    assert lib.lsl_sampler_path(net._handle, T, L) == 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, L, Cc, generator=g).to(dev)
    x_cond = torch.randn(B, T, L, Cc, generator=g).to(dev)
    mask = torch.zeros(B, T, L, dtype=torch.long, device=dev)
    n = B * T * L
    trace = torch.full((2, n, Cc), float("nan"), device=dev)
    io, keep = net.make_io(x, x_cond, mask, None)
    ws = net.workspace(B, T, L, dev)
    steps = (L_.Step * 2)(L_.Step(0.25, 0.0, 0.0, 1.0), L_.Step(0.5, 0.0, 0.0, 1.0))  # record s: stream step s, trace slice s
    L_.check(lib.lsl_sample(net._handle, C.byref(io), steps, 2, None, 0, SEED, OFFSET, trace.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    del keep
    w0, w1 = (lib_noise(net, n, SEED, s, OFFSET, dev) for s in STEPS)
    assert torch.equal(trace[0], w0), (int((trace[0] != w0).sum()), "elements of the first record's trace slice differ")
    assert torch.equal(x.reshape(n, Cc), w1), (int((x.reshape(n, Cc) != w1).sum()), "elements of the final state differ")
    assert torch.equal(trace[1], w1)


def test_one_update_three_destinations(dev, head_case):
    net, h, mods, x = head_case
    L_, lib = _lib()
    n, Cc = x.shape
    # by the head
    out, trace, save, _ = head(net, h, mods, 1, 1, n, dev, rec=(0.75, -0.5, 1.25, 0.0), x=x, want_trace=True, want_save=True, seed=SEED, offset=OFFSET, step=1)
    assert torch.isfinite(out).all() and not torch.equal(out, x)
    assert torch.equal(trace, out) and torch.equal(save, out)
    # as a no-network record; the saved state lives in the call's workspace: a second record x <- 0 x + 1 saved hands it out
    def run(records):
        xs = x.reshape(1, 1, n, Cc).clone()
        io, keep = net.make_io(xs, torch.zeros_like(xs), torch.zeros(1, 1, n, dtype=torch.long, device=dev), None)
        ws = net.workspace(1, 1, n, dev)
        ws.fill_(0xFF)  # (float32 NaNs: a saved state that was not written shows)
        tr = torch.full((len(records), n, Cc), float("nan"), device=dev)
        steps = (L_.StepEx * len(records))(*records)
        L_.check(lib.lsl_sample_ex(net._handle, C.byref(io), steps, len(records), None, 0, SEED, OFFSET, tr.data_ptr(), len(records), ws.data_ptr(), ws.numel(),
                                   _stream()))
        torch.cuda.synchronize()
        del keep
        return xs.reshape(n, Cc), tr
    update = L_.StepEx(0.5, 0.75, 0.0, 1.25, 0.0, L_.STEP_NO_NETWORK | L_.STEP_SAVE, 1, 0)
    hand_out = L_.StepEx(0.5, 0.0, 0.0, 0.0, 1.0, L_.STEP_NO_NETWORK, 0, 1)
    x1, tr1 = run([update])
    x2, tr2 = run([update, hand_out])
    assert torch.isfinite(x1).all() and not torch.equal(x1, x)
    assert torch.equal(tr1[0], x1), "the trace slice against x"
    assert torch.equal(tr2[0], x1) and torch.equal(x2, x1) and torch.equal(tr2[1], x1), "the saved state against x"
