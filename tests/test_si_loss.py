"""``Transport.training_losses`` - the stochastic-interpolant validation loss - without a GPU: the generic path against fixtures generated
from the reference (tools/make_fixtures.py f15 f16), the draw order of ``Transport.sample``, enum equality by name, the gradient guard, and
the C ABI of the new entry points (symbols, header, argument validation before anything touches a GPU).

Bars.  F15's times lie in [0.05, 0.9], where the worst-conditioned coefficient is the VP path's ``1 - exp(.) >= 0.1``: one fp32 ulp of the
reference's ``exp`` becomes 6e-7 relative in the loss; 1e-5 leaves about 30x for another libm and another summation order.  The F16 bars
are the ones ``test_f9_real_lightning_module_sample_chain`` holds the oracle to on the same weights."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import rel_l2
from oracle import latent_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS, PREDS, WEIGHTS = ("Linear", "GVP", "VP"), ("velocity", "data", "noise", "score"), (None, "velocity", "likelihood")
COMBOS = [(p, m, w) for p in PATHS for m in PREDS for w in WEIGHTS]


def f15_model(xt, t, **kw):
    """The closed-form "network" of fixture F15 (tools/make_fixtures.py: f15_model)."""
    return 0.7 * torch.tanh(xt) + 0.3 * torch.sin(3 * xt + t.reshape(-1, *([1] * (xt.dim() - 1))))


def rel_rows(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


@pytest.mark.parametrize("path,pred,weight", COMBOS)
def test_training_losses_generic_path_matches_reference(golden, path, pred, weight):
    from lam_slide_amd import CreateTransport
    f = golden("f15_si_loss.npz")
    want = f.group(f"{path}_{pred}_{weight}")
    tr = CreateTransport(path, pred, weight)()
    out = tr.training_losses(f15_model, f["x1"], t=f["t"], x0=f["x0"])
    assert set(out) == {"pred", "loss"} and out["loss"].shape == (f["x1"].shape[0],) and tr.last_path == "generic"
    e_loss, e_pred = rel_rows(out["loss"], want["loss"]), rel_l2(out["pred"], want["pred"])
    print(f"F15 {path} {pred} {weight}: loss {e_loss:.2e} pred {e_pred:.2e}")
    assert e_loss < 1e-5 and e_pred < 1e-6
    # model_kwargs reach the callable, and the output-shape assertion of transport.py:130-131 holds
    seen = {}
    tr.training_losses(lambda xt, t, **kw: seen.update(kw) or f15_model(xt, t), f["x1"], {"flag": 3}, t=f["t"], x0=f["x0"])
    assert seen == {"flag": 3}
    with pytest.raises(AssertionError):
        tr.training_losses(lambda xt, t: f15_model(xt, t)[..., :4], f["x1"], t=f["t"], x0=f["x0"])


def test_sample_draw_order_and_interval(golden):
    from lam_slide_amd import CreateTransport
    f = golden("f15_si_loss.npz")
    d = f.group("draws")
    x1 = f["x1"]
    for path, pred in (("GVP", "data"), ("Linear", "velocity")):
        torch.manual_seed(1234)
        t, x0, same = CreateTransport(path, pred)().sample(x1)
        assert same is x1 and x0.shape == x1.shape and t.shape == (x1.shape[0],) and t.dtype == x1.dtype
        assert torch.equal(t, d[f"{path}_{pred}_t"])  # a uniform draw is an integer scaled in fp32: bit for bit
        assert float((x0[0, 0, 0, :4] - d[f"{path}_{pred}_x0"]).abs().max()) < 1e-6  # (normal draws pass through the host's vector libm)
    # without fixed draws training_losses uses sample(): same seed, same result
    tr = CreateTransport("GVP", "data")()
    torch.manual_seed(1234)
    a = tr.training_losses(f15_model, x1)
    torch.manual_seed(1234)
    t, x0, _ = tr.sample(x1)
    b = tr.training_losses(f15_model, x1, t=t, x0=x0)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["pred"], b["pred"])
    big = torch.zeros(4096, 1, 1, 2)
    for path in PATHS:
        for pred in PREDS:
            tr = CreateTransport(path, pred)()
            t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps)
            t = tr.sample(big)[0]
            assert t0 <= float(t.min()) and float(t.max()) <= t1 and float(t.max()) - float(t.min()) > 0.9 * (t1 - t0), (path, pred)


def test_f16_real_model_step_generic_path(golden):
    """F16 = the reference's real md17 ``Wrapper.model_step`` (Loss.forward with calc_additional_losses); here its ``si_loss`` through
    the generic path with the oracle network on F9's weights."""
    from lam_slide_amd import CreateTransport
    f, f9 = golden("f16_model_step.npz"), golden("f9_sample.npz")
    sd = f9.group("backbone")
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=64, mlp_ratio=2, num_heads=4)
    model = lambda xt, t, x_cond, x_cond_mask: latent_net.forward(sd, sh, xt, t, x_cond, x_cond_mask)  # noqa: E731
    tr = CreateTransport("GVP", "data")()
    out = tr.training_losses(model, f["latents"], {"x_cond": f["x_cond"], "x_cond_mask": f["mask"]}, t=f["t"], x0=f["x0"])
    e_pred, e_loss = rel_l2(out["pred"], f["pred"]), rel_rows(out["loss"], f["loss"])
    e_si = abs(float(out["loss"].mean()) - float(f.group("losses")["si_loss"])) / float(f.group("losses")["si_loss"])
    print(f"F16 generic: pred {e_pred:.2e} loss {e_loss:.2e} si_loss {e_si:.2e}")
    assert e_pred < 5e-6 and e_loss < 1e-5 and e_si < 1e-5
    assert set(f.group("losses")) == {"si_loss", "pos_loss", "inter_dist_loss", "dist", "loss"}


def test_si_rows_table():
    """The affine table behind both paths: trajectory b's loss is w mean((p pred + q1 x1 + q0 x0)^2) with xt = alpha x1 + sigma x0."""
    import math
    from lam_slide_amd import CreateTransport
    t = torch.tensor([0.25, 0.5], dtype=torch.float32)
    rows = CreateTransport("Linear", "velocity")().si_rows(t)
    assert rows.shape == (2, 6) and rows.dtype == torch.float32
    assert torch.equal(rows, torch.tensor([[0.25, 0.75, 1, -1, 1, 1], [0.5, 0.5, 1, -1, 1, 1]]))
    rows = CreateTransport("GVP", "data")().si_rows(t)
    assert torch.allclose(rows[1], torch.tensor([math.sin(math.pi / 4), math.cos(math.pi / 4), 1, -1, 0, 1]), atol=1e-7, rtol=0)
    rows = CreateTransport("Linear", "score", "likelihood")().si_rows(t)  # W = drift_var / sigma^2 = 1/t + 1/(1 - t) on the linear path
    assert torch.allclose(rows[:, 2:], torch.tensor([[0.75, 0, 1, 4 + 4 / 3], [0.5, 0, 1, 4.0]]), atol=0, rtol=1e-6)


def test_enums_compare_and_hash_by_name():
    import enum
    from lam_slide_amd import CreateTransport, ModelType, PathType, WeightType, as_transport

    class Foreign:  # enum classes of another module with the reference's class names (transport.py:15-37)
        class ModelType(enum.Enum):
            NOISE = enum.auto()
            SCORE = enum.auto()
            VELOCITY = enum.auto()
            DATA = enum.auto()

        class PathType(enum.Enum):
            LINEAR = enum.auto()
            GVP = enum.auto()
            VP = enum.auto()

        class WeightType(enum.Enum):
            NONE = enum.auto()
            VELOCITY = enum.auto()
            LIKELIHOOD = enum.auto()

    for mine, theirs in ((ModelType, Foreign.ModelType), (PathType, Foreign.PathType), (WeightType, Foreign.WeightType)):
        for m in mine:
            assert m == theirs[m.name] and theirs[m.name] == m and not (m != theirs[m.name]) and not (theirs[m.name] != m)
            assert {m: 1}[theirs[m.name]] == 1 and {theirs[m.name]: 2}[m] == 2
            for o in theirs:
                if o.name != m.name:
                    assert m != o and o != m
        assert len(set(mine)) == len(list(mine)) and all(m is mine[m.name] for m in mine)
    assert ModelType.VELOCITY != WeightType.VELOCITY and ModelType.VELOCITY != Foreign.WeightType.VELOCITY and ModelType.DATA != "DATA"
    si = CreateTransport("GVP", "data")()
    assert si.model_type == Foreign.ModelType.DATA  # what Loss.forward asserts (second_stage/md17.py:232-234)
    assert as_transport(si) is si

    class RefLike:  # the reference's Transport read by duck typing keeps working
        model_type, loss_type, train_eps, sample_eps = Foreign.ModelType.NOISE, Foreign.WeightType.LIKELIHOOD, 1e-3, 1e-3
        path_type = Foreign.PathType.VP

    got = as_transport(RefLike())
    assert got.model_type is ModelType.NOISE and got.path_type is PathType.VP and got.loss_type is WeightType.LIKELIHOOD


def test_gradient_guard():
    """The HIP path has no backward: with grad mode on and a trainable backbone the call refuses instead of returning a loss that trains
    nothing; under no_grad (every validation_step), or with a frozen backbone, the guard is silent (on this CPU-only host the call then
    reaches the network, which has no CPU implementation)."""
    from lam_slide_amd import CreateTransport, LatentSIV3
    net = LatentSIV3(depth=1, in_dim=8, hidden_size=64, num_heads=4)
    x1 = torch.zeros(2, 3, 4, 8)
    kw = {"x_cond": x1, "x_cond_mask": torch.zeros(2, 3, 4, dtype=torch.long)}
    tr = CreateTransport("GVP", "data")()

    class Module:  # LightningModule-shaped: Loss.forward passes the module itself, whose bound forward calls the backbone
        def __init__(self):
            self.backbone, self.si = net, tr

        def forward(self, xt, t, **model_kwargs):
            return self.backbone(x=xt, t=t, **model_kwargs)

        __call__ = forward

    for model in (net, net.forward, Module(), Module().forward):
        with torch.enable_grad():
            with pytest.raises(RuntimeError, match="no_grad"):
                tr.training_losses(model, x1, kw)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                tr.training_losses(model, x1, kw)
    net.requires_grad_(False)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tr.training_losses(net, x1, kw)
    with torch.enable_grad():  # any other callable: the generic path, gradients flow as in the reference
        x = torch.ones(2, 3, 4, 8)
        w = torch.full((), 2.0, requires_grad=True)
        out = tr.training_losses(lambda xt, t: w * xt, x)
        out["loss"].mean().backward()
        assert w.grad is not None and tr.last_path == "generic"


def test_library_exports_and_header_declare_the_objective():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in ("lsl_si_loss", "lsl_si_reduce", "lsl_si_loss_workspace_bytes"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6
    assert re.search(r"#define LSL_SI_SLAB (\d+)", header).group(1) == str(_lib.SI_SLAB)
    assert C.sizeof(_lib.SiRow) == 24
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"lsl_si_loss", "lsl_si_reduce", "lsl_si_loss_workspace_bytes"} <= {line.split()[-1] for line in nm.splitlines()}


def test_stale_library_asks_for_a_rebuild(tmp_path):
    """A library that predates the objective reports the same ABI version 6: the binding finds it by the missing symbols and says "rebuild"."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "old.c"
    from lam_slide_amd import _lib
    old = [s for s in _lib.EXPORTED if not s.startswith("lsl_si_")]
    src.write_text("int lsl_version(void) { return 6; }\n" + "".join(f"void {s}(void) {{}}\n" for s in old if s != "lsl_version"))
    so = tmp_path / "libold.so"
    subprocess.run([cc, "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    code = ("import sys; sys.path.insert(0, %r)\nfrom lam_slide_amd import _lib\n_lib.LIB_PATH = %r\n"
            "try:\n    _lib.load()\nexcept RuntimeError as e:\n    print('MSG', e)\n" % (ROOT, str(so)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert "MSG" in out and "rebuild" in out and "lsl_si_loss" in out, out


def test_new_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    desc = _lib.ModelDesc(32, 256, 16, 16, 16, 512, 4, 0, 0, 10000.0)
    assert lib.lsl_model_create(C.byref(desc), C.byref(h)) == 0
    fwd, tot = lib.lsl_workspace_bytes(h, 4, 30, 192), lib.lsl_si_loss_workspace_bytes(h, 4, 30, 192)
    slabs = (30 * 192 * 32 + _lib.SI_SLAB - 1) // _lib.SI_SLAB
    assert fwd > 0 and fwd + 4 * slabs * 4 <= tot <= fwd + 4 * slabs * 4 + 512  # the forward's need + one float per trajectory and slab
    assert lib.lsl_si_loss_workspace_bytes(None, 4, 30, 192) == 0 and lib.lsl_si_loss_workspace_bytes(h, 0, 30, 192) == 0
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    io = _lib.IO(one, one, one, None, one, one, 1, 1, 1)
    assert lib.lsl_si_loss(None, C.byref(io), one, one, one, one, one, 1 << 40, None) == -1
    assert lib.lsl_si_loss(h, C.byref(io), one, one, one, one, one, 1 << 40, None) == -2  # weights not set
    assert b"weights" in lib.lsl_last_error()
    lib.lsl_model_destroy(h)
    assert lib.lsl_si_reduce(None, one, one, one, 2, 96, one, one, 1024, None) == -1
    assert lib.lsl_si_reduce(one, one, one, None, 2, 96, one, one, 1024, None) == -1
    assert lib.lsl_si_reduce(one, one, one, one, 2, 96, None, one, 1024, None) == -1
    assert lib.lsl_si_reduce(one, one, one, one, 0, 96, one, one, 1024, None) == -3
    assert lib.lsl_si_reduce(one, one, one, one, -1, 96, one, one, 1024, None) == -3
    assert lib.lsl_si_reduce(one, one, one, one, 2, 0, one, one, 1024, None) == -3
    assert lib.lsl_si_reduce(one, one, one, one, 2, 3 * 4096 + 5, one, one, 2 * 4 * 4 - 1, None) == -4  # 2 trajectories x 4 slabs
    assert b"scratch" in lib.lsl_last_error()
    assert lib.lsl_si_reduce(one, one, one, one, 2, 96, one, None, 1024, None) == -4
    with pytest.raises(ValueError):
        _lib.check(-3)


def test_python_wrappers_refuse_cpu_tensors():
    from lam_slide_amd import CreateTransport, si_reduce
    x = torch.zeros(2, 3, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        si_reduce(x, x, x, CreateTransport("GVP", "data")().si_rows(torch.tensor([0.3, 0.6])))
