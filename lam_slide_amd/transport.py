"""``CreateTransport`` / ``Transport`` / ``Sampler``: drop-in for ``src.modules.transport`` on the sampling
side (``configs/model/*/second-stage.yaml`` ``transport:`` blocks, lightning_base.py:219-234).

``Sampler(transport).get_sample_fn(method, kwargs)`` returns ``fn(init, model, **model_kwargs)`` exactly like
the reference (transport.py:475-503).  When ``model`` resolves to a :class:`lam_slide_amd.LatentSIV3`
(the module itself, its bound ``forward``, or a bound method of an object whose ``.backbone`` is one, which is
what ``SecondStageCondLightningBase.forward`` is) and the solver is fixed-grid Euler / Euler-Maruyama, the
whole loop runs inside liblamslide_hip.so (``lsl_sample``): every step is the affine update
``x <- ax x + am net(x,t) + aw w`` with (ax, am, aw) derived here in float64 from the reference's formulas.
Any other callable or solver goes through the generic per-step loop below, which mirrors
integrators.py:7-120 and calls ``model`` once per drift evaluation.

Preserved semantics: ``num_steps=N`` means N-1 Euler updates on ``linspace(t0, t1, N)``; the SDE result has
``len == num_steps``; (t0, t1) come from ``check_interval`` (transport.py:69-101); errors are the reference's
(KeyError unknown path, NotImplementedError unknown sampler / diffusion form / last step, AssertionError t0<t1).
"""
from __future__ import annotations

import ctypes as C
import enum
import math
from collections.abc import Sequence
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .latent_si import LatentSIV3
# the solvers (ode.py); their names stay importable from here
from .ode import (DOPRI_MAX_STEPS_MESSAGE, DOPRI_NON_FINITE_MESSAGE, FIXED_GRID_RK_METHODS, _DP_ALPHA, _DP_BETA, _DP_C_ERR, _DP_C_MID,  # noqa: F401
                  _RkOps, _f32, _rms, dopri5_solve, dopri5_solve_each, dopri_each_failure, fixed_grid_rk_solve)


class _ByName(enum.Enum):
    """Members compare and hash by NAME against any enum class of the same class name, so ``model.si.model_type == ModelType.DATA`` holds
    with the reference's own ``ModelType`` on the other side (second_stage/md17.py:232-234 asserts exactly that) and either enum finds the
    other's entry in a dict (``Enum.__hash__`` is the hash of the member name there too)."""

    def __eq__(self, other):
        if isinstance(other, enum.Enum) and type(other).__name__ == type(self).__name__:
            return self.name == other.name
        return NotImplemented

    def __hash__(self):
        return hash(self._name_)


class ModelType(_ByName):
    NOISE = enum.auto()
    SCORE = enum.auto()
    VELOCITY = enum.auto()
    DATA = enum.auto()


class PathType(_ByName):
    LINEAR = enum.auto()
    GVP = enum.auto()
    VP = enum.auto()


class WeightType(_ByName):
    NONE = enum.auto()
    VELOCITY = enum.auto()
    LIKELIHOOD = enum.auto()


_SMIN, _SMAX = 0.1, 20.0


class _Schedule:
    """Scalar (float64) alpha/sigma schedule of one path type: path.py:21-206 evaluated at one t."""

    def __init__(self, path_type: PathType):
        self.kind = path_type

    def alpha(self, t: float) -> Tuple[float, float]:
        if self.kind is PathType.LINEAR:
            return t, 1.0
        if self.kind is PathType.GVP:
            return math.sin(t * math.pi / 2), math.pi / 2 * math.cos(t * math.pi / 2)
        a = math.exp(self._lm(t))
        return a, a * self._dlm(t)

    def sigma(self, t: float) -> Tuple[float, float]:
        if self.kind is PathType.LINEAR:
            return 1 - t, -1.0
        if self.kind is PathType.GVP:
            return math.cos(t * math.pi / 2), -math.pi / 2 * math.sin(t * math.pi / 2)
        p = 2 * self._lm(t)
        s = math.sqrt(1 - math.exp(p))
        return s, math.exp(p) * (2 * self._dlm(t)) / (-2 * s)

    def _lm(self, t):
        return -0.25 * ((1 - t) ** 2) * (_SMAX - _SMIN) - 0.5 * (1 - t) * _SMIN

    def _dlm(self, t):
        return 0.5 * (1 - t) * (_SMAX - _SMIN) + 0.5 * _SMIN

    def drift_terms(self, t: float) -> Tuple[float, float]:
        """(k, var): the reference's compute_drift returns (-k x ... ) i.e. drift_mean = k * x, drift_var = var."""
        if self.kind is PathType.VP:
            beta = _SMIN + (1 - t) * (_SMAX - _SMIN)
            return -0.5 * beta, beta / 2
        if self.kind is PathType.LINEAR:
            ratio = 1 / t if t != 0 else math.inf  # torch gives inf here too (Linear path evaluated at t0 = 0)
        else:
            ratio = math.pi / (2 * math.tan(t * math.pi / 2))
        s, ds = self.sigma(t)
        return -ratio, ratio * s * s - s * ds

    def coeffs(self, t: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        """(alpha, d_alpha, sigma, d_sigma, drift_var) of every entry of the float64 tensor ``t``: the formulas above, vectorised
        (path.py: compute_alpha_t / compute_sigma_t / compute_drift of ICPlan, GVPCPlan, VPCPlan)."""
        one = torch.ones_like(t)
        if self.kind is PathType.VP:
            lm, dlm = self._lm(t), self._dlm(t)
            a = torch.exp(lm)
            e2 = torch.exp(2 * lm)
            s = torch.sqrt(1 - e2)
            return a, a * dlm, s, e2 * (2 * dlm) / (-2 * s), (_SMIN + (1 - t) * (_SMAX - _SMIN)) / 2
        if self.kind is PathType.LINEAR:
            a, da, s, ds = t, one, 1 - t, -one
            ratio = 1 / t
        else:
            h = t * (math.pi / 2)
            a, da, s, ds = torch.sin(h), math.pi / 2 * torch.cos(h), torch.cos(h), -math.pi / 2 * torch.sin(h)
            ratio = math.pi / (2 * torch.tan(h))
        return a, da, s, ds, ratio * s * s - s * ds

    def diffusion(self, t: float, form: str, norm: float) -> float:
        if form == "constant":
            return norm
        if form == "SBDM":
            return norm * self.drift_terms(t)[1]
        if form == "sigma":
            return norm * self.sigma(t)[0]
        if form == "linear":
            return norm * (1 - t)
        if form == "decreasing":
            return 0.25 * (norm * math.cos(math.pi * t) + 1) ** 2
        if form == "inccreasing-decreasing":
            return norm * math.sin(math.pi * t) ** 2
        raise NotImplementedError(f"Diffusion form {form} not implemented")


class Transport:
    def __init__(self, *, model_type, path_type, loss_type, train_eps, sample_eps):
        self.loss_type = loss_type
        self.model_type = model_type
        self.path_type = path_type
        self.schedule = _Schedule(path_type)
        self.train_eps = train_eps
        self.sample_eps = sample_eps
        self.last_path: Optional[str] = None  # "fused" | "generic" after a training_losses / si_loss call

    def check_interval(self, train_eps, sample_eps, *, diffusion_form="SBDM", sde=False, reverse=False, eval=False,
                       last_step_size=0.0):
        t0, t1 = 0, 1
        eps = train_eps if not eval else sample_eps
        if self.path_type is PathType.VP:
            t1 = 1 - eps if (not sde or last_step_size == 0) else 1 - last_step_size
        elif self.model_type != ModelType.VELOCITY or sde:
            t0 = eps if (diffusion_form == "SBDM" and sde) or self.model_type != ModelType.VELOCITY else 0
            t1 = 1 - eps if (not sde or last_step_size == 0) else 1 - last_step_size
        if reverse:
            t0, t1 = 1 - t0, 1 - t1
        return t0, t1

    # velocity(x, m) = vx * x + vm * m and score(x, m) = sx * x + sm * m for network output m (transport.py:158-226)
    def velocity_coeffs(self, t: float) -> Tuple[float, float]:
        if self.model_type is ModelType.VELOCITY:
            return 0.0, 1.0
        k, var = self.schedule.drift_terms(t)  # v = -drift_mean + var * score, drift_mean = k * x
        sx, sm = self.score_coeffs(t)
        return -k + var * sx, var * sm

    def score_coeffs(self, t: float) -> Tuple[float, float]:
        sch = self.schedule
        if self.model_type is ModelType.SCORE:
            return 0.0, 1.0
        if self.model_type is ModelType.NOISE:
            return 0.0, -1.0 / sch.sigma(t)[0]
        if self.model_type is ModelType.DATA:
            s, _ = sch.sigma(t)
            a, _ = sch.alpha(t)
            return -1.0 / (s * s), a / (s * s)
        a, da = sch.alpha(t)
        s, ds = sch.sigma(t)
        rev = a / da
        var = s * s - rev * ds * s
        return -1.0 / var, rev / var

    def prior_logp(self, z: Tensor) -> Tensor:
        """Log-density of the standard normal prior per sample of a batched ``z`` (transport.py:62-67): ``-N/2 log 2 pi - sum(z^2) / 2`` over
        the N elements of a sample, shape [B], in z's dtype, on z's device."""
        n = z[0].numel()
        return -0.5 * n * math.log(2.0 * math.pi) - z.reshape(z.shape[0], -1).pow(2).sum(dim=1) / 2.0

    # ---- the stochastic-interpolant objective without gradients (transport.py:103-156) ---------------------------------------------
    def sample(self, x1: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        """(t, x0, x1) with the reference's draws in the reference's order (transport.py:103-114): the noise first, then one uniform per
        trajectory from the CPU generator scaled into the training interval.  Same seed, same device: the reference's ``t`` and ``x0``."""
        x0 = torch.randn_like(x1)
        t0, t1 = self.check_interval(self.train_eps, self.sample_eps)
        t = torch.rand((x1.shape[0],)) * (t1 - t0) + t0
        t = t.to(x1)
        return t, x0, x1

    def si_rows(self, t: Tensor) -> Tensor:
        """The ``[B, 6]`` float32 table (alpha, sigma, p, q1, q0, w) of ``lsl_si_row`` (include/lsl_api.h) on the host: for trajectory b
            xt = alpha x1 + sigma x0,   r = p pred + q1 x1 + q0 x0,   loss_b = w mean(r^2)
        restates transport.py:135-154 for this transport's prediction and loss weight.  Derived once per call, vectorised over ``t``, in
        float64 from the float32 times and rounded to float32 (as ``velocity_coeffs`` does for the samplers)."""
        t64 = t.detach().to(device="cpu", dtype=torch.float32).double()
        a, da, s, ds, var = self.schedule.coeffs(t64)
        one, zero = torch.ones_like(t64), torch.zeros_like(t64)
        if self.model_type == ModelType.VELOCITY:
            p, q1, q0, w = one, -da, -ds, one
        elif self.model_type == ModelType.DATA:
            p, q1, q0, w = one, -one, zero, one
        else:
            if self.loss_type == WeightType.VELOCITY:
                w = (var / s) ** 2
            elif self.loss_type == WeightType.LIKELIHOOD:
                w = var / (s * s)
            elif self.loss_type == WeightType.NONE:
                w = one
            else:
                raise NotImplementedError()
            p, q1, q0 = (one, zero, -one) if self.model_type == ModelType.NOISE else (s, zero, one)
        return torch.stack([a, s, p, q1, q0, w], dim=1).float()

    def si_loss(self, model: Callable, x1: Tensor, t: Tensor, x0: Tensor, model_kwargs: Optional[Dict[str, Any]] = None) -> Dict[str, Tensor]:
        """``training_losses`` on given draws: {"pred", "loss" [B], "xt"}.  A ``lam_slide_amd.LatentSIV3`` behind ``model`` (the module, its
        bound ``forward``, a LightningModule or its bound ``forward``, through ``torch.compile`` wrappers) with a contiguous float32 GPU
        ``x1`` runs as ONE library call (``lsl_si_loss``: interpolant, network, reduction); any other callable goes through the same affine
        table in torch.  No backward exists on the HIP path: with grad mode on and a trainable backbone this raises instead of returning
        a loss that trains nothing."""
        model_kwargs = {} if model_kwargs is None else model_kwargs
        net = resolve_backbone(model)
        if net is None:  # Loss.forward hands over the LightningModule itself (second_stage/md17.py:221): its bound forward is the trusted case
            net = resolve_backbone(getattr(model, "forward", None))
        if net is not None and torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters()):
            raise RuntimeError("lam_slide_amd evaluates the stochastic-interpolant loss without gradients (the HIP path has no backward): call "
                               "training_losses under torch.no_grad() (as every validation_step does), or freeze the backbone")
        rows = self.si_rows(t)
        if net is not None and x1.is_cuda and x1.dtype == torch.float32 and x1.is_contiguous():
            self.last_path = "fused"
            return self._si_loss_fused(net, x1, t, x0, rows, model_kwargs)
        self.last_path = "generic"
        bshape = (x1.shape[0],) + (1,) * (x1.dim() - 1)
        alpha, sigma, p, q1, q0, w = (rows[:, i].to(x1).reshape(bshape) for i in range(6))
        xt = alpha * x1 + sigma * x0
        pred = model(xt, t, **model_kwargs)
        B, *_, Cc = xt.shape
        assert pred.size() == (B, *xt.size()[1:-1], Cc)
        r = p * pred + q1 * x1 + q0 * x0
        loss = w.reshape(-1) * (r ** 2).mean(dim=list(range(1, r.dim())))
        return {"pred": pred, "loss": loss, "xt": xt}

    def _si_loss_fused(self, net: "LatentSIV3", x1: Tensor, t: Tensor, x0: Tensor, rows: Tensor, model_kwargs: Dict[str, Any]) -> Dict[str, Tensor]:
        check_model_kwargs(model_kwargs)  # (where its tensors are: make_io below)
        dev = x1.device
        B = x1.shape[0]
        if tuple(x0.shape) != tuple(x1.shape) or tuple(t.shape) != (B,):
            raise ValueError(f"x0 must be shaped like x1 {tuple(x1.shape)} and t ({B},), got {tuple(x0.shape)} and {tuple(t.shape)}")
        same_device((("t", t), ("x0", x0)), dev, "x1")
        net.ensure_packed(dev)
        x1 = x1.detach()
        x0 = x0.detach().float().contiguous()
        tt = t.detach().float().contiguous()
        xt, pred = torch.empty_like(x1), torch.empty_like(x1)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        table = rows.contiguous().to(dev)
        io, keep = net.make_io(xt, model_kwargs["x_cond"], model_kwargs["x_cond_mask"], model_kwargs.get("y"), tt, pred)
        ws = net.workspace(io.B, io.T, io.L, dev, need=_lib.load().lsl_si_loss_workspace_bytes(net._handle, io.B, io.T, io.L))
        _lib.call(dev, "lsl_si_loss", net._handle, C.byref(io), x1.data_ptr(), x0.data_ptr(), table.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel())
        net.last_path = "hip"
        del keep
        return {"pred": pred, "loss": loss, "xt": xt}

    def training_losses(self, model: Callable, x1: Tensor, model_kwargs: Optional[Dict[str, Any]] = None, *, t: Optional[Tensor] = None,
                        x0: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """``Transport.training_losses`` of the reference (transport.py:116-156) evaluated without gradients: {"pred", "loss"} with ``loss``
        of shape [B].  ``t`` / ``x0`` (keyword only) fix the draws; whichever is missing comes from :meth:`sample`."""
        if t is None or x0 is None:
            td, x0d, _ = self.sample(x1)
            t = td if t is None else t
            x0 = x0d if x0 is None else x0
        out = self.si_loss(model, x1, t, x0, model_kwargs)
        return {"pred": out["pred"], "loss": out["loss"]}


def si_reduce(pred: Tensor, x1: Tensor, x0: Tensor, rows: Tensor) -> Tensor:
    """The reduction of the objective alone on the device (``lsl_si_reduce``): loss[b] = w_b mean((p_b pred + q1_b x1 + q0_b x0)^2) for
    contiguous float32 GPU tensors [B, ...] and a ``Transport.si_rows`` table.  Deterministic, and independent of the batch a trajectory
    is in."""
    if not pred.is_cuda:
        raise RuntimeError("si_reduce runs on the GPU (HIP kernel); there is no CPU fallback")
    B = pred.shape[0]
    per = pred[0].numel()
    for name, ten in (("pred", pred), ("x1", x1), ("x0", x0)):
        if ten.shape != pred.shape or ten.dtype != torch.float32 or not ten.is_contiguous() or ten.device != pred.device:
            raise ValueError(f"{name} must be a contiguous float32 tensor shaped like pred on pred's device")
    if tuple(rows.shape) != (B, 6):
        raise ValueError(f"rows must be [{B}, 6], got {tuple(rows.shape)}")
    dev = pred.device
    table = rows.float().contiguous().to(dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    scratch = torch.empty(B * ((per + _lib.SI_SLAB - 1) // _lib.SI_SLAB), dtype=torch.float32, device=dev)
    _lib.call(dev, "lsl_si_reduce", pred.data_ptr(), x1.data_ptr(), x0.data_ptr(), table.data_ptr(), B, per, loss.data_ptr(), scratch.data_ptr(),
              scratch.numel() * 4)
    return loss


def dot_rows(a: Tensor, b: Tensor) -> Tensor:
    """``out[i] = sum(a[i] * b[i])`` over everything behind the first axis, float64 [B], on the device (``lsl_dot_rows``): fp64 sums of the
    exact fp32 products in a fixed order, so a row's bits are the same alone and in any batch.  Contiguous float32 GPU tensors of one shape."""
    if not a.is_cuda:
        raise RuntimeError("dot_rows runs on the GPU (HIP kernel); there is no CPU fallback")
    if a.shape != b.shape or a.dim() < 1 or a.device != b.device or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("a and b must be float32 tensors of one shape on one device")
    a, b = a.contiguous(), b.contiguous()
    B = a.shape[0]
    per = a[0].numel()
    dev = a.device
    out = torch.empty(B, dtype=torch.float64, device=dev)
    scratch = torch.empty(B * ((per + _lib.SI_SLAB - 1) // _lib.SI_SLAB), dtype=torch.float64, device=dev)
    _lib.call(dev, "lsl_dot_rows", a.data_ptr(), b.data_ptr(), B, per, out.data_ptr(), scratch.data_ptr(), scratch.numel() * 8)
    return out


class CreateTransport:
    """Same keywords as the reference factory (transport/__init__.py:7-77); call it to get the Transport."""

    def __init__(self, path_type="Linear", prediction="velocity", loss_weight=None, train_eps=None, sample_eps=None):
        from . import dropin
        dropin.install()  # no-op unless a reference checkout's sampler modules are already imported (dropin.py)
        self.path_type = path_type
        self.prediction = prediction
        self.loss_weight = loss_weight
        self.train_eps = train_eps
        self.sample_eps = sample_eps

    def __call__(self) -> Transport:
        model_type = {"noise": ModelType.NOISE, "score": ModelType.SCORE, "data": ModelType.DATA}.get(self.prediction, ModelType.VELOCITY)
        loss_type = {"velocity": WeightType.VELOCITY, "likelihood": WeightType.LIKELIHOOD}.get(self.loss_weight, WeightType.NONE)
        path_type = {"Linear": PathType.LINEAR, "GVP": PathType.GVP, "VP": PathType.VP}[self.path_type]  # KeyError as the reference
        if path_type is PathType.VP:
            train_eps = 1e-5 if self.train_eps is None else self.train_eps
            sample_eps = 1e-3 if self.sample_eps is None else self.sample_eps
        elif model_type != ModelType.VELOCITY:
            train_eps = 1e-3 if self.train_eps is None else self.train_eps
            sample_eps = 1e-3 if self.sample_eps is None else self.sample_eps
        else:
            train_eps = 0
            sample_eps = 0
        return Transport(model_type=model_type, path_type=path_type, loss_type=loss_type, train_eps=train_eps, sample_eps=sample_eps)


def as_transport(obj) -> "Transport":
    """Accept the reference's own ``Transport`` object (src/modules/transport/transport.py:40-58) wherever this module wants one: a
    LightningModule built from the ORIGINAL ``transport._target_: src.modules.transport.CreateTransport`` hands ``Sampler`` such an
    object.  It is read by duck typing - enum member NAMES of ``model_type`` / ``loss_type``, the class name of ``path_sampler``
    (ICPlan / GVPCPlan / VPCPlan, path.py:21-206) - and restated as a :class:`Transport` with the same eps values."""
    if isinstance(obj, Transport):
        return obj
    try:
        model_type = ModelType[obj.model_type.name]
        loss_type = WeightType[getattr(getattr(obj, "loss_type", None), "name", "NONE")]
        if hasattr(obj, "path_type"):
            path_type = PathType[obj.path_type.name]
        else:
            path_type = {"ICPlan": PathType.LINEAR, "GVPCPlan": PathType.GVP, "VPCPlan": PathType.VP}[type(obj.path_sampler).__name__]
        return Transport(model_type=model_type, path_type=path_type, loss_type=loss_type, train_eps=obj.train_eps, sample_eps=obj.sample_eps)
    except (AttributeError, KeyError) as e:
        raise TypeError(f"cannot interpret {type(obj).__name__} as a stochastic-interpolant Transport: {e}") from None


_MASK64 = (1 << 64) - 1


def mix_seed(seed: int, index: int) -> int:
    """splitmix64 of (seed, index): the seed of call number ``index`` of an object seeded with ``seed``."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(index) + 1)) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def device_randn(shape, device, seed: int, elem_offset: int = 0) -> Tensor:
    """Standard-normal tensor from the library's counter stream (``lsl_randn``): element e of the result is global element
    ``elem_offset + e`` of stream ``seed``, so a rank that holds rows [lo, hi) of a batch draws exactly rows [lo, hi) of the
    unsharded draw.  Counterpart of ``torch.randn_like(x_cond)`` in lightning_base.py:231."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("device_randn draws on the GPU (HIP kernel); there is no CPU fallback")
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _lib.call(device, "lsl_randn", out.data_ptr(), out.numel(), int(seed) & _MASK64, int(elem_offset))
    return out


class SampleResult(Sequence):
    """What the fused samplers return: indexable like the reference's stacked tensor / list of states.
    ``[-1]`` (the only element the reference's callers read, lightning_base.py:230-234) is always there;
    earlier states only when the sampler was built with ``keep_trajectory=True``."""

    def __init__(self, final: Tensor, n: int, trace: Optional[Tensor] = None, first: Optional[Tensor] = None, offset: int = 0):
        self.final, self.n, self.trace, self.first, self.offset = final, n, trace, first, offset

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        if i < 0:
            i += self.n
        if i == self.n - 1:
            return self.final
        if not 0 <= i < self.n:
            raise IndexError(i)
        if self.trace is None:
            raise IndexError("intermediate states were not kept: build the sampler with keep_trajectory=True")
        if self.offset and i == 0:
            return self.first
        return self.trace[i - self.offset]


def _unwrap(mod):
    """``torch.compile`` wraps a module in an ``OptimizedModule`` that keeps the original as ``_orig_mod`` (the reference compiles its
    backbone when ``compile: True``, second_stage/md17.py:53-55).  The HIP path has nothing for a tracing compiler to do; the fused
    loop looks through the wrapper instead of silently losing the native path."""
    seen = 0
    while mod is not None and not isinstance(mod, LatentSIV3) and hasattr(mod, "_orig_mod") and seen < 4:
        mod = mod._orig_mod
        seen += 1
    return mod


def resolve_backbone(model: Callable) -> Optional[LatentSIV3]:
    model = _unwrap(model)
    if isinstance(model, LatentSIV3):
        return model
    tagged = _unwrap(getattr(model, "lsl_backbone", None))
    if isinstance(tagged, LatentSIV3):
        return tagged
    owner = _unwrap(getattr(model, "__self__", None))
    if isinstance(owner, LatentSIV3) and getattr(model, "__name__", "") in ("forward", "__call__"):
        return owner
    if owner is not None and getattr(model, "__name__", "") == "forward":
        inner = _unwrap(getattr(owner, "backbone", None))
        if isinstance(inner, LatentSIV3):
            return inner  # LightningModule.forward == backbone(x=xt, t=t, **kw) (lightning_base.py:173-174)
    return None


def same_device(named, dev, anchor: str) -> None:
    """The reference's device-mismatch error for the first of ``named`` = (name, tensor or None) pairs that is not on ``dev``, the device of
    what ``anchor`` names"""
    for name, ten in named:
        if ten is not None and ten.device != dev:
            raise RuntimeError(f"Expected all tensors to be on the same device, but {name} is on {ten.device} and {anchor} is on {dev}")


def check_model_kwargs(model_kwargs: Dict[str, Any], dev=None, then: Optional[Callable[[], Any]] = None) -> None:
    """The check of the conditioning every library path takes as ``model_kwargs``, in this order: unexpected keys, (``then()``: what a
    caller has always checked at this point,) missing ``x_cond`` / ``x_cond_mask``, and - given the state's device ``dev`` - tensors
    elsewhere."""
    extra = set(model_kwargs) - {"x_cond", "x_cond_mask", "y"}
    if extra:
        raise TypeError(f"unexpected model kwargs {sorted(extra)}")
    if then is not None:
        then()
    for name in ("x_cond", "x_cond_mask"):
        if name not in model_kwargs:
            raise TypeError(f"missing model kwarg {name!r}")
    if dev is not None:
        same_device(model_kwargs.items(), dev, "the state")


def stage_inputs(net: LatentSIV3, init: Tensor, model_kwargs: Dict[str, Any], dev, fresh: bool):
    """The state and the conditioning of a sampling call as the library takes them: (state, the call's lsl_io, what it keeps alive, replay).
    ``fresh``: the library updates the state in place, so it gets a private copy.  ``replay``: the library may replay the call as a hipGraph
    (``graph_replay_enabled``), so every input lies in a persistent buffer (see ``LatentSIV3.staged``)."""
    replay = net.graph_replay_enabled(tokens=int(init.shape[0]) * int(init.shape[1]) * int(init.shape[2]))
    x = net.staged("state", init, torch.float32, dev, fresh=fresh, persistent=replay)
    xc = net.staged("x_cond", model_kwargs["x_cond"], torch.float32, dev, persistent=replay)
    xm = net.staged("x_cond_mask", model_kwargs["x_cond_mask"], torch.int64, dev, persistent=replay)
    yv = model_kwargs.get("y")
    if yv is not None:
        yv = net.staged("y", yv, torch.float32, dev, persistent=replay)
    io, keep = net.make_io(x, xc, xm, yv)
    return x, io, keep, replay


def _dopri_head(each: bool, B: int, log_rows: int, logp: bool = False) -> Dict[str, Any]:
    """Where a device solve's caller finds things: the entry points' common name, ``last_path``, the record polled between chunks of
    attempts, and the offsets of the controller record(s), the log(s) and the state in the workspace (include/lsl_api.h).  ``logp``: the
    augmented solve of ``sample_ode_likelihood`` (``lsl_dopri_logp_*``: the same records at the same offsets)."""
    D = _lib.Dopri
    if each:
        head = {"entry": "lsl_dopri_each", "path": "dopri5-device-each", "polled": _lib.DopriEachSummary, "polled_at": D.EACH_SUMMARY_OFFSET,
                "ctl_at": D.EACH_CTL_OFFSET, "ctl_stride": D.EACH_CTL_STRIDE, "log_at": D.each_log_offset(B), "state_at": D.each_state_offset(B, log_rows)}
    else:
        head = {"entry": "lsl_dopri", "path": "dopri5-device", "polled": _lib.DopriCtl, "polled_at": D.CTL_OFFSET, "ctl_at": D.CTL_OFFSET, "ctl_stride": 0,
                "log_at": D.LOG_OFFSET, "state_at": D.STATE_OFFSET}
    if logp:
        head.update(entry="lsl_dopri_logp", path="likelihood-device-solve-each" if each else "likelihood-device-solve")
    return head


class Sampler:
    """``Sampler(transport)`` as in the reference (transport.py:229-244; rebuilt on every ``sample()`` call, lightning_base.py:219).

    Device noise (Euler-Maruyama steps without an explicit ``noise=`` tensor): every sampling CALL draws from a stream of its own, as
    the reference draws fresh ``randn`` per step and per call (integrators.py:30).  ``seed=None`` (default): the call's stream seed
    comes from torch's global generator, so ``torch.manual_seed`` / ``seed_everything`` make a run reproducible and consecutive calls
    differ.  ``seed=int``: call number k of this object uses ``mix_seed(seed, k)`` - reproducible by rebuilding the Sampler with the
    same seed."""

    def __init__(self, transport: Transport, fused: Optional[bool] = None, keep_trajectory: bool = False, seed: Optional[int] = None):
        self._given_transport = transport  # (as passed: the reference's Transport object when installed into a reference checkout)
        self.transport = as_transport(transport)
        self.fused = fused
        self.keep_trajectory = keep_trajectory
        self.seed = seed
        self.calls = 0
        self.last_seed: Optional[int] = None  # stream seed of the most recent fused call
        self.last_path: Optional[str] = None
        self.last_kernels: Optional[str] = None  # "general" | "resident" (lsl_sampler_path) after a fused call
        self.elem_offset = 0  # global element index of this rank's first state element (device noise stream)
        self._rk_ops: Dict[Any, "_RkOps"] = {}  # per device: the library's Runge-Kutta arithmetic (scratch buffers allocated once)
        self.ode_max_steps = 100000  # attempts (accepted + rejected) after which an adaptive solve gives up
        # controller="device": attempts enqueued between two reads of the controller record (the one synchronisation of a chunk).  Attempts
        # behind the one that finishes change nothing but each costs a whole attempt.  Measured (tools/dopri5_cost.py,
        # profiles/dopri5_cost.txt): at the peptide and md17 shapes an attempt is 4-6 ms of device work, 2 / 4 / 8 are within 0.3 % of
        # each other and at most 0.6 % ahead of 1 - so the smallest of them, whose idle attempt at the end of a call costs least
        self.attempts_per_poll = 2
        # step_control="trajectory": the rows of a trajectory's log that are kept (attempts beyond them are counted, not logged).  128 rows
        # are 4 KiB a trajectory - 16 MiB of workspace at B = 4096 - and more than twice the attempts of a solve at the default tolerances
        self.ode_log_rows = 128
        self.last_ode_stats: Optional[Dict[str, Any]] = None  # (step_control="trajectory": per-trajectory lists, "attempts", "network_passes")
        # controller="device": float64 [attempts, 4] rows (t, dt, ratio, accepted); step_control="trajectory": a list of B such tensors
        self.last_ode_log: Any = None
        self.last_ode_state: Optional[Tensor] = None  # controller="device": the state at the end of the last accepted step
        self.last_ode_logp_state: Optional[Tensor] = None  # sample_ode_likelihood(controller="device"): the logp part of that state, float32 [B]
        self.last_delta_logp: Optional[Tensor] = None  # sample_ode_likelihood: the integrated change of the log-density, [B] (logp = prior_logp(z) - it)

    def next_call_seed(self, draw: bool = True) -> int:
        """Seed of this call's device-noise stream.  The call counter advances on every call (ranks of a sharded run stay in step even
        when one of them has an empty shard); the global generator is consumed only when ``draw`` (the call really uses device noise)."""
        k = self.calls
        self.calls += 1
        if self.seed is None:
            return int(torch.randint(0, 1 << 62, (1,)).item()) if draw else 0
        return mix_seed(self.seed, k)

    # ---- step tables ------------------------------------------------------------------------------------
    def ode_steps(self, num_steps: int, reverse: bool = False) -> Tuple[List[Tuple[float, float, float, float]], Tensor]:
        tr = self.transport
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=reverse, last_step_size=0.0)
        assert t0 < t1, "ODE sampler has to be in forward time"
        grid = torch.linspace(t0, t1, num_steps)
        steps = []
        for i in range(num_steps - 1):
            ti = float(grid[i])
            dt = float(grid[i + 1] - grid[i])  # fp32 difference, as torchdiffeq's fixed grid forms it
            te = _f32(1 - ti) if reverse else ti
            vx, vm = tr.velocity_coeffs(te)
            steps.append((te, 1.0 + dt * vx, dt * vm, 0.0))
        return steps, grid

    def sde_drift_coeffs(self, t: float, diffusion_form: str, diffusion_norm: float) -> Tuple[float, float, float]:
        """(dx, dm, g): the SDE's drift at time t is dx x + dm net(x, t) - velocity plus g times the score - under the diffusion coefficient g"""
        tr = self.transport
        vx, vm = tr.velocity_coeffs(t)
        sx, sm = tr.score_coeffs(t)
        g = tr.schedule.diffusion(t, diffusion_form, diffusion_norm)
        return vx + g * sx, vm + g * sm, g

    def sde_steps(self, *, diffusion_form, diffusion_norm, last_step, last_step_size, num_steps):
        tr = self.transport
        if last_step is None:
            last_step_size = 0.0
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=diffusion_form, sde=True, eval=True, reverse=False,
                                   last_step_size=last_step_size)
        assert t0 < t1, "SDE sampler has to be in forward time"
        grid = torch.linspace(t0, t1, num_steps)
        dt = float(grid[1] - grid[0])
        sch = tr.schedule
        steps = []
        for i in range(num_steps - 1):
            ti = float(grid[i])
            dx, dm, g = self.sde_drift_coeffs(ti, diffusion_form, diffusion_norm)
            steps.append((ti, 1.0 + dt * dx, dt * dm, math.sqrt(2 * g) * math.sqrt(dt)))
        t1f = _f32(t1)
        if last_step is None:
            pass
        elif last_step == "Mean":
            dx, dm, _ = self.sde_drift_coeffs(t1f, diffusion_form, diffusion_norm)
            steps.append((t1f, 1.0 + last_step_size * dx, last_step_size * dm, 0.0))
        elif last_step == "Euler":
            vx, vm = tr.velocity_coeffs(t1f)
            steps.append((t1f, 1.0 + last_step_size * vx, last_step_size * vm, 0.0))
        elif last_step == "Tweedie":
            a = sch.alpha(t1f)[0]
            s = sch.sigma(t1f)[0]
            sx, sm = tr.score_coeffs(t1f)
            steps.append((t1f, 1.0 / a + s * s / a * sx, s * s / a * sm, 0.0))
        else:
            raise NotImplementedError()
        return steps, grid

    def heun_records(self, *, diffusion_form, diffusion_norm, last_step, last_step_size, num_steps):
        """Extended step records (``lsl_step_ex``: t, ax, am, aw, as, flags, noise slice, trace slice) of the stochastic Heun sampler
        (integrators.py:39-51) followed by the reference's last step.  drift(x, t) = a(t) x + b(t) net(x, t), so per step
            x_hat = x + sqrt(2 g(t) dt) w                       no network, state kept
            x_p   = (1 + dt a(t)) x_hat + dt b(t) net(x_hat, t)
            x'    = x_hat + dt/2 (K1 + K2) = x_hat / 2 + (1/2 + dt a(t')/2) x_p + dt b(t')/2 net(x_p, t'),   t' = t + dt
        (dt K1 = x_p - x_hat).  Returned with the EM table's last step appended (same last-step rule as Euler-Maruyama)."""
        em, grid = self.sde_steps(diffusion_form=diffusion_form, diffusion_norm=diffusion_norm, last_step=last_step,
                                  last_step_size=last_step_size, num_steps=num_steps)
        dt = float(grid[1] - grid[0])
        rec = []
        for i in range(num_steps - 1):
            ti = float(grid[i])
            tn = _f32(_f32(ti) + _f32(dt))  # t_cur + dt in fp32, as the reference forms it
            dx, dm, g = self.sde_drift_coeffs(ti, diffusion_form, diffusion_norm)
            dx2, dm2, _ = self.sde_drift_coeffs(tn, diffusion_form, diffusion_norm)
            rec.append((ti, 1.0, 0.0, math.sqrt(2 * g) * math.sqrt(dt), 0.0, _lib.STEP_NO_NETWORK | _lib.STEP_SAVE, i, -1))
            rec.append((ti, 1.0 + dt * dx, dt * dm, 0.0, 0.0, 0, 0, -1))
            rec.append((tn, 0.5 + 0.5 * dt * dx2, 0.5 * dt * dm2, 0.0, 0.5, 0, 0, i))
        if len(em) == num_steps:  # the last step (Mean / Euler / Tweedie)
            te, ax, am, _ = em[-1]
            rec.append((te, ax, am, 0.0, 0.0, 0, 0, num_steps - 1))
        return rec, grid

    # ---- fused execution ----------------------------------------------------------------------------------
    def run_fused(self, net: LatentSIV3, init: Tensor, steps, n_result: int, model_kwargs: Dict[str, Any],
                  noise: Optional[Tensor] = None, duplicate_last: bool = False, records=None) -> SampleResult:
        """``steps``: plain (t, ax, am, aw) records -> lsl_sample; ``records``: extended ones (heun_records) -> lsl_sample_ex, with
        ``steps`` then only giving the number of kept states."""
        dev = init.device
        check_model_kwargs(model_kwargs, dev, then=lambda: net._require_gpu(init))
        lib = _lib.load()
        # The call's noise-stream seed is drawn only when the call uses device noise (an Euler-Maruyama step without an explicit noise
        # tensor).  ODE calls and SDE calls with stored noise leave torch's global generator untouched, like the reference.
        table = records if records is not None else steps
        needs_device_noise = noise is None and any(s[3] != 0.0 for s in table)
        call_seed = self.next_call_seed(draw=needs_device_noise)
        self.last_seed = call_seed if needs_device_noise else None
        net.ensure_packed(dev)
        # the state is updated in place by the library: always a private copy
        x, io, keep, replay = stage_inputs(net, init, model_kwargs, dev, fresh=True)
        ws = net.workspace(io.B, io.T, io.L, dev)
        if records is None:
            arr = (_lib.Step * len(steps))(*[_lib.Step(*s) for s in steps])
        else:
            arr = (_lib.StepEx * len(records))(*[_lib.StepEx(*r) for r in records])
        trace = None
        if self.keep_trajectory:
            trace = torch.empty((len(steps),) + tuple(x.shape), dtype=torch.float32, device=dev)
        nz = None
        if noise is not None:  # slice s belongs to step s, like the reference's one draw per EM / Heun step
            nz = noise.detach().float().contiguous().to(dev)
            if records is None:
                need = max([i + 1 for i, s in enumerate(steps) if s[3] != 0.0], default=0)
            else:
                need = max([r[6] + 1 for r in records if r[3] != 0.0], default=0)
            if nz.shape[0] < need or tuple(nz.shape[1:]) != tuple(x.shape):
                raise ValueError(f"noise must be [>={need}, {tuple(x.shape)}], got {tuple(nz.shape)}")
        head = (net._handle, C.byref(io), arr, len(arr), nz.data_ptr() if nz is not None else None,
                nz.shape[0] if nz is not None else 0, call_seed, self.elem_offset, trace.data_ptr() if trace is not None else None)
        if records is None:
            _lib.call(dev, "lsl_sample", *head, ws.data_ptr(), ws.numel())
        else:  # (the library checks every record's trace slice against the slices the buffer really has)
            _lib.call(dev, "lsl_sample_ex", *head, trace.shape[0] if trace is not None else 0, ws.data_ptr(), ws.numel())
        net.last_path = "hip"
        self.last_path = "fused"
        # (extended records always run the general kernels: the trajectory-resident kernel implements the plain affine step only)
        self.last_kernels = "resident" if records is None and lib.lsl_sampler_path(net._handle, io.T, io.L) == 1 else "general"
        del keep
        if replay:
            x = x.clone()  # the persistent buffer is overwritten by the next call
        if x.dtype != init.dtype:
            x = x.to(init.dtype)
        if trace is None:
            return SampleResult(x, n_result)
        if duplicate_last:  # last_step=None: the reference appends xs[-1] again (transport.py:353-357)
            trace = torch.cat([trace, trace[-1:]], dim=0)
            return SampleResult(x, n_result, trace, None, 0)
        if n_result == len(steps) + 1:  # ODE: state 0 is the initial noise
            return SampleResult(x, n_result, trace, init, 1)
        return SampleResult(x, n_result, trace, None, 0)

    # ---- generic execution (any callable; mirrors integrators.py) -------------------------------------------
    def _vel(self, x, t, model, **kw):
        tr = self.transport
        out = model(x, t, **kw)
        tf = float(t.flatten()[0])
        vx, vm = tr.velocity_coeffs(tf)
        v = None
        if _lib.device_form(x, out) and out.shape == x.shape:
            # one library launch instead of three element-wise kernels; the same two rounded products and their rounded sum
            ops = self._rk_ops.get(x.device)
            if ops is None:
                try:
                    ops = _RkOps(x)
                except _lib.LibraryMissing:  # an arbitrary callable on a GPU needs no library: the torch expression below, same values
                    ops = False              # (remembered per device; HIP errors and out-of-memory conditions propagate)
                self._rk_ops[x.device] = ops
            if ops:
                v = ops.lincomb([(vx, x), (vm, out)])
        if v is None:
            v = vx * x + vm * out
        assert v.shape == x.shape, "Output shape from ODE solver must match input shape"
        return v, out

    def _sde_drift(self, x, t, model, form, norm, **kw):
        tr = self.transport
        v, out = self._vel(x, t, model, **kw)
        tf = float(t.flatten()[0])
        sx, sm = tr.score_coeffs(tf)
        g = tr.schedule.diffusion(tf, form, norm)
        return v + g * (sx * x + sm * out), g

    # ---- reference API --------------------------------------------------------------------------------------
    def sample_ode(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, reverse=False, controller="host", step_control="batch"):
        """``controller`` (this package's extra, adaptive ``dopri5`` only): ``"host"`` keeps the step controller in Python around the
        library's network and Runge-Kutta calls (:func:`dopri5_solve`); ``"device"`` runs the whole solve inside the library
        (``lsl_dopri_begin`` / ``lsl_dopri_advance``: controller state in device memory, attempts replayed as a hipGraph, the host reads the
        controller once per ``attempts_per_poll`` attempts) and needs a ``lam_slide_amd.LatentSIV3`` on a GPU behind ``model``.

        ``step_control`` (this package's extra, adaptive ``dopri5`` only): ``"batch"``, the default, is torchdiffeq's rule - one controller
        whose error norm runs over the whole state, so the steps of a trajectory depend on the batch it is sampled in.  ``"trajectory"``
        gives every trajectory (row of the initial state) a controller of its own - time, step size, decisions, error norm over that
        trajectory alone - and evaluates the network once per stage for all of them, at one time per trajectory: trajectory ``b`` of the
        call is the ``"batch"`` call on ``[b:b+1]``, bit for bit with ``controller="device"`` (``lsl_dopri_each_*``, ``last_path ==
        "dopri5-device-each"``) and exactly with ``controller="host"`` on CPU tensors (:func:`dopri5_solve_each`; ``model`` then receives
        a different time per row).  ``last_ode_stats`` holds per-trajectory lists of ``nfe`` / ``accepted`` / ``rejected``, ``attempts``
        (the largest count) and ``network_passes``; ``last_ode_log`` a list of per-trajectory logs of at most ``ode_log_rows`` rows.  A
        trajectory that fails (``ode_max_steps`` attempts, a non-finite error ratio) stops alone; the call raises once all have stopped
        and names the failed trajectories."""
        if controller not in ("host", "device"):
            raise ValueError(f"controller must be 'host' or 'device', got {controller!r}")
        if step_control not in ("batch", "trajectory"):
            raise ValueError(f"step_control must be 'batch' or 'trajectory', got {step_control!r}")
        if controller == "device" and sampling_method != "dopri5":
            raise ValueError(f"controller='device' is the adaptive dopri5 solver's; {sampling_method!r} has no step controller")
        if step_control == "trajectory" and sampling_method != "dopri5":
            raise ValueError(f"step_control='trajectory' is the adaptive dopri5 solver's; {sampling_method!r} has no step controller")
        if sampling_method == "dopri5" or sampling_method in FIXED_GRID_RK_METHODS:
            return self._sample_ode_dopri5(num_steps=num_steps, atol=atol, rtol=rtol, reverse=reverse, method=sampling_method, controller=controller,
                                           each=step_control == "trajectory")
        if sampling_method != "euler":
            # Other torchdiffeq solvers: not implemented here.  When this class stands in for the reference's Sampler (dropin.install) and
            # was given the reference's own Transport object, hand the call to the class it replaced instead of breaking a flow that worked
            # before the install.
            from . import dropin
            orig = dropin.original_sampler()
            if orig is not None and hasattr(self._given_transport, "get_drift"):
                return orig(self._given_transport).sample_ode(sampling_method=sampling_method, num_steps=num_steps, atol=atol, rtol=rtol,
                                                              reverse=reverse)
            raise NotImplementedError(f"ODE solver {sampling_method!r}: torchdiffeq's fixed-grid 'euler' / 'midpoint' / 'heun3' / 'rk4' and adaptive 'dopri5' are "
                                      "implemented (SURVEY.md 8c)")
        steps, grid = self.ode_steps(num_steps, reverse)

        def _sample(init, model, **model_kwargs):
            net = resolve_backbone(model) if self.fused is not False else None
            if net is not None and init.is_cuda:
                return self.run_fused(net, init, steps, num_steps, model_kwargs)
            if self.fused:
                raise RuntimeError("fused sampling requested but the model is not a lam_slide_amd.LatentSIV3 on a GPU")
            self.last_path = "generic"
            x = init
            xs = [x]
            for (te, _, _, _), i in zip(steps, range(num_steps - 1)):
                tv = torch.ones(x.size(0), device=x.device) * te
                v, _ = self._vel(x, tv, model, **model_kwargs)
                x = x + (grid[i + 1] - grid[i]).to(x.device) * v
                xs.append(x)
            return torch.stack(xs)

        return _sample

    def run_dopri_device(self, net: LatentSIV3, init: Tensor, grid: Sequence[float], rtol: float, atol: float, reverse: bool,
                         model_kwargs: Dict[str, Any]) -> Tensor:
        """The adaptive solve inside the library with one controller for the batch (``_run_dopri_device``)."""
        return self._run_dopri_device(net, init, grid, rtol, atol, reverse, model_kwargs, each=False)

    def run_dopri_device_each(self, net: LatentSIV3, init: Tensor, grid: Sequence[float], rtol: float, atol: float, reverse: bool,
                              model_kwargs: Dict[str, Any]) -> Tensor:
        """The adaptive solve inside the library with one controller per trajectory (``_run_dopri_device``)."""
        return self._run_dopri_device(net, init, grid, rtol, atol, reverse, model_kwargs, each=True)

    def _run_dopri_device(self, net: LatentSIV3, init: Tensor, grid: Sequence[float], rtol: float, atol: float, reverse: bool,
                          model_kwargs: Dict[str, Any], each: bool, logp: Optional[Dict[str, Any]] = None):
        """The adaptive solve inside the library: ``lsl_dopri[_each]_begin``, then ``lsl_dopri[_each]_advance`` in chunks of
        ``attempts_per_poll`` attempts with one read of the polled record (``_dopri_head``: the controller record, 128 bytes, or the summary
        of the per-trajectory form, 20 bytes - the one synchronisation) behind each, until it says done; then the controller record(s), the
        log(s) and the state.  Returns float32 [len(grid), *init.shape].

        Batch form: ``last_ode_stats`` holds the counters, ``last_ode_log`` a float64 [attempts, 4] tensor.  ``each``: per-trajectory lists
        ``nfe`` / ``accepted`` / ``rejected``, ``attempts`` (the largest count: the attempts the call ran) and ``network_passes``
        (evaluations of the network on the batch); ``last_ode_log`` a list of B float64 [min(attempts_b, ode_log_rows), 4] tensors;
        trajectories that failed are named in the error, raised once all have stopped.  ``last_ode_state``: the state (every trajectory's)
        at the end of the last accepted step.

        ``logp`` (``sample_ode_likelihood``): the augmented solve ``lsl_dopri_logp_*`` on ``[x | logp]`` with ``{"eps": the probe tensor or
        None, "seeds": one integer per trajectory where the probe is drawn on the device}``.  Returns ``(out, out_logp)``, float32
        [len(grid), *init.shape] and [len(grid), B]; ``last_ode_logp_state`` holds the logp part of the state beside ``last_ode_state``."""
        check_model_kwargs(model_kwargs, init.device)
        if int(self.attempts_per_poll) < 1:
            raise ValueError(f"attempts_per_poll must be at least 1, got {self.attempts_per_poll}")
        lib, dev = _lib.load(), init.device
        net.ensure_packed(dev)
        # (the solver state lives in the workspace: no private copy of the initial state)
        x, io, keep, _ = stage_inputs(net, init, model_kwargs, dev, fresh=False)
        D = _lib.Dopri
        B, n_out, log_rows = int(io.B), len(grid), int(self.ode_log_rows) if each else D.MAX_ATTEMPTS
        if each and not 0 <= log_rows <= D.MAX_ATTEMPTS:
            raise ValueError(f"ode_log_rows must be in 0..{D.MAX_ATTEMPTS}, got {self.ode_log_rows}")
        if each and B > D.EACH_MAX_B:
            raise ValueError(f"step_control='trajectory' takes at most {D.EACH_MAX_B} trajectories a call, got {B}")
        head = _dopri_head(each, B, log_rows, logp is not None)
        layout = (n_out, log_rows) if each else (n_out,)
        out = torch.empty((n_out,) + tuple(x.shape), dtype=torch.float32, device=dev)
        begin_args = (*layout[:1], out.data_ptr(), *layout[1:])
        if logp is not None:
            if B > D.EACH_MAX_B:
                raise ValueError(f"the likelihood solve takes at most {D.EACH_MAX_B} trajectories a call, got {B}")
            layout = (n_out, int(each), log_rows)
            out_logp = torch.empty((n_out, B), dtype=torch.float32, device=dev)
            probe = logp.get("eps")
            seeds = None
            if probe is not None:
                if tuple(probe.shape) != tuple(x.shape):
                    raise ValueError(f"eps must be shaped like the state {tuple(x.shape)}, got {tuple(probe.shape)}")
                same_device([("eps", probe)], dev, "the state")
                probe = probe.detach().to(torch.float32).contiguous()
            else:
                if len(logp["seeds"]) != B:
                    raise ValueError(f"probe_seeds must hold one integer per trajectory ({B}), got {len(logp['seeds'])}")
                wrapped = [(int(v) & _MASK64) - (1 << 64) if (int(v) & _MASK64) >> 63 else int(v) & _MASK64 for v in logp["seeds"]]
                seeds = torch.tensor(wrapped, dtype=torch.int64).to(dev)  # (the bits of the unsigned seeds)
            begin_args = (n_out, out.data_ptr(), out_logp.data_ptr(), int(each), log_rows, probe.data_ptr() if probe is not None else None,
                          seeds.data_ptr() if seeds is not None else None)
        ws = net.workspace(io.B, io.T, io.L, dev, need=getattr(lib, head["entry"] + "_workspace_bytes")(net._handle, io.B, io.T, io.L, *layout))
        desc, times = self._dopri_desc(grid, rtol, atol, reverse)

        def records(cls, at, count=1, stride=0):
            raw = _lib.to_host(ws[at:at + max(stride * count, C.sizeof(cls))]).tobytes()
            return [cls.from_buffer_copy(raw, stride * i) for i in range(count)]

        _lib.call(dev, head["entry"] + "_begin", net._handle, C.byref(io), C.byref(desc), times, *begin_args, ws.data_ptr(), ws.numel())
        polled, = records(head["polled"], head["polled_at"])
        while not polled.done:
            _lib.call(dev, head["entry"] + "_advance", net._handle, C.byref(io), int(self.attempts_per_poll), ws.data_ptr(), ws.numel())
            polled, = records(head["polled"], head["polled_at"])
        net.last_path = "hip"
        self.last_path = head["path"]
        if each:
            ctl = records(_lib.DopriCtl, head["ctl_at"], B, head["ctl_stride"])
            self.last_ode_stats = {"nfe": [c.nfe for c in ctl], "accepted": [c.accepted for c in ctl], "rejected": [c.rejected for c in ctl],
                                   "attempts": int(polled.max_attempts), "network_passes": 2 + 6 * int(polled.max_attempts)}
        else:  # (the polled record is the controller's)
            ctl = [polled]
            self.last_ode_stats = {"nfe": polled.nfe, "accepted": polled.accepted, "rejected": polled.rejected}
            log_rows = polled.accepted + polled.rejected  # (every attempt has its row: the rows to read)
        logs = [torch.zeros(0, 4, dtype=torch.float64) for _ in ctl]
        if log_rows:
            rows = _lib.to_host(ws[head["log_at"]:head["log_at"] + 32 * len(ctl) * log_rows])
            table = torch.from_numpy(rows.copy()).view(torch.float64).reshape(len(ctl), log_rows, 4)
            logs = [table[b, :min(c.accepted + c.rejected, log_rows)].clone() for b, c in enumerate(ctl)]
        self.last_ode_log = logs if each else logs[0]
        self.last_ode_state = ws[head["state_at"]:head["state_at"] + 4 * x.numel()].view(torch.float32).reshape(x.shape).clone()
        if logp is not None:
            side_at = D.logp_side_offset(head["state_at"], x.numel())
            self.last_ode_logp_state = ws[side_at:side_at + 4 * B].view(torch.float32).clone()
        del keep
        hit_limit = [b for b, c in enumerate(ctl) if c.status == D.STATUS_MAX_STEPS]
        non_finite = [b for b, c in enumerate(ctl) if c.status == D.STATUS_NON_FINITE]
        if each:
            failure = dopri_each_failure(hit_limit, non_finite)
        else:
            failure = DOPRI_MAX_STEPS_MESSAGE if hit_limit else DOPRI_NON_FINITE_MESSAGE if non_finite else None
        if failure:
            raise RuntimeError(failure)
        if logp is not None:
            return (out if out.dtype == init.dtype else out.to(init.dtype)), out_logp
        return out if out.dtype == init.dtype else out.to(init.dtype)

    def _dopri_desc(self, grid, rtol, atol, reverse):
        """The solver's description and output times as the library takes them"""
        tr = self.transport
        desc = _lib.DopriDesc(_lib.Dopri.PATHS[tr.path_type.name], _lib.Dopri.PREDICTIONS[tr.model_type.name], int(bool(reverse)),
                              min(int(self.ode_max_steps), _lib.Dopri.MAX_ATTEMPTS), float(rtol), float(atol))
        return desc, (C.c_double * len(grid))(*[float(g) for g in grid])

    def _sample_ode_dopri5(self, *, num_steps, atol, rtol, reverse, method="dopri5", controller="host", each=False):
        """The reference's default ODE sampler (transport.py:486-494, integrators.py:67-78 with method "dopri5"): adaptive steps, the solution
        reported at linspace(t0, t1, num_steps).  Every network evaluation runs on the HIP path (LatentSIV3.forward); the stage
        combinations and the error norm are a handful of element-wise device operations per step."""
        tr = self.transport
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=reverse, last_step_size=0.0)
        assert t0 < t1, "ODE sampler has to be in forward time"
        grid = [float(g) for g in torch.linspace(t0, t1, num_steps)]

        def _sample(init, model, **model_kwargs):
            if controller == "device":
                net = resolve_backbone(model)
                if net is None or not init.is_cuda:
                    raise RuntimeError("fused sampling requested but the model is not a lam_slide_amd.LatentSIV3 on a GPU")
                run = self.run_dopri_device_each if each else self.run_dopri_device
                return run(net, init, grid, rtol, atol, reverse, model_kwargs)
            self.last_path = method

            def f(t, x):
                tv = torch.ones(x.size(0), device=x.device) * (_f32(1 - t) if reverse else t)
                return self._vel(x, tv, model, **model_kwargs)[0]

            if each:
                self.last_path = "dopri5-each"

                def f_each(ts, x):  # one time per trajectory: the model on the batch, the drift row by row with each row's coefficients
                    tv = torch.tensor([_f32(1 - t) if reverse else t for t in ts], dtype=torch.float32, device=x.device)
                    out = model(x, tv, **model_kwargs)
                    return torch.cat([self._vel(x[b:b + 1], tv[b:b + 1], lambda *a, **k: out[b:b + 1])[0] for b in range(x.size(0))])

                stats = None
                try:
                    ys, stats = dopri5_solve_each(f_each, init, grid, rtol, atol, max_steps=self.ode_max_steps)
                except RuntimeError as err:
                    stats = getattr(err, "stats", None)
                    raise
                finally:
                    if stats is not None:
                        self.last_ode_log, self.last_ode_state = stats.pop("log"), stats.pop("state")
                        stats["network_passes"] = stats.pop("passes")
                        self.last_ode_stats = stats
                return torch.stack(ys)
            if method == "dopri5":
                ys, self.last_ode_stats = dopri5_solve(f, init, grid, rtol, atol, max_steps=self.ode_max_steps)
            else:  # (torchdiffeq's fixed-grid midpoint / heun3 / rk4: one step per output interval)
                ys = fixed_grid_rk_solve(f, init, grid, method)
            return torch.stack(ys)

        return _sample

    def _prior_logp_rows(self, z: Tensor) -> Tensor:
        """``Transport.prior_logp(z)`` for the forms of ``sample_ode_likelihood`` whose trajectories do not depend on the batch: on float32
        GPU tensors the sum of squares is ``dot_rows(z, z)`` - fp64, a fixed order per row - where a torch reduction may choose its order by
        the shape of the batch; the value, rounded once to ``z``'s dtype, is the same number to within that rounding."""
        if not _lib.device_form(z):
            return self.transport.prior_logp(z)
        try:
            sq = dot_rows(z, z)
        except _lib.LibraryMissing:  # (an arbitrary callable on a GPU needs no library)
            return self.transport.prior_logp(z)
        return (-0.5 * z[0].numel() * math.log(2.0 * math.pi) - sq / 2.0).to(z.dtype)

    def sample_ode_likelihood(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, eps=None, controller="host", step_control="batch",
                              probe_seeds=None):
        """``fn(x, model, **model_kwargs) -> (logp, z)`` as the reference's ``Sampler.sample_ode_likelihood`` (transport.py:413-473): the
        probability-flow ODE from the data ``x`` to the prior with the log-density change beside it, the divergence of the drift estimated by
        Hutchinson's ``eps . (J eps)`` with a Rademacher probe.  The drift is evaluated at ``1 - t``; the augmented right-hand side is
        ``(-drift, vx N + vm eps . j)`` with ``j = (d net / d x) eps`` and ``N`` the elements of a sample (the drift is ``vx x + vm net`` and
        ``eps_i = +-1``); ``z`` is the last state and ``logp = prior_logp(z) - delta_logp``.

        The augmented state is one flat vector ``[x.flatten() | logp]`` solved by :func:`dopri5_solve`, :func:`fixed_grid_rk_solve` or Euler
        steps on ``linspace(t0, t1, num_steps)``: torchdiffeq's flattening of a tuple state with equal tolerances (the RMS error norm runs over
        all ``B N + B`` elements).  ``eps`` (this package's extra): ``None`` draws ``torch.randint(2, x.size(), dtype=torch.float,
        device=x.device) * 2 - 1`` at every drift evaluation (the reference's draw, in its order); a tensor is used at every evaluation (a
        deterministic ODE); a callable ``(shape, device) -> Tensor`` is called at every evaluation.

        A ``lam_slide_amd.LatentSIV3`` on a GPU behind ``model`` (softmax attention, default form) runs the device path: one tangent pass of the
        library per evaluation (``LatentSIV3.jvp``) and ``lsl_dot_rows`` (``last_path == "likelihood-device"``); one the device path cannot
        serve raises ``NotImplementedError``.  Any other callable runs the reference's autograd expression in torch
        (``"likelihood-generic"``): autograd through ``model`` gives the divergence term of every evaluation; as in the reference (no
        ``create_graph``) the state, the drift and that term leave the evaluation detached, so ``logp`` carries no graph to the caller's
        parameters.  ``last_ode_stats["nfe"]`` counts the drift evaluations.

        ``controller`` / ``step_control`` (this package's extras, adaptive ``dopri5`` only; the defaults run the path above bit for bit), as
        in :meth:`sample_ode`.  ``step_control="trajectory"`` solves ``B`` vectors ``[x_b | logp_b]`` with a step controller each, so that a
        trajectory's ``logp`` does not depend on its batch companions; with ``controller="host"`` through :func:`dopri5_solve_each` (one time
        per row; in torch on CPU tensors and any callable).  ``controller="device"`` runs the whole augmented solve inside the library
        (``lsl_dopri_logp_*``, DESIGN.md 6.2.1: a tangent pass per evaluation, the controller in device memory; ``last_path ==
        "likelihood-device-solve"`` / ``"likelihood-device-solve-each"``): trajectory ``b`` of the per-trajectory call has the bits of the
        batch-form call on ``[b:b+1]``.  It takes ``eps`` as a tensor or ``None`` - then the probe of trajectory ``b`` is drawn on the
        device from ``probe_seeds[b]`` (one integer per trajectory; default ``mix_seed(next_call_seed(), b)``), its evaluation count and
        the element's index, so it does not depend on the batch either; a callable ``eps`` raises ``NotImplementedError``.
        ``last_ode_stats`` / ``last_ode_log`` / ``last_ode_state`` (and ``last_ode_logp_state``) are filled as by :meth:`sample_ode`."""
        tr = self.transport
        fixed = sampling_method in FIXED_GRID_RK_METHODS
        if controller not in ("host", "device"):
            raise ValueError(f"controller must be 'host' or 'device', got {controller!r}")
        if step_control not in ("batch", "trajectory"):
            raise ValueError(f"step_control must be 'batch' or 'trajectory', got {step_control!r}")
        if controller == "device" and sampling_method != "dopri5":
            raise ValueError(f"controller='device' is the adaptive dopri5 solver's; {sampling_method!r} has no step controller")
        if step_control == "trajectory" and sampling_method != "dopri5":
            raise ValueError(f"step_control='trajectory' is the adaptive dopri5 solver's; {sampling_method!r} has no step controller")
        if controller == "device" and callable(eps):
            raise NotImplementedError("sample_ode_likelihood(controller='device') takes eps as a tensor or None (drawn on the device): a callable "
                                      "probe would need the host at every evaluation")
        each = step_control == "trajectory"
        if sampling_method not in ("dopri5", "euler") and not fixed:
            raise NotImplementedError(f"ODE solver {sampling_method!r}: 'euler', 'midpoint', 'heun3', 'rk4' and adaptive 'dopri5' are implemented")
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
        grid = [float(g) for g in torch.linspace(t0, t1, num_steps)]

        def draw(xs: Tensor) -> Tensor:
            if eps is None:
                return torch.randint(2, xs.size(), dtype=torch.float, device=xs.device) * 2 - 1
            e = eps(tuple(xs.shape), xs.device) if callable(eps) else eps
            if tuple(e.shape) != tuple(xs.shape):
                raise ValueError(f"eps must be shaped like the state {tuple(xs.shape)}, got {tuple(e.shape)}")
            return e

        def _solve_each(x, model, net, model_kwargs):
            """The host restatement of the per-trajectory augmented solve: :func:`dopri5_solve_each` on rows ``[x_b | logp_b]``, one time per
            row, the right-hand side of ``rhs`` below row by row with each row's coefficients"""
            B, shape, n_el = x.shape[0], tuple(x.shape), x[0].numel()
            wide = (B,) + (1,) * (x.dim() - 1)

            def rhs_each(ts: Sequence[float], state: Tensor) -> Tensor:
                xs = state[:, :n_el].reshape(shape)
                tfs = [_f32(1.0 - t) for t in ts]
                tv = torch.tensor(tfs, dtype=torch.float32, device=x.device)
                try:
                    coeffs = [tr.velocity_coeffs(tf) for tf in tfs]
                except ZeroDivisionError:
                    raise ZeroDivisionError(f"sample_ode_likelihood: the {tr.path_type.name} path with {tr.model_type.name} prediction has no finite "
                                            f"velocity at one of the times {tfs} (sigma = 0 there; the reference's expression returns NaN): its "
                                            f"interval [{t0}, {t1}] evaluates the drift at 1 - t") from None
                e = draw(xs)
                if net is not None:
                    e = e.to(device=x.device, dtype=torch.float32)
                    out, jt = net.jvp(xs.contiguous(), tv, model_kwargs["x_cond"], model_kwargs["x_cond_mask"], model_kwargs.get("y"), tangent=e)
                    dots = dot_rows(e, jt)
                    drift = torch.cat([vx * xs[b:b + 1] + vm * out[b:b + 1] for b, (vx, vm) in enumerate(coeffs)])
                    dlogp = torch.cat([(vx * n_el + vm * dots[b:b + 1]).to(state.dtype) for b, (vx, vm) in enumerate(coeffs)])
                else:
                    e = e.to(xs)
                    vx = torch.tensor([c[0] for c in coeffs], dtype=xs.dtype, device=xs.device).reshape(wide)
                    vm = torch.tensor([c[1] for c in coeffs], dtype=xs.dtype, device=xs.device).reshape(wide)
                    with torch.enable_grad():
                        xg = xs.detach().requires_grad_(True)
                        drift = vx * xg + vm * model(xg, tv.to(xs.dtype), **model_kwargs)
                        grad = torch.autograd.grad(torch.sum(drift * e), xg)[0]
                    dlogp = torch.stack([torch.sum(grad[b] * e[b]) for b in range(B)])
                    drift = drift.detach()
                return torch.cat([-drift.reshape(B, n_el), dlogp.reshape(B, 1).to(state.dtype)], dim=1)

            y0 = torch.cat([x.detach().reshape(B, n_el), torch.zeros(B, 1, dtype=x.dtype, device=x.device)], dim=1)
            stats = None
            try:
                ys, stats = dopri5_solve_each(rhs_each, y0, grid, rtol, atol, max_steps=self.ode_max_steps)
            except RuntimeError as err:
                stats = getattr(err, "stats", None)
                raise
            finally:
                if stats is not None:
                    self.last_ode_log, state = stats.pop("log"), stats.pop("state")
                    self.last_ode_state, self.last_ode_logp_state = state[:, :n_el].reshape(shape), state[:, n_el]
                    stats["network_passes"] = stats.pop("passes")
                    self.last_ode_stats = stats
            z = ys[-1][:, :n_el].reshape(shape).contiguous()
            self.last_delta_logp = ys[-1][:, n_el]
            return self._prior_logp_rows(z) - ys[-1][:, n_el], z

        def _sample_fn(x, model, **model_kwargs):
            B, shape, n_el = x.shape[0], tuple(x.shape), x[0].numel()
            net = resolve_backbone(model)
            if net is not None:
                if x.is_cuda:
                    net.ensure_packed(x.device)  # (the handle's forms - LSL_TAIL / LSL_LN_FUSE defaults included - exist once it does)
                why = "the state is not on a GPU" if not x.is_cuda else net.jvp_supported()
                if why is None and not _lib.device_form(x):
                    why = "the state must be float32 and must not require grad (the tangent pass is forward mode without a tape)"
                if why is not None:
                    raise NotImplementedError(f"sample_ode_likelihood on a lam_slide_amd.LatentSIV3 needs the library's tangent pass: {why}")
                check_model_kwargs(model_kwargs)  # (where its tensors are: LatentSIV3.jvp)
            if controller == "device":
                if net is None:
                    raise RuntimeError("fused sampling requested but the model is not a lam_slide_amd.LatentSIV3 on a GPU")
                seeds = None
                if eps is None:
                    call_seed = self.next_call_seed() if probe_seeds is None else None
                    seeds = [mix_seed(call_seed, b) for b in range(B)] if probe_seeds is None else [int(v) for v in probe_seeds]
                out, out_logp = self._run_dopri_device(net, x.detach(), grid, rtol, atol, True, model_kwargs, each=each, logp={"eps": eps, "seeds": seeds})
                z = out[-1]
                self.last_delta_logp = out_logp[-1]
                return self._prior_logp_rows(z) - out_logp[-1].to(z.dtype), z
            self.last_path = ("likelihood-device" if net is not None else "likelihood-generic") + ("-each" if each else "")
            if each:
                return _solve_each(x, model, net, model_kwargs)
            count = [0]

            def rhs(t: float, state: Tensor) -> Tensor:
                count[0] += 1
                xs = state[:B * n_el].reshape(shape)
                tf = _f32(1.0 - t)
                tv = torch.full((B,), tf, dtype=torch.float32, device=x.device)
                try:
                    vx, vm = tr.velocity_coeffs(tf)
                except ZeroDivisionError:
                    raise ZeroDivisionError(f"sample_ode_likelihood: the {tr.path_type.name} path with {tr.model_type.name} prediction has no finite "
                                            f"velocity at time {tf} (sigma = 0 there; the reference's expression returns NaN): its interval "
                                            f"[{t0}, {t1}] evaluates the drift at 1 - t") from None
                e = draw(xs)
                if net is not None:
                    out, jt = net.jvp(xs.contiguous(), tv, model_kwargs["x_cond"], model_kwargs["x_cond_mask"], model_kwargs.get("y"),
                                      tangent=e.to(device=x.device, dtype=torch.float32))
                    drift = vx * xs + vm * out
                    dlogp = (vx * n_el + vm * dot_rows(e.to(device=x.device, dtype=torch.float32), jt)).to(state.dtype)
                else:
                    e = e.to(xs)
                    with torch.enable_grad():
                        xg = xs.detach().requires_grad_(True)
                        drift = vx * xg + vm * model(xg, tv.to(xs.dtype), **model_kwargs)
                        grad = torch.autograd.grad(torch.sum(drift * e), xg)[0]
                    dlogp = torch.sum(grad * e, dim=tuple(range(1, xs.dim())))
                    drift = drift.detach()
                return torch.cat([-drift.reshape(-1), dlogp.reshape(-1).to(state.dtype)])

            y0 = torch.cat([x.detach().reshape(-1), torch.zeros(B, dtype=x.dtype, device=x.device)])
            if sampling_method == "dopri5":
                ys, stats = dopri5_solve(rhs, y0, grid, rtol, atol, max_steps=self.ode_max_steps)
                last = ys[-1]
                self.last_ode_stats = dict(stats)
            elif fixed:
                last = fixed_grid_rk_solve(rhs, y0, grid, sampling_method)[-1]
            else:
                last = y0
                for ta, tb in zip(grid[:-1], grid[1:]):
                    last = last + (tb - ta) * rhs(ta, last)
            if sampling_method != "dopri5":
                self.last_ode_stats = {"nfe": count[0], "accepted": len(grid) - 1, "rejected": 0}
            z = last[:B * n_el].reshape(shape)
            delta_logp = last[B * n_el:]
            self.last_delta_logp = delta_logp
            return tr.prior_logp(z) - delta_logp, z

        return _sample_fn

    def sample_sde(self, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean",
                   last_step_size=0.04, num_steps=250, noise: Optional[Tensor] = None):
        if sampling_method not in ("Euler", "Heun"):
            raise NotImplementedError("Smapler type not implemented.")
        if last_step not in (None, "Mean", "Tweedie", "Euler"):
            raise NotImplementedError()
        steps, grid = self.sde_steps(diffusion_form=diffusion_form, diffusion_norm=diffusion_norm, last_step=last_step,
                                     last_step_size=last_step_size, num_steps=num_steps)
        dt = grid[1] - grid[0]
        records = None
        if sampling_method == "Heun":
            records, _ = self.heun_records(diffusion_form=diffusion_form, diffusion_norm=diffusion_norm, last_step=last_step,
                                           last_step_size=last_step_size, num_steps=num_steps)

        def _sample(init, model, **model_kwargs):
            net = resolve_backbone(model) if self.fused is not False else None
            if net is not None and init.is_cuda:
                return self.run_fused(net, init, steps, num_steps, model_kwargs, noise=noise, duplicate_last=last_step is None,
                                      records=records)
            if self.fused:
                raise RuntimeError("fused sampling requested but unavailable for this model / solver")
            self.last_path = "generic"
            x = init
            xs = []
            for i in range(num_steps - 1):
                ti = grid[i]
                w = noise[i].to(x) if noise is not None else torch.randn(x.size()).to(x)
                dw = w * torch.sqrt(dt).to(x)
                tv = torch.ones(x.size(0)).to(x) * ti.to(x)
                if sampling_method == "Euler":
                    d, g = self._sde_drift(x, tv, model, diffusion_form, diffusion_norm, **model_kwargs)
                    x = x + d * dt.to(x) + math.sqrt(2 * g) * dw
                else:
                    g = self.transport.schedule.diffusion(float(ti), diffusion_form, diffusion_norm)
                    xhat = x + math.sqrt(2 * g) * dw
                    k1, _ = self._sde_drift(xhat, tv, model, diffusion_form, diffusion_norm, **model_kwargs)
                    xp = xhat + dt.to(x) * k1
                    k2, _ = self._sde_drift(xp, tv + dt.to(x), model, diffusion_form, diffusion_norm, **model_kwargs)
                    x = xhat + 0.5 * dt.to(x) * (k1 + k2)
                xs.append(x)
            if last_step is None:
                xs.append(xs[-1])
            else:
                te, ax, am, _ = steps[-1]
                tv = torch.ones(init.size(0), device=x.device) * te
                out = model(xs[-1], tv, **model_kwargs)
                xs.append(ax * xs[-1] + am * out)
            assert len(xs) == num_steps, "Samples does not match the number of steps"
            return xs

        return _sample

    def get_sample_fn(self, sampling_method: str = "ODE", sampling_kwargs: Dict[str, Any] = {}):
        sde_kwargs = {"sampling_method": "Euler", "diffusion_form": "linear", "diffusion_norm": 1.0, "last_step": "Mean",
                      "last_step_size": 0.04, "num_steps": 250}
        ode_kwargs = {"sampling_method": "dopri5", "num_steps": 50, "atol": 1e-6, "rtol": 1e-3, "reverse": False}
        if sampling_method == "SDE":
            sde_kwargs.update(sampling_kwargs)
            return self.sample_sde(**sde_kwargs)
        if sampling_method == "ODE":
            ode_kwargs.update(sampling_kwargs)
            return self.sample_ode(**ode_kwargs)
        return None
