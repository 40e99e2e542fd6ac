"""CPU tests of the adaptive ODE sampler's ``controller`` keyword (lam_slide_amd/transport.py) and of the binding of lsl_dopri_*: the
keyword's dispatch and errors, the header's records against their ctypes mirrors, and the exact solution the GPU suite measures the device
solve against (tests/test_hip_dopri5.py), checked here with the host solver and a callable."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT


def exact_solution(c, x0, t0, t, reverse=False):
    """The state at solver time ``t`` of the GVP / data transport around a network that returns the constant ``c``, from ``x0`` at ``t0``.
    Forward: the drift is (sigma'/sigma) x + (alpha' - alpha sigma'/sigma) c, so x = alpha(t) c + sigma(t) / sigma(t0) (x0 - alpha(t0) c).
    Reverse (the drift evaluated at u = 1 - t, not negated): with h = pi u / 2, (cos(h) g)' = pi / 2 in t gives the particular solution
    g(u) c, g = -h / cos(h), and the homogeneous one 1 / cos(h): x = g(u) c + cos(h0) / cos(h) (x0 - g(u0) c)."""
    if not reverse:
        a, s = (lambda v: math.sin(v * math.pi / 2)), (lambda v: math.cos(v * math.pi / 2))
        return a(t) * c + s(t) / s(t0) * (x0 - a(t0) * c)
    h, h0 = (1 - t) * math.pi / 2, (1 - t0) * math.pi / 2
    g = lambda v: -v / math.cos(v)  # noqa: E731
    return g(h) * c + math.cos(h0) / math.cos(h) * (x0 - g(h0) * c)


def solver_norm(a, b, rtol, atol):
    """The distance of two states in the controller's own norm: sqrt(mean(((a - b) / (atol + rtol max(|a|, |b|)))^2))"""
    a, b = a.double(), b.double()
    return float(((a - b) / (atol + rtol * torch.maximum(a.abs(), b.abs()))).pow(2).mean().sqrt())


def _sampler(path="GVP", pred="data"):
    from lam_slide_amd import CreateTransport, Sampler
    return Sampler(CreateTransport(path, pred)())


@pytest.mark.parametrize("reverse", [False, True])
def test_exact_solution_of_the_constant_network(reverse):
    """The formula the GPU suite uses, against dopri5_solve at tight tolerances with the drift of Sampler._vel around a constant network."""
    from lam_slide_amd.transport import _f32, dopri5_solve
    s = _sampler()
    g = torch.Generator().manual_seed(0)
    c, x0 = torch.randn(1, 2, 3, 4, generator=g, dtype=torch.float64), torch.randn(1, 2, 3, 4, generator=g, dtype=torch.float64)
    model = lambda x, t, **kw: c  # noqa: E731
    grid = [0.05, 0.3, 0.55, 0.95]

    def f(t, x):
        tv = torch.ones(x.size(0), dtype=torch.float64) * (_f32(1 - t) if reverse else t)
        return s._vel(x, tv, model)[0]

    ys, stats = dopri5_solve(f, x0, grid, 1e-9, 1e-12)
    assert stats["accepted"] > 10
    for t, y in zip(grid, ys):
        assert solver_norm(y, exact_solution(c, x0, grid[0], t, reverse), 1e-6, 1e-9) < 1.0, t


def test_controller_keyword_dispatch_on_the_cpu():
    s = _sampler()
    g = torch.Generator().manual_seed(1)
    init, cond = torch.randn(2, 3, 4, 5, generator=g), torch.randn(2, 3, 4, 5, generator=g)
    model = lambda x, t, **kw: 0.3 * x + kw["x_cond"] * t.reshape(-1, 1, 1, 1)  # noqa: E731
    with pytest.raises(RuntimeError, match="not a lam_slide_amd.LatentSIV3 on a GPU"):
        s.get_sample_fn("ODE", dict(controller="device", num_steps=4))(init, model, x_cond=cond)
    plain = s.get_sample_fn("ODE", dict(num_steps=4))(init, model, x_cond=cond)
    assert s.last_path == "dopri5"
    host = s.get_sample_fn("ODE", dict(num_steps=4, controller="host"))(init, model, x_cond=cond)
    assert s.last_path == "dopri5" and torch.equal(plain, host) and plain.shape == (4, 2, 3, 4, 5)
    with pytest.raises(ValueError, match="controller"):
        s.get_sample_fn("ODE", dict(controller="gpu"))
    with pytest.raises(ValueError, match="dopri5"):
        s.get_sample_fn("ODE", dict(controller="device", sampling_method="euler"))
    assert torch.equal(s.get_sample_fn("ODE", dict(sampling_method="euler", num_steps=4, controller="host"))(init, model, x_cond=cond)[-1],
                       s.get_sample_fn("ODE", dict(sampling_method="euler", num_steps=4))(init, model, x_cond=cond)[-1])


def test_host_solver_honours_the_attempt_limit():
    s = _sampler("Linear", "velocity")
    s.ode_max_steps = 2
    model = lambda x, t, **kw: torch.sin(40 * t.reshape(-1, 1)) * x  # noqa: E731
    with pytest.raises(RuntimeError, match="max_steps reached"):
        s.get_sample_fn("ODE", dict(num_steps=3))(torch.ones(1, 4), model)


def test_header_records_and_constants_match_the_binding():
    """lsl_dopri_desc / lsl_dopri_ctl field for field (order and C type) against the ctypes structures, the offsets and enums against
    ``_lib.Dopri`` - the wrapper reads the controller record by these."""
    from lam_slide_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "float *": C.c_void_p}

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(int32_t|double|float \*)\s*(.+)", decl, re.S)
            assert m, decl
            out += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
        return out

    assert fields("lsl_dopri_desc") == list(_lib.DopriDesc._fields_)
    assert fields("lsl_dopri_ctl") == list(_lib.DopriCtl._fields_)
    assert C.sizeof(_lib.DopriCtl) <= _lib.Dopri.LOG_OFFSET - _lib.Dopri.CTL_OFFSET
    macro = lambda n: int(eval(re.search(r"#define %s ([\d\s()+*A-Z_]+)$" % n, header, re.M).group(1).replace("LSL_DOPRI_MAX_ATTEMPTS", str(_lib.Dopri.MAX_ATTEMPTS))))  # noqa: E731
    assert macro("LSL_DOPRI_MAX_ATTEMPTS") == _lib.Dopri.MAX_ATTEMPTS
    assert (macro("LSL_DOPRI_CTL_OFFSET"), macro("LSL_DOPRI_LOG_OFFSET"), macro("LSL_DOPRI_STATE_OFFSET")) == (
        _lib.Dopri.CTL_OFFSET, _lib.Dopri.LOG_OFFSET, _lib.Dopri.STATE_OFFSET)
    enums = {k: int(v) for k, v in re.findall(r"\b(LSL_(?:PATH|PRED|DOPRI)_[A-Z_]+) = (\d+)", header)}
    assert {k[len("LSL_PATH_"):]: v for k, v in enums.items() if k.startswith("LSL_PATH_")} == _lib.Dopri.PATHS
    assert {k[len("LSL_PRED_"):]: v for k, v in enums.items() if k.startswith("LSL_PRED_")} == _lib.Dopri.PREDICTIONS
    assert (enums["LSL_DOPRI_MAX_STEPS"], enums["LSL_DOPRI_NON_FINITE"]) == (_lib.Dopri.STATUS_MAX_STEPS, _lib.Dopri.STATUS_NON_FINITE)
    from lam_slide_amd.transport import ModelType, PathType
    assert set(_lib.Dopri.PATHS) == {p.name for p in PathType} and set(_lib.Dopri.PREDICTIONS) == {m.name for m in ModelType}


def test_refused_calls_enqueue_nothing_and_say_why():
    """Argument checks of lsl_dopri_* that need no device: null pointers, a decreasing grid, limits (the pointers are never dereferenced)."""
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    assert lib.lsl_dopri_workspace_bytes(None, 1, 1, 1, 1) == 0
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    io = _lib.IO(p, p, p, None, None, None, 1, 2, 3)
    grid = (C.c_double * 2)(0.5, 0.25)
    desc = _lib.DopriDesc(1, 1, 0, 10, 1e-3, 1e-6)
    assert lib.lsl_dopri_begin(None, C.byref(io), C.byref(desc), grid, 2, p, p, 1 << 30, None) == -3 and "non-decreasing" in _lib.last_error()
    grid = (C.c_double * 2)(0.25, 0.5)
    desc.max_steps = _lib.Dopri.MAX_ATTEMPTS + 1
    assert lib.lsl_dopri_begin(None, C.byref(io), C.byref(desc), grid, 2, p, p, 1 << 30, None) == -3 and "max_steps" in _lib.last_error()
    desc.max_steps, desc.path_type = 10, 7
    assert lib.lsl_dopri_begin(None, C.byref(io), C.byref(desc), grid, 2, p, p, 1 << 30, None) == -3
    desc.path_type = 1
    assert lib.lsl_dopri_begin(None, C.byref(io), C.byref(desc), grid, 2, p, p, 1 << 30, None) == -1  # (no model)
    assert lib.lsl_dopri_advance(None, C.byref(io), 1, p, 1 << 30, None) == -1
    assert lib.lsl_debug_dopri_coeffs(3, 0, p, 1, p, None) == -3
