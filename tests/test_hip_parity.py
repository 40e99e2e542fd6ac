"""GPU parity tests: the HIP path (through the C ABI, via lam_slide_amd) against the CPU oracle and the
committed golden vectors.

Tolerances (relative L2 unless noted).  Every bar is about 5x the value measured on MI355X in round 2 (gpurun log excerpt in
profiles/r02_parity.txt; conftest.parity prints "PARITY name measured bar" so both are on record); the north-star bar of
BASELINE.json (decoded coordinates within 1e-3) is 4-25x looser than any of them.
  * fp32-only kernels (conditioning vector, modulation tables): measured 5-7e-7, bar 5e-6
  * one block update with bf16 MFMA operands against the reference's own intermediates: measured 3-4e-3 of the UPDATE, bar 1e-2
  * one network evaluation: measured 0.3-1.4e-4, bars 4-6e-4
  * samplers end to end: final latents measured 0.4-2.4e-4, bars 6e-4..1e-3; decoded coordinates measured 2.6-5.9e-5, bars 1.5-3e-4
  * fp32 stage-1 encode / decode: measured 2.4-3.8e-7, bar 2e-6 (every head tile, key limit and remainder path: test_hip_stage1.py)
  * attention kernels per row against an fp64 softmax of the tapped bf16 q | k | v (test_hip_attention.py, attention_cases.py): per element
    2^-6 A for the MFMA forms (A = p |v|; three bf16 roundings of 2^-8 A each, bar four), 2^-8 |o| + (S + head_dim + 16) 2^-23 A for
    k_attention_tiny and, with A_lin, for k_attention_linear: derived, not measured (profiles/attention_rowwise_parity.txt)
  * LayerNorm + modulate, linear1, linear2 and k_tail per element against fp64 references built from the tapped bf16 operands
    (test_hip_gemm.py, gemm_cases.py): one rounding to bf16 (half a unit in the last place) + (K + 2) 2^-24 sum |w x| of accumulation for
    a, q, k, v, GELU(mlp); |gate| (K2 + 3) 2^-24 sum |w z| + 2^-23 |h| for the residual update: derived, not measured
    (profiles/gemm_rowwise_parity.txt)
  * the fp32 frame - conditioning chain, embeddings, k_ln_inplace, STATS + k_ln_finalize, output head + state update - per element against
    fp64 references built from the tapped fp32 operands (test_hip_frame.py, frame_cases.py): (K + 3) 2^-24 sum |w x| + 2^-24 per added
    term for every chain, the LayerNorm statistics term without the bf16 rounding, |am| bar(m) + 2^-22 sum |terms| for the update;
    derived, with three measured constants (cosf / sinf, __expf, rsqrtf: 4 x the worst seen, at most 16 units of 2^-24)
    (profiles/frame_rowwise_parity.txt)
  * integer / indexing behaviour (sharding, chunking, batch independence, K-folding, graph replay): bit-exact
"""
import ctypes as C

import pytest
import torch

from conftest import parity, rel_l2, shape_from

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def build_net(sh, params, dev):
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=sh.depth, in_dim=sh.in_dim, hidden_size=sh.hidden_size, num_heads=sh.num_heads,
                     vec_in_dim=sh.vec_in_dim, mlp_ratio=sh.mlp_ratio, theta=sh.theta, normalize=sh.normalize,
                     share_weights=sh.share_weights, attention_mode=sh.attention_mode, reset_parameters=False)
    net.load_state_dict(params)
    return net.to(dev)


def test_library_loaded_and_fails_loudly_on_cpu(dev):
    from lam_slide_amd import LatentSIV3, _lib
    lib = _lib.load()
    assert lib.lsl_version() == _lib.ABI_VERSION == 6
    net = LatentSIV3(depth=1, in_dim=8, hidden_size=64, num_heads=4, reset_parameters=False)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 2, 3, 8), torch.zeros(1), torch.zeros(1, 2, 3, 8), torch.zeros(1, 2, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        LatentSIV3(depth=1, in_dim=8, hidden_size=65, num_heads=4)


def test_conditioning_vector_and_modulation_fp32(golden, dev):
    from lam_slide_amd import _lib
    f = golden("f1_block.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    net.ensure_packed(dev)
    lib = _lib.load()
    B, D = 2, sh.hidden_size
    modw = (6 * sh.depth + 2) * D
    t, y = f["t"].to(dev), f["y"].to(dev).contiguous()
    vec = torch.empty(B, D, device=dev)
    mods = torch.empty(B, modw, device=dev)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
    _lib.check(lib.lsl_debug_mods(net._handle, t.data_ptr(), y.data_ptr(), B, vec.data_ptr(), mods.data_ptr(), ws.data_ptr(),
                                  ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    taps = f.group("taps")
    parity("f1.vec", rel_l2(vec.cpu(), taps["vec"]), 5e-6)
    for i in range(sh.depth):
        parity(f"f1.mod{i}", rel_l2(mods[:, 6 * D * i:6 * D * (i + 1)].cpu(), taps[f"l{i}.mod"]), 5e-6)
    parity("f1.final_mod", rel_l2(mods[:, 6 * D * sh.depth:].cpu(), taps["final_mod"].reshape(B, 2 * D)), 5e-6)


def test_each_block_against_reference_intermediates(golden, dev):
    """Feed every sub-block the reference's own input state and compare the state it produces."""
    from lam_slide_amd import _lib
    f = golden("f1_block.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    net.ensure_packed(dev)
    lib = _lib.load()
    taps = f.group("taps")
    B, T, L, D = 2, 5, 6, sh.hidden_size
    from oracle import latent_net
    o_taps = {}
    latent_net.forward(f.group("p"), sh, f["x"], f["t"], f["x_cond"], f["mask"], f["y"], taps=o_taps)
    mods = torch.cat([taps[f"l{i}.mod"] for i in range(sh.depth)] + [taps["final_mod"].reshape(B, 2 * D)], dim=1).to(dev).contiguous()
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=dev)
    h_prev = o_taps["h0"]
    for i in range(sh.depth):
        g1 = taps[f"l{i}.mod"][:, 2 * D:3 * D][:, None, None, :]
        h_mid = h_prev + g1 * taps[f"l{i}.sp.out"].reshape(B, T, L, D)
        h_end = taps[f"l{i}.h"]
        for bi, (hin, hout) in ((2 * i, (h_prev, h_mid)), (2 * i + 1, (h_mid, h_end))):
            a = hin.to(dev).contiguous()
            o = torch.empty_like(a)
            _lib.check(lib.lsl_debug_block(net._handle, bi, a.data_ptr(), o.data_ptr(), mods.data_ptr(), B, T, L, ws.data_ptr(),
                                           ws.numel(), torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            upd, want = o.cpu() - hin, hout - hin
            parity(f"f1.block{bi}.update", rel_l2(upd, want), 1e-2)
        h_prev = h_end


def test_forward_f1(golden, dev):
    f = golden("f1_block.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    out = net(f["x"].to(dev), f["t"].to(dev), f["x_cond"].to(dev), f["mask"].to(dev), f["y"].to(dev))
    assert net.last_path == "hip"
    parity("f1.forward", rel_l2(out.cpu(), f.group("taps")["out"]), 5e-4)


def test_forward_shape_classes(golden, dev):
    """hd 16 / 24 (padded) / 32, S in {2, 8, 30, 33, 40, 64}, normalize, y, shared weights, ragged tiles."""
    from oracle import latent_net
    f = golden("f2_shapes.npz")
    names = sorted({k.split("/")[0] for k in f.raw.files})
    for n in names:
        g = f.group(n)
        sh = shape_from({k[6:]: v for k, v in g.items() if k.startswith("shape.")})
        p = latent_net.random_params(sh, seed=int(g["weight_seed"]))
        net = build_net(sh, p, dev)
        y = g.get("y")
        out = net(g["x"].to(dev), g["t"].to(dev), g["x_cond"].to(dev), g["mask"].to(dev), y.to(dev) if y is not None else None)
        parity(f"f2.{n}", rel_l2(out.cpu(), g["out"]), 6e-4)


def test_linear_attention_mode_against_reference_outputs(golden, dev):
    """attention_mode="linear" (mmdit.py:58-72): F10 = outputs of the reference module built with that mode (hd 16 / 24 padded / 32, axes
    of 2 .. 300 positions, normalize, y)."""
    import dataclasses
    from lam_slide_amd import _lib
    from oracle import latent_net
    f = golden("f10_linear_attention.npz")
    for n in sorted({k.split("/")[0] for k in f.raw.files}):
        g = f.group(n)
        sh = dataclasses.replace(shape_from({k[6:]: v for k, v in g.items() if k.startswith("shape.")}), attention_mode="linear")
        net = build_net(sh, latent_net.random_params(sh, seed=int(g["weight_seed"])), dev)
        y = g.get("y")
        out = net(g["x"].to(dev), g["t"].to(dev), g["x_cond"].to(dev), g["mask"].to(dev), y.to(dev) if y is not None else None)
        parity(f"f10.{n}", rel_l2(out.cpu(), g["out"]), 6e-4)
        assert _lib.load().lsl_sampler_path(net._handle, 4, 2) == 0


@pytest.mark.parametrize("kw,T,L", [
    (dict(depth=1, in_dim=8, hidden_size=64, num_heads=4, mlp_ratio=2), 70, 6),                          # tile-GEMM linear1, 16-wide heads
    (dict(depth=1, in_dim=16, hidden_size=384, num_heads=16, mlp_ratio=4), 33, 2),                       # 24 -> 32 padded heads
    (dict(depth=1, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2), 3, 300),                      # token-stationary linear1, S > 256
    (dict(depth=1, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2, vec_in_dim=16), 20, 2),         # the trajectory-resident shape
], ids=["d64", "d384", "d512", "d128_resident_shape"])
def test_linear_attention_mode_stage_taps_and_sampler(kw, T, L, dev):
    """attention_linear stage by stage against the pinned oracle's taps (q / k WITHOUT the softmax pre-multiplier, the context product),
    then a 5-update Euler solve through lsl_sample (graph replay included) against the oracle's sampler."""
    from lam_slide_amd import _lib
    from oracle import harness, latent_net, transport as otr
    sh = latent_net.NetShape(**kw, attention_mode="linear")
    p = latent_net.random_params(sh, seed=41)
    net = build_net(sh, p, dev)
    net.ensure_packed(dev)
    B, C, D = 2, kw["in_dim"], kw["hidden_size"]
    g = torch.Generator().manual_seed(5)
    x, xc = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    mask = (torch.rand(B, T, L, generator=g) > 0.5).long()
    t = torch.rand(B, generator=g)
    y = torch.randn(B, sh.vec_in_dim, generator=g) if sh.vec_in_dim else None
    taps = {}
    latent_net.forward(p, sh, x, t, xc, mask, y, taps=taps)
    mods = torch.cat([taps[f"l{i}.mod"] for i in range(sh.depth)] + [taps["final_mod"].reshape(B, 2 * D)], dim=1).to(dev).contiguous()
    g1 = taps["l0.mod"][:, 2 * D:3 * D][:, None, None, :]
    h_states = [taps["h0"], taps["h0"] + g1 * taps["l0.sp.out"].reshape(B, T, L, D)]
    _check_stage_taps(f"linear_taps.{D}", net, _lib.load(), sh, taps, h_states, mods, B, T, L, dev,
                      dict(q=1.5e-2, k=1.5e-2, v=1.5e-2, attn=1.5e-2, gelu=1.5e-2))
    assert _lib.load().lsl_sampler_path(net._handle, T, L) == 0  # linear mode never takes the trajectory-resident kernel
    s = _sampler(net)
    fn = s.get_sample_fn("ODE", {"sampling_method": "euler", "num_steps": 6})
    kwargs = dict(x_cond=xc.to(dev), x_cond_mask=mask.to(dev), **({"y": y.to(dev)} if y is not None else {}))
    first = fn(x.to(dev), net.forward, **kwargs)[-1].cpu()
    again = fn(x.to(dev), net.forward, **kwargs)[-1].cpu()  # second appearance of the argument set: captured / replayed
    assert s.last_path == "fused" and torch.equal(first, again)
    want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), x, xc, mask, y, "ODE", {"sampling_method": "euler", "num_steps": 6})
    parity(f"linear_sample.{D}", rel_l2(first, want), 1e-3)


def _sampler(net, path="GVP", pred="data", **kw):
    from lam_slide_amd import CreateTransport, Sampler
    return Sampler(CreateTransport(path, pred)(), **kw)


def test_ode_samplers_against_reference_outputs(golden, dev):
    f = golden("f4_sampler.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    init, xc, mask = f["init"].to(dev), f["x_cond"].to(dev), f["mask"].to(dev)
    for n in (2, 11, 51):
        s = _sampler(net)
        res = s.get_sample_fn("ODE", {"sampling_method": "euler", "num_steps": n})(init, net.forward, x_cond=xc, x_cond_mask=mask)
        assert s.last_path == "fused" and len(res) == n
        parity(f"f4.ode{n}", rel_l2(res[-1].cpu(), f[f"ode{n}"]), 6e-4)
    for path, pred in (("Linear", "velocity"), ("Linear", "data"), ("VP", "noise"), ("GVP", "score")):
        s = _sampler(net, path, pred)
        res = s.get_sample_fn("ODE", {"sampling_method": "euler", "num_steps": 6})(init, net, x_cond=xc, x_cond_mask=mask)
        parity(f"f4.ode6.{path}.{pred}", rel_l2(res[-1].cpu(), f[f"ode6.{path}.{pred}"]), 6e-4)


def test_runge_kutta_arithmetic_kernels(dev):
    """lsl_rk_lincomb / lsl_rk_dense / lsl_rk_error_ratio (the state arithmetic of the adaptive sampler) against the same operations with torch
    ops: the combinations bit for bit (every term a rounded product added to the rounded running sum, in list order: what torch's
    element-wise kernels do), the error ratio against a float64 evaluation; odd sizes, one to eight terms, an aliased output."""
    from lam_slide_amd.transport import _RkOps, _f32
    g = torch.Generator().manual_seed(3)
    for n in (1, 257, 30 * 256 * 32 + 5):
        xs = [torch.randn(n, generator=g).to(dev) * (1 + j) for j in range(8)]
        ops = _RkOps(xs[0])
        assert ops.hip
        for n_terms in (1, 2, 5, 8):
            cs = [0.37 * (-1) ** j / (j + 1) for j in range(n_terms)]
            terms = list(zip(cs, xs[:n_terms]))
            want = xs[0] * _f32(cs[0])
            for c, x in terms[1:]:
                want = want + x * _f32(c)
            assert torch.equal(ops.lincomb(terms), want), (n, n_terms)
        a, b, c, d, e = xs[:5]
        x = 0.3125 + 1e-3
        xf = _f32(x)
        assert torch.equal(ops.poly4(a, b, c, d, e, x), e + xf * (d + xf * (c + xf * (b + xf * a))))
        terms = [(0.01, xs[2]), (-0.02, xs[3]), (0.005, xs[4])]
        err = (0.01 * xs[2].double() - 0.02 * xs[3].double() + 0.005 * xs[4].double())
        want = float((err / (1e-6 + 1e-3 * torch.maximum(xs[0].abs(), xs[1].abs()).double())).pow(2).mean().sqrt())
        got = ops.error_ratio(xs[0], xs[1], terms, 1e-6, 1e-3)
        assert got == ops.error_ratio(xs[0], xs[1], terms, 1e-6, 1e-3)  # deterministic
        parity(f"rk.error_ratio.n{n}", abs(got - want) / want, 2e-5)


def test_ode_dopri5_default_method_on_the_hip_network(golden, dev):
    """The reference's default ODE method (adaptive dopri5, transport.py:486-494) with every network evaluation on the HIP path, against
    the same solver driven by the pinned oracle network on the CPU.  torchdiffeq itself is absent (parity unpinned against it; the solver
    is checked against scipy and exact solutions in the CPU suite): two rtol = 1e-3 solves may choose different steps, so the bar is the
    solver tolerance, not the kernel rounding."""
    from oracle import latent_net
    f = golden("f4_sampler.npz")
    sh = shape_from(f.group("shape"))
    p = f.group("p")
    net = build_net(sh, p, dev)
    init, xc, mask = f["init"], f["x_cond"], f["mask"]
    oracle_model = lambda x, t, **kw: latent_net.forward(p, sh, x, t, kw["x_cond"], kw["x_cond_mask"], None)
    for path, pred in (("GVP", "data"), ("Linear", "velocity")):
        # (a) the reference's default tolerances: the two solves may accept / reject different steps, so they agree to the solver's
        #     tolerance class only; (b) ten times tighter (still above the bf16 network's own noise, ~ 1e-4: below it the error estimate
        #     of an adaptive solver is that noise): the solutions agree to the kernels' rounding
        for tag, kw, bar in (("default", {}, 3e-2), ("tight", {"rtol": 1e-4, "atol": 1e-7}, 5e-3)):
            s = _sampler(net, path, pred)
            res = s.get_sample_fn("ODE", dict(kw, num_steps=8))(init.to(dev), net, x_cond=xc.to(dev), x_cond_mask=mask.to(dev))
            assert s.last_path == "dopri5" and len(res) == 8 and net.last_path == "hip"
            so = _sampler(net, path, pred)
            want = so.get_sample_fn("ODE", dict(kw, num_steps=8))(init, oracle_model, x_cond=xc, x_cond_mask=mask)
            parity(f"f4.dopri5.{tag}.{path}.{pred}", rel_l2(res[-1].cpu(), want[-1]), bar)
            assert abs(s.last_ode_stats["accepted"] - so.last_ode_stats["accepted"]) <= 3 + so.last_ode_stats["accepted"] // 4


def test_ode_fixed_grid_runge_kutta_methods_on_the_hip_network(golden, dev):
    """torchdiffeq's other fixed-grid methods (midpoint, heun3, rk4; integrators.py:119 passes any `method` through): HIP network + library
    Runge-Kutta kernels against the same scheme driven by the pinned oracle network on the CPU (no step control: the two runs differ by the
    kernels' rounding only).  The 3/8 rule's last stage sits at y + dt (k1 - k2 + k3) - differences of network outputs that each carry the
    bf16 path's ~1e-3 error - so its bar is wider (2.6e-3 measured at five coarse steps)."""
    from oracle import latent_net
    from lam_slide_amd.transport import FIXED_GRID_RK_METHODS
    f = golden("f4_sampler.npz")
    sh = shape_from(f.group("shape"))
    p = f.group("p")
    net = build_net(sh, p, dev)
    init, xc, mask = f["init"], f["x_cond"], f["mask"]
    oracle_model = lambda x, t, **kw: latent_net.forward(p, sh, x, t, kw["x_cond"], kw["x_cond_mask"], None)
    for method in FIXED_GRID_RK_METHODS:
        s = _sampler(net, "GVP", "data")
        res = s.get_sample_fn("ODE", {"sampling_method": method, "num_steps": 6})(init.to(dev), net, x_cond=xc.to(dev), x_cond_mask=mask.to(dev))
        assert s.last_path == method and len(res) == 6 and net.last_path == "hip" and torch.equal(res[0].cpu(), init)
        want = _sampler(net, "GVP", "data").get_sample_fn("ODE", {"sampling_method": method, "num_steps": 6})(init, oracle_model, x_cond=xc, x_cond_mask=mask)
        parity(f"f4.{method}.GVP.data", rel_l2(res[-1].cpu(), want[-1]), 5e-3 if method == "rk4" else 1e-3)


def test_sde_samplers_with_stored_noise(golden, dev):
    f = golden("f4_sampler.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    init, xc, mask = f["init"].to(dev), f["x_cond"].to(dev), f["mask"].to(dev)
    for n, form, last in ((3, "linear", "Mean"), (10, "linear", "Mean"), (10, "SBDM", None), (6, "sigma", "Euler"), (6, "decreasing", "Tweedie")):
        tag = f"sde{n}.{form}.{last}.Euler"
        s = _sampler(net, keep_trajectory=True)
        fn = s.sample_sde(sampling_method="Euler", diffusion_form=form, last_step=last, num_steps=n, noise=f[tag + ".noise"].to(dev))
        res = fn(init, net.forward, x_cond=xc, x_cond_mask=mask)
        assert s.last_path == "fused" and len(res) == n
        parity(f"f4.{tag}.final", rel_l2(res[-1].cpu(), f[tag + ".final"]), 7e-4)
        parity(f"f4.{tag}.penultimate", rel_l2(res[-2].cpu(), f[tag + ".penultimate"]), 7e-4)
    # stochastic Heun (integrators.py:39-51): fused too (lsl_sample_ex: three extended records per step), against the reference's output;
    # the generic per-step loop (fused=False: the network alone on the HIP path) gives the same states
    tag = "sde5.linear.Mean.Heun"
    s = _sampler(net, keep_trajectory=True)
    fn = s.sample_sde(sampling_method="Heun", diffusion_form="linear", last_step="Mean", num_steps=5, noise=f[tag + ".noise"].to(dev))
    res = fn(init, net.forward, x_cond=xc, x_cond_mask=mask)
    assert s.last_path == "fused" and s.last_kernels == "general" and net.last_path == "hip" and len(res) == 5
    parity(f"f4.{tag}.final", rel_l2(res[-1].cpu(), f[tag + ".final"]), 7e-4)
    sg = _sampler(net, fused=False)
    gen = sg.sample_sde(sampling_method="Heun", diffusion_form="linear", last_step="Mean", num_steps=5, noise=f[tag + ".noise"].to(dev))(
        init, net.forward, x_cond=xc, x_cond_mask=mask)
    assert sg.last_path == "generic" and len(gen) == 5
    for i in range(5):
        parity(f"f4.{tag}.state{i}.fused_vs_generic", rel_l2(res[i].cpu(), gen[i].cpu()), 2e-4)
    # device noise: same seed -> same bits, and the sharded halves reproduce the whole batch (noise slice = Heun step, global element)
    def heun_dev(lo, hi, seed):
        sd = _sampler(net, seed=seed)
        sd.elem_offset = lo * init[0].numel()
        return sd.sample_sde(sampling_method="Heun", diffusion_form="linear", last_step="Mean", num_steps=5)(
            init[lo:hi], net.forward, x_cond=xc[lo:hi], x_cond_mask=mask[lo:hi])[-1]
    B = init.shape[0]
    whole = heun_dev(0, B, 3)
    assert torch.equal(whole, heun_dev(0, B, 3)) and not torch.equal(whole, heun_dev(0, B, 4))
    if B > 1:
        assert torch.equal(whole, torch.cat([heun_dev(0, 1, 3), heun_dev(1, B, 3)]))


def test_cfg1_decoded_coordinates(golden, dev):
    """BASELINE config 1 (T=30, L=192, D=256, H=16, depth 4; 10 Euler updates; batch 4): final latents decoded by the frozen stage-1
    decoder (oracle restatement, CPU) must match the reference path's own output (fixture F4_cfg1) within 1e-3 relative L2, at batch 1 and -
    through bit-equality of the trajectory inside a batch of 4 - at the stated batch."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    from oracle import harness, latent_net
    f = golden("f4_cfg1.npz")
    sh = shape_from(f.group("shape"))
    p = latent_net.random_params(sh, seed=int(f["weight_seed"]))
    net = build_net(sh, p, dev)
    lat = torch.randn(1, 30, 192, 32, generator=torch.Generator().manual_seed(int(f["latent_seed"])))
    init = torch.randn(1, 30, 192, 32, generator=torch.Generator().manual_seed(int(f["init_seed"])))
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=tuple(f["cond_idx"].tolist()), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": int(f["num_steps"])})
    got = drv.sample_latents(lat.to(dev), init=init.to(dev)).cpu()
    assert drv.last_sampler.last_path == "fused"
    want = f["final"]
    lat_err = rel_l2(got, want)
    d = golden("f6_decode.npz")
    ent = torch.arange(21)[None].expand(30, 21)
    pos_got = harness.decode(d.group("p"), harness.DecoderShape(), got[0], ent)
    pos_want = harness.decode(d.group("p"), harness.DecoderShape(), want[0], ent)
    pos_err = rel_l2(pos_got, pos_want)
    parity("cfg1.latents", lat_err, 5e-4)
    parity("cfg1.decoded_coords", pos_err, 3e-4)
    # BASELINE configs[0] as stated: batch = 4.  Trajectory 0 = the reference-pinned one above, three more beside it: its bits in the batch of 4
    # are those of the batch of 1 (so the reference comparison above holds for the batch-4 call), and every trajectory of the batch equals
    # the same trajectory sampled alone.
    g = torch.Generator().manual_seed(77)
    lat4 = torch.cat([lat, torch.randn(3, 30, 192, 32, generator=g)]).to(dev)
    init4 = torch.cat([init, torch.randn(3, 30, 192, 32, generator=g)]).to(dev)
    got4 = drv.sample_latents(lat4, init=init4).cpu()
    assert torch.equal(got4[0], got[0])
    for b in (1, 3):
        assert torch.equal(got4[b], drv.sample_latents(lat4[b:b + 1], init=init4[b:b + 1]).cpu()[0])


def test_batch_independence_and_chunking_bit_exact(dev):
    """Trajectories never mix: a batch, its halves, and any pass size give identical bits."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    from oracle import latent_net
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=3), dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(5, 12, 24, 32, generator=g).to(dev)
    init = torch.randn(5, 12, 24, 32, generator=g).to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 4), sampling_kwargs={"sampling_method": "euler", "num_steps": 5})
    full = drv.sample_latents(lat, init=init)
    net.set_chunk(2)
    chunked = drv.sample_latents(lat, init=init)
    net.set_chunk(0)
    parts = torch.cat([drv.sample_latents(lat[i:i + 1], init=init[i:i + 1]) for i in range(5)])
    assert torch.equal(full, chunked)
    assert torch.equal(full, parts)
    assert torch.isfinite(full).all()


def test_batch_independence_across_the_linear2_tiling_threshold_384(dev):
    """384-wide models (peptide family: linear2 K = 2 048 has no weight-stationary instance): linear2 runs the 192 x 128 tiling from about
    8 192 tokens per pass (host_launch.hip.h, gemm_variant 28) and the 128 x 128 one below.  The two must be bit-identical - "a trajectory's
    bits are the same in any batch" rests on it here: trajectory k of a 6-trajectory call (12 000 tokens: tiling 28) against the same
    trajectory sampled alone (2 000 tokens: tiling 11), and against passes of 2 (4 000 tokens)."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    from oracle import latent_net
    sh = latent_net.NetShape(depth=2, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4)
    net = build_net(sh, latent_net.random_params(sh, seed=13), dev)
    g = torch.Generator().manual_seed(4)
    lat = torch.randn(6, 1000, 2, 96, generator=g).to(dev)
    init = torch.randn(6, 1000, 2, 96, generator=g).to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 1), sampling_kwargs={"sampling_method": "euler", "num_steps": 3})
    full = drv.sample_latents(lat, init=init)
    for k in (0, 5):
        assert torch.equal(full[k:k + 1], drv.sample_latents(lat[k:k + 1], init=init[k:k + 1])), f"trajectory {k}: alone vs in the batch of 6"
    net.set_chunk(2)
    assert torch.equal(full, drv.sample_latents(lat, init=init)), "passes of 2 trajectories"
    net.set_chunk(0)
    assert torch.isfinite(full).all()


def test_batch_independence_across_the_linear1_wave_count_threshold_512(dev):
    """512-wide models: linear1 runs 4-wave workgroups on 128-token tiles up to 10 240 tokens per pass and 8-wave workgroups on 256-token
    tiles above (host_launch.hip.h, linear1_ts_waves; tools/lin1_harness.hip -DLIN1_NW=4 compares both with the tile kernel bit for
    bit).  Here through the sampler: trajectory k of a 3-trajectory call (23 040 tokens: 8 waves) against the same trajectory sampled alone
    (7 680 tokens - md17_bench B = 1 -: 4 waves), and a ragged length whose last 128-token tile is partial."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    from oracle import latent_net
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=17), dev)
    for T, L in ((30, 256), (7, 251)):
        g = torch.Generator().manual_seed(5)
        lat = torch.randn(3, T, L, 32, generator=g).to(dev)
        init = torch.randn(3, T, L, 32, generator=g).to(dev)
        drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 2), sampling_kwargs={"sampling_method": "euler", "num_steps": 3})
        full = drv.sample_latents(lat, init=init)
        if T * L * 3 > 10240:
            for k in (0, 2):
                assert torch.equal(full[k:k + 1], drv.sample_latents(lat[k:k + 1], init=init[k:k + 1])), f"trajectory {k}: alone vs in the batch of 3"
        else:  # (both sides on the 4-wave form; the 8-wave side through a batch large enough to cross the threshold)
            big = torch.cat([lat, lat]), torch.cat([init, init])
            assert torch.equal(full, drv.sample_latents(big[0], init=big[1])[:3]), "ragged length: 3 trajectories alone vs inside 6"
        assert torch.isfinite(full).all()


def test_pass_size_rule_equal_passes_under_the_token_cap(dev):
    """lsl_pass_size: a pass holds at most 256 Ki tokens, and a batch that needs several passes is cut into EQUAL ones (1024 trajectories of
    640 tokens: 342 + 342 + 340, not 409 + 409 + 206 - the short pass fills the chip worse); results do not depend on it (test above)."""
    from lam_slide_amd import _lib
    from oracle import latent_net
    sh = latent_net.NetShape(depth=1, in_dim=8, hidden_size=64, num_heads=4, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=1), dev)
    net.ensure_packed(dev)
    lib = _lib.load()
    ps = lambda B, T, L: lib.lsl_pass_size(net._handle, B, T, L)
    assert ps(32, 30, 256) == 32                     # the headline batch: one pass (245 760 tokens)
    assert ps(1024, 20, 8) == 1024                   # NBA: 163 840 tokens, one pass
    assert ps(1024, 80, 8) == 342                    # 640 tokens each: cap 409 -> three equal passes
    assert ps(35, 30, 256) == 18                     # cap 34 -> two passes of 18 + 17
    assert ps(3, 1000, 300) == 1                     # one trajectory above the cap still runs, alone
    for B, T, L in ((1024, 80, 8), (35, 30, 256), (1000, 7, 100)):
        c = ps(B, T, L)
        assert c * T * L <= 262144 and -(-B // c) == -(-B // (262144 // (T * L)))  # same number of passes as the plain cap would give


def test_device_noise_stream(dev):
    """Philox noise: reproducible, independent of how the batch is sharded (elem_offset), N(0,1) moments."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import latent_net
    sh = latent_net.NetShape(depth=1, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=4), dev)
    tr = CreateTransport("GVP", "data")()
    g = torch.Generator().manual_seed(0)
    init = torch.randn(4, 8, 16, 32, generator=g).to(dev)
    xc = torch.randn(4, 8, 16, 32, generator=g).to(dev)
    mask = torch.zeros(4, 8, 16, dtype=torch.long, device=dev)

    def run(lo, hi, seed=7):
        s = Sampler(tr, seed=seed)
        s.elem_offset = lo * 8 * 16 * 32
        fn = s.get_sample_fn("SDE", {"num_steps": 4})
        return fn(init[lo:hi], net.forward, x_cond=xc[lo:hi], x_cond_mask=mask[lo:hi])[-1]

    a, b = run(0, 4), run(0, 4)
    assert torch.equal(a, b)
    assert torch.equal(a, torch.cat([run(0, 2), run(2, 4)]))
    assert not torch.equal(a, run(0, 4, seed=8))
    # moments: one pure-noise step x <- 0*x + 0*m + 1*w
    from lam_slide_amd import _lib
    net.ensure_packed(dev)
    x = torch.zeros(8, 8, 64, 32, device=dev)
    io, keep = net.make_io(x, torch.zeros_like(x), torch.zeros(8, 8, 64, dtype=torch.long, device=dev), None)
    ws = net.workspace(8, 8, 64, dev)
    steps = (_lib.Step * 1)(_lib.Step(0.5, 0.0, 0.0, 1.0))
    _lib.check(_lib.load().lsl_sample(net._handle, C.byref(io), steps, 1, None, 0, 123, 0, None, ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert abs(float(x.mean())) < 0.02 and abs(float(x.std()) - 1.0) < 0.02
    assert abs(float((x ** 4).mean()) - 3.0) < 0.2


def test_error_behaviour_matches_reference(dev):
    from lam_slide_amd import CreateTransport, Sampler
    with pytest.raises(KeyError):
        CreateTransport("nope", "data")()
    s = Sampler(CreateTransport("GVP", "data")())
    with pytest.raises(NotImplementedError):
        s.sample_sde(sampling_method="RK4")
    with pytest.raises(NotImplementedError):
        s.sample_sde(diffusion_form="bogus")
    with pytest.raises(NotImplementedError):
        s.sample_sde(last_step="bogus")


# ---- the other BASELINE.json configurations (reduced batch; weights from oracle.random_params) -------------------------
CONFIG_SHAPES = {
    # name: (NetShape kwargs, B, T, L, cond frames, sampler, kwargs)
    "pedestrian": (dict(depth=6, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2, vec_in_dim=256, normalize=True), 40, 20, 2, 8, "ODE",
                   {"sampling_method": "euler", "num_steps": 11}),
    "nba": (dict(depth=6, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4, vec_in_dim=256, normalize=True), 24, 20, 8, 5, "ODE",
            {"sampling_method": "euler", "num_steps": 11}),
    "peptide_T300": (dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4), 2, 300, 2, 1, "SDE", {"num_steps": 6}),
    "peptide_T1000": (dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4), 1, 1000, 2, 1, "ODE",
                      {"sampling_method": "euler", "num_steps": 3}),
    "md17_ref": (dict(depth=4, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2), 2, 30, 192, 10, "ODE",
                 {"sampling_method": "euler", "num_steps": 4}),
}


@pytest.mark.parametrize("name", sorted(CONFIG_SHAPES))
def test_baseline_config_shapes(name, dev):
    """Every model family of BASELINE.json (head_dim 16 / 24 / 32, S from 2 to 1000, C = 32 / 96, class conditioning,
    normalize) through the fused sampler against the oracle, final latents within 3e-3 relative L2."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness, latent_net, transport as otr
    kw, B, T, L, cond, method, skw = CONFIG_SHAPES[name]
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=11)
    net = build_net(sh, p, dev)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, T, L, sh.in_dim, generator=g)
    init = torch.randn(B, T, L, sh.in_dim, generator=g)
    y = torch.randn(B, sh.vec_in_dim, generator=g) if sh.vec_in_dim else None
    xc, mask = harness.setup_conditioning(lat, (0, cond), True)
    mk = {"x_cond": xc.to(dev), "x_cond_mask": mask.to(dev)}
    if y is not None:
        mk["y"] = y.to(dev)
    s = Sampler(CreateTransport("GVP", "data")(), fused=True)
    if method == "SDE":
        n = skw["num_steps"]
        noise = torch.randn(n - 1, B, T, L, sh.in_dim, generator=g)
        got = s.sample_sde(**{"diffusion_form": "linear", "last_step": "Mean", **skw}, noise=noise.to(dev))(init.to(dev), net.forward, **mk)[-1]
        want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, mask, y, "SDE", skw, noise=list(noise), single_eval=True)
    else:
        got = s.get_sample_fn("ODE", skw)(init.to(dev), net.forward, **mk)[-1]
        want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, mask, y, "ODE", skw)
    assert s.last_path == "fused"
    parity(f"config.{name}.latents", rel_l2(got.cpu(), want), {"pedestrian": 1e-3, "nba": 9e-4}.get(name, 6e-4))


def test_k_sample_batching_equals_sequential_calls(dev):
    """K samples folded into the batch (one fused call, conditioning computed once) must reproduce K
    sequential sample() calls bit for bit."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    from oracle import latent_net
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2, vec_in_dim=16, normalize=True)
    net = build_net(sh, latent_net.random_params(sh, seed=8), dev)
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(3, 20, 2, 32, generator=g).to(dev)
    y = torch.randn(3, 16, generator=g).to(dev)
    inits = torch.randn(4, 3, 20, 2, 32, generator=g).to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 8), sampling_kwargs={"sampling_method": "euler", "num_steps": 6})
    batched = drv.sample_latents_k(lat, 4, y=y, inits=inits)
    assert drv.last_sampler.last_path == "fused" and batched.shape == (4, 3, 20, 2, 32)
    for k in range(4):
        assert torch.equal(batched[k], drv.sample_latents(lat, y=y, init=inits[k]))


def test_stage1_decode_against_reference_positions(golden, dev):
    """post_quant + Decoder on the HIP path against positions produced by the reference's own Decoder module
    (tests/golden/f6_decode.npz; the entity table holds rows above unit norm, so the max_norm clipping is exercised)."""
    from lam_slide_amd import Stage1Decoder
    d = golden("f6_decode.npz")
    dec = Stage1Decoder(d.group("p"), num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16, act="gelu_erf")
    pos = dec.decode(d["z"].to(dev), d["entities"].to(dev)).cpu()
    parity("f6.decode", rel_l2(pos, d["pos"]), 2e-6)
    # frames are independent: any subset decodes to the same bits
    part = dec.decode(d["z"][1:3].to(dev), d["entities"][1:3].to(dev)).cpu()
    assert torch.equal(part, pos[1:3])
    with pytest.raises(RuntimeError):
        dec.decode(d["z"], d["entities"])


def test_sample_then_decode_on_device(golden, dev):
    """The whole tail of SecondStageCondLightningBase.sample (lightning_base.py:230-238) on the device: fused sampler, then the
    HIP decoder; decoded coordinates against the reference latents decoded by the oracle must stay within 1e-3."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder
    from oracle import harness, latent_net
    f = golden("f4_cfg1.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, latent_net.random_params(sh, seed=int(f["weight_seed"])), dev)
    lat = torch.randn(1, 30, 192, 32, generator=torch.Generator().manual_seed(int(f["latent_seed"])))
    init = torch.randn(1, 30, 192, 32, generator=torch.Generator().manual_seed(int(f["init_seed"])))
    d = golden("f6_decode.npz")
    dec = Stage1Decoder(d.group("p"), num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16, act="gelu_erf")
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=tuple(f["cond_idx"].tolist()), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": int(f["num_steps"])}, decode=dec)
    final = drv.sample_latents(lat.to(dev), init=init.to(dev))
    ent = torch.arange(21)[None].expand(30, 21)
    pos = dec.decode(final[0], ent.to(dev)).cpu()
    want = harness.decode(d.group("p"), harness.DecoderShape(), f["final"][0], ent)
    parity("cfg1.sample_decode_on_device", rel_l2(pos, want), 3e-4)


def test_stage1_encode_against_reference_latents(golden, dev):
    """Encoder + quant on the HIP path against latents produced by the reference's own Encoder module with a ragged
    entity mask (tests/golden/f7_encode.npz)."""
    from lam_slide_amd import Stage1Encoder
    d = golden("f7_encode.npz")
    enc = Stage1Encoder(d.group("p"), num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16, act="gelu_erf")
    z = enc.encode(d["x"].to(dev), d["entities"].to(dev), d["mask"].to(dev)).cpu()
    parity("f7.encode", rel_l2(z, d["z"]), 2e-6)
    part = enc.encode(d["x"][1:2].to(dev), d["entities"][1:2].to(dev), d["mask"][1:2].to(dev)).cpu()
    assert torch.equal(part, z[1:2])
    # masked-out entities do not influence the latents
    x2 = d["x"].clone()
    x2[1, 15:] = 1e3
    z2 = enc.encode(x2.to(dev), d["entities"].to(dev), d["mask"].to(dev)).cpu()
    assert torch.equal(z2[1], z[1])


def test_stage1_decode_query_splitter_cross_block_tanh(golden, dev):
    """The peptide decoder variant (DecoderQuerySplitter: every latent expands to 4 context tokens through a 1x1 conv), with one
    latent<-query cross-attention block and the tanh GELU, against the reference module's positions (f8_decode_split.npz)."""
    from lam_slide_amd import Stage1Decoder
    d = golden("f8_decode_split.npz")
    dec = Stage1Decoder(d.group("p"), num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16, act="gelu_tanh")
    assert (dec.num_split, dec.num_block_cross) == (4, 1)
    pos = dec.decode(d["z"].to(dev), d["entities"].to(dev)).cpu()
    parity("f8.decode_split", rel_l2(pos, d["pos"]), 2e-6)


RANDOM_SHAPES = {
    # name: (NetShape kwargs, B, T, L)      edge cases beyond the reference-generated shape classes
    "one_token": (dict(depth=1, in_dim=8, hidden_size=64, num_heads=4, mlp_ratio=2), 1, 1, 1),
    "d320_hd32_odd_tiles": (dict(depth=2, in_dim=32, hidden_size=320, num_heads=10, mlp_ratio=2), 3, 7, 19),
    "d448_hd28_padded": (dict(depth=1, in_dim=16, hidden_size=448, num_heads=16, mlp_ratio=1), 2, 5, 9),
    "c96_d192": (dict(depth=2, in_dim=96, hidden_size=192, num_heads=12, mlp_ratio=4), 2, 33, 2),
    "long_axis_257": (dict(depth=1, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2), 1, 257, 3),
    "long_axis_300_y_norm": (dict(depth=1, in_dim=32, hidden_size=256, num_heads=8, mlp_ratio=2, vec_in_dim=24, normalize=True), 2, 3, 300),
    "c64_d512_ragged_tokens": (dict(depth=1, in_dim=64, hidden_size=512, num_heads=16, mlp_ratio=2), 5, 3, 21),
}


@pytest.mark.parametrize("name", sorted(RANDOM_SHAPES))
def test_forward_edge_shapes_vs_oracle(name, dev):
    """One network evaluation against the oracle (itself pinned to the reference) on shapes the shipped configs do not hit: a single
    token, odd k-tile / feature-tile counts, padded head widths, C up to 96, attended axes just above 256 (LDS tile limit of
    the short-sequence kernel), token counts that are not multiples of any tile."""
    from oracle import latent_net
    kw, B, T, L = RANDOM_SHAPES[name]
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=11)
    net = build_net(sh, p, dev)
    g = torch.Generator().manual_seed(5)
    x, xc = torch.randn(B, T, L, sh.in_dim, generator=g), torch.randn(B, T, L, sh.in_dim, generator=g)
    mask = (torch.rand(B, T, L, generator=g) < 0.4).long()
    t = torch.rand(B, generator=g)
    y = torch.randn(B, sh.vec_in_dim, generator=g) if sh.vec_in_dim else None
    want = latent_net.forward(p, sh, x, t, xc, mask, y)
    got = net(x.to(dev), t.to(dev), xc.to(dev), mask.to(dev), y.to(dev) if y is not None else None).cpu()
    assert net.last_path == "hip" and torch.isfinite(got).all()
    parity(f"edge.{name}", rel_l2(got, want), 4e-4)


@pytest.mark.parametrize("gain", [1.0, 2.5, 6.0], ids=["unit", "x2.5", "x6"])
def test_attention_softmax_shift_bound_and_fallback(gain, dev):
    """k_attention_rows shifts the softmax by the Cauchy-Schwarz bound |q| max|k| instead of the row maximum while that bound is <= 60
    (k_attn.hip.h); larger bounds take the max pass.  QK-norm scales multiplied by `gain` (both q and k: scores x gain^2) walk through
    the regimes: bound ~ 8 (shifted), ~ 50 (shifted, probabilities down to 2^-100), ~ 290 (max pass).  Axes of 40 and 300 positions
    run the short-sequence and the run-time-length instance."""
    from oracle import latent_net
    kw = dict(depth=1, in_dim=16, hidden_size=128, num_heads=4, mlp_ratio=2)
    B, T, L = 2, 300, 40
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=31)
    for k in p:
        if k.endswith("query_norm.scale") or k.endswith("key_norm.scale"):
            p[k] = p[k] * gain
    net = build_net(sh, p, dev)
    g = torch.Generator().manual_seed(9)
    x, xc = torch.randn(B, T, L, sh.in_dim, generator=g), torch.randn(B, T, L, sh.in_dim, generator=g)
    mask = (torch.rand(B, T, L, generator=g) < 0.4).long()
    t = torch.rand(B, generator=g)
    want = latent_net.forward(p, sh, x, t, xc, mask, None)
    got = net(x.to(dev), t.to(dev), xc.to(dev), mask.to(dev), None).cpu()
    assert torch.isfinite(got).all()
    # sharper softmaxes amplify the bf16 rounding of q and k (d softmax / d score ~ score range): the bar follows the gain
    parity(f"attn_shift.gain{gain}", rel_l2(got, want), 4e-4 * max(1.0, gain * gain / 2))


def test_full_chain_encode_sample_decode_on_device(golden, dev):
    """Everything SecondStageCondLightningBase.sample does after prepare_inputs (lightning_base.py:217-238 with second_stage/md17.py:
    115-131), on the device: Stage1Encoder -> setup_conditioning -> fused sampler -> Stage1Decoder, against the same chain on the
    oracle (each stage of which is pinned to the reference).  Decoded coordinates within the north-star bar."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder
    from oracle import harness, latent_net, transport as otr
    e, d = golden("f7_encode.npz"), golden("f6_decode.npz")
    enc = Stage1Encoder(e.group("p"), num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(d.group("p"), num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2)
    p = latent_net.random_params(sh, seed=21)
    net = build_net(sh, p, dev)
    B, T, A = 2, 6, 21
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B * T, A, 128, generator=g)                       # prepare_inputs output, one row of entities per frame
    ent = torch.stack([torch.randperm(32, generator=g)[:A] for _ in range(B * T)])
    mask = torch.ones(B * T, A, dtype=torch.bool)
    mask[:, 18:] = False
    init = torch.randn(B, T, 48, 32, generator=g)
    skw = {"sampling_method": "euler", "num_steps": 6}

    def encode(batch):
        z = enc.encode(batch["x"].to(dev), batch["entities"].to(dev), batch["mask"].to(dev))
        return z.reshape(B, T, *z.shape[1:])

    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 2), mask_cond_mean=True, sampling_kwargs=skw,
                             encode=encode, decode=dec)
    lat = drv.encode({"x": x, "entities": ent, "mask": mask})
    final = drv.sample_latents(lat, init=init.to(dev))
    pos = dec.decode(final.reshape(B * T, 48, 32), ent.to(dev)).cpu()

    lat_o = harness.encode(e.group("p"), harness.EncoderShape(num_latents=48), x, ent, mask).reshape(B, T, 48, 32)
    xc, m = harness.setup_conditioning(lat_o, (0, 2), True)
    final_o = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, m, None, "ODE", skw)
    pos_o = harness.decode(d.group("p"), harness.DecoderShape(), final_o.reshape(B * T, 48, 32), ent)
    err_lat, err_pos = rel_l2(final.cpu(), final_o), rel_l2(pos, pos_o)
    parity("chain.encoded", rel_l2(lat.cpu(), lat_o), 2e-6)
    parity("chain.sampled", err_lat, 4e-4)
    parity("chain.decoded", err_pos, 1.5e-4)


def test_f9_real_lightning_sample_on_device(golden, dev):
    """F9: what the reference's REAL LightningModule returned from `sample(batch)` (lightning_base.py:217-238 executed unchanged on the
    real second_stage/md17.py Wrapper in the build container; the fixture holds inputs, weights, the fixed initial noise and the decoded
    positions).  The same inputs through the drop-in on the device: Stage1Encoder -> setup_conditioning -> fused sampler -> Stage1Decoder."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder
    from oracle import latent_net
    f = golden("f9_sample.npz")
    B, T, A, L, c0, c1, n = (int(v) for v in f["meta"])
    s1 = f.group("stage1")
    enc = Stage1Encoder(s1, num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(s1, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=64, mlp_ratio=2, num_heads=4)
    net = build_net(sh, f.group("backbone"), dev)
    flat = lambda t: t.reshape(B * T, *t.shape[2:])  # noqa: E731

    def encode(batch):
        z = enc.encode(flat(batch["pos"]).to(dev), flat(batch["entities"]).to(dev), flat(batch["attention_mask"]).to(dev))
        return z.reshape(B, T, *z.shape[1:])

    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(c0, c1), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": n}, encode=encode, decode=dec)
    lat = drv.encode({"pos": f["x"], "entities": f["entities"], "attention_mask": f["attention_mask"]})
    parity("f9.encoded", rel_l2(lat.cpu(), f["latents"]), 2e-6)
    final = drv.sample_latents(lat, init=f["noise"].to(dev))
    assert drv.last_sampler.last_path == "fused"
    parity("f9.sampled", rel_l2(final.cpu(), f["final"]), 5e-4)
    pos = dec.decode(final.reshape(B * T, L, 32), flat(f["entities"]).to(dev)).cpu().reshape(f["pos"].shape)
    parity("f9.decoded", rel_l2(pos, f["pos"]), 3e-4)


def test_f11_real_pedestrian_k_sample_evaluation_on_device(golden, dev):
    """F11: what the reference's REAL pedestrian CondWrapper produced in the build container - `prepare_batch` (y = Embedding(cond_scene),
    second_stage/pedestrian.py:242-251) and the K = 20 `test_step` loop (:186-212: K sequential sample() calls, future frames, real agents,
    best-of-K ADE / FDE) - against the drop-in on the device at the true pedestrian shape (T = 20, L = 2: the trajectory-resident kernel):
    Stage1Encoder -> one fused K-sample call -> Stage1Decoder -> min_ade_fde (`best_of_k_errors`), with the fixture's K initial noises."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder
    from lam_slide_amd.sampling import best_of_k_errors
    from oracle import latent_net
    f = golden("f11_pedestrian_k.npz")
    B, T, A, L, K, c0, c1, n = (int(v) for v in f["meta"])
    sh = shape_from(f.group("shape"))
    net = build_net(sh, latent_net.random_params(sh, seed=int(f["weight_seed"])), dev)
    s1 = f.group("stage1")
    enc = Stage1Encoder(s1, num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(s1, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    flat = lambda t: t.reshape(-1, *t.shape[2:])  # noqa: E731
    pos = f["pos"].clone()
    pos[:, c1:] = 0  # (the reference hides the future frames from the encoder: :175-176)
    lat = enc.encode(flat(pos @ f["lift"]).to(dev), flat(f["entities"]).to(dev), flat(f["attention_mask"]).to(dev)).reshape(B, T, L, 32)
    y = f["embedding"].to(dev)[f["cond_scene"].long().to(dev)]  # CondWrapper.prepare_batch
    assert torch.equal(y.cpu(), f["y"])
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(c0, c1), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": n})
    ent = flat(f["entities"]).to(dev)
    seen = {}

    def decode(z):  # [K*B, T, L, C] -> [K*B, T, A, 3]
        seen["final"] = z
        p = dec.decode(z.reshape(-1, L, 32), ent.repeat(z.shape[0] // B, 1))
        seen["pos"] = p.reshape(z.shape[0], T, A, 3)
        return seen["pos"]

    ades, fdes = best_of_k_errors(drv, lat, f["true_future"].to(dev), K, decode, agent_mask=f["attention_mask"][:, -1].to(dev), y=y,
                                  inits=f["noises"].to(dev), num_runs=K)
    assert drv.last_sampler.last_path == "fused" and drv.last_sampler.last_kernels == "resident"
    parity("f11.finals", rel_l2(seen["final"].reshape(K, B, T, L, 32).cpu(), f["finals"]), 1e-3)
    parity("f11.positions", rel_l2(seen["pos"].reshape(K, B, T, A, 3).cpu(), f["positions"]), 5e-4)
    parity("f11.ade", rel_l2(ades.cpu(), f["ades"]), 5e-4)
    parity("f11.fde", rel_l2(fdes.cpu(), f["fdes"]), 5e-4)


def test_f12_real_nba_k_sample_evaluation_on_device(golden, dev):
    """F12: what the reference's REAL NBA CondWrapper produced in the build container - `prepare_batch` (second_stage/nba.py:254-263) and
    the `test_step` loop with the class defaults K = 60 / num_runs = 20 (:205-225, :229) - against the drop-in on the device at the NBA
    shape (T = 20, L = 8, hidden 256, 16 heads, mlp 4, class vector: the general kernels, per-trajectory modulation rows): Stage1Encoder ->
    ONE fused 60-sample call -> Stage1Decoder -> best-of-the-first-20 ADE / FDE, in the default and in the tail decomposition."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder
    from lam_slide_amd.sampling import best_of_k_errors
    from oracle import latent_net
    f = golden("f12_nba_k.npz")
    B, T, A, L, K, c0, c1, n, R = (int(v) for v in f["meta"])
    sh = shape_from(f.group("shape"))
    s1 = f.group("stage1")
    enc = Stage1Encoder(s1, num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(s1, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    flat = lambda t: t.reshape(-1, *t.shape[2:])  # noqa: E731
    pos = f["pos"].clone()
    pos[:, c1:] = 0  # (the reference hides the future frames from the encoder: :188-189)
    lat = enc.encode(flat(pos @ f["lift"]).to(dev), flat(f["entities"]).to(dev), flat(f["attention_mask"]).to(dev)).reshape(B, T, L, 32)
    y = f["embedding"].to(dev)[f["cond_scene"].long().to(dev)]  # CondWrapper.prepare_batch
    assert torch.equal(y.cpu(), f["y"])
    noises = torch.randn(K, B, T, L, 32, generator=torch.Generator().manual_seed(int(f["noise_seed"]))).to(dev)
    ent = flat(f["entities"]).to(dev)
    kept = [int(k) for k in f["kept"]]
    for tail in (False, True):
        net = build_net(sh, latent_net.random_params(sh, seed=int(f["weight_seed"])), dev)
        if tail:
            net.set_tail(True)
        drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(c0, c1), mask_cond_mean=True,
                                 sampling_kwargs={"sampling_method": "euler", "num_steps": n})
        seen = {}

        def decode(z):  # [K*B, T, L, C] -> [K*B, T, A, 3]
            seen["final"] = z
            p = dec.decode(z.reshape(-1, L, 32), ent.repeat(z.shape[0] // B, 1))
            seen["pos"] = p.reshape(z.shape[0], T, A, 3)
            return seen["pos"]

        ades, fdes = best_of_k_errors(drv, lat, f["true_future"].to(dev), K, decode, agent_mask=f["attention_mask"][:, -1].to(dev), y=y,
                                      inits=noises, num_runs=R)
        assert drv.last_sampler.last_path == "fused" and net.tail == tail
        tag = "f12.tail" if tail else "f12"
        parity(tag + ".finals", rel_l2(seen["final"].reshape(K, B, T, L, 32)[kept].cpu(), f["finals"]), 1e-3)
        parity(tag + ".positions", rel_l2(seen["pos"].reshape(K, B, T, A, 3)[kept].cpu(), f["positions"]), 5e-4)
        parity(tag + ".ade", rel_l2(ades.cpu(), f["ades"]), 5e-4)
        parity(tag + ".fde", rel_l2(fdes.cpu(), f["fdes"]), 5e-4)


def test_f13_real_peptide_wrapper_sample_on_device(golden, dev):
    """F13: what the reference's REAL peptide second-stage Wrapper produced in the build container at T = 1000 (`encode`, the base class's
    `sample`, `decode` to atom14 positions: second_stage/peptide.py:85-102, lightning_base.py:217-238) against the drop-in on the device:
    Stage1Encoder (2 latents of 96, no entity mask) -> one fused sampling call at the peptide shape (T = 1000: chunked-key temporal attention
    with the denominator column, packed L = 2 spatial attention, 24 -> 32 padded heads, the K2 = 2 048 linear2 tiling) -> Stage1Decoder with
    the query splitter and the 42-wide atom14 head.  Compared on the frames the fixture keeps (every 8th)."""
    from golden_inputs import peptide_frames
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder
    from oracle import latent_net
    f = golden("f13_peptide.npz")
    B, T, R, L, c0, c1, n = (int(v) for v in f["meta"])
    st = int(f["frame_stride"])
    sh = shape_from(f.group("shape"))
    net = build_net(sh, latent_net.random_params(sh, seed=int(f["weight_seed"])), dev)
    s1 = f.group("stage1")
    enc = Stage1Encoder(s1, num_head_cross=2, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(s1, num_head_latent=2, dim_head_latent=16, num_head_cross=2, dim_head_cross=16, output="atom14_pos")
    assert dec.num_split == 8 and dec.out_dim == 42
    batch = peptide_frames(int(f["batch_seed"]), B, T, R)
    flat = lambda t: t.reshape(-1, *t.shape[2:])  # noqa: E731
    x = flat(batch["atom14_pos"].flatten(-2) @ f["lift"]).to(dev)
    ent = flat(batch["entities"]).to(dev)
    lat = enc.encode(x, ent, None).reshape(B, T, L, 96)
    parity("f13.cond_latents", rel_l2(lat[:, :1].cpu(), f["cond_latents"]), 5e-4)
    noise = torch.randn(B, T, L, 96, generator=torch.Generator().manual_seed(int(f["noise_seed"]))).to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(c0, c1), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": n})
    final = drv.sample_latents(lat, init=noise)
    assert drv.last_sampler.last_path == "fused"
    parity("f13.finals", rel_l2(final[:, ::st].cpu(), f["finals"]), 1e-3)
    pos = dec.decode(final.reshape(B * T, L, 96), ent).reshape(B, T, R, 14, 3)
    parity("f13.atom14_positions", rel_l2(pos[:, ::st].cpu(), f["positions"]), 1e-3)


def test_graph_replay_matches_eager_bits(dev):
    """LSL_GRAPH=2: repeated sampling calls with the same buffers are captured into a hipGraph on their second appearance and replayed
    afterwards; results must be the bits of the eager path, also when the INPUT VALUES change between replays (the graph reads through
    the pointers).  The knob is read once per process, so both arms run in subprocesses."""
    import os
    import subprocess
    import sys
    code = (
        "import torch, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from lam_slide_amd import CreateTransport, SecondStageSampler\n"
        "from oracle import latent_net\n"
        "from test_hip_parity import build_net\n"
        "dev = torch.device('cuda:0')\n"
        "sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2)\n"
        "net = build_net(sh, latent_net.random_params(sh, seed=4), dev)\n"
        "drv = SecondStageSampler(net, CreateTransport('GVP', 'data')(), cond_idx=(0, 3), sampling_kwargs={'sampling_method': 'euler', 'num_steps': 7})\n"
        "g = torch.Generator().manual_seed(9)\n"
        "outs = []\n"
        "for i in range(5):\n"
        "    lat = torch.randn(3, 10, 6, 32, generator=g).to(dev); init = torch.randn(3, 10, 6, 32, generator=g).to(dev)\n"
        "    outs.append(drv.sample_latents(lat, init=init).cpu())\n"
        "torch.save(torch.stack(outs), sys.argv[1])\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("0", "2"):
        path = f"/tmp/lsl_graph_{mode}_{os.getpid()}.pt"
        env = dict(os.environ, LSL_GRAPH=mode)
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=600)
        res[mode] = torch.load(path)
        os.remove(path)
    assert torch.equal(res["0"], res["2"])
    assert not torch.equal(res["0"][0], res["0"][1])


def test_kernel_choice_knobs_do_not_change_bits(dev):
    """The knobs that pick between bit-identical kernel paths, exercised at the headline shape (T = 30, L = 256, D = 512: linear2 on the
    weight-stationary kernel k_linear2_ws, 18 trajectories = 138 240 tokens): LSL_LIN2_WS=0 (linear2 back on the 256 x 256-tile kernel),
    LSL_QKV_PLANES=0 (q / k / v as token-major rows) and the modulation tables computed per evaluation (LSL_MODS_GROUP=0) or in groups of
    two records (=2: the default computes all records of the call in one group) must reproduce the default run's bits.  The knobs are read
    once per process, so every arm runs in a subprocess."""
    import os
    import subprocess
    import sys
    code = (
        "import torch, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from lam_slide_amd import CreateTransport, SecondStageSampler\n"
        "from oracle import latent_net\n"
        "from test_hip_parity import build_net\n"
        "dev = torch.device('cuda:0')\n"
        "sh = latent_net.NetShape(depth=1, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2)\n"
        "net = build_net(sh, latent_net.random_params(sh, seed=11), dev)\n"
        "drv = SecondStageSampler(net, CreateTransport('GVP', 'data')(), cond_idx=(0, 10), sampling_kwargs={'sampling_method': 'euler', 'num_steps': 3})\n"
        "g = torch.Generator().manual_seed(5)\n"
        "lat = torch.randn(18, 30, 256, 32, generator=g).to(dev); init = torch.randn(18, 30, 256, 32, generator=g).to(dev)\n"
        "torch.save(drv.sample_latents(lat, init=init).cpu(), sys.argv[1])\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    arms = (("default", {}), ("tile_linear2", {"LSL_LIN2_WS": "0"}), ("token_major_qkv", {"LSL_QKV_PLANES": "0"}), ("mods_per_eval", {"LSL_MODS_GROUP": "0"}),
            ("mods_groups_of_2", {"LSL_MODS_GROUP": "2"}))
    for name, extra in arms:
        path = f"/tmp/lsl_knob_{name}_{os.getpid()}.pt"
        env = {k: v for k, v in os.environ.items() if k not in ("LSL_LIN2_WS", "LSL_QKV_PLANES", "LSL_MODS_GROUP")}
        env.update(extra)
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=900)
        res[name] = torch.load(path)
        os.remove(path)
    assert torch.isfinite(res["default"]).all()
    assert torch.equal(res["default"], res["tile_linear2"])
    assert torch.equal(res["default"], res["token_major_qkv"])
    assert torch.equal(res["default"], res["mods_per_eval"])
    assert torch.equal(res["default"], res["mods_groups_of_2"])


@pytest.mark.parametrize("kw,B,T,L", [
    (dict(depth=2, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2), 20, 30, 256),   # headline model: k_linear2_ws<1536>, stream attention LONG (planes) + SHORT
    (dict(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4), 300, 20, 8),    # NBA family: k_linear2_ws<1280> (5 chunks), SHORT with 16-wide heads
    (dict(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2), 9, 30, 192),    # MD17 reference shape: k_linear2_ws<768>, LONG with 16-wide heads
    (dict(depth=2, in_dim=32, hidden_size=384, num_heads=16, mlp_ratio=4), 3, 1000, 2),    # peptide family: chunked LONG (4 x 4 stages, denominator column), packed L = 2, tile linear2
], ids=["md17", "nba", "md17_ref", "peptide"])
def test_general_path_rerun_bits(kw, B, T, L, dev):
    """The round-4 kernels keep hand-counted vector-memory waits (LDS-DMA rings, hand-offs between waves through LDS): the same sampling
    call repeated 25 times must give the same bits every time (a miscounted wait shows as a timing-dependent difference, as the resident
    kernel's did in round 2)."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    from oracle import latent_net
    sh = latent_net.NetShape(**kw)
    net = build_net(sh, latent_net.random_params(sh, seed=11), dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 5), sampling_kwargs={"sampling_method": "euler", "num_steps": 4})
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, T, L, 32, generator=g).to(dev)
    init = torch.randn(B, T, L, 32, generator=g).to(dev)
    ref = drv.sample_latents(lat, init=init)
    assert torch.isfinite(ref).all()
    differing = sum(int(not torch.equal(drv.sample_latents(lat, init=init), ref)) for _ in range(25))
    assert differing == 0, differing


def test_attention_stream_kernel_against_rows_kernel(dev):
    """k_attention_stream (persistent, LDS-DMA double-buffered; the large axes of every config) against k_attention_rows (LSL_ATTN_STREAM=0)
    on the attention output of one spatial and one temporal sub-block: ragged last key tile (S = 200, 30, 9), both head widths, the
    head-major q / k / v planes (hidden 512) and token-major rows, more and fewer units than workgroups; round 5: the chunked form for axes
    beyond 256 positions (S = 1000 with 24-wide heads and the denominator column - peptide -, 300, 700, 512 = two full chunks) and the tiny
    spatial axes (L = 2, 4, 8) packed 32 / L sequences to a tile with a block-diagonal mask, against k_attention_tiny (fp32 probabilities),
    a last tile of 12 tokens included.  The two differ only by the bf16
    rounding of the probabilities (another softmax shift): 1.6 - 2.2e-3 relative L2 measured."""
    import os
    import subprocess
    import sys
    code = (
        "import torch, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from lam_slide_amd import _lib\n"
        "from oracle import latent_net\n"
        "from test_hip_parity import build_net, _hip_taps\n"
        "dev = torch.device('cuda:0')\n"
        "out = {}\n"
        "for name, kw, B, T, L in (('d512', dict(depth=1, in_dim=16, hidden_size=512, num_heads=16, mlp_ratio=2), 2, 30, 200),\n"
        "                          ('d512_full', dict(depth=1, in_dim=16, hidden_size=512, num_heads=16, mlp_ratio=2), 40, 9, 256),\n"
        "                          ('d256', dict(depth=1, in_dim=16, hidden_size=256, num_heads=16, mlp_ratio=2), 3, 20, 192),\n"
        "                          ('d128', dict(depth=1, in_dim=16, hidden_size=128, num_heads=8, mlp_ratio=2), 5, 32, 130),\n"
        "                          ('pep_xl', dict(depth=1, in_dim=16, hidden_size=384, num_heads=16, mlp_ratio=4), 2, 1000, 2),\n"
        "                          ('d512_xl', dict(depth=1, in_dim=16, hidden_size=512, num_heads=16, mlp_ratio=2), 1, 3, 300),\n"
        "                          ('d256_xl', dict(depth=1, in_dim=16, hidden_size=256, num_heads=16, mlp_ratio=2), 1, 2, 700),\n"
        "                          ('d128_xl512', dict(depth=1, in_dim=16, hidden_size=128, num_heads=8, mlp_ratio=2), 2, 512, 3),\n"
        "                          ('nba_packed', dict(depth=1, in_dim=16, hidden_size=256, num_heads=16, mlp_ratio=4), 3, 20, 8),\n"
        "                          ('l4_packed_ragged', dict(depth=1, in_dim=16, hidden_size=256, num_heads=8, mlp_ratio=2), 1, 11, 4)):\n"
        "    sh = latent_net.NetShape(**kw)\n"
        "    net = build_net(sh, latent_net.random_params(sh, seed=21), dev); net.ensure_packed(dev)\n"
        "    D = kw['hidden_size']; g = torch.Generator().manual_seed(3)\n"
        "    h = torch.randn(B, T, L, D, generator=g).to(dev)\n"
        "    mods = (torch.randn(B, 8 * D, generator=g) * 0.3).to(dev).contiguous()\n"
        "    for bi in (0, 1):\n"
        "        qkv, z = _hip_taps(net, _lib.load(), bi, h, mods, B, T, L, dev)\n"
        "        out[f'{name}.{bi}.attn'] = z[:, :net.dims.hhd].clone(); out[f'{name}.{bi}.qkv'] = qkv.clone()\n"
        "torch.save(out, sys.argv[1])\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("0", "1"):
        path = f"/tmp/lsl_attn_{mode}_{os.getpid()}.pt"
        env = dict({k: v for k, v in os.environ.items() if k != "LSL_ATTN_STREAM"}, LSL_ATTN_STREAM=mode)
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=900)
        res[mode] = torch.load(path)
        os.remove(path)
    for key in res["0"]:
        a, b = res["0"][key], res["1"][key]
        assert torch.isfinite(b).all(), key
        if key.endswith(".qkv"):  # q / k / v are the same bits in either layout (lsl_debug_taps hands the planes out as rows)
            assert torch.equal(a, b), key
        else:
            parity(f"attn_stream.{key}", rel_l2(b, a), 6e-3)


def _hip_taps(net, lib, bi, h_in, mods, B, T, L, dev):
    """qkv / z of sub-block bi as the kernels leave them (lsl_debug_taps), as float tensors [n, 3, H, hdp] and [n, HHD + M]."""
    from lam_slide_amd import _lib
    dm = net.dims
    n = B * T * L
    qkv = torch.empty(n, 3 * dm.hhd, dtype=torch.bfloat16, device=dev)
    z = torch.empty(n, dm.hhd + dm.mlp_dim_pad, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(int(lib.lsl_workspace_bytes(net._handle, B, T, L)) + (1 << 20), dtype=torch.uint8, device=dev)
    _lib.check(lib.lsl_debug_taps(net._handle, bi, h_in.data_ptr(), mods.data_ptr(), B, T, L, qkv.data_ptr(), z.data_ptr(), ws.data_ptr(),
                                  ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return qkv.float().cpu().reshape(n, 3, dm.heads, dm.head_dim_pad), z.float().cpu()


def _check_stage_taps(name, net, lib, sh, taps, h_states, mods, B, T, L, dev, bars):
    """Every stage between the GEMMs against the reference's (or the oracle's) own intermediates (per-kernel parity):
    q / k after QK-norm + RoPE, v, attention output, GELU(mlp).  A compensating error between two stages cannot hide here."""
    import math
    from oracle import latent_net
    D, H, hd = sh.hidden_size, sh.num_heads, sh.head_dim
    premul = 1.4426950408889634 / math.sqrt(hd) if sh.attention_mode == "scaled_dot_product" else 1.0  # (attention_linear: plain q)
    worst = {}
    for i in range(sh.depth):
        for bi, tag in ((2 * i, f"l{i}.sp."), (2 * i + 1, f"l{i}.tm.")):
            qkv, z = _hip_taps(net, lib, bi, h_states[bi].to(dev).contiguous(), mods, B, T, L, dev)
            temporal = bi & 1

            def tok(x):  # reference layout [G, H, S, hd] -> token-major [n, H, hd]
                if not temporal:
                    return x.permute(0, 2, 1, 3).reshape(B * T * L, H, hd)
                return x.reshape(B, L, H, T, hd).permute(0, 3, 1, 2, 4).reshape(B * T * L, H, hd)

            def tok_rows(x):  # [G, S, F] -> [n, F]
                if not temporal:
                    return x.reshape(B * T * L, -1)
                return x.reshape(B, L, T, -1).permute(0, 2, 1, 3).reshape(B * T * L, -1)

            zt = tok_rows(taps[tag + "z"])
            want = {
                "q": tok(taps[tag + "q_rope"]), "k": tok(taps[tag + "k_rope"]), "v": zt[:, 2 * D:3 * D].reshape(-1, H, hd),
                "attn": tok_rows(taps[tag + "attn"]).reshape(-1, H, hd), "gelu": latent_net.gelu_erf(zt[:, 3 * D:]),
            }
            got = {
                "q": qkv[:, 0, :, :hd] / premul, "k": qkv[:, 1, :, :hd], "v": qkv[:, 2, :, :hd],
                "attn": z[:, :net.dims.hhd].reshape(-1, H, net.dims.head_dim_pad)[:, :, :hd], "gelu": z[:, net.dims.hhd:net.dims.hhd + net.dims.mlp_dim],
            }
            for k in want:
                e = rel_l2(got[k], want[k])
                worst[k] = max(worst.get(k, 0.0), e)
            if net.dims.head_dim_pad > hd:  # padded head columns carry nothing into the attention products
                assert float(qkv[:, :2, :, hd:].abs().max()) == 0.0
    for k, e in worst.items():
        parity(f"{name}.{k}", e, bars[k])


def test_stage_taps_against_reference_intermediates(golden, dev):
    """F1: the reference module's own q_norm / rope / attention / linear1 taps (tools/make_fixtures.py), every sub-block fed the reference's
    input state (16-wide heads, hidden 64: the tile GEMM kernels)."""
    from lam_slide_amd import _lib
    from oracle import latent_net
    f = golden("f1_block.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    net.ensure_packed(dev)
    taps = f.group("taps")
    B, T, L, D = 2, 5, 6, sh.hidden_size
    o_taps = {}
    latent_net.forward(f.group("p"), sh, f["x"], f["t"], f["x_cond"], f["mask"], f["y"], taps=o_taps)
    mods = torch.cat([taps[f"l{i}.mod"] for i in range(sh.depth)] + [taps["final_mod"].reshape(B, 2 * D)], dim=1).to(dev).contiguous()
    h_states, h_prev = [], o_taps["h0"]
    for i in range(sh.depth):
        g1 = taps[f"l{i}.mod"][:, 2 * D:3 * D][:, None, None, :]
        h_states += [h_prev, h_prev + g1 * taps[f"l{i}.sp.out"].reshape(B, T, L, D)]
        h_prev = taps[f"l{i}.h"]
    _check_stage_taps("f1.taps", net, _lib.load(), sh, taps, h_states, mods, B, T, L, dev,
                      dict(q=1.5e-2, k=1.5e-2, v=1.5e-2, attn=1.5e-2, gelu=1.5e-2))


@pytest.mark.parametrize("kw,T,L", [
    (dict(depth=1, in_dim=16, hidden_size=128, num_heads=4, mlp_ratio=2), 6, 40),                       # 32-wide heads (pedestrian family)
    (dict(depth=1, in_dim=16, hidden_size=256, num_heads=16, mlp_ratio=4, normalize=True), 20, 8),      # 16-wide heads (NBA family)
    (dict(depth=1, in_dim=16, hidden_size=384, num_heads=16, mlp_ratio=4), 33, 2),                      # 24 -> 32 padded heads (peptide family)
    (dict(depth=1, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2), 3, 256),                     # the headline model's block
], ids=["d128", "d256", "d384", "d512"])
def test_stage_taps_of_the_token_stationary_linear1(kw, T, L, dev):
    """The same stage-by-stage comparison on the hidden sizes that run the token-stationary linear1 kernel (k_lin1.hip.h), against the
    pinned oracle's taps; B*T*L is not a multiple of 256 in three of the four shapes (ragged last token tile)."""
    from lam_slide_amd import _lib
    from oracle import latent_net
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=21)
    net = build_net(sh, p, dev)
    net.ensure_packed(dev)
    B, C, D = 2, kw["in_dim"], kw["hidden_size"]
    g = torch.Generator().manual_seed(3)
    x, xc = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    mask = (torch.rand(B, T, L, generator=g) > 0.5).long()
    t = torch.rand(B, generator=g)
    taps = {}
    latent_net.forward(p, sh, x, t, xc, mask, None, taps=taps)
    mods = torch.cat([taps[f"l{i}.mod"] for i in range(sh.depth)] + [taps["final_mod"].reshape(B, 2 * D)], dim=1).to(dev).contiguous()
    g1 = taps["l0.mod"][:, 2 * D:3 * D][:, None, None, :]
    h_states = [taps["h0"], taps["h0"] + g1 * taps["l0.sp.out"].reshape(B, T, L, D)]
    _check_stage_taps(f"taps.{D}", net, _lib.load(), sh, taps, h_states, mods, B, T, L, dev,
                      dict(q=1.5e-2, k=1.5e-2, v=1.5e-2, attn=1.5e-2, gelu=1.5e-2))
