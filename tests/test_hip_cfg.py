"""GPU parity at the BASELINE.json configurations themselves and of the evaluation steps next to the path:
  * cfg 2 (the headline): T=30, L=256, C=32, D=512, H=16, depth 4, 50 Euler updates, through SecondStageSampler + Stage1Decoder against
    the oracle chain; B=32 (the 960-tile persistent regime of the bench) bit-equal to B=1;
  * cfg 4 family: a 250-step Euler-Maruyama run with stored noise (error growth over a long stochastic solve);
  * f4: best-of-K ADE/FDE on decoded K-sample output and chained rollouts through the real encode -> sample -> decode closure;
  * noise: consecutive calls differ, reseed() replays, sharded == unsharded without explicit noise.
Bars are ~5x the values measured on MI355X (conftest.parity prints both)."""
import pytest
import torch

from conftest import parity, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _net(kw, seed, dev):
    from lam_slide_amd import LatentSIV3
    from oracle import latent_net
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=seed)
    net = LatentSIV3(reset_parameters=False, **kw)
    net.load_state_dict(p)
    return net.to(dev), sh, p


def test_cfg2_md17_bench_full(dev):
    """BASELINE configs[1] as benchmarked: 7680 tokens per trajectory, D=512 (K=512 / 1536 GEMMs, head_dim 32, S=256 spatial and S=30
    temporal attention), num_steps=51 = 50 state updates.  B=2 against the CPU oracle, latents and decoded coordinates."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder
    from lam_slide_amd.synthetic import seeded_decoder_state_dict
    from oracle import harness, transport as otr
    kw = dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2)
    net, sh, p = _net(kw, 0, dev)
    B, T, L = 2, 30, 256
    g = torch.Generator().manual_seed(1)
    lat, init = torch.randn(B, T, L, 32, generator=g), torch.randn(B, T, L, 32, generator=g)
    skw = {"sampling_method": "euler", "num_steps": 51}
    dsd = seeded_decoder_state_dict(seed=7)
    dec = Stage1Decoder(dsd, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 10), mask_cond_mean=True, sampling_kwargs=skw, decode=dec)
    got = drv.sample_latents(lat.to(dev), init=init.to(dev))
    assert drv.last_sampler.last_path == "fused" and net.last_path == "hip"
    ent = torch.arange(21)[None].expand(B * T, 21)
    pos = dec.decode(got.reshape(B * T, L, 32), ent.to(dev)).cpu()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    xc, m = harness.setup_conditioning(lat, (0, 10), True)
    want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, m, None, "ODE", skw)
    pos_want = harness.decode(dsd, harness.DecoderShape(), want.reshape(B * T, L, 32), ent)
    parity("cfg2.latents", rel_l2(got.cpu(), want), 3e-4)
    parity("cfg2.decoded_coords", rel_l2(pos, pos_want), 2e-4)


def test_cfg2_batch32_equals_batch1_bits(dev):
    """The bench runs 32 trajectories per pass (960 token tiles, persistent GEMM workgroups walking several tiles each); a trajectory's
    bits must not depend on that: B=32 against the same trajectories sampled alone (30 tiles, one round of the grid)."""
    from lam_slide_amd import CreateTransport, SecondStageSampler
    kw = dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2)
    net, _, _ = _net(kw, 0, dev)
    B, T, L = 32, 30, 256
    g = torch.Generator().manual_seed(5)
    lat, init = torch.randn(B, T, L, 32, generator=g).to(dev), torch.randn(B, T, L, 32, generator=g).to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 10), sampling_kwargs={"sampling_method": "euler", "num_steps": 6})
    full = drv.sample_latents(lat, init=init)
    assert torch.isfinite(full).all()
    for i in (0, 17, 31):
        assert torch.equal(full[i:i + 1], drv.sample_latents(lat[i:i + 1], init=init[i:i + 1])), i


def test_long_sde_250_steps_with_stored_noise(dev):
    """Peptide family (D=384, head_dim 24 padded to 32, C=96, depth 7, L=2) at T=64: 250-step Euler-Maruyama, linear diffusion, "Mean"
    last step, every noise slice stored; the drift gain (pi/2)/cos(pi t/2) and 250 accumulated bf16-operand evaluations are where an
    error would grow.  Final and mid-trajectory states against the oracle (one evaluation per step on both sides)."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness, transport as otr
    kw = dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4)
    net, sh, p = _net(kw, 11, dev)
    B, T, L, n = 1, 64, 2, 250
    g = torch.Generator().manual_seed(8)
    lat, init = torch.randn(B, T, L, 96, generator=g), torch.randn(B, T, L, 96, generator=g)
    noise = torch.randn(n - 1, B, T, L, 96, generator=g)
    xc, m = harness.setup_conditioning(lat, (0, 1), True)
    s = Sampler(CreateTransport("GVP", "data")(), fused=True, keep_trajectory=True)
    res = s.sample_sde(diffusion_form="linear", last_step="Mean", num_steps=n, noise=noise.to(dev))(init.to(dev), net.forward, x_cond=xc.to(dev),
                                                                                                     x_cond_mask=m.to(dev))
    assert s.last_path == "fused" and len(res) == n
    states = {}

    def model(xt, t, **kw_):
        from oracle import latent_net
        return latent_net.forward(p, sh, xt, t.to(xt.dtype), **kw_)

    xs = otr.sample_sde(otr.Transport("GVP", "data"), init, model, noise=list(noise), diffusion_form="linear", last_step="Mean", num_steps=n,
                        single_eval=True, x_cond=xc, x_cond_mask=m)
    assert len(xs) == n
    for i, tag in ((n // 2, "mid"), (n - 2, "penultimate"), (n - 1, "final")):
        states[tag] = rel_l2(res[i].cpu(), xs[i])
    parity("sde250.mid", states["mid"], 1.5e-4)
    parity("sde250.penultimate", states["penultimate"], 3e-4)
    parity("sde250.final", states["final"], 7e-4)


def _pedestrian_chain(dev, B=4, K=20):
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder
    from conftest import Fixture
    e, d = Fixture("f7_encode.npz"), Fixture("f6_decode.npz")
    enc = Stage1Encoder(e.group("p"), num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(d.group("p"), num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    kw = dict(depth=6, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2, vec_in_dim=256, normalize=True)
    net, sh, p = _net(kw, 17, dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 8), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": 11})
    return enc, dec, net, sh, p, drv, e.group("p"), d.group("p")


def test_best_of_k_errors_on_device_against_the_oracle_chain(dev):
    """f4(i): pedestrian shape (T=20, D=128, class vector, normalize), K=20 samples per scene folded into one fused call, decoded on the
    device, best-of-K ADE/FDE reduced on the device - against K sequential oracle samples + oracle decode + the reference formula."""
    from lam_slide_amd import best_of_k_errors
    from oracle import harness, transport as otr
    enc, dec, net, sh, p, drv, ep, dp = _pedestrian_chain(dev)
    B, T, L, A, K = 3, 20, 48, 10, 20
    g = torch.Generator().manual_seed(23)
    lat = torch.randn(B, T, L, 32, generator=g)
    y = torch.randn(B, 256, generator=g)
    inits = torch.randn(K, B, T, L, 32, generator=g)
    ent = torch.stack([torch.randperm(32, generator=g)[:A] for _ in range(B)])         # entity ids of a scene, same on all frames
    target = torch.randn(B, T - 8, A, 3, generator=g)
    amask = torch.rand(B, A, generator=g) > 0.2

    def decode_dev(z):  # [K*B, T, L, C] -> [K*B, T, A, 3]
        n = z.shape[0]
        e_ = ent.to(dev).repeat(K, 1)[:n].repeat_interleave(T, dim=0)
        return dec.decode(z.reshape(n * T, L, 32), e_).reshape(n, T, A, 3)

    ade, fde = best_of_k_errors(drv, lat.to(dev), target.to(dev), K, decode_dev, agent_mask=amask.to(dev), y=y.to(dev), inits=inits.to(dev))
    assert ade.is_cuda and drv.last_sampler.last_path == "fused"
    xc, m = harness.setup_conditioning(lat, (0, 8), True)
    per_k = []
    for k in range(K):  # the reference's loop: one sample() per k
        fin = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), inits[k], xc, m, y, "ODE", {"sampling_method": "euler", "num_steps": 11})
        pos = harness.decode(dp, harness.DecoderShape(), fin.reshape(B * T, L, 32), ent.repeat_interleave(T, dim=0)).reshape(B, T, A, 3)
        per_k.append(pos[:, 8:].permute(0, 2, 1, 3).reshape(B * A, T - 8, 3)[amask.reshape(-1)])
    want_a, want_f = harness.compute_errors(torch.stack(per_k, dim=1), target.permute(0, 2, 1, 3).reshape(B * A, T - 8, 3)[amask.reshape(-1)])
    parity("f4.best_of_k.ade", rel_l2(ade.cpu(), want_a), 2.5e-5)
    parity("f4.best_of_k.fde", rel_l2(fde.cpu(), want_f), 2.5e-5)


def test_rollouts_through_the_real_closure_on_device(dev):
    """f4(ii): three chained rollouts (modules/sampling.py:44-63); each rollout = encode the conditioning frame repeated over T ->
    setup_conditioning -> fused sampler -> decode, all on the device with no host copy between rollouts, against the same chain on the
    oracle with the same initial noises."""
    from lam_slide_amd import sample_rollout
    from oracle import harness, transport as otr
    enc, dec, net, sh, p, drv, ep, dp = _pedestrian_chain(dev)
    T, A, R = 20, 12, 3
    g = torch.Generator().manual_seed(29)
    feat = torch.randn(3, 128, generator=g)   # stands for the dataset-specific prepare_inputs: positions -> encoder input
    ent = torch.randperm(32, generator=g)[:A]
    y = torch.randn(1, 256, generator=g)
    inits = torch.randn(R, 1, T, 48, 32, generator=g)
    cond = torch.randn(A, 3, generator=g) * 2.0 + 1.5
    shift, scale = 1.5, 2.0
    calls = {"n": 0}

    def sample_positions_dev(pos):  # pos [A, 3] on the device -> [T, A, 3]
        assert pos.is_cuda
        x = (pos @ feat.to(dev))[None].expand(T, A, 128).contiguous()
        z = enc.encode(x, ent.to(dev)[None].expand(T, A).contiguous(), torch.ones(T, A, dtype=torch.bool, device=dev))
        fin = drv.sample_latents(z[None], y=y.to(dev), init=inits[calls["n"]].to(dev))
        calls["n"] += 1
        return dec.decode(fin[0], ent.to(dev)[None].expand(T, A).contiguous())

    out = sample_rollout(sample_positions_dev, cond.to(dev), num_rollouts=R, shift=shift, scale=scale)
    assert out.is_cuda and out.shape == (R * T, A, 3) and calls["n"] == R
    k = {"n": 0}

    def sample_positions_cpu(pos):
        x = (pos @ feat)[None].expand(T, A, 128)
        z = harness.encode(ep, harness.EncoderShape(num_latents=48), x, ent[None].expand(T, A), torch.ones(T, A, dtype=torch.bool))
        xc, m = harness.setup_conditioning(z[None], (0, 8), True)
        fin = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), inits[k["n"]], xc, m, y, "ODE", {"sampling_method": "euler", "num_steps": 11})
        k["n"] += 1
        return harness.decode(dp, harness.DecoderShape(), fin[0], ent[None].expand(T, A))

    want = sample_rollout(sample_positions_cpu, cond, num_rollouts=R, shift=shift, scale=scale)
    assert torch.equal(out[0].cpu(), cond)
    parity("f4.rollout.first", rel_l2(out[:T].cpu(), want[:T]), 1.5e-4)
    parity("f4.rollout.third", rel_l2(out[2 * T:].cpu(), want[2 * T:]), 2e-4)   # errors chain through the conditioning frame


def test_fresh_noise_per_call_and_shard_invariance(dev):
    """without explicit noise every sampling call must draw fresh noise (K calls -> K different samples), reseed() replays, and
    a rank holding rows [lo, hi) of a batch draws exactly the rows of the unsharded call (initial state AND per-step SDE noise)."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, device_randn
    kw = dict(depth=1, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2)
    net, _, _ = _net(kw, 4, dev)
    lat = torch.randn(4, 8, 16, 32, generator=torch.Generator().manual_seed(0)).to(dev)
    for method, skw in (("ODE", {"sampling_method": "euler", "num_steps": 4}), ("SDE", {"num_steps": 4})):
        drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 2), sampling_method=method, sampling_kwargs=skw, seed=9)
        a, b = drv.sample_latents(lat), drv.sample_latents(lat)
        assert not torch.equal(a, b), method
        drv.reseed()
        assert torch.equal(a, drv.sample_latents(lat)) and torch.equal(b, drv.sample_latents(lat))
        drv.reseed()
        parts = []
        for lo, hi in ((0, 1), (1, 4)):           # every "rank" makes the same number of calls
            drv.reseed()
            parts.append(drv.sample_latents(lat[lo:hi], first_index=lo))
        assert torch.equal(a, torch.cat(parts)), method
        k1 = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 2), sampling_method=method, sampling_kwargs=skw, seed=9)
        ks = k1.sample_latents_k(lat, 3)
        assert not torch.equal(ks[0], ks[1]) and not torch.equal(ks[1], ks[2])
    r = device_randn((1 << 18,), dev, 3)
    assert abs(float(r.mean())) < 0.01 and abs(float(r.std()) - 1) < 0.01
    assert torch.equal(device_randn((100,), dev, 3, elem_offset=50), r[50:150])


def test_forward_argument_checks_on_device(dev):
    """a scalar / [1] time broadcasts like the reference; a tensor on another device raises instead of faulting the GPU."""
    kw = dict(depth=1, in_dim=8, hidden_size=64, num_heads=4)
    net, _, _ = _net(kw, 2, dev)
    g = torch.Generator().manual_seed(0)
    x, xc = torch.randn(3, 4, 5, 8, generator=g).to(dev), torch.randn(3, 4, 5, 8, generator=g).to(dev)
    m = torch.zeros(3, 4, 5, dtype=torch.long, device=dev)
    full = net(x, torch.full((3,), 0.3, device=dev), xc, m)
    assert torch.equal(full, net(x, torch.tensor(0.3, device=dev), xc, m)) and torch.equal(full, net(x, torch.tensor([0.3], device=dev), xc, m))
    with pytest.raises(RuntimeError):
        net(x, torch.full((3,), 0.3), xc, m)
    with pytest.raises(RuntimeError):
        net(x, torch.full((3,), 0.3, device=dev), xc.cpu(), m)
    with pytest.raises(ValueError):
        net(x, torch.full((2,), 0.3, device=dev), xc, m)


def test_forward_refuses_axis_too_long_for_rows_kernel(dev):
    """LSL_ATTN_STREAM=0 keeps the axes off the stream kernel; k_attention_rows holds K | V of a whole (sequence, head) in LDS, so at 32-wide
    heads a temporal axis of T = 1300 (key tiles: 1312 rows, 168 000 B > 160 KiB) is refused by the pass plan (ValueError, nothing launched)
    and T = 1200 (155 712 B) still runs.  In a child process: the library reads the variable once."""
    import os
    import subprocess
    import sys
    code = (
        "import torch, pytest, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_hip_cfg import _net\n"
        "dev = torch.device('cuda:0')\n"
        "net, _, _ = _net(dict(depth=1, in_dim=8, hidden_size=128, num_heads=4), 2, dev)\n"
        "def run(T):\n"
        "    g = torch.Generator().manual_seed(0)\n"
        "    x, xc = torch.randn(1, T, 1, 8, generator=g).to(dev), torch.randn(1, T, 1, 8, generator=g).to(dev)\n"
        "    out = net(x, torch.full((1,), 0.3, device=dev), xc, torch.zeros(1, T, 1, dtype=torch.long, device=dev))\n"
        "    torch.cuda.synchronize()\n"
        "    return out\n"
        "assert torch.isfinite(run(1200)).all()\n"
        "with pytest.raises(ValueError, match='attention axis of 1300 positions'):\n"
        "    run(1300)\n"
        "assert torch.isfinite(run(1200)).all()\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    env = dict({k: v for k, v in os.environ.items() if k != "LSL_ATTN_STREAM"}, LSL_ATTN_STREAM="0")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=600)


RESIDENT_CASES = {
    # name: (T, L, C, vec_in_dim, normalize, depth, method)      all with hidden 128, 4 heads of 32, mlp_ratio 2 (the pedestrian family)
    "ped_like_T20_L2": (20, 2, 32, 256, True, 6, "ODE"),          # temporal attention on MFMA (S = 20), spatial per lane (S = 2)
    "T5_L6_two_tiles": (5, 6, 32, None, False, 2, "ODE"),         # 30 tokens: two 16-token tiles, both axes per lane
    "T12_L4_C16": (12, 4, 16, 24, False, 2, "SDE"),               # 48 tokens (three full tiles), narrow state, stored noise + trajectory
    "T3_L1_C8": (3, 1, 8, None, True, 1, "ODE"),                  # S = 1 along the spatial axis
    "T17_L2_sde_tweedie": (17, 2, 32, None, False, 3, "SDE2"),    # odd T: padded key tile of the MFMA attention masked
}


@pytest.mark.parametrize("name", sorted(RESIDENT_CASES))
def test_trajectory_resident_kernel_against_oracle(name, dev):
    """csrc/k_resident.hip.h (one workgroup per trajectory, every state update in one launch) against the oracle: ODE and SDE step tables,
    stored noise, kept trajectory, class vector, normalize, padded token tiles, both attention forms.  The path must actually be taken."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness, transport as otr
    T, L, C, V, norm, depth, method = RESIDENT_CASES[name]
    kw = dict(depth=depth, in_dim=C, hidden_size=128, num_heads=4, mlp_ratio=2, normalize=norm)
    if V:
        kw["vec_in_dim"] = V
    net, sh, p = _net(kw, 31, dev)
    B = 5
    g = torch.Generator().manual_seed(41)
    lat, init = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    y = torch.randn(B, V, generator=g) if V else None
    xc, m = harness.setup_conditioning(lat, (0, max(1, T // 3)), True)
    mk = {"x_cond": xc.to(dev), "x_cond_mask": m.to(dev)}
    if y is not None:
        mk["y"] = y.to(dev)
    s = Sampler(CreateTransport("GVP", "data")(), fused=True, keep_trajectory=method != "ODE")
    if method == "ODE":
        skw = {"sampling_method": "euler", "num_steps": 9}
        got = s.get_sample_fn("ODE", skw)(init.to(dev), net.forward, **mk)[-1]
        want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, m, y, "ODE", skw)
        assert s.last_kernels == "resident"
        parity(f"resident.{name}", rel_l2(got.cpu(), want), {"ped_like_T20_L2": 1e-3}.get(name, 4e-4))
    else:
        n = 7
        form, last = ("linear", "Mean") if method == "SDE" else ("sigma", "Tweedie")
        noise = torch.randn(n - 1, B, T, L, C, generator=g)
        res = s.sample_sde(diffusion_form=form, last_step=last, num_steps=n, noise=noise.to(dev))(init.to(dev), net.forward, **mk)
        assert s.last_kernels == "resident" and len(res) == n

        def model(xt, t, **kw_):
            from oracle import latent_net
            return latent_net.forward(p, sh, xt, t.to(xt.dtype), **kw_)

        mko = {"x_cond": xc, "x_cond_mask": m}
        if y is not None:
            mko["y"] = y
        xs = otr.sample_sde(otr.Transport("GVP", "data"), init, model, noise=list(noise), diffusion_form=form, last_step=last, num_steps=n,
                            single_eval=True, **mko)
        parity(f"resident.{name}.final", rel_l2(res[-1].cpu(), xs[-1]), 7e-4)
        parity(f"resident.{name}.mid", rel_l2(res[3].cpu(), xs[3]), 3e-4)
    # a trajectory's bits do not depend on the batch it is sampled in (the path choice does not depend on B either)
    s1 = Sampler(CreateTransport("GVP", "data")(), fused=True)
    mk1 = {k: v[3:4] for k, v in mk.items()}
    if method == "ODE":
        alone = s1.get_sample_fn("ODE", skw)(init[3:4].to(dev), net.forward, **mk1)[-1]
        assert torch.equal(alone, got[3:4])
    else:
        alone = s1.sample_sde(diffusion_form=form, last_step=last, num_steps=n, noise=noise[:, 3:4].to(dev))(init[3:4].to(dev), net.forward, **mk1)[-1]
        assert torch.equal(alone, res[-1][3:4])


def test_resident_kernel_many_updates_and_device_noise(dev):
    """More state updates than one launch of the resident kernel holds (48): the groups chain through the state in HBM; and the device
    noise stream (Philox) of the resident path is shard-invariant like the general path's."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness, transport as otr
    kw = dict(depth=2, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2)
    net, sh, p = _net(kw, 7, dev)
    B, T, L = 3, 10, 2
    g = torch.Generator().manual_seed(3)
    lat, init = torch.randn(B, T, L, 32, generator=g), torch.randn(B, T, L, 32, generator=g)
    xc, m = harness.setup_conditioning(lat, (0, 3), True)
    mk = {"x_cond": xc.to(dev), "x_cond_mask": m.to(dev)}
    skw = {"sampling_method": "euler", "num_steps": 61}   # 60 updates = 48 + 12
    s = Sampler(CreateTransport("GVP", "data")(), fused=True)
    got = s.get_sample_fn("ODE", skw)(init.to(dev), net.forward, **mk)[-1]
    assert s.last_kernels == "resident"
    want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, m, None, "ODE", skw)
    parity("resident.60_updates", rel_l2(got.cpu(), want), 6e-4)

    def run(lo, hi):
        sd = Sampler(CreateTransport("GVP", "data")(), fused=True, seed=5)
        sd.elem_offset = lo * T * L * 32
        return sd.get_sample_fn("SDE", {"num_steps": 5})(init[lo:hi].to(dev), net.forward, **{k: v[lo:hi] for k, v in mk.items()})[-1]

    full = run(0, 3)
    assert torch.equal(full, torch.cat([run(0, 1), run(1, 3)])) and torch.isfinite(full).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(10, 2, 32, False, 2), (8, 4, 32, False, 2), (5, 6, 32, False, 2), (3, 1, 8, True, 1), (17, 1, 32, False, 1),
                                   (20, 2, 32, True, 6), (12, 4, 16, False, 2)])
def test_resident_kernel_rerun_bits(shape, dev):
    """The same call, repeated: every run gives the same bits.  Regression test for two defects found in round 2 while the resident
    kernel was rebuilt around its weight stream: an inline-asm v_max_f32 that read an MFMA result with no wait states (wrong results,
    timing-dependent), and run-to-run differences of 1e-7..1e-5 in the two-tile instance when weight loads were issued directly behind
    the MFMAs of the tile they refill (profiles/r02_resident.txt; since round 3 the product keeps every weight load behind the GELU block and
    tests/test_isa_scan.py checks the distance in the code object).  8 state updates x 300 reruns on the two-tile shapes, x 30 on the others."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness
    T, L, C, norm, depth = shape
    kw = dict(depth=depth, in_dim=C, hidden_size=128, num_heads=4, mlp_ratio=2, normalize=norm)
    net, sh, p = _net(kw, 31, dev)
    B = 5
    g = torch.Generator().manual_seed(5)
    lat, init = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    xc, m = harness.setup_conditioning(lat, (0, min(3, T - 1)), True)
    mk = {"x_cond": xc.to(dev), "x_cond_mask": m.to(dev)}
    s = Sampler(CreateTransport("GVP", "data")(), fused=True)
    fn = s.get_sample_fn("ODE", {"sampling_method": "euler", "num_steps": 9})
    ref = fn(init.to(dev), net.forward, **mk)[-1]
    assert s.last_kernels == "resident" and torch.isfinite(ref).all()
    # T * L <= 32 runs the two-token-tile instance, the one that showed the defect: 300 reruns there, 30 elsewhere
    reruns = 300 if T * L <= 32 else 30
    x0 = init.to(dev)
    differ = sum(0 if torch.equal(fn(x0, net.forward, **mk)[-1], ref) else 1 for _ in range(reruns))
    assert differ == 0, f"{differ}/{reruns} reruns differ"


FULL_SHAPES = {
    # BASELINE.json configs[3] / [4] at their true token counts (the benchmark's shapes), few state updates
    "peptide_T1000_L2": (dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4), 1000, 2, None, "SDE", 5e-4),
    "nba_T20_L8": (dict(depth=6, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4, vec_in_dim=256, normalize=True), 20, 8, 256, "ODE", 8e-4),
}


@pytest.mark.parametrize("name", sorted(FULL_SHAPES))
def test_full_size_shapes_of_cfg4_and_cfg5(name, dev):
    """The peptide (T = 1000: the long-sequence attention kernel, 24-wide heads padded to 32, 96 input channels on the fp32-MFMA
    embedding) and NBA (16-wide heads, class vector) models at the token counts of the benchmark: one network evaluation and a short
    sampler run against the oracle, and a trajectory's bits independent of the batch it is sampled in."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness, latent_net, transport as otr
    kw, T, L, V, method, bar = FULL_SHAPES[name]
    net, sh, p = _net(kw, 11, dev)
    B, C = 2, kw["in_dim"]
    g = torch.Generator().manual_seed(9)
    lat, init = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    y = torch.randn(B, V, generator=g) if V else None
    xc, m = harness.setup_conditioning(lat, (0, 1) if T > 100 else (0, 5), True)
    mk = {"x_cond": xc.to(dev), "x_cond_mask": m.to(dev)}
    mko = {"x_cond": xc, "x_cond_mask": m}
    if y is not None:
        mk["y"], mko["y"] = y.to(dev), y
    t = torch.tensor([0.3, 0.7])
    got = net(init.to(dev), t.to(dev), **mk)
    want = latent_net.forward(p, sh, init, t, **mko)
    assert net.last_path == "hip"
    parity(f"full.{name}.forward", rel_l2(got.cpu(), want), bar)
    s = Sampler(CreateTransport("GVP", "data")(), fused=True)
    if method == "ODE":
        skw = {"sampling_method": "euler", "num_steps": 4}
        run = lambda lo, hi: s.get_sample_fn("ODE", skw)(init[lo:hi].to(dev), net.forward, **{k: v[lo:hi] for k, v in mk.items()})[-1]
        want_s = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init, xc, m, y, "ODE", skw)
    else:
        n = 4
        noise = torch.randn(n - 1, B, T, L, C, generator=g)
        run = lambda lo, hi: s.sample_sde(diffusion_form="linear", last_step="Mean", num_steps=n, noise=noise[:, lo:hi].to(dev))(
            init[lo:hi].to(dev), net.forward, **{k: v[lo:hi] for k, v in mk.items()})[-1]

        def model(xt, tt, **kw_):
            return latent_net.forward(p, sh, xt, tt.to(xt.dtype), **kw_)

        want_s = otr.sample_sde(otr.Transport("GVP", "data"), init, model, noise=list(noise), diffusion_form="linear", last_step="Mean", num_steps=n,
                                single_eval=True, **mko)[-1]
    full = run(0, B)
    assert s.last_path == "fused" and torch.isfinite(full).all()
    parity(f"full.{name}.sampler", rel_l2(full.cpu(), want_s), 1.4 * bar if T > 100 else bar)
    assert torch.equal(full, torch.cat([run(0, 1), run(1, 2)]))


def test_cfg5_nba_full_batch_1024(dev):
    """BASELINE configs[4] at a full single-GPU batch: NBA model (hidden 256, 16 heads of 16, mlp 1024, class vector), T = 20 x L = 8,
    B = 1024 trajectories x 50 Euler updates: the multi-hundred-tile regime of the K = 256 linear1 / K = 1280 linear2 kernels.  Three
    trajectories of the big call are bit-equal to the same trajectories sampled alone, two are compared with the oracle."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness, transport as otr
    kw = dict(depth=6, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4, vec_in_dim=256, normalize=True)
    net, sh, p = _net(kw, 13, dev)
    B, T, L, C, V = 1024, 20, 8, 32, 256
    g = torch.Generator().manual_seed(17)
    lat, init = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    y = torch.randn(B, V, generator=g)
    xc, m = harness.setup_conditioning(lat, (0, 5), True)
    skw = {"sampling_method": "euler", "num_steps": 51}
    s = Sampler(CreateTransport("GVP", "data")(), fused=True)
    fn = s.get_sample_fn("ODE", skw)

    def run(idx):
        return fn(init[idx].to(dev), net.forward, x_cond=xc[idx].to(dev), x_cond_mask=m[idx].to(dev), y=y[idx].to(dev))[-1]

    full = run(slice(0, B))
    assert s.last_path == "fused" and s.last_kernels == "general" and torch.isfinite(full).all()
    for i in (0, 511, 1023):
        assert torch.equal(full[i:i + 1], run(slice(i, i + 1))), f"trajectory {i} depends on the batch it is sampled in"
    pick = [3, 777]
    want = harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init[pick], xc[pick], m[pick], y[pick], "ODE", skw)
    parity("cfg5.nba_b1024.sampler", rel_l2(full[pick].cpu(), want), 1.5e-3)


def test_cfg4_peptide_1000_step_sde_device_noise(dev):
    """BASELINE configs[3] as stated: tetrapeptide model (hidden 384, 16 heads of 24, mlp 1536, 96 channels), T = 1000 x L = 2, the
    1000-step Euler-Maruyama sampler with the DEVICE Philox stream (no stored noise: the mode production runs use).  Checked: finite,
    a rerun with the same seed gives the same bits, two half-batches with their global element offsets give the bits of the whole
    batch (shard invariance of the network AND of the noise), and the injected noise has the moments of N(0, 2 g dt) at every step
    (recovered from the kept trajectory against a noise-free replay of single steps)."""
    from lam_slide_amd import CreateTransport, Sampler
    from oracle import harness
    kw = dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4)
    net, sh, p = _net(kw, 19, dev)
    B, T, L, C = 2, 1000, 2, 96
    g = torch.Generator().manual_seed(23)
    lat, init = torch.randn(B, T, L, C, generator=g), torch.randn(B, T, L, C, generator=g)
    xc, m = harness.setup_conditioning(lat, (0, 1), True)
    skw = dict(sampling_method="Euler", diffusion_form="linear", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=1000)

    def run(lo, hi, seed=5, keep=False):
        s = Sampler(CreateTransport("GVP", "data")(), fused=True, seed=seed, keep_trajectory=keep)
        s.elem_offset = lo * T * L * C
        out = s.sample_sde(**skw)(init[lo:hi].to(dev), net.forward, x_cond=xc[lo:hi].to(dev), x_cond_mask=m[lo:hi].to(dev))
        assert s.last_path == "fused"
        return out

    full = run(0, B)[-1]
    assert torch.isfinite(full).all()
    assert torch.equal(full, run(0, B)[-1]), "same seed, different bits"
    assert not torch.equal(full, run(0, B, seed=6)[-1]), "the seed does not reach the noise"
    assert torch.equal(full, torch.cat([run(0, 1)[-1], run(1, 2)[-1]])), "sharded halves differ from the whole batch"
    # per-step moments of the injected noise: x_{s+1} - (ax x_s + am net(x_s, t_s)) = aw w_s; replay single noise-free steps from the kept
    # states of a short prefix (every 100th step of the first 900) and compare the residual's mean / variance with N(0, aw^2)
    s = Sampler(CreateTransport("GVP", "data")(), fused=True, seed=5, keep_trajectory=True)
    steps, _ = s.sde_steps(diffusion_form="linear", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=1000)
    traj = s.sample_sde(**skw)(init.to(dev), net.forward, x_cond=xc.to(dev), x_cond_mask=m.to(dev))
    assert torch.equal(traj[-1], full)
    for k in range(0, 900, 100):
        te, ax, am, aw = steps[k + 1]
        x_s = traj[k]           # state after update k = input of update k + 1
        tv = torch.full((B,), te, device=dev)
        mean_next = ax * x_s + am * net(x_s, tv, x_cond=xc.to(dev), x_cond_mask=m.to(dev))
        w = ((traj[k + 1] - mean_next) / aw).flatten().double().cpu()
        assert abs(float(w.mean())) < 0.02 and abs(float(w.var()) - 1.0) < 0.03, (k, float(w.mean()), float(w.var()))
