"""CPU tests of the host side: weight packing, the affine step tables the fused sampler consumes, the generic
sampler loop, the C-ABI surface (load + symbols + argument validation, no compute), and the 2-rank sharding
over gloo."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, rel_l2
from oracle import harness, latent_net, transport as otr


def test_library_builds_and_exports_header_symbols():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    declared = set(re.findall(r"\b(lsl_[a-z_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTED), declared ^ set(_lib.EXPORTED)
    for s in declared:
        assert hasattr(lib, s), s
    assert re.search(r"#define LSL_VERSION (\d+)", header).group(1) == str(_lib.ABI_VERSION)
    # built with -fvisibility=hidden: the dynamic symbol table defines the entry points of the header and nothing else (no device stubs,
    # no C++ helpers)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.split()[-2:-1] and line.split()[-2] in "TDBRWV"}
    assert defined == declared, defined ^ declared


def test_every_limit_the_binding_mirrors_equals_its_macro():
    """The limits the dispatch rules read (_lib.py) are copies of ``#define`` s of the header and the kernel headers: each equals the
    integer value of its macro's expression (``(1 << 21)``, ``16777215LL``, ``(LSL_GEOM_MAX_A / 14)``), so a limit changed in a header
    alone cannot send a shape the kernel refuses down the device path."""
    import glob
    from lam_slide_amd import _lib, peptide_loss
    defines = {}
    for path in [os.path.join(ROOT, "include", "lsl_api.h")] + sorted(glob.glob(os.path.join(_lib.SRC_DIR, "*.hip.h"))):
        for name, expr in re.findall(r"^#define (LSL_\w+)[ \t]+([^\n]*?)[ \t]*(?://[^\n]*|/\*[^\n]*)?$", open(path).read(), re.M):
            defines[name] = expr

    def macro(name):
        expr = re.sub(r"LSL_\w+", lambda m: str(macro(m.group(0))), defines[name])
        expr = re.sub(r"(\d)L+\b", r"\1", expr).replace("/", "//")
        assert re.fullmatch(r"[\d\s()<>*/+-]+", expr), (name, expr)
        return eval(expr)  # (digits, brackets and integer operators only)

    mirrors = {"RK_SCRATCH_BYTES": "LSL_RK_SCRATCH_BYTES", "SI_SLAB": "LSL_SI_SLAB", "GEOM_MAX_A": "LSL_GEOM_MAX_A", "GEOM_MAX_D": "LSL_GEOM_MAX_D",
               "DISP_MAX_D": "LSL_DISP_MAX_D", "DISP_MAX_UNITS": "LSL_DISP_MAX_UNITS", "TORS_MAX_A": "LSL_TORS_MAX_A", "TORS_MAX_Q": "LSL_TORS_MAX_Q",
               "HIST_MAX_BINS": "LSL_HIST_MAX_BINS", "HIST2_MAX_BINS": "LSL_HIST2_MAX_BINS", "LAG_CHUNK": "LSL_LAG_CHUNK",
               "LAG_MAX_LAGS": "LSL_LAG_MAX_PART", "LAG_MAX_ROWS": "LSL_LAG_MAX_ROWS", "MOM_SEG": "LSL_MOM_SEG", "MOM_CHAIN": "LSL_MOM_SEG",
               "MOM_MAX_F": "LSL_MOM_MAX_F", "PROJ_MAX_D": "LSL_PROJ_MAX_D", "ASG_MAX_K": "LSL_ASG_MAX_K", "ASG_MAX_D": "LSL_ASG_MAX_D",
               "ASG_CELLS": "LSL_ASG_CELLS", "ASG_MAX_STATES": "LSL_ASG_MAX_STATES", "TR_MAX_STATES": "LSL_TR_MAX_STATES",
               "KM_SEG": "LSL_KM_SEG", "KM_MAX_S": "LSL_KM_MAX_S", "WMOM_MIN_F": "LSL_WMOM_MIN_F", "WMOM_MAX_F": "LSL_WMOM_MAX_F",
               "WPROJ_MAX_D": "LSL_WPROJ_MAX_D", "WMOM_SEG": "LSL_WMOM_SEG", "WMOM_CHAIN": "LSL_WMOM_CHAIN", "PAIR_MAX_P": "LSL_PAIR_MAX_P",
               "CA_MAX_R": "LSL_CA_MAX_R", "CLS_MAX_K": "LSL_CLS_MAX_K", "CLS_IGNORE": "LSL_CLS_IGNORE"}
    # every upper-case integer of the binding is in the table, except the ABI version (checked above) and the two step flags
    ints = {k for k, v in vars(_lib).items() if k.isupper() and type(v) is int}
    assert ints - {"ABI_VERSION", "STEP_NO_NETWORK", "STEP_SAVE"} == set(mirrors), ints ^ set(mirrors)
    for attr, name in mirrors.items():
        assert getattr(_lib, attr) == macro(name), (attr, name, getattr(_lib, attr), macro(name))
    assert (_lib.LAG_MAX_LAGS, _lib.DISP_MAX_UNITS, _lib.TORS_MAX_Q, _lib.LAG_MAX_ROWS) == (1 << 21, 16777215, 65536, 65535)
    assert peptide_loss.MAX_R == macro("LSL_PEPT_MAX_R") == 146
    assert (_lib.STEP_NO_NETWORK, _lib.STEP_SAVE) == (macro("LSL_STEP_NO_NETWORK"), macro("LSL_STEP_SAVE"))


def test_model_create_validation_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    ok = _lib.ModelDesc(32, 256, 16, 16, 16, 512, 4, 0, 0, 10000.0)
    assert lib.lsl_model_create(C.byref(ok), C.byref(h)) == 0
    assert lib.lsl_workspace_bytes(h, 4, 30, 192) > 0
    io = _lib.IO(None, None, None, None, None, None, 1, 1, 1)
    assert lib.lsl_forward(h, C.byref(io), None, 0, None) == -2  # weights not set: refuses before touching the GPU
    assert b"weights" in lib.lsl_last_error()
    lib.lsl_model_destroy(h)
    bad = _lib.ModelDesc(32, 250, 16, 15, 16, 512, 4, 0, 0, 10000.0)
    assert lib.lsl_model_create(C.byref(bad), C.byref(h)) == -20
    assert b"divisible" in lib.lsl_last_error()
    with pytest.raises(ValueError):
        _lib.check(-20)


def test_module_state_dict_contract_and_errors():
    from lam_slide_amd import LatentSIV3
    for kw in (dict(depth=2, in_dim=8, hidden_size=64, num_heads=4, vec_in_dim=16), dict(depth=3, in_dim=32, hidden_size=128, num_heads=4, share_weights=True),
               dict(depth=1, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4)):
        net = LatentSIV3(reset_parameters=False, **kw)
        sh = latent_net.NetShape(**kw)
        ref = latent_net.random_params(sh, seed=0)
        sd = net.state_dict()
        assert set(sd) == set(ref)
        assert all(sd[k].shape == ref[k].shape for k in ref)
        net.load_state_dict(ref)
        assert all(torch.equal(net.state_dict()[k], ref[k]) for k in ref)
        # a backbone saved while wrapped by torch.compile carries the `_orig_mod.` prefix (second_stage/md17.py:53-55)
        other = latent_net.random_params(sh, seed=1)
        net.load_state_dict({"_orig_mod." + k: v for k, v in other.items()})
        assert all(torch.equal(net.state_dict()[k], other[k]) for k in other)
    z = LatentSIV3(depth=1, in_dim=8, hidden_size=64, num_heads=4)  # reset_parameters=True: AdaLN-Zero init
    assert float(z.blocks[0].modulation.lin.weight.detach().abs().sum()) == 0 and float(z.linear.weight.detach().abs().sum()) == 0
    with pytest.raises(ValueError):
        LatentSIV3(depth=1, in_dim=8, hidden_size=66, num_heads=4)
    with pytest.raises(RuntimeError):  # no CPU fallback
        z(torch.zeros(1, 2, 3, 8), torch.zeros(1), torch.zeros(1, 2, 3, 8), torch.zeros(1, 2, 3, dtype=torch.long))


@pytest.mark.parametrize("hidden,heads,mlp", [(64, 4, 2), (192, 8, 1), (128, 4, 2), (384, 16, 4)])
def test_packing_preserves_the_linear_maps(hidden, heads, mlp):
    """Packed (padded, reordered, bf16) weights must compute the same block as the originals: run the
    oracle block with weights unpacked from the packed tensors."""
    from lam_slide_amd.packing import make_dims, pack_block
    sh = latent_net.NetShape(depth=1, in_dim=8, hidden_size=hidden, num_heads=heads, mlp_ratio=mlp)
    p = latent_net.random_params(sh, seed=1)
    dm = make_dims(1, 8, hidden, heads, mlp, None, False, 10000)
    pk = pack_block(p, "blocks.0.spatial_block", dm, "cpu")
    H, hd, hdp, D, M = heads, hidden // heads, dm.head_dim_pad, hidden, sh.mlp_dim
    assert pk["w1"].shape == (-(-dm.f1 // 256) * 256, D) and pk["w2"].shape == (-(-D // 256) * 256, dm.k2) and dm.k2 % 64 == 0 and dm.hhd % 32 == 0
    assert float(pk["w1"][dm.f1:].float().abs().sum()) == 0 and float(pk["w2"][D:].float().abs().sum()) == 0
    w1 = pk["w1"].float()
    rows = torch.cat([w1[s * dm.hhd:(s + 1) * dm.hhd].view(H, hdp, D)[:, :hd].reshape(H * hd, D) for s in range(3)] + [w1[3 * dm.hhd:3 * dm.hhd + M]])
    assert torch.equal(rows, p["blocks.0.spatial_block.linear1.weight"].to(torch.bfloat16).float())
    pad = w1[: dm.hhd].view(H, hdp, D)[:, hd:]
    assert float(pad.abs().sum()) == 0
    w2 = pk["w2"].float()[:D]
    cols = torch.cat([w2[:, : dm.hhd].view(D, H, hdp)[:, :, :hd].reshape(D, H * hd), w2[:, dm.hhd:dm.hhd + M]], dim=1)
    assert torch.equal(cols, p["blocks.0.spatial_block.linear2.weight"].to(torch.bfloat16).float())
    assert torch.equal(pk["qs"][:hd], p["blocks.0.spatial_block.norm.query_norm.scale"]) and float(pk["qs"][hd:].abs().sum()) == 0


def _toy_model(x, t, **kw):
    return torch.tanh(x) * 0.7 + 0.1 * t.view(-1, 1, 1, 1).to(x.dtype)


@pytest.mark.parametrize("path", otr.PATHS)
@pytest.mark.parametrize("pred", otr.PREDICTIONS)
def test_affine_step_tables_reproduce_the_oracle_ode(path, pred):
    """x <- ax x + am m with the float64-derived coefficients must equal the reference arithmetic."""
    from lam_slide_amd import CreateTransport, Sampler
    g = torch.Generator().manual_seed(0)
    init = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    want = otr.sample_ode(otr.Transport(path, pred), init, _toy_model, num_steps=9)[-1]
    s = Sampler(CreateTransport(path, pred)())
    steps, grid = s.ode_steps(9)
    x = init.clone()
    for te, ax, am, aw in steps:
        assert aw == 0.0
        x = ax * x + am * _toy_model(x, torch.ones(2) * te)
    assert rel_l2(x, want) < 1e-5  # the oracle (like the reference) evaluates sin/cos(t) in fp32
    got = s.get_sample_fn("ODE", {"sampling_method": "euler", "num_steps": 9})(init, _toy_model)
    assert s.last_path == "generic" and got.shape[0] == 9
    assert rel_l2(got[-1], want) < 1e-5


@pytest.mark.parametrize("form,last", [("linear", "Mean"), ("SBDM", None), ("sigma", "Euler"), ("decreasing", "Tweedie"), ("inccreasing-decreasing", "Mean")])
@pytest.mark.parametrize("path,pred", [("GVP", "data"), ("Linear", "velocity"), ("VP", "noise"), ("Linear", "score")])
def test_affine_step_tables_reproduce_the_oracle_sde(form, last, path, pred):
    from lam_slide_amd import CreateTransport, Sampler
    g = torch.Generator().manual_seed(1)
    init = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    n = 7
    noise = [torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64) for _ in range(n - 1)]
    want = otr.sample_sde(otr.Transport(path, pred), init, _toy_model, noise=noise, diffusion_form=form, last_step=last, num_steps=n)
    if not torch.isfinite(want[-1]).all():
        pytest.skip("degenerate in the reference too: Linear path + SBDM diffusion divides by t0 = 0")
    s = Sampler(CreateTransport(path, pred)())
    steps, _ = s.sde_steps(diffusion_form=form, diffusion_norm=1.0, last_step=last, last_step_size=0.04, num_steps=n)
    x = init.clone()
    for i, (te, ax, am, aw) in enumerate(steps):
        m = _toy_model(x, torch.ones(2) * te)
        x = ax * x + am * m + (aw * noise[i] if aw != 0.0 else 0.0)  # noise slice i belongs to step i
    assert rel_l2(x, want[-1]) < 1e-5
    got = s.sample_sde(diffusion_form=form, last_step=last, num_steps=n, noise=torch.stack(noise))(init, _toy_model)
    assert len(got) == n and rel_l2(got[-1], want[-1]) < 1e-5
    heun_w = otr.sample_sde(otr.Transport(path, pred), init, _toy_model, noise=noise, sampling_method="Heun", diffusion_form=form, last_step=last, num_steps=n)
    heun_g = s.sample_sde(sampling_method="Heun", diffusion_form=form, last_step=last, num_steps=n, noise=torch.stack(noise))(init, _toy_model)
    assert rel_l2(heun_g[-1], heun_w[-1]) < 1e-5


def test_intervals_and_defaults_match_golden(golden):
    from lam_slide_amd import CreateTransport
    f = golden("f3_transport.npz")
    for path in otr.PATHS:
        for pred in otr.PREDICTIONS:
            tr = CreateTransport(path, pred)()
            iv = []
            for sde in (False, True):
                for form in ("SBDM", "linear"):
                    for ls in (0.0, 0.04):
                        iv.append(list(map(float, tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=form, sde=sde, eval=True, last_step_size=ls))))
            assert torch.equal(torch.tensor(iv, dtype=torch.float64), f.group(f"{path}.{pred}")["intervals"])
            # scalar coefficient functions against the reference's tensors on the fixture's t grid
            x, mo, t = f["x"], f["model_out"], f["t"]
            v = torch.stack([tr.velocity_coeffs(float(ti))[0] * x[i] + tr.velocity_coeffs(float(ti))[1] * mo[i] for i, ti in enumerate(t)])
            s = torch.stack([tr.score_coeffs(float(ti))[0] * x[i] + tr.score_coeffs(float(ti))[1] * mo[i] for i, ti in enumerate(t)])
            assert rel_l2(v, f.group(f"{path}.{pred}")["velocity"]) < 1e-5
            assert rel_l2(s, f.group(f"{path}.{pred}")["score"]) < 1e-5


def test_setup_conditioning_bit_exact(golden):
    from lam_slide_amd import setup_conditioning
    f = golden("f5_cond.npz")
    for mean in (True, False):
        for ci in ((0, 3), (0, 1), (2, 5)):
            xc, mask = setup_conditioning(f["latents"], ci, mean)
            assert torch.equal(xc, f[f"m{int(mean)}.{ci[0]}_{ci[1]}.x_cond"]) and torch.equal(mask, f[f"m{int(mean)}.{ci[0]}_{ci[1]}.mask"])


def test_shard_bounds_cover_and_order():
    from lam_slide_amd import shard_bounds
    for total in (0, 1, 7, 8, 8192, 8193):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(total, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["LSL_ROOT"])
from lam_slide_amd import sample_sharded
from oracle import harness, latent_net, transport as otr
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"], rank=int(os.environ["RANK"]), world_size=2)
sh = latent_net.NetShape(depth=1, in_dim=8, hidden_size=64, num_heads=4)
p = latent_net.random_params(sh, seed=0)
g = torch.Generator().manual_seed(0)
lat = torch.randn(5, 4, 6, 8, generator=g)
init = torch.randn(5, 4, 6, 8, generator=g)
def local(l, lo):
    xc, m = harness.setup_conditioning(l, (0, 2), True)
    return harness.sample_latents(p, sh, otr.Transport("GVP", "data"), init[lo:lo + l.shape[0]], xc, m, None, "ODE", {"sampling_method": "euler", "num_steps": 4})
out = sample_sharded(local, lat)            # one gather onto rank 0: only rank 0 holds the result
full = local(lat, 0)
if int(os.environ["RANK"]) == 0:
    assert out.shape == full.shape and torch.allclose(out, full, atol=1e-6), float((out - full).abs().max())
else:
    assert out is None
every = sample_sharded(local, lat, dst=None)  # all_gather form: every rank
assert every.shape == full.shape and torch.allclose(every, full, atol=1e-6)
dist.destroy_process_group()
print("rank", os.environ["RANK"], "ok")
"""


def test_two_rank_sharding_over_gloo(tmp_path):
    """N>1 path on CPU: contiguous batch split, no data-path collective, one gather onto rank 0 (or an all_gather on request); the CPU oracle
    stands in for the per-rank compute (checker role only)."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), PORT=str(port), LSL_ROOT=ROOT, OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_min_ade_fde_matches_reference_formula(golden):
    """The product against the oracle and a brute-force loop, and against what the reference's own `_compute_errors`
    (pedestrian.py:178-185) returned for these inputs (tests/golden/f14_compute_errors.npz)."""
    from lam_slide_amd import min_ade_fde
    g = torch.Generator().manual_seed(3)
    traj, target = torch.randn(7, 5, 12, 2, generator=g), torch.randn(7, 12, 2, generator=g)
    a, f = min_ade_fde(traj, target)
    oa, of = harness.compute_errors(traj, target)
    assert torch.equal(a, oa) and torch.equal(f, of)
    brute = torch.stack([torch.stack([(traj[n, k] - target[n]).norm(dim=-1).mean() for k in range(5)]).min() for n in range(7)])
    assert torch.allclose(a, brute, atol=1e-6)
    ref = golden("f14_compute_errors.npz")
    ra, rf = min_ade_fde(ref["traj"], ref["target"])
    assert torch.equal(ra, ref["ade"]) and torch.equal(rf, ref["fde"])


def test_stage1_decoder_packing_on_cpu(golden):
    """Host logic of the decoder wrapper: shapes read off the reference-named state dict, max_norm clipping done once at load
    (same formula as the oracle / torch embedding_renorm_), loud failure without a GPU."""
    from lam_slide_amd import Stage1Decoder
    from lam_slide_amd.decoder import renorm_table
    d = golden("f6_decode.npz")
    p = d.group("p")
    dec = Stage1Decoder(p, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    assert (dec.in_dim, dec.dim_latent, dec.dim_query, dec.dim_emb, dec.n_entities, dec.out_dim) == (32, 32, 128, 128, 32, 3)
    assert (dec.num_block_attn, dec.num_block_cross, dec.qk_norm) == (1, 0, True)
    table = p["decoder.entity_embedding.embedding.weight"]
    clipped = renorm_table(table, 1.0)
    norms = table.norm(dim=-1, keepdim=True)
    # torch's embedding_renorm_ multiplies by max_norm / (norm + 1e-7); the oracle divides: equal to an ulp
    assert torch.allclose(clipped, torch.where(norms > 1.0, table / (norms + 1e-7), table), rtol=3e-7, atol=0) and float(clipped.norm(dim=-1).max()) <= 1.0 + 1e-6
    assert (norms > 1.0).any() and (norms <= 1.0).any()
    with pytest.raises(RuntimeError):
        dec.decode(d["z"], d["entities"])
    with pytest.raises(ValueError):
        Stage1Decoder(p, num_head_latent=2, dim_head_latent=16, num_head_cross=4, dim_head_cross=16)
    with pytest.raises(KeyError):
        Stage1Decoder({k: v for k, v in p.items() if k != "post_quant.1.bias"}, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)


def test_sample_rollout_chains_on_last_frame():
    """modules/sampling.py:44-63: rollout r is conditioned on the last frame of rollout r-1, frame 0 of the result is the
    conditioning frame, shift / scale are removed before and restored after."""
    from lam_slide_amd import sample_rollout
    seen = []

    def sample_positions(pos):
        seen.append(pos.clone())
        return torch.stack([pos + (t + 1) for t in range(3)])  # T = 3 frames drifting away from the conditioning frame

    cond = torch.arange(8, dtype=torch.float32).reshape(2, 2, 2) * 2.0 + 10.0
    out = sample_rollout(sample_positions, cond, num_rollouts=3, shift=10.0, scale=2.0)
    norm = (cond - 10.0) / 2.0
    assert out.shape == (9, 2, 2, 2) and len(seen) == 3
    assert torch.equal(seen[0], norm) and torch.equal(seen[1], norm + 3) and torch.equal(seen[2], norm + 6)
    assert torch.equal(out[0], cond)                                # frame 0 = the conditioning frame
    assert torch.equal(out[4], (norm + 3 + 2) * 2.0 + 10.0)        # rollout 1, frame 1


def test_stage1_encoder_packing_on_cpu(golden):
    """Host logic of the encoder wrapper: shapes read off the reference-named state dict, loud failure without a GPU, mismatching
    head arguments rejected."""
    from lam_slide_amd import Stage1Encoder
    d = golden("f7_encode.npz")
    p = d.group("p")
    enc = Stage1Encoder(p, num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    assert (enc.dim_input, enc.dim_emb, enc.n_entities, enc.dim_latent, enc.num_latents) == (128, 128, 32, 32, 48)
    assert (enc.num_block_cross, enc.num_block_attn, enc.qk_norm) == (1, 1, True)
    with pytest.raises(RuntimeError):
        enc.encode(d["x"], d["entities"], d["mask"])
    with pytest.raises(ValueError):
        Stage1Encoder(p, num_head_cross=4, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    with pytest.raises(KeyError):
        Stage1Encoder({k: v for k, v in p.items() if k != "encoder.latents"}, num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)


def test_decoder_query_splitter_rows_reordered(golden):
    """The 1x1-conv extender of DecoderQuerySplitter as a Linear whose output IS the (latent, split) token sequence: row n*D + d of the
    packed weight = conv channel d*N + n (decoder.py:384-388 'B (D N) L -> B (L N) D')."""
    from lam_slide_amd import Stage1Decoder
    d = golden("f8_decode_split.npz")
    p = d.group("p")
    dec = Stage1Decoder(p, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16, act="gelu_tanh")
    w, b = p["decoder.extender.1.weight"][..., 0], p["decoder.extender.1.bias"]
    D, N = dec.dim_latent, dec.num_split
    lat = torch.randn(3, 5, D, generator=torch.Generator().manual_seed(1))
    ref = torch.nn.functional.linear(lat, w, b).reshape(3, 5, D, N).permute(0, 1, 3, 2).reshape(3, 5 * N, D)
    mine = torch.nn.functional.linear(lat, dec._sd["decoder.extender.rows"], dec._sd["decoder.extender.rows_bias"]).reshape(3, 5 * N, D)
    assert N == 4 and torch.equal(ref, mine)


def test_bench_self_launches_its_ranks(tmp_path):
    """`python bench.py --gpus 2` without a launcher must start two ranks itself and print ONE JSON line with n_gpus 2.  The sampling call
    is stubbed (no GPU here) and the collective runs over gloo; the rank start-up, the barrier / max-over-ranks timing, the all_gather of
    the final latents and the single-line contract are the real code."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--backend", "gloo",
                          "--stub-compute", "--batch", "3", "--no-cpu"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["collective_backend"] == "gloo" and out["steps"] == 2
    assert out["config"]["global_batch"] == 6 and out["gather_ms"] is not None and out["value"] > 0 and out["scaling"] == "weak"
    assert "stub" in out["data"]
    assert [r["rank"] for r in out["per_rank"]] == [0, 1] and all(r["ms_per_step"] > 0 for r in out["per_rank"])  # a straggler would show here
    assert max(r["ms_per_step"] for r in out["per_rank"]) == pytest.approx(out["ms_per_step"], rel=1e-9)       # the step is the max over ranks
    # the product path refuses gloo / CPU
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backend", "gloo", "--no-cpu"], env=env, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain `bench.py` run prints one line with the headline keys and times exactly --steps steps; `--dump-outputs DIR` writes what the
    last step returned as DIR/latents.npy (float32), the same bytes in two runs with the same arguments.  Sampling call stubbed (no GPU)."""
    import json
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    dumped = []
    for run in ("a", "b"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--stub-compute",
                              "--batch", "3", "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, res.stdout
        out = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in out, k
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["value"] == pytest.approx(3 * 3 / (out["ms_per_step"] * 3 * 1e-3), rel=1e-9)  # trajectories / timed seconds
        assert sorted(os.listdir(tmp_path / run)) == ["latents.npy"]
        dumped.append(np.load(tmp_path / run / "latents.npy"))
    assert dumped[0].dtype == np.float32 and dumped[0].shape == (3, 4, 4, 32)
    assert dumped[0].tobytes() == dumped[1].tobytes()
    for bad in (["--steps", "0"], ["--breakdown"]):  # no timed step to report; --breakdown is a leg of --full
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub-compute"] + bad, env=env, capture_output=True, text=True, timeout=120)
        assert res.returncode == 2 and "error" in res.stderr, (bad, res.stderr)


def test_bench_dump_outputs_samples_whole_trajectories_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    t = torch.arange(50 * 10 * 4, dtype=torch.float64).reshape(50, 10, 4)  # 160 bytes per trajectory in float32: 6 fit
    bench.dump_outputs(str(tmp_path / "a"), {"latents": t})
    bench.dump_outputs(str(tmp_path / "b"), {"latents": t})
    a, b = np.load(tmp_path / "a" / "latents.npy"), np.load(tmp_path / "b" / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (6, 10, 4) and a.nbytes <= 1000 and a.tobytes() == b.tobytes()
    rows = (a[:, 0, 0] / 40).astype(int)
    assert (np.diff(rows) > 0).all() and all(np.array_equal(a[i], t[r].float().numpy()) for i, r in enumerate(rows))
    small = torch.ones(2, 3)
    bench.dump_outputs(str(tmp_path / "c"), {"x": small})
    assert np.array_equal(np.load(tmp_path / "c" / "x.npy"), small.numpy())


def test_bench_launcher_fails_fast_when_a_rank_dies_before_the_rendezvous():
    """One of four self-launched ranks exits (code 7) before init_process_group: the launcher must stop the other three - which are
    waiting in the rendezvous - and return that code within seconds, not after the collective library's timeout."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    t0 = time.monotonic()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0", "--backend", "gloo",
                          "--stub-compute", "--stub-fail-rank", "2", "--batch", "2", "--no-cpu", "--rendezvous-timeout", "600"],
                         env=env, capture_output=True, text=True, timeout=300)
    took = time.monotonic() - t0
    assert res.returncode == 7, (res.returncode, res.stderr)
    assert "rank 2 exited with code 7" in res.stderr and not [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert took < 120, took  # (process start-up + torch import dominate; the rendezvous timeout above is 600 s)
    # and a launch that never finishes is stopped by --launch-timeout
    res = subprocess.run([sys.executable, "-c", "import sys; sys.argv=['bench.py','--gpus','2','--launch-timeout','0.5']; import bench; a=bench.parse_args(); "
                          "import subprocess as sp; real=sp.Popen; bench.subprocess.Popen=lambda *x, **k: real([sys.executable,'-c','import time; time.sleep(60)']); "
                          "sys.exit(bench.launch_ranks(a))"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "no result after --launch-timeout" in res.stderr, res.stderr


@pytest.mark.parametrize("workload,batch,stride", [("nba", 1024, 1024 * 20 * 8 * 32), ("peptide", 8, 8 * 1000 * 2 * 96)])
def test_bench_eight_ranks_weak_scaling_lines(workload, batch, stride):
    """The two documented 8-GPU weak-scaling lines (BASELINE configs[4] / [3]) through the real launcher with 8 stub ranks over gloo: eight
    processes start, rank 0 prints ONE line with the whole-job batch, eight collective ranks and the per-rank stride of the noise stream.
    No multi-GPU hardware run was available to the builder: this is what can be checked without one."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--backend", "gloo",
                          "--stub-compute", "--workload", workload, "--batch", str(batch), "--no-cpu"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["rccl_ranks"] == 8 and out["scaling"] == "weak" and out["config"]["workload"] == workload
    assert out["config"]["batch_per_gpu"] == batch and out["config"]["global_batch"] == 8 * batch
    assert out["config"]["noise_elem_stride_per_rank"] == stride
    assert out["gather_ms"] is not None and out["value"] > 0


@pytest.mark.parametrize("path,pred,form,last", [("GVP", "data", "linear", "Mean"), ("GVP", "data", "SBDM", "Euler"), ("GVP", "noise", "sigma", "Tweedie"),
                                                 ("GVP", "score", "decreasing", None), ("VP", "data", "constant", "Mean")])
def test_heun_records_reproduce_the_reference_heun_step(path, pred, form, last):
    """The extended step records handed to lsl_sample_ex for the stochastic Heun sampler (three records per step: noise in + keep,
    predictor, corrector with the kept state) interpreted on the CPU give the states of the reference's own Heun loop
    (integrators.py:39-51, here the generic per-step loop of Sampler) for a model that is a known function of (x, t)."""
    from lam_slide_amd import CreateTransport, Sampler, _lib
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    n = 7
    noise = torch.randn(n - 1, 2, 3, 4, 5, generator=g, dtype=torch.float64)

    def model(x, t, **kw):
        return torch.tanh(0.7 * x) * (1.0 + t.reshape(-1, 1, 1, 1).to(x.dtype)) - 0.2 * x

    s = Sampler(CreateTransport(path, pred)(), fused=False)
    kw = dict(sampling_method="Heun", diffusion_form=form, diffusion_norm=1.3, last_step=last, last_step_size=0.04, num_steps=n)
    want = s.sample_sde(**kw, noise=noise)(x0, model)
    rec, _ = s.heun_records(diffusion_form=form, diffusion_norm=1.3, last_step=last, last_step_size=0.04, num_steps=n)
    x, saved, states = x0.clone(), None, {}
    for (t, ax, am, aw, as_, flags, ni, ti) in rec:
        tv = torch.full((x.shape[0],), t, dtype=torch.float64)
        new = ax * x
        if not flags & _lib.STEP_NO_NETWORK:
            new = new + am * model(x, tv)
        if aw != 0.0:
            new = new + aw * noise[ni]
        if as_ != 0.0:
            new = new + as_ * saved
        x = new
        if flags & _lib.STEP_SAVE:
            saved = x.clone()
        if ti >= 0:
            states[ti] = x.clone()
    assert sorted(states) == list(range(n if last is not None else n - 1))
    for i, st in states.items():
        assert torch.isfinite(want[i]).all()
        assert torch.allclose(st, want[i].double(), rtol=2e-5, atol=2e-6), (i, float((st - want[i]).abs().max()))


# ---- adaptive dopri5 (the reference's default ODE method; torchdiffeq absent: parity unpinned, checked against scipy and exact solutions) ----
def test_dopri5_solver_against_exact_solution_and_scipy():
    import numpy as np
    from scipy.integrate import solve_ivp

    from lam_slide_amd.transport import dopri5_solve
    A = torch.tensor([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.0, -0.3, -0.1]], dtype=torch.float64)

    def f(t, y):  # stiff-free linear system with a time-dependent forcing, batch of 4 states
        return y @ A.T + torch.sin(torch.tensor(3.0 * t, dtype=torch.float64)) * torch.tensor([1.0, 0.0, -1.0], dtype=torch.float64)

    y0 = torch.tensor([[1.0, 0.0, 0.5], [0.2, -1.0, 0.0], [0.0, 0.0, 0.0], [3.0, 1.0, -2.0]], dtype=torch.float64)
    grid = np.linspace(0.0, 2.0, 9)
    for rtol, atol in ((1e-3, 1e-6), (1e-6, 1e-9)):
        ys, st = dopri5_solve(f, y0, list(grid), rtol, atol)
        ref = solve_ivp(lambda t, y: f(t, torch.from_numpy(y).reshape(4, 3)).reshape(-1).numpy(), (0.0, 2.0), y0.reshape(-1).numpy(),
                        method="DOP853", rtol=1e-12, atol=1e-14, t_eval=grid)
        sp = solve_ivp(lambda t, y: f(t, torch.from_numpy(y).reshape(4, 3)).reshape(-1).numpy(), (0.0, 2.0), y0.reshape(-1).numpy(),
                       method="RK45", rtol=rtol, atol=atol, t_eval=grid)
        got = torch.stack(ys).reshape(len(grid), -1).numpy()
        err = np.abs(got - ref.y.T).max()
        err_sp = np.abs(sp.y.T - ref.y.T).max()
        assert err < 30 * rtol, (rtol, err)                  # global error of an rtol-controlled solve
        assert err < 5 * err_sp + 10 * atol, (err, err_sp)   # same class of accuracy as scipy's Dormand-Prince at the same tolerances
        assert st["accepted"] >= 3 and st["nfe"] == 2 + 6 * (st["accepted"] + st["rejected"])
        assert abs(st["accepted"] + st["rejected"] - sp.nfev / 6) <= 0.35 * sp.nfev / 6 + 3  # same controller family: similar step counts
    # outputs are interpolated inside steps, not stepped to: a grid much finer than the steps costs no evaluations
    ys_f, st_f = dopri5_solve(f, y0, list(np.linspace(0.0, 2.0, 201)), 1e-3, 1e-6)
    ys_c, st_c = dopri5_solve(f, y0, [0.0, 2.0], 1e-3, 1e-6)
    assert st_f["nfe"] == st_c["nfe"] and torch.allclose(ys_f[-1], ys_c[-1], rtol=0, atol=1e-12)
    # degenerate grids: a single point, and output times that do not exceed the current time before any step was accepted
    ys_1, _ = dopri5_solve(f, y0, [0.0], 1e-3, 1e-6)
    assert len(ys_1) == 1 and torch.equal(ys_1[0], y0)
    ys_r, _ = dopri5_solve(f, y0, [0.0, 0.0, 0.5, 0.5], 1e-6, 1e-9)
    assert torch.equal(ys_r[0], y0) and torch.equal(ys_r[1], y0) and torch.allclose(ys_r[2], ys_r[3], rtol=0, atol=0)


def test_fixed_grid_runge_kutta_methods_have_their_orders():
    """torchdiffeq's other fixed-grid methods (midpoint, heun3, rk4 = 3/8 rule; transport.fixed_grid_rk_solve, parity with torchdiffeq unpinned:
    absent): on y' = -2 t y + cos t the error at t = 1.5 falls by 2^order when the step is halved, and every method returns one state per
    grid point starting with the initial one."""
    import numpy as np
    from scipy.integrate import solve_ivp
    from lam_slide_amd.transport import FIXED_GRID_RK_METHODS, fixed_grid_rk_solve
    y0 = torch.tensor([0.7, -1.3], dtype=torch.float64)
    import math
    f = lambda t, y: -2.0 * t * y + math.cos(t)
    exact = solve_ivp(lambda t, y: -2.0 * t * y + np.cos(t), (0.0, 1.5), y0.numpy(), method="DOP853", rtol=1e-13, atol=1e-14).y[:, -1]
    for method, order in zip(FIXED_GRID_RK_METHODS, (2, 3, 4)):
        errs = []
        for n in (16, 32, 64):
            ys = fixed_grid_rk_solve(f, y0, list(np.linspace(0.0, 1.5, n + 1)), method)
            assert len(ys) == n + 1 and torch.equal(ys[0], y0)
            errs.append(float(np.abs(ys[-1].numpy() - exact).max()))
        for a, b in zip(errs[:-1], errs[1:]):
            assert 0.8 * 2 ** order < a / b < 1.25 * 2 ** order, (method, errs)
    with pytest.raises(NotImplementedError):
        fixed_grid_rk_solve(f, y0, [0.0, 1.0], "bosh3")


@pytest.mark.parametrize("path,pred,reverse", [("GVP", "data", False), ("Linear", "velocity", False), ("VP", "noise", False)])
def test_sample_ode_dopri5_default_method_runs_and_converges(path, pred, reverse):
    """get_sample_fn("ODE", {}) - the reference's defaults (dopri5, 50 outputs, atol 1e-6, rtol 1e-3) - on a callable model: same states as
    a float64 solve of the same ODE at rtol 1e-9 within the solver tolerance (the stiff GVP / VP ends near t = 1 included, where a 4000-step
    Euler solve is off by 30 %), 50 outputs, state 0 = the initial noise."""
    from lam_slide_amd import CreateTransport, Sampler
    torch.manual_seed(0)
    W = torch.randn(6, 6) * 0.3

    def model(x, t, **kw):
        return torch.tanh(x @ W.to(x.dtype)) * (1.0 + t.to(x.dtype).view(-1, 1, 1)) - 0.2 * x

    init = torch.randn(3, 5, 6)
    s = Sampler(CreateTransport(path, pred)())
    kw = {"reverse": True} if reverse else {}
    out = s.get_sample_fn("ODE", dict(kw))(init, model)
    assert out.shape == (50, 3, 5, 6) and torch.equal(out[0], init) and s.last_path == "dopri5"
    stats = dict(s.last_ode_stats)
    tight = s.get_sample_fn("ODE", dict(kw, rtol=1e-9, atol=1e-12))(init.double(), model)
    for i in (10, 25, 49):
        scale = float(tight[i].abs().max())
        assert float((out[i] - tight[i]).abs().max()) < 1e-2 * scale, (i, scale)
    assert stats["accepted"] >= 3 and s.last_ode_stats["nfe"] > stats["nfe"]


def test_sample_ode_reverse_asserts_like_the_reference():
    """reverse=True turns the interval into (1 - t0, 1 - t1) and the reference's ode class then asserts t0 < t1 (integrators.py:67-70):
    the same AssertionError for both native methods."""
    from lam_slide_amd import CreateTransport, Sampler
    s = Sampler(CreateTransport("Linear", "velocity")())
    for method in ("euler", "dopri5"):
        with pytest.raises(AssertionError):
            s.sample_ode(sampling_method=method, reverse=True)


def test_committed_traffic_file_reproduces_from_the_committed_pmc_summary(tmp_path):
    """bench.py's `roofline_step` / `traffic` figures come from profiles/rNN_traffic*.json; every such file of the newest round must be what
    tools/traffic_from_pmc.py derives from the committed rocprofv3 summary it names (no hand-edited numbers), and every BASELINE
    configuration family that runs the general kernels has one."""
    import glob
    import json
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic*.json")))
    newest_round = max(os.path.basename(f)[:3] for f in files)
    newest = [f for f in files if os.path.basename(f).startswith(newest_round) and "step" in json.load(open(f))]
    assert newest, "no scripted traffic file committed"
    workloads = set()
    for f in newest:
        committed = json.load(open(f))
        workloads.add(committed["workload"])
        summary = os.path.join(ROOT, committed["source"])
        assert os.path.exists(summary), (f, committed["source"])
        out = tmp_path / "t.json"
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "traffic_from_pmc.py"), summary, "--commit", committed.get("commit", ""), "-o", str(out)],
                       check=True, capture_output=True, cwd=ROOT)
        again = json.load(open(out))
        assert again == committed, f
        # the decomposition's floors as DESIGN.md section 5 states them: HBM floor above the MFMA floor
        assert committed["step"]["hbm_floor_ms_at_8_tb_s"] > committed["step"]["mfma_floor_ms_at_2_5_pflop_s"] > 0, f
        # (a profile of an ln_fuse handle may hold no LayerNorm kernel at all: the statistics come from the embedding and from linear2)
        for cls in ("linear1", "linear2", "attention") + (() if committed.get("ln_fuse") else ("ln_modulate",)):
            assert committed[cls]["bytes"] > 0 and committed[cls]["avg_us"] > 0, (f, cls)
    assert {"md17_bench", "md17_ref", "nba", "peptide"} <= workloads


def test_runtime_switches_are_exactly_the_documented_ones():
    """Every environment variable the product reads (library sources outside -DLSL_EXPERIMENTS tuning: env_int / getenv; the Python package:
    os.environ) is a row of INTEGRATION.md section 6, and the table lists nothing that is not read - the list of switches cannot grow
    unnoticed.  tools/gpu.sh, the one script of the GPU box, parses."""
    import glob
    import re
    src = ""
    for f in glob.glob(os.path.join(ROOT, "lam_slide_amd", "csrc", "*")):
        src += open(f).read()
    read = set(re.findall(r'env_int\("(LSL_[A-Z0-9_]+)"', src)) | set(re.findall(r'getenv\("(LSL_[A-Z0-9_]+)"', src))
    for f in glob.glob(os.path.join(ROOT, "lam_slide_amd", "*.py")):
        read |= set(re.findall(r'os\.environ(?:\.get)?\(\s*"(LSL_[A-Z0-9_]+)"', open(f).read()))
    read -= {"LSL_FORCE_BUILD", "LSL_VERBOSE"}  # (build-time only, __graft_entry__.py)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("## 6. Runtime switches"):]
    listed = set(re.findall(r"^\| `(LSL_[A-Z0-9_]+)", table, flags=re.M))
    assert read == listed, (sorted(read - listed), sorted(listed - read))
    assert subprocess.run(["bash", "-n", os.path.join(ROOT, "tools", "gpu.sh")]).returncode == 0
