"""The reference side of the stage-1 case table (stage1_cases.py), on the CPU: at every case the fp32 oracle stays within 1e-6 (relative
L2) of the fp64 oracle and both are finite.  That pins the reference's own rounding where test_hip_stage1.py compares the HIP kernels
with it: the bar there (2e-6, or 5x this distance where that is larger) rests on the reference alone.

The distance follows the BLAS the fp32 oracle runs on (its summation order).  Seen so far: 0.3e-7 .. 6.5e-7 everywhere except
md17-1x496x5, where it was 4.4e-7 with one BLAS and 8.8e-7, the worst figure of the table, with another.  A failure of the 1e-6
assertion at that case on a new host is therefore first a statement about that host's fp32 GEMM, not about the case table.

Also here, because it needs no device: the scratch size the library reports for every case (``lsl_decode_workspace_bytes`` /
``lsl_encode_workspace_bytes``) against the recorded table of stage1_cases.py."""
import ctypes as C

import pytest
import torch

import stage1_cases as sc


def test_case_table_stays_within_the_key_limits():
    tile = lambda dh: 16 if dh <= 16 else 32 if dh <= 32 else 64  # noqa: E731
    for name, F, L, A in sc.DECODER_CASES:
        m = sc.DECODER_MODELS[name]
        assert not m.n_self or L <= sc.KEY_LIMIT[tile(m.latent[1])]
        assert not m.n_cross or A <= sc.KEY_LIMIT[tile(m.cross[1])]
        assert L * max(m.num_split, 1) <= sc.KEY_LIMIT[tile(m.cross[1])]
    for name, F, A in sc.ENCODER_CASES:
        m = sc.ENCODER_MODELS[name]
        assert not m.n_cross or A <= sc.KEY_LIMIT[tile(m.cross[1])]
        assert not m.n_self or m.num_latents <= sc.KEY_LIMIT[tile(m.latent[1])]
    # every head tile at its last accepted key count, padded and unpadded, and at two passes of the 256-thread loops where the limit allows
    assert ("md17", 1, 496, 5) in sc.DECODER_CASES and ("w32", 1, 252, 130) in sc.DECODER_CASES and ("w64", 1, 127, 127) in sc.DECODER_CASES
    assert ("md17", 2, 300) in sc.ENCODER_CASES and ("w32", 2, 252) in sc.ENCODER_CASES and ("w64", 2, 127) in sc.ENCODER_CASES


def test_variants_change_the_state_dict_as_described():
    base, split, noqk = sc.decoder_model("w32").sd, sc.decoder_model("w32_split5").sd, sc.decoder_model("w32_noqk").sd
    assert tuple(split["decoder.extender.1.weight"].shape) == (96 * 5, 96, 1) and tuple(split["decoder.extender.1.bias"].shape) == (96 * 5,)
    assert set(split) - set(base) == {"decoder.extender.1.weight", "decoder.extender.1.bias"}
    dropped = set(base) - set(noqk)
    assert len(dropped) == 2 * 3 and all(k.endswith(("query_norm.scale", "key_norm.scale")) for k in dropped)  # self, cross, output block
    assert all(torch.equal(base[k], noqk[k]) for k in noqk)
    enc, enc_noqk = sc.encoder_model("w32").sd, sc.encoder_model("w32_noqk").sd
    assert len(set(enc) - set(enc_noqk)) == 2 * 3 and not any("_norm.scale" in k for k in enc_noqk)


@pytest.mark.parametrize("case", sc.DECODER_CASES, ids=sc.case_id)
def test_decoder_oracle_fp32_within_1e6_of_fp64(case):
    c = sc.decoder_case(*case)
    name, F, _, A = case
    assert c.want.dtype == torch.float64 and tuple(c.want.shape) == (F, A, sc.DECODER_MODELS[name].out_dim)
    assert torch.isfinite(c.want).all() and torch.isfinite(sc.decode32(name, c.z, c.entities)).all()
    print(f"ORACLE s1.dec.{sc.case_id(case)} fp32 vs fp64 {c.ref_err:.3e}")
    assert c.ref_err < 1e-6, c.ref_err


@pytest.mark.parametrize("case", sc.ENCODER_CASES, ids=sc.case_id)
def test_encoder_oracle_fp32_within_1e6_of_fp64(case):
    c = sc.encoder_case(*case)
    name, F, _ = case
    assert c.want.dtype == torch.float64 and tuple(c.want.shape) == (F,) + tuple(sc.encoder_model(name).sd["encoder.latents"].shape)
    for mask, want in ((c.mask, c.want), (None, c.want_nomask)):
        assert torch.isfinite(want).all() and torch.isfinite(sc.encode32(name, c.x, c.entities, mask)).all()
    print(f"ORACLE s1.enc.{sc.case_id(case)} fp32 vs fp64 {c.ref_err:.3e} (mask) {c.ref_err_nomask:.3e} (no mask)")
    assert c.ref_err < 1e-6 and c.ref_err_nomask < 1e-6, (c.ref_err, c.ref_err_nomask)
    assert c.mask[:, 0].all()
    if c.mask.shape[1] > 1:  # the mask is ragged and matters
        assert not c.mask.all() and not torch.equal(c.want, c.want_nomask)


def test_oracle_gives_nan_for_a_fully_masked_frame_only():
    """softmax over a row of -inf is NaN in the oracle; the frames beside it are untouched.  lsl_encode shows the same pattern
    (test_hip_stage1.py).  F.scaled_dot_product_attention is not asserted here: what it returns for a fully masked row (NaN or zeros)
    has differed between PyTorch versions, so an empty frame has no portable meaning in the reference."""
    x, entities, mask = sc.encoder_inputs("w32", 3, 65)
    dead = mask.clone()
    dead[0] = False
    for enc in (sc.encode32, sc.encode64):
        z, z_dead = enc("w32", x, entities, mask), enc("w32", x, entities, dead)
        assert torch.isnan(z_dead[0]).all() and torch.isfinite(z_dead[1:]).all()
        assert torch.equal(z_dead[1:], z[1:])


def test_workspace_bytes_of_every_case_are_the_recorded_ones():
    """The create calls only copy the description and the pointers and the size calls only add: handles made through ctypes from the
    description of each model class, with placeholder weight pointers, need no device."""
    from lam_slide_amd import _lib
    from lam_slide_amd.decoder import _ACT
    lib = _lib.load()
    blocks = lambda n: (_lib.DecBlock * max(n, 1))()  # noqa: E731

    def decoder(name):
        r, h = sc.DECODER_MODELS[name], C.c_void_p()
        desc = _lib.DecoderDesc(r.in_dim, r.dim_latent, r.dim_query, r.dim_emb, sc.N_ENTITIES, *r.latent, *r.cross, r.n_self, r.n_cross, _ACT[r.act],
                                r.out_dim, r.num_split)
        w = _lib.DecoderWeights(self_blocks=blocks(r.n_self), cross_blocks=blocks(r.n_cross), ext_w=64, ext_b=64)
        _lib.check(lib.lsl_decoder_create(C.byref(desc), C.byref(w), C.byref(h)))
        return h

    def encoder(name):
        r, h = sc.ENCODER_MODELS[name], C.c_void_p()
        desc = _lib.EncoderDesc(r.dim_input, r.dim_emb, sc.N_ENTITIES, r.dim_latent, r.num_latents, *r.cross, *r.latent, r.n_cross, r.n_self, _ACT[r.act])
        w = _lib.EncoderWeights(self_blocks=blocks(r.n_self), cross_blocks=blocks(r.n_cross))
        _lib.check(lib.lsl_encoder_create(C.byref(desc), C.byref(w), C.byref(h)))
        return h

    assert len(sc.DECODE_WORKSPACE_BYTES) == len(sc.DECODER_CASES) == 12 and len(sc.ENCODE_WORKSPACE_BYTES) == len(sc.ENCODER_CASES) == 6
    for (name, F, L, A), want in zip(sc.DECODER_CASES, sc.DECODE_WORKSPACE_BYTES):
        h = decoder(name)
        assert lib.lsl_decode_workspace_bytes(h, F, L, A) == want, (name, F, L, A)
        assert lib.lsl_decode_workspace_bytes(h, 0, L, A) == 0 and lib.lsl_decode_workspace_bytes(None, F, L, A) == 0
        lib.lsl_decoder_destroy(h)
    for (name, F, A), want in zip(sc.ENCODER_CASES, sc.ENCODE_WORKSPACE_BYTES):
        h = encoder(name)
        assert lib.lsl_encode_workspace_bytes(h, F, A) == want, (name, F, A)
        assert lib.lsl_encode_workspace_bytes(h, F, 0) == 0 and lib.lsl_encode_workspace_bytes(None, F, A) == 0
        lib.lsl_encoder_destroy(h)
