"""The fp32 stage-1 kernels (csrc/k_decode.hip.h: k_dec_ln, k_dec_gather, k_enc_context, k_enc_broadcast, k_dec_dense<0|1|2>,
k_dec_attn<16|32|64>) through Stage1Decoder / Stage1Encoder and the C ABI, at the case table of stage1_cases.py: every head tile of the
attention at padded and unpadded head widths (4 in 16, 16 in 16; 24 in 32, 32 in 32; 48 in 64, 64 in 64), key and query axes of one and
two passes of the 256-thread loops, the last key count each tile accepts (496 / 252 / 127) and the first one it refuses, input widths
that leave a k-loop remainder in k_dec_dense (4, 8, 12, 20, 36, 68, 132), LayerNorm rows of 4 .. 132 floats, no QK norm, no mask, a
fully masked frame, num_split = 5, two self / cross blocks.

Parity: relative L2 against the fp64 oracle, bar = the project's stage-1 bar 2e-6, or 5x the fp32 oracle's own distance from the fp64
oracle at that case where that is larger (computed here from the reference alone; 5x covers another summation order, __expf, rsqrtf).
Measured on MI355X (profiles/stage1_parity.txt); in brackets the fp32 oracle's own distance, which follows its BLAS:
  * decode, 16-tile: md17 3.6e-7 (1 key), 7.8e-7 at 300 latents [6.2-6.5e-7, bar 3.1-3.2e-6], 1.3e-6 at 496 [4.4-8.8e-7, bar 2.2-4.4e-6]
    (the sequential fp32 sums over 496 keys; both figures are under the flat 2e-6 as well); tiny 0.3-1.1e-7
  * decode, 32-tile: w32 1.6-5.2e-7, split5 1.4e-7, no QK norm 1.8e-7 [1.5-1.8e-7];  64-tile: w64 2.6e-7 [2.4-2.6e-7]
  * encode, every class, with and without the mask: 1.7-2.5e-7 [1.6-2.5e-7]
  every other bar is 2e-6.

Everything else is bit-exact: frame subsets, a reused handle, calls on side streams (each with a scratch buffer of its own), mask forms,
masked-out inputs, views and index types, clamped indices.
A key count beyond the tile is refused by `_lib.check` as every shape refusal of the library is (code -3, ValueError) with a message
that names the LDS tile."""
import ctypes as C

import pytest
import torch

import stage1_cases as sc
from conftest import parity, rel_l2

pytestmark = pytest.mark.gpu

STAGE1_BAR, MARGIN = 2e-6, 5.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_HANDLES = {}


def decoder(name, dev, fresh=False):
    from lam_slide_amd import Stage1Decoder
    if fresh or ("dec", name) not in _HANDLES:
        m = sc.decoder_model(name)
        d = Stage1Decoder(m.sd, device=dev, **m.ctor)
        if fresh:
            return d
        _HANDLES["dec", name] = d
    return _HANDLES["dec", name]


def encoder(name, dev, fresh=False):
    from lam_slide_amd import Stage1Encoder
    if fresh or ("enc", name) not in _HANDLES:
        m = sc.encoder_model(name)
        e = Stage1Encoder(m.sd, device=dev, **m.ctor)
        if fresh:
            return e
        _HANDLES["enc", name] = e
    return _HANDLES["enc", name]


def bar(ref_err):
    return max(STAGE1_BAR, MARGIN * ref_err)


# ---------------------------------------------------------------------------------------------------------- parity


@pytest.mark.parametrize("case", sc.DECODER_CASES, ids=sc.case_id)
def test_decode_parity(case, dev):
    name = case[0]
    c = sc.decoder_case(*case)
    dec = decoder(name, dev)
    m = sc.DECODER_MODELS[name]
    assert (dec.num_block_attn, dec.num_block_cross, dec.num_split, dec.qk_norm) == (m.n_self, m.n_cross, m.num_split, m.qk_norm)
    got = dec.decode(c.z.to(dev), c.entities.to(dev)).cpu()
    assert got.shape == c.want.shape and torch.isfinite(got).all()
    parity(f"s1.dec.{sc.case_id(case)}", rel_l2(got, c.want), bar(c.ref_err))


@pytest.mark.parametrize("case", sc.ENCODER_CASES, ids=sc.case_id)
def test_encode_parity(case, dev):
    name = case[0]
    c = sc.encoder_case(*case)
    enc = encoder(name, dev)
    m = sc.ENCODER_MODELS[name]
    assert (enc.num_block_cross, enc.num_block_attn, enc.qk_norm) == (m.n_cross, m.n_self, m.qk_norm)
    got = enc.encode(c.x.to(dev), c.entities.to(dev), c.mask.to(dev)).cpu()
    assert got.shape == c.want.shape and torch.isfinite(got).all()
    parity(f"s1.enc.{sc.case_id(case)}.mask", rel_l2(got, c.want), bar(c.ref_err))
    got = enc.encode(c.x.to(dev), c.entities.to(dev), None).cpu()
    assert torch.isfinite(got).all()
    parity(f"s1.enc.{sc.case_id(case)}.nomask", rel_l2(got, c.want_nomask), bar(c.ref_err_nomask))


# ---------------------------------------------------------------------------------------------------------- bits


def _slices(F):
    """Contiguous frame ranges [a, b) of a call of F >= 2 frames: every proper one for F = 2 and 3, a sample of five for larger F (first,
    last and middle frame, the run without the first and the run without the last frame)."""
    return sorted({(0, 1), (F - 1, F), (1, F), (0, F - 1), (F // 2, F // 2 + 1)})


@pytest.mark.parametrize("name", sorted(sc.DECODER_MULTI))
def test_decode_frame_subsets_views_and_index_types_keep_the_bits(name, dev):
    F, L, A = sc.DECODER_MULTI[name]
    c = sc.decoder_case(name, F, L, A)
    dec = decoder(name, dev)
    z, ent = c.z.to(dev), c.entities.to(dev)
    full = dec.decode(z, ent)
    for a, b in _slices(F):  # frames are independent: a contiguous subset (_slices: all of them up to F = 3, a sample beyond) keeps its bits
        assert torch.equal(dec.decode(z[a:b], ent[a:b]), full[a:b]), (a, b)
    # non-contiguous views: every other latent of a twice-as-long array, a transposed entity table; int32 indices
    wide = torch.empty(F, 2 * L, z.shape[-1], device=dev).fill_(7.0)
    wide[:, ::2] = z
    ent_t = ent.t().contiguous().t()
    assert not wide[:, ::2].is_contiguous() and (A == 1 or F == 1 or not ent_t.is_contiguous())
    assert torch.equal(dec.decode(wide[:, ::2], ent_t), full)
    assert torch.equal(dec.decode(z, ent.to(torch.int32)), full)
    assert torch.equal(dec.decode(z.transpose(0, 1).contiguous().transpose(0, 1), ent_t.to(torch.int32)), full)


@pytest.mark.parametrize("name", sorted(sc.ENCODER_MULTI))
def test_encode_frame_subsets_views_and_index_types_keep_the_bits(name, dev):
    F, A = sc.ENCODER_MULTI[name]
    c = sc.encoder_case(name, F, A)
    enc = encoder(name, dev)
    x, ent, mask = c.x.to(dev), c.entities.to(dev), c.mask.to(dev)
    full, full_nomask = enc.encode(x, ent, mask), enc.encode(x, ent, None)
    for a, b in _slices(F):
        assert torch.equal(enc.encode(x[a:b], ent[a:b], mask[a:b]), full[a:b]), (a, b)
        assert torch.equal(enc.encode(x[a:b], ent[a:b], None), full_nomask[a:b]), (a, b)
    wide = torch.empty(F, 2 * A, x.shape[-1], device=dev).fill_(7.0)
    wide[:, 1::2] = x
    ent_t, mask_t = ent.t().contiguous().t(), mask.t().contiguous().t()
    assert not wide[:, 1::2].is_contiguous()
    assert torch.equal(enc.encode(wide[:, 1::2], ent_t, mask_t), full)
    assert torch.equal(enc.encode(x, ent.to(torch.int32), mask), full)
    # mask forms: None = all true; bool = the same bytes as uint8 (any non-zero byte attends)
    assert torch.equal(enc.encode(x, ent, torch.ones_like(mask)), full_nomask)
    assert torch.equal(enc.encode(x, ent, mask.to(torch.uint8)), full)
    assert torch.equal(enc.encode(x, ent, mask.to(torch.uint8) * 255), full)
    # masked-out entities do not reach the latents, whatever they hold
    loud = x.clone()
    loud[~mask] = 1e3
    assert (~mask).any() and torch.equal(enc.encode(loud, ent, mask), full)


def test_decode_handle_reused_across_shapes_matches_fresh_handles(dev):
    """large -> small -> large on one handle (the workspace is allocated for the large shape and carved anew for each call) against a
    fresh handle per call."""
    for name, shapes in (("w32", ((1, 252, 130), (1, 1, 1), (3, 65, 21), (1, 252, 130))), ("w32_split5", ((2, 50, 7), (1, 1, 1), (2, 50, 7)))):
        dec = decoder(name, dev, fresh=True)
        for F, L, A in shapes:
            z, ent = (t.to(dev) for t in sc.decoder_inputs(name, F, L, A))
            assert torch.equal(dec.decode(z, ent), decoder(name, dev, fresh=True).decode(z, ent)), (name, F, L, A)


def test_encode_handle_reused_across_shapes_matches_fresh_handles(dev):
    enc = encoder("w32", dev, fresh=True)
    for F, A in ((2, 252), (1, 1), (3, 65), (2, 252)):
        x, ent, mask = (t.to(dev) for t in sc.encoder_inputs("w32", F, A))
        assert torch.equal(enc.encode(x, ent, mask), encoder("w32", dev, fresh=True).encode(x, ent, mask)), (F, A)


def test_scratch_is_per_stream_for_the_stage1_objects_and_the_model(dev):
    """One decoder / encoder called on the default stream and on two side streams: the same bits three times, a scratch buffer of its
    own per stream (two calls in flight on two streams never write the same LayerNorm, q/k/v and attention buffers), and the buffer of a
    stream reused by the next call on it.  ``LatentSIV3.workspace`` keeps its buffers the same way.  (The race of a shared buffer is
    not staged here: only who owns which buffer.)"""
    from lam_slide_amd import LatentSIV3
    dec, enc = decoder("tiny", dev, fresh=True), encoder("w32", dev, fresh=True)
    z, ent = (t.to(dev) for t in sc.decoder_inputs("tiny", 5, 3, 2))
    x, ent_e, mask = (t.to(dev) for t in sc.encoder_inputs("w32", 3, 65))
    side = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()  # the inputs are there before any side stream reads them

    def on(stream, run):
        with torch.cuda.stream(stream):
            out = run()
        stream.synchronize()
        return out

    for obj, run in ((dec, lambda: dec.decode(z, ent)), (enc, lambda: enc.encode(x, ent_e, mask))):
        buf = lambda stream: obj._scratch.buffers[dev, stream.cuda_stream]  # noqa: E731
        first = on(torch.cuda.current_stream(dev), run)
        main = buf(torch.cuda.current_stream(dev))
        assert torch.equal(on(side[0], run), first) and torch.equal(on(side[1], run), first)
        a, b = buf(side[0]), buf(side[1])
        assert len({main.data_ptr(), a.data_ptr(), b.data_ptr()}) == 3 and min(main.numel(), a.numel(), b.numel()) > 0
        assert torch.equal(on(side[0], run), first)
        assert buf(side[0]) is a and buf(side[1]) is b and len(obj._scratch.buffers) == 3
    net = LatentSIV3(depth=1, in_dim=8, hidden_size=64, num_heads=4)
    net.ensure_packed(dev)
    ws = lambda: net.workspace(2, 3, 5, dev)  # noqa: E731
    main, a, b = ws(), on(side[0], ws), on(side[1], ws)
    assert len({main.data_ptr(), a.data_ptr(), b.data_ptr()}) == 3 and min(main.numel(), a.numel(), b.numel()) > 0
    assert on(side[0], ws) is a and on(side[1], ws) is b and ws() is main


# ---------------------------------------------------------------------------------------------------------- boundaries


POISON = -12345.0


def _raw_decode(dec, z, ent, out):
    from lam_slide_amd import _lib
    lib = _lib.load()
    F, L, _ = z.shape
    A = ent.shape[1]
    ws = torch.empty(lib.lsl_decode_workspace_bytes(dec._handle, F, L, A), dtype=torch.uint8, device=z.device)
    _lib.check(lib.lsl_decode(dec._handle, z.data_ptr(), ent.data_ptr(), F, L, A, out.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream(z.device).cuda_stream))
    torch.cuda.synchronize()


def _raw_encode(enc, x, ent, out):
    from lam_slide_amd import _lib
    lib = _lib.load()
    F, A, _ = x.shape
    ws = torch.empty(lib.lsl_encode_workspace_bytes(enc._handle, F, A), dtype=torch.uint8, device=x.device)
    _lib.check(lib.lsl_encode(enc._handle, x.data_ptr(), ent.data_ptr(), None, F, A, out.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream(x.device).cuda_stream))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,last", [("md17", 496), ("w32", 252), ("w64", 127)])
def test_decode_key_limit_of_each_head_tile(name, last, dev):
    """L = the last key count of the self block's tile decodes (to finite values, into the caller's tensor); L + 1 is refused before the
    first attention launch and leaves the output untouched."""
    dec = decoder(name, dev)
    A = 5
    out = torch.full((1, A, dec.out_dim), POISON, device=dev)
    z, ent = (t.to(dev) for t in sc.decoder_inputs(name, 1, last, A))
    _raw_decode(dec, z, ent, out)
    assert torch.isfinite(out).all() and not (out == POISON).any()
    assert torch.equal(out, dec.decode(z, ent))
    out.fill_(POISON)
    z, ent = (t.to(dev) for t in sc.decoder_inputs(name, 1, last + 1, A))
    with pytest.raises(ValueError, match=f"{last + 1} keys exceed the LDS tile"):
        _raw_decode(dec, z, ent, out)
    torch.cuda.synchronize()
    assert (out == POISON).all()
    with pytest.raises(ValueError, match="LDS tile"):
        dec.decode(z, ent)


def test_decode_split_key_limit_is_counted_in_context_tokens(dev):
    """num_split = 5: the output block sees 5 L keys, so L = 50 (250 keys, in the case table) decodes and L = 51 (255 > 252) is refused,
    by the output block, after the self and cross blocks (51 and 7 keys) were enqueued: only the error is asserted."""
    dec = decoder("w32_split5", dev)
    z, ent = (t.to(dev) for t in sc.decoder_inputs("w32_split5", 2, 51, 7))
    with pytest.raises(ValueError, match="255 keys exceed the LDS tile"):
        dec.decode(z, ent)
    torch.cuda.synchronize()
    c = sc.decoder_case("w32_split5", 2, 50, 7)  # the handle still works
    assert rel_l2(dec.decode(c.z.to(dev), c.entities.to(dev)).cpu(), c.want) < bar(c.ref_err)


def test_encode_key_limit(dev):
    enc = encoder("w32", dev)
    x, ent, _ = (t.to(dev) for t in sc.encoder_inputs("w32", 1, 253))
    out = torch.full((1, enc.num_latents, enc.dim_latent), POISON, device=dev)
    with pytest.raises(ValueError, match="253 keys exceed the LDS tile"):
        _raw_encode(enc, x, ent, out)
    torch.cuda.synchronize()
    assert (out == POISON).all()
    _raw_encode(enc, x[:, :252].contiguous(), ent[:, :252].contiguous(), out)
    assert torch.isfinite(out).all()
    assert torch.equal(out, enc.encode(x[:, :252], ent[:, :252], None))


def test_create_refuses_widths_off_4_and_heads_wider_than_64(dev):
    from lam_slide_amd import Stage1Decoder, Stage1Encoder
    from lam_slide_amd.synthetic import seeded_decoder_state_dict, seeded_encoder_state_dict
    small = dict(in_dim=8, dim_latent=8, dim_query=8, dim_emb=8, num_head_latent=1, dim_head_latent=4, num_head_cross=1, dim_head_cross=4)
    heads = lambda kw: {k: kw[k] for k in ("num_head_latent", "dim_head_latent", "num_head_cross", "dim_head_cross")}  # noqa: E731
    Stage1Decoder(seeded_decoder_state_dict(**small), device=dev, **heads(small))
    for bad in (dict(in_dim=6), dict(dim_latent=10), dict(dim_query=9), dict(dim_emb=7), dict(num_head_cross=3, dim_head_cross=5),
                dict(num_head_latent=2, dim_head_latent=3)):
        kw = dict(small, **bad)
        with pytest.raises(ValueError, match="multiples of 4"):
            Stage1Decoder(seeded_decoder_state_dict(**kw), device=dev, **heads(kw))
    for bad in (dict(num_head_cross=4, dim_head_cross=65), dict(num_head_latent=4, dim_head_latent=65)):
        kw = dict(small, **bad)
        with pytest.raises(ValueError, match="dim_head must be 1..64"):
            Stage1Decoder(seeded_decoder_state_dict(**kw), device=dev, **heads(kw))
    kw = dict(small, num_head_cross=1, dim_head_cross=64, num_head_latent=1, dim_head_latent=64)  # 64 itself is accepted
    Stage1Decoder(seeded_decoder_state_dict(**kw), device=dev, **heads(kw))
    esmall = dict(dim_input=8, dim_latent=8, num_latents=3, dim_emb=8, num_head_latent=1, dim_head_latent=4, num_head_cross=1, dim_head_cross=4)
    Stage1Encoder(seeded_encoder_state_dict(**esmall), device=dev, **heads(esmall))
    for bad in (dict(dim_input=6), dict(dim_latent=10), dict(dim_emb=7), dict(num_head_cross=3, dim_head_cross=5)):
        kw = dict(esmall, **bad)
        with pytest.raises(ValueError, match="multiples of 4"):
            Stage1Encoder(seeded_encoder_state_dict(**kw), device=dev, **heads(kw))
    for bad in (dict(num_head_cross=4, dim_head_cross=65), dict(num_head_latent=4, dim_head_latent=65)):
        kw = dict(esmall, **bad)
        with pytest.raises(ValueError, match="dim_head must be 1..64"):
            Stage1Encoder(seeded_encoder_state_dict(**kw), device=dev, **heads(kw))


# ---------------------------------------------------------------------------------------------------------- masks and indices


def test_encode_fully_masked_frame_is_nan_and_leaves_its_neighbours(dev):
    """A frame without a real entity has no softmax: its latents are NaN, as in the oracle (test_stage1_cases.py), and the frames beside
    it keep their bits."""
    enc = encoder("w32", dev)
    c = sc.encoder_case("w32", 3, 65)
    x, ent, mask = c.x.to(dev), c.entities.to(dev), c.mask.to(dev)
    dead = mask.clone()
    dead[0] = False
    z, z_dead = enc.encode(x, ent, mask), enc.encode(x, ent, dead)
    assert torch.isnan(z_dead[0]).all() and torch.isfinite(z_dead[1:]).all()
    assert torch.equal(z_dead[1:], z[1:])
    want = sc.encode64("w32", c.x, c.entities, dead.cpu())
    assert torch.equal(torch.isnan(want), torch.isnan(z_dead.cpu()))


def test_entity_indices_first_last_and_clamped(dev):
    """Rows 0 and n_entities - 1 of the table are read exactly; an index outside the table reads the nearest row (k_dec_gather,
    k_enc_context), where the reference's nn.Embedding raises."""
    n = sc.N_ENTITIES
    ent = torch.tensor([[0, n - 1, -1, -2 ** 40, n, n + 5, 2 ** 40, 3]] * 2)
    clamped = torch.tensor([[0, n - 1, 0, 0, n - 1, n - 1, n - 1, 3]] * 2)
    for name in ("w32", "tiny"):
        dec = decoder(name, dev)
        z, _ = sc.decoder_inputs(name, 2, 9, 8)
        got = dec.decode(z.to(dev), clamped.to(dev))
        ref32, want = sc.decode32(name, z, clamped), sc.decode64(name, z, clamped)
        assert rel_l2(got.cpu(), want) < bar(rel_l2(ref32, want))
        assert torch.equal(dec.decode(z.to(dev), ent.to(dev)), got)
        assert torch.equal(got[:, 2], got[:, 0]) and torch.equal(got[:, 4], got[:, 1]) and not torch.equal(got[:, 0], got[:, 1])
        # the int32 form of the indices that fit
        assert torch.equal(dec.decode(z.to(dev), ent.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).to(dev)), got)
    enc = encoder("w32", dev)
    x, _, _ = sc.encoder_inputs("w32", 2, 8)
    got = enc.encode(x.to(dev), clamped.to(dev))
    ref32, want = sc.encode32("w32", x, clamped, None), sc.encode64("w32", x, clamped, None)
    assert rel_l2(got.cpu(), want) < bar(rel_l2(ref32, want))
    assert torch.equal(enc.encode(x.to(dev), ent.to(dev)), got)
