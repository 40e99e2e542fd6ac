"""The case table of the stage-1 encode / decode tests (test_stage1_cases.py on the CPU, test_hip_stage1.py on the MI355X): model
classes that reach every instance of k_dec_attn (head tiles of 16, 32 and 64 floats, at padded and unpadded head widths), the k-loop
remainder of k_dec_dense (input widths that are no multiple of 16), LayerNorm rows narrower than a wave or no multiple of 64, the
variant without QK norm and the query splitter at num_split = 5; shapes at one and two passes of the 256-thread staging and query loops
and at the last key count each head tile accepts.  State dicts come from ``lam_slide_amd.synthetic`` (unchanged: its draws feed the
benchmark and the other tests); the reference is ``oracle.harness`` with every parameter and input cast to fp64, computed once per case
and shared.  Not a test module.

The key limit of one attention call is the LDS tile of k_dec_attn, (2 * keys * tile + keys) * 4 <= 65536 bytes with tile = 16 / 32 / 64
floats for dim_head <= 16 / <= 32 / <= 64: 496 / 252 / 127 keys.  In the decoder a self block has L keys, a cross block A keys, the
output block L * num_split keys; in the encoder a cross block has A keys and a self block num_latents keys."""
import functools
from collections import namedtuple

import torch

from lam_slide_amd.synthetic import seeded_decoder_state_dict, seeded_encoder_state_dict
from oracle import harness

KEY_LIMIT = {16: 496, 32: 252, 64: 127}  # keys per attention call by head tile
N_ENTITIES = 32

# latent / cross: (heads, dim_head) of the self blocks / of the cross and output blocks
DecoderRow = namedtuple("DecoderRow", "in_dim dim_latent dim_query dim_emb latent cross n_self n_cross out_dim act num_split qk_norm")
DECODER_MODELS = {
    "md17": DecoderRow(32, 32, 128, 128, (2, 16), (8, 16), 1, 0, 3, "gelu_erf", 0, True),
    "w32": DecoderRow(8, 96, 36, 20, (3, 32), (2, 24), 1, 1, 3, "gelu_tanh", 0, True),
    "w64": DecoderRow(4, 132, 68, 4, (1, 64), (3, 48), 2, 0, 42, "gelu_erf", 0, True),
    "tiny": DecoderRow(12, 4, 4, 8, (1, 4), (1, 4), 0, 0, 1, "gelu_erf", 0, True),
}
DECODER_MODELS["w32_split5"] = DECODER_MODELS["w32"]._replace(num_split=5)
DECODER_MODELS["w32_noqk"] = DECODER_MODELS["w32"]._replace(qk_norm=False)
# (model, frames, L, A)
DECODER_CASES = (
    ("md17", 1, 1, 1), ("md17", 2, 300, 270), ("md17", 1, 496, 5),
    ("w32", 1, 1, 1), ("w32", 3, 65, 21), ("w32", 1, 252, 130),
    ("w64", 3, 65, 21), ("w64", 1, 127, 127),
    ("tiny", 1, 1, 1), ("tiny", 5, 3, 2),
    ("w32_split5", 2, 50, 7),
    ("w32_noqk", 3, 65, 21),
)
# the multi-frame case of each model class (frame subsets, views, index types)
DECODER_MULTI = {"md17": (2, 300, 270), "w32": (3, 65, 21), "w64": (3, 65, 21), "tiny": (5, 3, 2), "w32_split5": (2, 50, 7),
                 "w32_noqk": (3, 65, 21)}

EncoderRow = namedtuple("EncoderRow", "dim_input dim_emb dim_latent num_latents cross latent n_cross n_self act qk_norm")
ENCODER_MODELS = {
    "md17": EncoderRow(128, 128, 32, 192, (8, 16), (2, 16), 1, 1, "gelu_erf", True),
    "w32": EncoderRow(12, 20, 96, 70, (2, 24), (3, 32), 2, 1, "gelu_tanh", True),
    "w64": EncoderRow(4, 4, 132, 127, (3, 48), (1, 64), 1, 1, "gelu_erf", True),
}
ENCODER_MODELS["w32_noqk"] = ENCODER_MODELS["w32"]._replace(qk_norm=False)
# (model, frames, A)
ENCODER_CASES = (
    ("md17", 1, 1), ("md17", 2, 300),
    ("w32", 3, 65), ("w32", 2, 252),
    ("w64", 2, 127),
    ("w32_noqk", 3, 65),
)
ENCODER_MULTI = {"md17": (2, 300), "w32": (3, 65), "w64": (2, 127), "w32_noqk": (3, 65)}

# lsl_decode_workspace_bytes / lsl_encode_workspace_bytes of every case, in the order of the case tables, recorded from the library as it
# was before dec_carve and enc_carve were put on one carve function: callers size their scratch by these, the carve must keep them
DECODE_WORKSPACE_BYTES = (4736, 2810880, 2097664, 4416, 832768, 1083200, 990656, 668608, 512, 4544, 2152448, 832768)
ENCODE_WORKSPACE_BYTES = (1106944, 4042752, 912000, 2053632, 1276224, 912000)

Model = namedtuple("Model", "sd shape ctor")  # state dict, oracle.harness shape, keyword arguments of Stage1Decoder / Stage1Encoder
DecoderCase = namedtuple("DecoderCase", "z entities want ref_err")
EncoderCase = namedtuple("EncoderCase", "x entities mask want want_nomask ref_err ref_err_nomask")


def case_id(case):
    return case[0] + "-" + "x".join(str(n) for n in case[1:])


def _seed(name, *dims):
    s = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    for d in dims:
        s = s * 1009 + d
    return s % (2 ** 31 - 1)


def _drop_qk_norm(sd):
    return {k: v for k, v in sd.items() if not k.endswith((".norm.query_norm.scale", ".norm.key_norm.scale"))}


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def decoder_model(name):
    r = DECODER_MODELS[name]
    in_dim, dl, dq, de, (hl, dhl), (hc, dhc) = r.in_dim, r.dim_latent, r.dim_query, r.dim_emb, r.latent, r.cross
    n_self, n_cross, out_dim, act, split, qk = r.n_self, r.n_cross, r.out_dim, r.act, r.num_split, r.qk_norm
    sd = seeded_decoder_state_dict(in_dim=in_dim, dim_latent=dl, dim_query=dq, dim_emb=de, n_entities=N_ENTITIES, num_head_latent=hl,
                                   dim_head_latent=dhl, num_head_cross=hc, dim_head_cross=dhc, num_block_attn=n_self,
                                   num_block_cross=n_cross, out_dim=out_dim, seed=_seed("dec." + name.split("_")[0]))
    if split:  # DecoderQuerySplitter: Conv1d(D, D * N, 1), PyTorch-default range of fan_in D
        g = torch.Generator().manual_seed(_seed("ext." + name))
        sd["decoder.extender.1.weight"] = (torch.rand(dl * split, dl, 1, generator=g) * 2 - 1) / dl ** 0.5
        sd["decoder.extender.1.bias"] = (torch.rand(dl * split, generator=g) * 2 - 1) / dl ** 0.5
    if not qk:
        sd = _drop_qk_norm(sd)
    shape = harness.DecoderShape(dim_latent=dl, dim_query=dq, dim_head_cross=dhc, dim_head_latent=dhl, num_head_cross=hc, num_head_latent=hl,
                                 num_block_cross=n_cross, num_block_attn=n_self, qk_norm=qk, n_entities=N_ENTITIES, out_pos=out_dim, act=act)
    ctor = dict(num_head_latent=hl, dim_head_latent=dhl, num_head_cross=hc, dim_head_cross=dhc, act=act)
    return Model(sd, shape, ctor)


@functools.lru_cache(maxsize=None)
def encoder_model(name):
    r = ENCODER_MODELS[name]
    di, de, dl, nl, (hc, dhc), (hl, dhl) = r.dim_input, r.dim_emb, r.dim_latent, r.num_latents, r.cross, r.latent
    n_cross, n_self, act, qk = r.n_cross, r.n_self, r.act, r.qk_norm
    sd = seeded_encoder_state_dict(dim_input=di, dim_latent=dl, num_latents=nl, dim_emb=de, n_entities=N_ENTITIES, num_head_cross=hc,
                                   dim_head_cross=dhc, num_head_latent=hl, dim_head_latent=dhl, num_block_cross=n_cross,
                                   num_block_attn=n_self, seed=_seed("enc." + name.split("_")[0]))
    if not qk:
        sd = _drop_qk_norm(sd)
    shape = harness.EncoderShape(dim_input=di, dim_latent=dl, num_latents=nl, dim_head_cross=dhc, dim_head_latent=dhl, num_head_cross=hc,
                                 num_head_latent=hl, num_block_cross=n_cross, num_block_attn=n_self, qk_norm=qk, act=act)
    ctor = dict(num_head_cross=hc, dim_head_cross=dhc, num_head_latent=hl, dim_head_latent=dhl, act=act)
    return Model(sd, shape, ctor)


def decoder_inputs(name, frames, L, A):
    g = torch.Generator().manual_seed(_seed("dec.in." + name, frames, L, A))
    z = torch.randn(frames, L, DECODER_MODELS[name].in_dim, generator=g)
    entities = torch.randint(0, N_ENTITIES, (frames, A), generator=g)
    return z, entities


def encoder_inputs(name, frames, A):
    """x, entities and the ragged mask (rand < 0.6, column 0 forced true: no frame is empty)."""
    g = torch.Generator().manual_seed(_seed("enc.in." + name, frames, A))
    x = torch.randn(frames, A, ENCODER_MODELS[name].dim_input, generator=g)
    entities = torch.randint(0, N_ENTITIES, (frames, A), generator=g)
    mask = torch.rand(frames, A, generator=g) < 0.6
    mask[:, 0] = True
    return x, entities, mask


def decode32(name, z, entities):
    m = decoder_model(name)
    with torch.no_grad():
        return harness.decode(m.sd, m.shape, z, entities)


def decode64(name, z, entities):
    m = decoder_model(name)
    with torch.no_grad():
        return harness.decode(to64(m.sd), m.shape, z.double(), entities)


def encode32(name, x, entities, mask):
    m = encoder_model(name)
    with torch.no_grad():
        return harness.encode(m.sd, m.shape, x, entities, mask)


def encode64(name, x, entities, mask):
    m = encoder_model(name)
    with torch.no_grad():
        return harness.encode(to64(m.sd), m.shape, x.double(), entities, mask)


@functools.lru_cache(maxsize=None)
def decoder_case(name, frames, L, A):
    """Inputs, the fp64 oracle's output and the fp32 oracle's relative L2 distance from it (the reference's own rounding at this case)."""
    z, entities = decoder_inputs(name, frames, L, A)
    want = decode64(name, z, entities)
    return DecoderCase(z, entities, want, harness.rel_l2(decode32(name, z, entities), want))


@functools.lru_cache(maxsize=None)
def encoder_case(name, frames, A):
    x, entities, mask = encoder_inputs(name, frames, A)
    want, want_nomask = encode64(name, x, entities, mask), encode64(name, x, entities, None)
    return EncoderCase(x, entities, mask, want, want_nomask, harness.rel_l2(encode32(name, x, entities, mask), want),
                       harness.rel_l2(encode32(name, x, entities, None), want_nomask))
