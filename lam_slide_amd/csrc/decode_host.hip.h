// Host side of lsl_decode / lsl_encode: the handles, what their two create calls check and build alike (stage1_check, stage1_make), the
// scratch layout of a call (stage1_carve, sized by dec_carve / enc_carve) and the launch helpers of the frozen stage-1 decode and encode
// (kernels in k_decode.hip.h; the entry points themselves in unit_stage1.hip).
#pragma once
#include <algorithm>
#include <initializer_list>
#include <new>
#include <vector>

#include "../../include/lsl_api.h"
#include "host_api.hip.h"
#include "k_decode.hip.h"

struct lsl_encoder {
    lsl_encoder_desc d;
    lsl_encoder_weights w;
    std::vector<lsl_dec_block> cross_blocks, self_blocks;
};

struct lsl_decoder {
    lsl_decoder_desc d;
    lsl_decoder_weights w;
    std::vector<lsl_dec_block> self_blocks, cross_blocks;
};

namespace {

struct DecWs {
    float *lat, *q, *xn, *cn, *qb, *kvb, *att, *hid, *ext;
};

inline size_t dec_align(size_t n) { return (n + 63) & ~(size_t)63; }

// The scratch of one call, shared by decode and encode: every size in floats, the buffers in this order, each aligned to 64 bytes; returns
// the total in bytes (base == nullptr: the size alone).  `rows` x `dmax` / `imax` hold a LayerNorm output, q | k | v, the attention output
// and the feed-forward hidden layer of the longer of the two token sets.
size_t stage1_carve(size_t lat, size_t q, size_t rows, int dmax, int inner_l, int inner_c, size_t ext, char *base, DecWs *ws) {
    const int imax = std::max(3 * inner_l, 2 * inner_c);
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(base + off) : nullptr;
        off += dec_align(floats * sizeof(float));
        return p;
    };
    DecWs w;
    w.lat = take(lat);
    w.q = take(q);
    w.xn = take(rows * dmax);
    w.cn = take(rows * dmax);
    w.qb = take(rows * imax);
    w.kvb = take(rows * imax);
    w.att = take(rows * std::max(inner_l, inner_c));
    w.hid = take(rows * dmax);
    w.ext = ext ? take(ext) : nullptr;
    if (ws) *ws = w;
    return off;
}

size_t dec_carve(const lsl_decoder_desc &d, int frames, int L, int A, char *base, DecWs *ws) {
    const int split = d.num_split > 1 ? d.num_split : 1;
    const size_t nl = (size_t)frames * L, na = (size_t)frames * A;
    const int dmax = std::max(std::max(d.dim_latent, d.dim_query), std::max(d.in_dim, d.dim_emb));
    return stage1_carve(nl * d.dim_latent, na * d.dim_query, std::max(nl * split, na), dmax, d.heads_latent * d.dim_head_latent,
                        d.heads_cross * d.dim_head_cross, split > 1 ? nl * split * d.dim_latent : 0, base, ws);
}

// latents [frames * N, dim_latent]; ws->q is the context [frames * A, dim_ctx]
size_t enc_carve(const lsl_encoder_desc &d, int frames, int A, char *base, DecWs *ws) {
    const size_t nl = (size_t)frames * d.num_latents, na = (size_t)frames * A;
    const int dim_ctx = d.dim_input + d.dim_emb;
    return stage1_carve(nl * d.dim_latent, na * dim_ctx, std::max(nl, na), std::max(dim_ctx, d.dim_latent), d.heads_latent * d.dim_head_latent,
                        d.heads_cross * d.dim_head_cross, 0, base, ws);
}

// What lsl_decoder_create and lsl_encoder_create check alike (`what` is "decoder" / "encoder", `dims` the widths beside the two
// attention widths, `rest` whether their own fields are in range) ...
template <class Desc>
int stage1_check(const char *what, const Desc &d, std::initializer_list<int> dims, bool rest) {
    bool ragged = (d.heads_latent * d.dim_head_latent) % 4 || (d.heads_cross * d.dim_head_cross) % 4;
    for (int w : dims) ragged |= w % 4 != 0;
    if (ragged) return fail(-3, "%s widths must be multiples of 4", what);
    if (d.dim_head_latent > 64 || d.dim_head_cross > 64 || d.dim_head_latent < 1 || d.dim_head_cross < 1) return fail(-3, "%s dim_head must be 1..64", what);
    if (d.act != 1 && d.act != 2) return fail(-3, "%s activation must be 1 (erf GELU) or 2 (tanh GELU)", what);
    if (d.num_block_attn < 0 || d.num_block_cross < 0 || !rest) return fail(-3, "bad %s description", what);
    return 0;
}

// ... and the handle they make: the description, the pointers, and its own copy of the two block vectors.
template <class Handle, class Desc, class Weights>
int stage1_make(const Desc &d, const Weights &w, Handle **out) {
    Handle *h = new (std::nothrow) Handle();
    if (!h) return fail(-5, "out of host memory");
    h->d = d;
    h->w = w;
    if (d.num_block_attn) h->self_blocks.assign(w.self_blocks, w.self_blocks + d.num_block_attn);
    if (d.num_block_cross) h->cross_blocks.assign(w.cross_blocks, w.cross_blocks + d.num_block_cross);
    h->w.self_blocks = h->self_blocks.data();
    h->w.cross_blocks = h->cross_blocks.data();
    *out = h;
    return 0;
}

void dec_ln(float *out, const float *in, const float *w, const float *b, int rows, int D, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_ln, dim3((rows + 3) / 4), dim3(256), 0, st, out, in, w, b, rows, D, 1e-5f);
}

void dec_dense(int act, float *out, const float *in, const float *W, const float *bias, const float *res, int rows, int I, int O,
               hipStream_t st) {
    const dim3 grid((O + 63) / 64, (rows + 63) / 64);
    if (act == 1) hipLaunchKernelGGL((k_dec_dense<1>), grid, dim3(256), 0, st, out, in, W, bias, res, rows, I, O);
    else if (act == 2) hipLaunchKernelGGL((k_dec_dense<2>), grid, dim3(256), 0, st, out, in, W, bias, res, rows, I, O);
    else hipLaunchKernelGGL((k_dec_dense<0>), grid, dim3(256), 0, st, out, in, W, bias, res, rows, I, O);
}

int dec_attn(const DecAttnArgs &a, int frames, hipStream_t st) {
    const size_t lds = ((size_t)2 * a.Sk * (a.dh <= 16 ? 16 : a.dh <= 32 ? 32 : 64) + a.Sk) * sizeof(float);
    if (a.dh > 64 || lds > 64 * 1024) return fail(-3, "decode attention: dim_head %d / %d keys exceed the LDS tile", a.dh, a.Sk);
    const dim3 grid(frames * a.H);
    if (a.dh <= 16) hipLaunchKernelGGL((k_dec_attn<16>), grid, dim3(256), lds, st, a);
    else if (a.dh <= 32) hipLaunchKernelGGL((k_dec_attn<32>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((k_dec_attn<64>), grid, dim3(256), lds, st, a);
    return 0;
}

// x <- x + to_out(attention(LN(x), LN_c(ctx)));  x <- x + FF(LN(x))     (torch_modules.py:221-264)
// x: [frames * Sx, dim]; ctx: [frames * Sc, cdim] or nullptr (self-attention)
int dec_block(const lsl_dec_block &b, float *x, int Sx, int dim, const float *ctx, int Sc, int cdim, int H, int dh, int act, int frames,
              const DecWs &ws, hipStream_t st, const unsigned char *key_mask = nullptr) {
    const int inner = H * dh, nx = frames * Sx;
    dec_ln(ws.xn, x, b.ln_w, b.ln_b, nx, dim, st);
    DecAttnArgs a{};
    a.q_scale = b.q_scale;
    a.k_scale = b.k_scale;
    a.key_mask = key_mask;
    a.dh = dh;
    a.H = H;
    a.Sq = Sx;
    a.out = ws.att;
    a.ldo = inner;
    if (!ctx) {
        dec_dense(0, ws.qb, ws.xn, b.w_q, nullptr, nullptr, nx, dim, 3 * inner, st);  // to_qkv, chunk(3) = column thirds
        a.q = ws.qb;
        a.k = ws.qb + inner;
        a.v = ws.qb + 2 * inner;
        a.ldq = a.ldk = a.ldv = 3 * inner;
        a.Sk = Sx;
    } else {
        const int nc = frames * Sc;
        dec_ln(ws.cn, ctx, b.lnc_w, b.lnc_b, nc, cdim, st);
        dec_dense(0, ws.qb, ws.xn, b.w_q, nullptr, nullptr, nx, dim, inner, st);
        dec_dense(0, ws.kvb, ws.cn, b.w_kv, nullptr, nullptr, nc, cdim, 2 * inner, st);  // to_kv, chunk(2)
        a.q = ws.qb;
        a.ldq = inner;
        a.k = ws.kvb;
        a.v = ws.kvb + inner;
        a.ldk = a.ldv = 2 * inner;
        a.Sk = Sc;
    }
    if (int rc = dec_attn(a, frames, st)) return rc;
    dec_dense(0, x, ws.att, b.w_out, b.b_out, x, nx, inner, dim, st);
    dec_ln(ws.xn, x, b.ff_ln_w, b.ff_ln_b, nx, dim, st);
    dec_dense(act, ws.hid, ws.xn, b.ff_w1, b.ff_b1, nullptr, nx, dim, dim, st);
    dec_dense(0, x, ws.hid, b.ff_w2, b.ff_b2, x, nx, dim, dim, st);
    return 0;
}

}  // namespace
