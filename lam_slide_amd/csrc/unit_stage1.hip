// The frozen stage-1 model's translation unit of liblamslide_hip.so (include/lsl_api.h): the encoder and decoder handles, lsl_encode,
// lsl_decode and lsl_decode_heads (every decoder head from one trunk).  decode_host.hip.h holds their scratch layout and launch helpers.
#include "decode_host.hip.h"

LSL_UNIT_INFO;

extern "C" {

int lsl_decoder_create(const lsl_decoder_desc *desc, const lsl_decoder_weights *w, lsl_decoder **out) try {
    if (!desc || !w || !out) return fail(-1, "null decoder argument");
    const lsl_decoder_desc &d = *desc;
    const bool rest = d.out_dim >= 1 && d.n_entities >= 1 && d.num_split >= 0;
    if (int rc = stage1_check("decoder", d, {d.in_dim, d.dim_latent, d.dim_query, d.dim_emb}, rest)) return rc;
    if (d.num_split > 1 && (!w->ext_w || !w->ext_b)) return fail(-2, "decoder with num_split > 1 needs the extender weights");
    return stage1_make(d, *w, out);
} LSL_API_CATCH

void lsl_decoder_destroy(lsl_decoder *d) { delete d; }

size_t lsl_decode_workspace_bytes(const lsl_decoder *d, int32_t frames, int32_t L, int32_t A) {
    if (!d || frames <= 0 || L <= 0 || A <= 0) return 0;
    return dec_carve(d->d, frames, L, A, nullptr, nullptr);
}

// Decoder.forward (decoder.py:88-102) after post_quant (lightning_base.py:28-31,42-44), up to the output block: leaves its rows
// [frames * A, dim_query] in ws.q.  Arguments already checked; -3 from a block whose keys exceed the LDS tile (nothing of a head is enqueued then).
static int decode_trunk(lsl_decoder *dec, const float *z, const int64_t *entities, int frames, int L, int A, const DecWs &ws, hipStream_t st) {
    const lsl_decoder_desc &d = dec->d;
    const lsl_decoder_weights &w = dec->w;
    const int nl = frames * L, na = frames * A;
    // post_quant: LayerNorm(C, elementwise_affine=False) then Linear(C, dim_latent)
    dec_ln(ws.xn, z, nullptr, nullptr, nl, d.in_dim, st);
    dec_dense(0, ws.lat, ws.xn, w.pq_w, w.pq_b, nullptr, nl, d.in_dim, d.dim_latent, st);
    // queries = query_mlp(entity_embedding(entities))   (dropout is identity in eval)
    hipLaunchKernelGGL(k_dec_gather, dim3((na + 3) / 4), dim3(256), 0, st, ws.xn, w.table, entities, na, d.dim_emb, d.n_entities);
    dec_dense(0, ws.q, ws.xn, w.qm_w, w.qm_b, nullptr, na, d.dim_emb, d.dim_query, st);
    for (int i = 0; i < d.num_block_attn; ++i)
        if (int rc = dec_block(w.self_blocks[i], ws.lat, L, d.dim_latent, nullptr, 0, 0, d.heads_latent, d.dim_head_latent, d.act, frames, ws, st)) return rc;
    for (int i = 0; i < d.num_block_cross; ++i)
        if (int rc = dec_block(w.cross_blocks[i], ws.lat, L, d.dim_latent, ws.q, A, d.dim_query, d.heads_cross, d.dim_head_cross, d.act, frames, ws, st)) return rc;
    const float *ctx = ws.lat;
    int Lc = L;
    if (d.num_split > 1) {  // extender: 1x1 conv D -> D*N per latent, "B (D N) L -> B (L N) D"; the host reordered the rows to (N, D)
        dec_dense(0, ws.ext, ws.lat, w.ext_w, w.ext_b, nullptr, nl, d.dim_latent, d.num_split * d.dim_latent, st);
        ctx = ws.ext;
        Lc = L * d.num_split;
    }
    return dec_block(w.out_block, ws.q, A, d.dim_query, ctx, Lc, d.dim_latent, d.heads_cross, d.dim_head_cross, d.act, frames, ws, st);
}

// output_layers.<name> on the trunk's rows: Linear(dim_query, dim_query), act, Linear(dim_query, out_dim).  ws.hid is rewritten head after
// head: the stream orders a head's second launch before the next head's first.
static void decode_head(const lsl_decoder_desc &d, const lsl_decoder_head &h, float *out, int na, const DecWs &ws, hipStream_t st) {
    dec_dense(d.act, ws.hid, ws.q, h.w1, h.b1, nullptr, na, d.dim_query, d.dim_query, st);
    dec_dense(0, out, ws.hid, h.w2, h.b2, nullptr, na, d.dim_query, h.out_dim, st);
}

// lsl_decode = the one-head case (the handle's own head); lsl_decode_heads = the caller's heads on one trunk
static int decode_call(lsl_decoder *dec, const lsl_decoder_head *heads, int n_heads, const float *z, const int64_t *entities, int frames, int L, int A,
                       float *const *outs, void *workspace, size_t workspace_bytes, hipStream_t st, const char *name) {
    if (frames <= 0 || L <= 0 || A <= 0) return fail(-3, "decode: empty input");
    const lsl_decoder_desc &d = dec->d;
    if (workspace_bytes < dec_carve(d, frames, L, A, nullptr, nullptr) || !workspace) return fail(-4, "decode workspace too small");
    DecWs ws;
    dec_carve(d, frames, L, A, (char *)workspace, &ws);
    if (int rc = decode_trunk(dec, z, entities, frames, L, A, ws, st)) return rc;
    for (int h = 0; h < n_heads; ++h) decode_head(d, heads[h], outs[h], frames * A, ws, st);
    LSL_CHECK_LAUNCH(name);
    return 0;
}

int lsl_decode(lsl_decoder *dec, const float *z, const int64_t *entities, int32_t frames, int32_t L, int32_t A, float *out, void *workspace,
               size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!dec || !z || !entities || !out) return fail(-1, "null decode argument");
    const lsl_decoder_head own{dec->w.head_w1, dec->w.head_b1, dec->w.head_w2, dec->w.head_b2, dec->d.out_dim};
    return decode_call(dec, &own, 1, z, entities, frames, L, A, &out, workspace, workspace_bytes, (hipStream_t)stream, "lsl_decode");
} LSL_API_CATCH

int lsl_decode_heads(lsl_decoder *dec, const lsl_decoder_head *heads, int32_t n_heads, const float *z, const int64_t *entities, int32_t frames,
                     int32_t L, int32_t A, float *const *outs, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!dec || !heads || !z || !entities || !outs) return fail(-1, "null decode argument");
    if (n_heads < 1 || n_heads > LSL_DECODE_MAX_HEADS) return fail(-3, "decode: n_heads = %d outside 1..%d", n_heads, LSL_DECODE_MAX_HEADS);
    for (int h = 0; h < n_heads; ++h) {
        if (!heads[h].w1 || !heads[h].b1 || !heads[h].w2 || !heads[h].b2 || !outs[h]) return fail(-1, "null decode argument (head %d)", h);
        if (heads[h].out_dim < 1) return fail(-3, "decode: head %d has out_dim = %d", h, heads[h].out_dim);
    }
    return decode_call(dec, heads, n_heads, z, entities, frames, L, A, outs, workspace, workspace_bytes, (hipStream_t)stream, "lsl_decode_heads");
} LSL_API_CATCH

int lsl_encoder_create(const lsl_encoder_desc *desc, const lsl_encoder_weights *w, lsl_encoder **out) try {
    if (!desc || !w || !out) return fail(-1, "null encoder argument");
    const lsl_encoder_desc &d = *desc;
    if (int rc = stage1_check("encoder", d, {d.dim_input, d.dim_emb, d.dim_latent}, d.num_latents >= 1 && d.n_entities >= 1)) return rc;
    return stage1_make(d, *w, out);
} LSL_API_CATCH

void lsl_encoder_destroy(lsl_encoder *e) { delete e; }

size_t lsl_encode_workspace_bytes(const lsl_encoder *e, int32_t frames, int32_t A) {
    if (!e || frames <= 0 || A <= 0) return 0;
    return enc_carve(e->d, frames, A, nullptr, nullptr);
}

// quant(Encoder.forward(x, entities, mask))   (encoder.py:96-103, lightning_base.py:37-40)
int lsl_encode(lsl_encoder *enc, const float *x, const int64_t *entities, const unsigned char *mask, int32_t frames, int32_t A, float *out,
               void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!enc || !x || !entities || !out) return fail(-1, "null encode argument");
    if (frames <= 0 || A <= 0) return fail(-3, "encode: empty input");
    const lsl_encoder_desc &d = enc->d;
    const lsl_encoder_weights &w = enc->w;
    if (workspace_bytes < enc_carve(d, frames, A, nullptr, nullptr) || !workspace) return fail(-4, "encode workspace too small");
    hipStream_t st = (hipStream_t)stream;
    DecWs ws;
    enc_carve(d, frames, A, (char *)workspace, &ws);
    float *ctx = ws.q;
    const int N = d.num_latents, nl = frames * N, na = frames * A, dim_ctx = d.dim_input + d.dim_emb;
    // prepare_inputs of EncoderBase: context = mlp(cat(x, entity_embedding(entities))), latents = the learned array per frame
    hipLaunchKernelGGL(k_enc_context, dim3((na + 3) / 4), dim3(256), 0, st, ws.xn, x, w.table, entities, na, d.dim_input, d.dim_emb, d.n_entities);
    dec_dense(d.act, ws.hid, ws.xn, w.mlp_w1, w.mlp_b1, nullptr, na, dim_ctx, d.dim_latent, st);
    dec_dense(0, ctx, ws.hid, w.mlp_w2, w.mlp_b2, nullptr, na, d.dim_latent, dim_ctx, st);
    const long total = (long)nl * d.dim_latent;
    hipLaunchKernelGGL(k_enc_broadcast, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws.lat, w.latents, total, N * d.dim_latent);
    for (int i = 0; i < d.num_block_cross; ++i)
        if (int rc = dec_block(w.cross_blocks[i], ws.lat, N, d.dim_latent, ctx, A, dim_ctx, d.heads_cross, d.dim_head_cross, d.act, frames, ws, st, mask)) return rc;
    for (int i = 0; i < d.num_block_attn; ++i)
        if (int rc = dec_block(w.self_blocks[i], ws.lat, N, d.dim_latent, nullptr, 0, 0, d.heads_latent, d.dim_head_latent, d.act, frames, ws, st)) return rc;
    // quant: Linear(dim_latent, dim_latent) then LayerNorm(dim_latent, elementwise_affine=False)
    dec_dense(0, ws.hid, ws.lat, w.quant_w, w.quant_b, nullptr, nl, d.dim_latent, d.dim_latent, st);
    dec_ln(out, ws.hid, nullptr, nullptr, nl, d.dim_latent, st);
    LSL_CHECK_LAUNCH("lsl_encode");
    return 0;
} LSL_API_CATCH

}  // extern "C"
