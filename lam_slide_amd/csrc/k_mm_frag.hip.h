// The fragments the matrix kernels share (k_lin1 / k_lin2 / k_tail / k_gemm / k_resident .hip.h), each written here once, so that "these
// kernels give the same bits" holds because they call the same functions, not because hand-written copies agree.  Index arithmetic is
// constexpr and checked by static_assert where it is defined.  A site that still restates a fragment says so in one line and names the line
// of profiles/matmul_fragments.txt that shows why (k_linear1_ts and k_linear2_ws stay instruction for instruction what they were).
#pragma once
#include <type_traits>

#include "common.hip.h"

// ---- compile-time integers, one spelling on the host and in the kernels: ic<N>() is a value whose type carries N; static_for<N>(f) calls
// f(ic<0>()), ..., f(ic<N - 1>()) in order ----
template <int N>
using ic = std::integral_constant<int, N>;
template <int N, int I = 0, class F>
__host__ __device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(ic<I>());
        static_for<N, I + 1>(f);
    }
}

// ---- token -> trajectory, token -> position: n / d by multiply-high: magic = floor(2^32 / d) + 1 (0 when d == 1, host: magic_of), exact for n d
// < 2^32 - the host admits no pass beyond that.  A trajectory is tokens_per_traj consecutive tokens; the position of token n inside its sequence
// is (n / pos_div) % pos_mod.
__device__ __forceinline__ unsigned magic_div(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }
__device__ __forceinline__ unsigned token_pos(unsigned n, unsigned div_magic, unsigned mod_magic, int pos_mod) {
    const unsigned n1 = magic_div(n, div_magic);
    return mod_magic ? n1 - __umulhi(n1, mod_magic) * (unsigned)pos_mod : 0u;
}

// ---- linear1's epilogue arithmetic (mmdit.py:129-148, 85-90) in the accumulator layout: a lane owns one token and, of a 32-feature tile, rows
// acc_row(e, hf): RoPE pairs (2 k, 2 k + 1) are lane-local and the other half of a head's sum of squares sits on lane ^ 32.  qk_factor: the head's
// RMS-norm factor from this lane's partial sum, times `post` (q: softmax scale x log2 e; k: 1); both lanes of a token get the same bits
// (half_pair_sum).  rope_rows: the lane's rows of the rotation table [n_pos][HDP / 2] x (c s0, sn s1, sn s0, c s1), the QK-norm scales folded in
// (k_rope_scaled): pair k of the lane sits at 4 (k >> 1) + (k & 1) behind its half's first pair 2 hf.  rope_pair: the pair (x0, x1) rotated and
// normed, two roundings per output after the factor.
__device__ __forceinline__ float qk_factor(float ss, float inv_hd, float post) { return rsqrtf(fmaf(half_pair_sum(ss), inv_hd, 1e-6f)) * post; }
template <int HDP, int NCO>
__device__ __forceinline__ void rope_rows(float4 (&co)[NCO], const float4 *tab, unsigned pos, int hf) {
    const float4 *t = tab + (size_t)pos * (HDP / 2) + 2 * hf;
#pragma unroll
    for (int k = 0; k < NCO; ++k) co[k] = t[4 * (k >> 1) + (k & 1)];
}
__device__ __forceinline__ void rope_pair(float rr, float4 cf, float x0, float x1, float &o0, float &o1) {
    o0 = rr * fmaf(cf.x, x0, -cf.y * x1);
    o1 = rr * fmaf(cf.z, x0, cf.w * x1);
}

// ---- linear2's gated residual update (latent_si_v31.py:53,60) on four consecutive features: h + gate (acc + bias), one add, one fma per element
// - the rounding every linear2 form shares.  (k_resident starts its accumulators from the bias and has no add: another rounding, its own line.)
__device__ __forceinline__ float4 gate_update4(float4 gt, float a0, float a1, float a2, float a3, float4 bias, float4 h) {
    h.x = fmaf(gt.x, a0 + bias.x, h.x);
    h.y = fmaf(gt.y, a1 + bias.y, h.y);
    h.z = fmaf(gt.z, a2 + bias.z, h.z);
    h.w = fmaf(gt.w, a3 + bias.w, h.w);
    return h;
}

// ---- a lane id the compiler cannot see through: hipcc hoists every per-lane address derived from the lane id out of the loops around it and
// keeps them alive across the main loops - as scratch spills; derived from this copy, made where they are used, they stay next to their use.
__device__ __forceinline__ int opaque_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// ---- an accumulator tile started from a bias row: the bias of a 32-feature block is the chain's initial value (no add in the epilogue): `row`
// points at the lane's first four features (4 hf) of the block's 32 in LDS; register group q4 is features 8 q4 + 4 hf .. + 3.
template <class Ptr>
__device__ __forceinline__ void acc_from_bias(f32x16 &a, Ptr row) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4_t b = row[2 * q4];
        a[4 * q4] = b[0]; a[4 * q4 + 1] = b[1]; a[4 * q4 + 2] = b[2]; a[4 * q4 + 3] = b[3];
    }
}

// ---- stream_store16 (inline asm on purpose): a streaming ("nt") 16-byte store at a 32-bit per-lane offset against a uniform base, invisible to
// hipcc's waitcnt pass (it would drain the LDS-DMA requests in flight in front of the next LDS access).  FRESH: the base may come straight from a
// scalar ALU instruction (5 wait states, nothing pads them inside asm).
template <bool FRESH>
__device__ __forceinline__ void stream_store16(unsigned voff, u32x4 v, const void *base) {
    if (FRESH) asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(base) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(base) : "memory");
}

// ---- the wave-private staging image: 32 (or more) rows of 128 bytes = eight 16-byte chunks; chunk c of row t sits in slot c ^ key(t), so that
// column-wise accesses in the accumulator layout (32 rows, one chunk) and row-wise ones (8 lanes per row, 8 rows per instruction) both spread
// over the banks.
//   stage_off       key = t & 7: the output images (linear1's bf16 slab, linear2's and the tail's fp32 rows, the residual rows of k_linear2_ws)
//   stage_off_pair  key = (t >> 1) & 7: a NAMED VARIANT, not the same layout - the operand images: swz_bk<64> of the tile GEMM (two rows
//                   of a fragment read share a bank group), and the row-wise lines -> B fragments transposition of line_to_frags below
//   swz_bk<32>      64-byte rows of four chunks, key = (t >> 2) & 3: the tile GEMM's BK = 32 stage image
//   res_swz         k_resident's images of 256-byte chunk groups (a: one group per row, z: three): key = t & 15 inside the group;
//                   returns the offset inside the row
__host__ __device__ __forceinline__ constexpr int stage_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
__host__ __device__ __forceinline__ constexpr int stage_off_pair(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
template <int BK>
__host__ __device__ __forceinline__ constexpr int swz_bk(int row, int chunk) {
    if (BK == 64) return stage_off_pair(row, chunk);
    return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4);
}
__host__ __device__ __forceinline__ constexpr int res_swz(int row, int chunk) { return ((chunk & ~15) | ((chunk ^ row) & 15)) << 4; }

// Checked here: each image holds every (row, chunk) of its 32 x 8 once; stage_off equals the forms it replaced (EpiLinear1::soff and
// swz_bk<64> had the very bodies above; stage_off<8>; k_tail's (c ^ row) & 7) and the per-lane forms that stay written out, as their sites
// spell them: k_linear1_ts put_group wr0 ^ (64 ii + 16 q) and flush_read rd0 + 1024 k (k_tail's wr_row likewise), k_linear2_ws epi_math and
// its h_request / epi_store (slot (row, lane & 7) holds chunk (lane & 7) ^ (row & 7): the XOR is its own inverse), finish_x of k_linear1_ts.
constexpr bool staging_forms_agree() {
    bool seen[2][256] = {};
    for (int row = 0; row < 32; ++row)
        for (int c = 0; c < 8; ++c) {
            const int o = stage_off(row, c), p = stage_off_pair(row, c);
            if ((o & 15) || (p & 15) || o >> 12 || p >> 12 || seen[0][o >> 4] || seen[1][p >> 4]) return false;
            seen[0][o >> 4] = seen[1][p >> 4] = true;
            if (o != (row * 8 + (c ^ (row & (8 - 1)))) << 4 || o != row * 128 + (((c ^ row) & 7) << 4)) return false;
        }
    for (int lane = 0; lane < 64; ++lane) {
        const int r = lane & 31, hf = lane >> 5, tr = lane >> 3, c = lane & 7;
        const int wr0 = r * 128 + 8 * hf + ((r & 7) << 4), rd0 = tr * 128 + ((c ^ (tr & 7)) << 4);
        for (int q = 0; q < 4; ++q) {
            if ((wr0 ^ (16 * q)) != stage_off(r, q) + 8 * hf || (wr0 ^ (64 + 16 * q)) != stage_off(r, 4 + q) + 8 * hf) return false;
            if (rd0 + 1024 * q != stage_off(8 * q + tr, c) || q * 1024 + lane * 16 != stage_off(8 * q + tr, c ^ (tr & 7))) return false;
            if (r * 128 + 16 * ((2 * q + hf) ^ (r & 7)) != stage_off(r, 2 * q + hf)) return false;
            if ((tr + 8 * q) * 128 + (((c ^ ((tr >> 1) + 4 * q)) & 7) << 4) != stage_off_pair(tr + 8 * q, c)) return false;
            if (r * 128 + ((((2 * q + hf) ^ (r >> 1)) & 7) << 4) != stage_off_pair(r, 2 * q + hf)) return false;
        }
    }
    return stage_off_pair(2, 0) != stage_off(2, 0);  // (the variant is another layout)
}
static_assert(staging_forms_agree(), "the staging image: one-to-one, and every site that restates it agrees with it");

// ---- row-wise lines -> MFMA B fragments, through the staging image: a wave's 32 rows of a [tokens][K] bf16 matrix arrive as whole 128-byte
// lines (8 lanes per row, 8 rows per instruction: 8 cache lines, where a fragment-shaped load of one k-step touches 32: load_lines); line j of
// every row holds the k-steps 4 j .. 4 j + 3.  line_to_frags turns one line (4 row-wise registers: register q = row (lane >> 3) + 8 q, chunk lane
// & 7) into its 4 fragments in place: written row-wise into the stage_off_pair image at `st` (an LDS byte address), read back as lane (r, hf),
// k-step m = chunk 2 m + hf of row r.  Conflict-free both ways.
template <int NK, class X>
__device__ __forceinline__ void load_lines(X &xreg, const u16 *src, int n0, int stride, int lane) {  // NK k-steps = NK / 4 lines of rows n0 .. n0 + 31
    const u16 *xr = src + (size_t)(n0 + (lane >> 3)) * stride + 8 * (lane & 7);
#pragma unroll
    for (int j = 0; j < NK / 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) xreg[4 * j + q] = as_bf16x8(*reinterpret_cast<const u32x4 *>(xr + (size_t)(8 * q) * stride + 64 * j));
}
__device__ __forceinline__ void line_to_frags(bf16x8 (&x4)[4], unsigned st, int lane) {
    const int chunk = lane & 7, rowi = lane >> 3, r = lane & 31, hf = lane >> 5;
    const unsigned xw = st + rowi * 128, xr0 = st + r * 128;
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<LDS_PTR(u32x4)>(xw + 1024 * q + (((chunk ^ ((rowi >> 1) + 4 * q)) & 7) << 4)) = as_u32x4(x4[q]);
#pragma unroll
    for (int m = 0; m < 4; ++m) x4[m] = as_bf16x8(*reinterpret_cast<const LDS_PTR(u32x4)>(xr0 + ((((2 * m + hf) ^ (r >> 1)) & 7) << 4)));
}

// ---- weights row-major -> MFMA A-fragment order: the A operand of an MFMA over ROWS feature rows (32: mfma32, 16-deep k-steps; 16: k_resident's
// 16x16x32, 32-deep): lane (r = lane % ROWS, g = lane / ROWS) of k-step ks reads the 8 elements W[f0 + r][k0 + (512 / ROWS) ks + 8 g ..].  The
// pack kernels write those 16 bytes at (tile, ks, lane), so that every fragment load of a kernel is 1 KiB contiguous.  Element offset into a
// row-major W of row length K:
template <int ROWS>
__host__ __device__ __forceinline__ constexpr size_t afrag_src(int f0, int k0, int ks, int lane, int K) {
    return (size_t)(f0 + (lane & (ROWS - 1))) * K + k0 + (512 / ROWS) * ks + 8 * (lane / ROWS);
}
static_assert(afrag_src<32>(64, 0, 3, 37, 1536) == (size_t)(64 + 5) * 1536 + 16 * 3 + 8 && afrag_src<16>(32, 0, 2, 37, 384) == (size_t)(32 + 5) * 384 + 32 * 2 + 16,
              "lane (r, hf) of mfma32, lane (r16, g4) of the 16x16x32 MFMA");
