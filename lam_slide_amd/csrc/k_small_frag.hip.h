// The fragments the fp32 frame shares (k_small.hip.h, the output head of k_resident.hip.h, tools/experiments/k_head_scalar.hip.h), each written
// here once, so that "a trajectory has the same bits in any batch", "a sharded run draws exactly its slice of the noise stream" and "a record's
// update is the same whichever kernel applies it" hold because the kernels call the same functions, not because hand-written copies agree.
// Each fragment's ordering rule stands at its definition.  A site that still restates one says so in a line and names the section of
// profiles/small_fragments.txt that shows why.
#pragma once
#include "common.hip.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;

// ---- exact fp32 multiply-add on the matrix pipe, one float4 per operand and lane: the k values go through the pipe in x, y, z, w order, one
// rounding per product-and-add like fmaf; any k order is fine as long as both operands use the same one.
//   mfma32_f32x4   v_mfma_f32_32x32x2_f32: lane (r, hf) supplies A[row r][k] and B[k][col r] for k = {4 hf + e} of an 8-deep step
//   mfma16_f32x4   v_mfma_f32_16x16x4_f32: lane (r16, g4), k = {4 g4 + e} of a 16-deep step
__device__ __forceinline__ f32x16 mfma32_f32x4(float4 a, float4 b, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4v mfma16_f32x4(float4 a, float4 b, f32x4v c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 f32x16_zero() {
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.0f;
    return z;
}

// ---- the four-wave hand-over of a 32 x 32 tile whose k range the four waves of a workgroup split: Ps is PartTile[4] in LDS (the odd row stride
// keeps the scatter off one bank), an array or a pointer to the first tile; wave w leaves its partial tile at Ps[w][tile row][tile column] (lane
// (r, hf) owns column r, rows acc_row(e, hf)), and behind a barrier any thread reads element (row, col) as ((P0 + P1) + P2) + P3: wave order,
// whatever the launch.
typedef float PartTile[32][33];
constexpr int PART_FLOATS = 4 * 32 * 33;
template <class P>
__device__ __forceinline__ void part_scatter(P &Ps, int wave, int r, int hf, const f32x16 &acc) {
#pragma unroll
    for (int e = 0; e < 16; ++e) Ps[wave][acc_row(e, hf)][r] = acc[e];
}
template <class P>
__device__ __forceinline__ float part_sum(const P &Ps, int row, int col) {
    return ((Ps[0][row][col] + Ps[1][row][col]) + Ps[2][row][col]) + Ps[3][row][col];
}

// ---- the dense epilogue: out[b][o] = post(s + bias[o] + add[b % add_mod][o]) (add_mod = 0: add[b]; add null: no row), in this order - the
// conditioning rows of a trajectory differ between the three dense kernels by the k order of s alone.
template <bool POST_SILU>
__device__ __forceinline__ void dense_store(float *out, float s, float bias_o, const float *add, int b, int o, int O, int add_stride, int add_mod) {
    s += bias_o;
    if (add) s += add[(size_t)(add_mod ? b % add_mod : b) * add_stride + o];
    if (POST_SILU) s = silu(s);
    out[(size_t)b * O + o] = s;
}

// ---- LayerNorm and modulate, one element: (v - mean) rstd (1 + scale) + shift.  ln_mod takes the pre-added sc1 = 1 + scale of a caller that
// keeps it in a register, ln_mod_scale adds at the use; the same bits either way: the sum is rounded once, in front of the product.  (Two
// spellings because the place of the add in the statement decides hipcc's schedule: profiles/small_fragments.txt section 5c.)
__device__ __forceinline__ float ln_mod(float v, float mean, float rstd, float sc1, float shift) { return (v - mean) * rstd * sc1 + shift; }
__device__ __forceinline__ float ln_mod_scale(float v, float mean, float rstd, float scale, float shift) { return (v - mean) * rstd * (1.0f + scale) + shift; }

// ---- the sum of 256 values, one per thread of a 256-thread workgroup, through red[256] in LDS: the halving tree 128, 64, ..., 1 (thread t adds
// red[t + o] onto red[t]); every thread calls, the total comes back in every thread.
template <class T>
__device__ __forceinline__ T block_tree_sum(T *red, T v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// ---- the noise stream.  Philox4x32-10 + Box-Muller: standard normal for (seed, step, element).  Documented stream:
// counter = (elem/4 lo, elem/4 hi, step, 0), key = (seed lo, seed hi); element e takes output e % 4
// after Box-Muller on the pairs (r0,r1) -> (z0,z1), (r2,r3) -> (z2,z3).
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        const unsigned n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned step, unsigned long long elem) {
    const unsigned long long blk = elem >> 2;
    unsigned c[4] = {(unsigned)blk, (unsigned)(blk >> 32), step, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const int pair = (int)(elem & 2);
    const float u1 = ((float)c[pair] + 1.0f) * 2.3283064365386963e-10f;  // (0, 1]
    const float u2 = (float)c[pair + 1] * 2.3283064365386963e-10f;
    const float rad = sqrtf(-2.0f * __logf(u1));
    float sn, cs;
    __sincosf(6.283185307179586f * u2, &sn, &cs);
    return (elem & 1) ? rad * sn : rad * cs;
}
// A Rademacher draw from the same counters: +-1 for (seed, step, element) by the top bit of the element's output word
// (counter = (elem/4 lo, elem/4 hi, step, 0), key = (seed lo, seed hi), word elem % 4)
__device__ __forceinline__ float philox_sign(unsigned long long seed, unsigned step, unsigned long long elem) {
    const unsigned long long blk = elem >> 2;
    unsigned c[4] = {(unsigned)blk, (unsigned)(blk >> 32), step, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    return (c[elem & 3] >> 31) ? -1.0f : 1.0f;
}

// ---- a record's update of one state element (lsl_step_ex):  xn = ax x + am m;  += aw w[e];  += as saved[e];  x, trace, save_out <- xn, the
// terms added in this order.  e is the element's index in the launch's state (x, noise, trace, saved and save_out all point at the launch's first
// element); w[e] is the caller's noise[e], or element elem_offset + e of the stream above under the record's step index - the global index,
// which is what makes a shard's draw the slice of the unsharded one.  The host fills the struct in one place (step_update, host_eval.hip.h).
// (Pointers first: in this member order every k_head_step_mfma instance keeps its scalar-register spills at or below those of the loose
// parameters it replaces - profiles/small_fragments.txt section 5a.)
struct StepUpdate {
    const float *noise;          // caller-supplied draw of this record, or null: the device stream
    float *trace;                // or null: the record's slice of the trace
    const float *saved;          // or null: a state kept by an earlier record (Heun's x_hat)
    float *save_out;             // or null: keeps xn for a later record
    unsigned long long seed, elem_offset;
    float ax, am, aw, as;        // state, network output, noise, saved state
    unsigned step;               // the record's noise index = the stream's step word
};
__device__ __forceinline__ float step_noise(const float *noise, unsigned long long seed, unsigned step, unsigned long long elem_offset, size_t e) {
    return noise ? noise[e] : philox_normal(seed, step, elem_offset + e);
}
template <bool NET>  // NET false: a record without a network evaluation has no am term
__device__ __forceinline__ float step_value(const StepUpdate &u, size_t e, float x_old, float m) {
    float xn = NET ? u.ax * x_old + u.am * m : u.ax * x_old;
    if (u.aw != 0.0f) xn += u.aw * step_noise(u.noise, u.seed, u.step, u.elem_offset, e);
    if (u.saved) xn += u.as * u.saved[e];
    return xn;
}
template <bool NET>
__device__ __forceinline__ void step_apply(const StepUpdate &u, float *x, size_t e, float x_old, float m) {
    const float xn = step_value<NET>(u, e, x_old, m);
    x[e] = xn;
    if (u.trace) u.trace[e] = xn;
    if (u.save_out) u.save_out[e] = xn;
}
