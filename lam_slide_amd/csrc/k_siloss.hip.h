// Stochastic-interpolant objective around one network evaluation (lsl_si_loss / lsl_si_reduce): the interpolant in front
// (path.py:124-134) and the per-trajectory mean squared residual behind (transport.py:135-154, utils.py mean_flat).
// For every path x prediction x loss weight the reference's loss of trajectory b is affine in (pred, x1, x0):
//      xt     = alpha_b x1 + sigma_b x0
//      r      = p_b pred + q1_b x1 + q0_b x0
//      loss_b = w_b mean(r^2)
// The host derives the six numbers per trajectory (lam_slide_amd/transport.py: si_rows); the device never learns about paths or predictions -
// the same idea as the affine step records of the samplers.  Bandwidth-bound passes over B * T*L*C floats next to a network that moves
// thousands of bytes per token.
//
// Orders (k_loss_frag.hip.h; the team is the workgroup): a trajectory is cut into slabs of a FIXED 4096 elements (a constant: not a function
// of B, T, L or the pass size); inside a slab thread i owns elements 4 (i + 256 j) + k (j, k = 0..3) and adds their squares in (j, k) order;
// the slabs of a trajectory are added in fp64 and rounded once.  A trajectory's loss has the same bits in any batch, shard or pass.  The
// 16-byte and the scalar access forms read the same elements into the same registers: which one runs (alignment) does not change a bit.
#pragma once
#include "common.hip.h"
#include "k_loss_frag.hip.h"

#define LSL_SI_SLAB_ELEMS 4096

struct SiRow {  // = lsl_si_row (include/lsl_api.h)
    float alpha, sigma, p, q1, q0, w;
};

// xt = alpha_b x1 + sigma_b x0, b = element / per.  VEC: per % 4 == 0 and 16-byte aligned pointers, one float4 per thread and round
// (a float4 never straddles two trajectories); otherwise one float.
template <bool VEC>
__global__ void __launch_bounds__(256) k_si_mix(float *xt, const float *x1, const float *x0, const SiRow *rows, unsigned long long per,
                                                unsigned long long total) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    if (VEC) {
        const unsigned long long n4 = total >> 2;
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            const unsigned long long b = (i << 2) / per;
            const float al = rows[b].alpha, sg = rows[b].sigma;
            const float4 a = reinterpret_cast<const float4 *>(x1)[i];
            const float4 z = reinterpret_cast<const float4 *>(x0)[i];
            float4 o;
            o.x = fmaf(al, a.x, sg * z.x);
            o.y = fmaf(al, a.y, sg * z.y);
            o.z = fmaf(al, a.z, sg * z.z);
            o.w = fmaf(al, a.w, sg * z.w);
            reinterpret_cast<float4 *>(xt)[i] = o;
        }
    } else {
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
            const unsigned long long b = i / per;
            xt[i] = fmaf(rows[b].alpha, x1[i], rows[b].sigma * x0[i]);
        }
    }
}

// partial[b * slabs + s] = sum over slab s of trajectory b of (p pred + q1 x1 + q0 x0)^2.  grid (slabs, B), 256 threads.
template <bool VEC>
__global__ void __launch_bounds__(256) k_si_loss_partial(float *partial, const float *pred, const float *x1, const float *x0, const SiRow *rows,
                                                         unsigned long long per) {
    __shared__ float wsum[4];
    const unsigned b = blockIdx.y;
    const SiRow r = rows[b];
    const unsigned long long base = (unsigned long long)b * per;
    const unsigned long long e0 = (unsigned long long)blockIdx.x * LSL_SI_SLAB_ELEMS;  // first element of the slab inside the trajectory
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long e = e0 + 4ull * (threadIdx.x + 256u * j);
        float m[4], a[4], z[4];
        if (VEC) {
            if (e < per) {  // (per % 4 == 0: the four elements are inside together)
                const float4 m4 = *reinterpret_cast<const float4 *>(pred + base + e);
                const float4 a4 = *reinterpret_cast<const float4 *>(x1 + base + e);
                const float4 z4 = *reinterpret_cast<const float4 *>(x0 + base + e);
                m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w;
                a[0] = a4.x, a[1] = a4.y, a[2] = a4.z, a[3] = a4.w;
                z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) m[k] = a[k] = z[k] = 0.0f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = e + k < per;
                m[k] = in ? pred[base + e + k] : 0.0f;
                a[k] = in ? x1[base + e + k] : 0.0f;
                z[k] = in ? x0[base + e + k] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // (an element outside the trajectory contributes an exact +0)
            const float v = fmaf(r.q0, z[k], fmaf(r.q1, a[k], r.p * m[k]));  // (explicit: both access forms contract alike)
            s = fmaf(v, v, s);
        }
    }
    s = wave_sum_dpp(s);  // (team_sums<256> of one value, written out: through the fragment this kernel gains an instruction, profiles/loss_fragments.txt)
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// loss[b] = w_b / per * sum_s partial[b * slabs + s]: lane l adds slabs l, l + 64, ... in index order, lane 0 adds the 64 lanes in lane order;
// fp64 throughout, rounded once.  grid B, 64 threads.
__global__ void __launch_bounds__(64) k_si_loss_final(float *loss, const float *partial, const SiRow *rows, int slabs, unsigned long long per) {
    __shared__ double lane_sum[64];
    const unsigned b = blockIdx.x;
    const float *p = partial + (size_t)b * slabs;
    double s = 0.0;
    lane_rows_add<1, 0>(&s, p, nullptr, slabs, threadIdx.x);
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[b] = (float)((double)rows[b].w * lane_order_total(lane_sum) / (double)per);
}
