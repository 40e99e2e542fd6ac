// The fragments the loss kernels share (k_siloss / k_geomloss / k_peptloss / k_disperr / k_classloss .hip.h): the team that owns a unit, the
// team's sums, and the fp64 totals of a table's columns - each written here once, so that the public contract of the per-frame sums holds
// because every kernel calls the same function, not because five reductions happen to agree.
//
// Determinism: no float atomics.  A unit (a frame, a sample trajectory) is owned by a team of 64 threads (up to 64 entities: one wave, four
// units per workgroup) or of 256 threads (one unit per workgroup); thread l of the team takes items l, l + TEAM, ... in ascending order into
// accumulators of its own, the wave sums by DPP (wave_sum_dpp: one fixed tree), the four waves of a 256-thread team are added in wave order.
// Every order is fixed by the unit's own shape: a unit's floats have the same bits whatever the batch, the grid, or the unit's place in
// either, and rows of different shards may be concatenated.  A final kernel adds rows in index order in fp64 - lane l adds rows l, l + 64,
// ..., thread k adds column k over the 64 lanes in lane order - and rounds each result once.  Each kernel header says only what is
// particular to it: its formulas, what it skips, its LDS layout.
#pragma once
#include "common.hip.h"

// ---- the team of a unit ----
inline int loss_team(long long entities) { return entities <= 64 ? 64 : 256; }  // host: a wave per unit up to 64 entities, the workgroup above

template <int TEAM>
struct LossTeam {  // of this thread, in a workgroup of 256: grid ceil(units / (256 / TEAM))
    static_assert(TEAM == 64 || TEAM == 256, "a wave or the workgroup");
    const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    const long long unit = (long long)blockIdx.x * (256 / TEAM) + team;
    const bool live;  // (the last workgroup of the 64-thread form may hold fewer than four units)
    __device__ __forceinline__ explicit LossTeam(long long units) : live(unit < units) {}
};
template <int TEAM>
inline unsigned loss_team_grid(long long units) { return (unsigned)((units + 256 / TEAM - 1) / (256 / TEAM)); }

// ---- the team's sums ----
// out(k, the team's sum of v[k]) for k < N, the caller's epilogue.  TEAM 64: the wave's sums, handed over by lane 0 of a live team, k
// ascending.  TEAM 256: the four waves' sums go through LDS and thread k of the workgroup adds value k in wave order (`live` is not looked
// at: the grid is the units); one barrier, so every thread of the workgroup calls.
template <int TEAM, int N, class Out>
__device__ __forceinline__ void team_sums(bool live, float (&v)[N], Out out) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum_dpp(v[k]);
    if constexpr (TEAM == 64) {
        if (live && (threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k) out(k, v[k]);
        }
    } else {
        __shared__ float wsum[4][N];
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k) wsum[threadIdx.x >> 6][k] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < N) out(threadIdx.x, ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x]);
    }
}

// ---- fp64 column totals ----
// s[k] += a[r * WA + k], s[WA + k] += b[r * WB + k] (WB == 0: one table) over the rows r = lane, lane + 64, ... below `rows` whose mask
// byte is nonzero (mask null: every row), both tables in one pass (their loads are in flight together); returns the number of rows added.
// The caller stores s to lane_sum[k][lane], places the barrier, and has thread k call lane_order_total.
template <int WA, int WB, class Index>
__device__ __forceinline__ double lane_rows_add(double *s, const float *a, const float *b, Index rows, int lane, const unsigned char *mask = nullptr) {
    double n = 0.0;
    for (Index r = lane; r < rows; r += 64) {
        if (mask && !mask[r]) continue;
#pragma unroll
        for (int k = 0; k < WA; ++k) s[k] += (double)a[(size_t)r * WA + k];
#pragma unroll
        for (int k = 0; k < WB; ++k) s[WA + k] += (double)b[(size_t)r * WB + k];
        n += 1.0;
    }
    return n;
}
__device__ __forceinline__ double lane_order_total(const double *col) {
    double tot = 0.0;
    for (int l = 0; l < 64; ++l) tot += col[l];
    return tot;
}

// ---- the quotient finals ----
// The table of a final: output o = column num / column den of the WA columns of table a followed by the WB of table b, one byte per output
// (num | den << 4) in a 64-bit kernel argument: thread o shifts its byte out, no table is read from memory behind the sums.
constexpr unsigned long long loss_quot(int o, int num, int den) { return (unsigned long long)(num | den << 4) << (8 * o); }

// out[o] = total of column num[o] / total of column den[o], o < NOUT, from a [F, WA] and b [F, WB] (WB == 0: one table): fp64 totals, each
// quotient rounded once; 0 / 0 = NaN like the reference.  One workgroup of 64 threads.
template <int WA, int WB, int NOUT>
__global__ void __launch_bounds__(64) k_loss_final(float *out, const float *a, const float *b, int F, unsigned long long quots) {
    __shared__ double lane_sum[WA + WB][64];
    double s[WA + WB] = {};
    lane_rows_add<WA, WB>(s, a, b, F, threadIdx.x);
#pragma unroll
    for (int k = 0; k < WA + WB; ++k) lane_sum[k][threadIdx.x] = s[k];
    __syncthreads();
    if (threadIdx.x < WA + WB) lane_sum[threadIdx.x][0] = lane_order_total(lane_sum[threadIdx.x]);
    __syncthreads();
    if (threadIdx.x < NOUT) {
        const unsigned q = (unsigned)(quots >> (8 * threadIdx.x));
        out[threadIdx.x] = (float)(lane_sum[q & 15][0] / lane_sum[(q >> 4) & 15][0]);
    }
}
