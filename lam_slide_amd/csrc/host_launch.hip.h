// The sampling path's launch rules: one launch helper per kernel family - grid / LDS arithmetic of a chosen kernel - and, next to it, the
// rule that chooses among the family's instances (which depends on the model and on T, L only where results could differ, never on the
// batch).  The sub-block's rules (linear1, attention, linear2 / tail) are asked by plan_pass (host_eval.hip.h) only: their launchers are a
// switch over what the plan says.  Each family's instances are listed ONCE (LSL_LIN1_TS_INSTANCES, LSL_LIN2_WS_INSTANCES; the switches of
// launch_gemm and launch_attention_t), and a gate that depends on a kernel's LDS need asks the kernel's own config for it.
#pragma once
#include <atomic>
#include <type_traits>

#include "host_common.hip.h"

namespace {

// One launch of the output head (run_head fills it): the rows h [n, D] with their modulation rows, the projection, and either `out` or
// the record's update u of x (do_step)
struct HeadArgs {
    float *x, *out;
    const float *h, *shift, *scale;
    int mod_stride;
    const float *Wo, *bo;
    int n, C, tpt, do_step;
    StepUpdate u;
};

// Rejected structures and A/B arms (ping-pong / drain GEMMs, tilings 6 / 8 / 13-18 / 23-26 / 29, the scalar output head k_head_step of
// tools/experiments/k_head_scalar.hip.h, every LSL_* tuning knob) live in tools/experiments/host_launch_experiments.hip.h, on the include path
// of tools/build_experiments.sh only; the product has empty hooks.
#ifdef LSL_EXPERIMENTS
constexpr bool lsl_experiments = true;
template <int NE, int VEC>
bool launch_head_experiment(const HeadArgs &, hipStream_t);
template <class Epi>
bool launch_gemm_experiment(int, const GemmArgs &, const Epi &, hipStream_t, bool);
#else
constexpr bool lsl_experiments = false;
template <int NE, int VEC>
bool launch_head_experiment(const HeadArgs &, hipStream_t) { return false; }
template <class Epi>
bool launch_gemm_experiment(int, const GemmArgs &, const Epi &, hipStream_t, bool) { return false; }
#endif

int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
// Kernel-selection / timing knobs (LSL_GEMM*, LSL_NT, LSL_STAGGER, LSL_PROBE, ...): read from the environment only in
// -DLSL_EXPERIMENTS builds; the product library always runs its measured defaults.
int tune_int(const char *name, int dflt) { return lsl_experiments ? env_int(name, dflt) : dflt; }

int device_cus() {  // of the current device (entry points switch to the stream's device first)
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int n = cache[dev & 63].load(std::memory_order_relaxed);
    if (n > 0) return n;
    n = 256;
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    if (n <= 0) n = 256;
    cache[dev & 63].store(n, std::memory_order_relaxed);
    return n;
}

constexpr size_t LDS_BUDGET = 160 * 1024;  // LDS a workgroup may use (gfx950: 160 KiB per CU)

// ---- launch helpers -------------------------------------------------------------------------------

template <int NE, int VEC>
void launch_ln_mod_t(u16 *a, const float *h, const float *shift, const float *scale, int stride, int n, int tpt, hipStream_t st) {
    if constexpr (NE % 4 == 0) {
        static const int persist = tune_int("LSL_LN_PERSIST", 16);  // workgroups per CU of the persistent form; 0 = one wave per token
        if (persist > 0) {
            const int grid = std::min((n + 3) / 4, device_cus() * persist);
            static const int nt = (tune_int("LSL_NT", 3) >> 3) & 1;
            hipLaunchKernelGGL((k_ln_modulate_v4<NE>), dim3(grid), dim3(256), 0, st, a, h, shift, scale, stride, n, tpt, nt);
            return;
        }
    }
    hipLaunchKernelGGL((k_ln_modulate<NE, VEC>), dim3((n + 3) / 4), dim3(256), 0, st, a, h, shift, scale, stride, n, tpt);
}
template <int NE, int VEC>
void launch_ln_inplace_t(float *h, int n, float eps, hipStream_t st) {
    hipLaunchKernelGGL((k_ln_inplace<NE, VEC>), dim3((n + 3) / 4), dim3(256), 0, st, h, n, eps);
}
template <int NE, int VEC>
void launch_head_mfma(const HeadArgs &a, hipStream_t st, Profiler *pr = nullptr) {
    if (launch_head_experiment<NE, VEC>(a, st)) return;  // (-DLSL_EXPERIMENTS builds only)
    auto kern = k_head_step_mfma<NE, VEC>;
    const size_t lds = head_mfma_lds_bytes<NE>(a.C <= 32);
    LSL_ALLOW_LDS(kern, head_mfma_lds_bytes<NE>(false));
    // two workgroups per CU where the LDS image allows it (any hidden size with <= 32 channels): one workgroup's LayerNorm / weight-load latencies under the other's MFMAs
    static const int per_cu = tune_int("LSL_HEAD_PER_CU", 2);
    const int wgs = device_cus() * (per_cu >= 2 && 2 * lds <= LDS_BUDGET ? 2 : 1);
    if (pr) pr->label(4, "k_head_step_mfma<%d, %d> (%s, %d per CU)", NE, VEC, a.C <= 32 ? "one slab" : "cycled slabs", wgs / device_cus());
    hipLaunchKernelGGL(kern, dim3(std::min((a.n + HEAD_TOK - 1) / HEAD_TOK, wgs)), dim3(256), lds, st, a.x, a.out, a.h, a.shift, a.scale, a.mod_stride,
                       a.Wo, a.bo, a.n, a.C, a.tpt, a.do_step, a.u);
}
// a record without a network evaluation, on the n elements behind x (k_state_affine)
void launch_state_affine(float *x, unsigned long long n, const StepUpdate &u, hipStream_t st) {
    hipLaunchKernelGGL(k_state_affine, dim3((unsigned)std::min<unsigned long long>((n + 255) / 256, 2048)), dim3(256), 0, st, x, n, u);
}

#define DISPATCH_D(D, FN, ...)                          \
    switch ((D) / 64) {                                 \
        case 1: FN<1, 1>(__VA_ARGS__); break;           \
        case 2: FN<2, 2>(__VA_ARGS__); break;           \
        case 3: FN<3, 1>(__VA_ARGS__); break;           \
        case 4: FN<4, 2>(__VA_ARGS__); break;           \
        case 5: FN<5, 1>(__VA_ARGS__); break;           \
        case 6: FN<6, 2>(__VA_ARGS__); break;           \
        case 7: FN<7, 1>(__VA_ARGS__); break;           \
        default: FN<8, 2>(__VA_ARGS__); break;          \
    }

// (stats / npad: ln_fuse handles, launch_embed<1> only - the rows' statistics for the first sub-block's fused LayerNorm; embed_stats_ok says where)
bool embed_stats_ok(int C, int D) { return C <= 32 && D % 256 == 0 && D <= 512; }
template <int MODE>
int launch_embed(float *out, const float *in, const float *W, const float *b, const float *b2, const float *me,
                 const int64_t *mask, const float *base, int n, int C, int D, hipStream_t st, float2 *stats = nullptr, int npad = 0,
                 Profiler *pr = nullptr) {  // (pr: the launch leaves its label under profile class 5)
    if (C > 32 && C % 8 == 0 && C <= 128 && D % 32 == 0) {  // wide inputs: fp32 MFMA form (k_embed_mfma)
        const int tpw = 3, ngrp = (D / 32 + tpw - 1) / tpw;
        const long units = (long)((n + 31) / 32) * ngrp;
        const dim3 g((unsigned)((units + 3) / 4));
        if (pr) pr->label(5, "k_embed_mfma<%d, %d> (32-token tiles)", MODE, C / 8);
        switch (C / 8) {
#define LSL_EMB_CASE(CK) case CK: hipLaunchKernelGGL((k_embed_mfma<MODE, CK>), g, dim3(256), 0, st, out, in, W, b, b2, me, mask, base, n, C, D, tpw); return 0;
            LSL_EMB_CASE(5) LSL_EMB_CASE(6) LSL_EMB_CASE(7) LSL_EMB_CASE(8) LSL_EMB_CASE(9) LSL_EMB_CASE(10) LSL_EMB_CASE(11) LSL_EMB_CASE(12)
            LSL_EMB_CASE(13) LSL_EMB_CASE(14) LSL_EMB_CASE(15) LSL_EMB_CASE(16)
#undef LSL_EMB_CASE
        }
    }
    // persistent workgroups (weights fetched once each) over tiles of 64 tokens
    int tok = EMB_TOK;
    // 32 inputs, hidden <= 512 (every shipped narrow-input model): the weight rows reach the registers through LDS (k_embed), which makes
    // a workgroup's prologue cheap enough for 32- or 16-token tiles when the launch has fewer than two 64-token tiles per CU
    static const int stage = tune_int("LSL_EMBED_LDS", 1);
    const bool w_lds = stage && C == 32 && D % 4 == 0 && D <= 512;
    if (w_lds)
        while (tok > 16 && (n + tok - 1) / tok < 2 * device_cus()) tok /= 2;
    const dim3 grid(std::min((n + tok - 1) / tok, 2 * device_cus())), blk(256);
    const bool with_stats = stats && MODE == 1 && C <= 32 && embed_stats_ok(C, D);
    if (pr)
        pr->label(5, "k_embed<%d, %d, %d%s> (%d-token tiles%s)", C <= 32 ? 32 : C <= 64 ? 64 : C <= 96 ? 96 : 128, MODE, C <= 32 ? 4 : C <= 96 ? 2 : 1,
                  with_stats ? ", true" : "", tok, w_lds ? ", weights through LDS" : (C & 3) ? ", scalar weight loads" : "");
    if (C <= 32) {
        const size_t lds = w_lds ? embed_w_lds_bytes<32, 4>(D) : 0;
        if (with_stats) {
            auto kern = k_embed<32, 1, 4, true>;
            LSL_ALLOW_LDS(kern, (embed_w_lds_bytes<32, 4>(512)));
            hipLaunchKernelGGL(kern, grid, blk, lds, st, out, in, W, b, b2, me, mask, base, n, C, D, w_lds ? 1 : 0, tok, stats, npad);
            return 0;
        }
        auto kern = k_embed<32, MODE, 4>;
        LSL_ALLOW_LDS(kern, (embed_w_lds_bytes<32, 4>(512)));
        hipLaunchKernelGGL(kern, grid, blk, lds, st, out, in, W, b, b2, me, mask, base, n, C, D, w_lds ? 1 : 0, tok, (float2 *)nullptr, 0);
    } else if (C <= 64) hipLaunchKernelGGL((k_embed<64, MODE, 2>), grid, blk, 0, st, out, in, W, b, b2, me, mask, base, n, C, D, 0, tok, (float2 *)nullptr, 0);
    else if (C <= 96) hipLaunchKernelGGL((k_embed<96, MODE, 2>), grid, blk, 0, st, out, in, W, b, b2, me, mask, base, n, C, D, 0, tok, (float2 *)nullptr, 0);
    else hipLaunchKernelGGL((k_embed<128, MODE, 1>), grid, blk, 0, st, out, in, W, b, b2, me, mask, base, n, C, D, 0, tok, (float2 *)nullptr, 0);
    return 0;
}

template <int BF, int BT, int NWF, int NWT, int BK, int NS, bool PERSIST, class Epi>
void launch_gemm_glds(const GemmArgs &g, const Epi &epi, hipStream_t st) {
    auto kern = k_gemm_glds<BF, BT, NWF, NWT, BK, NS, PERSIST, Epi>;
    // + the bias vector of the whole GEMM, kept in LDS by epilogues that start the accumulators from it (k_gemm.hip.h)
    const size_t lds = GemmCfg<BF, BT, NWF, NWT, BK, NS, PERSIST, Epi>::lds_bytes + (Epi::lds_bias ? (size_t)((g.F + BF - 1) / BF) * BF * 4 : 0);
    LSL_ALLOW_LDS(kern, LDS_BUDGET);
    const int tiles = ((g.N + BT - 1) / BT) * ((g.F + BF - 1) / BF);
    int grid = tiles;
    if (PERSIST) {  // as many workgroups as fit at once (LDS-limited), a multiple of 8 so the XCD mapping stays regular
        const int per_cu = (int)std::max<size_t>(1, LDS_BUDGET / lds);
        grid = device_cus() * per_cu;
        grid -= grid % 8;
        if (grid > tiles) grid = tiles;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NWF * NWT * 64), lds, st, g, epi);
}

}  // namespace

#ifdef LSL_EXPERIMENTS
#include "host_launch_experiments.hip.h"  // (needs launch_gemm_glds / device_cus above)
#endif

namespace {

// linear1 on the token-stationary kernel (k_lin1.hip.h): hidden sizes 128 / 256 / 384 / 512, sections (q | k | v | mlp) on multiples of 64
// features.  Same bits as the tile kernels below (tools/lin1_harness.hip), so the choice between them may depend on the launch size.
// The kernel lives in unit_lin1.hip (its own compile options); k_lin1.hip.h gives this unit the configuration, THE instance list
// (LSL_LIN1_TS_INSTANCES: gates and launch go through it) and lsl_lin1_launch.
template <class Fn>
bool with_linear1_ts_instance(int hdp, int D, Fn &&fn) {  // fn(head width, hidden) as integral constants; false: no such instance
#define X(H, K) if (hdp == H && D == K) return fn(ic<H>{}, ic<K>{}), true;
    LSL_LIN1_TS_INSTANCES(X)
#undef X
    return false;
}
template <int HDP, int K, int NW = 8, bool LNF = false>
void launch_linear1_ts_t(const Lin1Args &a, hipStream_t st) {
    using C = Lin1Cfg<HDP, K, NW>;
    const int ntile = (a.N + C::TT - 1) / C::TT, nb = a.F / 32;
    const long units = (long)ntile * nb;
    int grid = (int)std::min<long>(device_cus(), units / 2);
    Lin1Args b = a;
    // fewer tiles than workgroups: whole workgroups per tile, one segment each (k_lin1.hip.h "Work split"); same bits either way
    static const int align = tune_int("LSL_LIN1_ALIGN", 1);
    const int wpt = std::min(device_cus() / ntile, nb / 2);
    b.wpt = align && wpt >= 2 ? wpt : 0;
    if (b.wpt) grid = b.wpt * ntile;
    lsl_lin1_launch(HDP, K, NW, LNF, b, grid, LNF ? C::lds_bytes_lnf(a.F) : C::lds_bytes(a.F), st);
}
// K = 512, few tokens (md17_bench B = 1: 7 680): 4-wave workgroups on 128-token tiles - twice the tiles, half the activation prologue per
// workgroup, one wave per SIMD (512 registers: no scratch).  Same bits (tools/lin1_harness.hip -DLIN1_NW=4); 3 840 tokens 24.0 -> 19.9 us,
// 7 680 34.4 -> 30.4, 15 360 50.4 -> 53.0 (so: up to 10 240); slower at every size for K <= 384 and at every large launch
// (profiles/r06_experiments.txt section 6).
int linear1_ts_waves(int D, int N) {
    static const int nw4_max = tune_int("LSL_LIN1_NW4_MAX", 10240);
    return D == 512 && N <= nw4_max ? 4 : 8;
}
bool linear1_ts_ok(int hdp, int D, int F1, int HHD, int N) {
    static const int on = tune_int("LSL_LIN1_TS", 1);
    if (!on || F1 % 64 != 0 || HHD % 64 != 0 || N < 1) return false;
    size_t lds = 0;  // of the 8-wave instance: weight ring + staging + bias vector
    return with_linear1_ts_instance(hdp, D, [&](auto h, auto k) { lds = Lin1Cfg<decltype(h)::value, decltype(k)::value, 8>::lds_bytes(F1); }) && lds <= LDS_BUDGET;
}
// LayerNorm + modulate inside linear1's activation load (k_lin1.hip.h, LNF instances): no LayerNorm launch, no bf16 `a` buffer - the kernel reads
// the fp32 residual stream.  Per HANDLE (lsl_model_set_ln_fuse; LSL_LN_FUSE=1 makes it the default of new handles, 0 disables it), never per
// batch: its rounding differs from the standalone kernel's.  Shapes: the token-stationary kernel's, with the (1 + scale | shift) rows of every
// trajectory a 256-token tile can touch in LDS (Lin1Cfg::LN_SLOTS) - one shared row, or tokens per trajectory >= half a tile (3 slots) / a tile (2).
int ln_fuse_env() {
    static const int v = env_int("LSL_LN_FUSE", -1);
    return v;
}
bool linear1_lnf_ok(int hdp, int D, int F1, int HHD, int N, int tpt, int mod_stride) {
    if (ln_fuse_env() == 0 || !linear1_ts_ok(hdp, D, F1, HHD, N)) return false;
    size_t lds = 0;
    int min_tpt = 0;
    with_linear1_ts_instance(hdp, D, [&](auto h, auto k) {
        using C = Lin1Cfg<decltype(h)::value, decltype(k)::value, 8>;
        lds = C::lds_bytes_lnf(F1);
        min_tpt = C::LN_SLOTS >= 3 ? C::TT / 2 : C::TT;
    });
    return (mod_stride == 0 || tpt >= min_tpt) && lds <= LDS_BUDGET;
}
void launch_linear1_ts(int hdp, int D, int waves, bool lnf, const Lin1Args &a, hipStream_t st) {  // (waves: linear1_ts_waves; lnf: 8 waves)
    with_linear1_ts_instance(hdp, D, [&](auto h, auto k) {
        constexpr int H = decltype(h)::value, K = decltype(k)::value;
        if (lnf) return launch_linear1_ts_t<H, K, 8, true>(a, st);
        if constexpr (K == 512) {
            if (waves == 4) return launch_linear1_ts_t<H, K, 4>(a, st);
        }
        launch_linear1_ts_t<H, K, 8>(a, st);
    });
}

// linear2 + gated residual update on the weight-stationary kernel (k_lin2.hip.h): F a multiple of 128, K2 one of the instantiated widths
// (K2 / 8 stationary registers per wave: 2 048, peptide, does not fit).  Same bits as the tile kernels (tools/lin2_harness.hip), so the
// choice may depend on the launch.  LSL_LIN2_WS=0 (read in the product too: the GPU suite compares the two paths bit for bit) turns it off.
// THE instance list (K2, chunks, ring slots).  (1280: 4 chunks of 160 columns - 40 of 64 lanes per LDS-DMA instruction instead of 32; round 5:
// 0.168-0.171 -> 0.165 ms at 163 840 tokens, 18.6 -> 17.1 us at 10 240)
#define LSL_LIN2_WS_INSTANCES(X) X(1536, 3, 3) X(1280, 4, 4) X(768, 3, 3) X(384, 3, 3)
template <class Fn>
bool with_linear2_ws_instance(int K2, Fn &&fn) {
#define X(K, NCH, NS) if (K2 == K) return fn(ic<K>{}, ic<NCH>{}, ic<NS>{}), true;
    LSL_LIN2_WS_INSTANCES(X)
#undef X
    return false;
}
bool linear2_ws_shape_ok(int D, int K2) {
    static const int on = env_int("LSL_LIN2_WS", 1);
    return on && D % 128 == 0 && D <= 512 && with_linear2_ws_instance(K2, [](auto, auto, auto) {});
}
// The grid of a k_linear2_ws launch: 8 x slices x rpx workgroups, at most one per CU, fewer token ranges than 32-token blocks; the LDS gate
// table holds the trajectories one token range can span.  The kernel takes the launch only if they fit (linear2_ws_max_gate_rows).
struct Lin2Grid {
    int slices, rpx, gate_rows;
};
Lin2Grid linear2_ws_grid(int F, int N, int tpt, bool shared) {
    const int slices = F / 128, cus = device_cus(), NBLK = (N + 31) / 32;
    int rpx = std::max(1, cus / (8 * slices));
    while (rpx > 1 && 8 * rpx > NBLK) --rpx;
    const int ranges = 8 * rpx, max_blocks = (NBLK + ranges - 1) / ranges + 1;
    return {slices, rpx, shared ? 1 : (max_blocks * 32 + tpt - 1) / tpt + 1};
}
int linear2_ws_max_gate_rows(int K2) {
    int rows = 0;
    with_linear2_ws_instance(K2, [&](auto k, auto nch, auto ns) { rows = Lin2Cfg<decltype(k)::value, decltype(nch)::value, decltype(ns)::value, true>::max_gate_rows; });
    return rows;
}
template <int K, int NCH, int NS, bool LNS>
void launch_linear2_ws_t(const Lin2Args &a, hipStream_t st) {  // (a.slices / rpx / gate_rows: linear2_ws_grid)
    using C = Lin2Cfg<K, NCH, NS, true>;
    auto kern = k_linear2_ws<K, NCH, NS, true, LNS>;
    LSL_ALLOW_LDS(kern, LDS_BUDGET);
    hipLaunchKernelGGL(kern, dim3(8 * a.slices * a.rpx), dim3(512), C::lds_bytes(a.gate_rows), st, a);
}
// LNS instances (a.stats): per-wave row statistics of the updated rows beside h (the next sub-block's LayerNorm runs inside linear1)
void launch_linear2_ws(int K2, const Lin2Args &a, hipStream_t st) {
    with_linear2_ws_instance(K2, [&](auto k, auto nch, auto ns) {
        constexpr int K = decltype(k)::value, NCH = decltype(nch)::value, NS = decltype(ns)::value;
        if (a.stats) launch_linear2_ws_t<K, NCH, NS, true>(a, st);
        else launch_linear2_ws_t<K, NCH, NS, false>(a, st);
    });
}

// The back half of a sub-block on the row-owning tail kernel (k_tail.hip.h): up-projection -> GELU in registers -> down-projection + attention
// out-projection + gated residual + the next sub-block's LayerNorm.  Instances: hidden 256 with heads * head_dim_pad = 256 (the output tile
// of a wave is hidden / 2 accumulator registers: 512 does not fit two waves per SIMD, and the one-wave-per-SIMD form measured slower than
// what it replaces - profiles/r06_tail_experiments.txt).  Chosen per HANDLE (lsl_model_set_tail; LSL_TAIL=1 makes it the default of new
// handles, LSL_TAIL=0 disables it - both read in the product: A/B runs and the GPU suite compare the two decompositions), never per batch.
int tail_env() {
    static const int v = env_int("LSL_TAIL", -1);
    return v;
}
bool tail_shape_ok(int D, int HHD, int M) {
    return tail_env() != 0 && D == 256 && HHD == 256 && M % 64 == 0 && M >= 64 && TailCfg<256, 256>::lds_bytes(M) <= LDS_BUDGET;  // (an even number of 32-feature mlp blocks: the kernel's pipeline has no parity branches)
}
size_t tail_stream_bytes(const lsl_model *m) { return TailCfg<256, 256>::stream_bytes(m->d.mlp_dim); }
void launch_tail(const TailArgs &a, hipStream_t st) {
    using C = TailCfg<256, 256>;
    auto kern = k_tail<256, 256>;
    LSL_ALLOW_LDS(kern, LDS_BUDGET);
    const int nwt = (a.N + 31) / 32;  // wave tiles of 32 tokens: every workgroup gets at least one
    hipLaunchKernelGGL(kern, dim3(std::min(nwt, device_cus())), dim3(512), C::lds_bytes(a.M), st, a);
}

// GEMM tiling (tuning knob LSL_GEMM; every variant sums k in the same order, so results are identical).
//   (features x tokens, waves, BK x ring stages):
//   5  256x256  8 waves 64x2, one tile per workgroup
//   6  256x256  8 waves 32x3, persistent workgroups + next-tile prefetch during the epilogue
//   10 128x128  4 waves 32x3 (used when F is not a multiple of 256: D = 128 / 384 models)
//   7  256x256  8 waves 64x2, persistent, piece-form epilogue (4 KiB staging per wave, next piece prefetched): linear2 default
//   8  256x256  8 waves 32x3, persistent, piece-form epilogue
//   11 128x128  4 waves 64x2
//   12 256x256  8 waves 64x2, persistent, two-phase epilogue staged in ring slot 1 (needs an even number of k-tiles)
//   13 256x128  4 waves 32x2, persistent, two workgroups per CU
//   15 256x256 16 waves 64x2 (64x64 per wave, 4 waves/SIMD: the light linear2 epilogue fits the 128-VGPR budget and the
//      extra occupancy hides load / store latency)
// 20-22: ping-pong halves (k_gemm_pp.hip.h).  Default (-1): 12 for linear1 (5 when K < 512 or not a multiple of 128, 6 when not a multiple of 64), 7 for linear2: the fastest pair measured on MI355X (profiles/r01_gemm_variants.txt lists
// every variant that was tried, including the ones no longer compiled in).
// Called by plan_pass only, once per GEMM (lin2: linear2's, else linear1's); launch_gemm takes the answer.
int gemm_variant(bool lin2, int F, int K, int N) {
    static const int forced_all = tune_int("LSL_GEMM", -1);
    static const int forced_1 = tune_int("LSL_GEMM1", -1), forced_2 = tune_int("LSL_GEMM2", -1);  // per GEMM: linear1 / linear2
    const int forced_one = lin2 ? forced_2 : forced_1;
    const int forced = forced_one >= 0 ? forced_one : forced_all;
    // 256-wide feature tiles waste MFMA work when F is not a multiple of 256 (D = 128 / 384 models): use 128 x 128 there
    const bool ragged = F % 256 != 0 && (F % 256 <= 128);
    const int ragged_variant = lin2 && K % 64 == 0 ? 11 : 10;  // measured on the D = 384 / 128 models
    if (forced >= 0) return forced;
    // linear2 of the 384-wide models (peptide: F = 384, K = 2 048, which no weight-stationary instance holds): the launch is bound by the
    // operand bytes each CU pulls through its L1 miss path (measured 49 GB/s per CU with two 128 x 128 workgroups per CU: the per-CU limit);
    // 192 x 128 tiles move 17 % fewer operand bytes per FLOP with as many workgroups as CUs, and a third ring slot covers the latency one
    // workgroup per CU leaves exposed: 63.5 -> 54.3 ms per 100 evaluations at 16 000 tokens (profiles/r05_experiments.txt).  Same bits as
    // every other tiling (same k order per element).  Only when the tiles fill at least half of the CUs.
    if (lin2 && F % 192 == 0 && F % 256 != 0 && K % 64 == 0 && (long)((N + 127) / 128) * (F / 192) * 2 >= (long)device_cus())
        return 28;
    if (ragged) return ragged_variant;
    // Small launches (one or two trajectories of the MD17 models, the reference's own B = 4 case): 256 x 256 tiles leave most of the chip
    // idle or run two rounds for 1.2 rounds of work; 128 x 128 tiles (two workgroups per CU) fill it.  Measured (profiles/
    // r02_experiments.txt): md17_bench B = 1 49.1 -> 38.0 ms per call, B = 2 63.0 -> 59.3, md17_ref B = 4 8.00 -> 7.65; from B = 4 of
    // md17_bench on the large tiles win again.  The tile shape does not change any output bit (every element is the same k-ascending
    // chain of 16-deep MFMA steps and the same epilogue arithmetic - checked by the batch-32-vs-batch-1 test at the headline shape),
    // so this may depend on the launch size.
    static const int small_rule = tune_int("LSL_SMALL_TILES", 1);
    const long tiles256 = (long)((N + 255) / 256) * ((F + 255) / 256);
    const int cus = device_cus();
    if (small_rule && K % 64 == 0 && tiles256 * (lin2 ? 2 : 4) <= (long)cus * (lin2 ? 1 : 5))
        return 11;  // linear2: tiles <= CUs / 2; linear1: tiles <= 1.25 CUs
    return lin2 ? (K % 128 == 0 ? 7 : 15) : (K % 128 == 0 ? 12 : 5);
}

// (variant: the plan's, gemm_variant.  The shape conditions below only keep a tiling FORCED in the experiments build inside what its kernel
// covers - gemm_variant itself never answers 12 or 7 outside them - and send it to tiling 5 otherwise.)
template <class Epi>
void launch_gemm(int variant, const u16 *W, const u16 *X, int F, int N, int K, const Epi &epi_in, hipStream_t st, int hhd = 32) {
    constexpr bool lin2 = std::is_same<Epi, EpiLinear2>::value;
    static const int probe = tune_int("LSL_PROBE", 0);
    static const int stagger = tune_int("LSL_STAGGER", 0);
    GemmArgs g{W, X, F, N, K, stagger, probe};
    // LSL_NT bit 0: linear1 output, bit 1: linear2 residual update, bit 2: attention output, bit 3: LayerNorm+modulate output
    static const int nt = tune_int("LSL_NT", 3);
    Epi epi = epi_in;
    epi.probe = probe | ((nt >> (lin2 ? 1 : 0)) & 1 ? 32 : 0);
    const bool pp_ok = lin2 || hhd % 32 == 0;  // linear1 sections start on 32-feature tiles
    if (launch_gemm_experiment(variant, g, epi, st, pp_ok)) return;  // (rejected structures: -DLSL_EXPERIMENTS builds only)
    if (variant == 12 && K % 128 == 0) return launch_gemm_glds<256, 256, 2, 4, 64, 2, true>(g, epi, st);  // 5 made persistent (staging in ring slot 1)
    if constexpr (lsl_experiments || lin2) {  // (linear1's piece epilogue exists in the experiments build only)
        if (variant == 7 && F % 32 == 0 && pp_ok && K % 128 == 0) return launch_gemm_glds<256, 256, 2, 4, 64, 2, true>(g, EpiPieces<Epi>(epi), st);  // persistent, 64-deep k-tiles, piece epilogue
    }
    switch (variant) {
        case 5: return launch_gemm_glds<256, 256, 2, 4, 64, 2, false>(g, epi, st);
        case 10: return launch_gemm_glds<128, 128, 2, 2, 32, 3, false>(g, epi, st);
        case 11: return launch_gemm_glds<128, 128, 2, 2, 64, 2, false>(g, epi, st);
        case 28:  // 192 features x 128 tokens, 8 waves of 96 x 32, three 64-deep ring slots (linear2 of the 384-wide models)
            if constexpr (lin2) return launch_gemm_glds<192, 128, 2, 4, 64, 3, false>(g, epi, st);
            else break;
        case 15: return launch_gemm_glds<256, 256, 4, 4, 64, 2, false>(g, epi, st);
        default: return launch_gemm_glds<256, 256, 2, 4, 64, 2, false>(g, epi, st);  // (K is a multiple of 64: hidden sizes are)
    }
}

// ---- attention: the form of an axis (plan_attention, called by plan_pass), then one launcher per form ---------------------------------

// persistent, double-buffered form (k_attention_stream): axes of more than 128 positions (unit = (sequence, head, group of 256 queries), keys in
// chunks of 256: peptide's T = 1000 is 4 groups x 4 chunks) and of 9 .. 32 positions
// with a multiple of 8 heads (8 heads of a sequence per unit).  The choice depends on the model and on T, L only - never on the batch - so a
// trajectory's bits are the same in any batch.  LSL_ATTN_STREAM=0 (read in the product too: A/B runs) keeps k_attention_rows.
int attention_stream_mode(int S, int H) {  // 0: k_attention_rows / tiny, 1: stream SHORT, 2: stream LONG
    static const int on = env_int("LSL_ATTN_STREAM", 1);
    if (!on) return 0;
    static const int long_min = tune_int("LSL_ATTN_LONG_MIN", 129);  // shortest axis on the LONG form
    if (S >= long_min) return 2;  // (round 5: any length - keys in chunks of 256 through the two images, queries in groups of 8 tiles)
    if (S > 8 && S <= 32 && H % 8 == 0) return 1;
    return 0;
}

enum class AttnForm {
    linear,           // k_attention_linear
    stream_short,     // k_attention_stream: 9 .. 32 positions, 8 heads of a sequence per unit
    stream_grouped,   // ... tiny spatial axes, 32 / S sequences to a 32-row tile (geometry rewritten below)
    stream_long,      // ... up to 256 positions: one key chunk
    stream_chunked,   // ... longer: keys in chunks of 256, queries in groups of 8 tiles
    stream_chunked_den,  // ... with the padded head's spare V column carrying the softmax denominator (peptide: head_dim 24 of 32)
    tiny,             // k_attention_tiny: one lane per (query, head)
    rows,             // k_attention_rows<nw, items, nkt>: two-pass softmax, K / V of `items` (sequence, head)s in LDS
    none              // not on the stream kernel and too long for k_attention_rows: plan_pass refuses the pass
};
// What the attention of one axis runs: the form, the sequence geometry the kernel is given (AttnArgs) and the instance of rows
struct AttnPlan {
    AttnForm form;
    int stream_mode;  // what attention_stream_mode said for this axis (2: q / k / v may travel as planes, qkv_planes_ok)
    int S, n_seq, inner, outer_stride, pos_stride, blk, n_tok;
    int nw, items, nkt;
    bool stream() const { return form >= AttnForm::stream_short && form <= AttnForm::stream_chunked_den; }
};
// tiny SPATIAL axes (L = 2, 4, 8: positions and sequences are consecutive tokens) on the SHORT stream kernel, 32 / L sequences to a tile with
// the scores outside the block diagonal masked (AttnArgs::blk): replaces k_attention_tiny.  LSL_ATTN_GROUP=0 keeps the lane-per-query kernel.
bool attention_grouped_ok(const AttnPlan &a, int H) {
    static const int on = env_int("LSL_ATTN_GROUP", 1), stream_on = env_int("LSL_ATTN_STREAM", 1);
    return on && stream_on && a.S >= 2 && a.S <= 8 && (a.S & (a.S - 1)) == 0 && a.inner == 1 && a.pos_stride == 1 && a.outer_stride == a.S && H % 8 == 0;
}
// LDS of the forms: stream - two images of K | V, 256 rows each, and a 32-row query image per wave; rows - K, V of every item (key tiles of
// 32 rows) and the key-norm slots
constexpr size_t attention_stream_lds(int hdp) { return (size_t)2 * 2 * 256 * hdp * 2 + (size_t)8 * 32 * hdp * 2; }
constexpr size_t attention_rows_lds(int hdp, int nw, int items, int key_rows) { return (size_t)items * 2 * key_rows * hdp * 2 + nw * sizeof(float); }
// the longest axis k_attention_rows takes: K | V of one (sequence, head) in whole key tiles, 16 waves' key-norm slots
constexpr int attention_rows_max_s(int hdp) { return (int)((LDS_BUDGET - 16 * sizeof(float)) / (4 * hdp)) & ~31; }
static_assert(attention_rows_lds(32, 16, 1, attention_rows_max_s(32)) <= LDS_BUDGET && attention_rows_lds(32, 16, 1, attention_rows_max_s(32) + 32) > LDS_BUDGET);

AttnPlan plan_attention(bool linear, int hdp, int H, int hd, int bc, int T, int L, bool temporal) {
    AttnPlan p{};
    if (!temporal) {  // sequences (b,t), positions l
        p.S = L; p.n_seq = bc * T; p.inner = 1; p.outer_stride = L; p.pos_stride = 1;
    } else {          // sequences (b,l), positions t
        p.S = T; p.n_seq = bc * L; p.inner = L; p.outer_stride = T * L; p.pos_stride = L;
    }
    p.form = AttnForm::linear;
    if (linear) return p;
    const AttnPlan axis = p;
    const bool grouped = attention_grouped_ok(p, H);
    if (grouped) {  // present the tokens as sequences of 32 rows
        p.blk = p.S;
        p.n_tok = p.n_seq * p.S;
        p.n_seq = (p.n_tok + 31) / 32;
        p.S = 32;
        p.outer_stride = 32;
    }
    p.stream_mode = attention_stream_mode(p.S, H);
    const bool is_long = p.stream_mode == 2;
    const long n_units = is_long ? (long)p.n_seq * H * (((p.S + 31) / 32 + 7) / 8) : (long)p.n_seq * (H / 8);  // LONG: (sequence, head, group of 8 query tiles)
    if (p.stream_mode && n_units + 2L * device_cus() < (1L << 31)) {  // (the kernel counts units in 32 bits: more go to the forms below)
        p.form = !is_long ? (grouped ? AttnForm::stream_grouped : AttnForm::stream_short)
                 : p.S <= 256 ? AttnForm::stream_long
                 : hdp == 32 && hd == 24 ? AttnForm::stream_chunked_den : AttnForm::stream_chunked;
        return p;
    }
    const int mode = p.stream_mode;
    p = axis;  // (not on the stream kernel: the axis as it is)
    p.stream_mode = mode;
    const int Sp = (p.S + 31) & ~31;
    auto inst = [&](AttnForm f, int nw, int items, int nkt) { p.form = f; p.nw = nw; p.items = items; p.nkt = nkt; return p; };
    if (p.S <= 8) return inst(AttnForm::tiny, 4, 1, 0);  // one lane per (query, head), no MFMA padding
    if (Sp <= attention_rows_max_s(hdp)) {  // two-pass softmax, K/V of one (sequence, head) in LDS
        // long axes (peptide T = 1000): 16 waves - with the max pass gone (AttnArgs::bound) the kernel is a chain of MFMA -> exp2 -> MFMA per
        // tile, and four waves per SIMD hide it better than two (attention 320.6 -> 303.8 ms per 1000-step call; with the max pass
        // 8 waves were as fast, profiles/r02_experiments.txt)
        static const int nw16 = tune_int("LSL_ATTN_NW16", 1);
        if (Sp > 256) return inst(AttnForm::rows, nw16 ? 16 : 8, 1, 0);
        if (Sp <= 32) return inst(AttnForm::rows, 4, 4, 1);
        if (Sp <= 64) return inst(AttnForm::rows, 4, 2, 2);
        if (Sp <= 128) return inst(AttnForm::rows, 4, 1, 4);
        return inst(AttnForm::rows, 4, 1, Sp <= 192 ? 6 : 8);
    }
    return inst(AttnForm::none, 0, 0, 0);  // (reachable with LSL_ATTN_STREAM=0, or 2^31 stream units: plan_pass refuses)
}
// q / k / v as head-major planes (k_lin1.hip.h, Lin1Args::planes): spatial sub-blocks (positions = consecutive tokens) whose attention
// runs the LONG stream kernel, token-stationary linear1.  LSL_QKV_PLANES=0 keeps token-major rows (A/B runs).
bool qkv_planes_ok(int hdp, int heads, int S, bool temporal, bool lin1_ts, const AttnPlan &attn) {
    static const int on = env_int("LSL_QKV_PLANES", 1);
    return on && !temporal && lin1_ts && heads % (64 / hdp) == 0 && S <= 256 && attn.form != AttnForm::linear && attn.stream_mode == 2;
}

template <auto KERN>
void launch_attention_stream(bool is_long, size_t lds, AttnArgs a, hipStream_t st) {
    LSL_ALLOW_LDS(KERN, lds);
    const long n_units = is_long ? (long)a.n_seq * a.H * (((a.S + 31) / 32 + 7) / 8) : (long)a.n_seq * (a.H / 8);  // (< 2^31 - 2 CUs: plan_attention)
    const int grid = (int)std::min<long>(2L * device_cus(), n_units);  // two workgroups per CU (2 x 80 KiB of LDS at 32-wide heads)
    a.nt = 0;  // plain stores: behind streaming stores the in-order vector-memory queue reports the next unit's requests late (measured: 0.78 vs 0.27 ms)
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(512), lds, st, a);
}
template <int HDP, int NW, int ITEMS, int NKT>
void launch_attention_rows(const AttnArgs &a, hipStream_t st) {
    auto kern = k_attention_rows<HDP, NW, ITEMS, NKT>;
    const size_t lds = attention_rows_lds(HDP, NW, ITEMS, NKT > 0 ? NKT * 32 : (a.S + 31) & ~31);
    LSL_ALLOW_LDS(kern, NKT > 0 ? lds : LDS_BUDGET);
    const long items = (long)a.n_seq * a.H;
    hipLaunchKernelGGL(kern, dim3((unsigned)((items + ITEMS - 1) / ITEMS)), dim3(NW * 64), lds, st, a);
}

// (a: the plan's geometry already in it - run_block)
template <int HDP>
void launch_attention_t(const AttnPlan &p, const AttnArgs &a, hipStream_t st) {
    constexpr size_t slds = attention_stream_lds(HDP);
    switch (p.form) {
        case AttnForm::linear:
            hipLaunchKernelGGL((k_attention_linear<HDP>), dim3((unsigned)std::min<long>((long)a.n_seq * a.H, 8L * device_cus())), dim3(256), 0, st, a);
            return;
        case AttnForm::stream_short: return launch_attention_stream<k_attention_stream<HDP, false>>(false, slds, a, st);
        case AttnForm::stream_grouped: return launch_attention_stream<k_attention_stream<HDP, false, false, false, true>>(false, slds, a, st);
        case AttnForm::stream_long: return launch_attention_stream<k_attention_stream<HDP, true>>(true, slds, a, st);
        case AttnForm::stream_chunked: return launch_attention_stream<k_attention_stream<HDP, true, true>>(true, slds, a, st);
        case AttnForm::stream_chunked_den:
            if constexpr (HDP == 32) return launch_attention_stream<k_attention_stream<HDP, true, true, true>>(true, slds, a, st);
            else return;  // (plan_attention: 32-wide heads only)
        case AttnForm::tiny:
            hipLaunchKernelGGL((k_attention_tiny<HDP>), dim3((unsigned)(((long)a.n_seq * a.S * a.H + 255) / 256)), dim3(256), 0, st, a);
            return;
        case AttnForm::rows:
            switch (p.nw * 100 + p.items * 10 + p.nkt) {
                case 1610: return launch_attention_rows<HDP, 16, 1, 0>(a, st);
                case 810: return launch_attention_rows<HDP, 8, 1, 0>(a, st);
                case 441: return launch_attention_rows<HDP, 4, 4, 1>(a, st);
                case 422: return launch_attention_rows<HDP, 4, 2, 2>(a, st);
                case 414: return launch_attention_rows<HDP, 4, 1, 4>(a, st);
                case 416: return launch_attention_rows<HDP, 4, 1, 6>(a, st);
                default: return launch_attention_rows<HDP, 4, 1, 8>(a, st);
            }
        case AttnForm::none: return;  // (plan_pass has refused the pass)
    }
}

template <bool PRE, bool POST>
void launch_dense(float *out, const float *in, const float *W, const float *bias, const float *add, int rows, int I, int O,
                  int add_stride, hipStream_t st, bool single = false, int add_mod = 0, char *name = nullptr) {
    // (name: 32 bytes or NULL - receives the kernel the branch taken below launches, for the label of profile class 6)
    auto named = [&](const char *kernel, int kq) {
        if (name && kq) snprintf(name, 32, "%s<%d, %d, %d>", kernel, (int)PRE, (int)POST, kq);
        else if (name) snprintf(name, 32, "%s<%d, %d>", kernel, (int)PRE, (int)POST);
    };
    // The choice must not depend on the BATCH: the two kernels sum k in different orders, and a trajectory's result has to be the
    // same bits whatever batch it is sampled in (K-sample batching, sharding, pass size).  `single` marks the calls that have one
    // row by construction (the sampler's shared time without class conditioning: one conditioning vector for any batch); they
    // take the wave-per-output kernel (a coalesced GEMV, 8x faster at one row than the 64-row tile kernel).
    if (single && rows == 1 && I <= 512) {
        named("k_dense_rows", 0);
        hipLaunchKernelGGL((k_dense_rows<PRE, POST>), dim3((O + 3) / 4), dim3(256), 0, st, out, in, W, bias, add, rows, I, O, add_stride, add_mod);
    } else if ((I == 128 || I == 256) && tune_int("LSL_DENSE_MFMA", 1)) {  // usual widths, any row count: the fp32 matrix pipe (k_dense_mfma) - the
                                                                            // general path's class-conditioned batches and the short chains in front of k_resident
        const dim3 grid((O + 31) / 32, (rows + 31) / 32);
        named("k_dense_mfma", I / 4);
        if (I == 128) hipLaunchKernelGGL((k_dense_mfma<PRE, POST, 32>), grid, dim3(256), 0, st, out, in, W, bias, add, rows, I, O, add_stride, add_mod);
        else hipLaunchKernelGGL((k_dense_mfma<PRE, POST, 64>), grid, dim3(256), 0, st, out, in, W, bias, add, rows, I, O, add_stride, add_mod);
    } else if (I % 4 == 0) {
        named("k_dense_tiled", 0);
        hipLaunchKernelGGL((k_dense_tiled<PRE, POST>), dim3((O + 63) / 64, (rows + 63) / 64), dim3(256), 0, st, out, in, W, bias, add, rows,
                           I, O, add_stride, add_mod);
    } else {
        named("k_dense_rows", 0);
        hipLaunchKernelGGL((k_dense_rows<PRE, POST>), dim3((O + 3) / 4), dim3(256), 0, st, out, in, W, bias, add, rows, I, O, add_stride, add_mod);
    }
}

}  // namespace
