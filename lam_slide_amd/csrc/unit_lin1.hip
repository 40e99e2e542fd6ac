// The translation unit of the token-stationary linear1 kernel (k_lin1.hip.h): every k_linear1_ts instance that host_launch.hip.h dispatches,
// and the launcher that starts them.  A unit of its own because the kernel fills the register file at hidden 512 and what hipcc makes of the
// code AROUND its steady loops (spilled registers, full vmcnt drains in front of their reloads) depends on compile options that cost other
// kernels time (profiles/lin1_unit.txt): lam_slide_amd/_lib.py UNITS names the options of this unit, lsl_build_info() reports them.
// No device call crosses the units (no -fgpu-rdc); the plan and the dispatch stay in lsl_api.hip.
#include <hip/hip_runtime.h>

#include "k_lin1.hip.h"

#include "host_api.hip.h"
#include "host_lds.hip.h"

LSL_UNIT_INFO;

namespace {

template <int HDP, int K, int NW, bool LNF>
void launch(const Lin1Args &a, int grid, size_t lds, hipStream_t st) {
    auto kern = k_linear1_ts<HDP, K, NW, LNF>;
    LSL_ALLOW_LDS(kern, (size_t)160 * 1024);  // (gfx950: the whole LDS of a CU; host_launch.hip.h gates on the same budget)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, st, a);
}

template <int HDP, int K>
bool launch4(const Lin1Args &a, int grid, size_t lds, hipStream_t st) {  // the 4-wave form exists at hidden 512 only
    if constexpr (K == 512) launch<HDP, K, 4, false>(a, grid, lds, st);
    return K == 512;
}

}  // namespace

bool lsl_lin1_launch(int hdp, int K, int waves, bool lnf, const Lin1Args &a, int grid, size_t lds, hipStream_t st) {
#define X(H, KK)                                                              \
    if (hdp == H && K == KK) {                                                \
        if (lnf) return launch<H, KK, 8, true>(a, grid, lds, st), true;       \
        if (waves == 4) return launch4<H, KK>(a, grid, lds, st);              \
        return launch<H, KK, 8, false>(a, grid, lds, st), true;               \
    }
    LSL_LIN1_TS_INSTANCES(X)
#undef X
    return false;
}
