// Per-device one-time kernel attributes: the dynamic-LDS allowance of a kernel (LSL_ALLOW_LDS at its launch site).  The attribute is set
// through the kernel's symbol, so every translation unit that launches a kernel with more than 64 KiB of dynamic LDS includes this and
// sets the attribute itself: the state (one flag per call site) is the unit's own.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace {

template <typename K>
void allow_lds(K kernel, size_t bytes) {
    hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// The dynamic-LDS attribute is a property of (kernel, device): one flag per device ordinal and per call site.
struct DevOnce {
    std::atomic<unsigned long long> bits{0};
    bool first() {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (bits.load(std::memory_order_relaxed) & bit) return false;
        bits.fetch_or(bit, std::memory_order_relaxed);
        return true;
    }
};

}  // namespace

#define LSL_ALLOW_LDS(kern, bytes)                  \
    do {                                            \
        static DevOnce once_;                       \
        if (once_.first()) allow_lds(kern, bytes);  \
    } while (0)
