// What the entry points of every translation unit share (lam_slide_amd/_lib.py UNITS): the error convention (fail, LSL_CHECK_LAUNCH,
// LSL_API_CATCH), align_up, the device guard, and the unit's line of lsl_build_info() (LSL_UNIT_INFO).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <new>

#ifndef LSL_UNIT_OPTIONS
#define LSL_UNIT_OPTIONS ""  // (the options this unit was compiled with: lam_slide_amd/_lib.py passes them)
#endif

// Defined once, in lsl_api.hip, and hidden: no unit's internals reach the dynamic symbol table, whatever the build's default visibility.
#define LSL_HIDDEN __attribute__((visibility("hidden")))

// The error of a refused call: the message goes to the calling thread's buffer (one in the library, beside lsl_last_error), `code` comes back.
LSL_HIDDEN int fail(int code, const char *fmt, ...);

// LSL_UNIT_INFO, once in every unit's .hip file: adds "<unit>: <options>" to what lsl_build_info() reports, when the library is loaded.
LSL_HIDDEN void lsl_add_unit_info(const char *line);
#define LSL_UNIT_INFO static const int lsl_unit_info_ = (lsl_add_unit_info(__FILE_NAME__ ": " LSL_UNIT_OPTIONS), 0)

#define LSL_CHECK_LAUNCH(name)                                                     \
    do {                                                                           \
        hipError_t e_ = hipGetLastError();                                         \
        if (e_ != hipSuccess) return fail(-10, "%s: %s", name, hipGetErrorString(e_)); \
    } while (0)

// Behind the function-try-block of every C entry point: no exception crosses the ABI
#define LSL_API_CATCH                                \
    catch (const std::bad_alloc &) {                 \
        return fail(-5, "out of host memory");       \
    } catch (...) {                                  \
        return fail(-11, "unexpected C++ exception"); \
    }

namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Calls may arrive with a current device other than the stream's (a model used on a second GPU of the process): launches,
// attributes and the CU count must follow the STREAM's device.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(hipStream_t st) {
        int cur = 0, want = 0;
        if (hipGetDevice(&cur) != hipSuccess) return;
        if (hipStreamGetDevice(st, &want) != hipSuccess) { (void)hipGetLastError(); return; }
        if (want != cur && hipSetDevice(want) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace
