// Shared host-side helpers for libsis_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/sis_hip.h"

extern thread_local char sis_err_buf[512];
extern thread_local const char* sis_kernel_name;  // device kernel the last call of an entry point that names its kernel dispatched to
                                                  // (the convolutions, norms, encoder, k-means, upsampling, EqualLinear, ToRGB: sis_last_kernel())

static inline int sis_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(sis_err_buf, sizeof(sis_err_buf), fmt, ap);
    va_end(ap);
    return 1;
}

// Launch-error check: no host sync, just the launch status.
// Development aid (SIS_OCC=1): what the runtime says fits on a CU for this launch -- a kernel's dynamic LDS size or register
// count can silently halve the workgroups per CU its design assumes (the transposed modconv ran one per CU for a round).
#define SIS_OCC_REPORT(kernel, threads, lds_bytes)                                                                      \
    do {                                                                                                                \
        static const bool occ_on_ = getenv("SIS_OCC") != nullptr;                                                       \
        if (occ_on_) {                                                                                                  \
            int nb_ = -1;                                                                                               \
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb_, kernel, (int)(threads), (size_t)(lds_bytes));      \
            fprintf(stderr, "[occ] %s: %d threads, %zu B LDS -> %d workgroups per CU\n", #kernel, (int)(threads), (size_t)(lds_bytes), nb_); \
        }                                                                                                               \
    } while (0)

#define SIS_CHECK_LAUNCH(name)                                                                   \
    do {                                                                                         \
        hipError_t e_ = hipGetLastError();                                                       \
        if (e_ != hipSuccess) return sis_fail("%s: launch failed: %s", name, hipGetErrorString(e_)); \
    } while (0)

#define SIS_REQUIRE(cond, ...)                     \
    do {                                           \
        if (!(cond)) return sis_fail(__VA_ARGS__); \
    } while (0)

static inline int sis_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Same-shape layers in one launch (the convolution weight gradients' *_multi entries: grid.z = layer, operands through pointer
// tables in the kernel parameters).
constexpr int SIS_JOBS_MAX = 16;   // layers per launch
template <class T> struct SisJobTab { T* dw[SIS_JOBS_MAX]; };   // the layers' dW pointers, passed to the reduction kernels by value

// Runs n_jobs layers in launches of at most SIS_JOBS_MAX: run(first, n), n halved while fits(n) says that the plan for n layers
// does not leave every layer its slabs in the workspace (a single layer is left to run's own check).  Stops at the first failure.
template <class Fits, class Run>
static inline int sis_run_jobs(int n_jobs, Fits fits, Run run) {
    for (int first = 0; first < n_jobs;) {
        int n = n_jobs - first < SIS_JOBS_MAX ? n_jobs - first : SIS_JOBS_MAX;
        while (n > 1 && !fits(n)) n = (n + 1) / 2;
        const int rc = run(first, n);
        if (rc) return rc;
        first += n;
    }
    return 0;
}

// Device-side scalar conversion helpers (compute type for f16/bf16 is float, as the
// reference kernels' scalar_t arithmetic on half promotes through float on the FMA path).
template <typename T> struct sis_acc { typedef T type; };
template <> struct sis_acc<__half> { typedef float type; };
template <> struct sis_acc<__hip_bfloat16> { typedef float type; };

template <typename T> __device__ __forceinline__ typename sis_acc<T>::type sis_ld(const T* p, int64_t i) { return p[i]; }
template <> __device__ __forceinline__ float sis_ld<__half>(const __half* p, int64_t i) { return __half2float(p[i]); }
template <> __device__ __forceinline__ float sis_ld<__hip_bfloat16>(const __hip_bfloat16* p, int64_t i) { return __bfloat162float(p[i]); }

template <typename T> __device__ __forceinline__ void sis_st(T* p, int64_t i, typename sis_acc<T>::type v) { p[i] = v; }
template <> __device__ __forceinline__ void sis_st<__half>(__half* p, int64_t i, float v) { p[i] = __float2half(v); }
template <> __device__ __forceinline__ void sis_st<__hip_bfloat16>(__hip_bfloat16* p, int64_t i, float v) { p[i] = __float2bfloat16(v); }
