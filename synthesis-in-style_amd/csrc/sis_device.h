// Device primitives shared by every kernel file of libsis_hip.so (gfx950 only): vector types, wave / workgroup sums,
// LDS-DMA, and 4 / 8 consecutive elements as floats.  Device-only; everything is sis_-prefixed and in the global namespace.
// A helper lives here only where its copies generated the same code: the order in which a sum adds its terms is part of the
// numerical contract of the kernels that call it (bit-exactness tests pin it), so it is stated at each sum and must not change.
#pragma once
#include "sis_common.h"

// ---- vector types.  Compiler vectors, not HIP's float4 / float2 structs: those are union classes whose ARRAYS end up in
// scratch (staging registers, MFMA accumulators), and a struct type aliases everything for the wait-count pass.
typedef __attribute__((ext_vector_type(2))) float sis_f32x2;
typedef __attribute__((ext_vector_type(4))) float sis_f32x4;
typedef __attribute__((ext_vector_type(16))) float sis_f32x16;
typedef __attribute__((ext_vector_type(2))) __bf16 sis_bf16x2;
typedef __attribute__((ext_vector_type(4))) __bf16 sis_bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 sis_bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned sis_u32x4;
typedef __attribute__((ext_vector_type(2))) long long sis_i64x2;
typedef unsigned short sis_u16;                                   // a bf16 / f16 element as raw bits
typedef __attribute__((address_space(3))) void sis_lds_void;      // LDS destination of the LDS-DMA builtins

// ---- the float32 source-index rule of bilinear interpolation with align_corners=True (PyTorch's upsample_bilinear2d):
// src = dst * (in - 1) / (out - 1), i0 = (int) src, i1 = i0 + (i0 < in - 1), lambda1 = src - i0, lambda0 = 1 - lambda1.  ONE
// definition for every kernel that interpolates (seg_ops.hip, upsample_ops.hip).
// The product is rounded to float BEFORE i0 is taken from it and subtracted from it (no contraction in here): as
// fma(scale, dst, -i0) the lambda comes from the unrounded product while i0 comes from the rounded one, so where the rounded
// product lands on an integer from below, l1 is a negative 1e-7 and cell i1 gets a share it has no part in (3 -> 7 at output 3:
// 3e-8 on a cell the rule gives weight exactly 0), and every other lambda differs from the float32 rule by up to half an ulp
// of src.
struct sis_lerp { int i0, i1; float l0, l1; };
__device__ __forceinline__ sis_lerp sis_lerp_index(int dst, float scale, int in_size) {
#pragma clang fp contract(off)
    const float src = scale * (float)dst;
    sis_lerp r;
    r.i0 = (int)src;
    if (r.i0 > in_size - 1) r.i0 = in_size - 1;
    r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// ---- sums.  All lanes / threads get the result.
// Sum over the 64 lanes of a wave: xor butterfly, partner distance 32, 16, 8, 4, 2, 1 in that order.
template <typename T>
__device__ __forceinline__ T sis_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over a workgroup of 256 threads (4 waves), float or double; red = 4 elements of LDS, reusable right after.
// ORDER (contract): each wave by the butterfly of sis_wave_sum, then (r0 + r1) + (r2 + r3) over the waves.
// (The butterfly is written out, not called: calling sis_wave_sum moved an instruction across the barrier in some kernels.)
template <typename T>
__device__ __forceinline__ T sis_block_sum4(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Sum over a workgroup of NW waves; red = NW elements of LDS.
// ORDER (contract): each wave by the butterfly, then 0 + r0 + r1 + ... in wave order, one after the other.
template <int NW>
__device__ __forceinline__ float sis_block_sum_waves(float v, float* red) {   // compile-time wave count
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ float sis_block_sum_waves(float v, float* red, int nw) {   // run-time wave count
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += red[w];
    return s;
}

// ---- LDS-DMA: global memory to LDS without passing through registers.  A wave instruction writes 64 x `size` consecutive
// bytes from the (wave-uniform) LDS address on; only the global side is per lane.
// Word 3 of a buffer resource descriptor for raw byte-addressed access: DATA_FORMAT = 32 bit (bits 15..18 = 4), every other
// field zero -- no swizzle, no structured index, stride 0, so the range check is (per-lane offset + access size <= num_records
// bytes) and a lane that fails it loads ZEROS.
constexpr int SIS_BUF_RSRC_FLAGS = 0x00020000;

// num_bytes: extent from `base` that lanes may read; the default (2 GiB - 1) leaves only offsets with bit 31 set out of range.
// Build it from wave-uniform values only.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sis_buffer_rsrc(const void* base, unsigned num_bytes = 0x7FFFFFFFu) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)num_bytes, SIS_BUF_RSRC_FLAGS);
}
// 16 bytes per lane from descriptor base + voff (per lane, VGPR) + soff (wave-uniform, SGPR) to l + 16 * lane
__device__ __forceinline__ void sis_buffer_load_lds16(__amdgpu_buffer_rsrc_t r, void* l, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (sis_lds_void*)l, 16, voff, soff, 0, 0);
}
// 16 / 4 bytes per lane from the lane's own global address g to l + 16 / 4 * lane
__device__ __forceinline__ void sis_global_load_lds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (sis_lds_void*)l, 16, 0, 0);
}
__device__ __forceinline__ void sis_global_load_lds4(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (sis_lds_void*)l, 4, 0, 0);
}

// ---- 4 / 8 consecutive elements (float, __half, __hip_bfloat16) as floats: one 16-byte load or store (two for 8 floats,
// 8 bytes for four 16-bit elements); p aligned to that.
template <typename T>
__device__ __forceinline__ void sis_load4(const T* p, float* v) {
    if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        T t[4];
        __builtin_memcpy(t, &q, 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = sis_ld(t, e);
    }
}
template <typename T>
__device__ __forceinline__ void sis_store4(T* p, const float* v) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        T t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) sis_st(t, e, v[e]);
        uint2 q;
        __builtin_memcpy(&q, t, 8);
        *reinterpret_cast<uint2*>(p) = q;
    }
}
template <typename T>
__device__ __forceinline__ void sis_load8(const T* p, float* v) {
    if constexpr (sizeof(T) == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        T t[8];
        __builtin_memcpy(t, &q, 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = sis_ld(t, e);
    }
}
template <typename T>
__device__ __forceinline__ void sis_store8(T* p, const float* v) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        T t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) sis_st(t, e, v[e]);
        uint4 q;
        __builtin_memcpy(&q, t, 16);
        *reinterpret_cast<uint4*>(p) = q;
    }
}
