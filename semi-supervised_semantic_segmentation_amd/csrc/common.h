// Shared device helpers for the ssseg HIP kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "../../include/ssseg.h"

#define SSSEG_WAVE 64

// Launch-error check: every extern "C" entry returns 0 or a hipError_t / SSSEG_E* code.
#define SSSEG_LAUNCH_CHECK()                                   \
  do {                                                         \
    hipError_t _e = hipGetLastError();                         \
    if (_e != hipSuccess) return (int)_e;                      \
  } while (0)

#define SSSEG_TRY(expr)                                        \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) return (int)_e;                      \
  } while (0)

typedef unsigned short bf16_t;   // raw bfloat16 bits

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(((unsigned)v) << 16);
}

// round-to-nearest-even f32 -> bf16 (NaN kept a NaN)
// round-to-nearest-even f32 -> bf16 in hardware (gfx950 v_cvt_pk_bf16_f32; NaN stays a quiet NaN): one
// instruction instead of the bit-twiddled rounding (~6 VALU) the epilogues and BN passes spent per value
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  return __builtin_bit_cast(bf16_t, (__bf16)f);
}

// IEEE half (the fp16 compute mode, config C5): hardware round-to-nearest-even conversions
typedef _Float16 f16_t;
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its global stores.
// __syncthreads() (release fence) also drains vmcnt, i.e. every store the wave issued before it: in an epilogue
// that stores its tile and then reduces statistics through LDS that is ~2 us of HBM write latency per tile,
// serialised (+60 % on the conv 1x1 expansions' fused-statistics launches).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <typename T> struct io;
template <> struct io<float> {
  __device__ __forceinline__ static float ld(const float* p, int64_t i) { return p[i]; }
  __device__ __forceinline__ static void st(float* p, int64_t i, float v) { p[i] = v; }
};
template <> struct io<bf16_t> {
  __device__ __forceinline__ static float ld(const bf16_t* p, int64_t i) { return bf16_to_f32(p[i]); }
  __device__ __forceinline__ static void st(bf16_t* p, int64_t i, float v) { p[i] = f32_to_bf16(v); }
};
template <> struct io<f16_t> {
  __device__ __forceinline__ static float ld(const f16_t* p, int64_t i) { return (float)p[i]; }
  __device__ __forceinline__ static void st(f16_t* p, int64_t i, float v) { p[i] = (f16_t)v; }
};

// two fp32 values rounded to one dword of bf16 (low half first); pairwise, so that the compiler picks the packed
// conversion (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned bf16x2_bits(float a, float b) {
  return (unsigned)f32_to_bf16(a) | ((unsigned)f32_to_bf16(b) << 16);
}

// Raw V-element chunks (16 or 8 bytes): ld() moves the bits only, cvt() converts to fp32 later and pack() is its
// inverse, in registers (for the sites that shuffle or stage the packed bits before they store them).  Streaming
// kernels issue every load of a batch first (clamped addresses, no branch around a load) and convert after,
// so the batch is in flight together: a conversion right behind each conditional load makes the compiler
// wait for that load (s_waitcnt vmcnt(0)) before issuing the next, serialising the memory round trips.
// These, Vec below, philox.h and Strides4 are the only copies of their kind: a kernel file defines none of its own.
template <typename T, int V> struct Chunk;
template <> struct Chunk<bf16_t, 8> {
  typedef uint4 raw;
  __device__ __forceinline__ static raw ld(const bf16_t* p) { return *(const uint4*)p; }
  __device__ __forceinline__ static raw zero() { return make_uint4(0, 0, 0, 0); }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[8]) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  __device__ __forceinline__ static raw pack(const float (&v)[8]) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = bf16x2_bits(v[2 * i], v[2 * i + 1]);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct Chunk<bf16_t, 4> {
  typedef uint2 raw;
  __device__ __forceinline__ static raw ld(const bf16_t* p) { return *(const uint2*)p; }
  __device__ __forceinline__ static raw zero() { return make_uint2(0, 0); }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[4]) {
    v[0] = __uint_as_float(q.x << 16); v[1] = __uint_as_float(q.x & 0xffff0000u);
    v[2] = __uint_as_float(q.y << 16); v[3] = __uint_as_float(q.y & 0xffff0000u);
  }
  __device__ __forceinline__ static raw pack(const float (&v)[4]) {
    const unsigned a = bf16x2_bits(v[0], v[1]), b = bf16x2_bits(v[2], v[3]);
    return make_uint2(a, b);
  }
};
template <> struct Chunk<f16_t, 8> {
  typedef uint4 raw;
  __device__ __forceinline__ static raw ld(const f16_t* p) { return *(const uint4*)p; }
  __device__ __forceinline__ static raw zero() { return make_uint4(0, 0, 0, 0); }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[8]) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f16x2_t h = __builtin_bit_cast(f16x2_t, w[i]);
      v[2 * i] = (float)h[0];
      v[2 * i + 1] = (float)h[1];
    }
  }
  __device__ __forceinline__ static raw pack(const float (&v)[8]) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f16x2_t h = {(f16_t)v[2 * i], (f16_t)v[2 * i + 1]};
      w[i] = __builtin_bit_cast(unsigned, h);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct Chunk<f16_t, 4> {
  typedef uint2 raw;
  __device__ __forceinline__ static raw ld(const f16_t* p) { return *(const uint2*)p; }
  __device__ __forceinline__ static raw zero() { return make_uint2(0, 0); }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[4]) {
    const f16x2_t a = __builtin_bit_cast(f16x2_t, q.x), b = __builtin_bit_cast(f16x2_t, q.y);
    v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)b[0]; v[3] = (float)b[1];
  }
  __device__ __forceinline__ static raw pack(const float (&v)[4]) {
    const f16x2_t a = {(f16_t)v[0], (f16_t)v[1]}, b = {(f16_t)v[2], (f16_t)v[3]};
    return make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
  }
};
template <> struct Chunk<float, 4> {
  typedef float4 raw;
  __device__ __forceinline__ static raw ld(const float* p) { return *(const float4*)p; }
  __device__ __forceinline__ static raw zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[4]) {
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
  __device__ __forceinline__ static raw pack(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Chunk<float, 2> {
  typedef float2 raw;
  __device__ __forceinline__ static raw ld(const float* p) { return *(const float2*)p; }
  __device__ __forceinline__ static raw zero() { return make_float2(0.f, 0.f); }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[2]) {
    v[0] = q.x; v[1] = q.y;
  }
  __device__ __forceinline__ static raw pack(const float (&v)[2]) { return make_float2(v[0], v[1]); }
};
template <> struct Chunk<float, 1> {   // the scalar member, for kernels templated on the vector width
  typedef float raw;
  __device__ __forceinline__ static raw ld(const float* p) { return *p; }
  __device__ __forceinline__ static raw zero() { return 0.f; }
  __device__ __forceinline__ static void cvt(const raw& q, float (&v)[1]) { v[0] = q; }
  __device__ __forceinline__ static raw pack(const float (&v)[1]) { return v[0]; }
};

// N consecutive elements at p (aligned to the chunk) as fp32 values: one load and convert, or pack and one store
template <typename T, int N> struct Vec {
  static constexpr int V = N;
  using CK = Chunk<T, N>;
  __device__ __forceinline__ static void ld(const T* p, float (&v)[N]) { CK::cvt(CK::ld(p), v); }
  __device__ __forceinline__ static void st(T* p, const float (&v)[N]) { *(typename CK::raw*)p = CK::pack(v); }
};
template <> struct Vec<float, 8> {   // two 16-byte accesses
  static constexpr int V = 8;
  __device__ __forceinline__ static void ld(const float* p, float (&v)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  __device__ __forceinline__ static void st(float* p, const float (&v)[8]) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
};
template <typename T> using Vec16 = Vec<T, 16 / sizeof(T)>;   // the 16-byte chunk of T: 8 x bf16 / fp16, 4 x fp32

// element strides of a 4-D tensor, as the entries receive them
struct Strides4 {
  int64_t n, c, h, w;
};
static inline Strides4 strides4(const int64_t* s) { return Strides4{s[0], s[1], s[2], s[3]}; }

// wave64 reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sum; `scratch` needs blockDim.x/64 entries; result valid in every thread
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  T t = 0;
  for (int i = 0; i < nw; ++i) t += scratch[i];
  return t;
}

// grid-stride launch size: one thread per element up to `cap` workgroups (SSSEG_GRID_CAP overrides the default
// cap for sweeps)
static inline int ssseg_grid_cap() {
  static const int cap = [] {
    const char* e = getenv("SSSEG_GRID_CAP");
    const int v = e ? atoi(e) : 256 * 16;
    return v > 0 ? v : 256 * 16;
  }();
  return cap;
}
static inline int ssseg_grid(int64_t n, int block, int cap = -1) {
  if (cap < 0) cap = ssseg_grid_cap();
  int64_t g = (n + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// activation codes (SSSEG_ACT_*): forward, and the derivative evaluated from the output y (sign and the
// open interval (0, 6) survive every activation here, so y decides like the pre-activation does) or from
// the pre-activation z.  PyTorch semantics: ReLU6 = hardtanh(0, 6) passes gradient for 0 < z < 6;
// LeakyReLU passes 1 for z > 0 and slope otherwise.
__device__ __forceinline__ float act_fwd(float z, int act, float slope) {
  if (act == SSSEG_ACT_RELU) return fmaxf(z, 0.f);
  if (act == SSSEG_ACT_RELU6) return fminf(fmaxf(z, 0.f), 6.f);
  if (act == SSSEG_ACT_LEAKY) return z > 0.f ? z : z * slope;
  return z;
}
// g * d act / d z with the gradient SELECTED (not multiplied) where it is cut, like threshold_backward
__device__ __forceinline__ float act_bwd(float g, float yz, int act, float slope) {
  if (act == SSSEG_ACT_RELU) return yz > 0.f ? g : 0.f;
  if (act == SSSEG_ACT_RELU6) return (yz > 0.f && yz < 6.f) ? g : 0.f;
  if (act == SSSEG_ACT_LEAKY) return yz > 0.f ? g : g * slope;
  return g;
}
