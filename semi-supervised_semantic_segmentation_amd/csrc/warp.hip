// Per-sample affine warp (rotate + zoom about the image centre) for the geometric consistency branch, gfx950:
// reversible_augmentations.RotateRescale (the reference's plan, train.py:16-17: "sample aug params, do forward, warp
// preds back, calc consistency loss").
//
// Convention: one 2x3 matrix per sample, fp32 in device memory, [a, b, tx, c, d, ty], mapping an OUTPUT pixel (x, y)
// to input coordinates sx = a x + b y + tx, sy = c x + d y + ty; pixel centres on integers, bilinear taps, zeros
// outside.  The coordinates are evaluated as fmaf(a, x, fmaf(b, y, tx)) everywhere (forward, validity, backward), so
// the identity matrix gives the integers back and the kernel copies its input bit for bit.
//
// Forward: one thread per (sample, pixel) -- and per channel lane when the tensor is channels-last -- computes the
// coordinates and the four weights once and loops over its channels.  Backward: the exact adjoint as a gather -- each
// INPUT pixel p walks the output pixels of a bounding box around mats_inv p, recomputes their coordinates with the
// forward's expression and sums, in row-major order, the gradients of those that tapped p: no atomics, no memset, the
// same bits on every run and under graph replay.  The matrices live in device memory, so a captured step replays
// whatever ssseg_affine_draw_dev drew last.
#include "common.h"
#include "philox.h"

namespace {

struct Taps {
  int x0, y0;
  float wx, wy;
  bool inside;   // some tap may lie in the image
  bool valid;    // the sampling point itself lies in the image: 0 <= sx <= W-1, 0 <= sy <= H-1
};

__device__ __forceinline__ Taps affine_taps(const float* __restrict__ m, int x, int y, int H, int W) {
  const float xf = (float)x, yf = (float)y;
  const float sx = fmaf(m[0], xf, fmaf(m[1], yf, m[2]));
  const float sy = fmaf(m[3], xf, fmaf(m[4], yf, m[5]));
  Taps t;
  t.valid = sx >= 0.f && sx <= (float)(W - 1) && sy >= 0.f && sy <= (float)(H - 1);
  t.inside = sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H;   // false for NaN: nothing is converted
  const float fx = floorf(sx), fy = floorf(sy);
  t.x0 = t.inside ? (int)fx : 0;
  t.y0 = t.inside ? (int)fy : 0;
  t.wx = sx - fx;
  t.wy = sy - fy;
  return t;
}

// CL channel lanes per pixel (1 for NCHW: consecutive lanes on consecutive x; up to 64 for channels-last: consecutive
// lanes on consecutive channels); I: index type of the decode (int while the thread count fits)
template <typename T, typename I>
__global__ void __launch_bounds__(256) affine_warp_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                              const float* __restrict__ mats, int64_t total_, int C,
                                                              int H, int W, int CL, Strides4 xs, Strides4 ys,
                                                              float* __restrict__ valid) {
  const I total = (I)total_;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const int cl = (int)(i % CL);
    const I pix = i / CL;
    const int px = (int)(pix % W), py = (int)((pix / W) % H);
    const int64_t n = (int64_t)(pix / ((I)W * H));
    const Taps t = affine_taps(mats + 6 * n, px, py, H, W);
    if (valid && cl == 0) valid[pix] = t.valid ? 1.f : 0.f;
    const bool x0in = (unsigned)t.x0 < (unsigned)W, x1in = (unsigned)(t.x0 + 1) < (unsigned)W;
    const bool y0in = (unsigned)t.y0 < (unsigned)H, y1in = (unsigned)(t.y0 + 1) < (unsigned)H;
    const bool i00 = t.inside && x0in && y0in, i01 = t.inside && x1in && y0in;
    const bool i10 = t.inside && x0in && y1in, i11 = t.inside && x1in && y1in;
    const float w00 = (1.f - t.wx) * (1.f - t.wy), w01 = t.wx * (1.f - t.wy);
    const float w10 = (1.f - t.wx) * t.wy, w11 = t.wx * t.wy;
    const bool exact = t.wx == 0.f && t.wy == 0.f;   // on a pixel centre: the value itself (signed zeros included)
    // clamped offsets: every load is issued (in bounds), the out-of-image taps are dropped by the selects
    const int cx0 = min(max(t.x0, 0), W - 1), cx1 = min(max(t.x0 + 1, 0), W - 1);
    const int cy0 = min(max(t.y0, 0), H - 1), cy1 = min(max(t.y0 + 1, 0), H - 1);
    const int64_t o00 = cy0 * xs.h + cx0 * xs.w, o01 = cy0 * xs.h + cx1 * xs.w;
    const int64_t o10 = cy1 * xs.h + cx0 * xs.w, o11 = cy1 * xs.h + cx1 * xs.w;
    const T* xb = x + n * xs.n;
    T* yb = y + n * ys.n + (int64_t)py * ys.h + (int64_t)px * ys.w;
    for (int c = cl; c < C; c += CL) {
      const T* xc = xb + (int64_t)c * xs.c;
      const float v00 = io<T>::ld(xc, o00), v01 = io<T>::ld(xc, o01);
      const float v10 = io<T>::ld(xc, o10), v11 = io<T>::ld(xc, o11);
      float v = 0.f;
      if (i00) v = fmaf(w00, v00, v);
      if (i01) v = fmaf(w01, v01, v);
      if (i10) v = fmaf(w10, v10, v);
      if (i11) v = fmaf(w11, v11, v);
      if (exact) v = i00 ? v00 : 0.f;
      io<T>::st(yb, (int64_t)c * ys.c, v);
    }
  }
}

// adjoint gather; each thread owns one input pixel and up to 4 channels per pass (cl, cl + CL, cl + 2 CL, cl + 3 CL)
template <typename T, typename I>
__global__ void __launch_bounds__(256) affine_warp_bwd_kernel(const T* __restrict__ gy, T* __restrict__ gx,
                                                              const float* __restrict__ mats,
                                                              const float* __restrict__ mats_inv, int64_t total_,
                                                              int C, int H, int W, int CL, Strides4 gys, Strides4 gxs) {
  const I total = (I)total_;
  for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const int cl = (int)(i % CL);
    const I pix = i / CL;
    const int px = (int)(pix % W), py = (int)((pix / W) % H);
    const int64_t n = (int64_t)(pix / ((I)W * H));
    const float* m = mats + 6 * n;
    const float* mi = mats_inv + 6 * n;
    // outputs q that tap p have |A q - p| < 1 per axis, so q - A^-1 p = L^-1 (A q - p) lies within (|ia| + |ib|,
    // |ic| + |id|); one more pixel covers the rounding of the centre.  Clamped in float: a NaN leaves the whole image.
    const float qx = fmaf(mi[0], (float)px, fmaf(mi[1], (float)py, mi[2]));
    const float qy = fmaf(mi[3], (float)px, fmaf(mi[4], (float)py, mi[5]));
    const float ex = fabsf(mi[0]) + fabsf(mi[1]) + 1.f, ey = fabsf(mi[3]) + fabsf(mi[4]) + 1.f;
    const int xlo = (int)fminf(fmaxf(ceilf(qx - ex), 0.f), (float)W), xhi = (int)fmaxf(fminf(floorf(qx + ex), (float)(W - 1)), -1.f);
    const int ylo = (int)fminf(fmaxf(ceilf(qy - ey), 0.f), (float)H), yhi = (int)fmaxf(fminf(floorf(qy + ey), (float)(H - 1)), -1.f);
    const T* gb = gy + n * gys.n;
    T* gxb = gx + n * gxs.n + (int64_t)py * gxs.h + (int64_t)px * gxs.w;
    for (int c0 = cl; c0 < C; c0 += 4 * CL) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int oy = ylo; oy <= yhi; ++oy) {
        for (int ox = xlo; ox <= xhi; ++ox) {
          const Taps t = affine_taps(m, ox, oy, H, W);
          const int dx = px - t.x0, dy = py - t.y0;
          if (!t.inside || (unsigned)dx > 1u || (unsigned)dy > 1u) continue;
          // the forward's weight of tap (dx, dy), the same product
          const float wgt = (dx ? t.wx : 1.f - t.wx) * (dy ? t.wy : 1.f - t.wy);
          if (wgt == 0.f) continue;
          const T* gq = gb + (int64_t)oy * gys.h + (int64_t)ox * gys.w;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * CL;
            if (c < C) acc[j] = fmaf(wgt, io<T>::ld(gq, (int64_t)c * gys.c), acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + j * CL;
        if (c < C) io<T>::st(gxb, (int64_t)c * gxs.c, acc[j]);
      }
    }
  }
}

// A(theta, s) and its inverse A(-theta, 1/s), built in fp64 and rounded once
__device__ __forceinline__ void affine_store(float* m, double al, double be, double cx, double cy) {
  m[0] = (float)al;
  m[1] = (float)be;
  m[2] = (float)(cx - al * cx - be * cy);
  m[3] = (float)(-be);
  m[4] = (float)al;
  m[5] = (float)(cy + be * cx - al * cy);
}

// One block: theta_b = max (2 u - 1), s_b = lo + u' (hi - lo) from Philox-4x32-10 at counter offset + b, stream 2 of
// the key (CowMix's noise is stream 0, its p / sigma draws stream 1); every thread reads the counter before thread 0
// advances it by B.
__global__ void __launch_bounds__(256) affine_draw_kernel(float* mats, float* mats_inv, int B, int H, int W,
                                                          float max_angle, float lo, float hi, uint64_t seed,
                                                          unsigned long long* offset_dev) {
  const uint64_t offset = (uint64_t)*offset_dev;
  const double cx = 0.5 * (double)(W - 1), cy = 0.5 * (double)(H - 1);
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    unsigned c[4];
    philox_block(c, offset + (uint64_t)b, 2u);
    philox4x32_10(c, seed);
    const float u1 = philox_u01(c[0]), u2 = philox_u01(c[1]);
    const float theta = max_angle * (2.f * u1 - 1.f);
    const float s = fminf(fmaxf(lo + u2 * (hi - lo), lo), hi);
    const double th = (double)theta * (3.14159265358979323846 / 180.0);
    const double cs = cos(th), sn = sin(th), sd = (double)s;
    affine_store(mats + 6 * b, cs / sd, -sn / sd, cx, cy);
    affine_store(mats_inv + 6 * b, cs * sd, sn * sd, cx, cy);
  }
  __syncthreads();
  if (threadIdx.x == 0) *offset_dev = (unsigned long long)(offset + (uint64_t)B);
}

// channel lanes per pixel: the channels of a channels-last tensor are its fastest axis
int channel_lanes(int64_t C, const Strides4& a, const Strides4& b) {
  if (C < 2 || a.c != 1 || b.c != 1) return 1;
  int cl = 1;
  while (cl < C && cl < 64) cl *= 2;
  return cl;
}

bool warp_args_ok(const void* a, const void* b, const float* m, int64_t N, int64_t C, int64_t H, int64_t W,
                  const int64_t* sa, const int64_t* sb) {
  return a && b && m && sa && sb && N >= 0 && C >= 0 && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) &&
         C <= 0x7fffffff;
}

}  // namespace

extern "C" int ssseg_affine_warp_fwd(const void* x, void* y, const float* mats, int64_t N, int64_t C, int64_t H,
                                     int64_t W, const int64_t* x_strides4_host, const int64_t* y_strides4_host,
                                     int dt, float* valid_out, ssseg_stream_t stream) {
  if (!warp_args_ok(x, y, mats, N, C, H, W, x_strides4_host, y_strides4_host)) return SSSEG_EINVAL;
  if (dt != SSSEG_F32 && dt != SSSEG_BF16 && dt != SSSEG_F16) return SSSEG_EUNSUPPORTED;
  if (N == 0 || (C == 0 && !valid_out)) return 0;
  const Strides4 xs = strides4(x_strides4_host), ys = strides4(y_strides4_host);
  const int cl = channel_lanes(C, xs, ys);
  const int64_t total = N * H * W * cl;
  const bool i32 = total < 0x7fffffffLL - (1LL << 24);   // i + grid stride stays in int range
  const dim3 g(ssseg_grid(total, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
#define WARP_FWD(T)                                                                                                    \
  if (i32)                                                                                                             \
    hipLaunchKernelGGL((affine_warp_fwd_kernel<T, int>), g, b, 0, s, (const T*)x, (T*)y, mats, total, (int)C, (int)H,  \
                       (int)W, cl, xs, ys, valid_out);                                                                 \
  else                                                                                                                 \
    hipLaunchKernelGGL((affine_warp_fwd_kernel<T, int64_t>), g, b, 0, s, (const T*)x, (T*)y, mats, total, (int)C,      \
                       (int)H, (int)W, cl, xs, ys, valid_out);
  if (dt == SSSEG_F32) {
    WARP_FWD(float)
  } else if (dt == SSSEG_BF16) {
    WARP_FWD(bf16_t)
  } else {
    WARP_FWD(f16_t)
  }
#undef WARP_FWD
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_affine_warp_bwd(const void* gy, void* gx, const float* mats, const float* mats_inv, int64_t N,
                                     int64_t C, int64_t H, int64_t W, const int64_t* gy_strides4_host,
                                     const int64_t* gx_strides4_host, int dt, ssseg_stream_t stream) {
  if (!warp_args_ok(gy, gx, mats, N, C, H, W, gy_strides4_host, gx_strides4_host) || !mats_inv) return SSSEG_EINVAL;
  if (dt != SSSEG_F32 && dt != SSSEG_BF16 && dt != SSSEG_F16) return SSSEG_EUNSUPPORTED;
  if (N == 0 || C == 0) return 0;
  const Strides4 gys = strides4(gy_strides4_host), gxs = strides4(gx_strides4_host);
  const int cl = channel_lanes((C + 3) / 4, gys, gxs);
  const int64_t total = N * H * W * cl;
  const bool i32 = total < 0x7fffffffLL - (1LL << 24);
  const dim3 g(ssseg_grid(total, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
#define WARP_BWD(T)                                                                                                    \
  if (i32)                                                                                                             \
    hipLaunchKernelGGL((affine_warp_bwd_kernel<T, int>), g, b, 0, s, (const T*)gy, (T*)gx, mats, mats_inv, total,      \
                       (int)C, (int)H, (int)W, cl, gys, gxs);                                                          \
  else                                                                                                                 \
    hipLaunchKernelGGL((affine_warp_bwd_kernel<T, int64_t>), g, b, 0, s, (const T*)gy, (T*)gx, mats, mats_inv, total,  \
                       (int)C, (int)H, (int)W, cl, gys, gxs);
  if (dt == SSSEG_F32) {
    WARP_BWD(float)
  } else if (dt == SSSEG_BF16) {
    WARP_BWD(bf16_t)
  } else {
    WARP_BWD(f16_t)
  }
#undef WARP_BWD
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_affine_draw_dev(float* mats, float* mats_inv, int64_t B, int64_t H, int64_t W,
                                     double max_angle_deg, double scale_lo, double scale_hi, uint64_t seed,
                                     unsigned long long* offset_dev, ssseg_stream_t stream) {
  if (!mats || !mats_inv || !offset_dev || B < 1 || B > 0x7fffffff || H < 1 || W < 1 || !(max_angle_deg >= 0) ||
      !(scale_lo > 0) || !(scale_hi >= scale_lo))
    return SSSEG_EINVAL;
  hipLaunchKernelGGL(affine_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mats, mats_inv, (int)B, (int)H,
                     (int)W, (float)max_angle_deg, (float)scale_lo, (float)scale_hi, seed, offset_dev);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
