// Sliding-window evaluation (build-defined: the reference evaluates the whole image in one forward).  Overlapping crops
// of the training size are cut from the image, the model's logits of each crop are upsampled, activated, weighted and
// summed into a full-resolution accumulator, and the accumulator is normalised by the summed weights:
//   window_gather      image -> a batch of crops (zero padding outside the image, optional horizontal mirror),
//   window_accumulate  the model's logits of one batch of crops -> acc += weight * activation(upsampled logits),
//                      wsum += weight,
//   window_merge       out (+)= scale_weight * bilinear(acc / wsum) at the image's own size.
// A window table is int32 [n][4] rows (b, y0, x0, flags): flags bit 0 = mirrored, bit 1 = null (padding of the last
// batch).  The accumulate kernel is a GATHER over accumulator pixels: a thread owns one pixel and all its channels, walks
// the windows in table order and adds the covering ones in that order, so there are no atomics, no address has two
// writers, and the sum at a pixel does not depend on how the window list is cut into calls (the running sum lives in
// fp32 memory between calls exactly as it lives in the fp32 register between windows of one call).
// Memory-bound: lanes run along x, so every channel of the NCHW accumulator is one coalesced row segment per wave; the
// window rows, the vertical window test and the vertical interpolation taps are uniform across a workgroup (one
// accumulator row of one image per workgroup).  Every fp32 operation is rounded as written (-ffp-contract=off).
#include "common.h"

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_MAX_WINDOWS = 64;
constexpr int SW_MAX_C = 64;
constexpr int SW_MIRROR = 1, SW_NULL = 2;

// the coordinate rule of ssseg_bilinear_fwd for align_corners=False (interp.hip src_index): source taps i0, i1 and
// their weights l0, l1 for output index d
struct Axis {
  int in, out;
  float scale;
};

static Axis make_axis(int64_t in, int64_t out) {
  Axis a;
  a.in = (int)in;
  a.out = (int)out;
  a.scale = (float)in / (float)out;
  return a;
}

__device__ __forceinline__ void src_index(const Axis& a, int d, int& i0, int& i1, float& l0, float& l1) {
  float src = __fsub_rn(__fmul_rn(a.scale, __fadd_rn((float)d, 0.5f)), 0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, a.in - 1);
  l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
  i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
  l0 = __fsub_rn(1.f, l1);
}

__device__ __forceinline__ float lerp2(float x00, float x01, float x10, float x11, float lw0, float lw1, float lh0,
                                       float lh1) {
  const float t0 = __fadd_rn(__fmul_rn(x00, lw0), __fmul_rn(x01, lw1));
  const float t1 = __fadd_rn(__fmul_rn(x10, lw0), __fmul_rn(x11, lw1));
  return __fadd_rn(__fmul_rn(t0, lh0), __fmul_rn(t1, lh1));
}

// ---- gather --------------------------------------------------------------------------------------------------------
// grid (x: blocks of crop pixels, y: window).  T is the raw element (4 or 2 bytes): values are moved, not converted.
template <typename T>
__global__ void __launch_bounds__(SW_THREADS) window_gather_kernel(const T* __restrict__ img, Strides4 is, int B,
                                                                   int Cimg, int Hs, int Ws,
                                                                   const int* __restrict__ win, int ch, int cw,
                                                                   T* __restrict__ out, Strides4 os) {
  const int j = blockIdx.y;
  const int p = blockIdx.x * SW_THREADS + threadIdx.x;
  if (p >= ch * cw) return;
  const int ly = p / cw, lx = p - ly * cw;
  const int wb = win[4 * j], flags = win[4 * j + 3];
  const int64_t sy = (int64_t)win[4 * j + 1] + ly;
  const int64_t sx = (int64_t)win[4 * j + 2] + ((flags & SW_MIRROR) ? cw - 1 - lx : lx);
  const bool inside = !(flags & SW_NULL) && wb >= 0 && wb < B && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
  const T* ip = img + (inside ? (int64_t)wb * is.n + sy * is.h + sx * is.w : 0);
  T* op = out + (int64_t)j * os.n + (int64_t)ly * os.h + (int64_t)lx * os.w;
  for (int c = 0; c < Cimg; ++c) op[(int64_t)c * os.c] = inside ? ip[(int64_t)c * is.c] : (T)0;
}

// ---- accumulate ----------------------------------------------------------------------------------------------------
// grid (x: blocks of accumulator columns, y: accumulator row, z: image).  CMAX is the channel bucket (2 .. 64, with
// 24 between 16 and 32): the pixel's running sums and the window's activated values are register arrays, the loops
// fully unrolled.  The accumulator is read at the first covering window and written once at the end; a pixel that no
// window of this call covers is not touched.  IDENT: the logits are at the crop's own resolution (taps (1, 0): the
// values themselves).
template <int CMAX, bool IDENT>
__global__ void __launch_bounds__(SW_THREADS) window_accumulate_kernel(const float* __restrict__ logits, Strides4 ls,
                                                                       Axis ah, Axis aw, const int* __restrict__ win,
                                                                       int n, int C, int ch, int cw, int activation,
                                                                       int weighting, float* __restrict__ acc,
                                                                       float* __restrict__ wsum, int Ha, int Wa) {
  const int x = blockIdx.x * SW_THREADS + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= Wa) return;
  const int64_t plane = (int64_t)Ha * Wa;
  float* ap = acc + (int64_t)b * C * plane + (int64_t)y * Wa + x;
  float* wp = wsum + (int64_t)b * plane + (int64_t)y * Wa + x;
  float a[CMAX];
  float wtot = 0.f;
  bool loaded = false;
  const float cy = 0.5f * (float)(ch - 1), cx = 0.5f * (float)(cw - 1);
  const float sgy = 0.125f * (float)ch, sgx = 0.125f * (float)cw;
  const float ky = 2.f * sgy * sgy, kx = 2.f * sgx * sgx;
  for (int j = 0; j < n; ++j) {
    // the row and the two tests on it are the same for every thread of the workgroup
    const int wb = win[4 * j], flags = win[4 * j + 3];
    if ((flags & SW_NULL) || wb != b) continue;
    const int64_t ly64 = (int64_t)y - win[4 * j + 1];
    if (ly64 < 0 || ly64 >= ch) continue;
    const int64_t lx64 = (int64_t)x - win[4 * j + 2];
    if (lx64 < 0 || lx64 >= cw) continue;
    const int ly = (int)ly64;
    const int lx = (flags & SW_MIRROR) ? cw - 1 - (int)lx64 : (int)lx64;   // the crop's column of this pixel
    if (!loaded) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c) a[c] = ap[(int64_t)(c < C ? c : 0) * plane];
      wtot = *wp;
      loaded = true;
    }
    float v[CMAX];
    const float* lp = logits + (int64_t)j * ls.n;
    if (IDENT) {
      const float* q = lp + (int64_t)ly * ls.h + (int64_t)lx * ls.w;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) v[c] = q[(int64_t)(c < C ? c : 0) * ls.c];
    } else {
      int h0, h1, w0, w1;
      float lh0, lh1, lw0, lw1;
      src_index(ah, ly, h0, h1, lh0, lh1);
      src_index(aw, lx, w0, w1, lw0, lw1);
      const int64_t o00 = h0 * ls.h + w0 * ls.w, o01 = h0 * ls.h + w1 * ls.w;
      const int64_t o10 = h1 * ls.h + w0 * ls.w, o11 = h1 * ls.h + w1 * ls.w;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        const float* q = lp + (int64_t)(c < C ? c : 0) * ls.c;
        v[c] = lerp2(q[o00], q[o01], q[o10], q[o11], lw0, lw1, lh0, lh1);
      }
    }
    if (activation == 2) {
      // prob_onehot_mc_kernel's softmax: the maximum subtracted, expf, one reciprocal
      float mx = -INFINITY, z = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) mx = fmaxf(mx, v[c]);
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        v[c] = c < C ? expf(v[c] - mx) : 0.f;
        z += v[c];
      }
      const float r = 1.f / z;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) v[c] *= r;
    } else if (activation == 1) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c) v[c] = 1.f / (1.f + expf(-v[c]));
    }
    float wgt = 1.f;
    if (weighting == 1) {
      const float dy = (float)ly - cy, dx = (float)lx - cx;
      wgt = expf(-(dy * dy / ky + dx * dx / kx));
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) a[c] += v[c] * wgt;
    wtot += wgt;
  }
  if (loaded) {
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) ap[(int64_t)c * plane] = a[c];
    *wp = wtot;
  }
}

// ---- merge ---------------------------------------------------------------------------------------------------------
// grid (x: blocks of output columns, y: output row, z: image).  Each tap is divided by its own weight sum before the
// interpolation; at the accumulator's own size the value is acc / wsum * scale_weight and nothing else.
__global__ void __launch_bounds__(SW_THREADS) window_merge_kernel(const float* __restrict__ acc,
                                                                  const float* __restrict__ wsum, int C, int Ha, int Wa,
                                                                  Axis ah, Axis aw, float scale_weight, int first,
                                                                  float* __restrict__ out) {
  const int x = blockIdx.x * SW_THREADS + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  const int H = ah.out, W = aw.out;
  if (x >= W) return;
  const int64_t plane = (int64_t)Ha * Wa, oplane = (int64_t)H * W;
  const float* ab = acc + (int64_t)b * C * plane;
  const float* wb = wsum + (int64_t)b * plane;
  float* ob = out + (int64_t)b * C * oplane + (int64_t)y * W + x;
  if (ah.in == H && aw.in == W) {
    const int64_t o = (int64_t)y * Wa + x;
    const float ws = wb[o];
    for (int c = 0; c < C; ++c) {
      const float v = ab[(int64_t)c * plane + o] / ws * scale_weight;
      ob[(int64_t)c * oplane] = first ? v : ob[(int64_t)c * oplane] + v;
    }
    return;
  }
  int h0, h1, w0, w1;
  float lh0, lh1, lw0, lw1;
  src_index(ah, y, h0, h1, lh0, lh1);
  src_index(aw, x, w0, w1, lw0, lw1);
  const int64_t o00 = (int64_t)h0 * Wa + w0, o01 = (int64_t)h0 * Wa + w1;
  const int64_t o10 = (int64_t)h1 * Wa + w0, o11 = (int64_t)h1 * Wa + w1;
  const float s00 = wb[o00], s01 = wb[o01], s10 = wb[o10], s11 = wb[o11];
  for (int c = 0; c < C; ++c) {
    const float* q = ab + (int64_t)c * plane;
    const float v = lerp2(q[o00] / s00, q[o01] / s01, q[o10] / s10, q[o11] / s11, lw0, lw1, lh0, lh1) * scale_weight;
    ob[(int64_t)c * oplane] = first ? v : ob[(int64_t)c * oplane] + v;
  }
}

// ---- labels --------------------------------------------------------------------------------------------------------
// torch.argmax over the channels of a contiguous [B,C,HW] map: the first maximum wins, NaN counts as the maximum.
// grid (x: pixel blocks, y: image), grid-strided over the pixels.
__global__ void __launch_bounds__(SW_THREADS) window_argmax_kernel(const float* __restrict__ x, int C, int64_t HW,
                                                                   int64_t* __restrict__ labels) {
  const float* xb = x + (int64_t)blockIdx.y * C * HW;
  int64_t* lb = labels + (int64_t)blockIdx.y * HW;
  for (int64_t p = (int64_t)blockIdx.x * SW_THREADS + threadIdx.x; p < HW; p += (int64_t)gridDim.x * SW_THREADS) {
    float best = xb[p];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = xb[(int64_t)c * HW + p];
      const bool take = v > best || (v != v && best == best);
      best = take ? v : best;
      arg = take ? c : arg;
    }
    lb[p] = arg;
  }
}

template <int CMAX>
void launch_accumulate(dim3 grid, hipStream_t st, bool ident, const float* logits, Strides4 ls, Axis ah, Axis aw,
                       const int* win, int n, int C, int ch, int cw, int activation, int weighting, float* acc,
                       float* wsum, int Ha, int Wa) {
  if (ident)
    hipLaunchKernelGGL((window_accumulate_kernel<CMAX, true>), grid, dim3(SW_THREADS), 0, st, logits, ls, ah, aw, win, n,
                       C, ch, cw, activation, weighting, acc, wsum, Ha, Wa);
  else
    hipLaunchKernelGGL((window_accumulate_kernel<CMAX, false>), grid, dim3(SW_THREADS), 0, st, logits, ls, ah, aw, win,
                       n, C, ch, cw, activation, weighting, acc, wsum, Ha, Wa);
}

// image-sized frames: each extent and the pixel count inside int32, rows and images inside the grid's y / z range
bool frame_ok(int64_t B, int64_t H, int64_t W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && H <= 65535 && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int ssseg_window_gather(const void* image, const int64_t* image_strides4, int64_t B, int64_t Cimg,
                                   int64_t Hs, int64_t Ws, const int32_t* windows, int64_t n, void* crops,
                                   const int64_t* crop_strides4, int64_t ch, int64_t cw, int dt,
                                   ssseg_stream_t stream) {
  if (!image || !image_strides4 || !windows || !crops || !crop_strides4) return SSSEG_EINVAL;
  if (!frame_ok(B, Hs, Ws) || !frame_ok(1, ch, cw) || Cimg < 1 || Cimg > SW_MAX_C || n < 1 || n > 65535)
    return SSSEG_EINVAL;
  if (dt != SSSEG_F32 && dt != SSSEG_BF16 && dt != SSSEG_F16) return SSSEG_EINVAL;
  const Strides4 is = strides4(image_strides4), os = strides4(crop_strides4);
  const dim3 grid((unsigned)((ch * cw + SW_THREADS - 1) / SW_THREADS), (unsigned)n);
  hipStream_t st = (hipStream_t)stream;
  if (dt == SSSEG_F32)
    hipLaunchKernelGGL(window_gather_kernel<float>, grid, dim3(SW_THREADS), 0, st, (const float*)image, is, (int)B,
                       (int)Cimg, (int)Hs, (int)Ws, (const int*)windows, (int)ch, (int)cw, (float*)crops, os);
  else
    hipLaunchKernelGGL(window_gather_kernel<unsigned short>, grid, dim3(SW_THREADS), 0, st,
                       (const unsigned short*)image, is, (int)B, (int)Cimg, (int)Hs, (int)Ws, (const int*)windows,
                       (int)ch, (int)cw, (unsigned short*)crops, os);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_window_accumulate(const float* logits, const int64_t* logit_strides4, int64_t n, int64_t C,
                                       int64_t h, int64_t w, const int32_t* windows, const int32_t* windows_host,
                                       int64_t ch, int64_t cw, int activation, int weighting, float* acc, float* wsum,
                                       int64_t B, int64_t Ha, int64_t Wa, ssseg_stream_t stream) {
  if (!logits || !logit_strides4 || !windows || !windows_host || !acc || !wsum) return SSSEG_EINVAL;
  if (n < 1 || n > SW_MAX_WINDOWS || C < 1 || C > SW_MAX_C) return SSSEG_EINVAL;
  if (!frame_ok(B, Ha, Wa) || !frame_ok(1, ch, cw) || !frame_ok(1, h, w)) return SSSEG_EINVAL;
  if (activation < 0 || activation > 2 || (weighting != 0 && weighting != 1)) return SSSEG_EINVAL;
  for (int64_t j = 0; j < n; ++j) {
    const int32_t* r = windows_host + 4 * j;
    if (r[3] & SW_NULL) continue;
    if (r[0] < 0 || r[0] >= B || r[1] < 0 || r[1] + ch > Ha || r[2] < 0 || r[2] + cw > Wa) return SSSEG_EINVAL;
  }
  const Strides4 ls = strides4(logit_strides4);
  const Axis ah = make_axis(h, ch), aw = make_axis(w, cw);
  const dim3 grid((unsigned)((Wa + SW_THREADS - 1) / SW_THREADS), (unsigned)Ha, (unsigned)B);
  const bool ident = h == ch && w == cw;
#define SW_ACC(N)                                                                                                   \
  launch_accumulate<N>(grid, (hipStream_t)stream, ident, logits, ls, ah, aw, (const int*)windows, (int)n, (int)C,  \
                       (int)ch, (int)cw, activation, weighting, acc, wsum, (int)Ha, (int)Wa)
  if (C <= 2) SW_ACC(2);
  else if (C <= 4) SW_ACC(4);
  else if (C <= 8) SW_ACC(8);
  else if (C <= 16) SW_ACC(16);
  else if (C <= 24) SW_ACC(24);   // the 19 and 21 classes of the usual sets: a third fewer registers than 32
  else if (C <= 32) SW_ACC(32);
  else SW_ACC(64);
#undef SW_ACC
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_window_merge(const float* acc, const float* wsum, int64_t B, int64_t C, int64_t Ha, int64_t Wa,
                                  int64_t Hs, int64_t Ws, float* out, int64_t H, int64_t W, float scale_weight,
                                  int first, ssseg_stream_t stream) {
  if (!acc || !wsum || !out || C < 1 || C > SW_MAX_C) return SSSEG_EINVAL;
  if (!frame_ok(B, Ha, Wa) || !frame_ok(B, H, W) || Hs < 1 || Ws < 1 || Hs > Ha || Ws > Wa) return SSSEG_EINVAL;
  const Axis ah = make_axis(Hs, H), aw = make_axis(Ws, W);
  const dim3 grid((unsigned)((W + SW_THREADS - 1) / SW_THREADS), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL(window_merge_kernel, grid, dim3(SW_THREADS), 0, (hipStream_t)stream, acc, wsum, (int)C, (int)Ha,
                     (int)Wa, ah, aw, scale_weight, first, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_window_argmax(const float* x, int64_t B, int64_t C, int64_t HW, int64_t* labels,
                                   ssseg_stream_t stream) {
  if (!x || !labels || B < 1 || B > 65535 || C < 1 || C > SW_MAX_C || HW < 1) return SSSEG_EINVAL;
  const dim3 grid((unsigned)ssseg_grid(HW, SW_THREADS), (unsigned)B);
  hipLaunchKernelGGL(window_argmax_kernel, grid, dim3(SW_THREADS), 0, (hipStream_t)stream, x, (int)C, HW, labels);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
