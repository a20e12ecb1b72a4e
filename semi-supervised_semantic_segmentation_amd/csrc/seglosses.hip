// The remaining losses of the reference's losses.py on the device:
//   dense CE (losses.py:25-39), OHEM CE (:51-69), FocalLoss (:72-90), NormalizedFocalLossSigmoid (:93-151),
//   DiceWithLogitsLoss (:157-167), dice_loss / log_dice_loss (:221-236), binary_entropy_loss / entropy_loss
//   (:253-264), BCE reduction 'none' / 'sum' (:41-48), smooth_labels (:267-268).
// Conventions of eltwise.hip: contiguous fp32 [B,C,HW]; reductions are per-block fp64 partials + one final block
// in a caller-owned workspace (no floating-point atomics: bitwise reproducible); nothing allocates or synchronises;
// backward kernels recompute from (x, t) and read gout from device memory.
// Softmax-family kernels: one thread per pixel, the C <= 64 channel values of the pixel in registers (template on
// the next power of two), loads coalesced across pixels (channel stride HW).
#include "common.h"

namespace {

constexpr int RED_BLOCKS = 1024;
constexpr int RED_THREADS = 256;
constexpr int HDR = 16;          // doubles at the start of every workspace (scalars kept for the backward)
constexpr int PLANE_CHUNKS = 64; // blocks per sample / per plane in the per-sample and per-plane reductions

__device__ __forceinline__ float sigmoidf_ref(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float bce_elem(float v, float tt) {
  return fmaxf(v, 0.f) - v * tt + log1pf(expf(-fabsf(v)));
}
// torch.pow(b, g) and its autograd derivative g * pow(b, g - 1); exponent 2 is b * b in torch
__device__ __forceinline__ float powg(float b, float g) { return g == 2.f ? b * b : powf(b, g); }
__device__ __forceinline__ float dpowg(float b, float g) { return g == 2.f ? 2.f * b : g * powf(b, g - 1.f); }

// softmax of one pixel in registers: d[c] = x_c - max, e[c] = exp(d[c]), s = sum e; channels >= C hold e = 0
template <int CM>
struct Soft {
  float d[CM], e[CM], s;
  __device__ __forceinline__ void load(const float* xp, int C, int64_t HW) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      d[c] = c < C ? xp[c * HW] : -INFINITY;
      m = fmaxf(m, d[c]);
    }
    s = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      d[c] -= m;
      e[c] = c < C ? expf(d[c]) : 0.f;
      s += e[c];
    }
  }
};

template <int CM>
__device__ __forceinline__ void load_t(const float* tp, int C, int64_t HW, float (&t)[CM]) {
#pragma unroll
  for (int c = 0; c < CM; ++c) t[c] = c < C ? tp[c * HW] : 0.f;
}

// out[0] = (float)(sum(part) * mul)
__global__ void __launch_bounds__(RED_THREADS) sum_final_kernel(const double* part, int nparts, double mul,
                                                                float* out) {
  __shared__ double red[RED_THREADS / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) acc += part[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = (float)(acc * mul);
}

// ---- dense CE ----
template <int CM>
__global__ void __launch_bounds__(RED_THREADS) ce_fwd_kernel(const float* x, const float* t, int C, int64_t HW,
                                                             int64_t npix, float* per_px, double* part) {
  __shared__ double red[RED_THREADS / 64];
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    float tv[CM];
    load_t<CM>(t + off, C, HW, tv);
    const float lse = logf(sm.s);
    float l = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) l += tv[c] * (sm.d[c] - lse);
    if (per_px) per_px[q] = -l;
    acc += (double)(-l);
  }
  if (part) {
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  }
}

// gx_c = g * (p_c * sum(t) - t_c); g = gpp[q] (reduction 'none') or gout[0] / npix
template <int CM>
__global__ void ce_bwd_kernel(const float* x, const float* t, int C, int64_t HW, int64_t npix, const float* gout,
                              int per_px, float* gx) {
  const float gs = per_px ? 0.f : gout[0] / (float)npix;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    float tv[CM];
    load_t<CM>(t + off, C, HW, tv);
    float st = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) st += tv[c];
    const float g = per_px ? gout[q] : gs;
    const float inv = 1.f / sm.s;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) gx[off + c * HW] = g * (sm.e[c] * inv * st - tv[c]);
  }
}

// ---- OHEM CE ----
// workspace: [HDR doubles: 0 threshold, 1 kept][2*RED_BLOCKS doubles][sel: 4 u32][hist: 4*256 u32][pred npix][ce npix]
struct OhemWs {
  double* hdr;
  double* part;
  unsigned* sel;   // [0] key prefix of the order statistic, [1] remaining rank inside the prefix
  unsigned* hist;
  float* pred;
  float* ce;
};
__host__ __device__ inline OhemWs ohem_ws(void* ws, int64_t npix) {
  OhemWs w;
  w.hdr = (double*)ws;
  w.part = w.hdr + HDR;
  w.sel = (unsigned*)(w.part + 2 * RED_BLOCKS);
  w.hist = w.sel + 4;
  w.pred = (float*)(w.hist + 4 * 256);
  w.ce = w.pred + npix;
  return w;
}

__global__ void ohem_init_kernel(unsigned* sel, unsigned* hist, unsigned k) {
  for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) hist[i] = 0u;
  if (threadIdx.x == 0) {
    sel[0] = 0u;
    sel[1] = k;
  }
}

template <int CM>
__global__ void ohem_px_kernel(const float* x, const float* t, int C, int64_t HW, int64_t npix, float* pred,
                               float* ce) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    float tv[CM];
    load_t<CM>(t + off, C, HW, tv);
    const float lse = logf(sm.s);
    float l = 0.f, best = tv[0], pe = sm.e[0];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < C) {
        l += tv[c] * (sm.d[c] - lse);
        if (c > 0 && tv[c] > best) {   // first maximum, like torch.argmax
          best = tv[c];
          pe = sm.e[c];
        }
      }
    }
    pred[q] = pe / sm.s;
    ce[q] = -l;
  }
}

// one radix pass (8 bits at `shift`) over the keys whose higher bits equal the prefix found so far.  pred >= 0,
// so the fp32 bit pattern orders like the value.  Integer atomics only: the counts do not depend on the order.
__global__ void __launch_bounds__(256) ohem_hist_kernel(const float* pred, int64_t npix, const unsigned* sel,
                                                        unsigned* hist, int shift) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned prefix = sel[0];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const unsigned key = __float_as_uint(pred[q]);
    const bool in = shift == 24 || ((key ^ prefix) >> (shift + 8)) == 0u;
    if (in) atomicAdd(&h[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// the digit of the order statistic in this pass: the counts staged in LDS by the whole block, scanned by one thread
__global__ void __launch_bounds__(256) ohem_pick_kernel(unsigned* sel, const unsigned* hist, int shift) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned k = sel[1], cum = 0u;
  int d = 0;
  for (; d < 255; ++d) {
    if (k < cum + h[d]) break;
    cum += h[d];
  }
  sel[0] |= (unsigned)d << shift;
  sel[1] = k - cum;
}

__global__ void __launch_bounds__(RED_THREADS) ohem_sum_kernel(const float* pred, const float* ce, int64_t npix,
                                                               const unsigned* sel, float thresh, double* part) {
  __shared__ double red[RED_THREADS / 64];
  const float thr = fmaxf(__uint_as_float(sel[0]), thresh);
  double num = 0.0, cnt = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    if (pred[q] < thr) {
      num += (double)ce[q];
      cnt += 1.0;
    }
  }
  num = block_sum(num, red);
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = num;
    part[2 * blockIdx.x + 1] = cnt;
  }
}

__global__ void __launch_bounds__(RED_THREADS) ohem_final_kernel(const double* part, int nparts, const unsigned* sel,
                                                                 float thresh, double* hdr, float* out) {
  __shared__ double red[RED_THREADS / 64];
  double num = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    num += part[2 * i];
    cnt += part[2 * i + 1];
  }
  num = block_sum(num, red);
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    hdr[0] = (double)fmaxf(__uint_as_float(sel[0]), thresh);
    hdr[1] = cnt;
    out[0] = (float)num / (float)cnt;   // empty selection: 0/0 = NaN, like the reference's mean of nothing
  }
}

template <int CM>
__global__ void ohem_bwd_kernel(const float* x, const float* t, int C, int64_t HW, int64_t npix, const double* hdr,
                                const float* pred, const float* gout, float* gx) {
  const float thr = (float)hdr[0];
  const float gs = gout[0] / (float)hdr[1];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    if (!(pred[q] < thr)) {
      for (int c = 0; c < C; ++c) gx[off + c * HW] = 0.f;
      continue;
    }
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    float tv[CM];
    load_t<CM>(t + off, C, HW, tv);
    float st = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) st += tv[c];
    const float inv = 1.f / sm.s;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) gx[off + c * HW] = gs * (sm.e[c] * inv * st - tv[c]);
  }
}

// ---- label-map CE and OHEM: labels [B,HW] uint8 / int64 read in place, with a void label ----
// The labelled channel is selected by comparison over the registers, never by indexing memory with the label: a label
// outside [0, C) that is not the ignore value selects nothing and is void like it (no host check without a sync).
__device__ __forceinline__ int64_t load_label(const void* labels, int kind, int64_t q) {
  return kind == SSSEG_LOVASZ_LABEL_U8 ? (int64_t)((const unsigned char*)labels)[q] : ((const int64_t*)labels)[q];
}
__device__ __forceinline__ bool label_valid(int64_t lab, int64_t ignore, int C) {
  return lab != ignore && lab >= 0 && lab < (int64_t)C;
}

// p_c - [c == y] with p_c = e_c * inv rounded before the subtraction: what the dense kernels'
// (e_c * inv) * sum(t) - t_c gives on a one-hot target, whether or not the compiler fuses that (the product by
// sum(t) = 1 is exact).  Here the fusion of e_c * inv into the subtraction would round once instead of twice, so
// contraction is off.
__device__ __forceinline__ float prob_minus_onehot(float e, float inv, float t) {
#pragma clang fp contract(off)
  const float p = e * inv;
  return p - t;
}

// F.cross_entropy(x, y, weight, ignore_index, reduction, label_smoothing) per pixel:
// l = (1 - eps) w_y (-logp_y) + eps / C sum_c w_c (-logp_c), 0 where void.  part: (sum l, sum w_y) per block.
// No weight and eps == 0: -(d_y - lse), the dense kernel's value on a one-hot target, bit for bit.
template <int CM>
__global__ void __launch_bounds__(RED_THREADS) cel_fwd_kernel(const float* x, const void* labels, int kind, int C,
                                                              int64_t HW, int64_t npix, const float* weight,
                                                              int64_t ignore, float eps, float* per_px, double* part) {
  __shared__ double red[RED_THREADS / 64];
  const bool plain = !weight && eps == 0.f;
  const float a = 1.f - eps, bs = eps / (float)C;
  double num = 0.0, den = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lab = load_label(labels, kind, q);
    float l = 0.f, wy = 0.f;
    if (label_valid(lab, ignore, C)) {
      const int y = (int)lab;
      const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
      Soft<CM> sm;
      sm.load(x + off, C, HW);
      const float lse = logf(sm.s);
      float dy = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c == y) dy = sm.d[c];
      if (plain) {
        l = -(dy - lse);
        wy = 1.f;
      } else {
        float all = 0.f;
        wy = 1.f;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          if (c < C) {
            const float wc = weight ? weight[c] : 1.f;
            if (c == y) wy = wc;
            all += wc * (lse - sm.d[c]);
          }
        }
        l = a * wy * (lse - dy) + bs * all;
      }
    }
    if (per_px) per_px[q] = l;
    num += (double)l;
    den += (double)wy;
  }
  if (part) {
    num = block_sum(num, red);
    den = block_sum(den, red);
    if (threadIdx.x == 0) {
      part[2 * blockIdx.x] = num;
      part[2 * blockIdx.x + 1] = den;
    }
  }
}

// hdr[0] = sum of w_y over the valid pixels (the 'mean' denominator, read by the backward); out[0] = num / den
// ('mean'; 0/0 = NaN like torch when everything is void, 0 with empty_zero) or num ('sum')
__global__ void __launch_bounds__(RED_THREADS) cel_final_kernel(const double* part, int nparts, int mean,
                                                                int empty_zero, double* hdr, float* out) {
  __shared__ double red[RED_THREADS / 64];
  double num = 0.0, den = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    num += part[2 * i];
    den += part[2 * i + 1];
  }
  num = block_sum(num, red);
  den = block_sum(den, red);
  if (threadIdx.x == 0) {
    hdr[0] = den;
    if (!mean) out[0] = (float)num;
    else out[0] = (den == 0.0 && empty_zero) ? 0.f : (float)(num / den);
  }
}

// gx_c = g * ((a w_y + bs sum_k w_k) p_c - a w_y [c == y] - bs w_c), zeros where void; g = gout[0] / hdr[0] (mean),
// gout[0] (sum) or gout[q] (none).  No weight and eps == 0: g * (p_c - [c == y]) as the dense kernel rounds it.
template <int CM>
__global__ void cel_bwd_kernel(const float* x, const void* labels, int kind, int C, int64_t HW, int64_t npix,
                               const float* weight, int64_t ignore, float eps, int reduction, const double* hdr,
                               const float* gout, float* gx) {
  const bool plain = !weight && eps == 0.f;
  const float a = 1.f - eps, bs = eps / (float)C;
  float gs = 0.f;
  if (reduction == SSSEG_RED_MEAN) gs = gout[0] / (float)hdr[0];
  else if (reduction == SSSEG_RED_SUM) gs = gout[0];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    const int64_t lab = load_label(labels, kind, q);
    if (!label_valid(lab, ignore, C)) {
      for (int c = 0; c < C; ++c) gx[off + c * HW] = 0.f;
      continue;
    }
    const int y = (int)lab;
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    const float g = reduction == SSSEG_RED_NONE ? gout[q] : gs;
    const float inv = 1.f / sm.s;
    if (plain) {
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) gx[off + c * HW] = g * prob_minus_onehot(sm.e[c], inv, c == y ? 1.f : 0.f);
    } else {
      float wy = 1.f, sw = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
          const float wc = weight ? weight[c] : 1.f;
          if (c == y) wy = wc;
          sw += wc;
        }
      }
      const float ay = a * wy, tot = ay + bs * sw;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
          const float wc = weight ? weight[c] : 1.f;
          gx[off + c * HW] = g * (sm.e[c] * inv * tot - (c == y ? ay : 0.f) - bs * wc);
        }
      }
    }
  }
}

// OHEM on a label map: pred = softmax at the label, +inf where void (its key sorts after every valid key and
// pred < threshold never holds), ce = 0 there; cnt[block] = the block's exact number of valid pixels
template <int CM>
__global__ void __launch_bounds__(RED_THREADS) ohl_px_kernel(const float* x, const void* labels, int kind, int C,
                                                             int64_t HW, int64_t npix, int64_t ignore, float* pred,
                                                             float* ce, double* cnt) {
  __shared__ double red[RED_THREADS / 64];
  double nv = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lab = load_label(labels, kind, q);
    if (!label_valid(lab, ignore, C)) {
      pred[q] = INFINITY;
      ce[q] = 0.f;
      continue;
    }
    const int y = (int)lab;
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    const float lse = logf(sm.s);
    float dy = 0.f, ey = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c == y) {
        dy = sm.d[c];
        ey = sm.e[c];
      }
    }
    pred[q] = ey / sm.s;
    ce[q] = -(dy - lse);
    nv += 1.0;
  }
  nv = block_sum(nv, red);
  if (threadIdx.x == 0) cnt[blockIdx.x] = nv;
}

// n_valid (integer-valued fp64 sum: exact in any order) -> hdr[2]; rank k = min(min_kept, n_valid - 1) for the
// radix select (0 when nothing is valid: the statistic is then a void key, +inf, and nothing is kept)
__global__ void __launch_bounds__(RED_THREADS) ohl_init_kernel(const double* cnt, int nparts, unsigned min_kept,
                                                               double* hdr, unsigned* sel, unsigned* hist) {
  __shared__ double red[RED_THREADS / 64];
  for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) hist[i] = 0u;
  double nv = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) nv += cnt[i];
  nv = block_sum(nv, red);
  if (threadIdx.x == 0) {
    const unsigned n = (unsigned)nv;
    hdr[2] = nv;
    sel[0] = 0u;
    sel[1] = n == 0u ? 0u : (min_kept < n - 1u ? min_kept : n - 1u);
  }
}

template <int CM>
__global__ void ohl_bwd_kernel(const float* x, const void* labels, int kind, int C, int64_t HW, int64_t npix,
                               const double* hdr, const float* pred, const float* gout, float* gx) {
  const float thr = (float)hdr[0];
  const float gs = gout[0] / (float)hdr[1];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    if (!(pred[q] < thr)) {   // void pixels hold +inf
      for (int c = 0; c < C; ++c) gx[off + c * HW] = 0.f;
      continue;
    }
    const int y = (int)load_label(labels, kind, q);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    const float inv = 1.f / sm.s;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) gx[off + c * HW] = gs * prob_minus_onehot(sm.e[c], inv, c == y ? 1.f : 0.f);
  }
}

// ---- FocalLoss ----
__global__ void __launch_bounds__(RED_THREADS) focal_partial_kernel(const float* x, const float* t, int64_t n,
                                                                    float alpha, float alpha1, float gamma,
                                                                    double* part) {
  __shared__ double red[RED_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i], tt = t[i];
    const float ce = bce_elem(v, tt);
    const float p = sigmoidf_ref(v);
    const float pt = tt * p + (1.f - tt) * (1.f - p);
    const float mod = powg(1.f - pt, gamma);
    const float aw = tt * alpha + (1.f - tt) * alpha1;
    acc += (double)(mod * aw * ce);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// autograd of the reference expression: aw * (ce * dmod/dx + mod * (p - t)),
// dmod/dx = -gamma (1 - p_t)^(gamma - 1) * (2 t - 1) * p (1 - p)
__global__ void focal_bwd_kernel(const float* x, const float* t, int64_t n, float alpha, float alpha1, float gamma,
                                 const float* gout, float* gx) {
  const float scale = gout[0] / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i], tt = t[i];
    const float ce = bce_elem(v, tt);
    const float p = sigmoidf_ref(v);
    const float pt = tt * p + (1.f - tt) * (1.f - p);
    const float om = 1.f - pt;
    const float mod = powg(om, gamma);
    const float aw = tt * alpha + (1.f - tt) * alpha1;
    const float dmod = -dpowg(om, gamma) * ((tt - (1.f - tt)) * (p * (1.f - p)));
    gx[i] = scale * aw * (ce * dmod + mod * (p - tt));
  }
}

// ---- NormalizedFocalLossSigmoid ----
// workspace: [HDR][part1: BC*CH*3 doubles (sum beta, #label != ignore, #label == -1)][plane: BC*3 doubles (the
// same, summed)][part2: BC*CH doubles][mult: BC floats][bsum: B floats]
struct NflWs {
  double* part1;
  double* plane;
  double* part2;
  float* mult;
  float* bsum;
};
__host__ __device__ inline NflWs nfl_ws(void* ws, int64_t B, int64_t C) {
  NflWs w;
  const int64_t BC = B * C;
  w.part1 = (double*)ws + HDR;
  w.plane = w.part1 + BC * PLANE_CHUNKS * 3;
  w.part2 = w.plane + BC * 3;
  w.mult = (float*)(w.part2 + BC * PLANE_CHUNKS);
  w.bsum = w.mult + BC;
  return w;
}

struct NflArgs {
  float alpha, alpha1, gamma, eps, scale, weight, ignore;
  int from_logits, size_average;
};

__device__ __forceinline__ float nfl_pt(float v, float lab, const NflArgs& a) {
  const float pred = a.from_logits ? v : sigmoidf_ref(v);
  const float pt = lab > 0.f ? pred : 1.f - pred;
  return lab != a.ignore ? pt : 1.f;
}

__global__ void __launch_bounds__(RED_THREADS) nfl_stats_kernel(const float* x, const float* label, int64_t HW,
                                                                NflArgs a, double* part1) {
  __shared__ double red[RED_THREADS / 64];
  const int64_t plane = blockIdx.y;
  const float* xp = x + plane * HW;
  const float* lp = label + plane * HW;
  double sb = 0.0, nv = 0.0, ni = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
    const float lab = lp[i];
    const float pt = nfl_pt(xp[i], lab, a);
    sb += (double)powg(1.f - pt, a.gamma);
    nv += lab != a.ignore ? 1.0 : 0.0;
    ni += lab == -1.f ? 1.0 : 0.0;
  }
  sb = block_sum(sb, red);
  nv = block_sum(nv, red);
  ni = block_sum(ni, red);
  if (threadIdx.x == 0) {
    double* o = part1 + (plane * gridDim.x + blockIdx.x) * 3;
    o[0] = sb;
    o[1] = nv;
    o[2] = ni;
  }
}

// mult[b,c] = HW / (sum beta + eps) in fp32, like the reference (a detached constant of the backward)
__global__ void nfl_mult_kernel(const double* part1, int nch, int64_t BC, int64_t HW, float eps, double* plane,
                                float* mult) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < BC; p += (int64_t)gridDim.x * blockDim.x) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nch; ++k)
      for (int j = 0; j < 3; ++j) s[j] += part1[(p * nch + k) * 3 + j];
    for (int j = 0; j < 3; ++j) plane[p * 3 + j] = s[j];
    mult[p] = (float)HW / ((float)s[0] + eps);
  }
}

__global__ void __launch_bounds__(RED_THREADS) nfl_loss_kernel(const float* x, const float* label, int64_t HW,
                                                               NflArgs a, const float* mult, double* part2) {
  __shared__ double red[RED_THREADS / 64];
  const int64_t plane = blockIdx.y;
  const float* xp = x + plane * HW;
  const float* lp = label + plane * HW;
  const float m = mult[plane];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
    const float lab = lp[i];
    const float pt = nfl_pt(xp[i], lab, a);
    const float al = lab > 0.f ? a.alpha : a.alpha1;
    const float beta = powg(1.f - pt, a.gamma) * m;
    const float l = -al * beta * logf(fminf(pt + a.eps, 1.f));
    const float sw = lab != a.ignore ? 1.f : 0.f;
    acc += (double)(a.weight * (l * sw));
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part2[plane * gridDim.x + blockIdx.x] = acc;
}

// per-sample loss, and the EMA of the mean mult over the samples without a -1 label (losses.py:135-138)
__global__ void nfl_final_kernel(const double* part2, const double* plane, const float* mult, int nch, int64_t B,
                                 int64_t C, NflArgs a, float* bsum, float* out, float* k_sum) {
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
    double s = 0.0, nv = 0.0;
    for (int64_t c = 0; c < C; ++c) {
      for (int k = 0; k < nch; ++k) s += part2[(b * C + c) * nch + k];
      nv += plane[(b * C + c) * 3 + 1];
    }
    const float den = a.size_average ? (float)nv + a.eps : 1.f;
    bsum[b] = den;
    out[b] = a.scale * ((float)s / den);
  }
  if (threadIdx.x == 0 && k_sum) {
    double tot = 0.0;
    int64_t cnt = 0;
    for (int64_t b = 0; b < B; ++b) {
      double ign = 0.0;
      float sm = 0.f;
      for (int64_t c = 0; c < C; ++c) {
        ign += plane[(b * C + c) * 3 + 2];
        sm += mult[b * C + c];
      }
      if (ign == 0.0) {
        tot += (double)(sm / (float)C);
        ++cnt;
      }
    }
    if (cnt > 0) k_sum[0] = (float)(0.9 * (double)k_sum[0] + 0.1 * (double)(float)(tot / (double)cnt));
  }
}

// d loss_b / d x: mult and the per-sample denominator are constants
__global__ void nfl_bwd_kernel(const float* x, const float* label, int64_t HW, int64_t C, NflArgs a,
                               const float* mult, const float* bsum, const float* gout, float* gx) {
  const int64_t plane = blockIdx.y, b = plane / C;
  const float* xp = x + plane * HW;
  const float* lp = label + plane * HW;
  float* gp = gx + plane * HW;
  const float m = mult[plane];
  const float gs = gout[b] * a.scale / bsum[b] * a.weight;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
    const float lab = lp[i], v = xp[i];
    float g = 0.f;
    if (lab != a.ignore) {
      const float pred = a.from_logits ? v : sigmoidf_ref(v);
      const float pt = lab > 0.f ? pred : 1.f - pred;
      const float al = lab > 0.f ? a.alpha : a.alpha1;
      const float om = 1.f - pt, pe = pt + a.eps;
      // d/dpt of -al * m * om^gamma * log(min(pt + eps, 1))
      const float dlog = pe < 1.f ? 1.f / pe : 0.f;
      const float dpt = -al * m * (-dpowg(om, a.gamma) * logf(fminf(pe, 1.f)) + powg(om, a.gamma) * dlog);
      const float dpred = lab > 0.f ? dpt : -dpt;
      g = gs * dpred * (a.from_logits ? 1.f : pred * (1.f - pred));
    }
    gp[i] = g;
  }
}

// ---- DiceWithLogitsLoss ----
// workspace: [HDR][part: B*CH*3*C doubles][dice, mask, A, Bc: 4 * B*C floats][nm: B floats]
struct DiceWs {
  double* part;
  float *dice, *mask, *A, *Bc, *nm;
};
__host__ __device__ inline DiceWs dice_ws(void* ws, int64_t B, int64_t C) {
  DiceWs w;
  w.part = (double*)ws + HDR;
  w.dice = (float*)(w.part + B * PLANE_CHUNKS * 3 * C);
  w.mask = w.dice + B * C;
  w.A = w.mask + B * C;
  w.Bc = w.A + B * C;
  w.nm = w.Bc + B * C;
  return w;
}

template <int CM>
__global__ void __launch_bounds__(RED_THREADS) dice_part_kernel(const float* x, const float* t, int C, int64_t HW,
                                                                double* part) {
  __shared__ double red[RED_THREADS / 64];
  const int64_t b = blockIdx.y;
  float ai[CM], ap[CM], at[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) ai[c] = ap[c] = at[c] = 0.f;
  for (int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < HW; pix += (int64_t)gridDim.x * blockDim.x) {
    const int64_t off = b * C * HW + pix;
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    float tv[CM];
    load_t<CM>(t + off, C, HW, tv);
    const float inv = 1.f / sm.s;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const float p = sm.e[c] * inv;
      ai[c] += p * tv[c];
      ap[c] += p;
      at[c] += tv[c];
    }
  }
  double* o = part + (b * gridDim.x + blockIdx.x) * 3 * C;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    if (c < C) {   // C is uniform over the block
      const double ri = block_sum((double)ai[c], red);
      const double rp = block_sum((double)ap[c], red);
      const double rt = block_sum((double)at[c], red);
      if (threadIdx.x == 0) {
        o[c] = ri;
        o[C + c] = rp;
        o[2 * C + c] = rt;
      }
    }
  }
}

__global__ void __launch_bounds__(256) dice_final_kernel(DiceWs w, int nch, int64_t B, int64_t C, float* out) {
  const int64_t BC = B * C;
  for (int64_t p = threadIdx.x; p < BC; p += blockDim.x) {
    const int64_t b = p / C, c = p - b * C;
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nch; ++k)
      for (int j = 0; j < 3; ++j) s[j] += w.part[((b * nch + k) * 3 + j) * C + c];
    const float inter = (float)s[0], card = (float)(s[1] + s[2]), st = (float)s[2];
    const float num = 2.f * inter + 1.f, den = card + 1.f;
    w.dice[p] = num / den;
    w.mask[p] = st > 1.f ? 1.f : 0.f;
    w.A[p] = num;   // staged for the coefficients below
    w.Bc[p] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int64_t b = 0; b < B; ++b) {
      float sd = 0.f, nm = 0.f;
      for (int64_t c = 0; c < C; ++c) {
        sd += w.dice[b * C + c] * w.mask[b * C + c];
        nm += w.mask[b * C + c];
      }
      w.nm[b] = nm;
      tot += sd / nm;   // no class present in the sample: 0/0 = NaN, as in the reference
    }
    out[0] = 1.f - tot / (float)B;
  }
  __syncthreads();
  // d loss / d p_c(pixel) = -(A t_c - Bc): A = k 2/den, Bc = k num/den^2, k = mask / (nm_b B)
  for (int64_t p = threadIdx.x; p < BC; p += blockDim.x) {
    const int64_t b = p / C;
    const float k = w.mask[p] / (w.nm[b] * (float)B), num = w.A[p], den = w.Bc[p];
    w.A[p] = k * 2.f / den;
    w.Bc[p] = k * num / (den * den);
  }
}

template <int CM>
__global__ void dice_bwd_kernel(const float* x, const float* t, int C, int64_t HW, int64_t npix, const float* A,
                                const float* Bc, const float* gout, float* gx) {
  const float g = gout[0];
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    float gp[CM];
    const float inv = 1.f / sm.s;
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      gp[c] = 0.f;
      if (c < C) {
        gp[c] = -g * (A[b * C + c] * t[off + c * HW] - Bc[b * C + c]);
        dot += gp[c] * (sm.e[c] * inv);
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) gx[off + c * HW] = sm.e[c] * inv * (gp[c] - dot);
  }
}

// ---- dice_loss / log_dice_loss on probabilities: per-sample sums over n = C*HW ----
// workspace: [HDR][part: B*CH*2 doubles][num, den: 2*B floats]
__global__ void __launch_bounds__(RED_THREADS) dicep_part_kernel(const float* x, const float* t, int64_t n,
                                                                 double* part) {
  __shared__ double red[RED_THREADS / 64];
  const int64_t b = blockIdx.y;
  const float* xp = x + b * n;
  const float* tp = t + b * n;
  double si = 0.0, sc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = xp[i], tt = tp[i];
    si += (double)(v * tt);
    sc += (double)(v + tt);
  }
  si = block_sum(si, red);
  sc = block_sum(sc, red);
  if (threadIdx.x == 0) {
    part[(b * gridDim.x + blockIdx.x) * 2] = si;
    part[(b * gridDim.x + blockIdx.x) * 2 + 1] = sc;
  }
}

__global__ void dicep_final_kernel(const double* part, int nch, int64_t B, int log_mode, float gamma, float* nd,
                                   float* out) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
    double si = 0.0, sc = 0.0;
    for (int k = 0; k < nch; ++k) {
      si += part[(b * nch + k) * 2];
      sc += part[(b * nch + k) * 2 + 1];
    }
    const float num = 2.f * (float)si + 1.f, den = (float)sc + 1.f;
    nd[2 * b] = num;
    nd[2 * b + 1] = den;
    const float r = num / den;
    out[b] = log_mode ? powf(-logf(r), gamma) : 1.f - r;
  }
}

__global__ void dicep_bwd_kernel(const float* t, int64_t n, int log_mode, float gamma, const float* nd,
                                 const float* gout, float* gx) {
  const int64_t b = blockIdx.y;
  const float num = nd[2 * b], den = nd[2 * b + 1], r = num / den;
  // d loss_b / d r
  const float dr = log_mode ? gamma * powf(-logf(r), gamma - 1.f) * (-1.f / r) : -1.f;
  const float g = gout[b] * dr;
  const float* tp = t + b * n;
  float* gp = gx + b * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    gp[i] = g * ((2.f * tp[i] * den - num) / (den * den));
}

// ---- entropies ----
// as written in the reference: sigmoid, then log (NaN where the fp32 sigmoid is exactly 1 or 0)
__global__ void __launch_bounds__(RED_THREADS) bent_partial_kernel(const float* x, int64_t n, double* part) {
  __shared__ double red[RED_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p = sigmoidf_ref(x[i]), q = 1.f - p;
    acc += (double)(p * logf(p) + q * logf(q));
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ void bent_bwd_kernel(const float* x, int64_t n, const float* gout, float* gx) {
  const float scale = -gout[0] / 2.f / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float p = sigmoidf_ref(x[i]), q = 1.f - p;
    // autograd of p*log(p) + q*log(q), q = 1 - p, term by term (NaN where the reference's is)
    const float dp = (logf(p) + p * (1.f / p)) - (logf(q) + q * (1.f / q));
    gx[i] = scale * dp * (p * q);
  }
}

template <int CM>
__global__ void __launch_bounds__(RED_THREADS) ent_partial_kernel(const float* x, int C, int64_t HW, int64_t npix,
                                                                  double* part) {
  __shared__ double red[RED_THREADS / 64];
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    const float lse = logf(sm.s), inv = 1.f / sm.s;
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) h += sm.e[c] * inv * (sm.d[c] - lse);
    acc += (double)(-h);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// d H / d x_c = -p_c (log p_c + H), H = -sum p log p
template <int CM>
__global__ void ent_bwd_kernel(const float* x, int C, int64_t HW, int64_t npix, const float* gout, float* gx) {
  const float gs = gout[0] / (float)npix;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = q / HW, off = b * C * HW + (q - b * HW);
    Soft<CM> sm;
    sm.load(x + off, C, HW);
    const float lse = logf(sm.s), inv = 1.f / sm.s;
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) h += sm.e[c] * inv * (sm.d[c] - lse);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) gx[off + c * HW] = -gs * (sm.e[c] * inv) * ((sm.d[c] - lse) - h);
  }
}

// ---- BCE with reduction 'none' / 'sum' ----
__global__ void __launch_bounds__(RED_THREADS) bce_red_kernel(const float* x, const float* t, int64_t n,
                                                              float* per_elem, double* part) {
  __shared__ double red[RED_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float l = bce_elem(x[i], t[i]);
    if (per_elem) per_elem[i] = l;
    acc += (double)l;
  }
  if (part) {
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
  }
}

__global__ void bce_red_bwd_kernel(const float* x, const float* t, int64_t n, const float* gout, int per_elem,
                                   float* gx) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    gx[i] = (sigmoidf_ref(x[i]) - t[i]) * (per_elem ? gout[i] : gout[0]);
}

// out = t * a + b, each operation rounded (no contraction): target * (1 - alpha) + alpha / C
__global__ void smooth_kernel(const float* __restrict__ t, float* __restrict__ out, int64_t n, float a, float b) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = __fadd_rn(__fmul_rn(t[i], a), b);
}

int red_blocks(int64_t n) { return ssseg_grid(n, RED_THREADS, RED_BLOCKS); }
int plane_chunks(int64_t n) { return ssseg_grid(n, RED_THREADS, PLANE_CHUNKS); }
bool bad_shape(int64_t B, int64_t C, int64_t HW) {
  return B <= 0 || C < 1 || C > 64 || HW <= 0 || B * HW >= ((int64_t)1 << 31) || B * C > 65535;
}

}  // namespace

// launch KERNEL<CM> with CM = the next power of two >= C (2 at the least)
#define SEG_LAUNCH_C(KERNEL, C, grid, block, stream, ...)                                        \
  do {                                                                                           \
    if ((C) <= 2) hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, stream, __VA_ARGS__);          \
    else if ((C) <= 4) hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, stream, __VA_ARGS__);     \
    else if ((C) <= 8) hipLaunchKernelGGL((KERNEL<8>), grid, block, 0, stream, __VA_ARGS__);     \
    else if ((C) <= 16) hipLaunchKernelGGL((KERNEL<16>), grid, block, 0, stream, __VA_ARGS__);   \
    else if ((C) <= 32) hipLaunchKernelGGL((KERNEL<32>), grid, block, 0, stream, __VA_ARGS__);   \
    else hipLaunchKernelGGL((KERNEL<64>), grid, block, 0, stream, __VA_ARGS__);                  \
  } while (0)

extern "C" size_t ssseg_segloss_workspace_bytes(int kind, int64_t B, int64_t C, int64_t HW) {
  if (B <= 0 || C <= 0 || HW <= 0) return 0;
  const size_t hdr = sizeof(double) * HDR, d = sizeof(double), f = sizeof(float);
  const size_t BC = (size_t)(B * C);
  switch (kind) {
    case SSSEG_LOSS_REDUCE: return hdr + d * RED_BLOCKS;
    case SSSEG_LOSS_OHEM: return hdr + d * 2 * RED_BLOCKS + 4 * (4 + 4 * 256) + f * 2 * (size_t)(B * HW);
    case SSSEG_LOSS_NFL: return hdr + d * (BC * PLANE_CHUNKS * 3 + BC * 3 + BC * PLANE_CHUNKS) + f * (BC + B);
    case SSSEG_LOSS_DICE_LOGITS: return hdr + d * BC * PLANE_CHUNKS * 3 + f * (4 * BC + B);
    case SSSEG_LOSS_DICE_PROB: return hdr + d * (size_t)B * PLANE_CHUNKS * 2 + f * 2 * (size_t)B;
    case SSSEG_LOSS_CE_LABELS: return hdr + d * 2 * RED_BLOCKS;
    case SSSEG_LOSS_OHEM_LABELS: return hdr + d * 2 * RED_BLOCKS + 4 * (4 + 4 * 256) + f * 2 * (size_t)(B * HW);
  }
  return 0;
}

#define SEG_WS_CHECK(kind, B, C, HW) \
  if (!ws || ws_bytes < ssseg_segloss_workspace_bytes(kind, B, C, HW)) return SSSEG_EWORKSPACE

extern "C" int ssseg_ce_fwd(const float* x, const float* t, int64_t B, int64_t C, int64_t HW, int reduction,
                            float* out, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !t || !out || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  if (reduction != SSSEG_RED_NONE && reduction != SSSEG_RED_MEAN) return SSSEG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = B * HW;
  const int nb = red_blocks(npix);
  if (reduction == SSSEG_RED_NONE) {
    SEG_LAUNCH_C(ce_fwd_kernel, C, dim3(nb), dim3(RED_THREADS), s, x, t, (int)C, HW, npix, out, (double*)nullptr);
  } else {
    SEG_WS_CHECK(SSSEG_LOSS_REDUCE, B, C, HW);
    double* part = (double*)ws + HDR;
    SEG_LAUNCH_C(ce_fwd_kernel, C, dim3(nb), dim3(RED_THREADS), s, x, t, (int)C, HW, npix, (float*)nullptr, part);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)part, nb,
                       1.0 / (double)npix, out);
  }
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_ce_bwd(const float* x, const float* t, int64_t B, int64_t C, int64_t HW, int reduction,
                            const float* gout, float* gx, ssseg_stream_t stream) {
  if (!x || !t || !gout || !gx || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  if (reduction != SSSEG_RED_NONE && reduction != SSSEG_RED_MEAN) return SSSEG_EINVAL;
  const int64_t npix = B * HW;
  SEG_LAUNCH_C(ce_bwd_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), (hipStream_t)stream, x, t, (int)C, HW, npix,
               gout, (int)(reduction == SSSEG_RED_NONE), gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_ohem_fwd(const float* x, const float* t, int64_t B, int64_t C, int64_t HW, float thresh,
                              int64_t min_kept, float* out, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !t || !out || bad_shape(B, C, HW) || min_kept < 0) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_OHEM, B, C, HW);
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = B * HW;
  const OhemWs w = ohem_ws(ws, npix);
  const unsigned k = (unsigned)(min_kept < npix - 1 ? min_kept : npix - 1);
  const int nb = red_blocks(npix);
  hipLaunchKernelGGL(ohem_init_kernel, dim3(1), dim3(256), 0, s, w.sel, w.hist, k);
  SEG_LAUNCH_C(ohem_px_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), s, x, t, (int)C, HW, npix, w.pred, w.ce);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hipLaunchKernelGGL(ohem_hist_kernel, dim3(nb), dim3(256), 0, s, (const float*)w.pred, npix,
                       (const unsigned*)w.sel, w.hist + 256 * pass, shift);
    hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(256), 0, s, w.sel, (const unsigned*)(w.hist + 256 * pass),
                       shift);
  }
  hipLaunchKernelGGL(ohem_sum_kernel, dim3(nb), dim3(RED_THREADS), 0, s, (const float*)w.pred, (const float*)w.ce,
                     npix, (const unsigned*)w.sel, thresh, w.part);
  hipLaunchKernelGGL(ohem_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)w.part, nb,
                     (const unsigned*)w.sel, thresh, w.hdr, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_ohem_bwd(const float* x, const float* t, int64_t B, int64_t C, int64_t HW, const float* gout,
                              float* gx, const void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !t || !gout || !gx || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_OHEM, B, C, HW);
  const int64_t npix = B * HW;
  const OhemWs w = ohem_ws(const_cast<void*>(ws), npix);
  SEG_LAUNCH_C(ohem_bwd_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), (hipStream_t)stream, x, t, (int)C, HW,
               npix, (const double*)w.hdr, (const float*)w.pred, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

static bool bad_labels(const void* labels, int label_kind, int64_t C) {
  return !labels || C < 2 || (label_kind != SSSEG_LOVASZ_LABEL_I64 && label_kind != SSSEG_LOVASZ_LABEL_U8);
}

extern "C" int ssseg_ce_labels_fwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                   int64_t HW, const float* weight, int64_t ignore_index, float label_smoothing,
                                   int reduction, int empty_zero, float* out, void* ws, size_t ws_bytes,
                                   ssseg_stream_t stream) {
  if (!x || !out || bad_shape(B, C, HW) || bad_labels(labels, label_kind, C)) return SSSEG_EINVAL;
  if (reduction < SSSEG_RED_NONE || reduction > SSSEG_RED_SUM) return SSSEG_EINVAL;
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return SSSEG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = B * HW;
  const int nb = red_blocks(npix);
  if (reduction == SSSEG_RED_NONE) {
    SEG_LAUNCH_C(cel_fwd_kernel, C, dim3(nb), dim3(RED_THREADS), s, x, labels, label_kind, (int)C, HW, npix, weight,
                 ignore_index, label_smoothing, out, (double*)nullptr);
  } else {
    SEG_WS_CHECK(SSSEG_LOSS_CE_LABELS, B, C, HW);
    double* hdr = (double*)ws;
    double* part = hdr + HDR;
    SEG_LAUNCH_C(cel_fwd_kernel, C, dim3(nb), dim3(RED_THREADS), s, x, labels, label_kind, (int)C, HW, npix, weight,
                 ignore_index, label_smoothing, (float*)nullptr, part);
    hipLaunchKernelGGL(cel_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)part, nb,
                       (int)(reduction == SSSEG_RED_MEAN), empty_zero, hdr, out);
  }
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_ce_labels_bwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                   int64_t HW, const float* weight, int64_t ignore_index, float label_smoothing,
                                   int reduction, const float* gout, float* gx, const void* ws, size_t ws_bytes,
                                   ssseg_stream_t stream) {
  if (!x || !gout || !gx || bad_shape(B, C, HW) || bad_labels(labels, label_kind, C)) return SSSEG_EINVAL;
  if (reduction < SSSEG_RED_NONE || reduction > SSSEG_RED_SUM) return SSSEG_EINVAL;
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return SSSEG_EINVAL;
  if (reduction == SSSEG_RED_MEAN) SEG_WS_CHECK(SSSEG_LOSS_CE_LABELS, B, C, HW);   // the denominator lives there
  const int64_t npix = B * HW;
  SEG_LAUNCH_C(cel_bwd_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), (hipStream_t)stream, x, labels, label_kind,
               (int)C, HW, npix, weight, ignore_index, label_smoothing, reduction, (const double*)ws, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_ohem_labels_fwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                     int64_t HW, int64_t ignore_label, float thresh, int64_t min_kept, float* out,
                                     void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !out || bad_shape(B, C, HW) || bad_labels(labels, label_kind, C) || min_kept < 0) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_OHEM_LABELS, B, C, HW);
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = B * HW;
  const OhemWs w = ohem_ws(ws, npix);
  const unsigned k = (unsigned)(min_kept < npix ? min_kept : npix);   // clamped to n_valid - 1 on the device
  const int nb = red_blocks(npix);
  SEG_LAUNCH_C(ohl_px_kernel, C, dim3(nb), dim3(RED_THREADS), s, x, labels, label_kind, (int)C, HW, npix,
               ignore_label, w.pred, w.ce, w.part);
  hipLaunchKernelGGL(ohl_init_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)w.part, nb, k, w.hdr, w.sel,
                     w.hist);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hipLaunchKernelGGL(ohem_hist_kernel, dim3(nb), dim3(256), 0, s, (const float*)w.pred, npix,
                       (const unsigned*)w.sel, w.hist + 256 * pass, shift);
    hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(256), 0, s, w.sel, (const unsigned*)(w.hist + 256 * pass),
                       shift);
  }
  hipLaunchKernelGGL(ohem_sum_kernel, dim3(nb), dim3(RED_THREADS), 0, s, (const float*)w.pred, (const float*)w.ce,
                     npix, (const unsigned*)w.sel, thresh, w.part);
  hipLaunchKernelGGL(ohem_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)w.part, nb,
                     (const unsigned*)w.sel, thresh, w.hdr, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_ohem_labels_bwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                     int64_t HW, const float* gout, float* gx, const void* ws, size_t ws_bytes,
                                     ssseg_stream_t stream) {
  if (!x || !gout || !gx || bad_shape(B, C, HW) || bad_labels(labels, label_kind, C)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_OHEM_LABELS, B, C, HW);
  const int64_t npix = B * HW;
  const OhemWs w = ohem_ws(const_cast<void*>(ws), npix);
  SEG_LAUNCH_C(ohl_bwd_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), (hipStream_t)stream, x, labels, label_kind,
               (int)C, HW, npix, (const double*)w.hdr, (const float*)w.pred, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_focal_fwd(const float* x, const float* t, int64_t n, double alpha, double gamma, float* out,
                               void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !t || !out || n <= 0) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_REDUCE, 1, 1, n);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws + HDR;
  const int nb = red_blocks(n);
  hipLaunchKernelGGL(focal_partial_kernel, dim3(nb), dim3(RED_THREADS), 0, s, x, t, n, (float)alpha,
                     (float)(1.0 - alpha), (float)gamma, part);
  hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)part, nb, 1.0 / (double)n,
                     out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_focal_bwd(const float* x, const float* t, int64_t n, double alpha, double gamma,
                               const float* gout, float* gx, ssseg_stream_t stream) {
  if (!x || !t || !gout || !gx || n <= 0) return SSSEG_EINVAL;
  hipLaunchKernelGGL(focal_bwd_kernel, dim3(ssseg_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, x, t, n,
                     (float)alpha, (float)(1.0 - alpha), (float)gamma, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

static NflArgs nfl_args(const ssseg_nfl_params* p) {
  NflArgs a;
  a.alpha = (float)p->alpha;
  a.alpha1 = (float)(1.0 - p->alpha);
  a.gamma = (float)p->gamma;
  a.eps = (float)p->eps;
  a.scale = (float)p->scale;
  a.weight = (float)p->weight;
  a.ignore = (float)p->ignore_label;
  a.from_logits = p->from_logits;
  a.size_average = p->size_average;
  return a;
}

extern "C" int ssseg_nfl_fwd(const float* x, const float* label, int64_t B, int64_t C, int64_t HW,
                             const ssseg_nfl_params* params_host, float* out, float* k_sum, void* ws,
                             size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !label || !params_host || !out || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_NFL, B, C, HW);
  hipStream_t s = (hipStream_t)stream;
  const NflArgs a = nfl_args(params_host);
  const NflWs w = nfl_ws(ws, B, C);
  const int nch = plane_chunks(HW);
  const dim3 grid(nch, (unsigned)(B * C));
  hipLaunchKernelGGL(nfl_stats_kernel, grid, dim3(RED_THREADS), 0, s, x, label, HW, a, w.part1);
  hipLaunchKernelGGL(nfl_mult_kernel, dim3(ssseg_grid(B * C, 256)), dim3(256), 0, s, (const double*)w.part1, nch,
                     B * C, HW, a.eps, w.plane, w.mult);
  hipLaunchKernelGGL(nfl_loss_kernel, grid, dim3(RED_THREADS), 0, s, x, label, HW, a, (const float*)w.mult, w.part2);
  hipLaunchKernelGGL(nfl_final_kernel, dim3(1), dim3(256), 0, s, (const double*)w.part2, (const double*)w.plane,
                     (const float*)w.mult, nch, B, C, a, w.bsum, out, k_sum);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_nfl_bwd(const float* x, const float* label, int64_t B, int64_t C, int64_t HW,
                             const ssseg_nfl_params* params_host, const float* gout, float* gx, const void* ws,
                             size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !label || !params_host || !gout || !gx || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_NFL, B, C, HW);
  const NflArgs a = nfl_args(params_host);
  const NflWs w = nfl_ws(const_cast<void*>(ws), B, C);
  const dim3 grid(ssseg_grid(HW, 256, 256), (unsigned)(B * C));
  hipLaunchKernelGGL(nfl_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, label, HW, C, a,
                     (const float*)w.mult, (const float*)w.bsum, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_dice_logits_fwd(const float* x, const float* t, int64_t B, int64_t C, int64_t HW, float* out,
                                     void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !t || !out || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_DICE_LOGITS, B, C, HW);
  hipStream_t s = (hipStream_t)stream;
  const DiceWs w = dice_ws(ws, B, C);
  const int nch = plane_chunks(HW);
  SEG_LAUNCH_C(dice_part_kernel, C, dim3(nch, (unsigned)B), dim3(RED_THREADS), s, x, t, (int)C, HW, w.part);
  hipLaunchKernelGGL(dice_final_kernel, dim3(1), dim3(256), 0, s, w, nch, B, C, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_dice_logits_bwd(const float* x, const float* t, int64_t B, int64_t C, int64_t HW,
                                     const float* gout, float* gx, const void* ws, size_t ws_bytes,
                                     ssseg_stream_t stream) {
  if (!x || !t || !gout || !gx || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_DICE_LOGITS, B, C, HW);
  const DiceWs w = dice_ws(const_cast<void*>(ws), B, C);
  const int64_t npix = B * HW;
  SEG_LAUNCH_C(dice_bwd_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), (hipStream_t)stream, x, t, (int)C, HW,
               npix, (const float*)w.A, (const float*)w.Bc, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_dice_prob_fwd(const float* p, const float* t, int64_t B, int64_t n, int log_mode, float gamma,
                                   float* out, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!p || !t || !out || B <= 0 || B > 65535 || n <= 0) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_DICE_PROB, B, 1, n);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws + HDR;
  float* nd = (float*)(part + B * PLANE_CHUNKS * 2);
  const int nch = plane_chunks(n);
  hipLaunchKernelGGL(dicep_part_kernel, dim3(nch, (unsigned)B), dim3(RED_THREADS), 0, s, p, t, n, part);
  hipLaunchKernelGGL(dicep_final_kernel, dim3(ssseg_grid(B, 256)), dim3(256), 0, s, (const double*)part, nch, B,
                     log_mode, gamma, nd, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_dice_prob_bwd(const float* t, int64_t B, int64_t n, int log_mode, float gamma,
                                   const float* gout, float* gx, const void* ws, size_t ws_bytes,
                                   ssseg_stream_t stream) {
  if (!t || !gout || !gx || B <= 0 || B > 65535 || n <= 0) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_DICE_PROB, B, 1, n);
  const float* nd = (const float*)((const double*)ws + HDR + B * PLANE_CHUNKS * 2);
  hipLaunchKernelGGL(dicep_bwd_kernel, dim3(ssseg_grid(n, 256, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     t, n, log_mode, gamma, nd, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_binary_entropy_fwd(const float* x, int64_t n, float* out, void* ws, size_t ws_bytes,
                                        ssseg_stream_t stream) {
  if (!x || !out || n <= 0) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_REDUCE, 1, 1, n);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws + HDR;
  const int nb = red_blocks(n);
  hipLaunchKernelGGL(bent_partial_kernel, dim3(nb), dim3(RED_THREADS), 0, s, x, n, part);
  hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)part, nb,
                     -0.5 / (double)n, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_binary_entropy_bwd(const float* x, int64_t n, const float* gout, float* gx,
                                        ssseg_stream_t stream) {
  if (!x || !gout || !gx || n <= 0) return SSSEG_EINVAL;
  hipLaunchKernelGGL(bent_bwd_kernel, dim3(ssseg_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_entropy_fwd(const float* x, int64_t B, int64_t C, int64_t HW, float* out, void* ws,
                                 size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !out || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  SEG_WS_CHECK(SSSEG_LOSS_REDUCE, B, C, HW);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws + HDR;
  const int64_t npix = B * HW;
  const int nb = red_blocks(npix);
  SEG_LAUNCH_C(ent_partial_kernel, C, dim3(nb), dim3(RED_THREADS), s, x, (int)C, HW, npix, part);
  hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)part, nb,
                     1.0 / (double)npix, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_entropy_bwd(const float* x, int64_t B, int64_t C, int64_t HW, const float* gout, float* gx,
                                 ssseg_stream_t stream) {
  if (!x || !gout || !gx || bad_shape(B, C, HW)) return SSSEG_EINVAL;
  const int64_t npix = B * HW;
  SEG_LAUNCH_C(ent_bwd_kernel, C, dim3(ssseg_grid(npix, 256)), dim3(256), (hipStream_t)stream, x, (int)C, HW, npix,
               gout, gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_bce_logits_red_fwd(const float* x, const float* t, int64_t n, int reduction, float* out,
                                        void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !t || !out || n <= 0) return SSSEG_EINVAL;
  if (reduction != SSSEG_RED_NONE && reduction != SSSEG_RED_SUM) return SSSEG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nb = red_blocks(n);
  if (reduction == SSSEG_RED_NONE) {
    hipLaunchKernelGGL(bce_red_kernel, dim3(ssseg_grid(n, 256)), dim3(RED_THREADS), 0, s, x, t, n, out,
                       (double*)nullptr);
  } else {
    SEG_WS_CHECK(SSSEG_LOSS_REDUCE, 1, 1, n);
    double* part = (double*)ws + HDR;
    hipLaunchKernelGGL(bce_red_kernel, dim3(nb), dim3(RED_THREADS), 0, s, x, t, n, (float*)nullptr, part);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, (const double*)part, nb, 1.0, out);
  }
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_bce_logits_red_bwd(const float* x, const float* t, int64_t n, int reduction, const float* gout,
                                        float* gx, ssseg_stream_t stream) {
  if (!x || !t || !gout || !gx || n <= 0) return SSSEG_EINVAL;
  if (reduction != SSSEG_RED_NONE && reduction != SSSEG_RED_SUM) return SSSEG_EINVAL;
  hipLaunchKernelGGL(bce_red_bwd_kernel, dim3(ssseg_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, x, t, n, gout,
                     (int)(reduction == SSSEG_RED_NONE), gx);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_smooth_labels(const float* t, float* out, int64_t n, float a, float b, ssseg_stream_t stream) {
  if (!t || !out || n < 0) return SSSEG_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(smooth_kernel, dim3(ssseg_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, t, out, n, a, b);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
