// The multi-class (2 <= C <= 64 mutually exclusive classes) forms of the semi-supervised step's two-class kernels:
//   softmax consistency loss  (train.py:97-108 with the softmax lines :97,:99 in place of the sigmoid ones),
//   pseudo-label consistency  (cross-entropy against the teacher's hard label, weighted by its confidence),
//   C-class validation metrics (train.py:171-175 with num_classes = C, lovasz.iou lovasz.py:54-73),
//   C-class inference head     (models/inference_wrapper.py:17-24).
// Conventions of eltwise.hip / seglosses.hip: contiguous fp32 [B,C,HW], per-block fp64 partials + one final block in
// the caller's workspace, no floating-point atomics, no allocation, no synchronisation (graph-capturable).
#include "common.h"

namespace {

constexpr int RED_BLOCKS = 1024;    // partial pairs that fit ssseg_reduce_workspace_bytes()
constexpr int RED_THREADS = 256;
constexpr int SM_TILE = 256;        // pixels of one sample per workgroup round: one pixel per thread
constexpr int SM_BWD_BLOCKS = 4096;

// ---- softmax consistency -------------------------------------------------------------------------------------------
// A tile is SM_TILE consecutive pixels of one sample; a workgroup walks tiles grid-strided (one 64-bit division per
// TILE, none per pixel).  Each thread owns one pixel and holds its CMAX student and CMAX teacher logits in registers:
// every load of the tile is issued before the first use (2*C loads in flight per thread, each coalesced across the
// wave at channel stride HW), and the maximum, the exponentials, the sum and the squared difference are all taken
// from those registers -- s and t come from memory exactly once per kernel, and nothing is staged in LDS.
// CMAX is the channel bucket (2, 4, 8, 16, 32, 64): the loops are fully unrolled so the arrays never leave registers.
template <int CMAX>
struct SmPixel {
  float ps[CMAX], pt[CMAX];   // logits, then probabilities
  float conf;                 // max_c pt

  __device__ __forceinline__ void load(const float* __restrict__ sp, const float* __restrict__ tp, int C, int64_t HW) {
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      // clamped address instead of a branch around the load: the whole batch stays in flight together
      const int64_t o = (int64_t)(c < C ? c : 0) * HW;
      ps[c] = sp[o];
      pt[c] = tp[o];
    }
  }

  // softmax of both rows in place (maximum subtracted: logits of +-1e4 stay finite); channels >= C become 0
  __device__ __forceinline__ void softmax(int C) {
    float ms = ps[0], mt = pt[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c) {
      if (c < C) {
        ms = fmaxf(ms, ps[c]);
        mt = fmaxf(mt, pt[c]);
      }
    }
    float zs = 0.f, zt = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      ps[c] = c < C ? expf(ps[c] - ms) : 0.f;
      pt[c] = c < C ? expf(pt[c] - mt) : 0.f;
      zs += ps[c];
      zt += pt[c];
    }
    const float rs = 1.f / zs, rt = 1.f / zt;
    conf = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      ps[c] *= rs;
      pt[c] *= rt;
      conf = fmaxf(conf, pt[c]);
    }
  }
};

template <int CMAX>
__global__ void __launch_bounds__(SM_TILE) cons_sm_partial_kernel(const float* __restrict__ s,
                                                                  const float* __restrict__ t,
                                                                  const float* __restrict__ w, int C, int64_t HW,
                                                                  int64_t tiles_per_sample, int64_t ntiles, float thr,
                                                                  double* __restrict__ part) {
  __shared__ double red[SM_TILE / 64];
  double num = 0.0, cnt = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b = tile / tiles_per_sample;
    const int64_t pix = (tile - b * tiles_per_sample) * SM_TILE + threadIdx.x;
    if (pix < HW) {
      const int64_t base = b * C * HW + pix;
      SmPixel<CMAX> px;
      px.load(s + base, t + base, C, HW);
      const float wv = w ? w[b * HW + pix] : 1.f;
      px.softmax(C);
      float d2 = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        const float d = px.ps[c] - px.pt[c];
        d2 += d * d;
      }
      if (px.conf > thr) {
        const double cmw = (double)wv;
        num += (double)d2 * cmw;
        cnt += cmw;
      }
    }
  }
  num = block_sum(num, red);
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = num;
    part[2 * blockIdx.x + 1] = cnt;
  }
}

__global__ void __launch_bounds__(RED_THREADS) cons_sm_final_kernel(const double* __restrict__ part, int nparts,
                                                                    int64_t npix, float* __restrict__ out3) {
  __shared__ double red[RED_THREADS / 64];
  double num = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    num += part[2 * i];
    cnt += part[2 * i + 1];
  }
  num = block_sum(num, red);
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    out3[0] = (float)num / (float)cnt;   // 0/0 = NaN when no pixel is confident (train.py:106)
    out3[1] = (float)(cnt / (double)npix);
    out3[2] = (float)cnt;
  }
}

// gs_c = 2 gout cm / sum(cm) * ps_c * (d_c - sum_k d_k ps_k): the softmax Jacobian applied to 2 d cm / sum(cm)
template <int CMAX>
__global__ void __launch_bounds__(SM_TILE) cons_sm_bwd_kernel(const float* __restrict__ s,
                                                                  const float* __restrict__ t,
                                                                  const float* __restrict__ w, int C, int64_t HW,
                                                                  int64_t tiles_per_sample, int64_t ntiles, float thr,
                                                                  const float* __restrict__ out3,
                                                                  const float* __restrict__ gout,
                                                                  float* __restrict__ gs) {
  const float scale = gout[0] / out3[2];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b = tile / tiles_per_sample;
    const int64_t pix = (tile - b * tiles_per_sample) * SM_TILE + threadIdx.x;
    if (pix >= HW) continue;
    const int64_t base = b * C * HW + pix;
    SmPixel<CMAX> px;
    px.load(s + base, t + base, C, HW);
    const float wv = w ? w[b * HW + pix] : 1.f;
    px.softmax(C);
    const float cm = px.conf > thr ? wv : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) dot += (px.ps[c] - px.pt[c]) * px.ps[c];
    const float k = 2.f * cm * scale;
    float* gp = gs + base;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) gp[(int64_t)c * HW] = k * (px.ps[c] * ((px.ps[c] - px.pt[c]) - dot));
  }
}

// ---- pseudo-label consistency: confidence-weighted cross-entropy ---------------------------------------------------
// The student is trained with cross-entropy against the teacher's hard label y = argmax_c t_c, weighted by the
// teacher's confidence conf = max_c softmax(t) = 1 / sum_c exp(t_c - max t) (FixMatch: per pixel, 'pixel'; ClassMix:
// the batch's confident fraction, 'batch').  The same tile walk as above.  The forward needs no C-wide row: both
// operands stream through K-channel chunks (K = 2, 4, 8; 2 * K loads in flight per thread) into a running maximum and a
// rescaled sum each, and the student logit at the teacher's running argmax is picked on the way.  The backward needs
// softmax(s) at every channel and keeps the student row in registers (the channel buckets above); its teacher pass is
// the forward's chunk for chunk, so that both decide conf > thr from the same bits.
constexpr int CE_SUMS = 3;   // N_w, S_cm and S_conf ('pixel') or S_all ('batch'): partials per workgroup

// running maximum m and sum z = sum_c exp(v_c - m) over the channels seen so far; channels >= C are left out.  FIRST:
// the chunk at channel 0, which has nothing to rescale.  FAST: the hardware exponential (v_exp_f32 of x log2 e:
// relative error about 2^-23 (1 + |x|) on these arguments <= 0) -- the teacher's sum feeds one comparison, conf > thr,
// and nothing else, and its exponentials were a sixth of the backward's time at 19 classes; the student's sums, which
// feed the loss and the gradient, take expf
template <bool FAST>
__device__ __forceinline__ float ce_exp(float x) {
  return FAST ? __expf(x) : expf(x);
}

template <int K, bool FIRST, bool FAST>
__device__ __forceinline__ void ce_absorb(float& m, float& z, const float (&v)[K], int c0, int C) {
  float mx = FIRST ? v[0] : m;
#pragma unroll
  for (int k = FIRST ? 1 : 0; k < K; ++k)
    if (c0 + k < C) mx = fmaxf(mx, v[k]);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) acc += c0 + k < C ? ce_exp<FAST>(v[k] - mx) : 0.f;
  z = FIRST ? acc : fmaf(z, ce_exp<FAST>(m - mx), acc);
  m = mx;
}

// torch.argmax over the channels, chunk after chunk (argmax_c's rule: the first maximum wins, NaN counts as the
// maximum, the first NaN wins); `pick` follows the winner (the student's logit at that channel)
template <int K, bool FIRST>
__device__ __forceinline__ void ce_argmax(float& best, int& arg, float& pick, const float (&tv)[K],
                                          const float (&sv)[K], int c0, int C) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = c0 + k;
    const float v = tv[k];
    const bool take = (FIRST && k == 0) || (c < C && (v > best || (v != v && best == best)));
    best = take ? v : best;
    arg = take ? c : arg;
    pick = take ? sv[k] : pick;
  }
}

// one pixel's running state of the forward, fed K channels of both operands at a time
struct CePixel {
  float mt, zt, ms, zs, best, sy;
  int arg;

  template <int K, bool FIRST>
  __device__ __forceinline__ void chunk(const float* __restrict__ sp, const float* __restrict__ tp, int c0, int C,
                                        int64_t HW) {
    float sv[K], tv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      // clamped address instead of a branch around the load: the whole chunk stays in flight together
      const int64_t o = (int64_t)(c0 + k < C ? c0 + k : c0) * HW;
      sv[k] = sp[o];
      tv[k] = tp[o];
    }
    ce_argmax<K, FIRST>(best, arg, sy, tv, sv, c0, C);
    ce_absorb<K, FIRST, true>(mt, zt, tv, c0, C);
    ce_absorb<K, FIRST, false>(ms, zs, sv, c0, C);
  }
};

// CLS: the threshold is per class, thr_c[y] (device, C floats: the self-adaptive thresholds of adaptive_thr.hip), in the
// place of the scalar thr -- one indexed load per pixel, y always inside [0, C); the scalar instantiations do not
// touch thr_c
template <int K, bool CLS>
__global__ void __launch_bounds__(SM_TILE) cons_ce_partial_kernel(const float* __restrict__ s,
                                                                  const float* __restrict__ t,
                                                                  const float* __restrict__ w, int C, int64_t HW,
                                                                  int64_t tiles_per_sample, int64_t ntiles, float thr,
                                                                  const float* __restrict__ thr_c, int weighting,
                                                                  double* __restrict__ part) {
  __shared__ double red[CE_SUMS][SM_TILE / 64];
  double nw = 0.0, scm = 0.0, sce = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b = tile / tiles_per_sample;
    const int64_t pix = (tile - b * tiles_per_sample) * SM_TILE + threadIdx.x;
    if (pix < HW) {
      const float* sp = s + b * C * HW + pix;
      const float* tp = t + b * C * HW + pix;
      const float wv = w ? w[b * HW + pix] : 1.f;
      CePixel px;
      px.chunk<K, true>(sp, tp, 0, C, HW);
      for (int c0 = K; c0 < C; c0 += K) px.chunk<K, false>(sp, tp, c0, C, HW);
      const float ce = (px.ms - px.sy) + logf(px.zs);
      const double wd = (double)wv, wce = (double)wv * (double)ce;
      const bool cm = 1.f / px.zt > (CLS ? thr_c[px.arg] : thr);
      nw += wd;
      if (cm) scm += wd;
      // 'pixel': selected, not multiplied -- an unconfident pixel's inf / NaN ce stays out of S_conf
      if (cm || weighting != 0) sce += wce;
    }
  }
  // the three sums through one pair of barriers
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  nw = wave_sum(nw);
  scm = wave_sum(scm);
  sce = wave_sum(sce);
  if (lane == 0) {
    red[0][wid] = nw;
    red[1][wid] = scm;
    red[2][wid] = sce;
  }
  __syncthreads();
  if (threadIdx.x < CE_SUMS) {
    double v = 0.0;
    for (int i = 0; i < SM_TILE / 64; ++i) v += red[threadIdx.x][i];
    part[(int64_t)CE_SUMS * blockIdx.x + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(RED_THREADS) cons_ce_final_kernel(const double* __restrict__ part, int nparts,
                                                                    int64_t npix, int weighting,
                                                                    float* __restrict__ out4) {
  __shared__ double red[RED_THREADS / 64];
  double acc[CE_SUMS] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += blockDim.x)
#pragma unroll
    for (int k = 0; k < CE_SUMS; ++k) acc[k] += part[(int64_t)CE_SUMS * i + k];
#pragma unroll
  for (int k = 0; k < CE_SUMS; ++k) acc[k] = block_sum(acc[k], red);
  if (threadIdx.x == 0) {
    const double nw = acc[0], scm = acc[1];
    // 'pixel': S_conf / N_w (exactly 0 when no pixel is confident);  'batch': (S_cm / N_w) (S_all / N_w);  N_w == 0: NaN
    out4[0] = (float)(weighting == 0 ? acc[2] / nw : (scm / nw) * (acc[2] / nw));
    out4[1] = (float)(scm / (double)npix);
    out4[2] = (float)scm;
    out4[3] = (float)nw;
  }
}

// gs_c = gout k (softmax(s)_c - [c == y]);  'pixel': k = w cm / N_w, exact zeros where cm == 0 (selected: the student's
// row may be inf / NaN there);  'batch': k = (S_cm / N_w) w / N_w at every pixel
template <int CMAX, bool CLS>
__global__ void __launch_bounds__(SM_TILE) cons_ce_bwd_kernel(const float* __restrict__ s,
                                                              const float* __restrict__ t,
                                                              const float* __restrict__ w, int C, int64_t HW,
                                                              int64_t tiles_per_sample, int64_t ntiles, float thr,
                                                              const float* __restrict__ thr_c, int weighting,
                                                              const float* __restrict__ out4,
                                                              const float* __restrict__ gout,
                                                              float* __restrict__ gs) {
  constexpr int K = CMAX < 8 ? CMAX : 8;   // the forward's chunk for this C
  const float scale = weighting == 0 ? gout[0] / out4[3] : gout[0] * (out4[2] / out4[3]) / out4[3];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b = tile / tiles_per_sample;
    const int64_t pix = (tile - b * tiles_per_sample) * SM_TILE + threadIdx.x;
    if (pix >= HW) continue;
    const int64_t base = b * C * HW + pix;
    const float* sp = s + base;
    const float* tp = t + base;
    float ps[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) ps[c] = sp[(int64_t)(c < C ? c : 0) * HW];
    const float wv = w ? w[b * HW + pix] : 1.f;
    float mt = 0.f, zt = 1.f, best = 0.f, pick = 0.f;
    int arg = 0;
    {
      float tv[K];
#pragma unroll
      for (int k = 0; k < K; ++k) tv[k] = tp[(int64_t)(k < C ? k : 0) * HW];
      ce_argmax<K, true>(best, arg, pick, tv, tv, 0, C);
      if (weighting == 0) ce_absorb<K, true, true>(mt, zt, tv, 0, C);
    }
#pragma unroll
    for (int c0 = K; c0 < CMAX; c0 += K) {
      if (c0 < C) {
        float tv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) tv[k] = tp[(int64_t)(c0 + k < C ? c0 + k : c0) * HW];
        ce_argmax<K, false>(best, arg, pick, tv, tv, c0, C);
        if (weighting == 0) ce_absorb<K, false, true>(mt, zt, tv, c0, C);
      }
    }
    const bool on = weighting != 0 || 1.f / zt > (CLS ? thr_c[arg] : thr);
    float ms = ps[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
      if (c < C) ms = fmaxf(ms, ps[c]);
    float zs = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      ps[c] = c < C ? expf(ps[c] - ms) : 0.f;
      zs += ps[c];
    }
    const float rs = 1.f / zs, k = wv * scale;
    float* gp = gs + base;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) gp[(int64_t)c * HW] = on ? k * (ps[c] * rs - (c == arg ? 1.f : 0.f)) : 0.f;
  }
}

// ---- C-class validation metrics ------------------------------------------------------------------------------------
constexpr int MET_THREADS = 256;
constexpr int MET_PIX_PER_THREAD = 8;
constexpr int MET_MAX_C = 64;
// rounds of MET_THREADS pixels between two flushes of the workgroup's u32 matrix: 2^22 * 256 = 2^30 increments at the
// most in one cell, so a u32 cannot wrap
constexpr int64_t MET_FLUSH_ROUNDS = (int64_t)1 << 22;

// ATen nearest_idx (UpSample.h) for scale_factor=None: identity, exact 2x, else floor(o * in/out).
__device__ __forceinline__ int64_t nearest_src(int64_t o, int64_t in, int64_t out) {
  if (out == in) return o;
  if (out == 2 * in) return o >> 1;
  const float scale = (float)in / (float)out;
  const int64_t i = (int64_t)floorf((float)o * scale);
  return i < in - 1 ? i : in - 1;
}

// torch.argmax over C strided values: first maximum wins, NaN counts as the maximum (the first NaN wins).
__device__ __forceinline__ int argmax_c(const float* __restrict__ p, int64_t stride, int C) {
  float best = p[0];
  int arg = 0;
  if (best != best) return 0;
  for (int c = 1; c < C; ++c) {
    const float v = p[(int64_t)c * stride];
    if (v != v) return c;
    if (v > best) {
      best = v;
      arg = c;
    }
  }
  return arg;
}

// grid (x: pixel blocks, y: image).  conf [C][C] u64 (zeroed by the caller): rows label, columns prediction, over the
// batch; dice [B][2] u64 (zeroed): I_b, card_b.  LABELS: target is a [B][H][W] int64 label map (ignore_on: pixels
// with label == ignore, and labels outside [0, C), are left out of every count), else a dense mask [B][C][H][W].
template <bool LABELS>
__global__ void __launch_bounds__(MET_THREADS)
seg_metrics_mc_count_kernel(const float* __restrict__ logits, int64_t lsb, int64_t lsc, int64_t lsh, int64_t lsw,
                            int64_t h, int64_t w, const void* __restrict__ target, int64_t msb, int64_t msc,
                            int64_t msh, int64_t msw, int64_t H, int64_t W, int C, int ignore_on, int64_t ignore,
                            unsigned long long* __restrict__ conf, unsigned long long* __restrict__ dice) {
  __shared__ unsigned mat[MET_MAX_C * MET_MAX_C];
  const int CC = C * C;
  for (int i = threadIdx.x; i < CC; i += MET_THREADS) mat[i] = 0u;
  __syncthreads();
  const int64_t b = blockIdx.y;
  const int64_t HW = H * W;
  const float* lb = logits + b * lsb;
  unsigned long long inter = 0, card = 0;
  const int64_t stride = (int64_t)gridDim.x * MET_THREADS;
  int64_t rounds = 0;
  // the trip count is the same for every thread of the workgroup (the flush below holds a barrier)
  for (int64_t p0 = (int64_t)blockIdx.x * MET_THREADS; p0 < HW; p0 += stride) {
    const int64_t p = p0 + threadIdx.x;
    if (p < HW) {
      const int64_t y = p / W, x = p - y * W;
      int label = -1;
      unsigned tsum = 0;        // sum_{c>=1} t_c
      const float* mp = nullptr;
      if (LABELS) {
        const int64_t lv = ((const int64_t*)target)[b * msb + y * msh + x * msw];
        if (!(ignore_on && lv == ignore) && lv >= 0 && lv < C) label = (int)lv;
        tsum = label >= 1 ? 1u : 0u;
      } else {
        mp = (const float*)target + b * msb + y * msh + x * msw;
        label = argmax_c(mp, msc, C);
        for (int c = 1; c < C; ++c) tsum += mp[(int64_t)c * msc] > 0.5f ? 1u : 0u;
      }
      if (label >= 0) {
        const int64_t sy = nearest_src(y, h, H), sx = nearest_src(x, w, W);
        const int pred = argmax_c(lb + sy * lsh + sx * lsw, lsc, C);
        atomicAdd(&mat[label * C + pred], 1u);
        if (pred >= 1) {
          const bool hit = LABELS ? pred == label : mp[(int64_t)pred * msc] > 0.5f;
          inter += hit ? 1u : 0u;
          card += 1u;
        }
        card += tsum;
      }
    }
    if (++rounds == MET_FLUSH_ROUNDS) {
      __syncthreads();
      for (int i = threadIdx.x; i < CC; i += MET_THREADS) {
        const unsigned v = mat[i];
        if (v) atomicAdd(conf + i, (unsigned long long)v);
        mat[i] = 0u;
      }
      __syncthreads();
      rounds = 0;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC; i += MET_THREADS) {
    const unsigned v = mat[i];
    if (v) atomicAdd(conf + i, (unsigned long long)v);
  }
  // the dice counters are 64-bit per thread (at most C per pixel): one wave reduction and one atomic per wave
  const int lane = threadIdx.x & (SSSEG_WAVE - 1);
  unsigned long long tot[2] = {inter, card};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    unsigned long long v = tot[k];
#pragma unroll
    for (int off = SSSEG_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SSSEG_WAVE);
    if (lane == 0 && v) atomicAdd(dice + b * 2 + k, v);
  }
}

// out[0] = mean_b (2 I_b + 1)/(card_b + 1) in fp32 (metrics.py:3-7);  out[2 + c] = 100 * IoU_c from the running total
// where one is given (EMPTY = 1 where union == 0);  out[1] = mean_c IoU_c
__global__ void __launch_bounds__(MET_THREADS) seg_metrics_mc_final_kernel(const unsigned long long* __restrict__ conf,
                                                                           const unsigned long long* __restrict__ dice,
                                                                           int64_t B, int C,
                                                                           unsigned long long* __restrict__ total,
                                                                           float* __restrict__ out) {
  __shared__ double iou[MET_MAX_C];
  const int CC = C * C;
  if (total) {
    for (int i = threadIdx.x; i < CC; i += MET_THREADS) total[i] += conf[i];
    __syncthreads();
  }
  const unsigned long long* m = total ? total : conf;
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    unsigned long long row = 0, col = 0;
    for (int k = 0; k < C; ++k) {
      row += m[c * C + k];
      col += m[k * C + c];
    }
    const unsigned long long in = m[c * C + c], un = row + col - in;
    iou[c] = un ? (double)in / (double)un : 1.0;
    out[2 + c] = 100.f * (float)iou[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) acc += iou[c];
    out[1] = (float)(acc / (double)C);
    double d = 0.0;
    for (int64_t b = 0; b < B; ++b) {
      const float inter = (float)dice[b * 2];
      const float card = (float)dice[b * 2 + 1];
      d += (double)((2.f * inter + 1.f) / (card + 1.f));
    }
    out[0] = (float)(d / (double)B);
  }
}

// ---- C-class inference head ----------------------------------------------------------------------------------------
// grid (x: pixel blocks, y: image); one pixel per thread, channel loads coalesced across the wave at stride HW.  The
// second and third walk over the C channels re-read lines this thread has just touched.
__global__ void prob_onehot_mc_kernel(const float* __restrict__ logits, int C, int64_t HW, int softmax,
                                      float* __restrict__ prob, float* __restrict__ onehot) {
  const int64_t b = blockIdx.y;
  const float* lb = logits + b * C * HW;
  float* pb = prob + b * C * HW;
  float* ob = onehot + b * C * HW;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (int64_t)gridDim.x * blockDim.x) {
    const int arg = argmax_c(lb + p, HW, C);
    if (softmax) {
      // the maximum over the non-NaN channels (fmaxf drops a NaN operand); a NaN logit then makes z, and with it the
      // whole row, NaN, like torch.softmax
      float mx = -INFINITY, z = 0.f;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, lb[(int64_t)c * HW + p]);
      for (int c = 0; c < C; ++c) z += expf(lb[(int64_t)c * HW + p] - mx);
      const float r = 1.f / z;
      for (int c = 0; c < C; ++c) pb[(int64_t)c * HW + p] = expf(lb[(int64_t)c * HW + p] - mx) * r;
    } else {
      for (int c = 0; c < C; ++c) pb[(int64_t)c * HW + p] = 1.f / (1.f + expf(-lb[(int64_t)c * HW + p]));
    }
    for (int c = 0; c < C; ++c) ob[(int64_t)c * HW + p] = c == arg ? 1.f : 0.f;
  }
}

template <int CMAX>
void launch_sm_fwd(int nb, hipStream_t st, const float* s, const float* t, const float* w, int C, int64_t HW,
                   int64_t tps, int64_t ntiles, float thr, double* part) {
  hipLaunchKernelGGL(cons_sm_partial_kernel<CMAX>, dim3(nb), dim3(SM_TILE), 0, st, s, t, w, C, HW, tps, ntiles, thr,
                     part);
}

template <int CMAX>
void launch_sm_bwd(int nb, hipStream_t st, const float* s, const float* t, const float* w, int C, int64_t HW,
                   int64_t tps, int64_t ntiles, float thr, const float* out3, const float* gout, float* gs) {
  hipLaunchKernelGGL(cons_sm_bwd_kernel<CMAX>, dim3(nb), dim3(SM_TILE), 0, st, s, t, w, C, HW, tps, ntiles, thr,
                     out3, gout, gs);
}

// thr_c == nullptr: the scalar threshold thr;  else the per-class thresholds (thr is not read)
template <int K>
void launch_ce_fwd(int nb, hipStream_t st, const float* s, const float* t, const float* w, int C, int64_t HW,
                   int64_t tps, int64_t ntiles, float thr, const float* thr_c, int weighting, double* part) {
  if (thr_c)
    hipLaunchKernelGGL((cons_ce_partial_kernel<K, true>), dim3(nb), dim3(SM_TILE), 0, st, s, t, w, C, HW, tps, ntiles,
                       thr, thr_c, weighting, part);
  else
    hipLaunchKernelGGL((cons_ce_partial_kernel<K, false>), dim3(nb), dim3(SM_TILE), 0, st, s, t, w, C, HW, tps, ntiles,
                       thr, thr_c, weighting, part);
}

template <int CMAX>
void launch_ce_bwd(int nb, hipStream_t st, const float* s, const float* t, const float* w, int C, int64_t HW,
                   int64_t tps, int64_t ntiles, float thr, const float* thr_c, int weighting, const float* out4,
                   const float* gout, float* gs) {
  if (thr_c)
    hipLaunchKernelGGL((cons_ce_bwd_kernel<CMAX, true>), dim3(nb), dim3(SM_TILE), 0, st, s, t, w, C, HW, tps, ntiles,
                       thr, thr_c, weighting, out4, gout, gs);
  else
    hipLaunchKernelGGL((cons_ce_bwd_kernel<CMAX, false>), dim3(nb), dim3(SM_TILE), 0, st, s, t, w, C, HW, tps, ntiles,
                       thr, thr_c, weighting, out4, gout, gs);
}

// the channel bucket of C: the smallest of 2, 4, 8, 16, 32, 64 that holds it
#define SM_DISPATCH(C, CALL)      \
  do {                            \
    if ((C) <= 2) CALL(2);        \
    else if ((C) <= 4) CALL(4);   \
    else if ((C) <= 8) CALL(8);   \
    else if ((C) <= 16) CALL(16); \
    else if ((C) <= 32) CALL(32); \
    else CALL(64);                \
  } while (0)

bool sm_args_ok(int64_t B, int64_t C, int64_t HW) {
  if (B <= 0 || C <= 0 || C > 64 || HW <= 0) return false;
  // the element count and the tile count stay far inside int64
  return B <= (INT64_MAX / 64) / HW / 64;
}

}  // namespace

extern "C" int ssseg_consistency_sm_fwd(const float* s, const float* t, const float* w, int64_t B, int64_t C,
                                        int64_t HW, float thr, float* out3, void* ws, size_t ws_bytes,
                                        ssseg_stream_t stream) {
  if (!s || !t || !out3 || !sm_args_ok(B, C, HW)) return SSSEG_EINVAL;
  if (!ws || ws_bytes < sizeof(double) * 2 * RED_BLOCKS) return SSSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tps = (HW + SM_TILE - 1) / SM_TILE, ntiles = B * tps;
  const int nb = (int)(ntiles < RED_BLOCKS ? ntiles : RED_BLOCKS);
#define SM_FWD(N) launch_sm_fwd<N>(nb, st, s, t, w, (int)C, HW, tps, ntiles, thr, (double*)ws)
  SM_DISPATCH(C, SM_FWD);
#undef SM_FWD
  hipLaunchKernelGGL(cons_sm_final_kernel, dim3(1), dim3(RED_THREADS), 0, st, (const double*)ws, nb, B * HW, out3);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_consistency_sm_bwd(const float* s, const float* t, const float* w, int64_t B, int64_t C,
                                        int64_t HW, float thr, const float* out3, const float* gout, float* gs,
                                        ssseg_stream_t stream) {
  if (!s || !t || !out3 || !gout || !gs || !sm_args_ok(B, C, HW)) return SSSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tps = (HW + SM_TILE - 1) / SM_TILE, ntiles = B * tps;
  const int nb = (int)(ntiles < SM_BWD_BLOCKS ? ntiles : SM_BWD_BLOCKS);
#define SM_BWD(N) launch_sm_bwd<N>(nb, st, s, t, w, (int)C, HW, tps, ntiles, thr, out3, gout, gs)
  SM_DISPATCH(C, SM_BWD);
#undef SM_BWD
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t ssseg_consistency_ce_workspace_bytes(int64_t) { return sizeof(double) * CE_SUMS * RED_BLOCKS; }

// both threshold forms of the two entry points: thr_c == nullptr is the scalar one
static int ce_fwd(const float* s, const float* t, const float* w, int64_t B, int64_t C, int64_t HW, float thr,
                  const float* thr_c, int weighting, float* out4, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!s || !t || !out4 || !sm_args_ok(B, C, HW) || (weighting != 0 && weighting != 1)) return SSSEG_EINVAL;
  if (!ws || ws_bytes < sizeof(double) * CE_SUMS * RED_BLOCKS) return SSSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tps = (HW + SM_TILE - 1) / SM_TILE, ntiles = B * tps;
  const int nb = (int)(ntiles < RED_BLOCKS ? ntiles : RED_BLOCKS);
  // the chunk of the streaming pass: the channel bucket up to 8
#define CE_FWD(N) launch_ce_fwd<N>(nb, st, s, t, w, (int)C, HW, tps, ntiles, thr, thr_c, weighting, (double*)ws)
  if (C <= 2) CE_FWD(2);
  else if (C <= 4) CE_FWD(4);
  else CE_FWD(8);
#undef CE_FWD
  hipLaunchKernelGGL(cons_ce_final_kernel, dim3(1), dim3(RED_THREADS), 0, st, (const double*)ws, nb, B * HW, weighting,
                     out4);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

static int ce_bwd(const float* s, const float* t, const float* w, int64_t B, int64_t C, int64_t HW, float thr,
                  const float* thr_c, int weighting, const float* out4, const float* gout, float* gs,
                  ssseg_stream_t stream) {
  if (!s || !t || !out4 || !gout || !gs || !sm_args_ok(B, C, HW) || (weighting != 0 && weighting != 1))
    return SSSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tps = (HW + SM_TILE - 1) / SM_TILE, ntiles = B * tps;
  const int nb = (int)(ntiles < SM_BWD_BLOCKS ? ntiles : SM_BWD_BLOCKS);
#define CE_BWD(N) launch_ce_bwd<N>(nb, st, s, t, w, (int)C, HW, tps, ntiles, thr, thr_c, weighting, out4, gout, gs)
  SM_DISPATCH(C, CE_BWD);
#undef CE_BWD
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_consistency_ce_fwd(const float* s, const float* t, const float* w, int64_t B, int64_t C,
                                        int64_t HW, float thr, int weighting, float* out4, void* ws, size_t ws_bytes,
                                        ssseg_stream_t stream) {
  return ce_fwd(s, t, w, B, C, HW, thr, nullptr, weighting, out4, ws, ws_bytes, stream);
}

extern "C" int ssseg_consistency_ce_bwd(const float* s, const float* t, const float* w, int64_t B, int64_t C,
                                        int64_t HW, float thr, int weighting, const float* out4, const float* gout,
                                        float* gs, ssseg_stream_t stream) {
  return ce_bwd(s, t, w, B, C, HW, thr, nullptr, weighting, out4, gout, gs, stream);
}

extern "C" int ssseg_consistency_ce_cls_fwd(const float* s, const float* t, const float* w, int64_t B, int64_t C,
                                            int64_t HW, const float* thr_c, int weighting, float* out4, void* ws,
                                            size_t ws_bytes, ssseg_stream_t stream) {
  if (!thr_c) return SSSEG_EINVAL;
  return ce_fwd(s, t, w, B, C, HW, 0.f, thr_c, weighting, out4, ws, ws_bytes, stream);
}

extern "C" int ssseg_consistency_ce_cls_bwd(const float* s, const float* t, const float* w, int64_t B, int64_t C,
                                            int64_t HW, const float* thr_c, int weighting, const float* out4,
                                            const float* gout, float* gs, ssseg_stream_t stream) {
  if (!thr_c) return SSSEG_EINVAL;
  return ce_bwd(s, t, w, B, C, HW, 0.f, thr_c, weighting, out4, gout, gs, stream);
}

extern "C" int ssseg_seg_metrics_mc(const float* logits, const int64_t* lstride, int64_t h, int64_t w,
                                    const void* target, const int64_t* tstride, int target_is_labels, int ignore_on,
                                    int64_t ignore, int64_t B, int64_t C, int64_t H, int64_t W,
                                    unsigned long long* conf, unsigned long long* total, unsigned long long* dice,
                                    float* out, ssseg_stream_t stream) {
  if (!logits || !lstride || !target || !tstride || !conf || !dice || !out) return SSSEG_EINVAL;
  if (B <= 0 || C <= 0 || C > MET_MAX_C || h <= 0 || w <= 0 || H <= 0 || W <= 0) return SSSEG_EINVAL;
  if (B > 65535) return SSSEG_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  SSSEG_TRY(hipMemsetAsync(conf, 0, (size_t)C * C * sizeof(unsigned long long), s));
  SSSEG_TRY(hipMemsetAsync(dice, 0, (size_t)B * 2 * sizeof(unsigned long long), s));
  const int64_t HW = H * W;
  int64_t bx = (HW + (int64_t)MET_THREADS * MET_PIX_PER_THREAD - 1) / ((int64_t)MET_THREADS * MET_PIX_PER_THREAD);
  if (bx < 1) bx = 1;
  if (bx > 4096) bx = 4096;
  const dim3 grid((unsigned)bx, (unsigned)B);
  if (target_is_labels)
    // label-map strides: tstride[0] batch, [1] row, [2] column (3 entries)
    hipLaunchKernelGGL(seg_metrics_mc_count_kernel<true>, grid, dim3(MET_THREADS), 0, s, logits, lstride[0], lstride[1],
                       lstride[2], lstride[3], h, w, target, tstride[0], (int64_t)0, tstride[1], tstride[2], H, W,
                       (int)C, ignore_on, ignore, conf, dice);
  else
    hipLaunchKernelGGL(seg_metrics_mc_count_kernel<false>, grid, dim3(MET_THREADS), 0, s, logits, lstride[0],
                       lstride[1], lstride[2], lstride[3], h, w, target, tstride[0], tstride[1], tstride[2], tstride[3],
                       H, W, (int)C, ignore_on, ignore, conf, dice);
  hipLaunchKernelGGL(seg_metrics_mc_final_kernel, dim3(1), dim3(MET_THREADS), 0, s, (const unsigned long long*)conf,
                     (const unsigned long long*)dice, B, (int)C, total, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_prob_onehot_mc(const float* logits, int64_t B, int64_t C, int64_t HW, int activation, float* prob,
                                    float* onehot, ssseg_stream_t stream) {
  if (!logits || !prob || !onehot || B <= 0 || C <= 0 || C > 64 || HW <= 0) return SSSEG_EINVAL;
  if (activation != 0 && activation != 1) return SSSEG_EINVAL;
  if (B > 65535) return SSSEG_EUNSUPPORTED;
  int64_t nb = (HW + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(prob_onehot_mc_kernel, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, (hipStream_t)stream, logits,
                     (int)C, HW, activation, prob, onehot);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
