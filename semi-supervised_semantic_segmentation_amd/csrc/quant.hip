// Post-training int8 inference (ssseg/quant.py): symmetric int8 per-tensor activations, symmetric int8 per-output-channel
// weights, int32 accumulation on the integer MFMA pipe, and the folded eval-BN epilogue of the 16-bit engine.
//   absmax_update    slot = max(slot, max finite |x|)                       (calibration observer)
//   quantize_i8      q = clamp(rint(x * (127 / slot)), -127, 127)           (activation -> int8 [P][rup(C,16)])
//   weight_quant_i8  per output channel: sw = amax / 127, qw = clamp(rint(w * (127 / amax)))  ([Kp][R][S][Cq])
//   conv_i8_fwd      acc = sum q * qw (exact, int32); y = act(fmaf(float(acc), (sx*sw)*scale, shift) + residual)
// Every fp32 operation is rounded as written (-ffp-contract=off; fmaf only where written), so the host restatement
// (tests/quant_ref.py) reproduces the quantised values bit for bit and bounds the epilogue by fp32 rounding alone.
//
// The conv is an implicit GEMM over 16-byte chunks of the contraction: chunk j of an output pixel is tap j / (Cq/16),
// channels 16 * (j % (Cq/16)) .. +15 of the input pixel that tap reaches (zeros outside the image), and chunk j of a
// filter is bytes 16j .. 16j+15 of its packed row, so any channel width that is a multiple of 16 bytes -- which the
// zero padding of q and qw guarantees -- runs the one loader.  A k-step is 4 chunks (64 bytes, one
// v_mfma_i32_16x16x64_i8); a short last step is zero-filled in LDS.  The FILTERS are the MFMA's A operand and the pixels
// its B operand: D then has the pixel on the lane (column = lane & 15) and four consecutive output channels in the
// lane's four registers (row = 4 * (lane >> 4) + reg), so a lane stores 4 channels of one pixel with one 8- or 16-byte
// store.  Operand map (pinned by the asymmetric exact test): lane l holds row / column l & 15, k = 16 * (l >> 4) .. +15.
#include "common.h"

namespace {

constexpr int Q_THREADS = 256;
constexpr int Q_GRID_CAP = 2048;   // workgroups of the grid-stride kernels

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block-wide max of non-negative values; scratch: Q_THREADS / 64 floats; result valid in every thread
__device__ __forceinline__ float block_max(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = wave_max(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < Q_THREADS / 64; ++i) t = fmaxf(t, scratch[i]);
  return t;
}

// |v| if finite, else 0
__device__ __forceinline__ float finite_abs(float v) {
  const float a = fabsf(v);
  return a <= 3.4028234663852886e38f ? a : 0.f;   // false for Inf and NaN
}

// the scheme's rounding: NaN -> 0, clamp to [-127, 127] (so +-Inf -> +-127), ties to even
__device__ __forceinline__ int quant1(float x, float inv) {
  const float t = __fmul_rn(x, inv);
  if (!(t == t)) return 0;
  return (int)fminf(fmaxf(rintf(t), -127.f), 127.f);
}

// ---- observer ------------------------------------------------------------------------------------------------------
// one thread per V-element group of a pixel's real channels; whole groups are one 16-byte load, the ragged tail and
// rows whose stride breaks the alignment are read element by element; channels >= C are never read
template <typename T>
__global__ void __launch_bounds__(Q_THREADS) absmax_kernel(const T* __restrict__ x, int64_t P, int C, int64_t ldx,
                                                          bool aligned, float* __restrict__ slot) {
  constexpr int V = Vec16<T>::V;
  __shared__ float scratch[Q_THREADS / 64];
  const int groups = (C + V - 1) / V;
  const int64_t total = P * groups;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * Q_THREADS) {
    const int64_t p = i / groups;
    const int c = (int)(i - p * groups) * V;
    const T* row = x + p * ldx + c;
    if (aligned && c + V <= C) {
      float v[V];
      Chunk<T, V>::cvt(Chunk<T, V>::ld(row), v);
#pragma unroll
      for (int e = 0; e < V; ++e) m = fmaxf(m, finite_abs(v[e]));
    } else {
      for (int e = 0; e < V && c + e < C; ++e) m = fmaxf(m, finite_abs(io<T>::ld(row, e)));
    }
  }
  m = block_max(m, scratch);
  // non-negative floats order like their bit patterns
  if (threadIdx.x == 0 && m > 0.f) atomicMax((unsigned*)slot, __float_as_uint(m));
}

// ---- activation quantise -------------------------------------------------------------------------------------------
// one thread per 16-byte output chunk (16 channels of one pixel); channels >= C are written as 0 and never read
template <typename T>
__global__ void __launch_bounds__(Q_THREADS) quantize_kernel(const T* __restrict__ x, int64_t P, int C, int64_t ldx,
                                                            bool aligned, const float* __restrict__ slot,
                                                            int8_t* __restrict__ q, int64_t ldq) {
  constexpr int V = Vec16<T>::V;
  const int chunks = (int)(ldq / 16);
  const int64_t total = P * chunks;
  const float a = slot[0];
  const float inv = a > 0.f ? __fdiv_rn(127.0f, a) : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * Q_THREADS) {
    const int64_t p = i / chunks;
    const int c0 = (int)(i - p * chunks) * 16;
    const T* row = x + p * ldx;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < 16 / V; ++g) {
      const int c = c0 + g * V;
      float v[V];
      if (aligned && c + V <= C) {
        Chunk<T, V>::cvt(Chunk<T, V>::ld(row + c), v);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = c + e < C ? io<T>::ld(row, c + e) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int b = g * V + e;
        const int qi = (a > 0.f && c + e < C) ? quant1(v[e], inv) : 0;
        w[b >> 2] |= ((unsigned)qi & 0xffu) << (8 * (b & 3));
      }
    }
    *(uint4*)(q + p * ldq + c0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ---- weight quantise + pack ----------------------------------------------------------------------------------------
// one workgroup per packed row k < Kp: rows >= K and channels >= C are zeros
__global__ void __launch_bounds__(Q_THREADS) weight_quant_kernel(const float* __restrict__ w, int K, int C, int R, int S,
                                                                int Cq, int8_t* __restrict__ qw,
                                                                float* __restrict__ sw) {
  __shared__ float scratch[Q_THREADS / 64];
  const int k = blockIdx.x;
  const int RS = R * S;
  const int64_t n = (int64_t)C * RS;
  int8_t* out = qw + (int64_t)k * RS * Cq;
  if (k >= K) {
    for (int64_t i = threadIdx.x; i < (int64_t)RS * Cq; i += Q_THREADS) out[i] = 0;
    if (threadIdx.x == 0) sw[k] = 0.f;
    return;
  }
  const float* wk = w + (int64_t)k * n;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += Q_THREADS) m = fmaxf(m, finite_abs(wk[i]));
  const float aw = block_max(m, scratch);
  const float inv = aw > 0.f ? __fdiv_rn(127.0f, aw) : 0.f;
  if (threadIdx.x == 0) sw[k] = aw > 0.f ? __fdiv_rn(aw, 127.0f) : 0.f;
  for (int64_t i = threadIdx.x; i < (int64_t)RS * Cq; i += Q_THREADS) {
    const int c = (int)(i % Cq);
    const int t = (int)(i / Cq);
    out[i] = (int8_t)((aw > 0.f && c < C) ? quant1(wk[(int64_t)c * RS + t], inv) : 0);
  }
}

// ---- int8 implicit-GEMM forward ------------------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int CV_BM = 128;       // pixels per tile
constexpr int CV_BK = 64;        // contraction bytes per k-step (4 chunks)

struct ConvI8 {
  int64_t M;                     // N * OH * OW
  int H, W, OH, OW, K, Kp;
  int R, S, sy, sx, dy, dx, py, px;
  int cpc;                       // 16-byte chunks per tap (Cq / 16)
  int nchunks;                   // R * S * cpc
  int64_t ldx, ldy, ldr;
  int act;
  float slope;
};

// LDS image of a tile: rows of 64 bytes; the 16-byte chunk c of row r lies at chunk (c ^ ((r >> 2) & 3)), so the 16 rows
// a ds_read_b128 of one k-chunk touches fall on 16 different 16-byte bank slots
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * CV_BK + ((chunk ^ ((row >> 2) & 3)) << 4); }

// 256 threads = 2 (pixel halves of 64) x 2 (channel halves of 16 * TN) waves; a wave owns TN x 4 MFMA tiles.
// BN = 32 * TN output channels per workgroup.
template <typename TO, int TN>
__global__ void __launch_bounds__(Q_THREADS) conv_i8_kernel(const int8_t* __restrict__ q, const int8_t* __restrict__ qw,
                                                           TO* __restrict__ y, ConvI8 g,
                                                           const float* __restrict__ slot,
                                                           const float* __restrict__ sw,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const TO* __restrict__ residual) {
  constexpr int BN = 32 * TN;
  constexpr int WROWS = BN / 64;   // filter rows each thread stages per k-step
  __shared__ __attribute__((aligned(16))) int8_t lds_x[2][CV_BM * CV_BK];
  __shared__ __attribute__((aligned(16))) int8_t lds_w[2][BN * CV_BK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.x * CV_BM;
  const int n0 = blockIdx.y * BN;

  // staging role: chunk column tid & 3 of rows (tid >> 2) + 64 i
  const int sc = tid & 3, sr = tid >> 2;
  int64_t xbase[2];
  int iy0[2], ix0[2];
  bool pvalid[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t m = m0 + sr + 64 * i;
    pvalid[i] = m < g.M;
    const int64_t mm = pvalid[i] ? m : 0;
    const int ox = (int)(mm % g.OW);
    const int64_t t = mm / g.OW;
    const int oy = (int)(t % g.OH);
    const int64_t n = t / g.OH;
    iy0[i] = oy * g.sy + g.py;
    ix0[i] = ox * g.sx + g.px;
    xbase[i] = n * g.H * (int64_t)g.W;
  }

  const int ksteps = (g.nchunks + 3) >> 2;
  uint4 rx[2], rw[WROWS];

  auto fetch = [&](int ks) {
    const int j = ks * 4 + sc;
    const bool live = j < g.nchunks;
    const int tap = live ? j / g.cpc : 0;
    const int c16 = j - tap * g.cpc;
    const int r = tap / g.S, s = tap - r * g.S;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int iy = iy0[i] + r * g.dy, ix = ix0[i] + s * g.dx;
      const bool ok = live && pvalid[i] && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
      rx[i] = make_uint4(0, 0, 0, 0);
      if (ok) rx[i] = *(const uint4*)(q + (xbase[i] + (int64_t)iy * g.W + ix) * g.ldx + (int64_t)c16 * 16);
    }
#pragma unroll
    for (int i = 0; i < WROWS; ++i) {
      const int n = n0 + sr + 64 * i;
      rw[i] = make_uint4(0, 0, 0, 0);
      if (live && n < g.Kp) rw[i] = *(const uint4*)(qw + ((int64_t)n * g.nchunks + j) * 16);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *(uint4*)(&lds_x[buf][lds_off(sr + 64 * i, sc)]) = rx[i];
#pragma unroll
    for (int i = 0; i < WROWS; ++i) *(uint4*)(&lds_w[buf][lds_off(sr + 64 * i, sc)]) = rw[i];
  };

  i32x4 acc[TN][4];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (i32x4){0, 0, 0, 0};

  fetch(0);
  stage(0);
  __syncthreads();
  const int fr = lane & 15, fc = lane >> 4;
  for (int ks = 0; ks < ksteps; ++ks) {
    const int buf = ks & 1;
    if (ks + 1 < ksteps) fetch(ks + 1);
    i32x4 fw[TN], fx[4];
#pragma unroll
    for (int i = 0; i < TN; ++i) fw[i] = *(const i32x4*)(&lds_w[buf][lds_off(wn * (16 * TN) + 16 * i + fr, fc)]);
#pragma unroll
    for (int j = 0; j < 4; ++j) fx[j] = *(const i32x4*)(&lds_x[buf][lds_off(wm * 64 + 16 * j + fr, fc)]);
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[i], fx[j], acc[i][j], 0, 0, 0);
    if (ks + 1 < ksteps) stage(buf ^ 1);   // the other buffer: its readers finished before the last barrier
    __syncthreads();
  }

  // epilogue: this lane holds channels nb .. nb + 3 of pixel m for every (i, j)
  const float sx = __fdiv_rn(slot[0], 127.0f);
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int nb = n0 + wn * (16 * TN) + 16 * i + 4 * fc;
    if (nb >= g.K) continue;
    float mul[4], sh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s1 = __fmul_rn(sx, sw[nb + e]);
      mul[e] = scale ? __fmul_rn(s1, scale[nb + e]) : s1;
      sh[e] = shift ? shift[nb + e] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t m = m0 + wm * 64 + 16 * j + fr;
      if (m >= g.M) continue;
      float v[4], res[4] = {0.f, 0.f, 0.f, 0.f};
      if (residual) Vec<TO, 4>::ld(residual + m * g.ldr + nb, res);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = fmaf((float)acc[i][j][e], mul[e], sh[e]);
        if (residual) t = __fadd_rn(t, res[e]);
        v[e] = act_fwd(t, g.act, g.slope);
      }
      Vec<TO, 4>::st(y + m * g.ldy + nb, v);
    }
  }
}

template <typename TO>
int launch_conv(const int8_t* q, const int8_t* qw, void* y, const ConvI8& g, const float* slot, const float* sw,
                const ssseg_conv_epilogue* epi, hipStream_t st) {
  const int64_t mt = (g.M + CV_BM - 1) / CV_BM;
  if (mt > 0x7fffffff) return SSSEG_EUNSUPPORTED;
  const float* scale = epi ? epi->scale : nullptr;
  const float* shift = epi ? epi->shift : nullptr;
  const TO* res = epi ? (const TO*)epi->residual : nullptr;
  if (g.K <= 64) {
    dim3 grid((unsigned)mt, (unsigned)((g.K + 63) / 64));
    hipLaunchKernelGGL((conv_i8_kernel<TO, 2>), grid, dim3(Q_THREADS), 0, st, q, qw, (TO*)y, g, slot, sw, scale, shift,
                       res);
  } else {
    dim3 grid((unsigned)mt, (unsigned)((g.K + 127) / 128));
    hipLaunchKernelGGL((conv_i8_kernel<TO, 4>), grid, dim3(Q_THREADS), 0, st, q, qw, (TO*)y, g, slot, sw, scale, shift,
                       res);
  }
  SSSEG_LAUNCH_CHECK();
  return SSSEG_OK;
}

bool fits_int(int64_t v) { return v >= -0x7fffffffLL && v <= 0x7fffffffLL; }

}  // namespace

extern "C" int ssseg_absmax_update(const void* x, int64_t P, int64_t C, int64_t ldx, int dt, float* slot,
                                   ssseg_stream_t stream) {
  if (!x || !slot) return SSSEG_EINVAL;
  if (P < 0 || C < 1 || ldx < C || C > 0x7fffffff) return SSSEG_EINVAL;
  if (dt != SSSEG_F32 && dt != SSSEG_BF16 && dt != SSSEG_F16) return SSSEG_EUNSUPPORTED;
  if (P == 0) return SSSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  const int V = dt == SSSEG_F32 ? 4 : 8;
  const bool aligned = ldx % V == 0 && ((uintptr_t)x & 15) == 0;
  const int grid = ssseg_grid(P * ((C + V - 1) / V), Q_THREADS, Q_GRID_CAP);
  if (dt == SSSEG_F32)
    hipLaunchKernelGGL(absmax_kernel<float>, dim3(grid), dim3(Q_THREADS), 0, st, (const float*)x, P, (int)C, ldx,
                       aligned, slot);
  else if (dt == SSSEG_BF16)
    hipLaunchKernelGGL(absmax_kernel<bf16_t>, dim3(grid), dim3(Q_THREADS), 0, st, (const bf16_t*)x, P, (int)C, ldx,
                       aligned, slot);
  else
    hipLaunchKernelGGL(absmax_kernel<f16_t>, dim3(grid), dim3(Q_THREADS), 0, st, (const f16_t*)x, P, (int)C, ldx,
                       aligned, slot);
  SSSEG_LAUNCH_CHECK();
  return SSSEG_OK;
}

extern "C" int ssseg_quantize_i8(const void* x, int64_t P, int64_t C, int64_t ldx, int dt, const float* slot, int8_t* q,
                                 int64_t ldq, ssseg_stream_t stream) {
  if (!x || !slot || !q) return SSSEG_EINVAL;
  if (P < 0 || C < 1 || ldx < C || C > 0x7fffffff - 16) return SSSEG_EINVAL;
  if (ldq != (C + 15) / 16 * 16 || ((uintptr_t)q & 15) != 0) return SSSEG_EINVAL;
  if (dt != SSSEG_F32 && dt != SSSEG_BF16 && dt != SSSEG_F16) return SSSEG_EUNSUPPORTED;
  if (P == 0) return SSSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  const int V = dt == SSSEG_F32 ? 4 : 8;
  const bool aligned = ldx % V == 0 && ((uintptr_t)x & 15) == 0;
  const int grid = ssseg_grid(P * (ldq / 16), Q_THREADS, Q_GRID_CAP);
  if (dt == SSSEG_F32)
    hipLaunchKernelGGL(quantize_kernel<float>, dim3(grid), dim3(Q_THREADS), 0, st, (const float*)x, P, (int)C, ldx,
                       aligned, slot, q, ldq);
  else if (dt == SSSEG_BF16)
    hipLaunchKernelGGL(quantize_kernel<bf16_t>, dim3(grid), dim3(Q_THREADS), 0, st, (const bf16_t*)x, P, (int)C, ldx,
                       aligned, slot, q, ldq);
  else
    hipLaunchKernelGGL(quantize_kernel<f16_t>, dim3(grid), dim3(Q_THREADS), 0, st, (const f16_t*)x, P, (int)C, ldx,
                       aligned, slot, q, ldq);
  SSSEG_LAUNCH_CHECK();
  return SSSEG_OK;
}

extern "C" int ssseg_weight_quant_i8(const float* w, int64_t K, int64_t C, int64_t R, int64_t S, int64_t Kp, int64_t Cq,
                                     int8_t* qw, float* sw, ssseg_stream_t stream) {
  if (!w || !qw || !sw) return SSSEG_EINVAL;
  if (K < 1 || C < 1 || R < 1 || S < 1 || Kp < K || Cq < C || Cq % 16 != 0) return SSSEG_EINVAL;
  if (!fits_int(Kp) || !fits_int(R * S * Cq) || !fits_int(C * R * S)) return SSSEG_EUNSUPPORTED;
  hipLaunchKernelGGL(weight_quant_kernel, dim3((unsigned)Kp), dim3(Q_THREADS), 0, (hipStream_t)stream, w, (int)K,
                     (int)C, (int)R, (int)S, (int)Cq, qw, sw);
  SSSEG_LAUNCH_CHECK();
  return SSSEG_OK;
}

extern "C" int ssseg_conv_i8_fwd(const int8_t* q, const int8_t* qw, void* y, const ssseg_conv_desc* d, int dt_out,
                                 const float* slot, const float* sw, const ssseg_conv_epilogue* epi,
                                 ssseg_stream_t stream) {
  if (!q || !qw || !y || !d || !slot || !sw) return SSSEG_EINVAL;
  if (epi && (epi->aux || epi->stats)) return SSSEG_EINVAL;
  if (dt_out != SSSEG_F32 && dt_out != SSSEG_BF16 && dt_out != SSSEG_F16) return SSSEG_EUNSUPPORTED;
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->OH < 1 || d->OW < 1) return SSSEG_EINVAL;
  // geometry the kernel covers: taps <= 7, stride 1 or 2, dense output map, 16-byte channel chunks, Cout in eights
  if (d->R < 1 || d->S < 1 || d->R > 7 || d->S > 7) return SSSEG_EUNSUPPORTED;
  if (d->sy < 1 || d->sy > 2 || d->sx < 1 || d->sx > 2 || d->dy < 1 || d->dx < 1) return SSSEG_EUNSUPPORTED;
  if (d->outH != d->OH || d->outW != d->OW || d->osy != 1 || d->osx != 1 || d->ooy != 0 || d->oox != 0)
    return SSSEG_EUNSUPPORTED;
  if (d->C < 16 || d->C % 16 != 0 || d->ldx < d->C || d->ldx % 16 != 0 || d->ldw != d->R * d->S * d->C)
    return SSSEG_EUNSUPPORTED;
  if (d->K < 8 || d->K % 8 != 0 || d->ldy < d->K || d->ldy % 4 != 0) return SSSEG_EUNSUPPORTED;
  if (epi && epi->residual && (epi->ldr < d->K || epi->ldr % 4 != 0)) return SSSEG_EUNSUPPORTED;
  if (epi && (epi->relu < SSSEG_ACT_NONE || epi->relu > SSSEG_ACT_LEAKY)) return SSSEG_EINVAL;
  const int esz = dt_out == SSSEG_F32 ? 4 : 2;
  if (((uintptr_t)q & 15) || ((uintptr_t)qw & 15) || ((uintptr_t)y % (4 * esz)) ||
      (epi && epi->residual && ((uintptr_t)epi->residual % (4 * esz))))
    return SSSEG_EUNSUPPORTED;
  const int64_t dims[] = {d->H, d->W, d->OH, d->OW, d->K, d->dy * (d->R - 1), d->dx * (d->S - 1), d->py, d->px,
                          d->OH * d->sy, d->OW * d->sx, d->ldw};
  for (int64_t v : dims)
    if (!fits_int(v) || v > (1 << 30) || v < -(1 << 30)) return SSSEG_EUNSUPPORTED;
  ConvI8 g;
  g.M = d->N * d->OH * d->OW;
  g.H = (int)d->H; g.W = (int)d->W; g.OH = (int)d->OH; g.OW = (int)d->OW;
  g.K = (int)d->K; g.Kp = (int)((d->K + 15) / 16 * 16);
  g.R = (int)d->R; g.S = (int)d->S; g.sy = (int)d->sy; g.sx = (int)d->sx; g.dy = (int)d->dy; g.dx = (int)d->dx;
  g.py = (int)d->py; g.px = (int)d->px;
  g.cpc = (int)(d->C / 16);
  g.nchunks = g.R * g.S * g.cpc;
  g.ldx = d->ldx; g.ldy = d->ldy; g.ldr = epi ? epi->ldr : 0;
  g.act = epi ? epi->relu : SSSEG_ACT_NONE;
  g.slope = epi ? epi->slope : 0.f;
  hipStream_t st = (hipStream_t)stream;
  if (dt_out == SSSEG_F32) return launch_conv<float>(q, qw, y, g, slot, sw, epi, st);
  if (dt_out == SSSEG_BF16) return launch_conv<bf16_t>(q, qw, y, g, slot, sw, epi, st);
  return launch_conv<f16_t>(q, qw, y, g, slot, sw, epi, st);
}
