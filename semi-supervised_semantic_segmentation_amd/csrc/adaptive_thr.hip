// Self-adaptive per-class confidence thresholds of the pseudo-label consistency loss (FreeMatch: Wang et al., ICLR 2023,
// section 3.2, eqs. 5-8).  The state -- tau, ptilde[C] and a step counter, fp64 -- lives on the device and is updated
// in the step (graph-capturable like the optimizers' step counters):
//   p = softmax_c(t) per pixel (fp32, expf, maximum subtracted),
//   m = mean_pix max_c p,  q_c = mean_pix p_c                       (over all B HW pixels, no weight map),
//   tau <- lam tau + (1 - lam) m,  ptilde_c <- lam ptilde_c + (1 - lam) q_c,
//   thr_c = (float)((ptilde_c / max_k ptilde_k) tau)                (fp64, in this order, one rounding).
// Conventions of multiclass.hip: contiguous fp32 [B,C,HW], the same tile walk (256 pixels of one sample per tile,
// grid-strided, at most 1024 workgroups), per-workgroup fp64 partials and one final block in the caller's workspace,
// no floating-point atomics, no allocation, no synchronisation.  This unit is compiled with -ffp-contract=off: the
// EMA's products and sums round one by one, as the rule is written.
#include "common.h"

namespace {

constexpr int AT_BLOCKS = 1024;     // partial rows in the workspace
constexpr int AT_TILE = 256;        // pixels of one sample per workgroup round: one pixel per thread
constexpr int AT_FINAL_THREADS = 1024;   // 16 waves: one slot of the partial rows each, at most 5 rounds at C = 64
constexpr int AT_MAX_C = 64;

// Each thread owns one pixel of the tile and holds its CMAX logits in registers (every load issued before the first
// use, clamped addresses, channel stride HW: coalesced across the wave), so t comes from memory exactly once.  The
// C + 1 sums are per-thread fp64 accumulators over the thread's own tiles (CMAX is the channel bucket, the loops are
// unrolled: they never leave registers); the workgroup folds them once, after its last tile, through wave reductions
// and a [CMAX + 1][4] LDS table.  Slot 0 of a partial row is sum max_c p, slot 1 + c is sum p_c; the workspace is laid
// out slot-major (part[slot * AT_BLOCKS + workgroup]) so that the final block reads each slot contiguously.
template <int CMAX>
__global__ void __launch_bounds__(AT_TILE) adaptive_thr_partial_kernel(const float* __restrict__ t, int C, int64_t HW,
                                                                       int64_t tiles_per_sample, int64_t ntiles,
                                                                       double* __restrict__ part) {
  __shared__ double red[CMAX + 1][AT_TILE / 64];
  double acc[CMAX], accm = 0.0;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) acc[c] = 0.0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b = tile / tiles_per_sample;
    const int64_t pix = (tile - b * tiles_per_sample) * AT_TILE + threadIdx.x;
    if (pix < HW) {
      const float* tp = t + b * C * HW + pix;
      float p[CMAX];
#pragma unroll
      for (int c = 0; c < CMAX; ++c) p[c] = tp[(int64_t)(c < C ? c : 0) * HW];
      float m = p[0];
#pragma unroll
      for (int c = 1; c < CMAX; ++c)
        if (c < C) m = fmaxf(m, p[c]);
      float z = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        p[c] = c < C ? expf(p[c] - m) : 0.f;
        z += p[c];
      }
      // max_c p = exp(0) / z: the confidence of the loss kernels (multiclass.hip), from the same expression
      const float conf = 1.f / z;
      accm += (double)conf;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) acc[c] += (double)(p[c] * conf);
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  accm = wave_sum(accm);
  if (lane == 0) red[0][wid] = accm;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    if (c < C) {   // uniform over the workgroup
      const double v = wave_sum(acc[c]);
      if (lane == 0) red[1 + c][wid] = v;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x <= C) {
    double v = 0.0;
    for (int i = 0; i < AT_TILE / 64; ++i) v += red[threadIdx.x][i];
    part[(int64_t)threadIdx.x * AT_BLOCKS + blockIdx.x] = v;
  }
}

// One block: wave k mod 16 folds slot k over the partial rows (a fixed order: bitwise reproducible), then one thread
// performs the EMA and writes the thresholds.  state: [0] tau, [1, C] ptilde, [C + 1] steps taken, [C + 2] this step's
// m, [C + 3, 2C + 2] this step's q_c (the last two for logs and tests; the rule does not read them).
__global__ void __launch_bounds__(AT_FINAL_THREADS) adaptive_thr_final_kernel(const double* __restrict__ part,
                                                                              int nparts, int C, double npix,
                                                                              double lam, double* __restrict__ state,
                                                                              float* __restrict__ thr_c) {
  __shared__ double sums[AT_MAX_C + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int k = wid; k <= C; k += AT_FINAL_THREADS / 64) {
    // the lane's AT_BLOCKS / 64 rows of the slot, every load issued before the first add (a loop of dependent
    // load-add steps was a sixth of the update's time at 19 classes)
    double r[AT_BLOCKS / 64];
#pragma unroll
    for (int j = 0; j < AT_BLOCKS / 64; ++j) {
      const int i = lane + 64 * j;
      r[j] = part[(int64_t)k * AT_BLOCKS + (i < nparts ? i : 0)];
    }
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < AT_BLOCKS / 64; ++j) v += lane + 64 * j < nparts ? r[j] : 0.0;
    v = wave_sum(v);
    if (lane == 0) sums[k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double keep = 1.0 - lam;
    const double m = sums[0] / npix;
    const double tau = lam * state[0] + keep * m;
    state[0] = tau;
    double pmax = 0.0;
    for (int c = 0; c < C; ++c) {
      const double q = sums[1 + c] / npix;
      const double pt = lam * state[1 + c] + keep * q;
      state[1 + c] = pt;
      state[C + 3 + c] = q;
      // torch.max's rule: a NaN is the maximum and stays it
      pmax = (c == 0 || pt > pmax || pt != pt) ? pt : pmax;
    }
    state[C + 1] += 1.0;
    state[C + 2] = m;
    for (int c = 0; c < C; ++c) thr_c[c] = (float)((state[1 + c] / pmax) * tau);
  }
}

template <int CMAX>
void launch_partial(int nb, hipStream_t st, const float* t, int C, int64_t HW, int64_t tps, int64_t ntiles,
                    double* part) {
  hipLaunchKernelGGL(adaptive_thr_partial_kernel<CMAX>, dim3(nb), dim3(AT_TILE), 0, st, t, C, HW, tps, ntiles, part);
}

}  // namespace

extern "C" size_t ssseg_adaptive_thr_workspace_bytes(int64_t C) {
  return C >= 1 && C <= AT_MAX_C ? sizeof(double) * (size_t)(C + 1) * AT_BLOCKS : 0;
}

extern "C" int ssseg_adaptive_thr_update(const float* t, int64_t B, int64_t C, int64_t HW, double momentum,
                                         double* state, float* thr_c, void* ws, size_t ws_bytes,
                                         ssseg_stream_t stream) {
  if (!t || !state || !thr_c || B <= 0 || C <= 0 || C > AT_MAX_C || HW <= 0) return SSSEG_EINVAL;
  if (!(momentum >= 0.0 && momentum < 1.0)) return SSSEG_EINVAL;   // a NaN too
  // the element count and the tile count stay far inside int64
  if (B > (INT64_MAX / 64) / HW / 64) return SSSEG_EINVAL;
  if (!ws || ws_bytes < ssseg_adaptive_thr_workspace_bytes(C)) return SSSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tps = (HW + AT_TILE - 1) / AT_TILE, ntiles = B * tps;
  const int nb = (int)(ntiles < AT_BLOCKS ? ntiles : AT_BLOCKS);
#define AT_PARTIAL(N) launch_partial<N>(nb, st, t, (int)C, HW, tps, ntiles, (double*)ws)
  // the channel bucket of C: the smallest of 2, 4, 8, 16, 32, 64 that holds it
  if (C <= 2) AT_PARTIAL(2);
  else if (C <= 4) AT_PARTIAL(4);
  else if (C <= 8) AT_PARTIAL(8);
  else if (C <= 16) AT_PARTIAL(16);
  else if (C <= 32) AT_PARTIAL(32);
  else AT_PARTIAL(64);
#undef AT_PARTIAL
  hipLaunchKernelGGL(adaptive_thr_final_kernel, dim3(1), dim3(AT_FINAL_THREADS), 0, st, (const double*)ws, nb, (int)C,
                     (double)(B * HW), momentum, state, thr_c);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
