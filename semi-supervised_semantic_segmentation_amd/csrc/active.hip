// Active-learning pool selection on the device: per-image uncertainty scores and a deterministic k-means.
// What the reference's get_active_learning_partition.py does per pool image (:94-99) and over the pool (:118-134),
// without its database, object store, cv2 and sklearn.
//
// ---- uncertainty scores ----
// x: contiguous fp32 [B,C,HW] logits, p = softmax_c(x).  Per image b, means over its HW pixels of
//   out[b,0] = -sum_c p_c log p_c       (entropy, :95)
//   out[b,1] = 1 - p1                   (least confidence; p1 >= p2 the two largest probabilities)
//   out[b,2] = 1 - (p1 - p2)            (margin; a shared maximum gives p2 = p1)
// DEVIATION from :95, on purpose: the entropy is log Z - sum_c p_c (x_c - m) with m = max_c x_c and
// Z = sum_c exp(x_c - m), never p * log(p).  A saturated pixel scores 0; the reference's expression gives
// 0 * -inf = NaN as soon as an fp32 softmax underflows.
// One read: a thread takes the channels of 4 neighbouring pixels through registers 8 at a time and folds them into a
// running (max, second max, Z, sum) state, rescaled when the maximum rises (online softmax); no probability is
// written.  Reduction: fp32 per-pixel terms, fp64 per-thread and per-block partials in the caller's workspace, one
// final block per image: no floating-point atomics, bitwise reproducible.  The blocks of an image and their summation
// order depend on HW only -- not on B, b or the alignment of x (the 16-byte loads and the scalar loads fill the same
// registers) -- so an image scores the same bits alone and inside any batch.
//
// ---- k-means ----
// X: fp32 [N,D]; every distance, sum and mean is fp64 on the fp32 data, in a fixed order, without atomics on
// floating-point values.  Seeding is k-means++ from caller-supplied uniforms; Lloyd iterations stop on the device
// (a `done` flag makes the remaining enqueued launches return at once), see include/ssseg.h for the rules.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// scores
// ------------------------------------------------------------------------------------------------
constexpr int ACT_THREADS = 256;      // threads of a scoring block
constexpr int ACT_MAX_BLOCKS = 256;   // blocks per image at the most (more pixels: every block loops)
constexpr int ACT_PX = 4;             // neighbouring pixels per thread: one 16-byte load per channel
constexpr int ACT_CHUNK = 8;          // channels in registers at a time (the buckets: C <= 2, C <= 4, then eights)

// blocks of one image: a function of HW only
int act_blocks(int64_t HW) {
  const int64_t per = (int64_t)ACT_THREADS * ACT_PX;
  const int64_t g = (HW + per - 1) / per;
  return (int)(g > ACT_MAX_BLOCKS ? ACT_MAX_BLOCKS : g);
}

// One thread scores ACT_PX neighbouring pixels.  The channels pass through registers CH at a time (all loads of a
// chunk issued before the first use) and fold into the running state of each pixel: m1 >= m2 the two largest logits
// so far (a second copy of the maximum lands in m2), z = sum exp(x - m1), t = sum exp(x - m1) (x - m1).  A chunk that
// raises the maximum by -dm rescales the state once: z' = s z, t' = s (t + dm z) with s = exp(dm) -- one extra exp per
// chunk and pixel, no logit read twice.  exp is the hardware's exp2 of x log2(e) (__expf): the argument is <= 0, its
// rounding costs |x| 2^-24 relative on a term of size exp(x), and exp(0) = 1, exp(-200) = 0 stay exact.
template <int CH>
__global__ void __launch_bounds__(ACT_THREADS) unc_partial_kernel(const float* __restrict__ x, int C, int64_t HW,
                                                                  int vec, double* __restrict__ part) {
  constexpr int PX = ACT_PX;
  __shared__ double red[ACT_THREADS / 64];
  const float* xb = x + (int64_t)blockIdx.y * C * HW;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  const int64_t ngroups = (HW + PX - 1) / PX;
  for (int64_t g = (int64_t)blockIdx.x * ACT_THREADS + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * ACT_THREADS) {
    const int64_t p0 = g * PX;
    const int np = HW - p0 < PX ? (int)(HW - p0) : PX;
    float m1[PX], m2[PX], z[PX], t[PX];
    for (int c0 = 0; c0 < C; c0 += CH) {
      float v[CH][PX];
      // channels past C re-read channel C - 1 (no branch around a load) and are left out below
      if (vec) {   // HW % 4 == 0 and x 16-byte aligned: every group is whole and every row aligned
        Chunk<float, 4>::raw r[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) r[i] = Chunk<float, 4>::ld(xb + (int64_t)min(c0 + i, C - 1) * HW + p0);
#pragma unroll
        for (int i = 0; i < CH; ++i) Chunk<float, 4>::cvt(r[i], v[i]);
      } else {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const float* row = xb + (int64_t)min(c0 + i, C - 1) * HW + p0;
#pragma unroll
          for (int j = 0; j < PX; ++j) v[i][j] = row[j < np ? j : 0];
        }
      }
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        float b1 = c0 ? m1[j] : -INFINITY, b2 = c0 ? m2[j] : -INFINITY;
#pragma unroll
        for (int i = 0; i < CH; ++i)
          if (c0 + i < C) {
            const float a = v[i][j];
            b2 = a > b1 ? b1 : fmaxf(b2, a);
            b1 = fmaxf(b1, a);
          }
        float zz = 0.f, tt = 0.f;
        if (c0) {
          const float dm = m1[j] - b1, s = __expf(dm);
          zz = z[j] * s;
          tt = (t[j] + dm * z[j]) * s;
        }
#pragma unroll
        for (int i = 0; i < CH; ++i)
          if (c0 + i < C) {
            const float d = v[i][j] - b1, e = __expf(d);
            zz += e;
            tt += e * d;
          }
        m1[j] = b1;
        m2[j] = b2;
        z[j] = zz;
        t[j] = tt;
      }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j)
      if (j < np) {
        const float inv = 1.f / z[j];
        a0 += (double)(logf(z[j]) - t[j] * inv);
        a1 += (double)(1.f - inv);
        a2 += (double)(1.f - (inv - __expf(m2[j] - m1[j]) * inv));
      }
  }
  a0 = block_sum(a0, red);
  a1 = block_sum(a1, red);
  a2 = block_sum(a2, red);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    p[0] = a0;
    p[1] = a1;
    p[2] = a2;
  }
}

// out[b, k] = (float)(sum over the image's blocks / HW); one block per image
__global__ void __launch_bounds__(ACT_THREADS) unc_final_kernel(const double* __restrict__ part, int nblk, int64_t HW,
                                                                float* __restrict__ out) {
  __shared__ double red[ACT_THREADS / 64];
  const double* p = part + (int64_t)blockIdx.x * nblk * 3;
  for (int k = 0; k < 3; ++k) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += ACT_THREADS) acc += p[i * 3 + k];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.x * 3 + k] = (float)(acc / (double)HW);
  }
}

bool unc_bad_shape(int64_t B, int64_t C, int64_t HW) {
  return B <= 0 || B > 65535 || C < 2 || C > 64 || HW <= 0 || HW >= ((int64_t)1 << 31);
}

// ------------------------------------------------------------------------------------------------
// k-means
// ------------------------------------------------------------------------------------------------
constexpr int KM_THREADS = 256;        // point kernels: one wave per point, 4 points per block
constexpr int KM_SCAN_THREADS = 1024;  // the single block of the seeding scan and of the final sums
constexpr int KM_UPD_SLICES = 16;      // row slices of an update block (x 64 columns = 1024 threads)
constexpr int KM_MAX_K = 64;

struct KmState {
  double thr;      // tol * mean_d Var(X[:, d])
  double shift;    // squared centroid shift of the last iteration, summed over clusters
  int done;
  int n_iter;
};

struct KmWs {
  KmState* st;
  double* d2;      // [N] squared distance to the nearest centre
  double* next;    // [K, D] centroids of the running update
  double* colvar;  // [D] population variance per column
};

size_t km_align(size_t n) { return (n + 255) & ~(size_t)255; }
size_t km_ws_bytes(int64_t N, int64_t D, int64_t K) {
  return km_align(sizeof(KmState)) + km_align(sizeof(double) * (size_t)N) + km_align(sizeof(double) * (size_t)(K * D)) +
         km_align(sizeof(double) * (size_t)D);
}
KmWs km_carve(void* ws, int64_t N, int64_t D, int64_t K) {
  char* p = (char*)ws;
  KmWs w;
  w.st = (KmState*)p;
  p += km_align(sizeof(KmState));
  w.d2 = (double*)p;
  p += km_align(sizeof(double) * (size_t)N);
  w.next = (double*)p;
  p += km_align(sizeof(double) * (size_t)(K * D));
  w.colvar = (double*)p;
  return w;
}

// fp64 squared distance of row x to the fp32 row c / the fp64 row c.  The order is part of the contract (ssseg.h): lane
// l adds the squares of d = l, l + 64, ... in that order, every product and sum rounded on its own (contraction is
// switched off by pragma over plain operators: __dmul_rn / __dadd_rn do not prevent an FMA in HIP),
// then the 64 lanes are summed by the xor butterfly with offsets 32, 16, ..., 1.
__device__ __forceinline__ double wave_dist(const float* x, const float* c, int64_t D, int lane) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int64_t d = lane; d < D; d += 64) {
    const double t = (double)x[d] - (double)c[d];
    const double sq = t * t;
    acc = acc + sq;
  }
  return wave_sum(acc);
}
__device__ __forceinline__ double wave_dist(const float* x, const double* c, int64_t D, int lane) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int64_t d = lane; d < D; d += 64) {
    const double t = (double)x[d] - c[d];
    const double sq = t * t;
    acc = acc + sq;
  }
  return wave_sum(acc);
}

// seed_idx[0] = min(floor(u[0] * N), N - 1)
__global__ void km_seed_first_kernel(const float* u, int64_t N, int* seed_idx) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int64_t i = (int64_t)floor((double)u[0] * (double)N);
    if (i > N - 1) i = N - 1;
    if (i < 0) i = 0;
    seed_idx[0] = (int)i;
  }
}

// d2[i] = min(d2[i], |x_i - x_seed[j-1]|^2)  (first == 1: no previous value)
__global__ void __launch_bounds__(KM_THREADS) km_seed_dist_kernel(const float* __restrict__ X, int64_t N, int64_t D,
                                                                  const int* __restrict__ seed_idx, int j, int first,
                                                                  double* __restrict__ d2) {
  const int lane = threadIdx.x & 63;
  const float* c = X + (int64_t)seed_idx[j - 1] * D;
  for (int64_t i = (int64_t)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6); i < N;
       i += (int64_t)gridDim.x * (KM_THREADS / 64)) {
    const double d = wave_dist(X + i * D, c, D, lane);
    if (lane == 0) d2[i] = first ? d : fmin(d2[i], d);
  }
}

// One block.  Thread t owns the contiguous slice [t * per, (t + 1) * per) of v[0..N).  Returns, in every thread, the
// exclusive prefix of the thread's slice (sums in slice order, prefixes in thread order) and the total in *total.
__device__ __forceinline__ double km_block_prefix(const double* v, int64_t N, int64_t per, double* sh, double* total) {
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < N ? lo + per : N;
  double s = 0.0;
  for (int64_t i = lo; i < hi; ++i) s += v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int t = 0; t < KM_SCAN_THREADS; ++t) {
      const double a = sh[t];
      sh[t] = run;
      run += a;
    }
    sh[KM_SCAN_THREADS] = run;
  }
  __syncthreads();
  *total = sh[KM_SCAN_THREADS];
  return sh[threadIdx.x];
}

// seed_idx[j] = the first i, in index order, whose inclusive cumulative sum of d2 exceeds u[j] * sum(d2); N - 1 when
// none does (a total of 0, or a threshold that rounding puts at the total)
__global__ void __launch_bounds__(KM_SCAN_THREADS) km_seed_pick_kernel(const double* __restrict__ d2, int64_t N,
                                                                       const float* __restrict__ u, int j,
                                                                       int* __restrict__ seed_idx) {
  __shared__ double sh[KM_SCAN_THREADS + 1];
  __shared__ int best;
  if (threadIdx.x == 0) best = (int)(N - 1);
  const int64_t per = (N + KM_SCAN_THREADS - 1) / KM_SCAN_THREADS;
  double total;
  double run = km_block_prefix(d2, N, per, sh, &total);
  const double thr = (double)u[j] * total;
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < N ? lo + per : N;
  for (int64_t i = lo; i < hi; ++i) {
    run += d2[i];
    if (run > thr) {
      atomicMin(&best, (int)i);
      break;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) seed_idx[j] = best;
}

// centroids[k, :] = X[seed_idx[k], :]
__global__ void km_seed_gather_kernel(const float* __restrict__ X, int64_t D, const int* __restrict__ seed_idx,
                                      double* __restrict__ cent) {
  const float* r = X + (int64_t)seed_idx[blockIdx.x] * D;
  for (int64_t d = threadIdx.x; d < D; d += blockDim.x) cent[(int64_t)blockIdx.x * D + d] = (double)r[d];
}

// population variance of 64 columns per block: threads (col, slice), two passes, slices combined in slice order
__global__ void __launch_bounds__(64 * KM_UPD_SLICES) km_colvar_kernel(const float* __restrict__ X, int64_t N,
                                                                       int64_t D, double* __restrict__ colvar) {
  __shared__ double sh[KM_UPD_SLICES][64];
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int64_t d = (int64_t)blockIdx.x * 64 + col;
  double s = 0.0;
  if (d < D)
    for (int64_t i = sl; i < N; i += KM_UPD_SLICES) s += (double)X[i * D + d];
  sh[sl][col] = s;
  __syncthreads();
  double mean = 0.0;
  for (int t = 0; t < KM_UPD_SLICES; ++t) mean += sh[t][col];
  mean /= (double)N;
  __syncthreads();
  s = 0.0;
  if (d < D)
    for (int64_t i = sl; i < N; i += KM_UPD_SLICES) {
      const double t = (double)X[i * D + d] - mean;
      s += t * t;
    }
  sh[sl][col] = s;
  __syncthreads();
  if (sl == 0 && d < D) {
    double v = 0.0;
    for (int t = 0; t < KM_UPD_SLICES; ++t) v += sh[t][col];
    colvar[d] = v / (double)N;
  }
}

// st = {thr = tol * mean(colvar), shift = 0, done = 0, n_iter = 0}
__global__ void __launch_bounds__(KM_SCAN_THREADS) km_init_kernel(const double* __restrict__ colvar, int64_t D,
                                                                  double tol, KmState* st) {
  __shared__ double sh[KM_SCAN_THREADS + 1];
  double total;
  km_block_prefix(colvar, D, (D + KM_SCAN_THREADS - 1) / KM_SCAN_THREADS, sh, &total);
  if (threadIdx.x == 0) {
    st->thr = tol * (total / (double)D);
    st->shift = 0.0;
    st->done = 0;
    st->n_iter = 0;
  }
}

// labels[i] = argmin_k |x_i - c_k|^2 (the lowest k wins an exact tie), d2[i] = that distance.  force == 0: a no-op once
// the fit is done.
__global__ void __launch_bounds__(KM_THREADS) km_assign_kernel(const float* __restrict__ X, int64_t N, int64_t D,
                                                               int K, const double* __restrict__ cent,
                                                               const KmState* st, int force, int* __restrict__ labels,
                                                               double* __restrict__ d2) {
  if (!force && st->done) return;
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6); i < N;
       i += (int64_t)gridDim.x * (KM_THREADS / 64)) {
    const float* x = X + i * D;
    double best = wave_dist(x, cent, D, lane);
    int bk = 0;
    for (int k = 1; k < K; ++k) {
      const double d = wave_dist(x, cent + (int64_t)k * D, D, lane);
      if (d < best) {
        best = d;
        bk = k;
      }
    }
    if (lane == 0) {
      labels[i] = bk;
      d2[i] = best;
    }
  }
}

// next[k, d] = mean over the points of cluster k, rows in index order inside a slice and slices in slice order;
// a cluster without points keeps cent[k, d].  grid (ceil(D / 64), K).
__global__ void __launch_bounds__(64 * KM_UPD_SLICES) km_update_kernel(const float* __restrict__ X, int64_t N,
                                                                       int64_t D, const int* __restrict__ labels,
                                                                       const double* __restrict__ cent,
                                                                       const KmState* st, double* __restrict__ next) {
  if (st->done) return;
  __shared__ double sh[KM_UPD_SLICES][64];
  __shared__ int cnt[KM_UPD_SLICES];
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6, k = blockIdx.y;
  const int64_t d = (int64_t)blockIdx.x * 64 + col;
  const int64_t per = (N + KM_UPD_SLICES - 1) / KM_UPD_SLICES;
  const int64_t lo = sl * per, hi = lo + per < N ? lo + per : N;
  double s = 0.0;
  int n = 0;
  for (int64_t i = lo; i < hi; ++i)
    if (labels[i] == k) {
      ++n;
      if (d < D) s += (double)X[i * D + d];
    }
  sh[sl][col] = s;
  if (col == 0) cnt[sl] = n;
  __syncthreads();
  if (sl == 0 && d < D) {
    double v = 0.0;
    int64_t m = 0;
    for (int t = 0; t < KM_UPD_SLICES; ++t) {
      v += sh[t][col];
      m += cnt[t];
    }
    next[(int64_t)k * D + d] = m > 0 ? v / (double)m : cent[(int64_t)k * D + d];
  }
}

// shift = sum (next - cent)^2 in a fixed order; cent = next; n_iter += 1; done = shift <= thr
__global__ void __launch_bounds__(KM_SCAN_THREADS) km_shift_kernel(double* __restrict__ cent,
                                                                   const double* __restrict__ next, int64_t KD,
                                                                   KmState* st) {
  if (st->done) return;
  __shared__ double red[KM_SCAN_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < KD; i += KM_SCAN_THREADS) {
    const double t = next[i] - cent[i];
    acc += t * t;
    cent[i] = next[i];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) {
    st->shift = acc;
    st->n_iter += 1;
    if (acc <= st->thr) st->done = 1;
  }
}

// inertia = sum d2 (slice sums in thread order), n_iter out
__global__ void __launch_bounds__(KM_SCAN_THREADS) km_finish_kernel(const double* __restrict__ d2, int64_t N,
                                                                    const KmState* st, double* inertia, int* n_iter) {
  __shared__ double sh[KM_SCAN_THREADS + 1];
  double total;
  km_block_prefix(d2, N, (N + KM_SCAN_THREADS - 1) / KM_SCAN_THREADS, sh, &total);
  if (threadIdx.x == 0) {
    inertia[0] = total;
    n_iter[0] = st->n_iter;
  }
}

bool km_bad_shape(int64_t N, int64_t D, int64_t K) {
  return N <= 0 || N >= ((int64_t)1 << 31) || D <= 0 || D >= ((int64_t)1 << 31) || K < 1 || K > KM_MAX_K || K > N;
}
int km_point_grid(int64_t N) { return ssseg_grid(N, KM_THREADS / 64); }

}  // namespace

// launch KERNEL<CH> with CH channels in registers at a time: the whole pixel for C <= 2 and C <= 4, else eights
#define ACT_LAUNCH_C(KERNEL, C, grid, block, stream, ...)                                        \
  do {                                                                                           \
    if ((C) <= 2) hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, stream, __VA_ARGS__);          \
    else if ((C) <= 4) hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, stream, __VA_ARGS__);     \
    else hipLaunchKernelGGL((KERNEL<ACT_CHUNK>), grid, block, 0, stream, __VA_ARGS__);           \
  } while (0)

extern "C" size_t ssseg_uncertainty_workspace_bytes(int64_t B, int64_t C, int64_t HW) {
  if (unc_bad_shape(B, C, HW)) return 0;
  return sizeof(double) * 3 * (size_t)B * (size_t)act_blocks(HW);
}

extern "C" int ssseg_uncertainty_scores(const float* x, int64_t B, int64_t C, int64_t HW, float* out, void* ws,
                                        size_t ws_bytes, ssseg_stream_t stream) {
  if (!x || !out || unc_bad_shape(B, C, HW)) return SSSEG_EINVAL;
  if (!ws || ws_bytes < ssseg_uncertainty_workspace_bytes(B, C, HW)) return SSSEG_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = act_blocks(HW);
  // the wide loads need whole groups and aligned rows; the registers they fill are the scalar loads' registers
  const int vec = HW % ACT_PX == 0 && ((uintptr_t)x % (sizeof(float) * ACT_PX)) == 0;
  double* part = (double*)ws;
  ACT_LAUNCH_C(unc_partial_kernel, C, dim3(nblk, (unsigned)B), dim3(ACT_THREADS), s, x, (int)C, HW, vec, part);
  hipLaunchKernelGGL(unc_final_kernel, dim3((unsigned)B), dim3(ACT_THREADS), 0, s, (const double*)part, nblk, HW, out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t ssseg_kmeans_workspace_bytes(int64_t N, int64_t D, int64_t K) {
  if (km_bad_shape(N, D, K)) return 0;
  return km_ws_bytes(N, D, K);
}

extern "C" int ssseg_kmeans_seed(const float* X, int64_t N, int64_t D, int64_t K, const float* u, int* seed_idx,
                                 double* centroids, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!X || !u || !seed_idx || !centroids || km_bad_shape(N, D, K)) return SSSEG_EINVAL;
  if (!ws || ws_bytes < km_ws_bytes(N, D, K)) return SSSEG_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const KmWs w = km_carve(ws, N, D, K);
  hipLaunchKernelGGL(km_seed_first_kernel, dim3(1), dim3(64), 0, s, u, N, seed_idx);
  for (int j = 1; j < (int)K; ++j) {
    hipLaunchKernelGGL(km_seed_dist_kernel, dim3(km_point_grid(N)), dim3(KM_THREADS), 0, s, X, N, D,
                       (const int*)seed_idx, j, j == 1 ? 1 : 0, w.d2);
    hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(KM_SCAN_THREADS), 0, s, (const double*)w.d2, N, u, j,
                       seed_idx);
  }
  hipLaunchKernelGGL(km_seed_gather_kernel, dim3((unsigned)K), dim3(256), 0, s, X, D, (const int*)seed_idx, centroids);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_kmeans_fit(const float* X, int64_t N, int64_t D, int64_t K, double tol, int64_t max_iter,
                                double* centroids, int* labels, double* inertia, int* n_iter, void* ws,
                                size_t ws_bytes, ssseg_stream_t stream) {
  if (!X || !centroids || !labels || !inertia || !n_iter || km_bad_shape(N, D, K) || !(tol >= 0.0) || max_iter < 1 ||
      max_iter > 100000)
    return SSSEG_EINVAL;
  if (!ws || ws_bytes < km_ws_bytes(N, D, K)) return SSSEG_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const KmWs w = km_carve(ws, N, D, K);
  const unsigned tiles = (unsigned)((D + 63) / 64);
  hipLaunchKernelGGL(km_colvar_kernel, dim3(tiles), dim3(64 * KM_UPD_SLICES), 0, s, X, N, D, w.colvar);
  hipLaunchKernelGGL(km_init_kernel, dim3(1), dim3(KM_SCAN_THREADS), 0, s, (const double*)w.colvar, D, tol, w.st);
  for (int64_t it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(km_assign_kernel, dim3(km_point_grid(N)), dim3(KM_THREADS), 0, s, X, N, D, (int)K,
                       (const double*)centroids, (const KmState*)w.st, 0, labels, w.d2);
    hipLaunchKernelGGL(km_update_kernel, dim3(tiles, (unsigned)K), dim3(64 * KM_UPD_SLICES), 0, s, X, N, D,
                       (const int*)labels, (const double*)centroids, (const KmState*)w.st, w.next);
    hipLaunchKernelGGL(km_shift_kernel, dim3(1), dim3(KM_SCAN_THREADS), 0, s, centroids, (const double*)w.next, K * D,
                       w.st);
  }
  // labels and inertia of the returned centroids
  hipLaunchKernelGGL(km_assign_kernel, dim3(km_point_grid(N)), dim3(KM_THREADS), 0, s, X, N, D, (int)K,
                     (const double*)centroids, (const KmState*)w.st, 1, labels, w.d2);
  hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(KM_SCAN_THREADS), 0, s, (const double*)w.d2, N,
                     (const KmState*)w.st, inertia, n_iter);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
