// Binary Lovász-softmax on the device (losses.binary_lovasz_loss_with_logits losses.py:239-250 ->
// lovasz.lovasz_softmax lovasz.py:155-201 with classes=[1], per_image=True; lovasz_grad lovasz.py:19-31).
//
// Per image b (a segment of HW pixels):
//   label = argmax_c target[b][c][p] (first max),  fg = [label == 1],  e = |fg - logit[b][1][p]|
//   sort e descending (stable: ties keep pixel order; the reference's torch.sort is unstable, the loss
//   is invariant to the order inside a tie), F(i) = #fg among the first i+1 sorted pixels,
//   J(i) = 1 - (gts - F(i)) / (gts + (i+1) - F(i)),  g(i) = J(i) - J(i-1) (g(0) = J(0)),  loss_b = <e, g>
//   loss = sum_b loss_b * valid_b / (sum_b valid_b + 0.001), valid_b = [gts_b > 0]
//   d loss / d logit[b][1][p] = -sign(fg - x) * g(rank(p)) * valid_b / denom  (other channels 0)
//
// The sort is an LSD radix sort over all segments at once: 4 passes of 8-bit digits on the key
// ~bits(e) (ascending key = descending e; e >= 0 so float bits are monotone), values = pixel index | fg<<31.
// Each pass: per-(segment, tile) digit histograms -> per-segment exclusive scan in (digit, tile) order
// -> stable scatter (rank inside a tile from wave ballots + per-(slot, wave) digit counts).
// Then a tile scan of fg in sorted order gives F(i); J/g follow in fp32 exactly as lovasz_grad computes
// them; the dot accumulates in fp64.  Deterministic; no atomics on data.
//
// The second half of the file is the general family on the same sort (multi-class softmax / sigmoid, hinge, 'present',
// batch-wide groups, ignore label: ssseg_lovasz_gen_*); its header comment states the key mapping, the class chunking
// rule, the peak workspace and the bounds.
#include "common.h"

namespace {

constexpr int LT = 256;              // threads per block
constexpr int ITEMS = 8;             // elements per thread per tile
constexpr int TILE = LT * ITEMS;     // 2048
constexpr int NW = LT / 64;

__device__ __forceinline__ unsigned long long lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// keys / values from the inputs
__global__ void lovasz_prep_kernel(const float* __restrict__ logits, const float* __restrict__ target, int64_t B,
                                   int C, int64_t HW, unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
  const int64_t n = B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, p = i - b * HW;
    const float* tb = target + b * C * HW + p;
    int lab = 0;
    float best = tb[0];
    for (int c = 1; c < C; ++c) {
      const float v = tb[(int64_t)c * HW];
      if (v > best) {   // torch.argmax: first maximal index
        best = v;
        lab = c;
      }
    }
    const unsigned fg = lab == 1;
    const float x = logits[b * C * HW + HW + p];
    const float e = fabsf((float)fg - x);
    keys[i] = ~__float_as_uint(e);
    vals[i] = (unsigned)p | (fg << 31);
  }
}

// hist[b][d][t] = count of digit d in tile t of segment b; dtot[b][d] += that count (integer atomics: exact, so the
// totals do not depend on the order of the adds; dtot zeroed before the pass)
__global__ void __launch_bounds__(LT) radix_hist_kernel(const unsigned* __restrict__ keys, int64_t HW, int T, int shift,
                                                        unsigned* __restrict__ hist, unsigned* __restrict__ dtot) {
  __shared__ unsigned cnt[256];
  const int b = blockIdx.y, t = blockIdx.x;
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* kb = keys + (int64_t)b * HW;
  const int64_t base = (int64_t)t * TILE;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + s * LT + threadIdx.x;
    if (i < HW) atomicAdd(&cnt[(kb[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  const unsigned c = cnt[threadIdx.x];
  hist[((int64_t)b * 256 + threadIdx.x) * T + t] = c;
  if (c) atomicAdd(&dtot[b * 256 + threadIdx.x], c);
}

// per segment: exclusive scan of hist[b] (digit-major) in place, one wave per (segment, digit) row: the row's base is
// the sum of the earlier digits' totals (dtot), then a carried wave scan along the T tiles.  (One 1024-thread block
// per segment walking 32 entries per thread in sequence took 52 us per pass at 16 x 512^2: a chain of dependent
// loads in 16 blocks.)
__global__ void __launch_bounds__(256) seg_rowscan_kernel(unsigned* __restrict__ hist, const unsigned* __restrict__ dtot,
                                                          int T) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y, d = blockIdx.x * 4 + (threadIdx.x >> 6);
  const unsigned* tb = dtot + b * 256;
  unsigned base = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int dd = lane * 4 + k;
    base += dd < d ? tb[dd] : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) base += __shfl_xor(base, o, 64);
  unsigned* row = hist + ((int64_t)b * 256 + d) * T;
  unsigned carry = base;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const unsigned v = t < T ? row[t] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (t < T) row[t] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
}

// stable scatter of one pass
__global__ void __launch_bounds__(LT) radix_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                           unsigned* __restrict__ kout, unsigned* __restrict__ vout,
                                                           int64_t HW, int T, int shift, const unsigned* __restrict__ off) {
  __shared__ unsigned cnt[ITEMS * NW][256];   // per (slot, wave) digit counts -> exclusive bases
  const int b = blockIdx.y, t = blockIdx.x;
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < ITEMS * NW * 256; i += LT) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int64_t seg = (int64_t)b * HW, base = (int64_t)t * TILE;
  unsigned key[ITEMS], val[ITEMS], dig[ITEMS], lrank[ITEMS];
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + s * LT + threadIdx.x;
    const bool ok = i < HW;
    key[s] = ok ? kin[seg + i] : 0u;
    val[s] = ok ? vin[seg + i] : 0u;
    dig[s] = ok ? (key[s] >> shift) & 255u : 256u;
    // lanes of this wave with the same digit: AND of 9 ballots (bit 8 separates the invalid sentinel)
    unsigned long long m = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 9; ++bit) {
      const unsigned long long bb = __ballot((dig[s] >> bit) & 1u);
      m &= ((dig[s] >> bit) & 1u) ? bb : ~bb;
    }
    lrank[s] = (unsigned)__popcll(m & lanemask_lt());
    if (ok && lrank[s] == 0) cnt[s * NW + wave][dig[s]] = (unsigned)__popcll(m);
  }
  __syncthreads();
  // exclusive scan over (slot, wave) per digit; thread = digit
  {
    const int d = threadIdx.x;
    unsigned run = off[((int64_t)b * 256 + d) * T + t];
    for (int q = 0; q < ITEMS * NW; ++q) {
      const unsigned v = cnt[q][d];
      cnt[q][d] = run;
      run += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    if (dig[s] > 255u) continue;
    const unsigned pos = cnt[s * NW + wave][dig[s]] + lrank[s];
    kout[seg + pos] = key[s];
    vout[seg + pos] = val[s];
  }
}

// fg count per (segment, tile) of the sorted order
__global__ void __launch_bounds__(LT) fg_count_kernel(const unsigned* __restrict__ vals, int64_t HW, int T,
                                                      unsigned* __restrict__ tile_fg) {
  __shared__ unsigned red[NW];
  const int b = blockIdx.y, t = blockIdx.x;
  const int64_t seg = (int64_t)b * HW, base = (int64_t)t * TILE;
  unsigned c = 0;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + s * LT + threadIdx.x;
    if (i < HW) c += vals[seg + i] >> 31;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
    for (int w = 0; w < NW; ++w) tot += red[w];
    tile_fg[(int64_t)b * (T + 1) + t] = tot;
  }
}

// per segment: exclusive scan of tile_fg[b][0..T) and gts into tile_fg[b][T]
__global__ void fg_scan_kernel(unsigned* __restrict__ tile_fg, int T) {
  unsigned* d = tile_fg + (int64_t)blockIdx.x * (T + 1);
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int i = 0; i < T; ++i) {
      const unsigned v = d[i];
      d[i] = run;
      run += v;
    }
    d[T] = run;
  }
}

__device__ __forceinline__ float jac(float gts, float F, float k1) {   // k1 = i + 1
  return 1.f - (gts - F) / (gts + (k1 - F));
}

// Lovász gradient in sorted order, scattered back to pixels (gpix[b][p]); fp64 partial dots per tile
__global__ void __launch_bounds__(LT) lovasz_grad_kernel(const unsigned* __restrict__ keys,
                                                         const unsigned* __restrict__ vals, int64_t HW, int T,
                                                         const unsigned* __restrict__ tile_fg,
                                                         float* __restrict__ gpix, double* __restrict__ dots) {
  __shared__ unsigned wsum[NW];
  __shared__ double dred[NW];
  const int b = blockIdx.y, t = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t seg = (int64_t)b * HW, base = (int64_t)t * TILE;
  const unsigned* tf = tile_fg + (int64_t)b * (T + 1);
  const float gts = (float)tf[T];
  // this thread owns ITEMS consecutive sorted positions: i = base + threadIdx.x*ITEMS + s
  unsigned fg[ITEMS], v[ITEMS];
  unsigned mine = 0;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + (int64_t)threadIdx.x * ITEMS + s;
    v[s] = i < HW ? vals[seg + i] : 0u;
    fg[s] = v[s] >> 31;
    mine += fg[s];
  }
  // block exclusive scan of per-thread fg counts
  unsigned incl = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned wbase = 0;
  for (int w = 0; w < wave; ++w) wbase += wsum[w];
  unsigned F = tf[t] + wbase + incl - mine;   // fg count before this thread's first item
  double dot = 0.0;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + (int64_t)threadIdx.x * ITEMS + s;
    if (i >= HW) break;
    const float Fprev = (float)F;
    F += fg[s];
    float g = jac(gts, (float)F, (float)(i + 1));
    if (i > 0) g = g - jac(gts, Fprev, (float)i);
    const float e = __uint_as_float(~keys[seg + i]);
    dot += (double)e * (double)g;
    gpix[seg + (v[s] & 0x7fffffffu)] = g;
  }
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
  if (lane == 0) dred[wave] = dot;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += dred[w];
    dots[(int64_t)b * T + t] = s;
  }
}

// loss and the per-image scale valid_b / denom (kept in ws for the gradient).  One wave per image sums its T tile
// dots (lane-strided, then a fixed xor tree: deterministic); lane 0 of block thread 0 combines the B images in order.
// (A single thread walking all B*T dots was a chain of dependent loads: 122 us at B=16, T=128.)
constexpr int FIN_T = 1024;
__global__ void __launch_bounds__(FIN_T) lovasz_final_kernel(const double* __restrict__ dots,
                                                             const unsigned* __restrict__ tile_fg, int B, int T,
                                                             float* __restrict__ loss_out, float* __restrict__ wscale) {
  extern __shared__ double img_dot[];   // [B] dots, then [B] valid flags
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = FIN_T / 64;
  for (int b = wv; b < B; b += nw) {
    double s = 0.0;
    for (int t = lane; t < T; t += 64) s += dots[(int64_t)b * T + t];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
      img_dot[b] = s;
      img_dot[B + b] = tile_fg[(int64_t)b * (T + 1) + T] > 0 ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float nvalid = 0.f;
  for (int b = 0; b < B; ++b) nvalid += (float)img_dot[B + b];
  const float denom = nvalid + 0.001f;
  float total = 0.f;
  for (int b = 0; b < B; ++b) {
    const float valid = (float)img_dot[B + b];
    total += (float)img_dot[b] * valid;   // losses.py:248: loss += lovasz_softmax(...) * mask_sample
    if (wscale) wscale[b] = valid / denom;
  }
  if (loss_out) loss_out[0] = total / denom;
}

__global__ void lovasz_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ target, int64_t B, int C,
                                  int64_t HW, const float* __restrict__ gpix, const float* __restrict__ wscale,
                                  const float* __restrict__ gout, float* __restrict__ grad) {
  const int64_t n = B * HW;
  const float go = gout ? gout[0] : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, p = i - b * HW;
    const float* tb = target + b * C * HW + p;
    int lab = 0;
    float best = tb[0];
    for (int c = 1; c < C; ++c) {
      const float v = tb[(int64_t)c * HW];
      if (v > best) {
        best = v;
        lab = c;
      }
    }
    const float d = (lab == 1 ? 1.f : 0.f) - logits[b * C * HW + HW + p];
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    float* gb = grad + b * C * HW + p;
    for (int c = 0; c < C; ++c) gb[(int64_t)c * HW] = 0.f;
    gb[HW] = -sg * gpix[i] * wscale[b] * go;
  }
}

struct Ws {
  unsigned *ka, *va, *kb, *vb, *hist, *tile_fg, *dtot;
  float *gpix, *wscale;
  double* dots;
};

int64_t tiles_of(int64_t HW) { return (HW + TILE - 1) / TILE; }

// The segmented sort: S segments of equal length L, ascending by key and stable, four passes of 8-bit digits.
// Pass 0 reads (kin, vin) and writes (ktmp, vtmp); the passes then alternate (kout, vout) and (ktmp, vtmp), so the
// sorted data ends in (kout, vout).  (kout, vout) may be (kin, vin): pass 0 has read them before pass 1 writes.
// hist: 256*S*T words, dtot: 4*256*S words (zeroed here).  1 <= S <= 65535 (gridDim.y), 1 <= L <= 2^24.
void seg_sort(const unsigned* kin, const unsigned* vin, unsigned* ktmp, unsigned* vtmp, unsigned* kout, unsigned* vout,
              unsigned S, int64_t L, unsigned* hist, unsigned* dtot_all, hipStream_t s) {
  const int T = (int)tiles_of(L);
  (void)hipMemsetAsync(dtot_all, 0, sizeof(unsigned) * (size_t)S * 256 * 4, s);   // the four passes' digit totals
  unsigned *kdst = ktmp, *vdst = vtmp;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    unsigned* dtot = dtot_all + (size_t)pass * S * 256;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(T, S), dim3(LT), 0, s, kin, L, T, shift, hist, dtot);
    hipLaunchKernelGGL(seg_rowscan_kernel, dim3(64, S), dim3(256), 0, s, hist, dtot, T);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(T, S), dim3(LT), 0, s, kin, vin, kdst, vdst, L, T, shift, hist);
    kin = kdst; vin = vdst;
    kdst = kdst == ktmp ? kout : ktmp;
    vdst = vdst == vtmp ? vout : vtmp;
  }
}

size_t ws_layout(int64_t B, int64_t HW, char* p, Ws* w) {
  const int64_t n = B * HW, T = tiles_of(HW);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return q;
  };
  char* ka = take(4 * n);
  char* va = take(4 * n);
  char* kb = take(4 * n);
  char* vb = take(4 * n);
  char* hist = take(4 * (size_t)B * 256 * T);
  char* tf = take(4 * (size_t)B * (T + 1));
  char* dots = take(8 * (size_t)B * T);
  char* wsc = take(4 * (size_t)B);
  char* dt = take(4 * (size_t)B * 256 * 4);   // per pass: digit totals of each segment
  if (w) {
    w->dtot = (unsigned*)dt;
    w->ka = (unsigned*)ka; w->va = (unsigned*)va; w->kb = (unsigned*)kb; w->vb = (unsigned*)vb;
    w->hist = (unsigned*)hist; w->tile_fg = (unsigned*)tf; w->dots = (double*)dots; w->wscale = (float*)wsc;
    w->gpix = (float*)kb;   // the sorted data ends in (ka, va); kb is free afterwards
  }
  return off;
}

// sort + Lovász gradient per pixel + loss (shared by fwd and bwd)
int lovasz_core(const float* logits, const float* target, int64_t B, int64_t C, int64_t HW, float* loss_out, Ws& w,
                hipStream_t s) {
  const int64_t n = B * HW;
  const int T = (int)tiles_of(HW);
  hipLaunchKernelGGL(lovasz_prep_kernel, dim3(ssseg_grid(n, 256)), dim3(256), 0, s, logits, target, B, (int)C, HW,
                     w.ka, w.va);
  seg_sort(w.ka, w.va, w.kb, w.vb, w.ka, w.va, (unsigned)B, HW, w.hist, w.dtot, s);   // sorted data back in (ka, va)
  hipLaunchKernelGGL(fg_count_kernel, dim3(T, (unsigned)B), dim3(LT), 0, s, w.va, HW, T, w.tile_fg);
  hipLaunchKernelGGL(fg_scan_kernel, dim3((unsigned)B), dim3(64), 0, s, w.tile_fg, T);
  hipLaunchKernelGGL(lovasz_grad_kernel, dim3(T, (unsigned)B), dim3(LT), 0, s, w.ka, w.va, HW, T, w.tile_fg, w.gpix,
                     w.dots);
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), dim3(FIN_T), 2 * B * sizeof(double), s, w.dots, w.tile_fg, (int)B, T, loss_out, w.wscale);
  return 0;
}

}  // namespace

extern "C" size_t ssseg_lovasz_workspace_bytes(int64_t B, int64_t HW) {
  if (B < 1 || HW < 1) return 0;
  return ws_layout(B, HW, nullptr, nullptr);
}

extern "C" int ssseg_lovasz_fwd(const float* logits, const float* target, int64_t B, int64_t C, int64_t HW,
                                float* loss_out, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!logits || !target || !loss_out || B < 1 || B > 4096 || C < 2 || HW < 1 || HW > 0x7fffffff) return SSSEG_EINVAL;
  if (!ws || ws_bytes < ssseg_lovasz_workspace_bytes(B, HW)) return SSSEG_EWORKSPACE;
  Ws w;
  ws_layout(B, HW, (char*)ws, &w);
  lovasz_core(logits, target, B, C, HW, loss_out, w, (hipStream_t)stream);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_lovasz_bwd(const float* logits, const float* target, int64_t B, int64_t C, int64_t HW,
                                const float* gout, float* grad_out, void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  if (!logits || !target || !grad_out || B < 1 || B > 4096 || C < 2 || HW < 1 || HW > 0x7fffffff) return SSSEG_EINVAL;
  if (!ws || ws_bytes < ssseg_lovasz_workspace_bytes(B, HW)) return SSSEG_EWORKSPACE;
  Ws w;
  ws_layout(B, HW, (char*)ws, &w);
  hipStream_t s = (hipStream_t)stream;
  lovasz_core(logits, target, B, C, HW, nullptr, w, s);
  hipLaunchKernelGGL(lovasz_bwd_kernel, dim3(ssseg_grid(B * HW, 256)), dim3(256), 0, s, logits, target, B, (int)C, HW,
                     w.gpix, w.wscale, gout, grad_out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

// the backward of a preceding ssseg_lovasz_fwd on the same inputs and workspace: the per-pixel Lovász gradient and the
// per-image scale it left in ws are scattered into grad_out (one launch; the sort is not repeated)
extern "C" int ssseg_lovasz_bwd_from_fwd(const float* logits, const float* target, int64_t B, int64_t C, int64_t HW,
                                         const float* gout, float* grad_out, const void* ws, size_t ws_bytes,
                                         ssseg_stream_t stream) {
  if (!logits || !target || !grad_out || B < 1 || B > 4096 || C < 2 || HW < 1 || HW > 0x7fffffff) return SSSEG_EINVAL;
  if (!ws || ws_bytes < ssseg_lovasz_workspace_bytes(B, HW)) return SSSEG_EWORKSPACE;
  Ws w;
  ws_layout(B, HW, (char*)ws, &w);
  hipLaunchKernelGGL(lovasz_bwd_kernel, dim3(ssseg_grid(B * HW, 256)), dim3(256), 0, (hipStream_t)stream, logits,
                     target, B, (int)C, HW, w.gpix, w.wscale, gout, grad_out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

// The losses' segmented sort on its own (seg_sort above, the same launches): workspace = one more pair of key / value
// buffers, the digit tables and the digit totals.
namespace {
size_t sort_ws_layout(int64_t S, int64_t L, char* p, unsigned** ktmp, unsigned** vtmp, unsigned** hist,
                      unsigned** dtot) {
  const int64_t T = tiles_of(L);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return (unsigned*)q;
  };
  unsigned* k = take(4 * (size_t)S * L);
  unsigned* v = take(4 * (size_t)S * L);
  unsigned* h = take(4 * (size_t)S * 256 * T);
  unsigned* d = take(4 * (size_t)S * 256 * 4);
  if (p) {
    *ktmp = k; *vtmp = v; *hist = h; *dtot = d;
  }
  return off;
}
}  // namespace

extern "C" size_t ssseg_lovasz_sort_workspace_bytes(int64_t S, int64_t L) {
  if (S < 1 || S > 65535 || L < 1 || L > ((int64_t)1 << 24)) return 0;
  return sort_ws_layout(S, L, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int ssseg_lovasz_sort(const unsigned* keys_in, const unsigned* vals_in, unsigned* keys_out,
                                 unsigned* vals_out, int64_t S, int64_t L, void* ws, size_t ws_bytes,
                                 ssseg_stream_t stream) {
  if (!keys_in || !vals_in || !keys_out || !vals_out || S < 1 || S > 65535 || L < 1 || L > ((int64_t)1 << 24))
    return SSSEG_EINVAL;
  if (!ws || ws_bytes < ssseg_lovasz_sort_workspace_bytes(S, L)) return SSSEG_EWORKSPACE;
  unsigned *ktmp, *vtmp, *hist, *dtot;
  sort_ws_layout(S, L, (char*)ws, &ktmp, &vtmp, &hist, &dtot);
  seg_sort(keys_in, vals_in, ktmp, vtmp, keys_out, vals_out, (unsigned)S, L, hist, dtot, (hipStream_t)stream);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// General Lovász losses (lovasz.py:79-127, 155-220): multi-class softmax / sigmoid errors and the binary hinge, any
// set of classes, 'present', per image or batch-wide, an ignore label.  The radix sort above is reused unchanged.
//
// group   = one image (per_image: G = B, L = HW) or the whole batch (G = 1, L = B*HW); segment = (group, selected
//           class k), S = G*K segments of equal length L.
// key     one mapping for both error kinds, ascending key = descending error:
//             e >= 0 (bit 31 clear):  key = ~bits(e) & 0x7fffffff      (0 .. 0x7fffffff, e = +0 -> 0x7fffffff)
//             e <  0 (bit 31 set):    key = bits(e)                    (0x80000001 .. 0xff800000 for finite e)
//           |fg - p| only has the first kind; the hinge error 1 - x*(2*label - 1) is signed (-0 is folded into +0).
//           No finite error maps to 0xffffffff (that is a negative NaN), so an ignored pixel gets that key: it sorts
//           strictly after every valid pixel, the stable sort keeps the valid pixels' relative order, and the sorted
//           positions 0 .. nvalid-1 are the positions the reference sees after it removed the void pixels.
//           Positions >= nvalid are skipped: no dot term, weight 0.
// value   pixel index inside the group (< 2^24) | fg << 31  (fg = 0 for ignored pixels)
// labels  read in place: int64, uint8, fp32 values, or a dense [B,C,HW] target whose argmax (first maximum) is the
//           label.  A label outside the selected classes that is not `ignore` is background for all of them.
// counts  one histogram pass over the labels gives the fg count per (group, class) (= gts, and the 'present'
//           decision) and the valid count per group, on the device: nothing is read back.
// chunks  classes are sorted Kc at a time in the same buffers: Kc = min(K, 8, max(1, 2^22 / (B*HW))).  Peak
//           workspace = 16*Kc*B*HW bytes of keys and values (at most 64 MiB unless one class alone is larger)
//           + 1024*G*Kc*(T+4) bytes of digit tables (T = ceil(L / 2048)) + 4*K*B*HW bytes for the per-pixel weights
//           the backward reads + O(G*(C+K)) tables.
// loss    per segment J, g in fp32 exactly as lovasz_grad_kernel, dot in fp64 (hinge: relu(e) in the dot, J over all
//           valid positions) -> table [G][K]; one final kernel: per group the fp32 mean over the counted classes
//           (all selected ones; under 'present' those with fg count > 0; none -> 0), then the fp32 mean over the
//           groups, both summed in index order by one thread each.
// softmax fused: p_c = fp32(exp(x_c - max) / sum_k exp(x_k - max)), the exponentials and their sum in fp64 so that
//           p is the correctly rounded softmax of the fp32 logits and the sort order does not hang on the last bit
//           of an fp32 exp; the backward turns dL/dp into dL/dx = p_c (dp_c - sum_k p_k dp_k) in one more pass.
// bounds  1 <= C <= 64, K <= 64, L <= 2^24 (fp32 counts exact), S <= 65535 (segments ride on gridDim.y).
// Defined where the reference breaks: an all-void group gives 0 loss and zero gradient and still counts in the mean
// over groups; a group with one valid pixel follows the formula.  Non-finite inputs are out of scope.
namespace {

constexpr int GEN_MAXSEL = 64;
constexpr int GEN_CHUNK_CLASSES = 8;
constexpr int64_t GEN_CHUNK_KEYS = (int64_t)1 << 22;

struct GenSel {
  int n;
  int cls[GEN_MAXSEL];
  int first[GEN_MAXSEL];        // 1: the first selection that maps to its channel (the backward stores), 0: it adds
  unsigned long long chmask;    // channels that some selection writes
};

struct GenArgs {
  const float* x;               // [B,C,HW]
  const void* labels;
  int lab_kind, C, G, mode, per_image, has_ignore, present;
  int64_t B, HW, L, ignore;
};

__device__ __forceinline__ int64_t gen_label(const GenArgs& a, int64_t i, int64_t b, int64_t pix) {
  if (a.lab_kind == SSSEG_LOVASZ_LABEL_I64) return ((const int64_t*)a.labels)[i];
  if (a.lab_kind == SSSEG_LOVASZ_LABEL_U8) return ((const unsigned char*)a.labels)[i];
  if (a.lab_kind == SSSEG_LOVASZ_LABEL_F32) return (int64_t)((const float*)a.labels)[i];
  const float* tb = (const float*)a.labels + b * a.C * a.HW + pix;
  int lab = 0;
  float best = tb[0];
  for (int c = 1; c < a.C; ++c) {
    const float v = tb[(int64_t)c * a.HW];
    if (v > best) {   // torch.argmax: first maximal index
      best = v;
      lab = c;
    }
  }
  return lab;
}

__device__ __forceinline__ unsigned gen_key(float e) {
  const unsigned u = __float_as_uint(e);
  return (u >> 31) ? u : (~u & 0x7fffffffu);
}
__device__ __forceinline__ float gen_err(unsigned key) {
  return __uint_as_float((key >> 31) ? key : (~key & 0x7fffffffu));
}

__device__ __forceinline__ void gen_softmax_stats(const float* xp, int C, int64_t HW, float& m, double& s) {
  m = xp[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, xp[(int64_t)c * HW]);
  s = 0.0;
  for (int c = 0; c < C; ++c) s += exp((double)xp[(int64_t)c * HW] - (double)m);
}
__device__ __forceinline__ float gen_softmax_p(float x, float m, double s) {
  return (float)(exp((double)x - (double)m) / s);
}

// cnt[g][c] = pixels of group g labelled c that are not ignored (C == 1: c = 0 counts the one selected class),
// cnt[g][C] = pixels that are not ignored.  Integer atomics: exact, order-free.  cnt zeroed before.
__global__ void __launch_bounds__(256) lovasz_gen_count_kernel(GenArgs a, GenSel sel, unsigned* __restrict__ cnt) {
  __shared__ unsigned c[GEN_MAXSEL + 1];
  const int g = blockIdx.y;
  for (int t = threadIdx.x; t <= a.C; t += 256) c[t] = 0;
  __syncthreads();
  unsigned nv = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.L; j += (int64_t)gridDim.x * 256) {
    const int64_t i = (int64_t)g * a.L + j, b = i / a.HW, pix = i - b * a.HW;
    const int64_t lab = gen_label(a, i, b, pix);
    if (a.has_ignore && lab == a.ignore) continue;
    ++nv;
    if (a.C == 1) {
      if (lab == sel.cls[0]) atomicAdd(&c[0], 1u);
    } else if (lab >= 0 && lab < a.C) {
      atomicAdd(&c[lab], 1u);
    }
  }
  for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
  if ((threadIdx.x & 63) == 0 && nv) atomicAdd(&c[a.C], nv);
  __syncthreads();
  for (int t = threadIdx.x; t <= a.C; t += 256)
    if (c[t]) atomicAdd(&cnt[(int64_t)g * (a.C + 1) + t], c[t]);
}

// keys / values of the classes k0 .. k0+kn-1: class kc of the chunk occupies [kc*N, (kc+1)*N), groups in order
__global__ void lovasz_gen_prep_kernel(GenArgs a, GenSel sel, int k0, int kn, unsigned* __restrict__ keys,
                                       unsigned* __restrict__ vals) {
  const int64_t n = a.B * a.HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / a.HW, pix = i - b * a.HW;
    const unsigned off = (unsigned)(a.per_image ? pix : i);
    const int64_t lab = gen_label(a, i, b, pix);
    const bool ign = a.has_ignore && lab == a.ignore;
    const float* xp = a.x + b * a.C * a.HW + pix;
    float m = 0.f;
    double ssum = 1.0;
    if (a.mode == SSSEG_LOVASZ_SOFTMAX && !ign) gen_softmax_stats(xp, a.C, a.HW, m, ssum);
    for (int kc = 0; kc < kn; ++kc) {
      const int cls = sel.cls[k0 + kc], ch = a.C == 1 ? 0 : cls;
      unsigned key = 0xffffffffu, fg = 0;
      if (!ign) {
        fg = lab == cls;
        const float xv = xp[(int64_t)ch * a.HW];
        float e;
        if (a.mode == SSSEG_LOVASZ_HINGE) e = (1.f - xv * (fg ? 1.f : -1.f)) + 0.f;
        else e = fabsf((float)fg - (a.mode == SSSEG_LOVASZ_SOFTMAX ? gen_softmax_p(xv, m, ssum) : xv));
        key = gen_key(e);
      }
      keys[(int64_t)kc * n + i] = key;
      vals[(int64_t)kc * n + i] = off | (fg << 31);
    }
  }
}

// lovasz_grad_kernel over the valid prefix of each sorted segment.  Segment blockIdx.y = kc*G + g; the weight of each
// pixel (g of its rank; for the hinge, 0 where relu cuts) goes to gpix[k0+kc][g*L + pixel], 0 for ignored pixels.
__global__ void __launch_bounds__(LT) lovasz_gen_grad_kernel(const unsigned* __restrict__ keys,
                                                             const unsigned* __restrict__ vals, int64_t L, int T, int G,
                                                             int C, int hinge, const unsigned* __restrict__ tile_fg,
                                                             const unsigned* __restrict__ cnt,
                                                             float* __restrict__ gpix, double* __restrict__ dots) {
  __shared__ unsigned wsum[NW];
  __shared__ double dred[NW];
  const int sg = blockIdx.y, t = blockIdx.x;
  const int kc = sg / G, grp = sg - kc * G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t seg = (int64_t)sg * L, base = (int64_t)t * TILE;
  const unsigned* tf = tile_fg + (int64_t)sg * (T + 1);
  const float gts = (float)tf[T];
  const int64_t nv = cnt[(int64_t)grp * (C + 1) + C];
  float* gp = gpix + seg;   // (k0 + kc) * N + grp * L with gpix already at class k0: N = G * L
  unsigned fg[ITEMS], v[ITEMS];
  unsigned mine = 0;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + (int64_t)threadIdx.x * ITEMS + s;
    v[s] = i < L ? vals[seg + i] : 0u;
    fg[s] = v[s] >> 31;
    mine += fg[s];
  }
  unsigned incl = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned wbase = 0;
  for (int w = 0; w < wave; ++w) wbase += wsum[w];
  unsigned F = tf[t] + wbase + incl - mine;
  double dot = 0.0;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t i = base + (int64_t)threadIdx.x * ITEMS + s;
    if (i >= L) break;
    const unsigned pixel = v[s] & 0x7fffffffu;
    if (i >= nv) {
      gp[pixel] = 0.f;
      continue;
    }
    const float Fprev = (float)F;
    F += fg[s];
    float g = jac(gts, (float)F, (float)(i + 1));
    if (i > 0) g = g - jac(gts, Fprev, (float)i);
    const float e = gen_err(keys[seg + i]);
    if (hinge) {
      dot += (double)fmaxf(e, 0.f) * (double)g;
      gp[pixel] = e > 0.f ? g : 0.f;
    } else {
      dot += (double)e * (double)g;
      gp[pixel] = g;
    }
  }
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
  if (lane == 0) dred[wave] = dot;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += dred[w];
    dots[(int64_t)sg * T + t] = s;
  }
}

// segloss[g][k0 + kc] = sum of the segment's T tile dots: one wave per segment, lane-strided then a fixed xor tree
__global__ void __launch_bounds__(256) lovasz_gen_segsum_kernel(const double* __restrict__ dots, int T, int S, int G,
                                                                int K, int k0, double* __restrict__ segloss) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= S) return;
  double s = 0.0;
  for (int t = lane; t < T; t += 64) s += dots[(int64_t)sg * T + t];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  const int kc = sg / G, grp = sg - kc * G;
  if (lane == 0) segloss[(int64_t)grp * K + k0 + kc] = s;
}

// the loss, and wscale[g][k] = [class k counted in group g] / (classes counted in g * G) for the backward
__global__ void __launch_bounds__(256) lovasz_gen_final_kernel(const double* __restrict__ segloss,
                                                               const unsigned* __restrict__ cnt, GenSel sel, int G,
                                                               int C, int present, float* __restrict__ gloss,
                                                               float* __restrict__ wscale, float* __restrict__ loss_out) {
  const int K = sel.n;
  for (int g = threadIdx.x; g < G; g += 256) {
    const unsigned* cg = cnt + (int64_t)g * (C + 1);
    float acc = 0.f;
    int nc = 0;
    for (int k = 0; k < K; ++k) {
      if (present && cg[C == 1 ? 0 : sel.cls[k]] == 0) continue;
      acc += (float)segloss[(int64_t)g * K + k];   // the reference's mean(): acc += v in order
      ++nc;
    }
    gloss[g] = nc > 1 ? acc / (float)nc : acc;
    const float w = nc ? 1.f / ((float)nc * (float)G) : 0.f;
    for (int k = 0; k < K; ++k)
      wscale[(int64_t)g * K + k] = (present && cg[C == 1 ? 0 : sel.cls[k]] == 0) ? 0.f : w;
  }
  __syncthreads();   // one block: the gloss stores above are visible to thread 0 below
  if (threadIdx.x != 0 || !loss_out) return;
  float tot = 0.f;
  for (int g = 0; g < G; ++g) tot += gloss[g];
  loss_out[0] = G > 1 ? tot / (float)G : tot;
}

// dL/dx [B,C,HW] from the per-pixel weights (for the softmax mode: dL/dp, turned into dL/dlogits by the next kernel)
__global__ void lovasz_gen_bwd_kernel(GenArgs a, GenSel sel, const float* __restrict__ gpix,
                                      const float* __restrict__ wscale, const float* __restrict__ gout,
                                      float* __restrict__ grad) {
  const int64_t n = a.B * a.HW;
  const float go = gout ? gout[0] : 1.f;
  const int K = sel.n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / a.HW, pix = i - b * a.HW;
    const int64_t grp = a.per_image ? b : 0;
    const int64_t lab = gen_label(a, i, b, pix);
    const bool ign = a.has_ignore && lab == a.ignore;
    const float* xp = a.x + b * a.C * a.HW + pix;
    float* gb = grad + b * a.C * a.HW + pix;
    for (int c = 0; c < a.C; ++c)
      if (ign || !((sel.chmask >> c) & 1ull)) gb[(int64_t)c * a.HW] = 0.f;
    if (ign) continue;
    float m = 0.f;
    double ssum = 1.0;
    if (a.mode == SSSEG_LOVASZ_SOFTMAX) gen_softmax_stats(xp, a.C, a.HW, m, ssum);
    for (int k = 0; k < K; ++k) {
      const int cls = sel.cls[k], ch = a.C == 1 ? 0 : cls;
      const bool fg = lab == cls;
      const float w = gpix[(int64_t)k * n + i] * (wscale[grp * K + k] * go);
      const float xv = xp[(int64_t)ch * a.HW];
      float v;
      if (a.mode == SSSEG_LOVASZ_HINGE) {
        v = fg ? -w : w;   // e = 1 - x * sign: de/dx = -sign; relu's cut is already in the weight
      } else {
        const float d = (fg ? 1.f : 0.f) - (a.mode == SSSEG_LOVASZ_SOFTMAX ? gen_softmax_p(xv, m, ssum) : xv);
        v = d > 0.f ? -w : (d < 0.f ? w : 0.f);
      }
      if (sel.first[k]) gb[(int64_t)ch * a.HW] = v;
      else gb[(int64_t)ch * a.HW] += v;
    }
  }
}

// in place: dp -> dx_c = p_c * (dp_c - sum_k p_k dp_k)
__global__ void lovasz_gen_softmax_bwd_kernel(GenArgs a, float* __restrict__ grad) {
  const int64_t n = a.B * a.HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / a.HW, pix = i - b * a.HW;
    const float* xp = a.x + b * a.C * a.HW + pix;
    float* gb = grad + b * a.C * a.HW + pix;
    float m;
    double ssum;
    gen_softmax_stats(xp, a.C, a.HW, m, ssum);
    float dotp = 0.f;
    for (int c = 0; c < a.C; ++c) dotp += gen_softmax_p(xp[(int64_t)c * a.HW], m, ssum) * gb[(int64_t)c * a.HW];
    for (int c = 0; c < a.C; ++c) {
      const float p = gen_softmax_p(xp[(int64_t)c * a.HW], m, ssum);
      gb[(int64_t)c * a.HW] = p * (gb[(int64_t)c * a.HW] - dotp);
    }
  }
}

struct GenWs {
  unsigned *ka, *va, *kb, *vb, *hist, *tile_fg, *dtot, *cnt;
  float *gpix, *wscale, *gloss;
  double *dots, *segloss;
};

int gen_chunk(int64_t N, int K) {
  int64_t kc = GEN_CHUNK_KEYS / N;
  if (kc < 1) kc = 1;
  if (kc > GEN_CHUNK_CLASSES) kc = GEN_CHUNK_CLASSES;
  if (kc > K) kc = K;
  return (int)kc;
}

size_t gen_ws_layout(int64_t B, int C, int64_t HW, int per_image, int K, char* p, GenWs* w) {
  const int64_t N = B * HW, G = per_image ? B : 1, L = per_image ? HW : N, T = tiles_of(L);
  const int64_t Kc = gen_chunk(N, K), Sc = G * Kc;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return q;
  };
  char* ka = take(4 * (size_t)Kc * N);
  char* va = take(4 * (size_t)Kc * N);
  char* kb = take(4 * (size_t)Kc * N);
  char* vb = take(4 * (size_t)Kc * N);
  char* hist = take(4 * (size_t)Sc * 256 * T);
  char* tf = take(4 * (size_t)Sc * (T + 1));
  char* dots = take(8 * (size_t)Sc * T);
  char* dt = take(4 * (size_t)Sc * 256 * 4);
  char* gpix = take(4 * (size_t)K * N);
  char* cnt = take(4 * (size_t)G * (C + 1));
  char* sl = take(8 * (size_t)G * K);
  char* wsc = take(4 * (size_t)G * K);
  char* gl = take(4 * (size_t)G);
  if (w) {
    w->ka = (unsigned*)ka; w->va = (unsigned*)va; w->kb = (unsigned*)kb; w->vb = (unsigned*)vb;
    w->hist = (unsigned*)hist; w->tile_fg = (unsigned*)tf; w->dots = (double*)dots; w->dtot = (unsigned*)dt;
    w->gpix = (float*)gpix; w->cnt = (unsigned*)cnt; w->segloss = (double*)sl; w->wscale = (float*)wsc;
    w->gloss = (float*)gl;
  }
  return off;
}

// argument check and the by-value structures of the kernels; 0 or SSSEG_EINVAL
int gen_setup(const float* x, const void* labels, int label_kind, int64_t B, int64_t C, int64_t HW, int mode,
              int per_image, int present, const int64_t* classes, int64_t nsel, int has_ignore, int64_t ignore,
              GenArgs* a, GenSel* sel) {
  if (!x || !labels || !classes || B < 1 || HW < 1 || C < 1 || C > 64 || nsel < 1 || nsel > GEN_MAXSEL)
    return SSSEG_EINVAL;
  if (label_kind < SSSEG_LOVASZ_LABEL_I64 || label_kind > SSSEG_LOVASZ_LABEL_DENSE) return SSSEG_EINVAL;
  if (mode < SSSEG_LOVASZ_PROBAS || mode > SSSEG_LOVASZ_HINGE) return SSSEG_EINVAL;
  if (label_kind == SSSEG_LOVASZ_LABEL_DENSE && C < 2) return SSSEG_EINVAL;
  if (C == 1 && nsel != 1) return SSSEG_EINVAL;
  if (mode == SSSEG_LOVASZ_HINGE && (C != 1 || classes[0] != 1)) return SSSEG_EINVAL;
  if (mode == SSSEG_LOVASZ_SOFTMAX && C < 2) return SSSEG_EINVAL;
  if (B > ((int64_t)1 << 24) || HW > ((int64_t)1 << 24)) return SSSEG_EINVAL;
  const int64_t G = per_image ? B : 1, L = per_image ? HW : B * HW;
  if (L > ((int64_t)1 << 24) || G * nsel > 65535) return SSSEG_EINVAL;
  sel->n = (int)nsel;
  sel->chmask = 0;
  for (int k = 0; k < GEN_MAXSEL; ++k) sel->cls[k] = sel->first[k] = 0;
  for (int k = 0; k < nsel; ++k) {
    const int64_t c = classes[k];
    if (C > 1 && (c < 0 || c >= C)) return SSSEG_EINVAL;
    if (c < -0x7fffffff || c > 0x7fffffff) return SSSEG_EINVAL;
    const int ch = C == 1 ? 0 : (int)c;
    sel->cls[k] = (int)c;
    sel->first[k] = !((sel->chmask >> ch) & 1ull);
    sel->chmask |= 1ull << ch;
  }
  a->x = x; a->labels = labels; a->lab_kind = label_kind; a->C = (int)C; a->G = (int)G; a->mode = mode;
  a->per_image = per_image != 0; a->has_ignore = has_ignore != 0; a->present = present != 0;
  a->B = B; a->HW = HW; a->L = L; a->ignore = ignore;
  return 0;
}

// counts, then per class chunk: keys -> sort -> fg scan -> weights and dots -> segment losses; then the loss
void gen_core(const GenArgs& a, const GenSel& sel, float* loss_out, GenWs& w, hipStream_t s) {
  const int64_t N = a.B * a.HW, L = a.L;
  const int G = a.G, K = sel.n, T = (int)tiles_of(L), Kc = gen_chunk(N, K);
  (void)hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * (size_t)G * (a.C + 1), s);
  const int cblocks = (int)((L + 256 * 16 - 1) / (256 * 16));
  hipLaunchKernelGGL(lovasz_gen_count_kernel, dim3(cblocks < 64 ? cblocks : 64, (unsigned)G), dim3(256), 0, s, a, sel,
                     w.cnt);
  for (int k0 = 0; k0 < K; k0 += Kc) {
    const int kn = K - k0 < Kc ? K - k0 : Kc;
    const unsigned S = (unsigned)(G * kn);
    hipLaunchKernelGGL(lovasz_gen_prep_kernel, dim3(ssseg_grid(N, 256)), dim3(256), 0, s, a, sel, k0, kn, w.ka, w.va);
    seg_sort(w.ka, w.va, w.kb, w.vb, w.ka, w.va, S, L, w.hist, w.dtot, s);
    hipLaunchKernelGGL(fg_count_kernel, dim3(T, S), dim3(LT), 0, s, w.va, L, T, w.tile_fg);
    hipLaunchKernelGGL(fg_scan_kernel, dim3(S), dim3(64), 0, s, w.tile_fg, T);
    hipLaunchKernelGGL(lovasz_gen_grad_kernel, dim3(T, S), dim3(LT), 0, s, w.ka, w.va, L, T, G, a.C,
                       (int)(a.mode == SSSEG_LOVASZ_HINGE), w.tile_fg, w.cnt, w.gpix + (size_t)k0 * N, w.dots);
    hipLaunchKernelGGL(lovasz_gen_segsum_kernel, dim3((S + 3) / 4), dim3(256), 0, s, w.dots, T, (int)S, G, K, k0,
                       w.segloss);
  }
  hipLaunchKernelGGL(lovasz_gen_final_kernel, dim3(1), dim3(256), 0, s, w.segloss, w.cnt, sel, G, a.C, a.present,
                     w.gloss, w.wscale, loss_out);
}

void gen_scatter(const GenArgs& a, const GenSel& sel, const GenWs& w, const float* gout, float* grad_out,
                 hipStream_t s) {
  const int64_t N = a.B * a.HW;
  hipLaunchKernelGGL(lovasz_gen_bwd_kernel, dim3(ssseg_grid(N, 256)), dim3(256), 0, s, a, sel, w.gpix, w.wscale, gout,
                     grad_out);
  if (a.mode == SSSEG_LOVASZ_SOFTMAX)
    hipLaunchKernelGGL(lovasz_gen_softmax_bwd_kernel, dim3(ssseg_grid(N, 256)), dim3(256), 0, s, a, grad_out);
}

}  // namespace

extern "C" size_t ssseg_lovasz_gen_workspace_bytes(int64_t B, int64_t C, int64_t HW, int per_image, int64_t nsel) {
  if (B < 1 || HW < 1 || C < 1 || C > 64 || nsel < 1 || nsel > GEN_MAXSEL) return 0;
  if (B > ((int64_t)1 << 24) || HW > ((int64_t)1 << 24)) return 0;
  if ((per_image ? HW : B * HW) > ((int64_t)1 << 24) || (per_image ? B : 1) * nsel > 65535) return 0;
  return gen_ws_layout(B, (int)C, HW, per_image, (int)nsel, nullptr, nullptr);
}

extern "C" int ssseg_lovasz_gen_fwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                    int64_t HW, int mode, int per_image, int present, const int64_t* classes,
                                    int64_t nsel, int has_ignore, int64_t ignore, float* loss_out, void* ws,
                                    size_t ws_bytes, ssseg_stream_t stream) {
  GenArgs a;
  GenSel sel;
  if (!loss_out) return SSSEG_EINVAL;
  if (int rc = gen_setup(x, labels, label_kind, B, C, HW, mode, per_image, present, classes, nsel, has_ignore, ignore,
                         &a, &sel))
    return rc;
  if (!ws || ws_bytes < ssseg_lovasz_gen_workspace_bytes(B, C, HW, per_image, nsel)) return SSSEG_EWORKSPACE;
  GenWs w;
  gen_ws_layout(B, (int)C, HW, per_image, (int)nsel, (char*)ws, &w);
  gen_core(a, sel, loss_out, w, (hipStream_t)stream);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_lovasz_gen_bwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                    int64_t HW, int mode, int per_image, int present, const int64_t* classes,
                                    int64_t nsel, int has_ignore, int64_t ignore, const float* gout, float* grad_out,
                                    void* ws, size_t ws_bytes, ssseg_stream_t stream) {
  GenArgs a;
  GenSel sel;
  if (!grad_out) return SSSEG_EINVAL;
  if (int rc = gen_setup(x, labels, label_kind, B, C, HW, mode, per_image, present, classes, nsel, has_ignore, ignore,
                         &a, &sel))
    return rc;
  if (!ws || ws_bytes < ssseg_lovasz_gen_workspace_bytes(B, C, HW, per_image, nsel)) return SSSEG_EWORKSPACE;
  GenWs w;
  gen_ws_layout(B, (int)C, HW, per_image, (int)nsel, (char*)ws, &w);
  gen_core(a, sel, nullptr, w, (hipStream_t)stream);
  gen_scatter(a, sel, w, gout, grad_out, (hipStream_t)stream);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

// the backward of a preceding ssseg_lovasz_gen_fwd on the same inputs, configuration and workspace: the per-pixel
// weights and the class scales it left in ws are scattered into grad_out; nothing is sorted again
extern "C" int ssseg_lovasz_gen_bwd_from_fwd(const float* x, const void* labels, int label_kind, int64_t B, int64_t C,
                                             int64_t HW, int mode, int per_image, int present,
                                             const int64_t* classes, int64_t nsel, int has_ignore, int64_t ignore,
                                             const float* gout, float* grad_out, const void* ws, size_t ws_bytes,
                                             ssseg_stream_t stream) {
  GenArgs a;
  GenSel sel;
  if (!grad_out) return SSSEG_EINVAL;
  if (int rc = gen_setup(x, labels, label_kind, B, C, HW, mode, per_image, present, classes, nsel, has_ignore, ignore,
                         &a, &sel))
    return rc;
  if (!ws || ws_bytes < ssseg_lovasz_gen_workspace_bytes(B, C, HW, per_image, nsel)) return SSSEG_EWORKSPACE;
  GenWs w;
  gen_ws_layout(B, (int)C, HW, per_image, (int)nsel, (char*)ws, &w);
  gen_scatter(a, sel, w, gout, grad_out, (hipStream_t)stream);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
