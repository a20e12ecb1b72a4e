// The tail of a training step over the flat arenas in ONE launch (ssseg_param_step): clip + SGD, teacher EMA, the
// bf16 repack of every conv weight (student and teacher) and the gradient clear.  Each master weight is read once
// and every pack written once; the separate sequence (ssseg_sgd_step, ssseg_ema_update, two ssseg_weight_pack_batch,
// the gradient memset) read p three times and ema twice.
//
// Arithmetic: the expressions of sgd_kernel / ema_kernel (eltwise.hip) and the packs' f32_to_bf16, element for
// element, so every output bit equals the separate sequence's.  sgd_kernel's momentum update is written there as
// __fadd_rn(__fmul_rn(buf, mom), d) and compiles, under the default -ffp-contract=fast, to one fma (DESIGN.md 20,
// tests/exact_step.py sgd_ref); it is spelled fmaf here so that no other product of this file can be picked for the
// contraction instead.  This file is built with the same flags as eltwise.hip (clip coefficient included).
#include <algorithm>

#include "common.h"

namespace {

constexpr int PS_E = 8 * 8 * 135;   // staged elements per tile: the smallest tile (8 x 8) of a 135-tap filter
constexpr int PS_MAXD = 1024;       // descriptors per launch (the host splits larger tables)
constexpr int PS_FLAT = 4096;       // elements per tile of a range without packs: 4 x 16 bytes per thread
constexpr int PS_U = 4;             // 16-byte pieces per thread and array in flight

// a / d by a float reciprocal, exact for 0 <= a < 4e6 (the argument of conv.hip's pk_div)
__device__ __forceinline__ int ps_div(int a, float inv_d) { return (int)(((float)a + 0.5f) * inv_d); }

// tile of a conv weight [A][B][RS]: TA rows x TB columns x every tap, both multiples of 8 so that either index can
// be a pack's channel (8 channels = one 16-byte store), sized to PS_E with the odd LDS row stride RS | 1
__device__ __forceinline__ void ps_tile_dims(int RS, int& TA, int& TB) {
  const int RSP = RS | 1;
  TA = RSP <= 2 ? 32 : (RSP <= 33 ? 16 : 8);
  TB = 128;
  while (TB > 8 && TA * TB * RSP > PS_E) TB >>= 1;
}

__device__ __forceinline__ int ps_tiles(const ssseg_pstep_desc& d) {
  if (d.A == 0) {   // flat range: whole 16-byte pieces of the arena that the range touches
    if (d.n <= 0) return 0;
    const long long q0 = d.off >> 2, q1 = (d.off + d.n + 3) >> 2;
    return (int)(((q1 - q0) * 4 + PS_FLAT - 1) / PS_FLAT);
  }
  const int RS = (int)(d.Rs * d.Ss);
  if (RS < 1 || RS > 135) return 0;   // (host contract: filters of <= 135 taps, ssseg.h)
  int TA, TB;
  ps_tile_dims(RS, TA, TB);
  return (int)((d.Ap + TA - 1) / TA) * (int)((d.Bp + TB - 1) / TB);
}

struct PsArgs {
  float* p;
  float* g;
  float* buf;
  float* ema;
  const ssseg_pstep_desc* descs;
  const ssseg_pstep_pack* packs;
  int n;
  float lr, mom, wd, max_norm;
  const float* sqnorm;
  const float* amp;
  int first, clear;
  float a, beta;
};

struct PsCoef {
  float coef;
  bool skip;
};

// one element: sgd_kernel's body (eltwise.hip), then ema_kernel's on the updated parameter
template <bool SGD, bool MOM, bool EMA>
__device__ __forceinline__ void ps_elem(float& p, float& g, float& b, float& e, const PsArgs& h, const PsCoef& k) {
  if (SGD && !k.skip) {
    const float gi = __fmul_rn(g, k.coef);
    g = gi;
    const float pi = p;
    const float d = h.wd != 0.f ? fmaf(pi, h.wd, gi) : gi;
    float nb;
    if (MOM) {
      nb = h.first ? d : fmaf(b, h.mom, d);
      b = nb;
    } else {
      nb = d;
    }
    p = fmaf(nb, -h.lr, pi);
  }
  if (EMA) e = fmaf(p, h.beta, __fmul_rn(e, h.a));
}

// phase 1 of a conv tile: rows a0 .. a0 + na of the source, L elements each from column b0, in source order; the
// updated values go back to the arenas and, as bf16, into the LDS images [al][bl][t] (row stride RSP)
template <bool SGD, bool MOM, bool EMA, int V>
__device__ __forceinline__ void ps_conv_update(const PsArgs& h, const PsCoef& k, long long base, int rowlen, int na,
                                               int L, int TB, int RS, int RSP, bf16_t* sS, bf16_t* sT) {
  using CK = Chunk<float, V>;
  const int Lq = L / V, nq = na * Lq;
  const float iLq = 1.f / (float)Lq, iRS = 1.f / (float)RS;
  for (int u0 = 0; u0 < nq; u0 += 256 * PS_U) {
    typename CK::raw P[PS_U], G[PS_U], Bf[PS_U], Em[PS_U];
    int gi[PS_U], li[PS_U], tt[PS_U];   // (a weight has < 2^31 elements: 32-bit offsets from its tile's base)
    // every load of the batch first, from clamped addresses: no branch around a load
#pragma unroll
    for (int it = 0; it < PS_U; ++it) {
      const int u = min(u0 + it * 256 + (int)threadIdx.x, nq - 1);
      const int al = ps_div(u, iLq);
      const int r = (u - al * Lq) * V;
      const int bl = ps_div(r, iRS);
      tt[it] = r - bl * RS;
      li[it] = (al * TB + bl) * RSP + tt[it];
      gi[it] = al * rowlen + r;
      P[it] = CK::ld(h.p + base + gi[it]);
      if (SGD) G[it] = CK::ld(h.g + base + gi[it]);
      if (MOM) Bf[it] = CK::ld(h.buf + base + gi[it]);
      if (EMA) Em[it] = CK::ld(h.ema + base + gi[it]);
    }
#pragma unroll
    for (int it = 0; it < PS_U; ++it) {
      if (u0 + it * 256 + (int)threadIdx.x >= nq) continue;
      float p[V], g[V], b[V], e[V];
      CK::cvt(P[it], p);
      if (SGD) CK::cvt(G[it], g);
      if (MOM) CK::cvt(Bf[it], b);
      if (EMA) CK::cvt(Em[it], e);
#pragma unroll
      for (int x = 0; x < V; ++x) ps_elem<SGD, MOM, EMA>(p[x], g[x], b[x], e[x], h, k);
      if (SGD && !k.skip) {
        Vec<float, V>::st(h.p + base + gi[it], p);
        if (MOM) Vec<float, V>::st(h.buf + base + gi[it], b);
      }
      if (EMA) Vec<float, V>::st(h.ema + base + gi[it], e);
      if (h.clear) {
#pragma unroll
        for (int x = 0; x < V; ++x) g[x] = 0.f;
        Vec<float, V>::st(h.g + base + gi[it], g);
      } else if (SGD && !k.skip) {
        Vec<float, V>::st(h.g + base + gi[it], g);   // left clipped, as sgd_kernel leaves it
      }
      int o = li[it], t = tt[it];
#pragma unroll
      for (int x = 0; x < V; ++x) {
        if (SGD) sS[o] = f32_to_bf16(p[x]);
        if (EMA) sT[o] = f32_to_bf16(e[x]);
        ++o;
        if (++t == RS) {   // next source column: skip the pad of the odd row stride
          t = 0;
          o += RSP - RS;
        }
      }
    }
  }
}

// phase 2 of a conv tile: one pack, written in packed order [k][rr][ss][c], 8 channels per thread
__device__ __forceinline__ void ps_conv_pack(const ssseg_pstep_pack& pk, const bf16_t* lds, int a0, int b0, int TA,
                                             int TB, int RSP, int Ss) {
  const bool l0 = pk.layout == 0;
  const int Kd = (int)pk.Kd, Cp = (int)pk.Cp, Sn = (int)pk.Sn, taps = (int)pk.Rn * Sn;
  const int r0 = (int)pk.r0, rstep = (int)pk.rstep, s0 = (int)pk.s0, sstep = (int)pk.sstep;
  const int kbase = l0 ? a0 : b0, kext = l0 ? TA : TB, cbase = l0 ? b0 : a0, cext = l0 ? TB : TA;
  if (taps < 1 || kbase >= Kd || cbase >= Cp) return;
  bf16_t* dst = (bf16_t*)pk.dst;
  const int c8n = cext / 8, lc8 = __builtin_ctz((unsigned)c8n);
  const int n2 = kext * taps * c8n;
  const float iTC = 1.f / (float)(taps * c8n), iSn = 1.f / (float)Sn;
  for (int j = threadIdx.x; j < n2; j += 256) {
    const int kk = ps_div(j, iTC);
    const int rem = j - kk * taps * c8n;
    const int tp = rem >> lc8, c8 = rem & (c8n - 1);
    const int k = kbase + kk, c = cbase + c8 * 8;
    if (k >= Kd || c >= Cp) continue;
    const int rr = ps_div(tp, iSn), ss = tp - rr * Sn;
    const int t = (r0 + rr * rstep) * Ss + s0 + ss * sstep;
    bf16_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = l0 ? lds[(kk * TB + c8 * 8 + e) * RSP + t] : lds[((c8 * 8 + e) * TB + kk) * RSP + t];
    const int o = (k * taps + tp) * Cp + c;
    if (c + 8 <= Cp && (Cp & 7) == 0) {
      uint4 q;
      q.x = (unsigned)v[0] | ((unsigned)v[1] << 16);
      q.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
      q.z = (unsigned)v[4] | ((unsigned)v[5] << 16);
      q.w = (unsigned)v[6] | ((unsigned)v[7] << 16);
      *(uint4*)(dst + o) = q;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c + e < Cp) dst[o + e] = v[e];
    }
  }
}

// a range without packs (BN, biases, heads, alignment gaps): the 16-byte pieces of the arena it touches, elements
// outside [off, off + n) masked (they belong to a neighbouring conv weight's tiles)
template <bool SGD, bool MOM, bool EMA>
__device__ __forceinline__ void ps_flat(const PsArgs& h, const PsCoef& k, long long off, long long n, int tile) {
  const long long lo = off, hi = off + n;
  const long long first = (off >> 2) * 4 + (long long)tile * PS_FLAT;
  const long long last = ((hi - 1) >> 2) * 4;   // the last piece of the range
  using F4 = Chunk<float, 4>;
  F4::raw P[PS_U], G[PS_U], Bf[PS_U], Em[PS_U];
  long long gi[PS_U];
#pragma unroll
  for (int it = 0; it < PS_U; ++it) {
    gi[it] = first + (long long)(it * 256 + (int)threadIdx.x) * 4;
    const long long i = gi[it] < last ? gi[it] : last;
    P[it] = F4::ld(h.p + i);
    if (SGD) G[it] = F4::ld(h.g + i);
    if (MOM) Bf[it] = F4::ld(h.buf + i);
    if (EMA) Em[it] = F4::ld(h.ema + i);
  }
#pragma unroll
  for (int it = 0; it < PS_U; ++it) {
    const long long i = gi[it];
    if (i > last) continue;
    float p[4], g[4], b[4], e[4];
    F4::cvt(P[it], p);
    if (SGD) F4::cvt(G[it], g);
    if (MOM) F4::cvt(Bf[it], b);
    if (EMA) F4::cvt(Em[it], e);
#pragma unroll
    for (int x = 0; x < 4; ++x) ps_elem<SGD, MOM, EMA>(p[x], g[x], b[x], e[x], h, k);
    const bool wr = SGD && !k.skip;
    if (i >= lo && i + 4 <= hi) {
      if (wr) {
        Vec<float, 4>::st(h.p + i, p);
        if (MOM) Vec<float, 4>::st(h.buf + i, b);
      }
      if (EMA) Vec<float, 4>::st(h.ema + i, e);
      if (h.clear) *(float4*)(h.g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      else if (wr) Vec<float, 4>::st(h.g + i, g);
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        if (i + x < lo || i + x >= hi) continue;
        if (wr) {
          h.p[i + x] = p[x];
          if (MOM) h.buf[i + x] = b[x];
        }
        if (EMA) h.ema[i + x] = e[x];
        if (h.clear) h.g[i + x] = 0.f;
        else if (wr) h.g[i + x] = g[x];
      }
    }
  }
}

template <bool SGD, bool MOM, bool EMA>
__global__ void __launch_bounds__(256) param_step_kernel(const PsArgs h) {
  __shared__ __attribute__((aligned(16))) bf16_t sS[PS_E];   // bf16(p') of the tile
  __shared__ __attribute__((aligned(16))) bf16_t sT[PS_E];   // bf16(ema')
  __shared__ int pre[PS_MAXD + 1];   // tile-count prefix sums of the descriptors (the flat tile space of the launch)
  const int n = h.n;
  if (threadIdx.x < 64) {
    int carry = 0;
    const int lane = threadIdx.x;
    for (int base = 0; base < n; base += 64) {
      const int d = base + lane;
      int v = d < n ? ps_tiles(h.descs[d]) : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
      }
      if (d < n) pre[d + 1] = carry + v;
      carry += __shfl(v, 63, 64);
    }
    if (lane == 0) pre[0] = 0;
  }
  // the clip coefficient, as sgd_kernel computes it
  PsCoef k{1.f, false};
  if (SGD) {
    float coef = 1.f;
    if (h.amp) {   // loss-scaled gradients: unscale; a non-finite norm skips the optimizer step (not the EMA)
      if (!isfinite(h.sqnorm[0])) k.skip = true;
      else coef = h.amp[3];
    }
    if (h.max_norm > 0.f && !k.skip) {
      const float total = sqrtf(h.sqnorm[0]) * coef;
      coef *= fminf(h.max_norm / (total + 1e-6f), 1.f);
    }
    k.coef = coef;
  }
  __syncthreads();
  const int total = pre[n];
  for (int gt = blockIdx.x; gt < total; gt += gridDim.x) {
    int lo = 0, hi = n - 1;   // the descriptor d with pre[d] <= gt < pre[d + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= gt) lo = mid;
      else hi = mid - 1;
    }
    const ssseg_pstep_desc& d = h.descs[lo];
    const int tile = gt - pre[lo];
    if (d.A == 0) {
      ps_flat<SGD, MOM, EMA>(h, k, d.off, d.n, tile);
      continue;
    }
    const int A = (int)d.A, B = (int)d.B, Ap = (int)d.Ap, Bp = (int)d.Bp, Ss = (int)d.Ss;
    const int RS = (int)d.Rs * Ss, RSP = RS | 1;
    int TA, TB;
    ps_tile_dims(RS, TA, TB);
    const int nb = (Bp + TB - 1) / TB;
    const int a0 = (tile / nb) * TA, b0 = (tile % nb) * TB;
    const int na = max(0, min(TA, A - a0)), nbl = max(0, min(TB, B - b0));
    // padding rows / channels of the packs inside this tile read as zero
    if (min(a0 + TA, Ap) > A || min(b0 + TB, Bp) > B) {
      for (int i = threadIdx.x; i < PS_E / 8; i += 256) {
        ((uint4*)sS)[i] = make_uint4(0, 0, 0, 0);
        ((uint4*)sT)[i] = make_uint4(0, 0, 0, 0);
      }
      __syncthreads();
    }
    if (na > 0 && nbl > 0) {
      const long long base = d.off + ((long long)a0 * B + b0) * RS;
      const int rowlen = B * RS, L = nbl * RS;
      if (((rowlen | L) & 3) == 0 && (base & 3) == 0)
        ps_conv_update<SGD, MOM, EMA, 4>(h, k, base, rowlen, na, L, TB, RS, RSP, sS, sT);
      else
        ps_conv_update<SGD, MOM, EMA, 1>(h, k, base, rowlen, na, L, TB, RS, RSP, sS, sT);
    }
    __syncthreads();
    for (int pi = 0; pi < (int)d.npacks; ++pi) {
      const ssseg_pstep_pack& pk = h.packs[d.pack0 + pi];
      if (pk.teacher ? !EMA : !SGD) continue;   // that master did not change
      ps_conv_pack(pk, pk.teacher ? sT : sS, a0, b0, TA, TB, RSP, Ss);
    }
    __syncthreads();
  }
}

template <bool SGD, bool MOM, bool EMA>
void ps_launch(const PsArgs& h, hipStream_t s) {
  hipLaunchKernelGGL((param_step_kernel<SGD, MOM, EMA>), dim3(2048), dim3(256), 0, s, h);
}

}  // namespace

extern "C" int ssseg_param_step(float* param, float* grad, float* momentum_buf, float* ema,
                                const ssseg_pstep_desc* descs, int64_t n_descs, const ssseg_pstep_pack* packs,
                                float lr, float momentum, float weight_decay, float max_norm, const float* sqnorm,
                                int first_step, const float* amp_state, double alpha, int flags,
                                ssseg_stream_t stream) {
  const bool sgd = flags & SSSEG_PSTEP_SGD, ema_on = flags & SSSEG_PSTEP_EMA, clear = flags & SSSEG_PSTEP_CLEAR;
  const bool mom = sgd && momentum != 0.f;
  if (!param || n_descs < 0 || n_descs > 65535 || (n_descs > 0 && !descs) || (flags & ~7)) return SSSEG_EINVAL;
  if (((sgd || clear) && !grad) || (mom && !momentum_buf) || (ema_on && !ema)) return SSSEG_EINVAL;
  if (sgd && (max_norm > 0.f || amp_state) && !sqnorm) return SSSEG_EINVAL;
  if ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)momentum_buf) | ((uintptr_t)ema)) & 15) return SSSEG_EINVAL;
  if (n_descs == 0 || !(sgd || ema_on || clear)) return 0;
  PsArgs h;
  h.p = param;
  h.g = grad;
  h.buf = momentum_buf;
  h.ema = ema;
  h.packs = packs;
  h.lr = lr;
  h.mom = momentum;
  h.wd = weight_decay;
  h.max_norm = max_norm;
  h.sqnorm = sqnorm;
  h.amp = amp_state;
  h.first = first_step;
  h.clear = clear;
  h.a = (float)alpha;
  h.beta = (float)(1.0 - alpha);
  for (int64_t b = 0; b < n_descs; b += PS_MAXD) {
    h.descs = descs + b;
    h.n = (int)std::min<int64_t>(PS_MAXD, n_descs - b);
    hipStream_t s = (hipStream_t)stream;
    if (sgd && mom && ema_on) ps_launch<true, true, true>(h, s);
    else if (sgd && mom) ps_launch<true, true, false>(h, s);
    else if (sgd && ema_on) ps_launch<true, false, true>(h, s);
    else if (sgd) ps_launch<true, false, false>(h, s);
    else if (ema_on) ps_launch<false, false, true>(h, s);
    else ps_launch<false, false, false>(h, s);
  }
  SSSEG_LAUNCH_CHECK();
  return 0;
}
