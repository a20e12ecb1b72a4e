// Fused optimizer step of the Adam family over the flat parameter arena: torch.optim.Adam and the reference's
// optimizers/ (AdaMod arXiv:1910.12249, diffGrad arXiv:1909.11015, DiffMod = diffGrad x AdaMod, Ranger = RAdam
// arXiv:1908.03265 + Lookahead arXiv:1907.08610), two launches per step with fixed arguments:
//   optim_prepare_kernel  one thread: step counter, clip / loss-scale coefficient, bias corrections, RAdam
//                         rectification and the Lookahead decision, all in fp64 on the device (the reference computes
//                         them in Python doubles on the host, which a captured graph would freeze at capture time)
//   optim_step_kernel     one float4 pass over param / grad / state arenas
// state block (double[SSSEG_OPT_STATE_DOUBLES]): [0] t  [1] skip  [2] gradient coefficient  [3] [4] step scalars of
// the mode (below)  [5] rectified  [6] lookahead step  [7] t == 1.
// Rounding: fp32 operations are rounded one by one in the order of the reference's tensor ops; fmaf appears exactly
// where torch's add_(x, alpha=) / lerp_ / addcmul_ fuse on the host.  This file is built with -ffp-contract=off.
#include "common.h"

namespace {

enum { ST_T = 0, ST_SKIP, ST_COEF, ST_A, ST_B, ST_RECT, ST_LOOK, ST_FIRST };

// Per mode: A, B =
//   Adam      -(lr / bc1),                 sqrt(bc2)
//   AdaMod    lr * sqrt(bc2) / bc1,        -weight_decay * lr
//   DiffGrad  -(lr * sqrt(bc2) / bc1),     -
//   DiffMod   lr * sqrt(bc2) / bc1,        -weight_decay * lr
//   Ranger    -step_size * lr,             -weight_decay * lr
__global__ void optim_prepare_kernel(double* st, int mode, double lr, double b1, double b2, double wd, double max_norm,
                                     int64_t k, double nsma_thr, const float* sqnorm, const float* amp) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double coef = 1.0;
  if (amp) {   // loss-scaled gradients: a non-finite norm skips the step and leaves the counter alone
    if (!isfinite(sqnorm[0])) {
      st[ST_SKIP] = 1.0;
      return;
    }
    coef = (double)amp[3];
  }
  if (max_norm > 0.0) {
    const double total = sqrt((double)sqnorm[0]) * coef;
    coef *= fmin(max_norm / (total + 1e-6), 1.0);
  }
  const double t = st[ST_T] + 1.0;
  st[ST_T] = t;
  st[ST_SKIP] = 0.0;
  st[ST_COEF] = coef;
  st[ST_FIRST] = t == 1.0 ? 1.0 : 0.0;
  const double b1t = pow(b1, t), b2t = pow(b2, t);
  const double bc1 = 1.0 - b1t, bc2 = 1.0 - b2t;
  double a = 0.0, b = 0.0, rect = 0.0, look = 0.0;
  if (mode == SSSEG_OPT_ADAM) {
    a = -(lr / bc1);
    b = sqrt(bc2);
  } else if (mode == SSSEG_OPT_RANGER) {
    const double n_max = 2.0 / (1.0 - b2) - 1.0;
    const double n_sma = n_max - 2.0 * t * b2t / (1.0 - b2t);
    double step;
    if (n_sma > nsma_thr) {
      rect = 1.0;
      step = sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) / bc1;
    } else {
      step = 1.0 / bc1;
    }
    a = -step * lr;
    b = -wd * lr;
    look = fmod(t, (double)k) == 0.0 ? 1.0 : 0.0;
  } else {
    a = lr * sqrt(bc2) / bc1;
    b = -wd * lr;
    if (mode == SSSEG_OPT_DIFFGRAD) a = -a;
  }
  st[ST_A] = a;
  st[ST_B] = b;
  st[ST_RECT] = rect;
  st[ST_LOOK] = look;
}

struct StepArgs {
  float* p;
  const float* g;
  float *m, *v, *s, *prev, *slow;
  int64_t n4;
  const double* st;
  float b1, omb1, b2, omb2, b3, omb3, eps, wd, alpha;
};

struct StepScalars {
  float coef, a, b;
  bool rect, look, first;
};

// diffGrad friction coefficient; 1./x and 9./x of the reference are reciprocal(x) * 1 and reciprocal(x) * 9
template <int VER>
__device__ __forceinline__ float dfc(float prev, float g) {
  float d = prev - g;
  if (VER == 0) d = fabsf(d);
  if (VER == 2) d = 0.5f * fabsf(d);
  const float c = 1.f / (1.f + expf(-d));
  return VER == 2 ? c * 9.f - 4.f : c;
}

// One element.  m == 0 contributes no update whatever the step size (0 * inf at eps == 0 would turn the arena's
// p = g = 0 padding slots into NaN).
template <int MODE, int VER>
__device__ __forceinline__ void update(const StepArgs& h, const StepScalars& c, float& p, float g, float& m, float& v,
                                       float& s, float& prev, float& slow) {
  g = g * c.coef;
  if (MODE == SSSEG_OPT_ADAM || MODE == SSSEG_OPT_DIFFGRAD) {
    if (h.wd != 0.f) g = fmaf(p, h.wd, g);
  }
  if (MODE == SSSEG_OPT_ADAM) {
    m = fmaf(h.omb1, g - m, m);
  } else {
    m = fmaf(g, h.omb1, m * h.b1);
  }
  v = fmaf(h.omb2 * g, g, v * h.b2);
  if (MODE == SSSEG_OPT_ADAM) {
    const float denom = sqrtf(v) / c.b + h.eps;
    const float u = (c.a * m) / denom;
    p = m == 0.f ? p : p + u;
    return;
  }
  const float denom = sqrtf(v) + h.eps;
  float mm = m;
  if (MODE == SSSEG_OPT_DIFFGRAD || MODE == SSSEG_OPT_DIFFMOD) {
    mm = m * dfc<VER>(prev, g);
    prev = g;
  }
  if (MODE == SSSEG_OPT_DIFFGRAD) {
    const float u = (c.a * mm) / denom;
    p = m == 0.f ? p : p + u;
    return;
  }
  if (MODE == SSSEG_OPT_RANGER && c.first) slow = p;
  if (c.b != 0.f) p = fmaf(p, c.b, p);
  if (MODE == SSSEG_OPT_ADAMOD || MODE == SSSEG_OPT_DIFFMOD) {
    const float eta = c.a / denom;
    s = fmaf(eta, h.omb3, s * h.b3);
    const float u = fminf(eta, s) * mm;
    p = m == 0.f ? p : p + (-u);
    return;
  }
  // Ranger: rectified (adaptive) or plain momentum step, then Lookahead every k-th step
  if (c.rect) {
    const float u = (c.a * m) / denom;
    p = m == 0.f ? p : p + u;
  } else {
    p = fmaf(m, c.a, p);
  }
  if (c.look) {
    slow = fmaf(p - slow, h.alpha, slow);
    p = slow;
  }
}

template <int MODE, int VER>
__global__ void __launch_bounds__(256) optim_step_kernel(StepArgs h) {
  constexpr bool HAS_S = MODE == SSSEG_OPT_ADAMOD || MODE == SSSEG_OPT_DIFFMOD;
  constexpr bool HAS_PREV = MODE == SSSEG_OPT_DIFFGRAD || MODE == SSSEG_OPT_DIFFMOD;
  using F4 = Chunk<float, 4>;   // every array is walked in 16-byte pieces, indexed as float4 (h.n4 of them)
  if (h.st[ST_SKIP] != 0.0) return;
  StepScalars c;
  c.coef = (float)h.st[ST_COEF];
  c.a = (float)h.st[ST_A];
  c.b = (float)h.st[ST_B];
  c.rect = h.st[ST_RECT] != 0.0;
  c.look = h.st[ST_LOOK] != 0.0;
  c.first = h.st[ST_FIRST] != 0.0;
  // slow is read on Lookahead steps (unless this step initialises it) and written on those and on the first step
  const bool slow_ld = MODE == SSSEG_OPT_RANGER && c.look && !c.first;
  const bool slow_st = MODE == SSSEG_OPT_RANGER && (c.look || c.first);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < h.n4; i += (int64_t)gridDim.x * blockDim.x) {
    float p[4], g[4], m[4], v[4], s[4] = {0.f, 0.f, 0.f, 0.f}, prev[4] = {0.f, 0.f, 0.f, 0.f},
                                  slow[4] = {0.f, 0.f, 0.f, 0.f};
    F4::cvt(((const float4*)h.p)[i], p);
    F4::cvt(((const float4*)h.g)[i], g);
    F4::cvt(((const float4*)h.m)[i], m);
    F4::cvt(((const float4*)h.v)[i], v);
    if (HAS_S) F4::cvt(((const float4*)h.s)[i], s);
    if (HAS_PREV) F4::cvt(((const float4*)h.prev)[i], prev);
    if (slow_ld) F4::cvt(((const float4*)h.slow)[i], slow);
#pragma unroll
    for (int j = 0; j < 4; ++j) update<MODE, VER>(h, c, p[j], g[j], m[j], v[j], s[j], prev[j], slow[j]);
    ((float4*)h.p)[i] = F4::pack(p);
    ((float4*)h.m)[i] = F4::pack(m);
    ((float4*)h.v)[i] = F4::pack(v);
    if (HAS_S) ((float4*)h.s)[i] = F4::pack(s);
    if (HAS_PREV) ((float4*)h.prev)[i] = F4::pack(prev);
    if (slow_st) ((float4*)h.slow)[i] = F4::pack(slow);
  }
}

template <int MODE, int VER>
void launch_step(const StepArgs& h, hipStream_t s) {
  hipLaunchKernelGGL((optim_step_kernel<MODE, VER>), dim3(ssseg_grid(h.n4, 256, 256 * 8)), dim3(256), 0, s, h);
}

template <int MODE>
void launch_step_version(int version, const StepArgs& h, hipStream_t s) {
  if (version == 0) launch_step<MODE, 0>(h, s);
  else if (version == 1) launch_step<MODE, 1>(h, s);
  else launch_step<MODE, 2>(h, s);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int ssseg_optim_prepare(double* state, int mode, double lr, double beta1, double beta2, double weight_decay,
                                   double max_norm, int64_t k, double nsma_threshold, const float* sqnorm,
                                   const float* amp_state, ssseg_stream_t stream) {
  if (!state || mode < SSSEG_OPT_ADAM || mode > SSSEG_OPT_RANGER || ((max_norm > 0.0 || amp_state) && !sqnorm) ||
      (mode == SSSEG_OPT_RANGER && k < 1))
    return SSSEG_EINVAL;
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, mode, lr, beta1, beta2,
                     weight_decay, max_norm, k, nsma_threshold, sqnorm, amp_state);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_optim_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* exp_avg_lr,
                                float* previous_grad, float* slow_buffer, int64_t n, int mode, int version,
                                double beta1, double beta2, double beta3, double eps, double weight_decay, double alpha,
                                const double* state, ssseg_stream_t stream) {
  const bool has_s = mode == SSSEG_OPT_ADAMOD || mode == SSSEG_OPT_DIFFMOD;
  const bool has_prev = mode == SSSEG_OPT_DIFFGRAD || mode == SSSEG_OPT_DIFFMOD;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !state || n < 0 || (n & 3) || mode < SSSEG_OPT_ADAM ||
      mode > SSSEG_OPT_RANGER || version < 0 || version > 2 || (has_s && !exp_avg_lr) ||
      (has_prev && !previous_grad) || (mode == SSSEG_OPT_RANGER && !slow_buffer))
    return SSSEG_EINVAL;
  if (!aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
      !aligned16(exp_avg_lr) || !aligned16(previous_grad) || !aligned16(slow_buffer))
    return SSSEG_EINVAL;
  if (n == 0) return 0;
  StepArgs h;
  h.p = param; h.g = grad; h.m = exp_avg; h.v = exp_avg_sq; h.s = exp_avg_lr; h.prev = previous_grad;
  h.slow = slow_buffer; h.n4 = n / 4; h.st = state;
  // the reference's Python-double scalars, rounded to fp32 once where a tensor op receives them
  h.b1 = (float)beta1; h.omb1 = (float)(1.0 - beta1); h.b2 = (float)beta2; h.omb2 = (float)(1.0 - beta2);
  h.b3 = (float)beta3; h.omb3 = (float)(1.0 - beta3); h.eps = (float)eps; h.wd = (float)weight_decay;
  h.alpha = (float)alpha;
  hipStream_t s = (hipStream_t)stream;
  switch (mode) {
    case SSSEG_OPT_ADAM: launch_step<SSSEG_OPT_ADAM, 0>(h, s); break;
    case SSSEG_OPT_ADAMOD: launch_step<SSSEG_OPT_ADAMOD, 0>(h, s); break;
    case SSSEG_OPT_DIFFGRAD: launch_step_version<SSSEG_OPT_DIFFGRAD>(version, h, s); break;
    case SSSEG_OPT_DIFFMOD: launch_step_version<SSSEG_OPT_DIFFMOD>(version, h, s); break;
    default: launch_step<SSSEG_OPT_RANGER, 0>(h, s); break;
  }
  SSSEG_LAUNCH_CHECK();
  return 0;
}
