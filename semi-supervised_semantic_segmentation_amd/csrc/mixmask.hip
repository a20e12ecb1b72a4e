// ClassMix (Olsson et al. 2021) and CutMix (French et al. 2020) masks for the consistency branch, for gfx950 (wave64).
//
// ClassMix, per call (all on `stream`, no host sync, graph-capturable):
//   memset(present) -> label (argmax over C, one byte per pixel, 64-bit presence word per image)
//   -> select (one wave per image: the ceil(n/2) present classes with the smallest (key, class))
//   -> write (mask = bit `label` of the chosen word).
// HBM traffic: read B*C*HW logits once, write + read B*HW label bytes, write B*HW*4 mask bytes.
// CutMix, per call: one launch; every workgroup derives its image's box in fp64 and writes its pixel tiles.
// The random inputs (a 31-bit key per image and class, four uniforms per image) come from Philox on CowMix's per-device
// seed and counter (ssseg_mixmask_draw_dev), so a captured step replays fresh masks.
#include "common.h"
#include "philox.h"

namespace {

constexpr int MM_TILE = 256;          // pixels of one image per workgroup round: one pixel per thread
constexpr int MM_BLOCKS = 1024;       // workgroups of the label and write kernels, shared among the images
constexpr int CUT_BLOCKS_X = 64;      // workgroups per image of the CutMix kernel

struct ClassmixWs {
  unsigned char* labels;          // [B][HW]
  unsigned long long* present;    // [B]
  unsigned long long* chosen;     // [B]
  int* nk;                        // [B][2]: n = classes present, k = classes chosen
};

size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

size_t carve(ClassmixWs* w, void* base, int64_t B, int64_t HW) {
  char* p = (char*)base;
  size_t off = 0;
  if (w) w->labels = (unsigned char*)(p + off);
  off = align16(off + (size_t)B * HW);
  if (w) w->present = (unsigned long long*)(p + off);
  off = align16(off + sizeof(unsigned long long) * B);
  if (w) w->chosen = (unsigned long long*)(p + off);
  off = align16(off + sizeof(unsigned long long) * B);
  if (w) w->nk = (int*)(p + off);
  off = align16(off + sizeof(int) * 2 * B);
  return off;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// grid (x: workgroups of the image, y: image): a workgroup walks 256-pixel tiles of ONE image grid-strided, so there is
// no division and its presence bits belong to one word.  Each thread owns one pixel of a tile and holds its CMAX logits
// in a register row: every load is issued before the first comparison, each coalesced across the wave at channel
// stride `sc` (HW for NCHW).  torch.argmax's rule: the first maximum wins, NaN counts as the maximum (the first NaN
// wins).  The presence bits are ORed per thread over the walk, then once per workgroup: wave OR -> one LDS atomic per
// wave -> one global atomic per workgroup.
template <int CMAX, typename T>
__global__ void __launch_bounds__(MM_TILE) classmix_label_kernel(const T* __restrict__ logits, int64_t sb, int64_t sc,
                                                                 int64_t sp, int C, int64_t HW,
                                                                 unsigned char* __restrict__ labels,
                                                                 unsigned long long* __restrict__ present) {
  __shared__ unsigned long long wg_bits;
  if (threadIdx.x == 0) wg_bits = 0ull;
  __syncthreads();
  const int64_t b = blockIdx.y;
  const T* lb = logits + b * sb;
  unsigned char* out = labels + b * HW;
  unsigned long long bits = 0ull;
  for (int64_t pix = (int64_t)blockIdx.x * MM_TILE + threadIdx.x; pix < HW; pix += (int64_t)gridDim.x * MM_TILE) {
    const T* p = lb + pix * sp;
    float v[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) v[c] = io<T>::ld(p, (int64_t)(c < C ? c : 0) * sc);   // clamped, no branch
    float best = v[0];
    int arg = 0;
#pragma unroll
    for (int c = 1; c < CMAX; ++c) {
      const bool take = c < C && best == best && (v[c] > best || v[c] != v[c]);
      best = take ? v[c] : best;
      arg = take ? c : arg;
    }
    out[pix] = (unsigned char)arg;
    bits |= 1ull << arg;
  }
  bits = wave_or(bits);
  if ((threadIdx.x & 63) == 0 && bits) atomicOr(&wg_bits, bits);
  __syncthreads();
  if (threadIdx.x == 0 && wg_bits) atomicOr(present + b, wg_bits);
}

// One wave per image, one lane per class.  n = popcount(present), k = ceil(n/2); lane c is chosen where class c is
// present and fewer than k present classes come before it in the order of (key, class); keys are signed int32.
__global__ void __launch_bounds__(64) classmix_select_kernel(const unsigned long long* __restrict__ present,
                                                             const int* __restrict__ keys, int C,
                                                             unsigned long long* __restrict__ chosen,
                                                             int* __restrict__ nk,
                                                             unsigned long long* __restrict__ present_out,
                                                             unsigned long long* __restrict__ chosen_out) {
  const int b = blockIdx.x, c = threadIdx.x;
  const unsigned long long pres = present[b];
  const int n = __popcll(pres), k = (n + (n & 1)) / 2;
  const int key = c < C ? keys[(int64_t)b * C + c] : 0x7fffffff;
  const bool mine = (pres >> c) & 1ull;
  int rank = 0;
  for (int j = 0; j < 64; ++j) {
    const int kj = __shfl(key, j, 64);
    const bool pj = (pres >> j) & 1ull;
    rank += (pj && (kj < key || (kj == key && j < c))) ? 1 : 0;
  }
  const unsigned long long ch = __ballot(mine && rank < k);
  if (c == 0) {
    chosen[b] = ch;
    nk[2 * b] = n;
    nk[2 * b + 1] = k;
    if (present_out) present_out[b] = pres;
    if (chosen_out) chosen_out[b] = ch;
  }
}

// the label kernel's grid and walk
__global__ void __launch_bounds__(MM_TILE) classmix_write_kernel(const unsigned char* __restrict__ labels,
                                                                 const unsigned long long* __restrict__ chosen,
                                                                 int64_t HW, float* __restrict__ mask) {
  const int64_t b = blockIdx.y;
  const unsigned long long ch = chosen[b];
  const unsigned char* lb = labels + b * HW;
  float* mb = mask + b * HW;
  for (int64_t pix = (int64_t)blockIdx.x * MM_TILE + threadIdx.x; pix < HW; pix += (int64_t)gridDim.x * MM_TILE)
    mb[pix] = (float)((ch >> lb[pix]) & 1ull);
}

// grid (x: workgroups of the image, y: image).  Thread 0 derives the image's box once per workgroup in fp64:
//   p = lo + (hi - lo) p',  h = rint(H p^u),  w = rint(W p^(1-u)),  top = rint((H - h) v1),  left = rint((W - w) v2)
// (rint rounds half to even), then the workgroup walks its tiles; HW < 2^31, so the row of a pixel is one 32-bit
// division.  boxes (nullable) [B][4] int32: top, left, h, w.
__global__ void __launch_bounds__(MM_TILE) cutmix_mask_kernel(const float* __restrict__ params, int H, int W,
                                                              double lo, double hi, float* __restrict__ mask,
                                                              int* __restrict__ boxes) {
  __shared__ int box[4];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    const float* q = params + 4 * (int64_t)b;
    const double pp = (double)q[0], u = (double)q[1], v1 = (double)q[2], v2 = (double)q[3];
    const double p = lo + (hi - lo) * pp;
    const double h = rint((double)H * pow(p, u)), w = rint((double)W * pow(p, 1.0 - u));
    const double top = rint(((double)H - h) * v1), left = rint(((double)W - w) * v2);
    box[0] = (int)top;
    box[1] = (int)left;
    box[2] = (int)h;
    box[3] = (int)w;
    if (boxes && blockIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) boxes[4 * (int64_t)b + i] = box[i];
    }
  }
  __syncthreads();
  const unsigned top = (unsigned)box[0], left = (unsigned)box[1], h = (unsigned)box[2], w = (unsigned)box[3];
  const unsigned HW = (unsigned)H * (unsigned)W;
  float* mb = mask + (int64_t)b * HW;
  for (unsigned pix = blockIdx.x * MM_TILE + threadIdx.x; pix < HW; pix += gridDim.x * MM_TILE) {
    const unsigned y = pix / (unsigned)W, x = pix - y * (unsigned)W;
    // unsigned wrap-around: y - top < h  <=>  top <= y < top + h
    mb[pix] = (y - top < h && x - left < w) ? 1.f : 0.f;
  }
}

// Streams 3 and 4 of the key (0: CowMix noise, 1: CowMix p / sigma, 2: the affine views).  Item i < B*Q (Q = ceil(C/4))
// is the Philox block at counter offset + i of stream 3: four 31-bit keys of image i / Q, classes 4 (i % Q) ...;
// item B*Q + b is the block at counter offset + B*Q + b of stream 4: the four 24-bit uniforms of image b.
__global__ void __launch_bounds__(256) mixmask_draw_kernel(int* __restrict__ keys, float* __restrict__ params,
                                                           int64_t B, int C, int Q, uint64_t seed,
                                                           const unsigned long long* __restrict__ offset_dev) {
  const uint64_t offset = (uint64_t)*offset_dev;
  const int64_t total = B * (Q + 1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < B * Q ? !keys : !params) continue;   // an output that is not asked for keeps its counters
    unsigned c[4];
    if (i < B * Q) {
      philox_block(c, offset + (uint64_t)i, 3u);
      philox4x32_10(c, seed);
      const int64_t b = i / Q;
      const int c0 = 4 * (int)(i - b * Q);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) keys[b * C + c0 + j] = (int)(c[j] & 0x7fffffffu);
    } else {
      philox_block(c, offset + (uint64_t)i, 4u);
      philox4x32_10(c, seed);
      const int64_t b = i - B * Q;
#pragma unroll
      for (int j = 0; j < 4; ++j) params[4 * b + j] = philox_u01(c[j]);
    }
  }
}

__global__ void mixmask_advance_kernel(unsigned long long* offset_dev, unsigned long long inc) { *offset_dev += inc; }

template <int CMAX>
int launch_label(int dt, dim3 grid, hipStream_t st, const void* logits, int64_t sb, int64_t sc, int64_t sp, int C,
                 int64_t HW, unsigned char* labels, unsigned long long* present) {
  if (dt == SSSEG_F32)
    hipLaunchKernelGGL((classmix_label_kernel<CMAX, float>), grid, dim3(MM_TILE), 0, st, (const float*)logits, sb,
                       sc, sp, C, HW, labels, present);
  else if (dt == SSSEG_BF16)
    hipLaunchKernelGGL((classmix_label_kernel<CMAX, bf16_t>), grid, dim3(MM_TILE), 0, st, (const bf16_t*)logits,
                       sb, sc, sp, C, HW, labels, present);
  else
    hipLaunchKernelGGL((classmix_label_kernel<CMAX, f16_t>), grid, dim3(MM_TILE), 0, st, (const f16_t*)logits, sb,
                       sc, sp, C, HW, labels, present);
  return 0;
}

}  // namespace

extern "C" size_t ssseg_classmix_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return carve(nullptr, nullptr, B, H * W);
}

extern "C" int ssseg_classmix_mask(const void* logits, const int64_t* strides4, int dt, const int* keys, int64_t B,
                                   int64_t C, int64_t H, int64_t W, float* mask_out,
                                   unsigned long long* present_out, unsigned long long* chosen_out, void* workspace,
                                   size_t workspace_bytes, ssseg_stream_t stream) {
  if (!logits || !strides4 || !keys || !mask_out || B < 1 || C < 1 || C > 64 || H < 1 || W < 1) return SSSEG_EINVAL;
  if (dt != SSSEG_F32 && dt != SSSEG_BF16 && dt != SSSEG_F16) return SSSEG_EUNSUPPORTED;
  if (B > 65535 || B > (INT64_MAX / 64) / H / W / 64) return SSSEG_EUNSUPPORTED;
  // the pixels of an image lie at one stride (NCHW-contiguous and channels-last both do); other views are copied by
  // the caller
  if (strides4[2] != W * strides4[3] && H != 1) return SSSEG_EUNSUPPORTED;
  if (!workspace || workspace_bytes < ssseg_classmix_workspace_bytes(B, H, W)) return SSSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = H * W;
  ClassmixWs w;
  carve(&w, workspace, B, HW);
  SSSEG_TRY(hipMemsetAsync(w.present, 0, sizeof(unsigned long long) * B, st));
  // MM_BLOCKS workgroups over the B images at the most (one per image at the least), no more than an image has tiles
  const int64_t tpi = (HW + MM_TILE - 1) / MM_TILE, per = MM_BLOCKS / B > 1 ? MM_BLOCKS / B : 1;
  const dim3 grid((unsigned)(tpi < per ? tpi : per), (unsigned)B);
  const int64_t sb = strides4[0], sc = strides4[1], sp = strides4[3];
#define MM_LABEL(N) launch_label<N>(dt, grid, st, logits, sb, sc, sp, (int)C, HW, w.labels, w.present)
  if (C <= 2) MM_LABEL(2);
  else if (C <= 4) MM_LABEL(4);
  else if (C <= 8) MM_LABEL(8);
  else if (C <= 16) MM_LABEL(16);
  else if (C <= 32) MM_LABEL(32);
  else MM_LABEL(64);
#undef MM_LABEL
  hipLaunchKernelGGL(classmix_select_kernel, dim3((unsigned)B), dim3(64), 0, st,
                     (const unsigned long long*)w.present, keys, (int)C, w.chosen, w.nk, present_out, chosen_out);
  hipLaunchKernelGGL(classmix_write_kernel, grid, dim3(MM_TILE), 0, st, (const unsigned char*)w.labels,
                     (const unsigned long long*)w.chosen, HW, mask_out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_cutmix_mask(const float* params, int64_t B, int64_t H, int64_t W, double lo, double hi,
                                 float* mask_out, int* boxes_out, ssseg_stream_t stream) {
  if (!params || !mask_out || B < 1 || H < 1 || W < 1 || !(lo >= 0.0) || !(hi >= lo) || !(hi <= 1.0))
    return SSSEG_EINVAL;
  if (B > 65535 || H > 0x7fffffff / W) return SSSEG_EUNSUPPORTED;
  int64_t bx = (H * W + MM_TILE - 1) / MM_TILE;
  if (bx > CUT_BLOCKS_X) bx = CUT_BLOCKS_X;
  hipLaunchKernelGGL(cutmix_mask_kernel, dim3((unsigned)bx, (unsigned)B), dim3(MM_TILE), 0, (hipStream_t)stream,
                     params, (int)H, (int)W, lo, hi, mask_out, boxes_out);
  SSSEG_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssseg_mixmask_draw_dev(int* keys, float* params, int64_t B, int64_t C, uint64_t seed,
                                      unsigned long long* offset_dev, ssseg_stream_t stream) {
  if ((!keys && !params) || !offset_dev || B < 1 || B > 0x7fffffff || C < 1 || C > 64) return SSSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int Q = (int)((C + 3) / 4);
  const int64_t total = B * (Q + 1);
  hipLaunchKernelGGL(mixmask_draw_kernel, dim3(ssseg_grid(total, 256)), dim3(256), 0, st, keys, params, B, (int)C, Q,
                     seed, (const unsigned long long*)offset_dev);
  // a function of (B, C) only, whichever outputs are asked for: B * (ceil(C/4) + 1)
  hipLaunchKernelGGL(mixmask_advance_kernel, dim3(1), dim3(1), 0, st, offset_dev, (unsigned long long)total);
  SSSEG_LAUNCH_CHECK();
  return 0;
}
