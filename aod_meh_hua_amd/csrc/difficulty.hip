// Class difficulty: the training-side half of PPAL's Difficulty-Calibrated Uncertainty Sampling (C. Yang, L. Huang, E. J. Crowley,
// "Plug and Play Active Learning for Object Detection", CVPR 2024).  While the detector trains, a running per-class difficulty is kept from
// its positive samples; at acquisition time aod_det_uncertainty_w (det_unc.hip) weights every detection's measure by its class's difficulty.
// The reference tree has no such rule: the semantics are fixed in DESIGN 3p.
//
// Over the loss operands of aod_*_focal_l1_*_fwd (cls [nrows][C] fp32 logits, labels, label_w, bbox_pred / bbox_tgt [nrows][4] deltas):
//   positive    row r with 0 <= labels[r] < C and label_w[r] > 0; nothing else of any other row is read
//   P           form 0 (EDL heads): softmax(cls[r])[c], the maximum subtracted;  form 1 (MyRetinaHead): 1 / (1 + exp(-cls[r][c]));  c = labels[r]
//   IoU         of the decoded prediction and the decoded target in the anchor-normalised frame (both are decoded from the same anchor and IoU
//               does not change under a translation or a per-axis scaling, so no anchor is read): t = delta * std + mean, centre (t0, t1), size
//               (exp(clamp(t2)), exp(clamp(t3))), clamp to +-|ln(wh_ratio_clip)|;  ov / max(un, 1e-6) as in aod_loc_stability
//   q           1 - P^xi IoU^(1 - xi), 1 when P or IoU is 0, clamped to [0, 1]
//   S[c], n[c]  sum of q / count over the positives of class c
// aod_class_difficulty_accum  acc[c] += S[c], acc[C + c] += n[c] (n is an fp32 count: exact below 2^24 positives per class)
//   partials    a grid-stride loop over chunks of 1024 rows, 4 consecutive rows per thread (16-B label loads).  Per chunk the positives are
//               compacted in row order into LDS (wave ballots; the wave counts are double-buffered by chunk parity: one barrier per chunk
//               without a positive), the threads that found them compute q, then thread c walks the list and adds class c's q in row order.
//   reduce      one block: thread j adds the blocks' partials of word j in block order, then adds the sum into acc[j]
//   No atomics.  Chunks are cut on the row index (a labels pointer that is only 8-B aligned moves the 16-B loads, not the chunks), so every
//   sum's order depends on nrows and the row indices alone: the same inputs give the same bits on every run, eager or replayed.
// aod_class_difficulty_update  d[c] = m d[c] + (1 - m) S[c] / n[c] where n[c] > 0 (else d[c] keeps its bits); acc is zeroed
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define CD_TB 256
#define CD_RPT 4                       // rows per thread and chunk
#define CD_CHUNK (CD_TB * CD_RPT)
#define CD_MAX_C 128
#define CD_MAX_GRID 256

typedef __attribute__((ext_vector_type(2))) long long i64x2;

struct cd_coder { float mean[4], std[4]; float max_ratio; };

__device__ __forceinline__ float cd_sample(const float* __restrict__ x, int C, int c, int form, f32x4 dp, f32x4 dt, const cd_coder& k, float xi) {
  float P;
  if (form == 0) {
    float m = x[0];
    for (int i = 1; i < C; ++i) m = fmaxf(m, x[i]);
    float S = 0.f;
    for (int i = 0; i < C; ++i) S = __fadd_rn(S, expf(__fsub_rn(x[i], m)));
    P = __fdiv_rn(expf(__fsub_rn(x[c], m)), S);
  } else {
    P = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x[c])));
  }
  float b[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const f32x4 d = s ? dt : dp;
    const float cx = __fadd_rn(__fmul_rn(d[0], k.std[0]), k.mean[0]), cy = __fadd_rn(__fmul_rn(d[1], k.std[1]), k.mean[1]);
    const float tw = __fadd_rn(__fmul_rn(d[2], k.std[2]), k.mean[2]), th = __fadd_rn(__fmul_rn(d[3], k.std[3]), k.mean[3]);
    const float w = expf(fminf(fmaxf(tw, -k.max_ratio), k.max_ratio)), h = expf(fminf(fmaxf(th, -k.max_ratio), k.max_ratio));
    b[s][0] = __fsub_rn(cx, __fmul_rn(0.5f, w)); b[s][1] = __fsub_rn(cy, __fmul_rn(0.5f, h));
    b[s][2] = __fadd_rn(cx, __fmul_rn(0.5f, w)); b[s][3] = __fadd_rn(cy, __fmul_rn(0.5f, h));
  }
  const float aa = __fmul_rn(__fsub_rn(b[0][2], b[0][0]), __fsub_rn(b[0][3], b[0][1]));
  const float ab = __fmul_rn(__fsub_rn(b[1][2], b[1][0]), __fsub_rn(b[1][3], b[1][1]));
  const float iw = fmaxf(__fsub_rn(fminf(b[0][2], b[1][2]), fmaxf(b[0][0], b[1][0])), 0.f);
  const float ih = fmaxf(__fsub_rn(fminf(b[0][3], b[1][3]), fmaxf(b[0][1], b[1][1])), 0.f);
  const float ov = __fmul_rn(iw, ih);
  const float un = __fsub_rn(__fadd_rn(aa, ab), ov);
  const float iou = __fdiv_rn(ov, fmaxf(un, 1e-6f));
  if (!(P > 0.f) || !(iou > 0.f)) return 1.0f;
  const float q = __fsub_rn(1.0f, __fmul_rn(powf(P, xi), powf(iou, __fsub_rn(1.0f, xi))));
  return fminf(fmaxf(q, 0.f), 1.0f);
}

__global__ __launch_bounds__(CD_TB) void class_difficulty_partials_kernel(const float* __restrict__ cls, const long long* __restrict__ labels,
                                                                          const float* __restrict__ lw, const float* __restrict__ bp,
                                                                          const float* __restrict__ bt, long long nrows, int C, int form,
                                                                          cd_coder coder, float xi, float* __restrict__ ws) {
  __shared__ int wcnt[2][CD_TB / 64];
  __shared__ int lcls[CD_CHUNK];
  __shared__ float lq[CD_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool odd = ((reinterpret_cast<unsigned long long>(labels) >> 3) & 1ull) != 0;      // labels + r is 16-B aligned for odd r
  const unsigned long long below = (1ull << lane) - 1ull;
  const long long nchunks = (nrows + CD_CHUNK - 1) / CD_CHUNK;
  float s = 0.f, n = 0.f;
  int par = 0;
  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x, par ^= 1) {
    const long long r0 = chunk * CD_CHUNK + (long long)tid * CD_RPT;
    long long lab[CD_RPT];
#pragma unroll
    for (int u = 0; u < CD_RPT; ++u) lab[u] = -1;
    // rows r0 .. r0 + 3 (r0 is a multiple of 4): the 16-B loads sit on the even rows, or on the odd ones behind an 8-B aligned pointer
    if (!odd) {
#pragma unroll
      for (int u = 0; u < CD_RPT; u += 2) {
        if (r0 + u + 1 < nrows) {
          const i64x2 v = *reinterpret_cast<const i64x2*>(labels + r0 + u);
          lab[u] = v[0]; lab[u + 1] = v[1];
        } else if (r0 + u < nrows) {
          lab[u] = labels[r0 + u];
        }
      }
    } else {
      if (r0 < nrows) lab[0] = labels[r0];
      if (r0 + 2 < nrows) {
        const i64x2 v = *reinterpret_cast<const i64x2*>(labels + r0 + 1);
        lab[1] = v[0]; lab[2] = v[1];
      } else if (r0 + 1 < nrows) {
        lab[1] = labels[r0 + 1];
      }
      if (r0 + 3 < nrows) lab[3] = labels[r0 + 3];
    }
    bool pos[CD_RPT];
    int before = 0, mine = 0;
#pragma unroll
    for (int u = 0; u < CD_RPT; ++u) {
      pos[u] = lab[u] >= 0 && lab[u] < (long long)C && lw[r0 + u] > 0.f;      // (lab = -1 past the last row: nothing is read there)
      const unsigned long long bal = __ballot(pos[u]);
      before += __popcll(bal & below);
      mine += __popcll(bal);
    }
    if (lane == 0) wcnt[par][wave] = mine;
    __syncthreads();
    int tot = 0, off = before;
#pragma unroll
    for (int w = 0; w < CD_TB / 64; ++w) {
      const int v = wcnt[par][w];
      tot += v;
      if (w < wave) off += v;
    }
    if (tot == 0) continue;                                  // (uniform: every thread reads the same four counts)
#pragma unroll
    for (int u = 0; u < CD_RPT; ++u) {
      if (pos[u]) {
        const long long r = r0 + u;
        const int c = (int)lab[u];
        const f32x4 dp = *reinterpret_cast<const f32x4*>(bp + r * 4), dt = *reinterpret_cast<const f32x4*>(bt + r * 4);
        lcls[off] = c;
        lq[off] = cd_sample(cls + r * C, C, c, form, dp, dt, coder, xi);
        ++off;
      }
    }
    __syncthreads();
    if (tid < C) {
      for (int i = 0; i < tot; ++i)
        if (lcls[i] == tid) { s = __fadd_rn(s, lq[i]); n = __fadd_rn(n, 1.0f); }
    }
    __syncthreads();                                         // the list is free again
  }
  if (tid < C) {
    ws[(long long)blockIdx.x * 2 * C + tid] = s;
    ws[(long long)blockIdx.x * 2 * C + C + tid] = n;
  }
}

__global__ __launch_bounds__(CD_TB) void class_difficulty_reduce_kernel(const float* __restrict__ ws, int nblocks, int C, float* __restrict__ acc) {
  const int j = threadIdx.x;
  if (j >= 2 * C) return;
  float v = 0.f;
  int b = 0;
  for (; b + 16 <= nblocks; b += 16) {                       // 16 loads in flight, added in block order
    float t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = ws[(long long)(b + u) * 2 * C + j];
#pragma unroll
    for (int u = 0; u < 16; ++u) v = __fadd_rn(v, t[u]);
  }
  for (; b < nblocks; ++b) v = __fadd_rn(v, ws[(long long)b * 2 * C + j]);
  acc[j] = __fadd_rn(acc[j], v);
}

__global__ __launch_bounds__(CD_MAX_C) void class_difficulty_update_kernel(float* __restrict__ acc, float* __restrict__ d, int C, float momentum) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const float S = acc[c], n = acc[C + c];
  if (n > 0.f) d[c] = __fadd_rn(__fmul_rn(momentum, d[c]), __fmul_rn(__fsub_rn(1.0f, momentum), __fdiv_rn(S, n)));
  acc[c] = 0.f;
  acc[C + c] = 0.f;
}

static inline int cd_grid(int64_t nrows) {
  const int64_t nchunks = (nrows + CD_CHUNK - 1) / CD_CHUNK;
  return (int)(nchunks < CD_MAX_GRID ? nchunks : CD_MAX_GRID);
}

// workspace of aod_class_difficulty_accum, in floats: the blocks' partials [grid][2C]
extern "C" size_t aod_class_difficulty_ws_len(int64_t nrows, int C) {
  if (nrows <= 0 || C < 1 || C > CD_MAX_C) return 0;
  return (size_t)cd_grid(nrows) * 2 * (size_t)C;
}

extern "C" int aod_class_difficulty_accum(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                          const float* bbox_tgt, int64_t nrows, int C, int form, const float* means4, const float* stds4,
                                          float wh_ratio_clip, float xi, float* acc, float* ws, aod_stream_t stream) {
  AOD_CHECK_ARG(nrows >= 0, "class_difficulty_accum: negative row count");
  AOD_CHECK_ARG(C >= 1 && C <= CD_MAX_C, "class_difficulty_accum: C must be in 1..%d (got %d)", CD_MAX_C, C);
  AOD_CHECK_ARG(form == 0 || form == 1, "class_difficulty_accum: form %d is none of 0 (softmax), 1 (sigmoid)", form);
  AOD_CHECK_ARG(xi >= 0.f && xi <= 1.f, "class_difficulty_accum: xi must be in [0, 1] (got %g)", (double)xi);
  AOD_CHECK_ARG(wh_ratio_clip > 0.f && wh_ratio_clip <= 3.4028234e38f, "class_difficulty_accum: wh_ratio_clip must be finite and > 0 (got %g)",
                (double)wh_ratio_clip);
  AOD_CHECK_ARG(means4 && stds4, "class_difficulty_accum: null pointer (means4 / stds4)");
  cd_coder k;
  for (int i = 0; i < 4; ++i) {
    AOD_CHECK_ARG(fabsf(means4[i]) <= 3.4028234e38f && fabsf(stds4[i]) <= 3.4028234e38f, "class_difficulty_accum: means4[%d] / stds4[%d] is not finite", i,
                  i);
    k.mean[i] = means4[i];
    k.std[i] = stds4[i];
  }
  k.max_ratio = fabsf(logf(wh_ratio_clip));
  AOD_CHECK_ARG(acc, "class_difficulty_accum: null pointer (acc)");
  AOD_CHECK_ARG((((size_t)acc) & 3) == 0, "class_difficulty_accum: acc must be aligned to its element size");
  if (nrows == 0) return 0;
  AOD_CHECK_ARG(cls && labels && label_w && bbox_pred && bbox_tgt && ws, "class_difficulty_accum: null pointer");
  AOD_CHECK_ARG(((((size_t)cls) | ((size_t)label_w) | ((size_t)ws)) & 3) == 0 && (((size_t)labels) & 7) == 0 &&
                    ((((size_t)bbox_pred) | ((size_t)bbox_tgt)) & 15) == 0,
                "class_difficulty_accum: cls / label_w / ws must be 4-B, labels 8-B, bbox_pred / bbox_tgt 16-B aligned");
  const int grid = cd_grid(nrows);
  hipLaunchKernelGGL(class_difficulty_partials_kernel, dim3((unsigned)grid), dim3(CD_TB), 0, (hipStream_t)stream, cls, (const long long*)labels, label_w,
                     bbox_pred, bbox_tgt, (long long)nrows, C, form, k, xi, ws);
  hipLaunchKernelGGL(class_difficulty_reduce_kernel, dim3(1), dim3(CD_TB), 0, (hipStream_t)stream, ws, grid, C, acc);
  AOD_LAUNCH_CHECK();
  return 0;
}

extern "C" int aod_class_difficulty_update(float* acc, float* d, int C, float momentum, aod_stream_t stream) {
  AOD_CHECK_ARG(C >= 1 && C <= CD_MAX_C, "class_difficulty_update: C must be in 1..%d (got %d)", CD_MAX_C, C);
  AOD_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "class_difficulty_update: momentum must be in [0, 1] (got %g)", (double)momentum);
  AOD_CHECK_ARG(acc && d, "class_difficulty_update: null pointer");
  AOD_CHECK_ARG(((((size_t)acc) | ((size_t)d)) & 3) == 0, "class_difficulty_update: pointers must be aligned to their element size");
  hipLaunchKernelGGL(class_difficulty_update_kernel, dim3(1), dim3(CD_MAX_C), 0, (hipStream_t)stream, acc, d, C, momentum);
  AOD_LAUNCH_CHECK();
  return 0;
}
