// Device form of tpfp_default (mmdet/core/evaluation/mean_ap.py:154-239, area_ranges=None) for a whole batch, every class and up to 8 IoU
// thresholds in one launch: the input is what aod_multiclass_nms leaves on the device (dets [B,M,5], labels [B,M] int64, num [B]) plus the
// batch's packed ground truth, the output is one flag per (threshold, image, detection row): 0 neither, 1 true positive, 2 false positive.
//
// One workgroup of 256 threads per image; a detection row belongs to thread (row mod 256).
//   1. scores / labels of the rows < num[b] go to LDS (rows >= num[b] are padding: never read).
//   2. the image's gts are staged through LDS in chunks of 64 (G is unbounded); every row keeps a running (best_iou, best_gt, ignored) over
//      the gts of ITS class -- strict `>` keeps the first index of the maximum across chunks, numpy's argmax rule.  The host stacks a
//      class's real gts above its ignored ones; the packed list (real gts, then ignored gts, each in annotation order) filtered by class
//      has that order.
//   3. rank of a row = number of same-label rows with a greater score, or an equal score and a lower row (a stable descending order;
//      O(M^2) per image, nothing at M <= 300; the rows need not arrive sorted).
//   4. per threshold: a row without a gt of its class, or with best_iou < thr, is fp; a row whose best gt is ignored is neither; the other
//      rows claim their gt with an LDS atomicMin of the rank (gt chunk by gt chunk), the claimant that holds the minimum is tp, the rest fp.
//
// IoU restates bbox_overlaps (bbox_overlaps.py:4-48) in fp32 op by op: area = (x2-x1)*(y2-y1); overlap = max(xe-xs,0)*max(ye-ys,0);
// union = (a_det + a_gt) - overlap; iou = overlap / max(union, 1e-6f) with an IEEE divide.  The _rn intrinsics name the roundings;
// bit-exactness relies on build.py's -ffp-contract=off (see image_xform.hip).
#include <limits.h>

#include "common.h"

namespace {

constexpr int EM_THREADS = 256;
constexpr int EM_GCHUNK = 64;
constexpr int EM_MAX_T = 8;
constexpr int EM_MAX_M = 2048;          // 24 B of LDS per detection row

struct em_thr_t {
  float v[EM_MAX_T];
};

__global__ __launch_bounds__(EM_THREADS) void eval_match_kernel(const float* __restrict__ dets, const int64_t* __restrict__ labels,
                                                                const int32_t* __restrict__ num, const float* __restrict__ gt_boxes,
                                                                const int32_t* __restrict__ gt_labels, const uint8_t* __restrict__ gt_ignore,
                                                                const int32_t* __restrict__ gt_num, int B, int M, int G, em_thr_t thr, int T,
                                                                uint8_t* __restrict__ flags) {
  extern __shared__ __align__(16) unsigned char em_lds[];
  float* s_score = reinterpret_cast<float*>(em_lds);          // [M]
  int* s_label = reinterpret_cast<int*>(s_score + M);         // [M]
  float* s_biou = reinterpret_cast<float*>(s_label + M);      // [M]
  int* s_best = reinterpret_cast<int*>(s_biou + M);           // [M] packed gt index of the best gt, -1: no gt of the row's class
  int* s_bign = s_best + M;                                   // [M] the best gt is an ignored one
  int* s_rank = s_bign + M;                                   // [M]
  __shared__ float g_box[EM_GCHUNK][4];
  __shared__ int g_label[EM_GCHUNK];
  __shared__ int g_ign[EM_GCHUNK];
  __shared__ int g_first[EM_GCHUNK];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(max(num[b], 0), M);
  const int ng = min(max(gt_num[b], 0), G);
  const float* drow = dets + (size_t)b * M * 5;
  const int64_t* lrow = labels + (size_t)b * M;

  for (int m = tid; m < n; m += EM_THREADS) {
    s_score[m] = drow[m * 5 + 4];
    s_label[m] = (int)lrow[m];
    s_biou[m] = -1.f;
    s_best[m] = -1;
    s_bign[m] = 0;
  }
  __syncthreads();

  // 2. best gt of the row's own class
  for (int g0 = 0; g0 < ng; g0 += EM_GCHUNK) {
    const int gc = min(EM_GCHUNK, ng - g0);
    if (tid < gc) {
      const size_t gi = (size_t)b * G + g0 + tid;
      g_box[tid][0] = gt_boxes[gi * 4 + 0];
      g_box[tid][1] = gt_boxes[gi * 4 + 1];
      g_box[tid][2] = gt_boxes[gi * 4 + 2];
      g_box[tid][3] = gt_boxes[gi * 4 + 3];
      g_label[tid] = gt_labels[gi];
      g_ign[tid] = gt_ignore[gi] ? 1 : 0;
    }
    __syncthreads();
    for (int m = tid; m < n; m += EM_THREADS) {
      const float x1 = drow[m * 5 + 0], y1 = drow[m * 5 + 1], x2 = drow[m * 5 + 2], y2 = drow[m * 5 + 3];
      const float a_det = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
      const int lab = s_label[m];
      float biou = s_biou[m];
      int best = s_best[m], bign = s_bign[m];
      for (int j = 0; j < gc; ++j) {
        if (g_label[j] != lab) continue;
        const float gx1 = g_box[j][0], gy1 = g_box[j][1], gx2 = g_box[j][2], gy2 = g_box[j][3];
        const float a_gt = __fmul_rn(__fsub_rn(gx2, gx1), __fsub_rn(gy2, gy1));
        const float xs = fmaxf(x1, gx1), ys = fmaxf(y1, gy1), xe = fminf(x2, gx2), ye = fminf(y2, gy2);
        const float ov = __fmul_rn(fmaxf(__fsub_rn(xe, xs), 0.f), fmaxf(__fsub_rn(ye, ys), 0.f));
        const float un = __fsub_rn(__fadd_rn(a_det, a_gt), ov);
        const float iou = __fdiv_rn(ov, fmaxf(un, 1e-6f));
        if (iou > biou) {
          biou = iou;
          best = g0 + j;
          bign = g_ign[j];
        }
      }
      s_biou[m] = biou;
      s_best[m] = best;
      s_bign[m] = bign;
    }
    __syncthreads();
  }

  // 3. stable rank by descending score inside (image, label)
  for (int m = tid; m < n; m += EM_THREADS) {
    const float s = s_score[m];
    const int lab = s_label[m];
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s_score[j];
      r += (s_label[j] == lab && (sj > s || (sj == s && j < m))) ? 1 : 0;
    }
    s_rank[m] = r;
  }
  __syncthreads();

  // 4. flags, threshold by threshold (best gt and best IoU do not depend on the threshold)
  for (int t = 0; t < T; ++t) {
    const float th = thr.v[t];
    uint8_t* frow = flags + ((size_t)t * B + b) * M;
    for (int m = tid; m < M; m += EM_THREADS) {
      uint8_t f = 0;
      if (m < n) {
        if (s_best[m] < 0 || !(s_biou[m] >= th)) f = 2;          // claimants of a countable gt are decided below
      }
      frow[m] = f;
    }
    for (int g0 = 0; g0 < ng; g0 += EM_GCHUNK) {
      if (tid < EM_GCHUNK) g_first[tid] = INT_MAX;
      __syncthreads();
      for (int m = tid; m < n; m += EM_THREADS) {
        const int k = s_best[m] - g0;
        if (k >= 0 && k < EM_GCHUNK && s_biou[m] >= th && !s_bign[m]) atomicMin(&g_first[k], s_rank[m]);
      }
      __syncthreads();
      for (int m = tid; m < n; m += EM_THREADS) {
        const int k = s_best[m] - g0;
        if (k >= 0 && k < EM_GCHUNK && s_biou[m] >= th && !s_bign[m]) frow[m] = (s_rank[m] == g_first[k]) ? 1 : 2;
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int aod_eval_match(const float* dets, const int64_t* labels, const int32_t* num, const float* gt_boxes, const int32_t* gt_labels,
                              const uint8_t* gt_ignore, const int32_t* gt_num, int B, int M, int G, const float* iou_thr_host, int T,
                              uint8_t* flags, aod_stream_t stream) {
  AOD_CHECK_ARG(iou_thr_host && T >= 1 && T <= EM_MAX_T, "eval_match: 1..8 IoU thresholds (got %d)", T);
  AOD_CHECK_ARG(B >= 0 && M >= 0 && G >= 0, "eval_match: bad shape B=%d M=%d G=%d", B, M, G);
  AOD_CHECK_ARG(M <= EM_MAX_M, "eval_match: at most %d detection rows per image (got %d)", EM_MAX_M, M);
  if (B == 0 || M == 0) return 0;
  AOD_CHECK_ARG(dets && labels && num && gt_num && flags, "eval_match: null pointer");
  AOD_CHECK_ARG(G == 0 || (gt_boxes && gt_labels && gt_ignore), "eval_match: null gt pointer with G=%d", G);
  em_thr_t thr;
  for (int t = 0; t < EM_MAX_T; ++t) thr.v[t] = t < T ? iou_thr_host[t] : 0.f;
  const size_t lds = (size_t)M * 24;
  hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)B), dim3(EM_THREADS), lds, (hipStream_t)stream, dets, labels, num, gt_boxes, gt_labels,
                     gt_ignore, gt_num, B, M, G, thr, T, flags);
  AOD_LAUNCH_CHECK();
  return 0;
}
