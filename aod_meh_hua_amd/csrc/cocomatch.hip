// Device form of the COCO bbox matching of core/coco_eval.py match_image for a whole batch, every class, A (<= 4) area ranges
// and T (<= 16) IoU thresholds in one launch: the input is what aod_multiclass_nms leaves on the device (dets [B,M,5], labels [B,M] int64,
// num [B]) plus the batch's packed ground truth (xywh boxes, the file's area, class, crowd flag, all in file order), the output is one state
// per (range, threshold, image, detection row): 1 matched to a counted gt (tp), 0 unmatched and counted (fp), 2 ignored.
//
// One workgroup of 256 threads per image.
//   1. scores / labels of the rows < num[b] and the image's gts go to LDS once (rows >= num[b] are padding: never read, their states are 0).
//   2. rank of a row = number of rows of the image with a greater score, or an equal score and a lower row.  The matching of a class reads
//      the gts of that class only, so walking ALL rows in this one order walks every class in its own stable descending order.
//   3. per row in rank order: all threads write the row's IoU with every gt of its class to LDS (fp64, recomputed per row: an M x G matrix
//      would not fit), then the A*T greedy matchers -- lane a*T + t of the first wave, each with its own matched-gt bitmask in LDS -- scan
//      that column: first the gts the range counts, then (only without a match) the ignored ones; `>=` lets a later gt with an equal IoU
//      replace an earlier one, a crowd gt may be matched again.
// No atomics, no host sync, nothing waits on another workgroup.
//
// IoU restates coco_eval.iou_matrix in fp64 op by op: w = x2 - x1 after the promotion of the fp32 row; iw = min(dx+dw, gx+gw) - max(dx, gx);
// inter = iw*ih; union = d_area (crowd) or (d_area + gw*gh) - inter; iou = inter / union with an IEEE divide.  Bit-exactness relies on
// build.py's -ffp-contract=off (see image_xform.hip): a threshold met exactly is decided as numpy decides it.
#include "common.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_MAX_T = 16;
constexpr int CM_MAX_A = 4;
constexpr int CM_MAX_M = 1024;          // 12 B of LDS per detection row
constexpr int CM_MAX_G = 512;           // 53 B of LDS per gt + one mask bit per matcher
constexpr int CM_WORDS = CM_MAX_G / 32;
constexpr int CM_LANES = CM_MAX_T * CM_MAX_A;

struct cm_par_t {
  double thr[CM_MAX_T];
  double lo[CM_MAX_A];
  double hi[CM_MAX_A];
};

__global__ __launch_bounds__(CM_THREADS) void coco_match_kernel(const float* __restrict__ dets, const int64_t* __restrict__ labels,
                                                                const int32_t* __restrict__ num, const double* __restrict__ gt_boxes,
                                                                const double* __restrict__ gt_area, const int32_t* __restrict__ gt_label,
                                                                const uint8_t* __restrict__ gt_crowd, const int32_t* __restrict__ gt_num,
                                                                int B, int M, int G, cm_par_t par, int A, int T, uint8_t* __restrict__ states) {
  extern __shared__ __align__(16) unsigned char cm_lds[];
  double* g_box = reinterpret_cast<double*>(cm_lds);            // [G][4] xywh
  double* g_area = g_box + (size_t)G * 4;                       // [G] the file's area (the range test reads it, not w*h)
  double* s_iou = g_area + G;                                   // [G] IoU of the current row, -1: gt of another class
  float* s_score = reinterpret_cast<float*>(s_iou + G);         // [M]
  int* s_label = reinterpret_cast<int*>(s_score + M);           // [M]
  int* s_order = s_label + M;                                   // [M] row at rank r
  int* g_lab = s_order + M;                                     // [G]
  unsigned char* g_crowd = reinterpret_cast<unsigned char*>(g_lab + G);      // [G]
  __shared__ unsigned s_mask[CM_WORDS * CM_LANES];              // matched-gt bits, word-major: [word][lane]

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(max(num[b], 0), M);
  const int ng = min(max(gt_num[b], 0), G);
  const int AT = A * T;
  const float* drow = dets + (size_t)b * M * 5;
  const int64_t* lrow = labels + (size_t)b * M;

  for (int m = tid; m < n; m += CM_THREADS) {
    s_score[m] = drow[m * 5 + 4];
    s_label[m] = (int)lrow[m];
    s_order[m] = m;          // (NaN scores give no permutation below: every entry still names a row of this image, but some rows are then
                             //  visited twice and others never -- their states stay what the caller put there, see aod_hip.h)
  }
  for (int g = tid; g < ng; g += CM_THREADS) {
    const size_t gi = (size_t)b * G + g;
    g_box[g * 4 + 0] = gt_boxes[gi * 4 + 0];
    g_box[g * 4 + 1] = gt_boxes[gi * 4 + 1];
    g_box[g * 4 + 2] = gt_boxes[gi * 4 + 2];
    g_box[g * 4 + 3] = gt_boxes[gi * 4 + 3];
    g_area[g] = gt_area[gi];
    g_lab[g] = gt_label[gi];
    g_crowd[g] = gt_crowd[gi] ? 1 : 0;
  }
  for (int i = tid; i < CM_WORDS * CM_LANES; i += CM_THREADS) s_mask[i] = 0u;
  // padding rows: state 0 in every (range, threshold) plane
  for (int p = 0; p < AT; ++p) {
    uint8_t* srow = states + ((size_t)p * B + b) * M;
    for (int m = n + tid; m < M; m += CM_THREADS) srow[m] = 0;
  }
  __syncthreads();

  // 2. stable descending order over the image's rows
  for (int m = tid; m < n; m += CM_THREADS) {
    const float s = s_score[m];
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s_score[j];
      r += (sj > s || (sj == s && j < m)) ? 1 : 0;
    }
    s_order[r] = m;
  }
  __syncthreads();

  // the matcher of this lane
  const bool matcher = tid < AT;
  const int a = matcher ? tid / T : 0;
  const int t = matcher ? tid - a * T : 0;
  const double lo = par.lo[a], hi = par.hi[a];
  const double b0 = fmin(par.thr[t], 1.0 - 1e-10);
  uint8_t* mine = states + ((size_t)(matcher ? tid : 0) * B + b) * M;

  for (int r = 0; r < n; ++r) {
    const int d = s_order[r];
    const int lab = s_label[d];
    const double dx = (double)drow[d * 5 + 0], dy = (double)drow[d * 5 + 1];
    const double dw = (double)drow[d * 5 + 2] - dx, dh = (double)drow[d * 5 + 3] - dy;
    const double d_area = dw * dh;
    for (int g = tid; g < ng; g += CM_THREADS) {
      double v = -1.0;
      if (g_lab[g] == lab) {
        const double gx = g_box[g * 4 + 0], gy = g_box[g * 4 + 1], gw = g_box[g * 4 + 2], gh = g_box[g * 4 + 3];
        const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
        const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        v = 0.0;
        if (iw > 0.0 && ih > 0.0) {
          const double inter = iw * ih;
          const double uni = g_crowd[g] ? d_area : (d_area + gw * gh) - inter;
          v = inter / uni;
        }
      }
      s_iou[g] = v;
    }
    __syncthreads();
    if (matcher) {
      double best = b0;
      int m = -1;
      for (int g = 0; g < ng; ++g) {                 // the gts this range counts, file order
        const double v = s_iou[g];
        if (v < 0.0) continue;
        const double ga = g_area[g];
        if (g_crowd[g] || ga < lo || ga > hi) continue;
        if ((s_mask[(g >> 5) * CM_LANES + tid] >> (g & 31)) & 1u) continue;
        if (v < best) continue;
        best = v;
        m = g;
      }
      bool ign = false;
      if (m < 0) {
        for (int g = 0; g < ng; ++g) {               // the ignored gts, file order; a crowd may be matched again
          const double v = s_iou[g];
          if (v < 0.0) continue;
          const double ga = g_area[g];
          const bool crowd = g_crowd[g] != 0;
          if (!(crowd || ga < lo || ga > hi)) continue;
          if (!crowd && ((s_mask[(g >> 5) * CM_LANES + tid] >> (g & 31)) & 1u)) continue;
          if (v < best) continue;
          best = v;
          m = g;
        }
        ign = m >= 0;
      }
      uint8_t st;
      if (m >= 0) {
        s_mask[(m >> 5) * CM_LANES + tid] |= 1u << (m & 31);
        st = ign ? 2 : 1;
      } else {
        st = (d_area < lo || d_area > hi) ? 2 : 0;
      }
      mine[d] = st;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int aod_coco_match(const float* dets, const int64_t* labels, const int32_t* num, const double* gt_boxes, const double* gt_area,
                              const int32_t* gt_label, const uint8_t* gt_crowd, const int32_t* gt_num, int B, int M, int G,
                              const double* area_rng_host, int A, const double* iou_thr_host, int T, uint8_t* states, aod_stream_t stream) {
  AOD_CHECK_ARG(iou_thr_host && T >= 1 && T <= CM_MAX_T, "coco_match: 1..16 IoU thresholds (got %d)", T);
  AOD_CHECK_ARG(area_rng_host && A >= 1 && A <= CM_MAX_A, "coco_match: 1..4 area ranges (got %d)", A);
  AOD_CHECK_ARG(B >= 0 && M >= 0 && G >= 0, "coco_match: bad shape B=%d M=%d G=%d", B, M, G);
  AOD_CHECK_ARG(M <= CM_MAX_M, "coco_match: at most %d detection rows per image (got %d)", CM_MAX_M, M);
  AOD_CHECK_ARG(G <= CM_MAX_G, "coco_match: at most %d gts per image (got %d)", CM_MAX_G, G);
  if (B == 0 || M == 0) return 0;
  AOD_CHECK_ARG(dets && labels && num && gt_num && states, "coco_match: null pointer");
  AOD_CHECK_ARG(G == 0 || (gt_boxes && gt_area && gt_label && gt_crowd), "coco_match: null gt pointer with G=%d", G);
  cm_par_t par;
  for (int t = 0; t < CM_MAX_T; ++t) par.thr[t] = t < T ? iou_thr_host[t] : 0.0;
  for (int a = 0; a < CM_MAX_A; ++a) {
    par.lo[a] = a < A ? area_rng_host[2 * a] : 0.0;
    par.hi[a] = a < A ? area_rng_host[2 * a + 1] : 0.0;
  }
  const size_t lds = (size_t)G * (6 * sizeof(double) + sizeof(int) + 1) + (size_t)M * 12 + 16;
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)B), dim3(CM_THREADS), lds, (hipStream_t)stream, dets, labels, num, gt_boxes, gt_area,
                     gt_label, gt_crowd, gt_num, B, M, G, par, A, T, states);
  AOD_LAUNCH_CHECK();
  return 0;
}
