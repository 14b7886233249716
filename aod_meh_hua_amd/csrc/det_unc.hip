// Posterior uncertainty pools: uncertainty sampling on the detector's own class posterior -- entropy ("Entropy" in the paper's
// tables), 1-vs-2 margin and least confidence (C.-A. Brust, C. Kaeding, J. Denzler, "Active Learning for Deep Object Detection", VISAPP
// 2019; S. Roy, A. Unmesh, V. P. Namboodiri, "Deep active learning for object detection", BMVC 2018), aggregated over an image's
// detections by max, mean or sum.  The reference tree has no such pool: the semantics are fixed in DESIGN 3l.
//
// Per image b, behind aod_pre_nms_levels / aod_multiclass_nms:
//   object      detection row j with j < num[b] and dets[b][j][4] > score_thr (strict); rows j >= num[b] are never read
//   score row   the candidate k of lowest index with boxes[b][k] == dets[b][j][0..3] and scores[b][k][labels[b][j]] == dets[b][j][4], bit for
//               bit (the NMS kernel copies both unchanged); an object without one is skipped and counted in missing[b]
//   measure     from the row's used columns s (layout 0 / 2: the first W - 1, layout 1: all W)
//                 entropy   layout 0 / 1: -sum s ln s;  layout 2: sum_c -s ln s - (1 - s) ln(1 - s), ln(1 - s) = log1pf(-s);  0 ln 0 = 0
//                 margin    1 - (s_(1) - s_(2)), the two largest used columns;   leastconf  1 - s_(1)
//   aggregate   max / mean / sum over the image's objects; an image without one scores 0
// One launch, one workgroup of 256 threads per image, no atomics, no workspace:
//   1. a thread per detection row: gate, label check, a 32-bit hash of the four box words into LDS
//   2. the candidates in tiles of DU_TILE: all threads hash the boxes of a tile into LDS, then a lane per detection row scans the tile's
//      hashes (every lane of a wave reads the same LDS words: broadcasts, 16 B per read) and compares the five words in global memory only
//      on a hash hit.  With max_num <= 128 the idle waves take further parts of the tile: wave w scans part w / ndw for the detection rows
//      of wave w % ndw; the lowest index over the parts is the minimum of the parts' own lowest.
//   3. a thread per detection row: the measure of its row (the classes in column order), written to obj_out and to LDS; the matched
//      candidate row itself goes to obj_cand (aod_det_uncertainty_ex: what the CCMS object descriptors of DESIGN 3o are gathered by).
//      With class_w (aod_det_uncertainty_w: the class-weighted pools of DESIGN 3p) the measure is first multiplied by class_w[label]
//   4. the aggregate: a pairwise tree over the next power of two >= max_num in LDS -- rows that are no object hold 0 -- so the association of
//      the sum depends on j and max_num alone: an image has the same score bits alone, at any place of any batch, eager or replayed.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define DU_TB 256
#define DU_TILE 2048          // candidates per tile: 8 KB of hashes
#define DU_MAX_DET 1024

__device__ __forceinline__ unsigned du_hash(unsigned a, unsigned b, unsigned c, unsigned d) {
  return a ^ ((b << 8) | (b >> 24)) ^ ((c << 16) | (c >> 16)) ^ ((d << 24) | (d >> 8));
}

// the measure of one score row: `used` columns, read once in column order
__device__ __forceinline__ float du_measure(const float* __restrict__ s, int used, int layout, int measure) {
  if (measure == 0) {
    float h = 0.f;
    if (layout == 2) {
      for (int c = 0; c < used; ++c) {
        const float v = s[c], t = 1.0f - v;
        const float a = v > 0.f ? -v * logf(v) : 0.f;
        const float e = t > 0.f ? -t * log1pf(-v) : 0.f;
        h += a + e;
      }
    } else {
      for (int c = 0; c < used; ++c) {
        const float v = s[c];
        h += v > 0.f ? -v * logf(v) : 0.f;
      }
    }
    return h;
  }
  float m1 = s[0], m2 = -INFINITY;
  for (int c = 1; c < used; ++c) {
    const float v = s[c];
    if (v > m1) { m2 = m1; m1 = v; }
    else if (v > m2) m2 = v;
  }
  return measure == 1 ? 1.0f - (m1 - m2) : 1.0f - m1;
}

__global__ __launch_bounds__(DU_TB) void det_unc_kernel(const unsigned* __restrict__ boxes, const float* __restrict__ scores,
                                                        const float* __restrict__ dets, const long long* __restrict__ labels,
                                                        const int* __restrict__ num, int n, int W, int max_num, int layout, int measure,
                                                        int aggregate, float thr, float* __restrict__ unc, float* __restrict__ obj_out,
                                                        int* __restrict__ missing, int* __restrict__ obj_cand,
                                                        const float* __restrict__ class_w) {
  __shared__ __align__(16) unsigned tile[DU_TILE];
  __shared__ unsigned dhash[DU_MAX_DET];
  __shared__ int lab[DU_MAX_DET];          // the label of an object row; -1: no object; -2: an object whose label names no column
  __shared__ int found[DU_MAX_DET];        // [part][row]: lowest matching candidate the part has seen
  __shared__ float val[DU_MAX_DET];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned* bx = boxes + (long long)b * n * 4;
  const float* sc = scores + (long long)b * n * W;
  const unsigned* scu = reinterpret_cast<const unsigned*>(sc);
  const float* dt = dets + (long long)b * max_num * 5;
  const unsigned* dtu = reinterpret_cast<const unsigned*>(dt);
  const long long* lb = labels + (long long)b * max_num;
  const int used = layout == 1 ? W : W - 1;
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  // 1. gate and hash of every detection row
  for (int j = tid; j < DU_MAX_DET; j += DU_TB) {
    int l = -1;
    unsigned h = 0;
    if (j < nd && dt[j * 5 + 4] > thr) {
      const long long q = lb[j];
      l = (q >= 0 && q < (long long)W) ? (int)q : -2;
      h = du_hash(dtu[j * 5], dtu[j * 5 + 1], dtu[j * 5 + 2], dtu[j * 5 + 3]);
    }
    lab[j] = l;
    dhash[j] = h;
    found[j] = INT_MAX;
  }
  // 2. lookup.  ndw waves hold a detection row per lane; P parts of a tile are scanned side by side
  const int ndw = (max_num + 63) >> 6;
  const int P = ndw == 1 ? 4 : (ndw == 2 ? 2 : 1);
  const int spp = P == 1 ? 0 : ndw * 64;                     // rows of `found` per part
  const int S = P == 1 ? ndw * 64 : DU_TB;                   // (detection row, part) slots
  const int per = DU_TILE / P;
  for (int t0 = 0; t0 < n; t0 += DU_TILE) {
    const int tn = n - t0 < DU_TILE ? n - t0 : DU_TILE;
    __syncthreads();                                         // (the first pass: step 1's writes; later: the previous tile has been scanned)
    for (int i = tid; i < DU_TILE; i += DU_TB) {
      unsigned h = 0;
      if (i < tn) {
        const unsigned* q = bx + (long long)(t0 + i) * 4;
        h = du_hash(q[0], q[1], q[2], q[3]);
      }
      tile[i] = h;
    }
    __syncthreads();
    for (int s = tid; s < S; s += DU_TB) {
      int part = 0, j = s;
      if (P > 1) { const int w = s >> 6; part = w / ndw; j = (w - part * ndw) * 64 + (s & 63); }
      if (j >= max_num) continue;
      const int l = lab[j];
      if (l < 0) continue;
      int fk = found[part * spp + j];
      if (fk != INT_MAX) continue;
      const unsigned h = dhash[j];
      const int q0 = part * per;
      const int q1 = q0 + per < tn ? q0 + per : tn;
      for (int q = q0; q < q1 && fk == INT_MAX; q += 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(&tile[q]);
        if (v[0] == h || v[1] == h || v[2] == h || v[3] == h) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (fk == INT_MAX && v[u] == h && q + u < tn) {
              const long long k = (long long)t0 + q + u;
              const unsigned* cb = bx + k * 4;
              const unsigned* db = dtu + j * 5;
              if (cb[0] == db[0] && cb[1] == db[1] && cb[2] == db[2] && cb[3] == db[3] && scu[k * W + l] == db[4]) fk = (int)k;
            }
          }
        }
      }
      if (fk != INT_MAX) found[part * spp + j] = fk;
    }
  }
  __syncthreads();
  // 3. the measure of every object row; lab[] becomes (counted | missing << 16)
  for (int j = tid; j < DU_MAX_DET; j += DU_TB) {
    float m = 0.f;
    int flag = 0;
    if (j < max_num) {
      const int l = lab[j];
      float o = NAN;
      int kc = -1;                                           // (obj_cand: the matched candidate row of an object, else -1)
      if (l != -1) {
        int k = INT_MAX;
        if (l >= 0)
          for (int p = 0; p < P; ++p) { const int f = found[p * spp + j]; k = f < k ? f : k; }
        if (k == INT_MAX) {
          flag = 1 << 16;
        } else {
          m = du_measure(sc + (long long)k * W, used, layout, measure);
          if (class_w) m = __fmul_rn(m, class_w[l]);         // (class-weighted pools, DESIGN 3p: one multiply in front of the tree)
          o = m;
          flag = 1;
          kc = k;
        }
      }
      if (obj_out) obj_out[(long long)b * max_num + j] = o;
      if (obj_cand) obj_cand[(long long)b * max_num + j] = kc;
    }
    val[j] = m;
    lab[j] = flag;            // (a row's lab[] and found[] words are read by the thread that owns the row alone)
  }
  // 4. pairwise tree over the next power of two >= max_num
  int np2 = 1;
  while (np2 < max_num) np2 <<= 1;
  for (int st = np2 >> 1; st > 0; st >>= 1) {
    __syncthreads();
    for (int i = tid; i < st; i += DU_TB) {
      const float a = val[i], c = val[i + st];
      val[i] = aggregate == 0 ? fmaxf(a, c) : a + c;
      lab[i] += lab[i + st];
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int cnt = lab[0] & 0xffff, miss = lab[0] >> 16;
    float r = val[0];
    if (aggregate == 1 && cnt > 0) r = r / (float)cnt;
    unc[b] = cnt > 0 ? r : 0.f;
    if (missing) missing[b] = miss;
  }
}

// obj_cand [B][max_num] int32 (nullable): the candidate row the lookup matched to every object row, -1 for a row that is no object or has none
// (aod_object_descriptors reads the neck row of that candidate's anchor: no second matching pass).  The other outputs are aod_det_uncertainty's.
// class_w [W] (nullable): the measure of an object row with label l is multiplied by class_w[l] before it goes to obj_out and into the aggregate
// (aod_class_difficulty_*: DESIGN 3p).  NULL: no multiply, aod_det_uncertainty_ex's bits.
extern "C" int aod_det_uncertainty_w(const float* boxes, const float* scores, const float* dets, const int64_t* labels, const int32_t* num, int B,
                                     int n, int W, int max_num, int layout, int measure, int aggregate, float score_thr, float* unc,
                                     float* obj_out, int32_t* missing, int32_t* obj_cand, const float* class_w, aod_stream_t stream) {
  AOD_CHECK_ARG(layout >= 0 && layout <= 2, "det_uncertainty: layout %d is none of 0 (cat), 1 (cat_bg), 2 (sigmoid)", layout);
  AOD_CHECK_ARG(measure >= 0 && measure <= 2, "det_uncertainty: measure %d is none of 0 (entropy), 1 (margin), 2 (leastconf)", measure);
  AOD_CHECK_ARG(aggregate >= 0 && aggregate <= 2, "det_uncertainty: aggregate %d is none of 0 (max), 1 (mean), 2 (sum)", aggregate);
  AOD_CHECK_ARG(B >= 1, "det_uncertainty: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(n >= 1, "det_uncertainty: at least one candidate row per image (got n = %d)", n);
  AOD_CHECK_ARG(W >= 2, "det_uncertainty: score rows of at least 2 columns (got W = %d)", W);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= DU_MAX_DET, "det_uncertainty: max_num must be in 1..%d (got %d)", DU_MAX_DET, max_num);
  const int used = layout == 1 ? W : W - 1;
  AOD_CHECK_ARG(measure != 1 || used >= 2, "det_uncertainty: margin needs two used columns (layout %d reads %d of W = %d)", layout, used, W);
  AOD_CHECK_ARG(boxes && scores && dets && labels && num && unc, "det_uncertainty: null pointer");
  AOD_CHECK_ARG(((((size_t)boxes) | ((size_t)scores) | ((size_t)dets) | ((size_t)num) | ((size_t)unc) | ((size_t)obj_out) | ((size_t)missing) |
                   ((size_t)obj_cand) | ((size_t)class_w)) & 3) == 0 &&
                    (((size_t)labels) & 7) == 0,
                "det_uncertainty: pointers must be aligned to their element size");
  AOD_CHECK_ARG(score_thr == score_thr, "det_uncertainty: score_thr is NaN");
  AOD_CHECK_ARG(n <= (1 << 30), "det_uncertainty: up to 2^30 candidate rows per image (got n = %d)", n);
  hipLaunchKernelGGL(det_unc_kernel, dim3((unsigned)B), dim3(DU_TB), 0, (hipStream_t)stream, (const unsigned*)boxes, scores, dets,
                     (const long long*)labels, num, n, W, max_num, layout, measure, aggregate, score_thr, unc, obj_out, missing, obj_cand,
                     class_w);
  AOD_LAUNCH_CHECK();
  return 0;
}

extern "C" int aod_det_uncertainty_ex(const float* boxes, const float* scores, const float* dets, const int64_t* labels, const int32_t* num, int B,
                                      int n, int W, int max_num, int layout, int measure, int aggregate, float score_thr, float* unc,
                                      float* obj_out, int32_t* missing, int32_t* obj_cand, aod_stream_t stream) {
  return aod_det_uncertainty_w(boxes, scores, dets, labels, num, B, n, W, max_num, layout, measure, aggregate, score_thr, unc, obj_out, missing,
                               obj_cand, nullptr, stream);
}

extern "C" int aod_det_uncertainty(const float* boxes, const float* scores, const float* dets, const int64_t* labels, const int32_t* num, int B,
                                   int n, int W, int max_num, int layout, int measure, int aggregate, float score_thr, float* unc,
                                   float* obj_out, int32_t* missing, aod_stream_t stream) {
  return aod_det_uncertainty_ex(boxes, scores, dets, labels, num, B, n, W, max_num, layout, measure, aggregate, score_thr, unc, obj_out, missing,
                                nullptr, stream);
}
