// Consistency acquisition: detect on the image, detect again on mirrored copies, map the boxes back and score the image by how
// much the detection lists disagree, in box position and in class posterior -- the acquisition rule of I. Elezi, Z. Yu, A. Anandkumar,
// L. Leal-Taixe, J. M. Alvarez, "Not All Labels Are Equal: Rationalizing the Labeling Costs for Training Object Detection", CVPR 2022
// (image vs. its horizontal flip) and the IoU + Jensen-Shannon form of CALD (W. Yu, S. Zhu, T. Yang, C. Chen, "Consistency-based Active
// Learning for Object Detection", CVPR Workshops 2022).  The reference tree has no such pool: the semantics are fixed in DESIGN 3q.
//
// aod_flip_images      dst[b][c][y][x] = src[b][c][fy ? h - 1 - y : y][fx ? w - 1 - x : x] inside img_shape (h, w), src's bits elsewhere: a
//                      bit copy, nothing is computed (words move as uint32).  flip bit 0: horizontal, bit 1: vertical.  With Wp % 4 == 0 and
//                      16-B aligned buffers one thread writes 4 consecutive x with one 16-B store (a 16-B load too where the quad is not
//                      mirrored in x); otherwise one thread per element.  The same bits either way.
// aod_det_posterior    post[b][j][:] = scores[b][obj_cand[b][j]][:] for j < num[b] with a candidate row (aod_det_uncertainty_ex's obj_cand
//                      under score_thr = -inf: every row j < num is looked up there), zero rows elsewhere: every word of post is written.
//                      missing[b]: the rows j < num[b] without a candidate.
// aod_det_consistency  per image b, over the stacked slots (slot 0: the clean detections, slot v + 1: those of view v):
//   object      row j of slot 0 with j < num[0][b] and dets[0][b][j][4] > score_thr (strict)
//   un-flip     a view box is mapped back first: horizontal x1' = ext_w - x2, x2' = ext_w - x1, vertical likewise with ext_h (one fp32
//               subtraction each; mmdet's bbox_flip)
//   match       argmax of the IoU (aod_loc_stability's form: no +1, union clamped at 1e-6, IEEE division) over the un-flipped rows
//               i < num[v+1][b] (same_class: rows of j's label only), lowest index on a tie; none, or a best IoU of 0: match -1, iou 0, js 1
//   js          p, q: the posterior rows of j and of its match.  t(a, b) = [a > 0] a (ln a - ln m) + [b > 0] b (ln b - ln m), m = (a + b) / 2;
//               cat / cat_bg: (sum_c t(p_c, q_c) / 2) / ln 2 over the used columns in column order; sigmoid: the mean over the used columns
//               of the Bernoulli value (t(p_c, q_c) + t(1 - p_c, 1 - q_c)) / 2 / ln 2.  Rows with the same bits give exactly 0
//   u_jv        box: 1 - iou;  cls: js;  both: ((1 - iou) + js) / 2;   u_j = (u_j0 + ... + u_j,V-1) / V, the views added in order
//   image       max / mean / sum of u_j over the objects; an image without one scores 0
// One launch, one workgroup of 256 threads per image, no atomics, no workspace: thread t owns the clean rows t, t + 256, ... in registers;
// per view all threads stage the un-flipped boxes and the labels in LDS (24 KB), then every owner scans them (all lanes of a wave read the
// same LDS words: broadcasts) and reads the W columns of its own and of its matched row from global memory.  The aggregate runs in a
// pairwise tree over the next power of two >= max_num in LDS -- rows that are no object hold 0 -- so its association depends on j and
// max_num alone: an image has the same score bits alone, at any place of any batch, eager or replayed.  Rows >= num of any slot are never
// read.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define CS_TB 256
#define CS_MAX_DET 1024
#define CS_ROWS (CS_MAX_DET / CS_TB)
#define CS_MAX_VIEWS 3
#define CS_LN2 0.69314718055994530942f

struct cs_flips { int v[CS_MAX_VIEWS]; };

// VEC: Wq = Wp / 4 quads per row, one thread per quad; else Wq = Wp, one thread per element
template <bool VEC>
__global__ __launch_bounds__(256) void flip_images_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int C, int Hp, int Wq,
                                                          const int* __restrict__ hw, int fx, int fy) {
  const int c = blockIdx.y, b = blockIdx.z;
  const int Wp = VEC ? 4 * Wq : Wq;
  int h = hw[2 * b], w = hw[2 * b + 1];
  h = h < 0 ? 0 : (h > Hp ? Hp : h);
  w = w < 0 ? 0 : (w > Wp ? Wp : w);
  const long long per = (long long)Hp * Wq, plane = ((long long)b * C + c) * Hp * Wp;
  const unsigned* s = src + plane;
  unsigned* d = dst + plane;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / Wq), xq = (int)(i - (long long)y * Wq);
    // a pixel of the window (y < h and x < w) reads the window's mirrored pixel; a pixel of the pad -- below the window OR to its right --
    // is its own source
    const unsigned* own = s + (long long)y * Wp;
    const unsigned* mir = s + (long long)((fy && y < h) ? h - 1 - y : y) * Wp;
    if (VEC) {
      const int x0 = 4 * xq;
      u32x4 v;
      if (y >= h || x0 >= w) {                               // the whole quad lies in the pad
        v = *reinterpret_cast<const u32x4*>(own + x0);
      } else if (!fx && x0 + 4 <= w) {                       // the whole quad lies in the window, not mirrored in x
        v = *reinterpret_cast<const u32x4*>(mir + x0);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int x = x0 + u;
          v[u] = x < w ? mir[fx ? w - 1 - x : x] : own[x];
        }
      }
      *reinterpret_cast<u32x4*>(d + (long long)y * Wp + x0) = v;
    } else {
      const int x = xq;
      d[(long long)y * Wp + x] = (y < h && x < w) ? mir[fx ? w - 1 - x : x] : own[x];
    }
  }
}

// the one place the view limit is written: the Python wrappers read it here
extern "C" int aod_consistency_max_views(void) { return CS_MAX_VIEWS; }

extern "C" int aod_flip_images(const float* src, float* dst, int B, int C, int Hp, int Wp, const int32_t* hw, int flip, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1 && B <= 65535, "flip_images: batch must be in 1..65535 (got %d)", B);
  AOD_CHECK_ARG(C >= 1 && C <= 65535, "flip_images: channels must be in 1..65535 (got C = %d)", C);
  AOD_CHECK_ARG(Hp >= 1 && Hp <= 65536, "flip_images: padded height must be in 1..65536 (got %d)", Hp);
  AOD_CHECK_ARG(Wp >= 1 && Wp <= 262144, "flip_images: padded width must be in 1..262144 (got %d)", Wp);
  AOD_CHECK_ARG(flip >= 1 && flip <= 3, "flip_images: flip %d is none of 1 (hflip), 2 (vflip), 3 (hvflip)", flip);
  AOD_CHECK_ARG(src && dst && hw, "flip_images: null pointer");
  AOD_CHECK_ARG(dst != src, "flip_images: dst == src: the kernel is out of place");
  const size_t bytes = (size_t)B * C * Hp * Wp * 4;
  AOD_CHECK_ARG((size_t)dst + bytes <= (size_t)src || (size_t)src + bytes <= (size_t)dst, "flip_images: dst overlaps src: the kernel is out of place");
  AOD_CHECK_ARG(((((size_t)src) | ((size_t)dst) | ((size_t)hw)) & 3) == 0, "flip_images: pointers must be aligned to their element size");
  const bool vec = Wp % 4 == 0 && ((((size_t)src) | ((size_t)dst)) & 15) == 0;
  const int Wq = vec ? Wp / 4 : Wp;
  const long long per = (long long)Hp * Wq;
  const int gx = (int)((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024);
  if (vec)
    hipLaunchKernelGGL(flip_images_kernel<true>, dim3(gx, C, B), dim3(256), 0, (hipStream_t)stream, (const unsigned*)src, (unsigned*)dst, C, Hp, Wq,
                       hw, flip & 1, (flip >> 1) & 1);
  else
    hipLaunchKernelGGL(flip_images_kernel<false>, dim3(gx, C, B), dim3(256), 0, (hipStream_t)stream, (const unsigned*)src, (unsigned*)dst, C, Hp, Wq,
                       hw, flip & 1, (flip >> 1) & 1);
  AOD_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(CS_TB) void det_posterior_kernel(const unsigned* __restrict__ scores, const int* __restrict__ obj_cand,
                                                              const int* __restrict__ num, int n, int W, int max_num,
                                                              unsigned* __restrict__ post, int* __restrict__ missing) {
  __shared__ int scand[CS_MAX_DET];        // the candidate row of every detection row; -1: a zero row
  __shared__ int smiss[CS_TB];
  const int b = blockIdx.x, tid = threadIdx.x;
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  int miss = 0;
  for (int j = tid; j < max_num; j += CS_TB) {
    int k = -1;
    if (j < nd) {
      k = obj_cand[(long long)b * max_num + j];
      if (k < 0 || k >= n) { k = -1; ++miss; }
    }
    scand[j] = k;
  }
  smiss[tid] = miss;
  __syncthreads();
  const unsigned* sc = scores + (long long)b * n * W;
  unsigned* po = post + (long long)b * max_num * W;
  const int total = max_num * W;
  for (int i = tid; i < total; i += CS_TB) {
    const int j = i / W, c = i - j * W;
    const int k = scand[j];
    po[i] = k >= 0 ? sc[(long long)k * W + c] : 0u;
  }
  for (int st = CS_TB >> 1; st > 0; st >>= 1) {
    if (tid < st) smiss[tid] += smiss[tid + st];
    __syncthreads();
  }
  if (tid == 0 && missing) missing[b] = smiss[0];
}

extern "C" int aod_det_posterior(const float* scores, const int32_t* obj_cand, const int32_t* num, int B, int n, int W, int max_num, float* post,
                                 int32_t* missing, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1, "det_posterior: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(n >= 1 && n <= (1 << 30), "det_posterior: candidate rows per image must be in 1..2^30 (got n = %d)", n);
  AOD_CHECK_ARG(W >= 2 && W <= 65536, "det_posterior: score rows of 2..65536 columns (got W = %d)", W);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= CS_MAX_DET, "det_posterior: max_num must be in 1..%d (got %d)", CS_MAX_DET, max_num);
  AOD_CHECK_ARG(scores && obj_cand && num && post, "det_posterior: null pointer");
  AOD_CHECK_ARG(((((size_t)scores) | ((size_t)obj_cand) | ((size_t)num) | ((size_t)post) | ((size_t)missing)) & 3) == 0,
                "det_posterior: pointers must be aligned to their element size");
  hipLaunchKernelGGL(det_posterior_kernel, dim3((unsigned)B), dim3(CS_TB), 0, (hipStream_t)stream, (const unsigned*)scores, obj_cand, num, n, W,
                     max_num, (unsigned*)post, missing);
  AOD_LAUNCH_CHECK();
  return 0;
}

// one column term of the Jensen-Shannon sum: [a > 0] a (ln a - ln m) + [b > 0] b (ln b - ln m), m = (a + b) / 2; a and b of the same bits: 0.
// The halving rounds m to 0 for a + b = 2^-149 alone (the smallest denormal against 0): that term, 2^-149 ln 2, is taken as 0 -- ln m
// would be -inf there and the term +inf
__device__ __forceinline__ float cs_term(float a, float b) {
  const float m = __fmul_rn(0.5f, __fadd_rn(a, b));
  if (m == 0.f) return 0.f;                                  // (a NaN entry is not caught here: it surfaces in the score)
  const float lm = logf(m);
  const float ta = a > 0.f ? __fmul_rn(a, __fsub_rn(logf(a), lm)) : 0.f;
  const float tb = b > 0.f ? __fmul_rn(b, __fsub_rn(logf(b), lm)) : 0.f;
  return __fadd_rn(ta, tb);
}

__device__ __forceinline__ float cs_js(const float* __restrict__ p, const float* __restrict__ q, int used, int layout) {
  float s = 0.f;
  if (layout == 2) {
    for (int c = 0; c < used; ++c) {
      const float a = p[c], b = q[c];
      s = __fadd_rn(s, __fadd_rn(cs_term(a, b), cs_term(__fsub_rn(1.0f, a), __fsub_rn(1.0f, b))));
    }
    return __fdiv_rn(__fdiv_rn(__fmul_rn(0.5f, s), (float)used), CS_LN2);
  }
  for (int c = 0; c < used; ++c) s = __fadd_rn(s, cs_term(p[c], q[c]));
  return __fdiv_rn(__fmul_rn(0.5f, s), CS_LN2);
}

__global__ __launch_bounds__(CS_TB) void det_consistency_kernel(const float* __restrict__ dets, const long long* __restrict__ labels,
                                                                const int* __restrict__ num, const float* __restrict__ post, int V,
                                                                cs_flips flips, const float* __restrict__ ext, int B, int max_num, int W,
                                                                int layout, int mode, int aggregate, float thr, int same_class,
                                                                float* __restrict__ unc, float* __restrict__ obj_out,
                                                                float* __restrict__ iou_out, float* __restrict__ js_out,
                                                                int* __restrict__ match_out) {
  __shared__ f32x4 sbox[CS_MAX_DET];       // the view's un-flipped boxes
  __shared__ long long slab[CS_MAX_DET];   // ... and labels
  __shared__ float val[CS_MAX_DET];        // u_j        (0: no object)
  __shared__ int cnt[CS_MAX_DET];          // 1: object
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long img = (long long)max_num, slot = (long long)B * max_num;
  const float* d0 = dets + b * img * 5;
  const long long* l0 = labels + b * img;
  const float* p0 = post + b * img * W;
  const int used = layout == 1 ? W : W - 1;
  const float ew = ext[2 * b], eh = ext[2 * b + 1];
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  // the clean rows this thread owns
  float ax1[CS_ROWS], ay1[CS_ROWS], ax2[CS_ROWS], ay2[CS_ROWS], aa[CS_ROWS], acc[CS_ROWS];
  long long alab[CS_ROWS];
  bool obj[CS_ROWS];
#pragma unroll
  for (int r = 0; r < CS_ROWS; ++r) {
    const int j = tid + r * CS_TB;
    obj[r] = false;
    ax1[r] = ay1[r] = ax2[r] = ay2[r] = aa[r] = acc[r] = 0.f;
    alab[r] = 0;
    if (j < nd && d0[j * 5 + 4] > thr) {
      obj[r] = true;
      ax1[r] = d0[j * 5]; ay1[r] = d0[j * 5 + 1]; ax2[r] = d0[j * 5 + 2]; ay2[r] = d0[j * 5 + 3];
      aa[r] = __fmul_rn(__fsub_rn(ax2[r], ax1[r]), __fsub_rn(ay2[r], ay1[r]));
      alab[r] = l0[j];
    }
  }
  for (int v = 0; v < V; ++v) {
    const float* dv = dets + (v + 1) * slot * 5 + b * img * 5;
    const long long* lv = labels + (v + 1) * slot + b * img;
    const float* pv = post + ((v + 1) * slot + b * img) * W;
    const int fx = flips.v[v] & 1, fy = flips.v[v] & 2;
    int nv = num[(long long)(v + 1) * B + b];
    nv = nv < 0 ? 0 : (nv > max_num ? max_num : nv);
    __syncthreads();                                         // the previous view has been scanned
    for (int i = tid; i < nv; i += CS_TB) {
      f32x4 q;
      q[0] = dv[i * 5]; q[1] = dv[i * 5 + 1]; q[2] = dv[i * 5 + 2]; q[3] = dv[i * 5 + 3];
      if (fx) { const float x1 = __fsub_rn(ew, q[2]), x2 = __fsub_rn(ew, q[0]); q[0] = x1; q[2] = x2; }
      if (fy) { const float y1 = __fsub_rn(eh, q[3]), y2 = __fsub_rn(eh, q[1]); q[1] = y1; q[3] = y2; }
      sbox[i] = q;
      slab[i] = lv[i];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CS_ROWS; ++r) {
      const int j = tid + r * CS_TB;
      const long long o = (long long)v * slot + b * img + j;
      if (!obj[r]) {
        if (j < max_num) {
          if (iou_out) iou_out[o] = NAN;
          if (js_out) js_out[o] = NAN;
          if (match_out) match_out[o] = -1;
        }
        continue;
      }
      float m = 0.f;
      int best = -1;
      for (int i = 0; i < nv; ++i) {
        if (same_class && slab[i] != alab[r]) continue;
        const f32x4 q = sbox[i];
        const float ab = __fmul_rn(__fsub_rn(q[2], q[0]), __fsub_rn(q[3], q[1]));
        const float iw = fmaxf(__fsub_rn(fminf(ax2[r], q[2]), fmaxf(ax1[r], q[0])), 0.f);
        const float ih = fmaxf(__fsub_rn(fminf(ay2[r], q[3]), fmaxf(ay1[r], q[1])), 0.f);
        const float ov = __fmul_rn(iw, ih);
        const float un = __fsub_rn(__fadd_rn(aa[r], ab), ov);
        const float iou = __fdiv_rn(ov, fmaxf(un, 1e-6f));
        if (iou > m) { m = iou; best = i; }
      }
      float js = 1.0f;
      if (best >= 0 && (mode != 0 || js_out)) js = cs_js(p0 + (long long)j * W, pv + (long long)best * W, used, layout);      // (box: js_out only)
      const float box = __fsub_rn(1.0f, m);
      const float u = mode == 0 ? box : (mode == 1 ? js : __fmul_rn(0.5f, __fadd_rn(box, js)));
      acc[r] = __fadd_rn(acc[r], u);
      if (iou_out) iou_out[o] = m;
      if (js_out) js_out[o] = js;
      if (match_out) match_out[o] = best;
    }
  }
  // u_j and the leaves of the tree
  const float fV = (float)V;
#pragma unroll
  for (int r = 0; r < CS_ROWS; ++r) {
    const int j = tid + r * CS_TB;
    const float u = __fdiv_rn(acc[r], fV);
    val[j] = obj[r] ? u : 0.f;
    cnt[j] = obj[r] ? 1 : 0;
    if (obj_out && j < max_num) obj_out[b * img + j] = obj[r] ? u : NAN;
  }
  // pairwise tree over the next power of two >= max_num
  int np2 = 1;
  while (np2 < max_num) np2 <<= 1;
  for (int st = np2 >> 1; st > 0; st >>= 1) {
    __syncthreads();
    for (int i = tid; i < st; i += CS_TB) {
      const float a = val[i], c = val[i + st];
      val[i] = aggregate == 0 ? fmaxf(a, c) : __fadd_rn(a, c);
      cnt[i] += cnt[i + st];
    }
  }
  __syncthreads();
  if (tid == 0) {
    float r = val[0];
    if (aggregate == 1 && cnt[0] > 0) r = __fdiv_rn(r, (float)cnt[0]);
    unc[b] = cnt[0] > 0 ? r : 0.f;
  }
}

extern "C" int aod_det_consistency(const float* dets, const int64_t* labels, const int32_t* num, const float* post, int V, const int32_t* flips,
                                   const float* ext, int B, int max_num, int W, int layout, int mode, int aggregate, float score_thr,
                                   int same_class, float* unc, float* obj_out, float* iou_out, float* js_out, int32_t* match_out,
                                   aod_stream_t stream) {
  AOD_CHECK_ARG(V >= 1 && V <= CS_MAX_VIEWS, "det_consistency: the number of views V must be in 1..%d (got %d)", CS_MAX_VIEWS, V);
  AOD_CHECK_ARG(B >= 1, "det_consistency: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= CS_MAX_DET, "det_consistency: max_num must be in 1..%d (got %d)", CS_MAX_DET, max_num);
  AOD_CHECK_ARG(W >= 2 && W <= 65536, "det_consistency: posterior rows of 2..65536 columns (got W = %d)", W);
  AOD_CHECK_ARG(layout >= 0 && layout <= 2, "det_consistency: layout %d is none of 0 (cat), 1 (cat_bg), 2 (sigmoid)", layout);
  AOD_CHECK_ARG(mode >= 0 && mode <= 2, "det_consistency: mode %d is none of 0 (box), 1 (cls), 2 (both)", mode);
  AOD_CHECK_ARG(aggregate >= 0 && aggregate <= 2, "det_consistency: aggregate %d is none of 0 (max), 1 (mean), 2 (sum)", aggregate);
  AOD_CHECK_ARG(same_class == 0 || same_class == 1, "det_consistency: same_class must be 0 or 1 (got %d)", same_class);
  AOD_CHECK_ARG(score_thr == score_thr, "det_consistency: score_thr is NaN");
  AOD_CHECK_ARG(dets && labels && num && post && flips && ext && unc, "det_consistency: null pointer");
  cs_flips fl = {{0, 0, 0}};
  for (int v = 0; v < V; ++v) {
    AOD_CHECK_ARG(flips[v] >= 1 && flips[v] <= 3, "det_consistency: flips[%d] = %d is none of 1 (hflip), 2 (vflip), 3 (hvflip)", v, (int)flips[v]);
    fl.v[v] = flips[v];
  }
  AOD_CHECK_ARG(((((size_t)dets) | ((size_t)num) | ((size_t)post) | ((size_t)ext) | ((size_t)unc) | ((size_t)obj_out) | ((size_t)iou_out) |
                   ((size_t)js_out) | ((size_t)match_out)) & 3) == 0 &&
                    (((size_t)labels) & 7) == 0,
                "det_consistency: pointers must be aligned to their element size");
  hipLaunchKernelGGL(det_consistency_kernel, dim3((unsigned)B), dim3(CS_TB), 0, (hipStream_t)stream, dets, (const long long*)labels, num, post, V,
                     fl, ext, B, max_num, W, layout, mode, aggregate, score_thr, same_class, unc, obj_out, iou_out, js_out, match_out);
  AOD_LAUNCH_CHECK();
  return 0;
}
