// Fused EDL softmax-focal + L1 loss (forward / backward) and MEH loss for gfx950.
// HBM-bound: one pass over the fp32 logits.  Rows are staged through LDS with coalesced 16-B
// loads, then one thread owns one anchor row (C = 20 logits) in registers.
// Compiled with -ffp-contract=off: the formulas follow the reference op order.
#include "common.h"

#define FLT_MIN_F 1.17549435e-38f
constexpr int LB = 256;     // rows per block
constexpr int MAXC = 96;

__device__ __forceinline__ float focal_pow(float b, float gamma) { return gamma == 2.f ? b * b : powf(b, gamma); }

// The row kernels are VALU-bound, not HBM-bound: per class the reference formula costs two exponentials, up to three logarithms and three
// divisions, and libm's expf / logf / IEEE division are 12-30 instructions each (~4000 instructions per 20-class row; PMC and the
// secondary roofline of bench.py: 0.10 of the HBM rate).  AOD_LOSS_FAST_MATH (default) evaluates them with the hardware transcendentals
// (v_exp_f32, v_log_f32, v_rcp_f32: 1 ulp each, arguments are normal floats), same formulas in the same order.  The golden parity tests
// keep their tolerances (rtol 2e-5 per row against the reference's own values); -DAOD_LOSS_FAST_MATH=0 restores libm.
#ifndef AOD_LOSS_FAST_MATH
#define AOD_LOSS_FAST_MATH 1
#endif
#if AOD_LOSS_FAST_MATH
__device__ __forceinline__ float l_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float l_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309f; }
__device__ __forceinline__ float l_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
#else
__device__ __forceinline__ float l_exp(float x) { return expf(x); }
__device__ __forceinline__ float l_log(float x) { return logf(x); }
__device__ __forceinline__ float l_div(float a, float b) { return a / b; }
#endif

// Row layout in the kernels below: LPR lanes share one anchor row, lane part j owns the classes [j*cpl, (j+1)*cpl) with
// cpl = ceil(C / LPR) <= CT.  CT is a compile-time bound: the loops are fully unrolled and predicated, so x[] / p[] / gp[] live in
// registers -- with a run-time trip count (or a 96-wide bound for the 80/81-class heads) they were demoted to scratch memory
// (400-1168 B per lane) and the kernels ran at an eighth of the HBM rate.  LPR = 1 (C <= 24: VOC's 20/21 classes, one lane per row, the
// reference's sequential op order) or 4 (C <= 96: COCO's 80/81; row maxima / sums are combined over the 4 lanes by two shuffles).
template <int LPR>
__device__ __forceinline__ float grp_max(float v) {
  if (LPR >= 2) v = fmaxf(v, __shfl_xor(v, 1, 64));
  if (LPR >= 4) v = fmaxf(v, __shfl_xor(v, 2, 64));
  return v;
}
template <int LPR>
__device__ __forceinline__ float grp_sum(float v) {
  if (LPR >= 2) v += __shfl_xor(v, 1, 64);
  if (LPR >= 4) v += __shfl_xor(v, 2, 64);
  return v;
}

// per-row forward core: fills p[] (softmax) and returns the row loss (identical in the LPR lanes of the row)
template <int CT, int LPR>
__device__ __forceinline__ float edl_row_fwd(const float* x, int n, int c0, long long label, float gamma, float alpha, float* p) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CT; ++c) if (c < n) m = fmaxf(m, x[c]);
  m = grp_max<LPR>(m);
  float S = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) if (c < n) { p[c] = l_exp(x[c] - m); S += p[c]; }
  S = grp_sum<LPR>(S);
  float tot = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) if (c < n) {
    const float pr = l_div(p[c], S);
    p[c] = pr;
    const float z = l_log(l_div(pr, 1.f - pr + 1e-9f) + 1e-9f);
    const float q = l_div(1.f, 1.f + l_exp(-z));
    const bool pos = label == c0 + c;
    // (one logarithm per class: its argument is selected, not its result)
    const float lg = l_log(fmaxf(pos ? q : 1.f - q, FLT_MIN_F));
    float l;
    if (pos) l = -alpha * focal_pow(1.f - q, gamma) * lg;
    else l = -(1.f - alpha) * focal_pow(q, gamma) * lg;
    tot += l;
  }
  return grp_sum<LPR>(tot);
}

// FORM (compile-time, on the row cores and kernels below): what stands between the logits and mmcv's sigmoid focal term
//   0  EDL    softmax -> log(p / (1 - p + 1e-9) + 1e-9) -> focal               EDL_Softmax_FocalLoss.py:51-69
//   1  plain  the focal term on the raw logits, per class, no softmax          focal_loss.py:85 (FocalLoss of MyRetinaHead)
// Both share the LDS staging, the lane split, the level table, the block partials and the finalize; the box term is the same code.
constexpr int FORM_EDL = 0, FORM_SIGMOID = 1;

// mmcv-full 1.3.8's sigmoid focal term on one logit (the reference's GPU path; FocalLoss at focal_loss.py:85): q = 1 / (1 + exp(-x)),
// target class -alpha (1-q)^gamma log(max(q, FLT_MIN)), other classes -(1-alpha) q^gamma log(max(1-q, FLT_MIN)).  Not the softplus form:
// q rounds to 0 / 1 at |x| >~ 17 and the clamp then bounds the term at -log(FLT_MIN) = 87.3, as in the reference.
// gz (optional) = d l / d x with the clamps as written (mmcv's backward kernel).
__device__ __forceinline__ float sig_focal_term(float x, bool pos, float gamma, float alpha, float* gz) {
  const float q = l_div(1.f, 1.f + l_exp(-x));
  const float lg = l_log(fmaxf(pos ? q : 1.f - q, FLT_MIN_F));
  if (gz) {
    if (pos) *gz = -alpha * focal_pow(1.f - q, gamma) * (1.f - q - gamma * q * lg);
    else *gz = -(1.f - alpha) * focal_pow(q, gamma) * (gamma * (1.f - q) * lg - q);
  }
  return pos ? -alpha * focal_pow(1.f - q, gamma) * lg : -(1.f - alpha) * focal_pow(q, gamma) * lg;
}

// per-row forward core of the plain form: the row loss (a label of C, background, makes every column negative)
template <int CT, int LPR>
__device__ __forceinline__ float sig_row_fwd(const float* x, int n, int c0, long long label, float gamma, float alpha) {
  float tot = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) if (c < n) tot += sig_focal_term(x[c], label == c0 + c, gamma, alpha, nullptr);
  return grp_sum<LPR>(tot);
}

// BOX (compile-time, next to FORM): the box term of a row whose lane part == 0 adds it to the block's second partial sum
//   0  l1    sum_j |pred_j - tgt_j| * bw_j on the encoded deltas                                            smooth_l1_loss.py:33-45 (L1Loss)
//   1  iou   w * -log(max(IoU, eps))  (w * (1 - max(IoU, eps)) when `linear`)                                 iou_loss.py:14-36  (IoULoss)
//   2  giou  w * (1 - (IoU - (E - U) / E)),  U = max(U, eps), E = max(E, eps)                                 iou_loss.py:87-102 (GIoULoss)
// with w = mean_j bw_j (iou_loss.py:275-280 `weight.mean(-1)`); a row with w == 0 is not evaluated: it adds exactly 0 and its four gradients
// are +0 whatever its deltas hold (the sparse forward leaves arbitrary values there; the sparse backward skips all-zero rows).
// Forms 1 and 2 decode the prediction row AND the target row in the anchor-normalised frame (delta2bbox of delta_xywh_bbox_coder.py:205-246
// on the anchor (-.5, -.5, .5, .5)): t = d * std + mean, centre (t0, t1), size exp(clamp(t2 | t3, +-max_ratio)), corners centre -+ size / 2.
// The map from that frame to pixels is a per-axis scaling plus a translation, under which intersection, union and enclosing area all scale by
// the same factor: IoU and GIoU are the numbers of the pixel frame and no anchor is read.  bbox_overlaps(is_aligned=True)
// (iou2d_calculator.py:212-260) in its order; the gradients are autograd's, subgradients included: torch.max(a, b) / torch.min(a, b) hand a
// tie half the gradient each, clamp(min=m) passes where x >= m, clamp(min, max) passes on the closed interval.
constexpr int BOX_L1 = 0, BOX_IOU = 1, BOX_GIOU = 2;
struct BoxForm { float mean[4], std[4]; float max_ratio, eps; int linear; };
// d max(a, b) / d a and d min(a, b) / d a
__device__ __forceinline__ float sub_max(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float sub_min(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

__device__ __forceinline__ float box_exp(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float box_log(float x) { return (float)log((double)x); }

// one row: the loss term l(pred deltas dp, target deltas dt) and, with GRAD, g[4] = d l / d dp  (constant indices only: all in registers).
// IEEE divisions and correctly rounded exp / log (evaluated in double, rounded once), not the l_exp / l_div / l_log of the class terms: the
// row sits at the end of cancelling differences of O(1) corners, -log(eps) = 13.8 has an ulp of 1e-6, and the row is held to a few ulps of
// the float64 value; only rows with a box weight -- the positives -- pay.
template <int BOX, bool GRAD>
__device__ __forceinline__ float box_row(const f32x4 dp, const f32x4 dt, const BoxForm& k, float* g) {
  float p1[2], p2[2], t1[2], t2[2], ps[2], pin[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float pc = dp[j] * k.std[j] + k.mean[j], tc = dt[j] * k.std[j] + k.mean[j];
    const float pl = dp[2 + j] * k.std[2 + j] + k.mean[2 + j], tl = dt[2 + j] * k.std[2 + j] + k.mean[2 + j];
    pin[j] = (pl >= -k.max_ratio && pl <= k.max_ratio) ? 1.f : 0.f;
    ps[j] = box_exp(fminf(fmaxf(pl, -k.max_ratio), k.max_ratio));
    const float ts = box_exp(fminf(fmaxf(tl, -k.max_ratio), k.max_ratio));
    p1[j] = pc - ps[j] * 0.5f; p2[j] = pc + ps[j] * 0.5f;
    t1[j] = tc - ts * 0.5f; t2[j] = tc + ts * 0.5f;
  }
  const float a1 = (p2[0] - p1[0]) * (p2[1] - p1[1]), a2 = (t2[0] - t1[0]) * (t2[1] - t1[1]);
  float iwr[2], iw[2], ewr[2], ew[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    iwr[j] = fminf(p2[j], t2[j]) - fmaxf(p1[j], t1[j]);
    iw[j] = fmaxf(iwr[j], 0.f);
    if (BOX == BOX_GIOU) {
      ewr[j] = fmaxf(p2[j], t2[j]) - fminf(p1[j], t1[j]);
      ew[j] = fmaxf(ewr[j], 0.f);
    }
  }
  const float ov = iw[0] * iw[1];
  const float un = a1 + a2 - ov;
  // (giou_loss hands its eps to bbox_overlaps; iou_loss calls it with the default 1e-6 and clamps the IoU at its own eps, iou_loss.py:31,100)
  const float ueps = BOX == BOX_GIOU ? k.eps : 1e-6f;
  const float U = fmaxf(un, ueps);
  const float iou = ov / U;
  float loss, Er = 0.f, E = 0.f, ic = 0.f;
  if (BOX == BOX_GIOU) {
    Er = ew[0] * ew[1];
    E = fmaxf(Er, k.eps);
    loss = 1.f - (iou - (E - U) / E);
  } else {
    ic = fmaxf(iou, k.eps);
    loss = k.linear ? 1.f - ic : -box_log(ic);
  }
  if (GRAD) {
    float g_ov, g_U, g_Er = 0.f;     // d l / d ov through IoU alone, d l / d (clamped union), d l / d (unclamped enclosing area)
    if (BOX == BOX_GIOU) {
      g_ov = -1.f / U;
      g_U = ov / (U * U) - 1.f / E;
      g_Er = U / (E * E) * sub_max(Er, k.eps);
    } else {
      const float gi = iou >= k.eps ? (k.linear ? -1.f : -1.f / ic) : 0.f;
      g_ov = gi / U;
      g_U = -gi * ov / (U * U);
    }
    const float g_un = g_U * sub_max(un, ueps);     // = d l / d a1 as well
    const float g_ovt = g_ov - g_un;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = 1 - j;
      float g2 = g_un * (p2[o] - p1[o]), g1 = -g2;    // the prediction's own area
      const float giw = iwr[j] >= 0.f ? g_ovt * iw[o] : 0.f;
      g2 += giw * sub_min(p2[j], t2[j]);
      g1 -= giw * sub_max(p1[j], t1[j]);
      if (BOX == BOX_GIOU) {
        const float gew = ewr[j] >= 0.f ? g_Er * ew[o] : 0.f;
        g2 += gew * sub_max(p2[j], t2[j]);
        g1 -= gew * sub_min(p1[j], t1[j]);
      }
      g[j] = (g1 + g2) * k.std[j];
      g[2 + j] = (g2 - g1) * 0.5f * ps[j] * pin[j] * k.std[2 + j];
    }
  }
  return loss;
}

// One launch over ALL pyramid levels (Lambda_L2.py:105-121 runs loss_single once per level through multi_apply): the levels' anchor rows are
// adjacent row ranges of the same buffers (level-batched prediction convs, level-major targets), and a block belongs to exactly one level --
// level l owns the blocks [blk_end[l-1], blk_end[l]) and the rows [row_end[l-1], row_end[l]), its blocks start at its first row.  Blocks, rows
// per block and the order of every sum are those of a per-level launch: identical bits.  (Unused entries: blk_end = INT_MAX.)
constexpr int MAXLV = 8;
struct LossLevels { int n; int blk_end[MAXLV]; long long row_end[MAXLV]; };
// (constant indices only: a run-time index into the by-value argument would move it to scratch memory)
__device__ __forceinline__ void level_of_block(const LossLevels& lv, int bid, int& level, int& blk0, long long& row0, long long& rend) {
  level = 0; blk0 = 0; row0 = 0; rend = lv.row_end[0];
#pragma unroll
  for (int q = 0; q + 1 < MAXLV; ++q)
    if (bid >= lv.blk_end[q]) { level = q + 1; blk0 = lv.blk_end[q]; row0 = lv.row_end[q]; rend = lv.row_end[q + 1]; }
}
static int fill_levels(LossLevels& lv, int nlevels, const int64_t* level_rows, int rows_per_block, long long& total_rows) {
  lv.n = nlevels;
  long long r = 0, b = 0;
  for (int l = 0; l < MAXLV; ++l) {
    if (l < nlevels) { r += level_rows[l]; b += (level_rows[l] + rows_per_block - 1) / rows_per_block; }
    lv.row_end[l] = r;
    lv.blk_end[l] = l < nlevels ? (int)b : 0x7fffffff;
  }
  total_rows = r;
  return (int)b;
}

template <int FORM, int BOX, int CT, int LPR>
__global__ __launch_bounds__(LB) void edl_l1_fwd_kernel(const float* __restrict__ cls, const long long* __restrict__ labels,
                                                        const float* __restrict__ lw, const float* __restrict__ bp,
                                                        const float* __restrict__ bt, const float* __restrict__ bw, const LossLevels lv, int C,
                                                        float gamma, float alpha, float* __restrict__ loss_noR, float* __restrict__ partials,
                                                        const BoxForm bf) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  constexpr int RB = LB / LPR;   // rows per block
  const int P = C | 1;  // odd pitch -> conflict-free row reads
  int level, blk0; long long row0, rend;
  level_of_block(lv, (int)blockIdx.x, level, blk0, row0, rend);
  const long long r0 = row0 + (long long)((int)blockIdx.x - blk0) * RB;
  const int nr = (int)min((long long)RB, rend - r0);
  aod_stage_rows<LB>(cls + r0 * C, srow, nr, C, P);
  __syncthreads();
  float s_cls = 0.f, s_box = 0.f, s_nor = 0.f;
  const int lrow = threadIdx.x / LPR, part = threadIdx.x % LPR;
  const bool live = lrow < nr;
  const int row = live ? lrow : nr - 1;          // every lane takes part in the row shuffles
  const int cpl = (C + LPR - 1) / LPR, c0 = part * cpl;
  const int n = min(cpl, C - c0);
  {
    const long long r = r0 + row;
    float x[CT], p[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c] = c < n ? srow[row * P + c0 + c] : 0.f;
    const float l = FORM == FORM_SIGMOID ? sig_row_fwd<CT, LPR>(x, n, c0, labels[r], gamma, alpha)
                                         : edl_row_fwd<CT, LPR>(x, n, c0, labels[r], gamma, alpha, p);
    if (live && part == 0) {
      loss_noR[r] = l;
      s_nor = l;
      s_cls = l * lw[r];
      if (bp) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(bp + r * 4), b = *reinterpret_cast<const f32x4*>(bt + r * 4),
                    w = *reinterpret_cast<const f32x4*>(bw + r * 4);
        if constexpr (BOX == BOX_L1) {
          for (int j = 0; j < 4; ++j) s_box += fabsf(a[j] - b[j]) * w[j];
        } else {
          const float wm = (((w[0] + w[1]) + w[2]) + w[3]) * 0.25f;
          if (wm != 0.f) s_box = wm * box_row<BOX, false>(a, b, bf, nullptr);
        }
      }
    }
  }
  // block reduction (fixed order -> deterministic)
  __shared__ float red[3][LB / 64];
  s_cls = wave_sum(s_cls); s_box = wave_sum(s_box); s_nor = wave_sum(s_nor);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s_cls; red[1][threadIdx.x >> 6] = s_box; red[2][threadIdx.x >> 6] = s_nor; }
  __syncthreads();
  if (threadIdx.x < 3) {
    float v = 0.f;
    for (int i = 0; i < LB / 64; ++i) v += red[threadIdx.x][i];
    partials[(long long)blockIdx.x * 3 + threadIdx.x] = v;
  }
}

// second stage: one block sums the per-block partials in a fixed order and ADDS into out[k]
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partials, long long nblocks, int k, float* __restrict__ out) {
  __shared__ float red[4];
  for (int j = 0; j < k; ++j) {
    float v = 0.f;
    for (long long i = threadIdx.x; i < nblocks; i += 256) v += partials[i * k + j];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[j] += red[0] + red[1] + red[2] + red[3];
    __syncthreads();
  }
}

// ... the same for every level of a level-fused launch: block l sums level l's partials (same order) and WRITES out[j * kstride + l * lstride]
// With `num_pos` (per-image positive counts of aod_max_iou_assign): the sums leave as the per-level loss terms of L_anchor_head.py:266-288 /
// SSL_Lambda.py:136-141 -- rows 0, 1 divided by num_total_samples = sum_b max(num_pos[b], 1) (L_anchor_head.py:300-303), row 2 (k = 3) by the
// level's row count (the mean of loss_noR) --, IEEE divisions like the tensor ops they replace; the divisors are kept for the backward pass.
__global__ __launch_bounds__(256) void reduce_partials_levels_kernel(const float* __restrict__ partials, const LossLevels lv, int k, float* __restrict__ out,
                                                                    int lstride, int kstride, const int* __restrict__ num_pos, int nimg,
                                                                    float* __restrict__ divisors, float* __restrict__ num_total) {
  __shared__ float red[4];
  int b0 = 0, b1 = lv.blk_end[0];
  long long r0 = 0, r1 = lv.row_end[0];
#pragma unroll
  for (int q = 0; q + 1 < MAXLV; ++q)
    if ((int)blockIdx.x > q) { b0 = lv.blk_end[q]; b1 = lv.blk_end[q + 1]; r0 = lv.row_end[q]; r1 = lv.row_end[q + 1]; }
  float nt = 1.f;
  if (num_pos && threadIdx.x == 0) {
    long long tot = 0;
    for (int b = 0; b < nimg; ++b) tot += max(num_pos[b], 1);
    nt = (float)tot;
    if (blockIdx.x == 0 && num_total) num_total[0] = nt;
  }
  const long long nblocks = b1 - b0;
  const float* pp = partials + (long long)b0 * k;
  for (int j = 0; j < k; ++j) {
    float v = 0.f;
    for (long long i = threadIdx.x; i < nblocks; i += 256) v += pp[i * k + j];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      const long long o = (long long)j * kstride + (long long)blockIdx.x * lstride;
      const float v = red[0] + red[1] + red[2] + red[3];
      if (num_pos) {
        const float d = j < 2 ? nt : (float)(r1 - r0);
        divisors[o] = d;
        out[o] = v / d;
      } else out[o] = v;
    }
    __syncthreads();
  }
}

static inline int edl_lpr(int C) { return C <= 24 ? 1 : 4; }
static inline long long edl_blocks(int64_t nrows, int C) { const int rb = LB / edl_lpr(C); return (nrows + rb - 1) / rb; }

// (sized for the LPR = 4 form: 64 rows per block)
extern "C" size_t aod_loss_partials_len(int64_t nrows) { return (size_t)((nrows + LB / 4 - 1) / (LB / 4)) * 3; }

// (one body per entry pair: `form` picks the kernel instantiation, `nm` names the entry in the error text)
#define AOD_FOCAL_FWD_(FORM_, LPR_, BOX_)                                                                                                  \
  hipLaunchKernelGGL((edl_l1_fwd_kernel<FORM_, BOX_, 24, LPR_>), dim3((unsigned)nb), dim3(LB), (size_t)(LB / LPR_) * (C | 1) * 4, (hipStream_t)stream, cls, \
                     (const long long*)labels, label_w, bbox_pred, bbox_tgt, bbox_w, lv, C, gamma, alpha, loss_noR, partials, bf)
#define AOD_FOCAL_FWD_B(FORM_, LPR_)                                                                                                       \
  do {                                                                                                                                     \
    if (box == BOX_GIOU) AOD_FOCAL_FWD_(FORM_, LPR_, BOX_GIOU); else if (box == BOX_IOU) AOD_FOCAL_FWD_(FORM_, LPR_, BOX_IOU);             \
    else AOD_FOCAL_FWD_(FORM_, LPR_, BOX_L1);                                                                                              \
  } while (0)
#define AOD_FOCAL_FWD()                                                                                                                    \
  do {                                                                                                                                     \
    if (form == FORM_SIGMOID) { if (C <= 24) AOD_FOCAL_FWD_B(FORM_SIGMOID, 1); else AOD_FOCAL_FWD_B(FORM_SIGMOID, 4); }                    \
    else { if (C <= 24) AOD_FOCAL_FWD_B(FORM_EDL, 1); else AOD_FOCAL_FWD_B(FORM_EDL, 4); }                                                 \
  } while (0)

// The `_ex` entries' box arguments -> (box, bf), checked; `nm` names the entry.  Box form l1 reads none of eps / linear / the coder (they
// may be anything, the pointers NULL): the entries without `_ex` forward here with it.
static const BoxForm BOX_FORM_L1 = {{0.f, 0.f, 0.f, 0.f}, {1.f, 1.f, 1.f, 1.f}, 0.f, 0.f, 0};
static int box_form_args(const char* nm, int focal_form, int box_form, const float* bbox_pred, float eps, int linear, const float* means4,
                         const float* stds4, float wh_ratio_clip, BoxForm& bf) {
  AOD_CHECK_ARG(focal_form == FORM_EDL || focal_form == FORM_SIGMOID, "%s: focal form must be 0 (edl) or 1 (sigmoid), got %d", nm, focal_form);
  AOD_CHECK_ARG(box_form >= BOX_L1 && box_form <= BOX_GIOU, "%s: box form must be 0 (l1), 1 (iou) or 2 (giou), got %d", nm, box_form);
  bf = BOX_FORM_L1;
  if (box_form == BOX_L1) return 0;
  AOD_CHECK_ARG(bbox_pred, "%s: box form %s needs bbox_pred", nm, box_form == BOX_IOU ? "iou" : "giou");
  AOD_CHECK_ARG(means4 && stds4, "%s: box form %s needs the coder's means and stds", nm, box_form == BOX_IOU ? "iou" : "giou");
  AOD_CHECK_ARG(fabsf(eps) <= 3.4028234e38f, "%s: eps must be finite (got %g)", nm, (double)eps);
  for (int j = 0; j < 4; ++j) {
    AOD_CHECK_ARG(fabsf(means4[j]) <= 3.4028234e38f && fabsf(stds4[j]) <= 3.4028234e38f, "%s: the coder's means and stds must be finite", nm);
    AOD_CHECK_ARG(stds4[j] > 0.f, "%s: the coder's stds must be > 0 (got %g)", nm, (double)stds4[j]);
    bf.mean[j] = means4[j]; bf.std[j] = stds4[j];
  }
  AOD_CHECK_ARG(wh_ratio_clip > 0.f && wh_ratio_clip <= 3.4028234e38f, "%s: wh_ratio_clip must be finite and > 0 (got %g)", nm, (double)wh_ratio_clip);
  bf.max_ratio = (float)fabs(log((double)wh_ratio_clip));      // |ln(wh_ratio_clip)| of delta2bbox, rounded once
  bf.eps = eps;
  bf.linear = linear != 0;
  return 0;
}

static int focal_l1_fwd(int form, int box, const BoxForm& bf, const char* nm, const float* cls, const int64_t* labels, const float* label_w,
                        const float* bbox_pred, const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha,
                        float* loss_noR, float* sums3, float* partials, aod_stream_t stream) {
  AOD_CHECK_ARG(nrows >= 0, "%s: negative row count", nm);
  if (nrows == 0) return 0;
  AOD_CHECK_ARG(cls && labels && label_w && loss_noR && sums3 && partials, "%s: null pointer", nm);
  AOD_CHECK_ARG(C >= 1 && C <= MAXC, "%s: C=%d out of range", nm, C);
  AOD_CHECK_ARG(!bbox_pred || (bbox_tgt && bbox_w), "%s: bbox_pred needs targets and weights", nm);
  LossLevels lv; long long tot;
  const long long nb = fill_levels(lv, 1, &nrows, LB / edl_lpr(C), tot);
  AOD_FOCAL_FWD();
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nb, 3, sums3);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_edl_focal_l1_fwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                    const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha,
                                    float* loss_noR, float* sums3, float* partials, aod_stream_t stream) {
  return focal_l1_fwd(FORM_EDL, BOX_L1, BOX_FORM_L1, "edl_fwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nrows, C, gamma, alpha, loss_noR, sums3,
                      partials, stream);
}
extern "C" int aod_focal_box_fwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                                    float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                    const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha, float* loss_noR,
                                    float* sums3, float* partials, aod_stream_t stream) {
  BoxForm bf;
  if (int e = box_form_args("focal_box_fwd_ex", focal_form, box_form, bbox_pred, box_eps, box_linear, means4, stds4, wh_ratio_clip, bf)) return e;
  return focal_l1_fwd(focal_form, box_form, bf, "focal_box_fwd_ex", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nrows, C, gamma, alpha, loss_noR,
                      sums3, partials, stream);
}
extern "C" int aod_sigmoid_focal_l1_fwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                        const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha,
                                        float* loss_noR, float* sums3, float* partials, aod_stream_t stream) {
  return focal_l1_fwd(FORM_SIGMOID, BOX_L1, BOX_FORM_L1, "sigmoid_focal_fwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nrows, C, gamma, alpha,
                      loss_noR, sums3, partials, stream);
}

extern "C" size_t aod_loss_levels_partials_len(int nlevels, const int64_t* level_rows) {
  size_t n = 0;
  for (int l = 0; l < nlevels; ++l) n += (size_t)((level_rows[l] + LB / 4 - 1) / (LB / 4)) * 3;
  return n;
}

static bool level_rows_ok(int nlevels, const int64_t* level_rows) {
  for (int l = 0; l < nlevels; ++l) if (level_rows[l] < 0) return false;
  return true;
}
static int focal_l1_levels_fwd(int form, int box, const BoxForm& bf, const char* nm, const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                               const float* bbox_tgt, const float* bbox_w, int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                               float* loss_noR, float* sums, float* partials, const int32_t* num_pos, int num_images, float* divisors,
                               float* num_total, aod_stream_t stream) {
  AOD_CHECK_ARG(nlevels >= 1 && nlevels <= MAXLV && level_rows, "%s: 1..8 levels", nm);
  AOD_CHECK_ARG(level_rows_ok(nlevels, level_rows), "%s: negative row count", nm);
  AOD_CHECK_ARG(!num_pos || (num_images >= 1 && divisors), "%s: num_pos needs the image count and a divisor buffer", nm);
  AOD_CHECK_ARG(cls && labels && label_w && loss_noR && sums && partials, "%s: null pointer", nm);
  AOD_CHECK_ARG(C >= 1 && C <= MAXC, "%s: C=%d out of range", nm, C);
  AOD_CHECK_ARG(!bbox_pred || (bbox_tgt && bbox_w), "%s: bbox_pred needs targets and weights", nm);
  LossLevels lv; long long tot;
  const int nb = fill_levels(lv, nlevels, level_rows, LB / edl_lpr(C), tot);
  if (nb) AOD_FOCAL_FWD();
  // sums[3][nlevels]: row 0 = sum l * w, row 1 = sum |d| * bw, row 2 = sum l, one column per level (an empty level: zeros)
  hipLaunchKernelGGL(reduce_partials_levels_kernel, dim3(nlevels), dim3(256), 0, (hipStream_t)stream, partials, lv, 3, sums, 1, nlevels, (const int*)num_pos,
                     num_images, divisors, num_total);
  AOD_LAUNCH_CHECK();
  return 0;
}
#undef AOD_FOCAL_FWD
#undef AOD_FOCAL_FWD_B
#undef AOD_FOCAL_FWD_
extern "C" int aod_edl_focal_l1_levels_fwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                           const float* bbox_tgt, const float* bbox_w, int nlevels, const int64_t* level_rows, int C, float gamma,
                                           float alpha, float* loss_noR, float* sums, float* partials, const int32_t* num_pos, int num_images,
                                           float* divisors, float* num_total, aod_stream_t stream) {
  return focal_l1_levels_fwd(FORM_EDL, BOX_L1, BOX_FORM_L1, "edl_levels_fwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nlevels, level_rows, C, gamma,
                             alpha, loss_noR, sums, partials, num_pos, num_images, divisors, num_total, stream);
}
extern "C" int aod_focal_box_levels_fwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                                           float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w,
                                           const float* bbox_pred, const float* bbox_tgt, const float* bbox_w, int nlevels,
                                           const int64_t* level_rows, int C, float gamma, float alpha, float* loss_noR, float* sums, float* partials,
                                           const int32_t* num_pos, int num_images, float* divisors, float* num_total, aod_stream_t stream) {
  BoxForm bf;
  if (int e = box_form_args("focal_box_levels_fwd_ex", focal_form, box_form, bbox_pred, box_eps, box_linear, means4, stds4, wh_ratio_clip, bf)) return e;
  return focal_l1_levels_fwd(focal_form, box_form, bf, "focal_box_levels_fwd_ex", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nlevels, level_rows, C,
                             gamma, alpha, loss_noR, sums, partials, num_pos, num_images, divisors, num_total, stream);
}
extern "C" int aod_sigmoid_focal_l1_levels_fwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                               const float* bbox_tgt, const float* bbox_w, int nlevels, const int64_t* level_rows, int C, float gamma,
                                               float alpha, float* loss_noR, float* sums, float* partials, const int32_t* num_pos, int num_images,
                                               float* divisors, float* num_total, aod_stream_t stream) {
  return focal_l1_levels_fwd(FORM_SIGMOID, BOX_L1, BOX_FORM_L1, "sigmoid_focal_levels_fwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nlevels,
                             level_rows, C, gamma, alpha, loss_noR, sums, partials, num_pos, num_images, divisors, num_total, stream);
}

// backward.  Output element (row r, class c) lives at (r / A) * pitch + (r % A) * C + c so that the
// gradient lands directly in the conv's [pixels, A*C (padded)] dZ layout, bf16 or fp32.
template <int FORM, int BOX, bool OUT_BF16, int CT, int LPR>
__global__ __launch_bounds__(LB) void edl_l1_bwd_kernel(const float* __restrict__ cls, const long long* __restrict__ labels,
                                                        const float* __restrict__ lw, const float* __restrict__ bp,
                                                        const float* __restrict__ bt, const float* __restrict__ bw, const LossLevels lv, int C,
                                                        float gamma, float alpha, const float* __restrict__ g_cls,
                                                        const float* __restrict__ g_bbox, const float* __restrict__ g_noR, float g_noR_s, int g_noR_bcast,
                                                        void* __restrict__ grad_cls, void* __restrict__ grad_bbox, int A, int pitch_cls,
                                                        int pitch_box, int g_lstride, const float* __restrict__ g_div, int nlv,
                                                        const BoxForm bf) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  constexpr int RB = LB / LPR;
  const int P = C | 1;
  int level, blk0; long long row0, rend;
  level_of_block(lv, (int)blockIdx.x, level, blk0, row0, rend);
  const long long r0 = row0 + (long long)((int)blockIdx.x - blk0) * RB;
  const int nr = (int)min((long long)RB, rend - r0);
  const int gl = level * g_lstride;          // the level's upstream gradients (per-level scalars of a level-fused launch; 0 otherwise)
  const int tot = nr * C;
  aod_stage_rows<LB>(cls + r0 * C, srow, nr, C, P);
  __shared__ long long s_obase[LB];       // element offset of each row's class 0 in the destination
  __syncthreads();
  const int lrow = threadIdx.x / LPR, part = threadIdx.x % LPR;
  const bool live = lrow < nr;
  const int row = live ? lrow : nr - 1;
  const int cpl = (C + LPR - 1) / LPR, c0 = part * cpl;
  const int n = min(cpl, C - c0);
  {
    const long long r = r0 + row;
    if (live && part == 0) s_obase[row] = (r / A) * pitch_cls + (r % A) * C;
    float x[CT], p[CT], gp[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) x[c] = c < n ? srow[row * P + c0 + c] : 0.f;
    float m = -INFINITY, S = 0.f;
    if (FORM == FORM_EDL) {
#pragma unroll
      for (int c = 0; c < CT; ++c) if (c < n) m = fmaxf(m, x[c]);
      m = grp_max<LPR>(m);
#pragma unroll
      for (int c = 0; c < CT; ++c) if (c < n) { p[c] = l_exp(x[c] - m); S += p[c]; }
      S = grp_sum<LPR>(S);
    }
    const long long label = labels[r];
    // (g_div: the upstream gradients are those of the DIVIDED sums -- the quotient is what autograd's division backward forms)
    const float gc_ = g_div ? g_cls[gl] / g_div[gl] : g_cls[gl];
    const float gn_ = g_noR ? (g_noR_bcast ? (g_div ? g_noR[gl] / g_div[2 * nlv + gl] : g_noR[gl]) : g_noR[r]) : g_noR_s;
    const float coef = gc_ * lw[r] + gn_;
    float dot = 0.f;
    if (FORM == FORM_SIGMOID) {
      // per class, no softmax Jacobian: d/dx_c = coef * d l_c / d x_c, back into the LDS row like the EDL form's below
      if (live) {
#pragma unroll
        for (int c = 0; c < CT; ++c) if (c < n) {
          float gz;
          sig_focal_term(x[c], label == c0 + c, gamma, alpha, &gz);
          srow[row * P + c0 + c] = coef * gz;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) if (c < n) {
        const float pr = l_div(p[c], S);
        p[c] = pr;
        const float om = 1.f - pr + 1e-9f;
        const float u = l_div(pr, om);
        const float z = l_log(u + 1e-9f);
        const float q = l_div(1.f, 1.f + l_exp(-z));
        const bool pos = label == c0 + c;
        const float lg = l_log(fmaxf(pos ? q : 1.f - q, FLT_MIN_F));
        float gz;   // d l / d z  (mmcv sigmoid_focal_loss backward)
        if (pos) gz = -alpha * focal_pow(1.f - q, gamma) * (1.f - q - gamma * q * lg);
        else gz = -(1.f - alpha) * focal_pow(q, gamma) * (gamma * (1.f - q) * lg - q);
        // dz/dp = (1+eps) / ((1-p+eps)^2 (u+eps))
        const float g = l_div(coef * gz * (1.f + 1e-9f), om * om * (u + 1e-9f));
        gp[c] = g;
        dot += pr * g;
      }
      dot = grp_sum<LPR>(dot);
      // the row's gradient goes back into its LDS row; the block then stores all rows with consecutive lanes on consecutive elements
      // (one thread storing its own 20 values writes 4 B per lane at an 80-B lane stride)
      if (live) {
#pragma unroll
        for (int c = 0; c < CT; ++c) if (c < n) srow[row * P + c0 + c] = p[c] * (gp[c] - dot);
      }
    }
    if (live && part == 0 && bp && grad_bbox) {
      const float gb = g_div ? g_bbox[gl] / g_div[nlv + gl] : g_bbox[gl];
      const long long bb = (r / A) * pitch_box + (r % A) * 4;
      if constexpr (BOX == BOX_L1) {
        for (int j = 0; j < 4; ++j) {
          const float d = bp[r * 4 + j] - bt[r * 4 + j];
          const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
          const float gx = sgn * bw[r * 4 + j] * gb;
          if (OUT_BF16) ((bf16_t*)grad_bbox)[bb + j] = (bf16_t)gx;
          else ((float*)grad_bbox)[bb + j] = gx;
        }
      } else {
        const f32x4 w = *reinterpret_cast<const f32x4*>(bw + r * 4);
        const float wm = (((w[0] + w[1]) + w[2]) + w[3]) * 0.25f;
        float g4[4] = {0.f, 0.f, 0.f, 0.f};
        if (wm != 0.f) {
          box_row<BOX, true>(*reinterpret_cast<const f32x4*>(bp + r * 4), *reinterpret_cast<const f32x4*>(bt + r * 4), bf, g4);
#pragma unroll
          for (int j = 0; j < 4; ++j) g4[j] = gb * wm * g4[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (OUT_BF16) ((bf16_t*)grad_bbox)[bb + j] = (bf16_t)g4[j];
          else ((float*)grad_bbox)[bb + j] = g4[j];
        }
      }
    }
  }
  __syncthreads();
  {
    const int drow = LB / C, dcol = LB - drow * C;
    int row = (int)threadIdx.x / C, c = (int)threadIdx.x - row * C;
    for (int i = threadIdx.x; i < tot; i += LB) {
      const long long o = s_obase[row] + c;
      const float gx = srow[row * P + c];
      if (OUT_BF16) ((bf16_t*)grad_cls)[o] = (bf16_t)gx;
      else ((float*)grad_cls)[o] = gx;
      row += drow; c += dcol;
      if (c >= C) { c -= C; ++row; }
    }
  }
}

#define AOD_FOCAL_BWD_(FORM_, BOX_, BF, LPR_)                                                                                              \
  hipLaunchKernelGGL((edl_l1_bwd_kernel<FORM_, BOX_, BF, 24, LPR_>), dim3((unsigned)nb), dim3(LB), (size_t)(LB / LPR_) * (C | 1) * 4, (hipStream_t)stream, cls, \
                     (const long long*)labels, label_w, bbox_pred, bbox_tgt, bbox_w, lv, C, gamma, alpha, g_cls, g_bbox, g_noR, \
                     g_noR_scalar, g_noR_is_scalar, grad_cls, grad_bbox, A, pitch_cls, pitch_box, g_lstride, g_div, nlv_, bf)
#define AOD_FOCAL_BWD_B(FORM_, BOX_)                                                                                                       \
  do {                                                                                                                                     \
    if (out_bf16) { if (C <= 24) AOD_FOCAL_BWD_(FORM_, BOX_, true, 1); else AOD_FOCAL_BWD_(FORM_, BOX_, true, 4); }                        \
    else { if (C <= 24) AOD_FOCAL_BWD_(FORM_, BOX_, false, 1); else AOD_FOCAL_BWD_(FORM_, BOX_, false, 4); }                               \
  } while (0)
#define AOD_FOCAL_BWD_F(FORM_)                                                                                                             \
  do {                                                                                                                                     \
    if (box == BOX_GIOU) AOD_FOCAL_BWD_B(FORM_, BOX_GIOU); else if (box == BOX_IOU) AOD_FOCAL_BWD_B(FORM_, BOX_IOU);                       \
    else AOD_FOCAL_BWD_B(FORM_, BOX_L1);                                                                                                   \
  } while (0)
#define AOD_FOCAL_BWD()                                                                                                                    \
  do {                                                                                                                                     \
    if (form == FORM_SIGMOID) AOD_FOCAL_BWD_F(FORM_SIGMOID); else AOD_FOCAL_BWD_F(FORM_EDL);                                               \
  } while (0)
static int focal_l1_bwd(int form, int box, const BoxForm& bf, const char* nm, const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                        const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha, const float* g_cls,
                        const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar, void* grad_cls, void* grad_bbox,
                        int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  AOD_CHECK_ARG(nrows >= 0, "%s: negative row count", nm);
  if (nrows == 0) return 0;
  AOD_CHECK_ARG(cls && labels && label_w && g_cls && grad_cls, "%s: null pointer", nm);
  AOD_CHECK_ARG(C >= 1 && C <= MAXC && A >= 1 && pitch_cls >= A * C, "%s: bad C/A/pitch", nm);
  AOD_CHECK_ARG(!grad_bbox || (bbox_pred && bbox_tgt && bbox_w && g_bbox && pitch_box >= A * 4), "%s: bbox args", nm);
  LossLevels lv; long long tot;
  const long long nb = fill_levels(lv, 1, &nrows, LB / edl_lpr(C), tot);
  const int g_lstride = 0, nlv_ = 1;
  const float* const g_div = nullptr;
  AOD_FOCAL_BWD();
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_edl_focal_l1_bwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                    const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha,
                                    const float* g_cls, const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar,
                                    void* grad_cls, void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  return focal_l1_bwd(FORM_EDL, BOX_L1, BOX_FORM_L1, "edl_bwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nrows, C, gamma, alpha, g_cls, g_bbox, g_noR,
                      g_noR_scalar, g_noR_is_scalar, grad_cls, grad_bbox, out_bf16, A, pitch_cls, pitch_box, stream);
}
extern "C" int aod_focal_box_bwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                                    float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                    const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha, const float* g_cls,
                                    const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar, void* grad_cls,
                                    void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  BoxForm bf;
  if (int e = box_form_args("focal_box_bwd_ex", focal_form, box_form, bbox_pred, box_eps, box_linear, means4, stds4, wh_ratio_clip, bf)) return e;
  return focal_l1_bwd(focal_form, box_form, bf, "focal_box_bwd_ex", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nrows, C, gamma, alpha, g_cls, g_bbox,
                      g_noR, g_noR_scalar, g_noR_is_scalar, grad_cls, grad_bbox, out_bf16, A, pitch_cls, pitch_box, stream);
}
extern "C" int aod_sigmoid_focal_l1_bwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                        const float* bbox_tgt, const float* bbox_w, int64_t nrows, int C, float gamma, float alpha,
                                        const float* g_cls, const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar,
                                        void* grad_cls, void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  return focal_l1_bwd(FORM_SIGMOID, BOX_L1, BOX_FORM_L1, "sigmoid_focal_bwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nrows, C, gamma, alpha, g_cls, g_bbox, g_noR,
                      g_noR_scalar, g_noR_is_scalar, grad_cls, grad_bbox, out_bf16, A, pitch_cls, pitch_box, stream);
}

// g_sums[3][nlevels] = the gradients of aod_edl_focal_l1_levels_fwd's sums (row 0: classification sums, row 1: box sums, row 2: row sums) --
// of the DIVIDED sums when `divisors` (the forward's) is given: the kernel forms g / divisor itself;
// g_noR_rows (optional): a gradient per anchor row of loss_noR, replaces row 2.
static int focal_l1_levels_bwd(int form, int box, const BoxForm& bf, const char* nm, const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                               const float* bbox_tgt, const float* bbox_w, int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                               const float* g_sums, const float* divisors, const float* g_noR_rows, void* grad_cls, void* grad_bbox, int out_bf16,
                               int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  AOD_CHECK_ARG(nlevels >= 1 && nlevels <= MAXLV && level_rows, "%s: 1..8 levels", nm);
  AOD_CHECK_ARG(level_rows_ok(nlevels, level_rows), "%s: negative row count", nm);
  AOD_CHECK_ARG(cls && labels && label_w && g_sums && grad_cls, "%s: null pointer", nm);
  AOD_CHECK_ARG(C >= 1 && C <= MAXC && A >= 1 && pitch_cls >= A * C, "%s: bad C/A/pitch", nm);
  AOD_CHECK_ARG(!grad_bbox || (bbox_pred && bbox_tgt && bbox_w && pitch_box >= A * 4), "%s: bbox args", nm);
  LossLevels lv; long long tot;
  const int nb = fill_levels(lv, nlevels, level_rows, LB / edl_lpr(C), tot);
  if (nb == 0) return 0;
  const float* g_cls = g_sums; const float* g_bbox = g_sums + nlevels;
  const float* g_noR = g_noR_rows ? g_noR_rows : g_sums + 2 * nlevels;
  const float g_noR_scalar = 0.f; const int g_noR_is_scalar = g_noR_rows ? 0 : 1, g_lstride = 1, nlv_ = nlevels;
  const float* const g_div = divisors;
  AOD_FOCAL_BWD();
  AOD_LAUNCH_CHECK();
  return 0;
}
#undef AOD_FOCAL_BWD
#undef AOD_FOCAL_BWD_F
#undef AOD_FOCAL_BWD_B
#undef AOD_FOCAL_BWD_
extern "C" int aod_edl_focal_l1_levels_bwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                           const float* bbox_tgt, const float* bbox_w, int nlevels, const int64_t* level_rows, int C, float gamma,
                                           float alpha, const float* g_sums, const float* divisors, const float* g_noR_rows, void* grad_cls,
                                           void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  return focal_l1_levels_bwd(FORM_EDL, BOX_L1, BOX_FORM_L1, "edl_levels_bwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nlevels, level_rows, C, gamma,
                             alpha, g_sums, divisors, g_noR_rows, grad_cls, grad_bbox, out_bf16, A, pitch_cls, pitch_box, stream);
}
extern "C" int aod_focal_box_levels_bwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                                           float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w,
                                           const float* bbox_pred, const float* bbox_tgt, const float* bbox_w, int nlevels,
                                           const int64_t* level_rows, int C, float gamma, float alpha, const float* g_sums, const float* divisors,
                                           const float* g_noR_rows, void* grad_cls, void* grad_bbox, int out_bf16, int A, int pitch_cls,
                                           int pitch_box, aod_stream_t stream) {
  BoxForm bf;
  if (int e = box_form_args("focal_box_levels_bwd_ex", focal_form, box_form, bbox_pred, box_eps, box_linear, means4, stds4, wh_ratio_clip, bf)) return e;
  return focal_l1_levels_bwd(focal_form, box_form, bf, "focal_box_levels_bwd_ex", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nlevels, level_rows, C,
                             gamma, alpha, g_sums, divisors, g_noR_rows, grad_cls, grad_bbox, out_bf16, A, pitch_cls, pitch_box, stream);
}
extern "C" int aod_sigmoid_focal_l1_levels_bwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred,
                                               const float* bbox_tgt, const float* bbox_w, int nlevels, const int64_t* level_rows, int C, float gamma,
                                               float alpha, const float* g_sums, const float* divisors, const float* g_noR_rows, void* grad_cls,
                                               void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream) {
  return focal_l1_levels_bwd(FORM_SIGMOID, BOX_L1, BOX_FORM_L1, "sigmoid_focal_levels_bwd", cls, labels, label_w, bbox_pred, bbox_tgt, bbox_w, nlevels, level_rows, C, gamma,
                             alpha, g_sums, divisors, g_noR_rows, grad_cls, grad_bbox, out_bf16, A, pitch_cls, pitch_box, stream);
}

// ---------------------------------------------------------------- MEH loss
// FORM (launch-uniform, one kernel instance each): how the Model Evidence Head is regressed onto the detached per-anchor loss
//   0  L2    sum(((|lam + 1e-9 - loss|) * w)^2)                       Lambda_L2.py:235-241
//   1  L1    sum(|(|lam + 1e-9 - loss|) * w|)                         Lambda_L1.py:239-241
//   2  MSLE  sum(((|log(lam + 1e-9 + 1) - log(loss + 1)|) * w)^2)     Lambda_MSLE.py:239-242
// The gradients are autograd's, factor by factor: abs' = sign (0 at 0), so the L1 gradient is g * sign(|d| * w) * w * sign(d) = g * |w| * sign(d)
// (a negative weight flips twice) and 0 where lam + 1e-9 == loss; MSLE's is ((g * 2 * (|d| * w)) * w) * sign(d) / (lam + 1e-9 + 1).  The two
// logs cancel where lam ~ loss: the accurate logf, not the hardware log2 -- the kernels are bound by their three input streams.
__device__ __forceinline__ float sign0(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
template <int FORM>
__global__ __launch_bounds__(256) void meh_fwd_kernel(const float* __restrict__ lam, const float* __restrict__ loss, const float* __restrict__ bw4,
                                                      const LossLevels lv, float* __restrict__ partials) {
  float s = 0.f;
  int level, blk0; long long row0, n;
  level_of_block(lv, (int)blockIdx.x, level, blk0, row0, n);
  const long long i = row0 + (long long)((int)blockIdx.x - blk0) * 256 + threadIdx.x;
  if (i < n) {
    if (FORM == 1) {
      s = fabsf(fabsf(lam[i] + 1e-9f - loss[i]) * bw4[i * 4]);
    } else if (FORM == 2) {
      const float d = fabsf(logf(lam[i] + 1e-9f + 1.f) - logf(loss[i] + 1.f)) * bw4[i * 4];
      s = d * d;
    } else {
      const float d = fabsf(lam[i] + 1e-9f - loss[i]) * bw4[i * 4];
      s = d * d;
    }
  }
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
template <bool OUT_BF16, int FORM>
__global__ void meh_bwd_kernel(const float* __restrict__ lam, const float* __restrict__ loss, const float* __restrict__ bw4, const LossLevels lv,
                               const float* __restrict__ g, void* __restrict__ grad, int A, int pitch, int g_lstride) {
  int level, blk0; long long row0, n;
  level_of_block(lv, (int)blockIdx.x, level, blk0, row0, n);
  const long long i = row0 + (long long)((int)blockIdx.x - blk0) * 256 + threadIdx.x;
  if (i < n) {
    const float w = bw4[i * 4];
    float v;
    if (FORM == 1) {
      const float d = lam[i] + 1e-9f - loss[i];
      v = g[level * g_lstride] * sign0(fabsf(d) * w) * w * sign0(d);
    } else if (FORM == 2) {
      const float x = lam[i] + 1e-9f + 1.f;
      const float d = logf(x) - logf(loss[i] + 1.f);
      v = g[level * g_lstride] * 2.f * (fabsf(d) * w) * w * sign0(d) / x;
    } else {
      v = g[level * g_lstride] * 2.f * w * w * (lam[i] + 1e-9f - loss[i]);
    }
    const long long o = (i / A) * pitch + (i % A);
    if (OUT_BF16) ((bf16_t*)grad)[o] = (bf16_t)v; else ((float*)grad)[o] = v;
  }
}
#define AOD_MEH_FWD(nb_)                                                                                                                   \
  do {                                                                                                                                     \
    if (form == 1) hipLaunchKernelGGL(meh_fwd_kernel<1>, dim3((unsigned)(nb_)), dim3(256), 0, (hipStream_t)stream, lam, loss_noR, bbox_w4, lv, partials); \
    else if (form == 2) hipLaunchKernelGGL(meh_fwd_kernel<2>, dim3((unsigned)(nb_)), dim3(256), 0, (hipStream_t)stream, lam, loss_noR, bbox_w4, lv, partials); \
    else hipLaunchKernelGGL(meh_fwd_kernel<0>, dim3((unsigned)(nb_)), dim3(256), 0, (hipStream_t)stream, lam, loss_noR, bbox_w4, lv, partials); \
  } while (0)
#define AOD_MEH_BWD_(BF, F_, nb_, ls_)                                                                                                     \
  hipLaunchKernelGGL((meh_bwd_kernel<BF, F_>), dim3((unsigned)(nb_)), dim3(256), 0, (hipStream_t)stream, lam, loss_noR, bbox_w4, lv, g, grad_lam, A, pitch, ls_)
#define AOD_MEH_BWD(nb_, ls_)                                                                                                              \
  do {                                                                                                                                     \
    if (out_bf16) { if (form == 1) AOD_MEH_BWD_(true, 1, nb_, ls_); else if (form == 2) AOD_MEH_BWD_(true, 2, nb_, ls_); else AOD_MEH_BWD_(true, 0, nb_, ls_); } \
    else { if (form == 1) AOD_MEH_BWD_(false, 1, nb_, ls_); else if (form == 2) AOD_MEH_BWD_(false, 2, nb_, ls_); else AOD_MEH_BWD_(false, 0, nb_, ls_); } \
  } while (0)
extern "C" int aod_meh_loss_fwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n, int form, float* out_sum,
                                   float* partials, aod_stream_t stream) {
  AOD_CHECK_ARG(lam && loss_noR && bbox_w4 && out_sum && partials, "meh_fwd: null pointer");
  AOD_CHECK_ARG(form >= 0 && form <= 2, "meh_fwd: form must be 0 (L2), 1 (L1) or 2 (MSLE)");
  if (n == 0) return 0;
  LossLevels lv; long long tot;
  const long long nb = fill_levels(lv, 1, &n, 256, tot);
  AOD_MEH_FWD(nb);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nb, 1, out_sum);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_meh_loss_fwd(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n, float* out_sum, float* partials,
                                aod_stream_t stream) {
  return aod_meh_loss_fwd_ex(lam, loss_noR, bbox_w4, n, 0, out_sum, partials, stream);
}
// all levels in one launch (Lambda_L2.py:235-241 / Lambda_L1.py:236-241 / Lambda_MSLE.py:236-242 once per level): out_sums[nlevels]
extern "C" int aod_meh_loss_levels_fwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                                          int form, float* out_sums, float* partials, aod_stream_t stream) {
  AOD_CHECK_ARG(nlevels >= 1 && nlevels <= MAXLV && level_rows, "meh_levels_fwd: 1..8 levels");
  AOD_CHECK_ARG(lam && loss_noR && bbox_w4 && out_sums && partials, "meh_levels_fwd: null pointer");
  AOD_CHECK_ARG(form >= 0 && form <= 2, "meh_levels_fwd: form must be 0 (L2), 1 (L1) or 2 (MSLE)");
  LossLevels lv; long long tot;
  const int nb = fill_levels(lv, nlevels, level_rows, 256, tot);
  if (nb) AOD_MEH_FWD(nb);
  hipLaunchKernelGGL(reduce_partials_levels_kernel, dim3(nlevels), dim3(256), 0, (hipStream_t)stream, partials, lv, 1, out_sums, 1, nlevels, (const int*)nullptr,
                     0, (float*)nullptr, (float*)nullptr);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_meh_loss_levels_fwd(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                                       float* out_sums, float* partials, aod_stream_t stream) {
  return aod_meh_loss_levels_fwd_ex(lam, loss_noR, bbox_w4, nlevels, level_rows, 0, out_sums, partials, stream);
}
extern "C" int aod_meh_loss_bwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n, int form, const float* g,
                                   void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream) {
  AOD_CHECK_ARG(lam && loss_noR && bbox_w4 && g && grad_lam && A >= 1 && pitch >= A, "meh_bwd: bad args");
  AOD_CHECK_ARG(form >= 0 && form <= 2, "meh_bwd: form must be 0 (L2), 1 (L1) or 2 (MSLE)");
  if (n == 0) return 0;
  LossLevels lv; long long tot;
  const long long nb = fill_levels(lv, 1, &n, 256, tot);
  AOD_MEH_BWD(nb, 0);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_meh_loss_bwd(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n, const float* g, void* grad_lam,
                                int out_bf16, int A, int pitch, aod_stream_t stream) {
  return aod_meh_loss_bwd_ex(lam, loss_noR, bbox_w4, n, 0, g, grad_lam, out_bf16, A, pitch, stream);
}
extern "C" int aod_meh_loss_levels_bwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                                          int form, const float* g, void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream) {
  AOD_CHECK_ARG(nlevels >= 1 && nlevels <= MAXLV && level_rows, "meh_levels_bwd: 1..8 levels");
  AOD_CHECK_ARG(lam && loss_noR && bbox_w4 && g && grad_lam && A >= 1 && pitch >= A, "meh_levels_bwd: bad args");
  AOD_CHECK_ARG(form >= 0 && form <= 2, "meh_levels_bwd: form must be 0 (L2), 1 (L1) or 2 (MSLE)");
  LossLevels lv; long long tot;
  const int nb = fill_levels(lv, nlevels, level_rows, 256, tot);
  if (nb == 0) return 0;
  AOD_MEH_BWD(nb, 1);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_meh_loss_levels_bwd(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                                       const float* g, void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream) {
  return aod_meh_loss_levels_bwd_ex(lam, loss_noR, bbox_w4, nlevels, level_rows, 0, g, grad_lam, out_bf16, A, pitch, stream);
}
#undef AOD_MEH_FWD
#undef AOD_MEH_BWD
#undef AOD_MEH_BWD_

// ---------------------------------------------------------------------------------------------------------------------------------
// Elementwise form [rows, C] of the EDL softmax-focal loss: what EDL_Softmax_FocalLoss.forward(reduction='none') returns in the
// reference (EDL_Softmax_FocalLoss.py:51-69 -> mmcv sigmoid_focal_loss(..., 'none')).  Lambda_L2Net.loss_single never needs it (its
// 'none' caller sums over the classes at once, Lambda_L2.py:116: the fused row kernel above) -- this serves stand-alone drop-in callers.
// One lane per row, classes streamed from global memory in three passes (same formulas and order as edl_row_fwd); not a hot kernel.
__device__ __forceinline__ float edl_elem_terms(float pr, bool pos, float gamma, float alpha, float* gz_out) {
  const float om = 1.f - pr + 1e-9f;
  const float u = l_div(pr, om);
  const float z = l_log(u + 1e-9f);
  const float q = l_div(1.f, 1.f + l_exp(-z));
  const float lg = l_log(fmaxf(pos ? q : 1.f - q, FLT_MIN_F));
  if (gz_out) {
    float gz;
    if (pos) gz = -alpha * focal_pow(1.f - q, gamma) * (1.f - q - gamma * q * lg);
    else gz = -(1.f - alpha) * focal_pow(q, gamma) * (gamma * (1.f - q) * lg - q);
    *gz_out = l_div(gz * (1.f + 1e-9f), om * om * (u + 1e-9f));       // d l / d p
  }
  return pos ? -alpha * focal_pow(1.f - q, gamma) * lg : -(1.f - alpha) * focal_pow(q, gamma) * lg;
}

template <int FORM>
__global__ __launch_bounds__(256) void edl_elem_kernel(const float* __restrict__ cls, const long long* __restrict__ labels, long long nrows, int C,
                                                      float gamma, float alpha, const float* __restrict__ g, float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= nrows) return;
  const float* x = cls + r * C;
  if (FORM == FORM_SIGMOID) {      // per class: out[r][c] = l_c (forward) or g[r][c] * d l_c / d x_c (backward)
    const long long label = labels[r];
    for (int c = 0; c < C; ++c) {
      float gz;
      const float l = sig_focal_term(x[c], label == c, gamma, alpha, g ? &gz : nullptr);
      out[r * C + c] = g ? g[r * C + c] * gz : l;
    }
    return;
  }
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
  float S = 0.f;
  for (int c = 0; c < C; ++c) S += l_exp(x[c] - m);
  const long long label = labels[r];
  if (!g) {                    // forward: out[r][c] = l_c
    for (int c = 0; c < C; ++c) out[r * C + c] = edl_elem_terms(l_div(l_exp(x[c] - m), S), label == c, gamma, alpha, nullptr);
    return;
  }
  // backward: out[r][k] = p_k * (G_k - sum_c p_c G_c),  G_c = g[r][c] * d l_c / d p_c
  float dot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float pr = l_div(l_exp(x[c] - m), S);
    float dl;
    edl_elem_terms(pr, label == c, gamma, alpha, &dl);
    dot += pr * (g[r * C + c] * dl);
  }
  for (int c = 0; c < C; ++c) {
    const float pr = l_div(l_exp(x[c] - m), S);
    float dl;
    edl_elem_terms(pr, label == c, gamma, alpha, &dl);
    out[r * C + c] = pr * (g[r * C + c] * dl - dot);
  }
}

extern "C" int aod_edl_focal_elem(const float* cls, const int64_t* labels, int64_t nrows, int C, float gamma, float alpha,
                                  const float* grad_out, float* out, aod_stream_t stream) {
  if (nrows == 0) return 0;
  AOD_CHECK_ARG(cls && labels && out, "edl_elem: null pointer");
  AOD_CHECK_ARG(C >= 1, "edl_elem: C=%d out of range", C);
  hipLaunchKernelGGL(edl_elem_kernel<FORM_EDL>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cls, (const long long*)labels,
                     (long long)nrows, C, gamma, alpha, grad_out, out);
  AOD_LAUNCH_CHECK();
  return 0;
}

// the plain form's [rows, C] loss: FocalLoss.forward(reduction='none') (focal_loss.py:85 -> mmcv sigmoid_focal_loss(..., 'none'))
extern "C" int aod_sigmoid_focal_elem(const float* cls, const int64_t* labels, int64_t nrows, int C, float gamma, float alpha,
                                      const float* grad_out, float* out, aod_stream_t stream) {
  AOD_CHECK_ARG(nrows >= 0, "sigmoid_focal_elem: negative row count");
  if (nrows == 0) return 0;
  AOD_CHECK_ARG(cls && labels && out, "sigmoid_focal_elem: null pointer");
  AOD_CHECK_ARG(C >= 1 && C <= MAXC, "sigmoid_focal_elem: C=%d out of range", C);
  hipLaunchKernelGGL(edl_elem_kernel<FORM_SIGMOID>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cls,
                     (const long long*)labels, (long long)nrows, C, gamma, alpha, grad_out, out);
  AOD_LAUNCH_CHECK();
  return 0;
}
