// CCMS acquisition: the instance-level half of PPAL (C. Yang, L. Huang, E. J. Crowley, "Plug and Play Active Learning for
// Object Detection", CVPR 2024) -- object descriptors and the category-conditioned matching distance between two images.  The reference
// tree has no such pool: the semantics are fixed in DESIGN 3o.
//
// 1. object_descriptors_kernel: one workgroup of 256 threads per image.
//      a. a thread per detection row: the gate (j < num[b], score > score_thr, strict), the candidate row k = obj_cand[b][j] that
//         aod_det_uncertainty_ex found, its anchor g = cand_anchor[b][k], the level l with anchor0_l <= g < anchor0_{l+1} and the cell
//         (g - anchor0_l) / num_anchors_l -> the row of the pyramid buffer, into LDS.  An object without a candidate row (or whose
//         anchor names no cell) is skipped and counted in missing[b].
//      b. thread 0 walks the rows in order and keeps the first max_obj objects.
//      c. a wave per kept object: 16-B loads of the row in either layout (plain bf16, or X-layout head + tail as pool_descriptor reads
//         it), lane j owns octets j and j + 64; sum of squares: per lane in element order, xor butterfly; f = v / sqrt(sum), all zeros
//         when the sum is 0.  A function of the row alone: the same bits for an image alone and inside a batch.  Slots >= cnt[b] are
//         written as (zeros, class -1, weight 0).
// 2. ccms_distance_kernel: d(a, b) = max(0, 1 - (S(a->b) + S(b->a)) / 2), S(a->b) = sum_i w_i m_i / sum_i w_i,
//    m_i = max(0, max_{j in b, c_j = c_i} <f_i, f_j>).  Images are padded to blocks of 32 objects (max_obj <= 64: one or two blocks).
//      * a workgroup keeps CC_BLOCKS = 4 blocks of a-images resident in LDS (4 images of <= 32 objects, 2 of <= 64; rows padded by 4
//        floats against bank conflicts: 4 x 32 x 260 x 4 B = 130 KB at C = 256) and streams b-images through them: each of the 4 waves
//        takes every fourth b-image of the workgroup's chunk, holds one 32-object block of it in registers (one 16-B load per 8
//        channels: 128 VGPRs at C = 256) and multiplies it with every resident block on v_mfma_f32_32x32x2_f32.
//      * the f32-input MFMA is bit for bit a k-ordered fmaf chain.  Lane half h feeds channels 8s + 4h .. 8s + 4h + 3 of step s, so the
//        chain takes the channels in the order 0 4 1 5 2 6 3 7 8 12 ...: a function of k alone.  Channels are padded with zeros to 64,
//        128 or 256 (fma(0, 0, acc) = acc).  <f_i, f_j> therefore has the same bits whichever image is the a-image, and an entry is a
//        function of the two images alone -- not of M, of its position, or of the tiling.
//      * both directions come out of the one 32 x 32 product tile: the column maximum (over the 16 accumulator registers and the two
//        lane halves) is m_j of the b-image, the row maximum (a 5-step butterfly over the 32 lanes of a half) is m_i of the a-image.
//        The maxima go to a per-wave LDS strip; lane t then adds the two weighted sums of a-image t in row order.  No atomics.
//      * only b >= the first image of the a-group is computed; a pair outside the group is written to d[a][b] and d[b][a] from the one
//        value, a pair inside it is computed in both orders (the same bits: products and the two-term sum commute).  d(a, a) = 0.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/aod_hip.h"
#include "row_layout.h"

#define OD_MAX_SEG 8
#define OD_MAX_DET 1024
#define OD_MAX_OBJ 64
#define OD_MAX_C 1024
#define CC_MAX_C 256
#define CC_PAD 4
#define CC_BLOCKS 4           // resident 32-object blocks of a-images
#define CC_ROWS (CC_BLOCKS * 32)
#define CC_BCHUNK 128         // b-images per workgroup: 32 per wave
#define CC_MAX_M 32768

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// ------------------------------------------------------------------------------------------------------------------ descriptors
struct OdSegs {
  const bf16_t* base[OD_MAX_SEG];      // first row of the level (image 0)
  long long a0[OD_MAX_SEG + 1];        // first global anchor id of the level
  int hw[OD_MAX_SEG];                  // cells (rows) per image
  int na[OD_MAX_SEG];                  // anchors per cell
  int nseg;
};

__global__ __launch_bounds__(256) void object_descriptors_kernel(const OdSegs s, int C, int x3, const int* __restrict__ cand_anchor, int n,
                                                                 const float* __restrict__ dets, const long long* __restrict__ labels,
                                                                 const int* __restrict__ num, const int* __restrict__ obj_cand, int max_num,
                                                                 int max_obj, float thr, float* __restrict__ feat, int* __restrict__ cls,
                                                                 float* __restrict__ w, int* __restrict__ cnt, int* __restrict__ missing) {
  __shared__ int state[OD_MAX_DET];            // -2: no object; -1: an object without a row; else the level of its row
  __shared__ long long rowoff[OD_MAX_DET];     // row of the level's map (image b included)
  __shared__ int slot_det[OD_MAX_OBJ];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* dt = dets + (long long)b * max_num * 5;
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  for (int j = tid; j < max_num; j += 256) {
    int st = -2;
    long long ro = 0;
    if (j < nd && dt[j * 5 + 4] > thr) {
      st = -1;
      const int k = obj_cand[(long long)b * max_num + j];
      const long long q = labels[(long long)b * max_num + j];
      if (k >= 0 && k < n && q >= 0 && q <= (long long)INT_MAX) {
        const long long g = cand_anchor[(long long)b * n + k];
        for (int l = 0; l < s.nseg; ++l) {
          if (g >= s.a0[l] && g < s.a0[l + 1]) {
            st = l;
            ro = (long long)b * s.hw[l] + (g - s.a0[l]) / s.na[l];      // (g < a0[l + 1] = a0[l] + hw * na: the cell is inside the image)
          }
        }
      }
    }
    state[j] = st;
    rowoff[j] = ro;
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0, miss = 0;
    for (int j = 0; j < max_num; ++j) {
      const int st = state[j];
      if (st == -2) continue;
      if (st == -1) { ++miss; continue; }
      if (c < max_obj) slot_det[c++] = j;
    }
    s_cnt = c;
    cnt[b] = c;
    missing[b] = miss;
  }
  __syncthreads();
  const int c = s_cnt, lane = tid & 63;
  const long long pitch = x3 ? 2ll * ((C + 31) / 32 * 32) : (long long)C;
  for (int sl = tid >> 6; sl < max_obj; sl += 4) {
    float* fo = feat + ((long long)b * max_obj + sl) * C;
    if (sl >= c) {                                                 // wave-uniform
      for (int o = lane; o * 8 < C; o += 64) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(fo + o * 8) = z;
        *reinterpret_cast<f32x4*>(fo + o * 8 + 4) = z;
      }
      if (lane == 0) { cls[(long long)b * max_obj + sl] = -1; w[(long long)b * max_obj + sl] = 0.f; }
      continue;
    }
    const int j = slot_det[sl];
    const bf16_t* p = s.base[state[j]] + rowoff[j] * pitch;
    float v[2][8];
    float ss = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int o = lane + 64 * m;
#pragma unroll
      for (int u = 0; u < 8; ++u) v[m][u] = 0.f;
      if (o * 8 < C) {
        const int col = row_col(x3, o);
        row_load(p + col, x3, v[m]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) ss += v[m][u] * v[m][u];
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int o = lane + 64 * m;
      if (o * 8 < C) {
        f32x4 lo, hi;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          lo[u] = ss > 0.f ? v[m][u] / nrm : 0.f;
          hi[u] = ss > 0.f ? v[m][4 + u] / nrm : 0.f;
        }
        *reinterpret_cast<f32x4*>(fo + o * 8) = lo;
        *reinterpret_cast<f32x4*>(fo + o * 8 + 4) = hi;
      }
    }
    if (lane == 0) {
      cls[(long long)b * max_obj + sl] = (int)labels[(long long)b * max_num + j];
      w[(long long)b * max_obj + sl] = dt[j * 5 + 4];
    }
  }
}

extern "C" int aod_object_descriptors(const void* const* seg_base, int nseg, const int32_t* seg_hw, const int32_t* seg_na, int C, int x3, int B,
                                      const int32_t* cand_anchor, int n, const float* dets, const int64_t* labels, const int32_t* num,
                                      const int32_t* obj_cand, int max_num, int max_obj, float score_thr, float* feat, int32_t* cls, float* w,
                                      int32_t* cnt, int32_t* missing, aod_stream_t stream) {
  AOD_CHECK_ARG(nseg >= 1 && nseg <= OD_MAX_SEG, "object_descriptors: 1..8 levels (got %d)", nseg);
  AOD_CHECK_ARG(seg_base && seg_hw && seg_na && cand_anchor && dets && labels && num && obj_cand && feat && cls && w && cnt && missing,
                "object_descriptors: null pointer");
  AOD_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= OD_MAX_C, "object_descriptors: channels must be a multiple of 8 in 8..%d (got %d)", OD_MAX_C, C);
  AOD_CHECK_ARG(B >= 1, "object_descriptors: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(n >= 1, "object_descriptors: at least one candidate row per image (got n = %d)", n);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= OD_MAX_DET, "object_descriptors: max_num must be in 1..%d (got %d)", OD_MAX_DET, max_num);
  AOD_CHECK_ARG(max_obj >= 1 && max_obj <= OD_MAX_OBJ, "object_descriptors: max_obj must be in 1..%d (got %d)", OD_MAX_OBJ, max_obj);
  AOD_CHECK_ARG(score_thr == score_thr, "object_descriptors: score_thr is NaN");
  AOD_CHECK_ARG((((size_t)feat) & 15) == 0, "object_descriptors: feat must be 16-B aligned");
  AOD_CHECK_ARG(((((size_t)cand_anchor) | ((size_t)dets) | ((size_t)num) | ((size_t)obj_cand) | ((size_t)cls) | ((size_t)w) | ((size_t)cnt) |
                  ((size_t)missing)) & 3) == 0 && (((size_t)labels) & 7) == 0,
                "object_descriptors: pointers must be aligned to their element size");
  OdSegs s;
  for (int l = 0; l < OD_MAX_SEG; ++l) { s.base[l] = nullptr; s.hw[l] = 1; s.na[l] = 1; s.a0[l] = 0; }
  s.a0[0] = 0;
  for (int l = 0; l < nseg; ++l) {
    AOD_CHECK_ARG(seg_base[l] && (((size_t)seg_base[l]) & 15) == 0, "object_descriptors: level %d: rows must be 16-B aligned", l);
    AOD_CHECK_ARG(seg_hw[l] >= 1 && seg_na[l] >= 1, "object_descriptors: level %d: %d cells per image, %d anchors per cell", l, (int)seg_hw[l],
                  (int)seg_na[l]);
    s.base[l] = (const bf16_t*)seg_base[l];
    s.hw[l] = seg_hw[l];
    s.na[l] = seg_na[l];
    s.a0[l + 1] = s.a0[l] + (long long)seg_hw[l] * seg_na[l];
  }
  for (int l = nseg; l < OD_MAX_SEG; ++l) s.a0[l + 1] = s.a0[l];
  s.nseg = nseg;
  hipLaunchKernelGGL(object_descriptors_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, s, C, x3 ? 1 : 0, cand_anchor, n, dets,
                     (const long long*)labels, num, obj_cand, max_num, max_obj, score_thr, feat, cls, w, cnt, missing);
  AOD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ distance
// LDS (floats / ints of 4 B): A [CC_ROWS][CP + CC_PAD] | clsA [CC_ROWS] | wA [CC_ROWS] | mA [4 waves][CC_ROWS] | mB [4][CC_ROWS] | wB [4][64]
// | cntA [4]
static inline size_t cc_lds_bytes(int CP) { return ((size_t)CC_ROWS * (CP + CC_PAD) + 2 * CC_ROWS + 8 * CC_ROWS + 4 * 64 + 4) * 4; }

template <int CP>
__global__ __launch_bounds__(256) void ccms_distance_kernel(const float* __restrict__ feat, const int* __restrict__ cls,
                                                            const float* __restrict__ w, const int* __restrict__ cnt, int M, int K, int C, int NB,
                                                            float* __restrict__ dist) {
  extern __shared__ __align__(16) float lds[];
  constexpr int ST = CP + CC_PAD;
  constexpr int S = CP / 8;
  float* A = lds;
  int* clsA = reinterpret_cast<int*>(A + CC_ROWS * ST);
  float* wA = reinterpret_cast<float*>(clsA + CC_ROWS);
  float* mAall = wA + CC_ROWS;
  float* mBall = mAall + 4 * CC_ROWS;
  float* wBall = mBall + 4 * CC_ROWS;
  int* cntA = reinterpret_cast<int*>(wBall + 4 * 64);
  const int NA = CC_BLOCKS / NB, KP = NB * 32;
  const int a0 = blockIdx.x * NA;
  const int b_begin = blockIdx.y * CC_BCHUNK;
  const int b_end = b_begin + CC_BCHUNK < M ? b_begin + CC_BCHUNK : M;
  if (b_end <= a0) return;                                         // (workgroup-uniform) the transposed pairs are another group's
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the a-group: rows >= cnt (and images >= M) are zeros of class -1
  for (int idx = tid; idx < CC_ROWS * (CP / 4); idx += 256) {
    const int r = idx / (CP / 4), c4 = (idx - r * (CP / 4)) * 4;
    const int ai = r / KP, i = r - ai * KP, a = a0 + ai;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (a < M && i < K && i < cnt[a] && c4 < C) v = *reinterpret_cast<const f32x4*>(feat + ((long long)a * K + i) * C + c4);
    *reinterpret_cast<f32x4*>(A + r * ST + c4) = v;
  }
  for (int r = tid; r < CC_ROWS; r += 256) {
    const int ai = r / KP, i = r - ai * KP, a = a0 + ai;
    const bool live = a < M && i < K && i < cnt[a];
    clsA[r] = live ? cls[(long long)a * K + i] : -1;
    wA[r] = live ? w[(long long)a * K + i] : 0.f;
  }
  if (tid < 4) {
    int c = 0;
    if (tid < NA && a0 + tid < M) { c = cnt[a0 + tid]; c = c < 0 ? 0 : (c > K ? K : c); }
    cntA[tid] = c;
  }
  __syncthreads();
  float* mA = mAall + wave * CC_ROWS;
  float* mB = mBall + wave * CC_ROWS;
  float* wB = wBall + wave * 64;
  const int j = lane & 31, h = lane >> 5;
  for (int b = b_begin + wave; b < b_end; b += 4) {
    if (b < a0) continue;
    int cb = cnt[b];
    cb = cb < 0 ? 0 : (cb > K ? K : cb);
    mA[lane] = 0.f;
    mA[lane + 64] = 0.f;
    mB[lane] = 0.f;
    mB[lane + 64] = 0.f;
    wB[lane] = lane < cb ? w[(long long)b * K + lane] : 0.f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int bb = 0; bb < NB; ++bb) {
      if (bb * 32 >= cb) break;                                    // (wave-uniform) no object in this block: every maximum stays 0
      const int jb = bb * 32 + j;
      const bool liveb = jb < cb;
      const int clsb = liveb ? cls[(long long)b * K + jb] : -2;
      const float* bp = feat + ((long long)b * K + jb) * C + 4 * h;
      f32x4 breg[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        breg[s] = (liveb && 8 * s + 4 * h < C) ? *reinterpret_cast<const f32x4*>(bp + 8 * s) : z;
      }
      for (int ai = 0; ai < NA; ++ai) {
        const int ca = cntA[ai];
        float colmax = 0.f;
        for (int ab = 0; ab < NB; ++ab) {
          if (ab * 32 >= ca) break;                                // (wave-uniform)
          const int r0 = (ai * NB + ab) * 32;
          const float* ap = A + (r0 + j) * ST + 4 * h;
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(ap + 8 * s);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], breg[s][u], acc, 0, 0, 0);
          }
          // accumulator r of this lane: a-row 8 (r >> 2) + 4 h + (r & 3), b-row j
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const i32x4 ca4 = *reinterpret_cast<const i32x4*>(clsA + r0 + 8 * g + 4 * h);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              float v = ca4[q] == clsb ? fmaxf(acc[4 * g + q], 0.f) : 0.f;
              colmax = fmaxf(colmax, v);
#pragma unroll
              for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
              if (j == 0) {
                const int i = r0 + 8 * g + 4 * h + q;
                mA[i] = fmaxf(mA[i], v);
              }
            }
          }
        }
        colmax = fmaxf(colmax, __shfl_xor(colmax, 32, 64));
        if (h == 0) mB[ai * KP + jb] = colmax;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < NA && a0 + lane < M) {
      const int a = a0 + lane, ca = cntA[lane];
      float numA = 0.f, denA = 0.f, numB = 0.f, denB = 0.f;
      for (int i = 0; i < ca; ++i) {
        const float wi = wA[lane * KP + i];
        numA += wi * mA[lane * KP + i];
        denA += wi;
      }
      for (int i = 0; i < cb; ++i) {
        const float wi = wB[i];
        numB += wi * mB[lane * KP + i];
        denB += wi;
      }
      const float sab = (ca > 0 && denA > 0.f) ? numA / denA : 0.f;
      const float sba = (cb > 0 && denB > 0.f) ? numB / denB : 0.f;
      const float d = a == b ? 0.f : fmaxf(0.f, 1.0f - (sab + sba) * 0.5f);
      dist[(long long)a * M + b] = d;
      if (b >= a0 + NA) dist[(long long)b * M + a] = d;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

template <int CP>
static int cc_launch(const float* feat, const int32_t* cls, const float* w, const int32_t* cnt, int M, int K, int C, float* dist, hipStream_t st) {
  const int NB = (K + 31) / 32, NA = CC_BLOCKS / NB;
  const size_t ldsb = cc_lds_bytes(CP);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ccms_distance_kernel<CP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb);
    attr = true;
  }
  const dim3 grid((unsigned)((M + NA - 1) / NA), (unsigned)((M + CC_BCHUNK - 1) / CC_BCHUNK));
  hipLaunchKernelGGL(ccms_distance_kernel<CP>, grid, dim3(256), ldsb, st, feat, cls, w, cnt, M, K, C, NB, dist);
  return 0;
}

extern "C" int aod_ccms_max_images(void) { return CC_MAX_M; }

extern "C" int aod_ccms_distance(const float* feat, const int32_t* cls, const float* w, const int32_t* cnt, int M, int max_obj, int C, float* dist,
                                 aod_stream_t stream) {
  AOD_CHECK_ARG(M >= 1 && M <= CC_MAX_M, "ccms_distance: 1..%d images (got %d)", CC_MAX_M, M);
  AOD_CHECK_ARG(max_obj >= 1 && max_obj <= OD_MAX_OBJ, "ccms_distance: max_obj must be in 1..%d (got %d): an image is one or two blocks of 32 objects",
                OD_MAX_OBJ, max_obj);
  AOD_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= CC_MAX_C,
                "ccms_distance: channels must be a multiple of 8 in 8..%d (got %d): four blocks of 32 objects x C fp32 stay resident in LDS", CC_MAX_C, C);
  AOD_CHECK_ARG(feat && cls && w && cnt && dist, "ccms_distance: null pointer");
  AOD_CHECK_ARG((((size_t)feat) & 15) == 0 && ((((size_t)cls) | ((size_t)w) | ((size_t)cnt) | ((size_t)dist)) & 3) == 0,
                "ccms_distance: feat must be 16-B aligned, the other pointers 4-B aligned");
  hipStream_t st = (hipStream_t)stream;
  if (C <= 64) cc_launch<64>(feat, cls, w, cnt, M, max_obj, C, dist, st);
  else if (C <= 128) cc_launch<128>(feat, cls, w, cnt, M, max_obj, C, dist, st);
  else cc_launch<256>(feat, cls, w, cnt, M, max_obj, C, dist, st);
  AOD_LAUNCH_CHECK();
  return 0;
}
