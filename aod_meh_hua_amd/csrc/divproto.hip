// ENMS + DivProto acquisition: J. Wu, J. Chen, D. Huang, "Entropy-based Active Learning for Object Detection with Progressive
// Diversity Constraint", CVPR 2022.  The reference tree has no such pool: the semantics are fixed in DESIGN 3s.
//
// <a, b> everywhere below is dp_dot16: 16 lanes per product, lane q owns the channels 4q + 64m (+0..3), m ascending; four running sums per
// lane (separate multiply and add), ((s0 + s1) + (s2 + s3)), then an xor butterfly over the 16 lanes.  Products and two-term sums commute,
// so the value is bit-symmetric in its arguments and a function of the two rows and C alone.
//
// 1. object_measure_kernel: h [B][max_obj] = the per-object posterior measure (aod_det_uncertainty*'s obj_out) compacted into the slots of
//    aod_object_descriptors: the gate (j < num[b], score > score_thr, strict), an object without a candidate row takes no slot, the first
//    max_obj in row order.  Padding 0.
// 2. enms_prototypes_kernel: one workgroup of 256 threads per image.
//      a. the image's <= 64 rows go to LDS (row pitch C + 4 floats against bank conflicts, as ccms.hip pads).
//      b. the same-class products <f_i, f_j>, i < j, into a [K][K + 1] LDS tile (both triangles from the one value); no other entry is
//         ever read.
//      c. wave 0, lane l = object l: the greedy.  key = (order-preserving bits of h << 32) | ~l, a 64-bit wave maximum: the largest h wins,
//         the lowest index on a tie.  E += h in pick order, every lane the same chain.  t_enms >= 1 suppresses nothing (a cosine cannot
//         exceed 1, the rounded product of a row with itself can); t_intra >= 1 likewise makes no image redundant.
//      d. wave 0: the distinct classes in ascending order (rank = number of smaller distinct classes), conf = max w of the class.
//      e. a wave per prototype: lane owns the channels 4 lane (+0..3); v += (h_k + 2^-10) * f_k over the class's objects in ascending k;
//         sum of squares ((v0^2 + v1^2) + (v2^2 + v3^2)) per lane, xor butterfly; p = v / sqrt(sum), zeros when the sum is 0.
//    A function of the image's rows alone: the same bits alone, in any batch, eager or replayed.
// 3. the selection: divproto_init_kernel, then ceil(M / chunk) launches of divproto_sweep_kernel -- ONE workgroup each; the state (counters,
//    presence counts n_c, per-class lists of accepted (image, slot) pairs, a flag per sweep position) lives in the workspace, so the
//    result does not depend on how the sweep is cut into launches -- and one divproto_fill_kernel over the flags.  A sweep launch that
//    finds the budget met exits at once.  Per candidate: its prototypes go to LDS; the 16 lane groups of the four waves split the entries
//    of each of its classes' lists; wave 0 (lane = slot) takes the minimum of the class maxima and runs the inter-class check; lane 0
//    records the decision and appends.  No atomics, no cross-workgroup wait, no host sync.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define DP_MAX_OBJ 64
#define DP_MAX_C 256
#define DP_PAD 4
#define DP_MAX_DET 1024
#define DP_MAX_CLS 128
#define DP_CHUNK 64           // sweep positions per launch (aod_divproto_chunk): ~2 ms at the measured time per candidate
#define DP_MAX_CHUNK 65536
#define DP_HDR 272            // workspace header, int32 words: n_acc, free_used, 2 spare, n_c [128], len [128], 12 spare
#define DP_ACCEPTED 1
#define DP_DEFERRED 2
#define DP_REDUNDANT 3

typedef unsigned long long u64;

__device__ __forceinline__ float dp_dot16(const float* a, const float* b, int C, int q) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int k = 4 * q; k < C; k += 64) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(a + k);
    const f32x4 y = *reinterpret_cast<const f32x4*>(b + k);
    s0 += x[0] * y[0];
    s1 += x[1] * y[1];
    s2 += x[2] * y[2];
    s3 += x[3] * y[3];
  }
  float t = (s0 + s1) + (s2 + s3);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

__device__ __forceinline__ u64 dp_wave_max(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(k, o, 64);
    k = other > k ? other : k;
  }
  return k;
}

__device__ __forceinline__ float dp_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// float bits -> unsigned, order-preserving over every non-NaN value (a non-negative h keeps its own bits' order)
__device__ __forceinline__ unsigned dp_mono(float h) {
  const unsigned u = __float_as_uint(h);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ------------------------------------------------------------------------------------------------------------------ per-object measure
__global__ __launch_bounds__(256) void object_measure_kernel(const float* __restrict__ obj_out, const float* __restrict__ dets,
                                                             const int* __restrict__ num, const int* __restrict__ obj_cand, int max_num,
                                                             int max_obj, float thr, float* __restrict__ h) {
  __shared__ unsigned char is_obj[DP_MAX_DET];
  __shared__ int slot_det[DP_MAX_OBJ];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  for (int j = tid; j < max_num; j += 256)
    is_obj[j] = j < nd && dets[((long long)b * max_num + j) * 5 + 4] > thr && (!obj_cand || obj_cand[(long long)b * max_num + j] >= 0);
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int j = 0; j < max_num && c < max_obj; ++j)
      if (is_obj[j]) slot_det[c++] = j;
    s_cnt = c;
  }
  __syncthreads();
  if (tid < max_obj) h[(long long)b * max_obj + tid] = tid < s_cnt ? obj_out[(long long)b * max_num + slot_det[tid]] : 0.f;
}

extern "C" int aod_object_measure(const float* obj_out, const float* dets, const int32_t* num, const int32_t* obj_cand, int B, int max_num,
                                  int max_obj, float score_thr, float* h, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1, "object_measure: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= DP_MAX_DET, "object_measure: max_num must be in 1..%d (got %d)", DP_MAX_DET, max_num);
  AOD_CHECK_ARG(max_obj >= 1 && max_obj <= DP_MAX_OBJ, "object_measure: max_obj must be in 1..%d (got %d)", DP_MAX_OBJ, max_obj);
  AOD_CHECK_ARG(score_thr == score_thr, "object_measure: score_thr is NaN");
  AOD_CHECK_ARG(obj_out && dets && num && h, "object_measure: null pointer");
  AOD_CHECK_ARG(((((size_t)obj_out) | ((size_t)dets) | ((size_t)num) | ((size_t)obj_cand) | ((size_t)h)) & 3) == 0,
                "object_measure: pointers must be 4-B aligned");
  hipLaunchKernelGGL(object_measure_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, obj_out, dets, num, obj_cand, max_num, max_obj,
                     score_thr, h);
  AOD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ ENMS + prototypes
// dynamic LDS (floats): F [K][C + DP_PAD] | sim [K][K + 1]
static inline size_t dp_enms_lds(int K, int C) { return ((size_t)K * (C + DP_PAD) + (size_t)K * (K + 1)) * sizeof(float); }

__global__ __launch_bounds__(256) void enms_prototypes_kernel(const float* __restrict__ feat, const int* __restrict__ cls,
                                                              const float* __restrict__ w, const float* __restrict__ h,
                                                              const int* __restrict__ cnt, int K, int C, float t_enms, float* __restrict__ enms,
                                                              int* __restrict__ kept, float* __restrict__ proto, int* __restrict__ pcls,
                                                              float* __restrict__ pconf, int* __restrict__ pcnt, int* __restrict__ pick) {
  extern __shared__ __align__(16) float lds[];
  __shared__ int s_cls[DP_MAX_OBJ], s_slot[DP_MAX_OBJ];
  __shared__ float s_h[DP_MAX_OBJ], s_w[DP_MAX_OBJ];
  __shared__ int s_pc;
  const int ST = C + DP_PAD, SS = K + 1, C4 = C >> 2;
  float* F = lds;
  float* sim = F + K * ST;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = cnt[b];
  n = n < 0 ? 0 : (n > K ? K : n);
  const float* fb = feat + (long long)b * K * C;
  for (int idx = tid; idx < n * C4; idx += 256) {
    const int r = idx / C4, c4 = (idx - r * C4) * 4;
    *reinterpret_cast<f32x4*>(F + r * ST + c4) = *reinterpret_cast<const f32x4*>(fb + (long long)r * C + c4);
  }
  if (tid < DP_MAX_OBJ) {
    const bool live = tid < n;
    s_cls[tid] = live ? cls[(long long)b * K + tid] : -1;
    s_h[tid] = live ? h[(long long)b * K + tid] : 0.f;
    s_w[tid] = live ? w[(long long)b * K + tid] : 0.f;
  }
  __syncthreads();
  // b. same-class products, 16 lanes each
  const int g = tid >> 4, q = tid & 15;
  for (int p0 = 0; p0 < n * n; p0 += 16) {
    const int p = p0 + g;
    const int i = p / n, j = p - i * n;
    const bool need = p < n * n && i < j && s_cls[i] == s_cls[j];
    if (__any(need)) {                                             // (wave-uniform: the butterfly runs with every lane)
      const float v = dp_dot16(F + (need ? i : 0) * ST, F + (need ? j : 0) * ST, C, q);
      if (need && q == 0) {
        sim[i * SS + j] = v;
        sim[j * SS + i] = v;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    // c. the greedy
    const int c = s_cls[lane];
    const bool nms_on = t_enms < 1.f;                              // (a cosine cannot exceed 1; the fp32 product of a row with itself can)
    bool alive = lane < n;
    float E = 0.f;
    int kp = 0;
    for (;;) {
      u64 key = alive ? (((u64)dp_mono(s_h[lane]) << 32) | (u64)(~(unsigned)lane)) : 0ull;
      key = dp_wave_max(key);
      if (key == 0ull) break;                                      // (wave-uniform)
      const int ks = (int)(~(unsigned)(key & 0xffffffffull));
      E += s_h[ks];
      if (pick && lane == 0) pick[(long long)b * K + kp] = ks;
      ++kp;
      if (lane == ks) alive = false;
      else if (alive && nms_on && c == s_cls[ks] && sim[ks * SS + lane] > t_enms) alive = false;
    }
    if (pick && lane >= kp && lane < K) pick[(long long)b * K + lane] = -1;
    if (lane == 0) {
      enms[b] = E;
      kept[b] = kp;
    }
    // d. the classes present, ascending
    bool first = lane < n;
    for (int j = 0; j < n; ++j)
      if (j < lane && s_cls[j] == c) first = false;
    const u64 fmask = __ballot(first);
    int rank = 0;
    float conf = 0.f;
    for (int j = 0; j < n; ++j) {
      if (((fmask >> j) & 1ull) && s_cls[j] < c) ++rank;
      if (s_cls[j] == c) conf = fmaxf(conf, s_w[j]);
    }
    const int pc = __popcll(fmask);
    s_slot[lane] = lane < n ? rank : -1;
    if (first) {
      pcls[(long long)b * K + rank] = c;
      pconf[(long long)b * K + rank] = conf;
    }
    if (lane >= pc && lane < K) {
      pcls[(long long)b * K + lane] = -1;
      pconf[(long long)b * K + lane] = 0.f;
    }
    if (lane == 0) {
      pcnt[b] = pc;
      s_pc = pc;
    }
  }
  __syncthreads();
  // e. a wave per prototype
  const int pc = s_pc;
  const bool own = 4 * lane < C;
  for (int r = wave; r < K; r += 4) {
    float* po = proto + ((long long)b * K + r) * C;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < pc) {                                                  // (wave-uniform)
      for (int k = 0; k < n; ++k) {
        if (s_slot[k] != r) continue;
        const float wk = s_h[k] + 0.0009765625f;
        if (own) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(F + k * ST + 4 * lane);
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] += wk * x[u];
        }
      }
    }
    const float ss = wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
    const float nrm = sqrtf(ss);
    if (own) {
      f32x4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = ss > 0.f ? v[u] / nrm : 0.f;
      *reinterpret_cast<f32x4*>(po + 4 * lane) = o;
    }
  }
}

extern "C" int aod_enms_prototypes(const float* feat, const int32_t* cls, const float* w, const float* h, const int32_t* cnt, int B, int max_obj,
                                   int C, float t_enms, float* enms, int32_t* kept, float* proto, int32_t* pcls, float* pconf, int32_t* pcnt,
                                   int32_t* pick, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1, "enms_prototypes: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(max_obj >= 1 && max_obj <= DP_MAX_OBJ, "enms_prototypes: max_obj must be in 1..%d (got %d)", DP_MAX_OBJ, max_obj);
  AOD_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= DP_MAX_C,
                "enms_prototypes: channels must be a multiple of 8 in 8..%d (got %d): an image's 64 rows stay resident in LDS", DP_MAX_C, C);
  AOD_CHECK_ARG(t_enms == t_enms, "enms_prototypes: t_enms is NaN");
  AOD_CHECK_ARG(feat && cls && w && h && cnt && enms && kept && proto && pcls && pconf && pcnt, "enms_prototypes: null pointer");
  AOD_CHECK_ARG(((((size_t)feat) | ((size_t)proto)) & 15) == 0, "enms_prototypes: feat and proto must be 16-B aligned");
  AOD_CHECK_ARG(((((size_t)cls) | ((size_t)w) | ((size_t)h) | ((size_t)cnt) | ((size_t)enms) | ((size_t)kept) | ((size_t)pcls) | ((size_t)pconf) |
                  ((size_t)pcnt) | ((size_t)pick)) & 3) == 0,
                "enms_prototypes: pointers must be 4-B aligned");
  const size_t ldsb = dp_enms_lds(max_obj, C);
  static unsigned long long attr_done = 0;
  if (aod_first_on_device(&attr_done)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&enms_prototypes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dp_enms_lds(DP_MAX_OBJ, DP_MAX_C));
  }
  hipLaunchKernelGGL(enms_prototypes_kernel, dim3((unsigned)B), dim3(256), ldsb, (hipStream_t)stream, feat, cls, w, h, cnt, max_obj, C, t_enms,
                     enms, kept, proto, pcls, pconf, pcnt, pick);
  AOD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ selection
struct DpSel {
  const long long* order;      // [M] pool indices in sweep order
  const float* proto;          // [N][K][C]
  const int* pcls;             // [N][K]
  const float* pconf;          // [N][K]
  const int* pcnt;             // [N]
  int* hdr;                    // [DP_HDR]
  long long* lists;            // [n_cls][budget]: (image << 8) | slot
  unsigned char* flags;        // [M]
  long long* picks;            // [budget]
  int* stage;                  // [budget]
  long long N;
  int M, K, C, n_cls, budget;
  float t_intra, t_inter;
  int n_minor, quota, nfree, balance;
};

__global__ __launch_bounds__(256) void divproto_init_kernel(DpSel a) {
  const long long i0 = blockIdx.x * 256ll + threadIdx.x, step = 256ll * gridDim.x;
  for (long long i = i0; i < DP_HDR; i += step) a.hdr[i] = 0;
  for (long long i = i0; i < a.M; i += step) a.flags[i] = 0;
  for (long long i = i0; i < a.budget; i += step) {
    a.picks[i] = -1ll;
    a.stage[i] = 0;
  }
}

__global__ __launch_bounds__(256) void divproto_sweep_kernel(DpSel a, int pos0, int pos1) {
  extern __shared__ __align__(16) float P[];                       // [K][C + DP_PAD]: the candidate's prototypes
  __shared__ int s_nc[DP_MAX_CLS], s_len[DP_MAX_CLS];
  __shared__ int s_cls[DP_MAX_OBJ];
  __shared__ float s_conf[DP_MAX_OBJ];
  __shared__ float gmax[16 * DP_MAX_OBJ];
  __shared__ int s_nacc, s_free;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, q = tid & 15;
  const int K = a.K, C = a.C, ST = C + DP_PAD, C4 = C >> 2;
  if (a.hdr[0] >= a.budget) return;                                // (workgroup-uniform) the budget is met: nothing to do
  if (tid < DP_MAX_CLS) {
    s_nc[tid] = a.hdr[4 + tid];
    s_len[tid] = a.hdr[4 + DP_MAX_CLS + tid];
  }
  if (tid == 0) {
    s_nacc = a.hdr[0];
    s_free = a.hdr[1];
  }
  __syncthreads();
  const float ninf = __uint_as_float(0xff800000u), pinf = __uint_as_float(0x7f800000u);
  for (int pos = pos0; pos < pos1; ++pos) {
    if (s_nacc >= a.budget) break;                                 // (workgroup-uniform: read behind a barrier)
    const long long img = a.order[pos];
    const bool in = img >= 0 && img < a.N;                         // (the caller validates; an index outside the pool is never dereferenced)
    int n = in ? a.pcnt[img] : 0;
    n = n < 0 ? 0 : (n > K ? K : n);
    const float* pb = a.proto + (in ? img : 0) * (long long)K * C;
    for (int idx = tid; idx < n * C4; idx += 256) {
      const int r = idx / C4, c4 = (idx - r * C4) * 4;
      *reinterpret_cast<f32x4*>(P + r * ST + c4) = *reinterpret_cast<const f32x4*>(pb + (long long)r * C + c4);
    }
    if (tid < DP_MAX_OBJ) {
      int c = tid < n ? a.pcls[img * K + tid] : -1;
      if (c < 0 || c >= a.n_cls) c = -1;                           // (a class outside [0, n_cls) names no list: the slot is ignored)
      s_cls[tid] = c;
      s_conf[tid] = tid < n ? a.pconf[img * K + tid] : 0.f;
    }
    for (int i = tid; i < 16 * DP_MAX_OBJ; i += 256) gmax[i] = ninf;
    __syncthreads();
    // 1. per class of the candidate: the largest product with an entry of the class's list; the 16 lane groups split the entries
    for (int s = 0; s < n; ++s) {
      const int c = s_cls[s];
      if (c < 0) continue;                                         // (workgroup-uniform)
      const int L = s_len[c];
      const float* prow = P + s * ST;
      float mx = ninf;
      for (int e0 = 0; e0 < L; e0 += 16) {
        const int e = e0 + g;
        const bool ok = e < L;
        const long long ent = ok ? a.lists[(long long)c * a.budget + e] : 0ll;
        const float* row = ok ? a.proto + ((ent >> 8) * K + (ent & 255)) * C : prow;
        const float v = dp_dot16(prow, row, C, q);
        if (ok) mx = fmaxf(mx, v);
      }
      if (q == 0) gmax[g * DP_MAX_OBJ + s] = mx;
    }
    __syncthreads();
    // 2. wave 0, lane = slot: the two checks; lane 0 records the decision
    if (wave == 0) {
      const int c = s_cls[lane];
      const bool has = lane < n && c >= 0;
      float m = pinf;
      if (has) {
        if (s_len[c] == 0) {
          m = 0.f;
        } else {
          m = ninf;
#pragma unroll
          for (int gg = 0; gg < 16; ++gg) m = fmaxf(m, gmax[gg * DP_MAX_OBJ + lane]);
        }
      }
      const bool anycls = __ballot(has) != 0ull;
      const float mmin = dp_wave_min(m);
      const bool redundant = anycls && a.t_intra < 1.f && mmin > a.t_intra;      // (t >= 1 switches the check off, as in the ENMS)
      int code = DP_REDUNDANT, st = 0;
      if (!redundant) {
        bool serves = false;
        if (a.balance) {
          bool sv = false;
          if (has) {
            const int nc = s_nc[c];
            int rank = 0;
            for (int cc = 0; cc < a.n_cls; ++cc) {
              const int o = s_nc[cc];
              rank += (o < nc || (o == nc && cc < c)) ? 1 : 0;
            }
            sv = rank < a.n_minor && s_conf[lane] > a.t_inter && nc < a.quota;
          }
          serves = __ballot(sv) != 0ull;
        }
        if (!a.balance || serves) {
          code = DP_ACCEPTED;
          st = 1;
        } else if (s_free < a.nfree) {
          code = DP_ACCEPTED;
          st = 2;
        } else {
          code = DP_DEFERRED;
        }
      }
      if (lane == 0) {
        a.flags[pos] = (unsigned char)code;
        if (code == DP_ACCEPTED) {
          const int t = s_nacc;
          a.picks[t] = img;
          a.stage[t] = st;
          if (st == 2) s_free = s_free + 1;
          for (int s = 0; s < n; ++s) {
            const int cs = s_cls[s];
            if (cs < 0) continue;
            const int L = s_len[cs];
            if (L < a.budget) {                                    // (one entry per class and accepted image: never full for distinct classes)
              a.lists[(long long)cs * a.budget + L] = (img << 8) | (long long)s;
              s_len[cs] = L + 1;
            }
            if (s_conf[s] > a.t_inter) s_nc[cs] = s_nc[cs] + 1;
          }
          s_nacc = t + 1;
        }
      }
    }
    __syncthreads();                                               // (the appended entries are visible to the workgroup's next candidate)
  }
  if (tid < DP_MAX_CLS) {
    a.hdr[4 + tid] = s_nc[tid];
    a.hdr[4 + DP_MAX_CLS + tid] = s_len[tid];
  }
  if (tid == 0) {
    a.hdr[0] = s_nacc;
    a.hdr[1] = s_free;
  }
}

// stage 3: the deferred positions in sweep order, then the redundant ones, until the budget is met
__global__ __launch_bounds__(256) void divproto_fill_kernel(DpSel a) {
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nacc = a.hdr[0];
  if (nacc >= a.budget) return;                                    // (workgroup-uniform)
  for (int tier = DP_DEFERRED; tier <= DP_REDUNDANT; ++tier) {
    for (long long base = 0; base < a.M && nacc < a.budget; base += 256) {
      const long long pos = base + tid;
      const bool f = pos < a.M && a.flags[pos] == tier;
      const u64 mask = __ballot(f);
      const int pre = __popcll(mask & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[wave] = __popcll(mask);
      __syncthreads();
      int off = 0, tot = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        off += v < wave ? wcnt[v] : 0;
        tot += wcnt[v];
      }
      const long long idx = (long long)nacc + off + pre;
      if (f && idx < a.budget) {
        a.picks[idx] = a.order[pos];
        a.stage[idx] = 3;
      }
      nacc = nacc + tot > a.budget ? a.budget : nacc + tot;
      __syncthreads();
    }
  }
  if (tid == 0) a.hdr[0] = nacc;
}

extern "C" int aod_divproto_chunk(void) { return DP_CHUNK; }

// workspace bytes: the header, the per-class lists (8 B per entry, budget entries per class), one flag byte per sweep position
extern "C" size_t aod_divproto_ws_len(int64_t M, int n_cls, int64_t budget) {
  if (M < 1 || M > 0x7fffffffll || n_cls < 1 || n_cls > DP_MAX_CLS || budget < 1 || budget > M) return 0;
  return (size_t)DP_HDR * sizeof(int) + (size_t)n_cls * (size_t)budget * sizeof(long long) + (((size_t)M + 15) & ~(size_t)15);
}

extern "C" int aod_divproto_select(const int64_t* order, int64_t M, int64_t N, const float* proto, const int32_t* pcls, const float* pconf,
                                   const int32_t* pcnt, int max_obj, int C, int n_cls, int64_t budget, float t_intra, float t_inter, int n_minor,
                                   int64_t quota, int64_t n_free, int class_balance, int chunk, int64_t* picks, int32_t* stage, void* ws,
                                   aod_stream_t stream) {
  AOD_CHECK_ARG(M >= 1 && M <= 0x7fffffffll, "divproto_select: 1 .. 2^31 - 1 candidates (got %lld)", (long long)M);
  AOD_CHECK_ARG(N >= M && N <= 0x7fffffffll, "divproto_select: the pool holds %lld images, the sweep %lld", (long long)N, (long long)M);
  AOD_CHECK_ARG(max_obj >= 1 && max_obj <= DP_MAX_OBJ, "divproto_select: max_obj must be in 1..%d (got %d)", DP_MAX_OBJ, max_obj);
  AOD_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= DP_MAX_C, "divproto_select: channels must be a multiple of 8 in 8..%d (got %d)", DP_MAX_C, C);
  AOD_CHECK_ARG(n_cls >= 1 && n_cls <= DP_MAX_CLS, "divproto_select: n_cls must be in 1..%d (got %d)", DP_MAX_CLS, n_cls);
  AOD_CHECK_ARG(budget >= 1 && budget <= M, "divproto_select: budget %lld outside 1 .. %lld candidates", (long long)budget, (long long)M);
  AOD_CHECK_ARG(t_intra == t_intra && t_inter == t_inter, "divproto_select: a threshold is NaN");
  AOD_CHECK_ARG(n_minor >= 1 && n_minor <= n_cls, "divproto_select: n_minor %d outside 1 .. n_cls = %d", n_minor, n_cls);
  AOD_CHECK_ARG(n_free >= 0 && n_free <= budget, "divproto_select: free slots %lld outside 0 .. budget = %lld", (long long)n_free, (long long)budget);
  AOD_CHECK_ARG(quota >= 1 && quota <= budget, "divproto_select: quota %lld outside 1 .. budget = %lld", (long long)quota, (long long)budget);
  AOD_CHECK_ARG(chunk >= 0 && chunk <= DP_MAX_CHUNK, "divproto_select: chunk %d outside 0 (default) .. %d", chunk, DP_MAX_CHUNK);
  AOD_CHECK_ARG(order && proto && pcls && pconf && pcnt && picks && stage && ws, "divproto_select: null pointer");
  AOD_CHECK_ARG((((size_t)proto) & 15) == 0 && ((((size_t)order) | ((size_t)picks) | ((size_t)ws)) & 7) == 0 &&
                    ((((size_t)pcls) | ((size_t)pconf) | ((size_t)pcnt) | ((size_t)stage)) & 3) == 0,
                "divproto_select: proto must be 16-B aligned, order / picks / ws 8-B aligned, the other pointers 4-B aligned");
  hipStream_t st = (hipStream_t)stream;
  DpSel a;
  a.order = (const long long*)order;
  a.proto = proto;
  a.pcls = pcls;
  a.pconf = pconf;
  a.pcnt = pcnt;
  a.hdr = (int*)ws;
  a.lists = (long long*)((char*)ws + (size_t)DP_HDR * sizeof(int));
  a.flags = (unsigned char*)ws + (size_t)DP_HDR * sizeof(int) + (size_t)n_cls * (size_t)budget * sizeof(long long);
  a.picks = (long long*)picks;
  a.stage = stage;
  a.N = N;
  a.M = (int)M;
  a.K = max_obj;
  a.C = C;
  a.n_cls = n_cls;
  a.budget = (int)budget;
  a.t_intra = t_intra;
  a.t_inter = t_inter;
  a.n_minor = n_minor;
  a.quota = (int)quota;
  a.nfree = (int)n_free;
  a.balance = class_balance ? 1 : 0;
  const size_t ldsb = (size_t)max_obj * (C + DP_PAD) * sizeof(float);
  static unsigned long long attr_done = 0;
  if (aod_first_on_device(&attr_done)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&divproto_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((size_t)DP_MAX_OBJ * (DP_MAX_C + DP_PAD) * sizeof(float)));
  }
  long long ig = (M + 255) / 256;
  ig = ig > 1024 ? 1024 : ig;
  hipLaunchKernelGGL(divproto_init_kernel, dim3((unsigned)ig), dim3(256), 0, st, a);
  const int ch = chunk > 0 ? chunk : DP_CHUNK;
  for (int64_t p0 = 0; p0 < M; p0 += ch) {
    const int64_t p1 = p0 + ch < M ? p0 + ch : M;
    hipLaunchKernelGGL(divproto_sweep_kernel, dim3(1), dim3(256), ldsb, st, a, (int)p0, (int)p1);
  }
  hipLaunchKernelGGL(divproto_fill_kernel, dim3(1), dim3(256), 0, st, a);
  AOD_LAUNCH_CHECK();
  return 0;
}
