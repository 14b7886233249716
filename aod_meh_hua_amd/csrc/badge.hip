// BADGE acquisition: J. T. Ash, C. Zhang, A. Krishnamurthy, J. Langford, A. Agarwal, "Deep Batch Active Learning by Diverse,
// Uncertain Gradient Lower Bounds", ICLR 2020 -- the gradient embedding of an image; the k-means++ seeding on the embeddings is
// kmeanspp.hip.  The reference tree has no such pool: the semantics are fixed in DESIGN 3t.
//
// 1. object_posterior_kernel: post [B][max_obj][W] = the candidate score row of every object in the slots of aod_object_descriptors, by
//    aod_object_measure's slot rule: the detection rows j < num[b] with score > score_thr (strict) that have a candidate row
//    (0 <= obj_cand[b][j] < n), the first max_obj in row order.  Rows >= cnt[b] are zero: every word is written.
// 2. badge_embedding_kernel: one workgroup of 256 threads per image.  a_o[c] = post[b][o][c] - [c == cls[b][o]] for c < n_cls (the gradient
//    of the cross-entropy with respect to the logits under the detection's own label) goes to LDS; then G[c][j] = sum_o a_o[c] * f_o[j]:
//    a work item is 4 classes x 4 features, 16 accumulators; the objects o < cnt[b] in ascending order, a separate multiply and add per
//    object, fp32, no atomics.  Columns c >= n_cls of post and rows o >= cnt[b] are never read.  A function of the image's rows alone: the
//    same bits alone, at any place of any batch, eager or replayed.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define BG_MAX_OBJ 64
#define BG_MAX_DET 1024
#define BG_MAX_C 256
#define BG_MAX_CLS 128
#define BG_CT 4               // classes per work item

__global__ __launch_bounds__(256) void object_posterior_kernel(const float* __restrict__ scores, const float* __restrict__ dets,
                                                               const int* __restrict__ num, const int* __restrict__ obj_cand, int n, int W,
                                                               int max_num, int max_obj, float thr, float* __restrict__ post) {
  __shared__ unsigned char is_obj[BG_MAX_DET];
  __shared__ int slot_row[BG_MAX_OBJ];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  for (int j = tid; j < max_num; j += 256) {
    const int k = obj_cand[(long long)b * max_num + j];
    is_obj[j] = j < nd && dets[((long long)b * max_num + j) * 5 + 4] > thr && k >= 0 && k < n;
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int j = 0; j < max_num && c < max_obj; ++j)
      if (is_obj[j]) slot_row[c++] = obj_cand[(long long)b * max_num + j];
    s_cnt = c;
  }
  __syncthreads();
  const int cnt = s_cnt;
  float* po = post + (long long)b * max_obj * W;
  for (int idx = tid; idx < max_obj * W; idx += 256) {
    const int sl = idx / W, c = idx - sl * W;
    po[idx] = sl < cnt ? scores[((long long)b * n + slot_row[sl]) * W + c] : 0.f;
  }
}

extern "C" int aod_object_posterior(const float* scores, const float* dets, const int32_t* num, const int32_t* obj_cand, int B, int n, int W,
                                    int max_num, int max_obj, float score_thr, float* post, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1, "object_posterior: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(n >= 1 && n <= (1 << 30), "object_posterior: candidate rows per image must be in 1..2^30 (got n = %d)", n);
  AOD_CHECK_ARG(W >= 1 && W <= 65536, "object_posterior: score rows of 1..65536 columns (got W = %d)", W);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= BG_MAX_DET, "object_posterior: max_num must be in 1..%d (got %d)", BG_MAX_DET, max_num);
  AOD_CHECK_ARG(max_obj >= 1 && max_obj <= BG_MAX_OBJ, "object_posterior: max_obj must be in 1..%d (got %d)", BG_MAX_OBJ, max_obj);
  AOD_CHECK_ARG(score_thr == score_thr, "object_posterior: score_thr is NaN");
  AOD_CHECK_ARG(scores && dets && num && obj_cand && post, "object_posterior: null pointer");
  AOD_CHECK_ARG(((((size_t)scores) | ((size_t)dets) | ((size_t)num) | ((size_t)obj_cand) | ((size_t)post)) & 3) == 0,
                "object_posterior: pointers must be 4-B aligned");
  hipLaunchKernelGGL(object_posterior_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, scores, dets, num, obj_cand, n, W, max_num,
                     max_obj, score_thr, post);
  AOD_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void badge_embedding_kernel(const float* __restrict__ feat, const float* __restrict__ post,
                                                              const int* __restrict__ cls, const int* __restrict__ cnt, int K, int Cf, int W,
                                                              int n_cls, float* __restrict__ out, long long out_stride) {
  extern __shared__ __align__(16) float a[];                       // [K][NP], NP = n_cls rounded up to BG_CT (the pad columns are zero)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int NP = (n_cls + BG_CT - 1) / BG_CT * BG_CT;
  int c = cnt[b];
  c = c < 0 ? 0 : (c > K ? K : c);
  for (int idx = tid; idx < c * NP; idx += 256) {
    const int o = idx / NP, k = idx - o * NP;
    float v = 0.f;
    if (k < n_cls) {
      v = post[((long long)b * K + o) * W + k];
      if (k == cls[(long long)b * K + o]) v -= 1.0f;
    }
    a[idx] = v;
  }
  __syncthreads();
  const int nq = Cf >> 2, nct = NP / BG_CT;
  const float* fb = feat + (long long)b * K * Cf;
  float* ob = out + (long long)b * out_stride;
  for (int item = tid; item < nq * nct; item += 256) {
    const int ct = item / nq, q = item - ct * nq;
    f32x4 acc[BG_CT];
#pragma unroll
    for (int u = 0; u < BG_CT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int o = 0; o < c; ++o) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(fb + (long long)o * Cf + 4 * q);
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + o * NP + BG_CT * ct);
#pragma unroll
      for (int u = 0; u < BG_CT; ++u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += av[u] * f[v];
      }
    }
#pragma unroll
    for (int u = 0; u < BG_CT; ++u) {
      const int k = BG_CT * ct + u;
      if (k < n_cls) *reinterpret_cast<f32x4*>(ob + (long long)k * Cf + 4 * q) = acc[u];
    }
  }
}

extern "C" int aod_badge_embedding(const float* feat, const float* post, const int32_t* cls, const int32_t* cnt, int B, int K, int Cf, int W,
                                   int n_cls, float* out, int64_t out_stride, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1, "badge_embedding: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(K >= 1 && K <= BG_MAX_OBJ, "badge_embedding: max_obj must be in 1..%d (got %d)", BG_MAX_OBJ, K);
  AOD_CHECK_ARG(Cf >= 8 && Cf % 8 == 0 && Cf <= BG_MAX_C, "badge_embedding: channels must be a multiple of 8 in 8..%d (got %d)", BG_MAX_C, Cf);
  AOD_CHECK_ARG(n_cls >= 1 && n_cls <= BG_MAX_CLS, "badge_embedding: n_cls must be in 1..%d (got %d)", BG_MAX_CLS, n_cls);
  AOD_CHECK_ARG(W >= n_cls && W <= 65536, "badge_embedding: posterior rows of n_cls = %d .. 65536 columns (got W = %d)", n_cls, W);
  AOD_CHECK_ARG(feat && post && cls && cnt && out, "badge_embedding: null pointer");
  AOD_CHECK_ARG(out_stride >= (int64_t)n_cls * Cf && out_stride % 4 == 0,
                "badge_embedding: row stride %lld: a multiple of 4 floats, at least n_cls * Cf = %lld", (long long)out_stride, (long long)n_cls * Cf);
  AOD_CHECK_ARG(((((size_t)feat) | ((size_t)out)) & 15) == 0 && ((((size_t)post) | ((size_t)cls) | ((size_t)cnt)) & 3) == 0,
                "badge_embedding: feat and out must be 16-B aligned, the other pointers 4-B aligned");
  const int NP = (n_cls + BG_CT - 1) / BG_CT * BG_CT;
  hipLaunchKernelGGL(badge_embedding_kernel, dim3((unsigned)B), dim3(256), (size_t)K * NP * sizeof(float), (hipStream_t)stream, feat, post, cls, cnt,
                     K, Cf, W, n_cls, out, (long long)out_stride);
  AOD_LAUNCH_CHECK();
  return 0;
}
