// Ensemble / MC-dropout mutual information of the sigmoid classification maps (the reference's comparison baselines:
// mmdet/apis/CalEnsembleUnc.py:164-180 ComputeMI, mmdet/apis/CalMCDropoutUnc.py:183-199 ComputeMCDropoutMI).
//
// Per image b and level l, with p_k = sigmoid(x_k) of member k of K and avg = mean_k p_k:
//     epistemic.mean() = ( sum over ALL elements of [ -avg ln avg + (1/K) sum_k p_k ln p_k ] ) / rows_l,   rows_l = n_l / n_cls
//     score[b]         = mean over levels of that
// The class structure only appears in the divisor, so the maps are streamed as flat [B][n_l] fp32 arrays (NCHW-contiguous and channels_last
// give the same sum).  Two launches, no atomics:
//   ensemble_mi_partial_kernel   one 256-thread workgroup per fixed chunk of MI_CHUNK elements of one (image, level): one partial each
//   ensemble_mi_finalize_kernel  one workgroup per image: chunks of each level added in index order in double, / rows_l, mean over levels
// Every sum has a fixed association that depends on the element's index inside its image only -- not on the batch size, the image's
// position in the batch or the load width: a launch is bit-reproducible and an image scores the same bits alone and inside a batch.
// Convention: 0 ln 0 = 0 (hua_closed_kernel's); the reference returns NaN for the image once a sigmoid underflows.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define MI_CHUNK 4096        // elements per workgroup: 256 threads x 4 pieces of 4 consecutive elements
#define MI_MAX_K 32
#define MI_MAX_L 8

// Pointers travel as kernel arguments (K * L <= 256 pointers = 2 KB of the 4 KB argument segment): no device table, no H2D copy, no sync.
struct MiPtrs {
  const float* p[MI_MAX_L * MI_MAX_K];        // [level][member]
};
struct MiShape {
  long long n[MI_MAX_L];                      // elements per image
  double rows[MI_MAX_L];                      // n / n_cls
  int nchunks[MI_MAX_L];                      // ceil(n / MI_CHUNK)
  int cum[MI_MAX_L];                          // chunks of the levels in front (per image)
  int tot;                                    // chunks per image
  int K, L;
};

// p = sigmoid(x), ln p = -softplus(-x); with t = exp(-|x|):  x >= 0: p = 1 / (1 + t), ln p = -log1p(t);  x < 0: p = t / (1 + t), ln p = x - log1p(t).
// p ln p is finite for every finite x (x -> -inf: p = 0, ln p = x, product 0).
__device__ __forceinline__ void mi_member(float x, float& sp, float& sl) {
  const float t = expf(-fabsf(x));
  const float p = (x >= 0.f ? 1.0f : t) / (1.0f + t);
  const float lp = (x >= 0.f ? 0.f : x) - log1pf(t);
  sp += p;
  sl += p > 0.f ? p * lp : 0.f;
}

__global__ __launch_bounds__(256) void ensemble_mi_partial_kernel(const MiPtrs ptrs, const MiShape s, float* __restrict__ partials) {
  __shared__ float red[4];
  const int b = blockIdx.x / s.tot, r = blockIdx.x % s.tot;
  int l = 0;
  for (int i = 1; i < s.L; ++i)
    if (r >= s.cum[i]) l = i;
  const int c = r - s.cum[l];
  const long long n = s.n[l];
  const long long img = (long long)b * n;
  const int K = s.K;
  // 16-B loads need every member's image base 16-B aligned (b * n * 4 bytes is not when n % 4 != 0); otherwise, and for a piece that
  // crosses the end of the image, the same elements are read one by one -- into the same registers, so the sums below do not change
  size_t mis = 0;
  for (int k = 0; k < K; ++k) mis |= (size_t)(ptrs.p[l * MI_MAX_K + k] + img);
  const bool vec = (mis & 15) == 0;
  const long long e0 = (long long)c * MI_CHUNK + 4 * (long long)threadIdx.x;        // piece j starts at e0 + 1024 * j
  float sp[4][4], sl[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) sp[j][u] = sl[j][u] = 0.f;
  for (int k = 0; k < K; ++k) {                      // members in pointer order
    const float* g = ptrs.p[l * MI_MAX_K + k] + img;
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = e0 + 1024 * j;
      if (vec && e + 3 < n) {
        v[j] = *reinterpret_cast<const f32x4*>(g + e);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[j][u] = e + u < n ? g[e + u] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) mi_member(v[j][u], sp[j][u], sl[j][u]);
  }
  const float Kf = (float)K;
  float acc = 0.f;                                   // this thread's 16 elements in index order
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (e0 + 1024 * j + u < n) {
        const float avg = sp[j][u] / Kf;
        const float total = avg > 0.f ? -(avg * logf(avg)) : 0.f;
        acc += total + sl[j][u] / Kf;
      }
    }
  acc = wave_sum(acc);                               // xor butterfly: the same tree in every lane
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void ensemble_mi_finalize_kernel(const float* __restrict__ partials, const MiShape s, float* __restrict__ out) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  double score = 0.0;
  for (int l = 0; l < s.L; ++l) {
    const float* q = partials + (long long)b * s.tot + s.cum[l];
    double v = 0.0;
    for (int i = threadIdx.x; i < s.nchunks[l]; i += 256) v += (double)q[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) score += red[0] / s.rows[l];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[b] = (float)(score / (double)s.L);
}

static int mi_shape(int K, int L, const int64_t* n_per_level, int B, int n_cls, MiShape* s) {
  AOD_CHECK_ARG(K >= 2 && K <= MI_MAX_K, "ensemble_mi: 2..32 members (got %d)", K);
  AOD_CHECK_ARG(L >= 1 && L <= MI_MAX_L, "ensemble_mi: 1..8 levels (got %d)", L);
  AOD_CHECK_ARG(B >= 1, "ensemble_mi: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(n_cls >= 1, "ensemble_mi: n_cls must be positive (got %d)", n_cls);
  AOD_CHECK_ARG(n_per_level, "ensemble_mi: null level sizes");
  long long tot = 0;
  for (int l = 0; l < L; ++l) {
    const long long n = n_per_level[l];
    AOD_CHECK_ARG(n >= 1 && n % n_cls == 0, "ensemble_mi: level %d holds %lld elements per image, not a positive multiple of n_cls = %d", l, n, n_cls);
    s->n[l] = n;
    s->rows[l] = (double)(n / n_cls);
    const long long ch = (n + MI_CHUNK - 1) / MI_CHUNK;
    AOD_CHECK_ARG(ch <= 0x7fffffffll, "ensemble_mi: level %d too large", l);
    s->nchunks[l] = (int)ch;
    s->cum[l] = (int)tot;
    tot += ch;
    AOD_CHECK_ARG(tot * B <= 0x7fffffffll, "ensemble_mi: grid too large (%lld chunks x %d images)", tot, B);
  }
  for (int l = L; l < MI_MAX_L; ++l) { s->n[l] = 0; s->rows[l] = 1.0; s->nchunks[l] = 0; s->cum[l] = (int)tot; }
  s->tot = (int)tot;
  s->K = K;
  s->L = L;
  return 0;
}

extern "C" size_t aod_ensemble_mi_partials_len(int L, const int64_t* n_per_level, int B) {
  MiShape s;
  if (mi_shape(2, L, n_per_level, B, 1, &s) != 0) return 0;
  return (size_t)s.tot * (size_t)B;
}

extern "C" int aod_ensemble_mi(const void* const* maps, int K, int L, const int64_t* n_per_level, int B, int n_cls, float* out,
                               float* partials_ws, int64_t ws_capacity, aod_stream_t stream) {
  MiShape s;
  const int rc = mi_shape(K, L, n_per_level, B, n_cls, &s);
  if (rc != 0) return rc;
  AOD_CHECK_ARG(maps && out && partials_ws, "ensemble_mi: null pointer");
  MiPtrs ptrs;
  for (int i = 0; i < MI_MAX_L * MI_MAX_K; ++i) ptrs.p[i] = nullptr;
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < L; ++l) {
      AOD_CHECK_ARG(maps[k * L + l], "ensemble_mi: null map pointer (member %d, level %d)", k, l);
      AOD_CHECK_ARG((((size_t)maps[k * L + l]) & 3) == 0, "ensemble_mi: map pointer not 4-B aligned (member %d, level %d)", k, l);
      ptrs.p[l * MI_MAX_K + k] = (const float*)maps[k * L + l];
    }
  const long long need = (long long)s.tot * B;
  if (need > ws_capacity) return aod_set_err(-2, "ensemble_mi: workspace too small (%lld partials, capacity %lld)", need, (long long)ws_capacity);
  hipLaunchKernelGGL(ensemble_mi_partial_kernel, dim3((unsigned)need), dim3(256), 0, (hipStream_t)stream, ptrs, s, partials_ws);
  hipLaunchKernelGGL(ensemble_mi_finalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)partials_ws, s, out);
  AOD_LAUNCH_CHECK();
  return 0;
}
