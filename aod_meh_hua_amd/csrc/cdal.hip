// CDAL acquisition (S. Agarwal, H. Arora, S. Anand, C. Arora, "Contextual Diversity for Active Learning", ECCV 2020), core-set form CDAL-CS:
// one class-mixture descriptor per image from the per-level classification maps.  The reference tree has no CDAL: the semantics are fixed
// in DESIGN 3j.
//
// Per anchor row r (C contiguous logits) of every level of image b:
//     p = softmax(x) = exp(x - max) / sum;  region iff max_k p[k] > score_thr (strict);  class c = argmax_k p[k], lowest index on a tie
//     w = H(p) + 2^-10,  H = -sum p ln p,  0 ln 0 = 0
// Per class c:  M[c] = sum_{r: c_r = c} w_r p_r / sum_{r: c_r = c} w_r   (1 / C where the class owns no region)
//               P[c] = (1 - 2^-10) M[c] + 2^-10 / C;   out[b] = [P | ln P], 2 C^2 fp32.
// Two launches, no atomics:
//   cdal_partial_kernel   one WAVE (a 64-thread workgroup) per fixed chunk of CD_CHUNK rows of one (image, level), 64 rows at a time: the
//                         64 x C logits are staged in LDS with 16-B loads, a lane per row computes softmax / class / entropy, then the rows
//                         that passed the threshold are taken in ascending row order: lane k adds w p[k] into the LDS accumulator
//                         acc[c][k], lane C adds w into acc[c][C].  The chunk's [C][C + 1] accumulator goes to the workspace.
//   cdal_finalize_kernel  one workgroup per (image, class): four waves add every fourth chunk partial each, in (level, chunk) order, a fixed
//                         tree adds the four; then it divides, fills an empty class, smooths, writes P and logf(P).
// Every sum has a fixed association that depends on the row's index inside its own image only -- not on the batch size, the image's
// position in the batch or the load width: an image has the same descriptor bits alone, in any batch, eager or replayed.
// ln p[k] = (x[k] - max) - log1p(t), t = the sum of the other exponentials (the maximum's own is exactly 1): every entropy term
// p[k] (log1p(t) - (x[k] - max)) is non-negative and carries a few ulp of RELATIVE error, also for a row that is all but one-hot.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define CD_CHUNK 128         // rows per workgroup: 2 passes of 64 rows (a lane per row); 16 x 512^2 then is 6 272 waves for 1 024 SIMDs
#define CD_MAX_C 32          // 2 C^2 <= 2048 = the k-center kernels' widest row
#define CD_MAX_L 8

// Pointers travel as kernel arguments (ensemble_mi.hip does the same): no device table, no H2D copy, no sync.
struct CdArgs {
  const float* p[CD_MAX_L];                   // level maps [B][rows][C]
  long long rows[CD_MAX_L];                   // rows per image
  int nchunks[CD_MAX_L];                      // ceil(rows / CD_CHUNK)
  int cum[CD_MAX_L];                          // chunks of the levels in front (per image)
  int tot;                                    // chunks per image
  int L, C;
};

__global__ __launch_bounds__(64) void cdal_partial_kernel(const CdArgs s, float thr, float* __restrict__ partials) {
  extern __shared__ __align__(16) float cd_lds[];                 // (2 * 64 * C + C * (C + 1)) floats: 11.9 KB at C = 20
  const int lane = threadIdx.x;
  const int b = blockIdx.x / s.tot, r = blockIdx.x % s.tot;
  int l = 0;
  for (int i = 1; i < s.L; ++i)
    if (r >= s.cum[i]) l = i;
  const int ch = r - s.cum[l];
  const int C = s.C, C1 = C + 1;
  float* xs = cd_lds;                                              // the logits of 64 rows as they lie in memory
  float* ps = xs + 64 * C;                                         // their exponentials, then probabilities
  float* acc = ps + 64 * C;                                        // [C][C + 1]: sum w p | sum w
  const long long rows = s.rows[l];
  const float* img = s.p[l] + (long long)b * rows * C;
  // 16-B loads need the image's base 16-B aligned (b * rows * C * 4 bytes is not for every C); otherwise, and for a piece that crosses the
  // end of the 64 rows, the same elements are read one by one into the same LDS words (a pass starts 64 * C floats = a multiple of 16 B in)
  const bool vec = (((size_t)img) & 15) == 0;
  for (int i = lane; i < C * C1; i += 64) acc[i] = 0.f;
  for (int pass = 0; pass < CD_CHUNK / 64; ++pass) {
    const long long r0 = (long long)ch * CD_CHUNK + pass * 64;
    if (r0 >= rows) break;                                         // (wave-uniform)
    const int nb = rows - r0 < 64 ? (int)(rows - r0) : 64;
    const int n = nb * C;
    const float* g = img + r0 * C;
    for (int e = 4 * lane; e < n; e += 256) {
      if (vec && e + 3 < n) {
        *reinterpret_cast<f32x4*>(xs + e) = *reinterpret_cast<const f32x4*>(g + e);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e + u < n) xs[e + u] = g[e + u];
      }
    }
    __syncthreads();
    bool region = false;
    int cls = 0;
    float w = 0.f;
    if (lane < nb) {
      const float* x = xs + lane * C;
      float* p = ps + lane * C;
      float m = x[0];
      int km = 0;
      for (int k = 1; k < C; ++k) {
        const float v = x[k];
        if (v > m) { m = v; km = k; }
      }
      float t = 0.f;                                               // the exponentials in class order, the maximum's own (exactly 1) left out
      for (int k = 0; k < C; ++k) {
        const float e = expf(x[k] - m);
        p[k] = e;
        t += k == km ? 0.f : e;
      }
      const float sum = 1.0f + t, ls = log1pf(t);
      float pm = -1.f, h = 0.f;
      for (int k = 0; k < C; ++k) {
        const float q = p[k] / sum;
        p[k] = q;
        if (q > pm) { pm = q; cls = k; }
        h += q > 0.f ? q * (ls - (x[k] - m)) : 0.f;
      }
      region = pm > thr;
      w = h + 0.0009765625f;
    }
    __syncthreads();
    unsigned long long mask = __ballot(region);
    while (mask) {                                                 // the rows that passed, in ascending row order (wave-uniform)
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int c = __shfl(cls, j, 64);
      const float wj = __shfl(w, j, 64);
      if (lane < C) acc[c * C1 + lane] += wj * ps[j * C + lane];
      else if (lane == C) acc[c * C1 + C] += wj;
    }
    __syncthreads();
  }
  float* q = partials + (long long)blockIdx.x * (C * C1);
  for (int i = lane; i < C * C1; i += 64) q[i] = acc[i];
}

// one workgroup per (image, class c): wave q adds the chunks q, q + 4, q + 8, ... in that order, lane k the element [c][k] (k <= C);
// ((s0 + s1) + (s2 + s3)); lane k < C then divides, smooths and writes P[c][k] and its logarithm
__global__ __launch_bounds__(256) void cdal_finalize_kernel(const float* __restrict__ partials, int tot, int C, float* __restrict__ out,
                                                            long long out_stride) {
  __shared__ float S[4][CD_MAX_C + 1];
  const int b = blockIdx.x / C, c = blockIdx.x % C, C1 = C + 1, n = C * C1;
  const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
  if (k < C1) {
    const float* src = partials + (long long)b * tot * n + c * C1 + k;
    float v = 0.f;
    for (int j = q; j < tot; j += 4) v += src[(long long)j * n];
    S[q][k] = v;
  }
  __syncthreads();
  if (q == 0 && k < C) {
    const float sw = (S[0][C] + S[1][C]) + (S[2][C] + S[3][C]);
    const float sp = (S[0][k] + S[1][k]) + (S[2][k] + S[3][k]);
    const float uni = 1.0f / (float)C, keep = 1.0f - 0.0009765625f, floor_ = 0.0009765625f / (float)C;
    const float mix = sw > 0.f ? sp / sw : uni;
    const float P = keep * mix + floor_;
    float* o = out + (long long)b * out_stride + c * C + k;
    o[0] = P;
    o[C * C] = logf(P);
  }
}

static int cd_shape(int L, const int64_t* rows_per_level, int C, int B, CdArgs* s) {
  AOD_CHECK_ARG(L >= 1 && L <= CD_MAX_L, "cdal_descriptor: 1..8 levels (got %d)", L);
  AOD_CHECK_ARG(C >= 1 && C <= CD_MAX_C, "cdal_descriptor: 1..%d classes (2 C^2 <= 2048 descriptor columns; got C = %d)", CD_MAX_C, C);
  AOD_CHECK_ARG(B >= 1, "cdal_descriptor: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(rows_per_level, "cdal_descriptor: null level sizes");
  long long tot = 0;
  for (int l = 0; l < L; ++l) {
    const long long n = rows_per_level[l];
    AOD_CHECK_ARG(n >= 1, "cdal_descriptor: level %d holds %lld rows per image", l, n);
    const long long ch = (n + CD_CHUNK - 1) / CD_CHUNK;
    s->rows[l] = n;
    s->nchunks[l] = (int)(ch > 0x7fffffffll ? 0x7fffffffll : ch);
    s->cum[l] = (int)tot;
    tot += ch;
    AOD_CHECK_ARG(tot * B <= 0x7fffffffll, "cdal_descriptor: grid too large (%lld chunks x %d images)", tot, B);
  }
  for (int l = L; l < CD_MAX_L; ++l) { s->p[l] = nullptr; s->rows[l] = 0; s->nchunks[l] = 0; s->cum[l] = (int)tot; }
  s->tot = (int)tot;
  s->L = L;
  s->C = C;
  return 0;
}

// workspace: one [C][C + 1] fp32 accumulator per chunk of CD_CHUNK rows of every (image, level); the count of floats, 0 for a bad shape
extern "C" size_t aod_cdal_ws_len(int L, const int64_t* rows_per_level, int C, int B) {
  CdArgs s;
  if (cd_shape(L, rows_per_level, C, B, &s) != 0) return 0;
  return (size_t)s.tot * (size_t)B * (size_t)(C * (C + 1));
}

extern "C" int aod_cdal_chunk(void) { return CD_CHUNK; }

extern "C" int aod_cdal_descriptor(const void* const* maps, int L, const int64_t* rows_per_level, int C, int B, float score_thr, float* out,
                                   int64_t out_stride, float* ws, int64_t ws_capacity, aod_stream_t stream) {
  CdArgs s;
  const int rc = cd_shape(L, rows_per_level, C, B, &s);
  if (rc != 0) return rc;
  AOD_CHECK_ARG(maps && out && ws, "cdal_descriptor: null pointer");
  AOD_CHECK_ARG(out_stride >= 2ll * C * C, "cdal_descriptor: row stride %lld is less than the %d descriptor columns", (long long)out_stride,
                2 * C * C);
  AOD_CHECK_ARG((((size_t)out) & 3) == 0 && (((size_t)ws) & 3) == 0, "cdal_descriptor: out and ws must be 4-B aligned");
  AOD_CHECK_ARG(score_thr == score_thr, "cdal_descriptor: score_thr is NaN");
  for (int l = 0; l < L; ++l) {
    AOD_CHECK_ARG(maps[l], "cdal_descriptor: null map pointer (level %d)", l);
    AOD_CHECK_ARG((((size_t)maps[l]) & 3) == 0, "cdal_descriptor: map pointer not 4-B aligned (level %d)", l);
    s.p[l] = (const float*)maps[l];
  }
  const long long need = (long long)s.tot * B * (C * (C + 1));
  if (need > ws_capacity) return aod_set_err(-2, "cdal_descriptor: workspace too small (%lld floats, capacity %lld)", need, (long long)ws_capacity);
  AOD_CHECK_ARG((long long)B * C <= 0x7fffffffll, "cdal_descriptor: grid too large (%d images x %d classes)", B, C);
  hipLaunchKernelGGL(cdal_partial_kernel, dim3((unsigned)((long long)s.tot * B)), dim3(64), (size_t)(128 * C + C * (C + 1)) * sizeof(float),
                     (hipStream_t)stream, s, score_thr, ws);
  hipLaunchKernelGGL(cdal_finalize_kernel, dim3((unsigned)(B * C)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, s.tot, C, out, (long long)out_stride);
  AOD_LAUNCH_CHECK();
  return 0;
}
