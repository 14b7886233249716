// Core-set acquisition (k-center greedy; O. Sener, S. Savarese, "Active Learning for Convolutional Neural Networks: A Core-Set Approach",
// ICLR 2018, Algorithm 1).  The reference tree has no Core-set: the semantics are fixed in DESIGN 3i.
//
// 1. pool_descriptor_kernel: the descriptor of an image = concatenation over pyramid levels of the global average of the neck output,
//    read from the bf16 / X-layout rows as they lie in the pyramid buffer (up to 8 row segments, one launch per batch).  One workgroup per
//    (image, level, group of 64 channels): 32 row lanes x 8 octets; row lane r adds rows r, r + 32, r + 64, ... in that order, a fixed
//    LDS tree adds the 32 lanes, one division by h * w.  The order of every sum depends on h * w only: an image's descriptor has the same
//    bits alone and in any batch.  16-B loads, no atomics.
// 2. k-center greedy on desc [N][D] fp32, everything on the device, no host sync and no cross-workgroup wait inside a launch:
//      kcenter_prepare_kernel   mind = +inf, selected = 0
//      kcenter_mark_kernel      selected[labelled] = 1
//      kcenter_centers_kernel   one launch per chunk of KC_CHUNK labelled centers staged in LDS: mind[i] = min(mind[i], min_c d(i, c))
//      kcenter_keys_kernel      per-workgroup partial of max over unselected i of key(i) = (bits(mind[i]) << 32) | ~i
//      kcenter_step_kernel      ONE launch per pick: every workgroup reduces the previous launch's partials (redundantly: an unsigned max is
//                               exact, so every workgroup finds the same pick), workgroup 0 records pick / radius / selected, then the
//                               workgroup sweeps its rows against the picked center and writes its partial into the other partial buffer.
//    d(i, c) = sum_k (x_ik - x_ck)^2 in the direct form; ONE wave per row, lane j owns the elements 4j + 256m (+0..3) (D % 4 == 0; else
//    j + 64m), four running sums per lane, ((s0 + s1) + (s2 + s3)), xor butterfly: a function of the two rows and D alone.
//    aod_kcenter_greedy_ex(..., metric = 1): the same kernels instantiated for the symmetrised KL divergence of [P | ln P] rows (CDAL,
//    DESIGN 3j; kc_dists); metric 0 keeps the arithmetic above.
//    aod_kcenter_greedy_matrix (CCMS): the same scheme on a precomputed [N][N] distance matrix (kcenter_matrix_* below).
//    Non-negative floats order like their bit patterns as unsigned integers (+inf included) and ~i makes the LOWEST index win a tie.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define PD_MAX_SEG 8
#define KC_CHUNK 8           // labelled centers per initialisation launch (aod_kcenter_chunk)
#define KC_MAX_D 2048        // KC_CHUNK * KC_MAX_D * 4 B = 64 KB of LDS
#define KC_MAX_GRID 1024     // workgroups (= partial keys) of a sweep
#define KC_WAVES 4

// ------------------------------------------------------------------------------------------------------------------ descriptor
struct PdSegs {
  long long row0[PD_MAX_SEG];        // first row of the level (image 0)
  int hw[PD_MAX_SEG];                // rows per image
  int nseg;
};

__device__ __forceinline__ void pd_load(const bf16_t* __restrict__ p, int x3, float (&v)[8]) {
  const bf16x8 h = *reinterpret_cast<const bf16x8*>(p);
  if (x3) {
    const bf16x8 l = *reinterpret_cast<const bf16x8*>(p + 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j] + (float)l[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
  }
}

__global__ __launch_bounds__(256) void pool_descriptor_kernel(const bf16_t* __restrict__ base, const PdSegs s, int C, int x3, int groups,
                                                              float* __restrict__ out, long long out_stride) {
  __shared__ float red[32][65];
  const int g = blockIdx.x % groups;
  const int l = (blockIdx.x / groups) % s.nseg;
  const int b = blockIdx.x / (groups * s.nseg);
  const int oc = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int o = g * 8 + oc;                                      // logical octet: channels 8o .. 8o + 7
  const bool live = o * 8 < C;                                   // (C % 8 == 0: an octet is all channels or all pad; pad is never read)
  const int hw = s.hw[l];
  const long long pitch = x3 ? 2ll * ((C + 31) / 32 * 32) : (long long)C;
  const int col = x3 ? ((o >> 2) << 6) + ((o & 3) << 3) : o * 8;
  const bf16_t* p = base + (s.row0[l] + (long long)b * hw) * pitch + col;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (live) {
    int m = r;
    for (; m + 96 < hw; m += 128) {                              // four rows in flight, added in row order
      float v0[8], v1[8], v2[8], v3[8];
      pd_load(p + (long long)m * pitch, x3, v0);
      pd_load(p + (long long)(m + 32) * pitch, x3, v1);
      pd_load(p + (long long)(m + 64) * pitch, x3, v2);
      pd_load(p + (long long)(m + 96) * pitch, x3, v3);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = (((acc[j] + v0[j]) + v1[j]) + v2[j]) + v3[j];
    }
    for (; m < hw; m += 32) {
      float v[8];
      pd_load(p + (long long)m * pitch, x3, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[r][oc * 8 + j] = acc[j];
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {                             // fixed tree over the 32 row lanes
    if (r < w) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[r][oc * 8 + j] += red[r + w][oc * 8 + j];
    }
    __syncthreads();
  }
  if (r == 0 && live) {
    const float n = (float)hw;
    float* q = out + (long long)b * out_stride + (long long)l * C + o * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = red[0][oc * 8 + j] / n;
  }
}

extern "C" int aod_pool_descriptor(const void* base, int nseg, const int64_t* seg_row0, const int32_t* seg_hw, int C, int x3, int B,
                                   float* out, int64_t out_stride, aod_stream_t stream) {
  AOD_CHECK_ARG(nseg >= 1 && nseg <= PD_MAX_SEG, "pool_descriptor: 1..8 segments (got %d)", nseg);
  AOD_CHECK_ARG(base && out && seg_row0 && seg_hw, "pool_descriptor: null pointer");
  AOD_CHECK_ARG(C >= 8 && C % 8 == 0, "pool_descriptor: channels must be a positive multiple of 8 (got %d)", C);
  AOD_CHECK_ARG(B >= 1, "pool_descriptor: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(out_stride >= (int64_t)nseg * C, "pool_descriptor: row stride %lld is less than the %lld descriptor columns", (long long)out_stride,
                (long long)nseg * C);
  AOD_CHECK_ARG((((size_t)base) & 15) == 0 && (((size_t)out) & 3) == 0, "pool_descriptor: rows must be 16-B aligned, out 4-B aligned");
  PdSegs s;
  for (int l = 0; l < PD_MAX_SEG; ++l) { s.row0[l] = 0; s.hw[l] = 1; }
  for (int l = 0; l < nseg; ++l) {
    AOD_CHECK_ARG(seg_row0[l] >= 0 && seg_hw[l] >= 1, "pool_descriptor: segment %d: first row %lld, %d rows per image", l, (long long)seg_row0[l],
                  (int)seg_hw[l]);
    s.row0[l] = seg_row0[l];
    s.hw[l] = seg_hw[l];
  }
  s.nseg = nseg;
  const int groups = (C + 63) / 64;
  const long long grid = (long long)B * nseg * groups;
  AOD_CHECK_ARG(grid <= 0x7fffffffll, "pool_descriptor: grid too large");
  hipLaunchKernelGGL(pool_descriptor_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)base, s, C, x3 ? 1 : 0, groups,
                     out, (long long)out_stride);
  AOD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ k-center greedy
typedef unsigned long long u64;

__device__ __forceinline__ u64 kc_key(float m, unsigned i) { return ((u64)__float_as_uint(m) << 32) | (u64)(~i); }

__device__ __forceinline__ u64 kc_wave_max(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(k, o, 64);
    k = other > k ? other : k;
  }
  return k;
}

// max over the workgroup's 256 threads, the same value in every thread (red: KC_WAVES entries; ends with a barrier)
__device__ __forceinline__ u64 kc_block_max(u64 k, u64* red) {
  k = kc_wave_max(k);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
  __syncthreads();
  u64 m = red[0];
#pragma unroll
  for (int w = 1; w < KC_WAVES; ++w) m = red[w] > m ? red[w] : m;
  __syncthreads();
  return m;
}

// distances of row x to NC centers staged in LDS (cen[c * D + k]); every lane returns all NC values.
// METRIC 0: the squared Euclidean distance.  METRIC 1 (CDAL): a row is [P | ln P], two halves of H = D / 2 columns, and
// d = 1/2 sum_k max((P_k - Q_k)(ln P_k - ln Q_k), 0): the symmetrised KL divergence (every term is non-negative; the max only guards
// against rounding).  The same lane ownership over the H columns of a half (4j + 256m (+0..3) when H % 4 == 0, else j + 64m), the same four
// running sums and the same butterfly as metric 0 over its D columns; the halving is exact.
template <int NC, int METRIC>
__device__ __forceinline__ void kc_dists(const float* __restrict__ x, const float* cen, int D, int lane, float (&d)[NC]) {
  float s[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c][0] = s[c][1] = s[c][2] = s[c][3] = 0.f;
  if constexpr (METRIC == 0) {
    if ((D & 3) == 0) {
      for (int k = 4 * lane; k < D; k += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + k);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(cen + c * D + k);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float t = v[u] - q[u];
            s[c][u] += t * t;
          }
        }
      }
    } else {
      for (int k = lane; k < D; k += 64) {
        const float v = x[k];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float t = v - cen[c * D + k];
          s[c][0] += t * t;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) d[c] = wave_sum((s[c][0] + s[c][1]) + (s[c][2] + s[c][3]));
  } else {
    const int H = D >> 1;                                          // (the entry refuses an odd D)
    if ((H & 3) == 0) {
      for (int k = 4 * lane; k < H; k += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + k);
        const f32x4 lv = *reinterpret_cast<const f32x4*>(x + H + k);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(cen + c * D + k);
          const f32x4 lq = *reinterpret_cast<const f32x4*>(cen + c * D + H + k);
#pragma unroll
          for (int u = 0; u < 4; ++u) s[c][u] += fmaxf((v[u] - q[u]) * (lv[u] - lq[u]), 0.f);
        }
      }
    } else {
      for (int k = lane; k < H; k += 64) {
        const float v = x[k], lv = x[H + k];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c][0] += fmaxf((v - cen[c * D + k]) * (lv - cen[c * D + H + k]), 0.f);
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) d[c] = 0.5f * wave_sum((s[c][0] + s[c][1]) + (s[c][2] + s[c][3]));
  }
}

__global__ __launch_bounds__(256) void kcenter_prepare_kernel(float* __restrict__ mind, unsigned char* __restrict__ sel, long long N) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    mind[i] = __uint_as_float(0x7f800000u);
    sel[i] = 0;
  }
}

__global__ __launch_bounds__(256) void kcenter_mark_kernel(const long long* __restrict__ lab, int n_lab, unsigned char* __restrict__ sel, long long N) {
  for (int j = blockIdx.x * 256 + threadIdx.x; j < n_lab; j += 256 * gridDim.x) {
    const long long c = lab[j];
    if (c >= 0 && c < N) sel[c] = 1;
  }
}

template <int METRIC>
__global__ __launch_bounds__(256) void kcenter_centers_kernel(const float* __restrict__ desc, long long N, int D, const long long* __restrict__ lab,
                                                              int nc, float* __restrict__ mind) {
  extern __shared__ __align__(16) float cen[];                   // [KC_CHUNK][D]
  unsigned ok = 0;                                               // (workgroup-uniform; the static LDS stays empty: the chunk may fill all 64 KB)
  for (int c = 0; c < KC_CHUNK; ++c) {                           // a short chunk repeats its last center: the minimum does not change
    const long long ci = lab[c < nc ? c : nc - 1];
    const bool in = ci >= 0 && ci < N;                            // (the caller validates; an index outside the matrix is never dereferenced)
    ok |= (in ? 1u : 0u) << c;
    for (int k = threadIdx.x; k < D; k += 256) cen[c * D + k] = in ? desc[ci * D + k] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long wave = blockIdx.x * (long long)KC_WAVES + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * KC_WAVES;
  for (long long i = wave; i < N; i += nwaves) {
    float d[KC_CHUNK];
    kc_dists<KC_CHUNK, METRIC>(desc + i * D, cen, D, lane, d);
    if (lane == 0) {
      float m = mind[i];
#pragma unroll
      for (int c = 0; c < KC_CHUNK; ++c) m = ((ok >> c) & 1u) ? fminf(m, d[c]) : m;
      mind[i] = m;
    }
  }
}

__global__ __launch_bounds__(256) void kcenter_keys_kernel(const float* __restrict__ mind, const unsigned char* __restrict__ sel, long long N,
                                                           u64* __restrict__ keys_out) {
  __shared__ u64 red[KC_WAVES];
  u64 key = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    if (!sel[i]) {
      const u64 k = kc_key(mind[i], (unsigned)i);
      key = k > key ? k : key;
    }
  }
  key = kc_block_max(key, red);
  if (threadIdx.x == 0) keys_out[blockIdx.x] = key;
}

// launch t = 1 .. budget: pick t - 1 (0-based) comes out of keys_in, is recorded, and every mind takes the distance to it
template <int METRIC>
__global__ __launch_bounds__(256) void kcenter_step_kernel(const float* __restrict__ desc, long long N, int D, float* __restrict__ mind,
                                                           unsigned char* __restrict__ sel, const u64* __restrict__ keys_in, int nkeys,
                                                           u64* __restrict__ keys_out, long long* __restrict__ picks, float* __restrict__ radius,
                                                           int t) {
  extern __shared__ __align__(16) float cen[];                   // [D]
  __shared__ u64 red[KC_WAVES];
  u64 best = 0;
  for (int j = threadIdx.x; j < nkeys; j += 256) {
    const u64 k = keys_in[j];
    best = k > best ? k : best;
  }
  best = kc_block_max(best, red);
  const unsigned p = ~(unsigned)(best & 0xffffffffull);
  const bool valid = best != 0 && (long long)p < N;               // (no candidate: budget exceeds the unselected rows -- refused by the entry)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    picks[t - 1] = valid ? (long long)p : -1ll;
    radius[t - 1] = __uint_as_float((unsigned)(best >> 32));
    if (valid) sel[p] = 1;
  }
  if (!valid) {                                                   // workgroup-uniform
    if (threadIdx.x == 0) keys_out[blockIdx.x] = 0;
    return;
  }
  for (int k = threadIdx.x; k < D; k += 256) cen[k] = desc[(long long)p * D + k];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long wave = blockIdx.x * (long long)KC_WAVES + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * KC_WAVES;
  u64 key = 0;
  for (long long i = wave; i < N; i += nwaves) {
    float d[1];
    kc_dists<1, METRIC>(desc + i * D, cen, D, lane, d);
    if (lane == 0) {
      const float m = fminf(mind[i], d[0]);
      mind[i] = m;
      if (i != (long long)p && !sel[i]) {                          // (workgroup 0 may or may not have set sel[p] yet: p is excluded by name)
        const u64 k = kc_key(m, (unsigned)i);
        key = k > key ? k : key;
      }
    }
  }
  key = kc_block_max(key, red);
  if (threadIdx.x == 0) keys_out[blockIdx.x] = key;
}

static inline int kc_grid(long long N) {
  long long g = (N + KC_WAVES - 1) / KC_WAVES;
  return (int)(g > KC_MAX_GRID ? KC_MAX_GRID : (g < 1 ? 1 : g));
}

extern "C" int aod_kcenter_chunk(void) { return KC_CHUNK; }

// workspace: two partial-key buffers of KC_MAX_GRID 64-bit words, then the selected mask (one byte per row)
extern "C" size_t aod_kcenter_ws_len(int64_t N) {
  if (N < 1 || N > 0x7fffffffll) return 0;
  return (size_t)2 * KC_MAX_GRID * sizeof(u64) + (((size_t)N + 15) & ~(size_t)15);
}

template <int METRIC>
static int kc_greedy(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks, float* radius,
                     float* mind, void* ws, aod_stream_t stream) {
  AOD_CHECK_ARG(N >= 1 && N <= 0x7fffffffll, "kcenter_greedy: 1 .. 2^31 - 1 rows (got %lld)", (long long)N);
  AOD_CHECK_ARG(D >= 1 && D <= KC_MAX_D, "kcenter_greedy: 1 .. %d descriptor columns (got %d)", KC_MAX_D, D);
  AOD_CHECK_ARG(n_labelled >= 0 && n_labelled <= N, "kcenter_greedy: labelled count %lld outside 0 .. N = %lld", (long long)n_labelled, (long long)N);
  AOD_CHECK_ARG(budget >= 1 && budget <= N - n_labelled, "kcenter_greedy: budget %lld outside 1 .. %lld unselected rows", (long long)budget,
                (long long)(N - n_labelled));
  AOD_CHECK_ARG(desc && picks && radius && mind && ws && (labelled || n_labelled == 0), "kcenter_greedy: null pointer");
  AOD_CHECK_ARG((((size_t)desc) & 15) == 0 && (((size_t)ws) & 7) == 0, "kcenter_greedy: desc must be 16-B aligned, ws 8-B aligned");
  hipStream_t st = (hipStream_t)stream;
  u64* keys[2] = {(u64*)ws, (u64*)ws + KC_MAX_GRID};
  unsigned char* sel = (unsigned char*)ws + (size_t)2 * KC_MAX_GRID * sizeof(u64);
  const int grid = kc_grid(N);
  const int egrid = (int)((N + 255) / 256 > KC_MAX_GRID ? KC_MAX_GRID : (N + 255) / 256);
  hipLaunchKernelGGL(kcenter_prepare_kernel, dim3(egrid), dim3(256), 0, st, mind, sel, (long long)N);
  if (n_labelled > 0) {
    const long long mg = (n_labelled + 255) / 256;
    hipLaunchKernelGGL(kcenter_mark_kernel, dim3((unsigned)(mg > KC_MAX_GRID ? KC_MAX_GRID : mg)), dim3(256), 0, st, (const long long*)labelled,
                       (int)n_labelled, sel, (long long)N);
    for (int64_t c0 = 0; c0 < n_labelled; c0 += KC_CHUNK) {
      const int nc = (int)(n_labelled - c0 < KC_CHUNK ? n_labelled - c0 : KC_CHUNK);
      hipLaunchKernelGGL(kcenter_centers_kernel<METRIC>, dim3(grid), dim3(256), (size_t)KC_CHUNK * D * sizeof(float), st, desc, (long long)N, D,
                         (const long long*)labelled + c0, nc, mind);
    }
  }
  hipLaunchKernelGGL(kcenter_keys_kernel, dim3(egrid), dim3(256), 0, st, (const float*)mind, (const unsigned char*)sel, (long long)N, keys[0]);
  int nkeys = egrid;
  for (int64_t t = 1; t <= budget; ++t) {
    hipLaunchKernelGGL(kcenter_step_kernel<METRIC>, dim3(grid), dim3(256), (size_t)D * sizeof(float), st, desc, (long long)N, D, mind, sel,
                       (const u64*)keys[(t - 1) & 1], nkeys, keys[t & 1], (long long*)picks, radius, (int)t);
    nkeys = grid;
  }
  AOD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ k-center on a matrix
// aod_kcenter_greedy_matrix (CCMS): the same prepare / mark / keys / one-launch-per-pick scheme, tie rule and workspace on a
// precomputed [N][N] distance matrix: the sweeps read dist[p][i] (a thread per row: coalesced along the center's matrix row) instead of
// computing a distance.  A minimum is exact in any order, so nothing here depends on the grid.
__global__ __launch_bounds__(256) void kcenter_matrix_centers_kernel(const float* __restrict__ dist, long long N, const long long* __restrict__ lab,
                                                                     long long n_lab, float* __restrict__ mind) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    float m = mind[i];
    for (long long c = 0; c < n_lab; ++c) {
      const long long ci = lab[c];
      if (ci >= 0 && ci < N) m = fminf(m, dist[ci * N + i]);      // (the caller validates; an index outside the matrix is never dereferenced)
    }
    mind[i] = m;
  }
}

__global__ __launch_bounds__(256) void kcenter_matrix_step_kernel(const float* __restrict__ dist, long long N, float* __restrict__ mind,
                                                                  unsigned char* __restrict__ sel, const u64* __restrict__ keys_in, int nkeys,
                                                                  u64* __restrict__ keys_out, long long* __restrict__ picks,
                                                                  float* __restrict__ radius, int t) {
  __shared__ u64 red[KC_WAVES];
  u64 best = 0;
  for (int j = threadIdx.x; j < nkeys; j += 256) {
    const u64 k = keys_in[j];
    best = k > best ? k : best;
  }
  best = kc_block_max(best, red);
  const unsigned p = ~(unsigned)(best & 0xffffffffull);
  const bool valid = best != 0 && (long long)p < N;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    picks[t - 1] = valid ? (long long)p : -1ll;
    radius[t - 1] = __uint_as_float((unsigned)(best >> 32));
    if (valid) sel[p] = 1;
  }
  if (!valid) {                                                   // workgroup-uniform
    if (threadIdx.x == 0) keys_out[blockIdx.x] = 0;
    return;
  }
  const float* row = dist + (long long)p * N;
  u64 key = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    const float m = fminf(mind[i], row[i]);
    mind[i] = m;
    if (i != (long long)p && !sel[i]) {                            // (workgroup 0 may or may not have set sel[p] yet: p is excluded by name)
      const u64 k = kc_key(m, (unsigned)i);
      key = k > key ? k : key;
    }
  }
  key = kc_block_max(key, red);
  if (threadIdx.x == 0) keys_out[blockIdx.x] = key;
}

extern "C" int aod_kcenter_greedy_matrix(const float* dist, int64_t N, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                                         float* radius, float* mind, void* ws, aod_stream_t stream) {
  AOD_CHECK_ARG(N >= 1 && N <= 0x7fffffffll, "kcenter_greedy_matrix: 1 .. 2^31 - 1 rows (got %lld)", (long long)N);
  AOD_CHECK_ARG(n_labelled >= 0 && n_labelled <= N, "kcenter_greedy_matrix: labelled count %lld outside 0 .. N = %lld", (long long)n_labelled,
                (long long)N);
  AOD_CHECK_ARG(budget >= 1 && budget <= N - n_labelled, "kcenter_greedy_matrix: budget %lld outside 1 .. %lld unselected rows", (long long)budget,
                (long long)(N - n_labelled));
  AOD_CHECK_ARG(dist && picks && radius && mind && ws && (labelled || n_labelled == 0), "kcenter_greedy_matrix: null pointer");
  AOD_CHECK_ARG((((size_t)dist) & 3) == 0 && (((size_t)ws) & 7) == 0, "kcenter_greedy_matrix: dist must be 4-B aligned, ws 8-B aligned");
  hipStream_t st = (hipStream_t)stream;
  u64* keys[2] = {(u64*)ws, (u64*)ws + KC_MAX_GRID};
  unsigned char* sel = (unsigned char*)ws + (size_t)2 * KC_MAX_GRID * sizeof(u64);
  const int egrid = (int)((N + 255) / 256 > KC_MAX_GRID ? KC_MAX_GRID : (N + 255) / 256);
  hipLaunchKernelGGL(kcenter_prepare_kernel, dim3(egrid), dim3(256), 0, st, mind, sel, (long long)N);
  if (n_labelled > 0) {
    const long long mg = (n_labelled + 255) / 256;
    hipLaunchKernelGGL(kcenter_mark_kernel, dim3((unsigned)(mg > KC_MAX_GRID ? KC_MAX_GRID : mg)), dim3(256), 0, st, (const long long*)labelled,
                       (int)n_labelled, sel, (long long)N);
    hipLaunchKernelGGL(kcenter_matrix_centers_kernel, dim3(egrid), dim3(256), 0, st, dist, (long long)N, (const long long*)labelled,
                       (long long)n_labelled, mind);
  }
  hipLaunchKernelGGL(kcenter_keys_kernel, dim3(egrid), dim3(256), 0, st, (const float*)mind, (const unsigned char*)sel, (long long)N, keys[0]);
  for (int64_t t = 1; t <= budget; ++t)
    hipLaunchKernelGGL(kcenter_matrix_step_kernel, dim3(egrid), dim3(256), 0, st, dist, (long long)N, mind, sel, (const u64*)keys[(t - 1) & 1], egrid,
                       keys[t & 1], (long long*)picks, radius, (int)t);
  AOD_LAUNCH_CHECK();
  return 0;
}

// metric 0: the squared Euclidean distance (Core-set); 1: the symmetrised KL divergence of [P | ln P] rows (CDAL)
extern "C" int aod_kcenter_greedy_ex(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget,
                                     int64_t* picks, float* radius, float* mind, void* ws, aod_stream_t stream, int metric) {
  AOD_CHECK_ARG(metric == 0 || metric == 1, "kcenter_greedy: metric %d (0: squared Euclidean, 1: symmetrised KL)", metric);
  if (metric == 0) return kc_greedy<0>(desc, N, D, labelled, n_labelled, budget, picks, radius, mind, ws, stream);
  AOD_CHECK_ARG(D < 1 || D > KC_MAX_D || (D & 1) == 0, "kcenter_greedy: the symmetrised KL metric reads a row as two halves [P | ln P]: D = %d is odd", D);
  return kc_greedy<1>(desc, N, D, labelled, n_labelled, budget, picks, radius, mind, ws, stream);
}

extern "C" int aod_kcenter_greedy(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                                  float* radius, float* mind, void* ws, aod_stream_t stream) {
  return aod_kcenter_greedy_ex(desc, N, D, labelled, n_labelled, budget, picks, radius, mind, ws, stream, 0);
}
