// k-center greedy (O. Sener, S. Savarese, "Active Learning for Convolutional Neural Networks: A Core-Set Approach", ICLR 2018, Algorithm 1)
// under the diversity pools: Core-set, CDAL (3j) and CCMS (3o).  The reference tree has none: the semantics are fixed there.
//
// Everything on the device, no host sync and no cross-workgroup wait inside a launch:
//      kcenter_prepare_kernel   mind = +inf, selected = 0
//      kcenter_mark_kernel      selected[labelled] = 1
//      the path's centers       mind[i] = min(mind[i], min_c d(i, c)) over the labelled centers c
//      kcenter_keys_kernel      per-workgroup partial of max over unselected i of key(i) = (bits(mind[i]) << 32) | ~i
//      kcenter_step_kernel      ONE launch per pick: every workgroup reduces the previous launch's partials (redundantly: an unsigned max is
//                               exact, so every workgroup finds the same pick), workgroup 0 records pick / radius / selected, then the
//                               workgroup sweeps its rows against the picked center and writes its partial into the other partial buffer.
// Non-negative floats order like their bit patterns as unsigned integers (+inf included) and ~i makes the LOWEST index win a tie.
// A path (KcRows<METRIC>, KcMatrix) says how mind is lowered against a center; the pick protocol and the host sequence are written once.
//    rows (aod_kcenter_greedy, aod_kcenter_greedy_ex) on desc [N][D] fp32: d(i, c) = sum_k (x_ik - x_ck)^2 in the direct form; ONE wave per
//      row, lane j owns the elements 4j + 256m (+0..3) (D % 4 == 0; else j + 64m), four running sums per lane, ((s0 + s1) + (s2 + s3)), xor
//      butterfly: a function of the two rows and D alone.  The centers are staged in LDS, KC_CHUNK labelled centers per launch.
//      metric = 1: the same kernels instantiated for the symmetrised KL divergence of [P | ln P] rows (CDAL; kc_dists).
//    matrix (aod_kcenter_greedy_matrix, CCMS) on a precomputed dist [N][N] fp32: the sweeps read dist[p][i] (a thread per row: coalesced
//      along the center's matrix row) instead of computing a distance.  A minimum is exact in any order, so nothing depends on the grid.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "common.h"
#include "kc_dist.h"           // kc_key, kc_block_max, kc_dists: shared with kmeanspp.hip

#define KC_CHUNK 8           // labelled centers per initialisation launch (aod_kcenter_chunk)
#define KC_MAX_D 2048        // KC_CHUNK * KC_MAX_D * 4 B = 64 KB of LDS
#define KC_MAX_GRID 1024     // workgroups (= partial keys) of a sweep

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

static inline int kc_egrid(long long n) { return (int)((n + 255) / 256 > KC_MAX_GRID ? KC_MAX_GRID : (n + 255) / 256); }

// ------------------------------------------------------------------------------------------------------------------ the two paths
// A path: sweep(x, N, D, p, lower) folds key = lower(i, d(i, p), key) from 0 over every row i the workgroup owns, each row in one thread,
// and returns that thread's key; grid / lds: the geometry of a step launch; centers: the launches that lower mind against the labelled
// centers; check_dims / check_align: the path's own argument checks, called at their place among the common ones (kc_greedy) so that
// the checks fire in the order they always did.
template <int METRIC>
struct KcRows {                                                    // x = desc [N][D]; the center staged in dynamic LDS, one wave per row
  static constexpr const char* name = "kcenter_greedy";
  template <class F>
  static __device__ __forceinline__ u64 sweep(const float* __restrict__ desc, long long N, int D, unsigned p, F lower) {
    extern __shared__ __align__(16) float cen[];                   // [D]
    for (int k = threadIdx.x; k < D; k += 256) cen[k] = desc[(long long)p * D + k];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long wave = blockIdx.x * (long long)KC_WAVES + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * KC_WAVES;
    u64 key = 0;
    for (long long i = wave; i < N; i += nwaves) {
      float d[1];
      kc_dists<1, METRIC>(desc + i * D, cen, D, lane, d);
      if (lane == 0) key = lower(i, d[0], key);
    }
    return key;
  }
  static int grid(long long N) {
    long long g = (N + KC_WAVES - 1) / KC_WAVES;
    return (int)(g > KC_MAX_GRID ? KC_MAX_GRID : (g < 1 ? 1 : g));
  }
  static size_t lds(int D) { return (size_t)D * sizeof(float); }
  static void centers(const float* desc, long long N, int D, const long long* lab, int64_t n_lab, float* mind, hipStream_t st) {
    for (int64_t c0 = 0; c0 < n_lab; c0 += KC_CHUNK) {
      const int nc = (int)(n_lab - c0 < KC_CHUNK ? n_lab - c0 : KC_CHUNK);
      hipLaunchKernelGGL(kcenter_centers_kernel<METRIC>, dim3(grid(N)), dim3(256), (size_t)KC_CHUNK * D * sizeof(float), st, desc, N, D, lab + c0,
                         nc, mind);
    }
  }
  static int check_dims(int D) {
    AOD_CHECK_ARG(D >= 1 && D <= KC_MAX_D, "kcenter_greedy: 1 .. %d descriptor columns (got %d)", KC_MAX_D, D);
    return 0;
  }
  static int check_align(const float* desc, const void* ws) {
    AOD_CHECK_ARG((((size_t)desc) & 15) == 0 && (((size_t)ws) & 7) == 0, "kcenter_greedy: desc must be 16-B aligned, ws 8-B aligned");
    return 0;
  }
};

struct KcMatrix {                                                  // x = dist [N][N]; a thread per row reads dist[p][i]
  static constexpr const char* name = "kcenter_greedy_matrix";
  template <class F>
  static __device__ __forceinline__ u64 sweep(const float* __restrict__ dist, long long N, int, unsigned p, F lower) {
    const float* row = dist + (long long)p * N;
    u64 key = 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < N; i += 256ll * gridDim.x) key = lower(i, row[i], key);
    return key;
  }
  static int grid(long long N) { return kc_egrid(N); }
  static size_t lds(int) { return 0; }
  static void centers(const float* dist, long long N, int, const long long* lab, int64_t n_lab, float* mind, hipStream_t st) {
    hipLaunchKernelGGL(kcenter_matrix_centers_kernel, dim3(kc_egrid(N)), dim3(256), 0, st, dist, N, lab, (long long)n_lab, mind);
  }
  static int check_dims(int) { return 0; }
  static int check_align(const float* dist, const void* ws) {
    AOD_CHECK_ARG((((size_t)dist) & 3) == 0 && (((size_t)ws) & 7) == 0, "kcenter_greedy_matrix: dist must be 4-B aligned, ws 8-B aligned");
    return 0;
  }
};

// ------------------------------------------------------------------------------------------------------------------ the pick protocol
// launch t = 1 .. budget: pick t - 1 (0-based) comes out of keys_in, is recorded, and every mind takes the distance to it
template <class PATH>
__global__ __launch_bounds__(256) void kcenter_step_kernel(const float* __restrict__ x, long long N, int D, float* __restrict__ mind,
                                                           unsigned char* __restrict__ sel, const u64* __restrict__ keys_in, int nkeys,
                                                           u64* __restrict__ keys_out, long long* __restrict__ picks, float* __restrict__ radius,
                                                           int t) {
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
  u64 key = PATH::sweep(x, N, D, p, [=](long long i, float d, u64 key) {
    const float m = fminf(mind[i], d);
    mind[i] = m;
    if (i != (long long)p && !sel[i]) {                            // (workgroup 0 may or may not have set sel[p] yet: p is excluded by name)
      const u64 k = kc_key(m, (unsigned)i);
      key = k > key ? k : key;
    }
    return key;
  });
  key = kc_block_max(key, red);
  if (threadIdx.x == 0) keys_out[blockIdx.x] = key;
}

extern "C" int aod_kcenter_chunk(void) { return KC_CHUNK; }

// workspace: two partial-key buffers of KC_MAX_GRID 64-bit words, then the selected mask (one byte per row)
extern "C" size_t aod_kcenter_ws_len(int64_t N) {
  if (N < 1 || N > 0x7fffffffll) return 0;
  return (size_t)2 * KC_MAX_GRID * sizeof(u64) + (((size_t)N + 15) & ~(size_t)15);
}

// ------------------------------------------------------------------------------------------------------------------ the host sequence
template <class PATH>
static int kc_greedy(const float* x, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks, float* radius,
                     float* mind, void* ws, aod_stream_t stream) {
  AOD_CHECK_ARG(N >= 1 && N <= 0x7fffffffll, "%s: 1 .. 2^31 - 1 rows (got %lld)", PATH::name, (long long)N);
  if (PATH::check_dims(D)) return -1;
  AOD_CHECK_ARG(n_labelled >= 0 && n_labelled <= N, "%s: labelled count %lld outside 0 .. N = %lld", PATH::name, (long long)n_labelled, (long long)N);
  AOD_CHECK_ARG(budget >= 1 && budget <= N - n_labelled, "%s: budget %lld outside 1 .. %lld unselected rows", PATH::name, (long long)budget,
                (long long)(N - n_labelled));
  AOD_CHECK_ARG(x && picks && radius && mind && ws && (labelled || n_labelled == 0), "%s: null pointer", PATH::name);
  if (PATH::check_align(x, ws)) return -1;
  hipStream_t st = (hipStream_t)stream;
  u64* keys[2] = {(u64*)ws, (u64*)ws + KC_MAX_GRID};
  unsigned char* sel = (unsigned char*)ws + (size_t)2 * KC_MAX_GRID * sizeof(u64);
  const int grid = PATH::grid(N), egrid = kc_egrid(N);
  hipLaunchKernelGGL(kcenter_prepare_kernel, dim3(egrid), dim3(256), 0, st, mind, sel, (long long)N);
  if (n_labelled > 0) {
    hipLaunchKernelGGL(kcenter_mark_kernel, dim3(kc_egrid(n_labelled)), dim3(256), 0, st, (const long long*)labelled, (int)n_labelled, sel,
                       (long long)N);
    PATH::centers(x, (long long)N, D, (const long long*)labelled, n_labelled, mind, st);
  }
  hipLaunchKernelGGL(kcenter_keys_kernel, dim3(egrid), dim3(256), 0, st, (const float*)mind, (const unsigned char*)sel, (long long)N, keys[0]);
  int nkeys = egrid;
  for (int64_t t = 1; t <= budget; ++t) {
    hipLaunchKernelGGL(kcenter_step_kernel<PATH>, dim3(grid), dim3(256), PATH::lds(D), st, x, (long long)N, D, mind, sel,
                       (const u64*)keys[(t - 1) & 1], nkeys, keys[t & 1], (long long*)picks, radius, (int)t);
    nkeys = grid;
  }
  AOD_LAUNCH_CHECK();
  return 0;
}

extern "C" int aod_kcenter_greedy_matrix(const float* dist, int64_t N, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                                         float* radius, float* mind, void* ws, aod_stream_t stream) {
  return kc_greedy<KcMatrix>(dist, N, 0, labelled, n_labelled, budget, picks, radius, mind, ws, stream);
}

// metric 0: the squared Euclidean distance (Core-set); 1: the symmetrised KL divergence of [P | ln P] rows (CDAL)
extern "C" int aod_kcenter_greedy_ex(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget,
                                     int64_t* picks, float* radius, float* mind, void* ws, aod_stream_t stream, int metric) {
  AOD_CHECK_ARG(metric == 0 || metric == 1, "kcenter_greedy: metric %d (0: squared Euclidean, 1: symmetrised KL)", metric);
  if (metric == 0) return kc_greedy<KcRows<0>>(desc, N, D, labelled, n_labelled, budget, picks, radius, mind, ws, stream);
  AOD_CHECK_ARG(D < 1 || D > KC_MAX_D || (D & 1) == 0, "kcenter_greedy: the symmetrised KL metric reads a row as two halves [P | ln P]: D = %d is odd", D);
  return kc_greedy<KcRows<1>>(desc, N, D, labelled, n_labelled, budget, picks, radius, mind, ws, stream);
}

extern "C" int aod_kcenter_greedy(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                                  float* radius, float* mind, void* ws, aod_stream_t stream) {
  return aod_kcenter_greedy_ex(desc, N, D, labelled, n_labelled, budget, picks, radius, mind, ws, stream, 0);
}
