// k-means++ D^2 seeding on the device (D. Arthur, S. Vassilvitskii, "k-means++: The Advantages of Careful Seeding", SODA 2007), the selection
// step of BADGE (J. T. Ash, C. Zhang, A. Krishnamurthy, J. Langford, A. Agarwal, "Deep Batch Active Learning by Diverse, Uncertain Gradient
// Lower Bounds", ICLR 2020).  The reference tree has none: the semantics are fixed in DESIGN 3t.
//
// The structure of the k-center loop (kcenter.hip) with a sampling step where that one has an arg-max: everything is enqueued on
// the caller's stream, one launch per pick, the pick travels through device memory; no host sync, no atomics, no cross-workgroup wait, no
// loop whose trip count depends on data.
//      kmeanspp_prepare_kernel  state = 0 (eligible)
//      kmeanspp_mark_kernel     state[excluded] = 1: excluded rows are never picked and are NOT centres
//      kmeanspp_norms_kernel    mind = +inf; per-workgroup partial of max over eligible i of key(i) = (bits(|x_i|^2) << 32) | ~i
//      kmeanspp_step_kernel<1>  pick 0 = the eligible row with the largest norm (the lowest index on a tie), then the sweep below
//      kmeanspp_step_kernel<0>  ONE launch per pick t >= 1.  Rows are dealt to workgroups in whole blocks of KPP_BLOCK consecutive rows; the
//                               launch before left per block b: S_b (fp64 sum of w_i in row order; w_i = mind[i] for an eligible row, else 0),
//                               the first and the last row with w_i > 0 and the first eligible row.  Every workgroup, redundantly (fixed
//                               association, so every workgroup finds the same pick):
//                                 1. T = S_0 + S_1 + ... in block order (one thread, fp64); T == 0: the pick is the lowest eligible row
//                                 2. target = draws[t] * T; P_b = the sum of the blocks before b.  The pick is the first row with w_i > 0
//                                    whose running sum ((P_b + w_..) + w_i), rows of its block in order, exceeds target.  A thread per block:
//                                    P_b > target -> its first row with w > 0; (P_b + S_b)(1 + 2^-40) <= target -> none (the running sum of
//                                    the block's last row is within 70 * 2^-53 relative of P_b + S_b); else the thread adds the block's
//                                    KPP_BLOCK rows itself.  The minimum of the candidates is the pick; none (draws[t] * T rounded up to T):
//                                    the last row with w_i > 0.
//                               The pick phase reads the launch before's w rows and partials only -- never mind or state, which the sweeps
//                               of this launch rewrite while a slower workgroup may still be looking for the pick.
//                               workgroup 0 records pick, weight = w[pick], total = T, state[pick] = 2, mind[pick] = 0; then every workgroup
//                               sweeps its blocks against the pick -- one wave per row, kc_dists<1, 0> (kc_dist.h: the k-center pair
//                               arithmetic; the centre is read from global memory, one row resident in L2: a row of 32 768 fp32 does not
//                               fit 64 KB of LDS) -- lowers mind and writes the new w rows and block partials into the OTHER of two buffers.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "common.h"
#include "kc_dist.h"

#define KPP_BLOCK 32          // rows per block (aod_kmeanspp_block): the unit of the fp64 sums and of the deal of rows to workgroups
#define KPP_MAX_D 32768
#define KPP_MAX_N (1ll << 24) // every workgroup scans N / KPP_BLOCK block sums per pick
#define KPP_MAX_GRID 1024
#define KPP_SCAN 256          // block sums per scan chunk: one per thread
#define KPP_GUARD 0x1p-40

struct KppPart {              // per row: w; per block: S, first / last row with w > 0 (-1: none), first eligible row (-1: none)
  float* w;
  double* S;
  int* fpos;
  int* lpos;
  int* felig;
};

// |x|^2 = d(x, 0) in kc_dists' arithmetic: the same lane ownership, four running sums and butterfly; (v - 0) * (v - 0) = v * v bit for bit
__device__ __forceinline__ float kpp_norm(const float* __restrict__ x, int D, int lane) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if ((D & 3) == 0) {
    for (int k = 4 * lane; k < D; k += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + k);
      s0 += v[0] * v[0];
      s1 += v[1] * v[1];
      s2 += v[2] * v[2];
      s3 += v[3] * v[3];
    }
  } else {
    for (int k = lane; k < D; k += 64) {
      const float v = x[k];
      s0 += v * v;
    }
  }
  return wave_sum((s0 + s1) + (s2 + s3));
}

__global__ __launch_bounds__(256) void kmeanspp_prepare_kernel(unsigned char* __restrict__ state, long long N) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < N; i += 256ll * gridDim.x) state[i] = 0;
}

__global__ __launch_bounds__(256) void kmeanspp_mark_kernel(const long long* __restrict__ excl, long long n_excl, unsigned char* __restrict__ state,
                                                            long long N) {
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < n_excl; j += 256ll * gridDim.x) {
    const long long c = excl[j];
    if (c >= 0 && c < N) state[c] = 1;                             // (the caller validates; an index outside the matrix is never dereferenced)
  }
}

__global__ __launch_bounds__(256) void kmeanspp_norms_kernel(const float* __restrict__ desc, long long N, int D, long long NB,
                                                             const unsigned char* __restrict__ state, float* __restrict__ mind,
                                                             u64* __restrict__ keys_out) {
  __shared__ u64 red[KC_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 key = 0;
  for (long long b = blockIdx.x; b < NB; b += gridDim.x) {
    for (int r = wave; r < KPP_BLOCK; r += KC_WAVES) {
      const long long i = b * KPP_BLOCK + r;
      if (i < N) {                                                 // wave-uniform
        const float nrm = kpp_norm(desc + i * D, D, lane);
        if (lane == 0) {
          mind[i] = __uint_as_float(0x7f800000u);
          if (state[i] == 0) {
            const u64 k = kc_key(nrm, (unsigned)i);
            key = k > key ? k : key;
          }
        }
      }
    }
  }
  key = kc_block_max(key, red);
  if (threadIdx.x == 0) keys_out[blockIdx.x] = key;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void kmeanspp_step_kernel(const float* __restrict__ desc, long long N, int D, long long NB, float* __restrict__ mind,
                                                            unsigned char* __restrict__ state, const u64* __restrict__ keys_in, int nkeys,
                                                            const KppPart in, const KppPart out, const double* __restrict__ draws,
                                                            long long* __restrict__ picks, float* __restrict__ weight,
                                                            double* __restrict__ total, int t) {
  __shared__ u64 red[KC_WAVES];
  __shared__ double sS[KPP_SCAN], sP[KPP_SCAN];
  __shared__ double sT;
  __shared__ float sw[KPP_BLOCK];
  __shared__ unsigned char se[KPP_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long p = -1;
  float wgt = 0.f;
  double T = 0.0;
  if constexpr (FIRST) {
    u64 best = 0;
    for (int j = tid; j < nkeys; j += 256) {
      const u64 k = keys_in[j];
      best = k > best ? k : best;
    }
    best = kc_block_max(best, red);
    if (best != 0) p = (long long)(~(unsigned)(best & 0xffffffffull));
    wgt = __uint_as_float((unsigned)(best >> 32));
  } else {
    // 1. T in block order; the lowest eligible row and the last row with w > 0 on the way (keys: ~row resp. row + 1; 0: none)
    u64 kfe = 0, klp = 0;
    double run = 0.0;
    for (long long c0 = 0; c0 < NB; c0 += KPP_SCAN) {
      const long long b = c0 + tid;
      double s = 0.0;
      if (b < NB) {
        s = in.S[b];
        const int fe = in.felig[b], lp = in.lpos[b];
        if (fe >= 0) { const u64 k = (u64)(~(unsigned)fe); kfe = k > kfe ? k : kfe; }
        if (lp >= 0) { const u64 k = (u64)(unsigned)lp + 1; klp = k > klp ? k : klp; }
      }
      sS[tid] = s;
      __syncthreads();
      if (tid == 0) {
        const int n = NB - c0 < KPP_SCAN ? (int)(NB - c0) : KPP_SCAN;
#pragma unroll 8
        for (int j = 0; j < n; ++j) run += sS[j];
      }
      __syncthreads();
    }
    if (tid == 0) sT = run;
    kfe = kc_block_max(kfe, red);                                  // (its barriers also publish sT)
    klp = kc_block_max(klp, red);
    T = sT;
    if (T > 0.0) {                                                 // workgroup-uniform
      // 2. the first row with w > 0 whose running sum exceeds target
      const double target = draws[t] * T;
      u64 kc = 0;
      run = 0.0;
      for (long long c0 = 0; c0 < NB; c0 += KPP_SCAN) {
        const long long b = c0 + tid;
        const double s = b < NB ? in.S[b] : 0.0;
        sS[tid] = s;
        __syncthreads();
        if (tid == 0) {
          const int n = NB - c0 < KPP_SCAN ? (int)(NB - c0) : KPP_SCAN;
#pragma unroll 8
          for (int j = 0; j < n; ++j) {
            sP[j] = run;
            run += sS[j];
          }
        }
        __syncthreads();
        if (b < NB && s > 0.0) {
          const double P = sP[tid];
          int cand = -1;
          if (P > target) {
            cand = in.fpos[b];
          } else if ((P + s) * (1.0 + KPP_GUARD) > target) {
            double r = P;
            for (int j = 0; j < KPP_BLOCK; ++j) {
              const long long i = b * KPP_BLOCK + j;
              const float w = i < N ? in.w[i] : 0.f;
              if (w > 0.f) {
                r += (double)w;
                if (cand < 0 && r > target) cand = (int)i;
              }
            }
          }
          if (cand >= 0) { const u64 k = (u64)(~(unsigned)cand); kc = k > kc ? k : kc; }
        }
      }
      kc = kc_block_max(kc, red);
      if (kc != 0) p = (long long)(~(unsigned)kc);
      else if (klp != 0) p = (long long)(klp - 1);
    } else if (kfe != 0) {
      p = (long long)(~(unsigned)kfe);
    }
  }
  const bool valid = p >= 0 && p < N;               // (no candidate: budget exceeds the eligible rows -- refused by the entry)
  if (blockIdx.x == 0 && tid == 0) {
    if (!FIRST && valid) wgt = in.w[p];             // (no sweep of this launch writes in.w, touches mind[p] or reads state[p])
    picks[t] = valid ? p : -1ll;
    weight[t] = wgt;
    total[t] = T;
    if (valid) {
      state[p] = 2;
      mind[p] = 0.f;
    }
  }
  const float* cen = desc + (valid ? p : 0) * D;
  for (long long b = blockIdx.x; b < NB; b += gridDim.x) {
    for (int r = wave; r < KPP_BLOCK; r += KC_WAVES) {
      const long long i = b * KPP_BLOCK + r;
      float w = 0.f;
      unsigned char e = 0;
      if (valid && i < N) {                                        // wave-uniform
        float d[1];
        kc_dists<1, 0>(desc + i * D, cen, D, lane, d);
        if (lane == 0 && i != p) {
          const float m = fminf(mind[i], d[0]);
          mind[i] = m;
          if (state[i] == 0) {
            e = 1;
            w = m;
          }
        }
      }
      if (lane == 0) {
        sw[r] = w;
        se[r] = e;
        if (i < N) out.w[i] = w;
      }
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      int fp = -1, lp = -1, fe = -1;
      for (int r = 0; r < KPP_BLOCK; ++r) {
        if (se[r]) {
          const int i = (int)(b * KPP_BLOCK + r);
          if (fe < 0) fe = i;
          if (sw[r] > 0.f) {
            s += (double)sw[r];
            if (fp < 0) fp = i;
            lp = i;
          }
        }
      }
      out.S[b] = s;
      out.fpos[b] = fp;
      out.lpos[b] = lp;
      out.felig[b] = fe;
    }
    __syncthreads();
  }
}

extern "C" int aod_kmeanspp_block(void) { return KPP_BLOCK; }

static inline size_t kpp_nb(int64_t N) { return (size_t)((N + KPP_BLOCK - 1) / KPP_BLOCK); }
static inline size_t kpp_nbpad(int64_t N) { return (kpp_nb(N) + 1) & ~(size_t)1; }
static inline size_t kpp_npad(int64_t N) { return ((size_t)N + 3) & ~(size_t)3; }

// workspace: KPP_MAX_GRID partial keys, two sets of block partials (an fp64 sum and three int32 rows per block), two sets of row weights
// (fp32), the state byte per row
extern "C" size_t aod_kmeanspp_ws_len(int64_t N) {
  if (N < 1 || N > KPP_MAX_N) return 0;
  return (size_t)KPP_MAX_GRID * sizeof(u64) + 2 * kpp_nbpad(N) * (sizeof(double) + 3 * sizeof(int)) + 2 * kpp_npad(N) * sizeof(float) +
         (((size_t)N + 15) & ~(size_t)15);
}

extern "C" int aod_kmeanspp_seed(const float* desc, int64_t N, int D, const int64_t* excluded, int64_t n_excluded, int64_t budget,
                                 const double* draws, int64_t* picks, float* weight, double* total, float* mind, void* ws, aod_stream_t stream) {
  AOD_CHECK_ARG(N >= 1 && N <= KPP_MAX_N, "kmeanspp_seed: 1 .. 2^24 rows (got %lld)", (long long)N);
  AOD_CHECK_ARG(D >= 1 && D <= KPP_MAX_D, "kmeanspp_seed: 1 .. %d descriptor columns (got %d)", KPP_MAX_D, D);
  AOD_CHECK_ARG(n_excluded >= 0 && n_excluded <= N, "kmeanspp_seed: excluded count %lld outside 0 .. N = %lld", (long long)n_excluded, (long long)N);
  AOD_CHECK_ARG(budget >= 1 && budget <= N - n_excluded, "kmeanspp_seed: budget %lld outside 1 .. %lld eligible rows", (long long)budget,
                (long long)(N - n_excluded));
  AOD_CHECK_ARG(desc && draws && picks && weight && total && mind && ws && (excluded || n_excluded == 0), "kmeanspp_seed: null pointer");
  AOD_CHECK_ARG((((size_t)desc) & 15) == 0 && ((((size_t)ws) | ((size_t)draws) | ((size_t)total) | ((size_t)picks) | ((size_t)excluded)) & 7) == 0 &&
                    ((((size_t)weight) | ((size_t)mind)) & 3) == 0,
                "kmeanspp_seed: desc must be 16-B aligned, ws / draws / total / picks / excluded 8-B aligned, weight / mind 4-B aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long NB = (long long)kpp_nb(N);
  const size_t nbp = kpp_nbpad(N);
  u64* keys = (u64*)ws;
  double* S = (double*)(keys + KPP_MAX_GRID);
  int* rows = (int*)(S + 2 * nbp);
  float* wrow = (float*)(rows + 6 * nbp);
  unsigned char* state = (unsigned char*)(wrow + 2 * kpp_npad(N));
  KppPart part[2];
  for (int h = 0; h < 2; ++h) {
    part[h].w = wrow + h * kpp_npad(N);
    part[h].S = S + h * nbp;
    part[h].fpos = rows + (3 * h + 0) * nbp;
    part[h].lpos = rows + (3 * h + 1) * nbp;
    part[h].felig = rows + (3 * h + 2) * nbp;
  }
  const int grid = (int)(NB > KPP_MAX_GRID ? KPP_MAX_GRID : NB);
  const int egrid = (int)((N + 255) / 256 > KPP_MAX_GRID ? KPP_MAX_GRID : (N + 255) / 256);
  hipLaunchKernelGGL(kmeanspp_prepare_kernel, dim3(egrid), dim3(256), 0, st, state, (long long)N);
  if (n_excluded > 0) {
    const int mgrid = (int)((n_excluded + 255) / 256 > KPP_MAX_GRID ? KPP_MAX_GRID : (n_excluded + 255) / 256);
    hipLaunchKernelGGL(kmeanspp_mark_kernel, dim3(mgrid), dim3(256), 0, st, (const long long*)excluded, (long long)n_excluded, state, (long long)N);
  }
  hipLaunchKernelGGL(kmeanspp_norms_kernel, dim3(grid), dim3(256), 0, st, desc, (long long)N, D, NB, (const unsigned char*)state, mind, keys);
  hipLaunchKernelGGL(kmeanspp_step_kernel<true>, dim3(grid), dim3(256), 0, st, desc, (long long)N, D, NB, mind, state, (const u64*)keys, grid, part[1],
                     part[0], draws, (long long*)picks, weight, total, 0);
  for (int64_t t = 1; t < budget; ++t)
    hipLaunchKernelGGL(kmeanspp_step_kernel<false>, dim3(grid), dim3(256), 0, st, desc, (long long)N, D, NB, mind, state, (const u64*)keys, 0,
                       part[(t - 1) & 1], part[t & 1], draws, (long long*)picks, weight, total, (int)t);
  AOD_LAUNCH_CHECK();
  return 0;
}
