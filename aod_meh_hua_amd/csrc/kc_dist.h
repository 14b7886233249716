// The pair arithmetic and the 64-bit key reductions of the order-dependent selection loops: k-center greedy (kcenter.hip)
// and k-means++ seeding (kmeanspp.hip).  One definition, so that a pair of rows has the same distance bits in both.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

#define KC_WAVES 4           // waves of a 256-thread workgroup

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

// distances of row x to NC centers at cen[c * D + k] (LDS in kcenter.hip, global memory in kmeanspp.hip); every lane returns all NC values.
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
