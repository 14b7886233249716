// Core-set acquisition (k-center greedy; O. Sener, S. Savarese, "Active Learning for Convolutional Neural Networks: A Core-Set Approach",
// ICLR 2018, Algorithm 1).  The reference tree has no Core-set: the semantics are fixed in DESIGN 3i.  This file holds the pool descriptor;
// the k-center greedy selection on the descriptors [N][D] is csrc/kcenter.hip.
//
// pool_descriptor_kernel: the descriptor of an image = concatenation over pyramid levels of the global average of the neck output,
// read from the bf16 / X-layout rows as they lie in the pyramid buffer (up to 8 row segments, one launch per batch).  One workgroup per
// (image, level, group of 64 channels): 32 row lanes x 8 octets; row lane r adds rows r, r + 32, r + 64, ... in that order, a fixed
// LDS tree adds the 32 lanes, one division by h * w.  The order of every sum depends on h * w only: an image's descriptor has the same
// bits alone and in any batch.  16-B loads, no atomics.
#include <hip/hip_runtime.h>
#include "../../include/aod_hip.h"
#include "row_layout.h"

#define PD_MAX_SEG 8

struct PdSegs {
  long long row0[PD_MAX_SEG];        // first row of the level (image 0)
  int hw[PD_MAX_SEG];                // rows per image
  int nseg;
};

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
  const int col = row_col(x3, o);
  const bf16_t* p = base + (s.row0[l] + (long long)b * hw) * pitch + col;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (live) {
    int m = r;
    for (; m + 96 < hw; m += 128) {                              // four rows in flight, added in row order
      float v0[8], v1[8], v2[8], v3[8];
      row_load(p + (long long)m * pitch, x3, v0);
      row_load(p + (long long)(m + 32) * pitch, x3, v1);
      row_load(p + (long long)(m + 64) * pitch, x3, v2);
      row_load(p + (long long)(m + 96) * pitch, x3, v3);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = (((acc[j] + v0[j]) + v1[j]) + v2[j]) + v3[j];
    }
    for (; m < hw; m += 32) {
      float v[8];
      row_load(p + (long long)m * pitch, x3, v);
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
