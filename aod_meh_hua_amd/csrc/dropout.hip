// MC-dropout baseline (mmdet/apis/CalMCDropoutUnc.py:137-163 with utils/functions.py:492-505): one train-mode Dropout2d(rate) behind every
// ReLU of an eval-mode network, n stochastic forwards per image.  Dropout2d draws one Bernoulli per (image, channel) and multiplies the whole
// plane by 0 or 1 / (1 - rate).  Two kernels, both outside the conv kernels:
//   dropout2d_masks_kernel   the factors of EVERY site of one forward, a dense fp32 table [B][T] (T = sum of the sites' channel counts)
//   dropout2d_apply_kernel   activation rows *= their image's factors, in place, behind a conv whose epilogue applied the ReLU
// The stream is this library's, not torch's generator (which cannot be restated): Philox4x32-10 at
//     counter (c >> 2, site, sample, (uint32) image id),   key (seed_lo ^ DROP_KEY_TAG, seed_hi),   seed_lo / seed_hi = the halves of `seed`
// word c & 3 of the block, u = u01(word) in (0, 1], factor = u > rate ? 1 / (1 - rate) : 0  (fp32; rate = 0: u > 0 always, factor 1).
// The tag keeps the stream apart from the HUA sampler's, whose key is (seed_lo, seed_hi) itself.  A factor is a function of (seed, sample,
// image id, site, channel) only: not of the batch, the image's position in it, the rank or eager / replayed execution.
#include "tile_prims.h"

#define DROP_KEY_TAG 0x44524F50u        // 'DROP'
#define DROP_MAX_SEG 8

// ---------------------------------------------------------------- the factor table of one forward
// grid (1, n_sites, B), one wave per (site, image): lane t produces the quads t, t + 64, ... of the site -- one Philox call = four channels
__global__ __launch_bounds__(64) void dropout2d_masks_kernel(float* __restrict__ table, const long long* __restrict__ image_ids,
                                                             const int* __restrict__ site_offsets, int n_sites, int T, float rate, float keep_scale,
                                                             unsigned k0, unsigned k1, unsigned sample) {
  const int s = blockIdx.y, b = blockIdx.z;
  const int off = site_offsets[s];
  const int end = s + 1 < n_sites ? site_offsets[s + 1] : T;
  if (off < 0 || end > T || end <= off) return;              // (a malformed offset list writes nothing rather than out of the table)
  const int Cs = end - off;
  const unsigned img = (unsigned)image_ids[b];
  float* row = table + (long long)b * T + off;
  const bool vec = ((reinterpret_cast<unsigned long long>(row)) & 15ull) == 0;
  for (int q = threadIdx.x; 4 * q < Cs; q += 64) {
    unsigned r[4];
    philox4x32_10((unsigned)q, (unsigned)s, sample, img, k0, k1, r);
    f32x4 f;
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = u01(r[j]) > rate ? keep_scale : 0.0f;
    if (vec && 4 * q + 3 < Cs) {
      *reinterpret_cast<f32x4*>(row + 4 * q) = f;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < Cs) row[4 * q + j] = f[j];
    }
  }
}

extern "C" int aod_dropout2d_masks(float* table, const int64_t* image_ids, int B, const int32_t* site_offsets, int n_sites, int T, float rate,
                                   uint64_t seed, uint32_t sample, aod_stream_t stream) {
  AOD_CHECK_ARG(table && image_ids && site_offsets, "dropout2d_masks: null pointer");
  AOD_CHECK_ARG(B >= 1 && B <= 65535, "dropout2d_masks: batch must be 1..65535 (got %d)", B);
  AOD_CHECK_ARG(n_sites >= 1 && n_sites <= 65535, "dropout2d_masks: 1..65535 sites (got %d)", n_sites);
  AOD_CHECK_ARG(T >= n_sites, "dropout2d_masks: table width %d is smaller than the number of sites %d", T, n_sites);
  AOD_CHECK_ARG(rate >= 0.0f && rate < 1.0f, "dropout2d_masks: rate must be in [0, 1) (got %g)", (double)rate);
  const float keep_scale = 1.0f / (1.0f - rate);
  const unsigned k0 = (unsigned)(seed & 0xffffffffull) ^ DROP_KEY_TAG, k1 = (unsigned)(seed >> 32);
  hipLaunchKernelGGL(dropout2d_masks_kernel, dim3(1, (unsigned)n_sites, (unsigned)B), dim3(64), 0, (hipStream_t)stream, table,
                     (const long long*)image_ids, (const int*)site_offsets, n_sites, T, rate, keep_scale, k0, k1, (unsigned)sample);
  AOD_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- rows *= factors, in place
// Up to 8 row segments of ONE buffer in one launch (the tower outputs of one depth: one segment per pyramid level, each with its own site):
// the segments travel as kernel arguments.  A work item is one 16-B piece of a row (plain bf16: 8 channels) or one octet (X-layout: 8
// channels = head piece + tail piece); consecutive lanes take consecutive pieces of a row.
struct DropSegs {
  long long row0[DROP_MAX_SEG];       // first row of the segment in the buffer
  long long cum[DROP_MAX_SEG + 1];    // rows of the segments in front (dense work-item numbering)
  int hw[DROP_MAX_SEG];               // rows per image
  int off[DROP_MAX_SEG];              // the segment's first column of the table
  int n;
};

template <bool X3>
__global__ __launch_bounds__(256) void dropout2d_apply_kernel(bf16_t* __restrict__ x, const float* __restrict__ table, long long stride_T,
                                                              const DropSegs sg, int C, int P, int CP) {
  const long long n = sg.cum[sg.n] * P;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(i % P);
    const long long r = i / P;
    int s = 0;
#pragma unroll
    for (int k = 1; k < DROP_MAX_SEG; ++k)
      if (k < sg.n && r >= sg.cum[k]) s = k;
    const long long local = r - sg.cum[s];
    const long long b = local / sg.hw[s];
    const float* f = table + b * stride_T + sg.off[s] + 8 * p;
    float fac[8];
    if (8 * p + 7 < C && (reinterpret_cast<unsigned long long>(f) & 15ull) == 0) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(f), c = *reinterpret_cast<const f32x4*>(f + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { fac[j] = a[j]; fac[4 + j] = c[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) fac[j] = 8 * p + j < C ? f[j] : 1.0f;       // (pad channels of an X row hold zeros and keep them)
    }
    bf16_t* px = x + (sg.row0[s] + local) * CP + (X3 ? xoct(p) : 8 * p);
    if (X3) {
      // XRows::load / multiply / XRows::store of row_layout.h on one octet, by hand.  A factor of exactly 1 keeps the element's (head, tail)
      // bits: re-splitting h + l is not idempotent (a tail that rounded up to half an ulp of its head makes h + l a bf16 tie, which may pick
      // the other head)
      bf16x8 h = *reinterpret_cast<const bf16x8*>(px), l = *reinterpret_cast<const bf16x8*>(px + 32);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float w = ((float)h[j] + (float)l[j]) * fac[j];
        const bf16_t nh = (bf16_t)w, nl = (bf16_t)(w - (float)nh);
        if (fac[j] != 1.0f) { h[j] = nh; l[j] = nl; }
      }
      *reinterpret_cast<bf16x8*>(px) = h;
      *reinterpret_cast<bf16x8*>(px + 32) = l;
    } else {
      bf16x8 h = *reinterpret_cast<const bf16x8*>(px);
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = (bf16_t)((float)h[j] * fac[j]);
      *reinterpret_cast<bf16x8*>(px) = h;
    }
  }
}

extern "C" int aod_dropout2d_apply_multi(void* x, const float* table, int64_t row_stride_T, int B, int nseg, const int64_t* seg_row0,
                                         const int32_t* seg_hw, const int32_t* seg_off, int C, int x3, aod_stream_t stream) {
  AOD_CHECK_ARG(x && table && seg_row0 && seg_hw && seg_off, "dropout2d_apply: null pointer");
  AOD_CHECK_ARG((((size_t)x) & 15) == 0, "dropout2d_apply: activation rows must be 16-B aligned");
  AOD_CHECK_ARG((((size_t)table) & 3) == 0, "dropout2d_apply: table pointer not 4-B aligned");
  AOD_CHECK_ARG(B >= 1, "dropout2d_apply: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(nseg >= 1 && nseg <= DROP_MAX_SEG, "dropout2d_apply: 1..8 segments (got %d)", nseg);
  AOD_CHECK_ARG(C >= 1, "dropout2d_apply: channels must be positive (got %d)", C);
  AOD_CHECK_ARG(x3 || C % 8 == 0, "dropout2d_apply: plain bf16 rows need a multiple of 8 channels (got %d)", C);
  DropSegs sg;
  memset(&sg, 0, sizeof(sg));
  sg.n = nseg;
  for (int s = 0; s < nseg; ++s) {
    AOD_CHECK_ARG(seg_row0[s] >= 0 && seg_hw[s] >= 1, "dropout2d_apply: segment %d has first row %lld and %d rows per image", s,
                  (long long)seg_row0[s], seg_hw[s]);
    AOD_CHECK_ARG(seg_off[s] >= 0 && (long long)seg_off[s] + C <= row_stride_T,
                  "dropout2d_apply: segment %d reads table columns %d..%d of a row of %lld", s, seg_off[s], seg_off[s] + C, (long long)row_stride_T);
    sg.row0[s] = seg_row0[s];
    sg.hw[s] = seg_hw[s];
    sg.off[s] = seg_off[s];
    sg.cum[s + 1] = sg.cum[s] + (long long)B * seg_hw[s];
  }
  for (int s = nseg; s < DROP_MAX_SEG; ++s) { sg.cum[s + 1] = sg.cum[nseg]; sg.hw[s] = 1; }
  const int Cp = (C + 31) / 32 * 32;
  const int P = x3 ? Cp / 8 : C / 8;              // work items per row
  const int CP = x3 ? 2 * Cp : C;                 // physical row width (bf16 columns)
  const long long items = sg.cum[nseg] * P;
  if (x3)
    hipLaunchKernelGGL(dropout2d_apply_kernel<true>, dim3(grid_for<2048>(items)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, table,
                       (long long)row_stride_T, sg, C, P, CP);
  else
    hipLaunchKernelGGL(dropout2d_apply_kernel<false>, dim3(grid_for<2048>(items)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, table,
                       (long long)row_stride_T, sg, C, P, CP);
  AOD_LAUNCH_CHECK();
  return 0;
}

extern "C" int aod_dropout2d_apply(void* x, const float* table_row0, int64_t row_stride_T, int B, int HW, int C, int x3, aod_stream_t stream) {
  const int64_t row0 = 0;
  const int32_t hw = HW, off = 0;
  AOD_CHECK_ARG(row_stride_T >= C, "dropout2d_apply: table row stride %lld is smaller than the %d channels", (long long)row_stride_T, C);
  return aod_dropout2d_apply_multi(x, table_row0, row_stride_T, B, 1, &row0, &hw, &off, C, x3, stream);
}
