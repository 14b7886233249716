// Localization-stability acquisition: C.-C. Kao, T.-Y. Lee, P. Sen, M.-Y. Liu, "Localization-Aware Active Learning for Object
// Detection", ACCV 2018 (LS and LS+C).  Detect on the clean image, detect again on copies with Gaussian pixel noise of growing strength,
// score the image by how far its boxes move.  The reference tree has no such pool: the semantics are fixed in DESIGN 3m.
//
// aod_pixel_noise     dst = src + (sigma / std_c) z inside img_shape, src's bits outside; z is a pure function of (seed, level, global image
//                     id, channel, y, x): element x & 3 of the four normals of the Philox4x32-10 block with counter
//                       c0 = (y << 16) | (x >> 2), c1 = 0x80000000 | (level << 8) | c, c2 = id & 0xffffffff, c3 = id >> 32
//                     and key (seed & 0xffffffff, seed >> 32).  Bit 31 of c1 keeps the stream apart from the synthetic pool's (its second
//                     counter word is the high half of an element index); z does not depend on B, the image's place in the batch, or Wp.
//                     One thread per 4 consecutive x: a 16-B load, one Philox block, a 16-B store.
// aod_loc_stability   per image b, over the stacked slots (slot 0: the clean detections, slots 1..K: the noisy ones):
//   object      reference row j of slot 0 with j < num[0][b] and dets[0][b][j][4] > score_thr (strict); weight w_j = that score
//   m_{j,k}     max IoU of reference box j over the rows < num[k+1][b] of slot k + 1 (same_class: rows of j's label only); 0 for an empty slot
//               iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih likewise, ov = iw ih, un = area_a + area_b - ov, IoU = ov / max(un, 1e-6)
//   S_j         (m_{j,0} + ... + m_{j,K-1}) / K, the levels added in order;  S_I = sum_j w_j S_j / sum_j w_j over the objects
//   score       ls: 1 - S_I;  ls+c: (1 - S_I) + (1 - max_j w_j);  an image without an object scores 0
// One launch, one workgroup of 256 threads per image, no atomics, no workspace: thread t owns the reference rows t, t + 256, ... in
// registers; per level all threads stage the level's rows in LDS (24 KB), then every owner scans them (all lanes of a wave read the same
// LDS words: broadcasts).  The two sums and the maximum over j run in a pairwise tree over the next power of two >= max_num in LDS -- rows
// that are no object hold 0 -- so their association depends on j and max_num alone: an image has the same score bits alone, at any place
// of any batch, eager or replayed.  Rows >= num of any slot are never read.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/aod_hip.h"
#include "common.h"

#define LS_TB 256
#define LS_MAX_DET 1024
#define LS_ROWS (LS_MAX_DET / LS_TB)
#define LS_MAX_LEVELS 16

struct ls_inv_std { float v[4]; };

__global__ __launch_bounds__(256) void pixel_noise_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int Hp, int W4,
                                                          const int* __restrict__ hw, ls_inv_std inv_std, float sigma, unsigned level,
                                                          unsigned k0, unsigned k1, const long long* __restrict__ ids) {
  const int c = blockIdx.y, b = blockIdx.z;
  const unsigned id_lo = (unsigned)ids[b], id_hi = (unsigned)((unsigned long long)ids[b] >> 32);
  int h = hw[2 * b], w = hw[2 * b + 1];
  h = h < 0 ? 0 : (h > Hp ? Hp : h);
  w = w < 0 ? 0 : (w > 4 * W4 ? 4 * W4 : w);
  const float scale = sigma * inv_std.v[c];
  if (scale == 0.f) h = 0;                                   // sigma = 0: a copy (x + 0 z would turn a -0 into +0)
  const long long per4 = (long long)Hp * W4, base = ((long long)b * C + c) * per4;
  const unsigned c1 = 0x80000000u | (level << 8) | (unsigned)c;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per4; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / W4), xq = (int)(i - (long long)y * W4);
    f32x4 v = *reinterpret_cast<const f32x4*>(src + (base + i) * 4);
    if (y < h && 4 * xq < w) {
      unsigned r[4];
      philox4x32_10(((unsigned)y << 16) | (unsigned)xq, c1, id_lo, id_hi, k0, k1, r);
      const f32x4 z = philox_normal4(r);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (4 * xq + u < w) v[u] = v[u] + scale * z[u];
    }
    *reinterpret_cast<f32x4*>(dst + (base + i) * 4) = v;
  }
}

// the one place the level limit is written: the Python wrappers read it here
extern "C" int aod_loc_stability_max_levels(void) { return LS_MAX_LEVELS; }

extern "C" int aod_pixel_noise(const float* src, float* dst, int B, int C, int Hp, int Wp, const int32_t* hw, const float* inv_std, float sigma,
                               int level, uint64_t seed, const int64_t* image_ids, aod_stream_t stream) {
  AOD_CHECK_ARG(B >= 1 && B <= 65535, "pixel_noise: batch must be in 1..65535 (got %d)", B);
  AOD_CHECK_ARG(C >= 1 && C <= 4, "pixel_noise: 1..4 channels are supported (got C = %d)", C);
  AOD_CHECK_ARG(Hp >= 1 && Hp <= 65536, "pixel_noise: padded height must be in 1..65536 (got %d)", Hp);
  AOD_CHECK_ARG(Wp >= 1 && Wp <= 262144, "pixel_noise: padded width must be in 1..262144 (got %d)", Wp);
  AOD_CHECK_ARG(Wp % 4 == 0, "pixel_noise: padded width must be a multiple of 4 (got %d)", Wp);
  AOD_CHECK_ARG(level >= 0 && level < LS_MAX_LEVELS, "pixel_noise: level must be in 0..%d (got %d)", LS_MAX_LEVELS - 1, level);
  AOD_CHECK_ARG(sigma >= 0.f && sigma <= 3.4028234e38f, "pixel_noise: sigma must be finite and >= 0 (got %g)", (double)sigma);
  AOD_CHECK_ARG(src && dst && hw && inv_std && image_ids, "pixel_noise: null pointer");
  ls_inv_std is = {{0.f, 0.f, 0.f, 0.f}};
  for (int c = 0; c < C; ++c) {
    AOD_CHECK_ARG(inv_std[c] > 0.f && inv_std[c] <= 3.4028234e38f, "pixel_noise: inv_std[%d] must be finite and > 0 (got %g)", c, (double)inv_std[c]);
    is.v[c] = inv_std[c];
  }
  AOD_CHECK_ARG(dst != src, "pixel_noise: dst == src: the kernel is out of place");
  const size_t bytes = (size_t)B * C * Hp * Wp * 4;
  AOD_CHECK_ARG((size_t)dst + bytes <= (size_t)src || (size_t)src + bytes <= (size_t)dst, "pixel_noise: dst overlaps src: the kernel is out of place");
  AOD_CHECK_ARG(((((size_t)src) | ((size_t)dst)) & 15) == 0 && (((size_t)hw) & 3) == 0 && (((size_t)image_ids) & 7) == 0,
                "pixel_noise: src / dst must be 16-B aligned, hw and image_ids aligned to their element size");
  const long long n4 = (long long)Hp * (Wp / 4);
  const int gx = (int)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
  hipLaunchKernelGGL(pixel_noise_kernel, dim3(gx, C, B), dim3(256), 0, (hipStream_t)stream, src, dst, C, Hp, Wp / 4, hw, is, sigma, (unsigned)level,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (const long long*)image_ids);
  AOD_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(LS_TB) void loc_stability_kernel(const float* __restrict__ dets, const long long* __restrict__ labels,
                                                              const int* __restrict__ num, int K, int B, int max_num, float thr, int same_class,
                                                              int combine, float* __restrict__ unc, float* __restrict__ stab_out) {
  __shared__ f32x4 sbox[LS_MAX_DET];       // the level's boxes
  __shared__ long long slab[LS_MAX_DET];   // ... and labels
  __shared__ float vw[LS_MAX_DET];         // w_j        (0: no object)
  __shared__ float vws[LS_MAX_DET];        // w_j S_j    (0: no object)
  __shared__ float vmx[LS_MAX_DET];        // w_j        (-inf: no object)
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long img = (long long)max_num, slot = (long long)B * max_num;
  const float* d0 = dets + b * img * 5;
  const long long* l0 = labels + b * img;
  int nd = num[b];
  nd = nd < 0 ? 0 : (nd > max_num ? max_num : nd);
  // the reference rows this thread owns
  float ax1[LS_ROWS], ay1[LS_ROWS], ax2[LS_ROWS], ay2[LS_ROWS], aa[LS_ROWS], w[LS_ROWS], acc[LS_ROWS];
  long long alab[LS_ROWS];
  bool obj[LS_ROWS];
#pragma unroll
  for (int r = 0; r < LS_ROWS; ++r) {
    const int j = tid + r * LS_TB;
    obj[r] = false;
    ax1[r] = ay1[r] = ax2[r] = ay2[r] = aa[r] = w[r] = acc[r] = 0.f;
    alab[r] = 0;
    if (j < nd) {
      const float s = d0[j * 5 + 4];
      if (s > thr) {
        obj[r] = true;
        w[r] = s;
        ax1[r] = d0[j * 5]; ay1[r] = d0[j * 5 + 1]; ax2[r] = d0[j * 5 + 2]; ay2[r] = d0[j * 5 + 3];
        aa[r] = __fmul_rn(__fsub_rn(ax2[r], ax1[r]), __fsub_rn(ay2[r], ay1[r]));
        alab[r] = l0[j];
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    const float* dk = dets + (k + 1) * slot * 5 + b * img * 5;
    const long long* lk = labels + (k + 1) * slot + b * img;
    int nk = num[(long long)(k + 1) * B + b];
    nk = nk < 0 ? 0 : (nk > max_num ? max_num : nk);
    __syncthreads();                                         // the previous level has been scanned
    for (int i = tid; i < nk; i += LS_TB) {
      f32x4 q;
      q[0] = dk[i * 5]; q[1] = dk[i * 5 + 1]; q[2] = dk[i * 5 + 2]; q[3] = dk[i * 5 + 3];
      sbox[i] = q;
      slab[i] = lk[i];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LS_ROWS; ++r) {
      if (!obj[r]) continue;
      float m = 0.f;
      for (int i = 0; i < nk; ++i) {
        if (same_class && slab[i] != alab[r]) continue;
        const f32x4 q = sbox[i];
        const float ab = __fmul_rn(__fsub_rn(q[2], q[0]), __fsub_rn(q[3], q[1]));
        const float iw = fmaxf(__fsub_rn(fminf(ax2[r], q[2]), fmaxf(ax1[r], q[0])), 0.f);
        const float ih = fmaxf(__fsub_rn(fminf(ay2[r], q[3]), fmaxf(ay1[r], q[1])), 0.f);
        const float ov = __fmul_rn(iw, ih);
        const float un = __fsub_rn(__fadd_rn(aa[r], ab), ov);
        const float iou = __fdiv_rn(ov, fmaxf(un, 1e-6f));
        if (iou > m) m = iou;
      }
      acc[r] = __fadd_rn(acc[r], m);
    }
  }
  // S_j and the leaves of the trees
  const float fK = (float)K;
#pragma unroll
  for (int r = 0; r < LS_ROWS; ++r) {
    const int j = tid + r * LS_TB;
    const float S = __fdiv_rn(acc[r], fK);
    vw[j] = obj[r] ? w[r] : 0.f;
    vws[j] = obj[r] ? __fmul_rn(w[r], S) : 0.f;
    vmx[j] = obj[r] ? w[r] : -INFINITY;
    if (stab_out && j < max_num) stab_out[b * img + j] = obj[r] ? S : NAN;
  }
  // pairwise tree over the next power of two >= max_num
  int np2 = 1;
  while (np2 < max_num) np2 <<= 1;
  for (int st = np2 >> 1; st > 0; st >>= 1) {
    __syncthreads();
    for (int i = tid; i < st; i += LS_TB) {
      vw[i] = __fadd_rn(vw[i], vw[i + st]);
      vws[i] = __fadd_rn(vws[i], vws[i + st]);
      vmx[i] = fmaxf(vmx[i], vmx[i + st]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    float u = 0.f;
    if (vmx[0] != -INFINITY) {
      u = __fsub_rn(1.0f, __fdiv_rn(vws[0], vw[0]));
      if (combine == 1) u = __fadd_rn(u, __fsub_rn(1.0f, vmx[0]));
    }
    unc[b] = u;
  }
}

extern "C" int aod_loc_stability(const float* dets, const int64_t* labels, const int32_t* num, int K, int B, int max_num, float score_thr,
                                 int same_class, int combine, float* unc, float* stab_out, aod_stream_t stream) {
  AOD_CHECK_ARG(K >= 1 && K <= LS_MAX_LEVELS, "loc_stability: the number of noise levels K must be in 1..%d (got %d)", LS_MAX_LEVELS, K);
  AOD_CHECK_ARG(B >= 1, "loc_stability: batch must be positive (got %d)", B);
  AOD_CHECK_ARG(max_num >= 1 && max_num <= LS_MAX_DET, "loc_stability: max_num must be in 1..%d (got %d)", LS_MAX_DET, max_num);
  AOD_CHECK_ARG(combine == 0 || combine == 1, "loc_stability: combine %d is none of 0 (ls), 1 (ls+c)", combine);
  AOD_CHECK_ARG(same_class == 0 || same_class == 1, "loc_stability: same_class must be 0 or 1 (got %d)", same_class);
  AOD_CHECK_ARG(score_thr == score_thr, "loc_stability: score_thr is NaN");
  AOD_CHECK_ARG(dets && labels && num && unc, "loc_stability: null pointer");
  AOD_CHECK_ARG(((((size_t)dets) | ((size_t)num) | ((size_t)unc) | ((size_t)stab_out)) & 3) == 0 && (((size_t)labels) & 7) == 0,
                "loc_stability: pointers must be aligned to their element size");
  hipLaunchKernelGGL(loc_stability_kernel, dim3((unsigned)B), dim3(LS_TB), 0, (hipStream_t)stream, dets, (const long long*)labels, num, K, B, max_num,
                     score_thr, same_class, combine, unc, stab_out);
  AOD_LAUNCH_CHECK();
  return 0;
}
