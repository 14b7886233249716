// Weight gradient of the NHWC implicit-GEMM convolution for gfx950 (MI355X); forward and dgrad: conv.hip.
//   dW[n][(r,s,c)] += sum_m dZ[m][n] * A[m][(r,s,c)]: both operands are contracted over their ROW index, so the LDS images keep the
//   global row-major form and fragments are read with ds_read_b64_tr_b16 (hardware transpose); the pixel axis m is split across
//   workgroups, which store per-split slabs (added in order by the unpack kernel of conv.hip) or add with fp32 atomics.
// Dispatch (at the end of the file):  wgrad_fill -> wgrad_make_plan -> wgrad_run   (DESIGN.md "How a weight gradient picks its kernel")
#include "common.h"
#include "conv_params.h"

// Row table: one 32-B record per GEMM row m (= destination pixel): where its receptive field starts.
// Depends only on the segment geometry / stride / pad, so it is built once per geometry and shared by every conv
// (and every iteration) with that geometry -- the per-step im2col decode of wgrad becomes one 32-B record per pixel.
struct RowRec {       // 32 B: two 16-B pieces, fetched by LDS-DMA (one wave-instruction = the records of 32 pixels)
  unsigned xrow;     // byte offset of the top-left tap pixel (b, y0, x0) in the source (wraps for y0/x0 < 0: only used when valid)
  unsigned zoff;     // byte offset of this pixel's row in the dZ buffer
  unsigned wc2;      // source row pitch in bytes: W * C * 2
  unsigned pad_;
  unsigned long long mask;   // bit (r*S + s) set <=> tap (r, s) lies inside the image for this pixel (R*S <= 64)
  unsigned long long pad2_;
};
static_assert(sizeof(RowRec) == 32, "row record layout");

__global__ void row_table_kernel(const ConvKParams p, RowRec* __restrict__ tab) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= p.M) return;
  int sg = 0, mstart = 0;
  while (sg < p.nseg - 1 && m >= p.seg_mend[sg]) { mstart = p.seg_mend[sg]; ++sg; }
  const int ml = m - mstart;
  const int ohw = p.segOH[sg] * p.segOW[sg];
  const int b = ml / ohw, rem = ml - b * ohw;
  const int oy = rem / p.segOW[sg], ox = rem - oy * p.segOW[sg];
  const int H = p.segH[sg], W = p.segW[sg];
  const int y0 = oy * p.stride - p.pad, x0 = ox * p.stride - p.pad;
  RowRec r;
  r.xrow = (unsigned)((p.seg_src0[sg] + (long long)b * H * W + (long long)y0 * W + x0) * p.C * 2);
  r.zoff = (unsigned)((p.seg_dst0[sg] + ml) * (long long)p.N * 2);
  r.wc2 = (unsigned)(W * p.C * 2);
  unsigned long long mk = 0;
  for (int tr = 0; tr < p.R; ++tr)
    for (int ts = 0; ts < p.S; ++ts) {
      const int y = y0 + tr * p.dil, x = x0 + ts * p.dil;
      if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) mk |= 1ull << (tr * p.S + ts);
    }
  r.mask = mk;
  r.pad_ = 0; r.pad2_ = 0;
  tab[m] = r;
}

extern "C" size_t aod_conv_row_table_bytes(const aod_conv_desc_t* d) {
  long long m = 0;
  for (int i = 0; i < d->nseg; ++i) m += (long long)d->seg[i].B * d->seg[i].OH * d->seg[i].OW;
  return (size_t)m * sizeof(RowRec);
}

extern "C" int aod_conv_row_table(const aod_conv_desc_t* d, void* table, aod_stream_t stream) {
  AOD_CHECK_ARG(d && table && !d->transposed, "row_table: bad args");
  ConvKParams cp;
  memset(&cp, 0, sizeof(cp));
  int rc = fill_params(d, cp);
  if (rc) return rc;
  if (cp.M == 0) return 0;
  AOD_CHECK_ARG(d->R * d->S <= 64, "row_table: at most 64 filter taps (got %d)", d->R * d->S);
  hipLaunchKernelGGL(row_table_kernel, dim3((cp.M + 255) / 256), dim3(256), 0, (hipStream_t)stream, cp, (RowRec*)table);
  AOD_LAUNCH_CHECK();
  return 0;
}

struct WgradParams {
  const bf16_t* x;
  const bf16_t* dz;
  float* dw;
  const RowRec* tab;
  int C, N, K, R, S, dil;
  int M;
  int tiles_n, tiles_k, splits, rows_per_split, stagger, xcd_order, x3;
  long long x_bytes, z_bytes, tab_bytes;
  long long slab_stride;     // > 0: split s STORES its partial tile into dw + s * slab_stride (deterministic, summed by the unpack); 0: fp32 atomics
  const unsigned char* zmap; // sparse backward (the wide x3 forms' SPARSE instances): row-activity map of dZ, one byte per 64 GEMM rows (dense dZ
                             // segments: GEMM row = dZ row); a workgroup walks only the pixel steps of its split whose block is 1.  nullptr: all
};

// byte offset of (row, 16-B chunk) in a 256-B-pitch bf16 image that serves transposed reads
__device__ __forceinline__ int tr_off(int row, int ch) {
  return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}

// dW[n][kk] += sum_m dZ[m][n] * X[pix(m, tap(kk))][c(kk)]: (128 TN) x (128 TK) output tile per workgroup, 64 pixels per step.
// Both operands are staged as 128-column SUB-IMAGES that keep the global row-major form ([pixel][128 columns], 256-B rows), TN of dZ and
// TK of X per stage, filled by LDS-DMA: one wave-instruction = 4 pixel rows x 16 chunks, the conflict-avoiding XOR applied on the SOURCE
// chunk index, which is the same for the 4 rows a lane serves -> every lane owns ONE fixed (tap, channel-chunk) column per sub-image.
// NW waves per workgroup (4 or 8).  128 x 128 tile: split 2 x 2 (64 x 64 per wave) or 2 x 4 (64 x 32 per wave), two workgroups per
// CU.  256 x 256 tile (TN = TK = 2, 8 waves as 2 x 4, 128 x 64 per wave, one workgroup per CU): the fragment reads are 8-B transposed
// reads, so the 128 x 128 form moves 768 B of LDS per MFMA -- more than the LDS delivers at the matrix pipe's rate; the big tile halves
// that (and the LDS-DMA traffic per MFMA), like the 256 x 256 tile of the forward kernel.
// X3 (aod_conv_desc_t.x3): dZ and X are X-layout rows, so a tile of dW' = dZ'^T X' holds the four products (zh, zl) x (xh, xl) of its
// logical entries in 32-wide bands.  A wave's block starts on a 64-column boundary in both directions and is a whole number of
// [h32 | l32] band pairs (4-wave 128 x 128 form: 64 x 64 per wave; 8-wave 256 x 256 form: 128 x 64): its zl x xl quarter (2^-16 of the
// result) is skipped at compile time, which leaves exactly the three products of the forward form; the unpack kernel adds the three bands
// of every slab.
// SPARSE (the 4-wave x3 instance; launches that carry a row-activity map of dZ): the active 64-row blocks of the whole pixel axis are dealt to
// the splits cyclically and a workgroup walks only its share -- see wgrad_tile_x3w below, the same scheme with one 64-pixel step per block.
constexpr int WG_SLIST_BYTES = 8192;      // LDS behind the row-record ring of a SPARSE instance: the list of a workgroup's blocks (16-bit entries)
template <int NW, int TN, int TK, bool X3, bool SPARSE = false>
__device__ __forceinline__ void wgrad_tile(const WgradParams& p, int bid_in) {
  static_assert(!X3 || (NW == 4 && TN == 1 && TK == 1) || (NW == 8 && TN == 2 && TK == 2), "X3: wave blocks must be whole [h32 | l32] band pairs");
  constexpr int RPW = 4 * NW;          // pixel rows covered per pass of all waves
  constexpr int PASSES = 64 / RPW;
  constexpr int WNC = NW / 2;          // waves along the (tap, channel) axis
  constexpr int NI = 4 * TN;           // 16-row groups per wave along the dZ-channel axis (2 waves along it)
  constexpr int NJ = 8 * TK / WNC;     // 16-column groups per wave along the (tap, channel) axis
  constexpr int BKM = 64;
  constexpr int IMG = BKM * 256;       // one 128-column sub-image
  constexpr int STAGE = (TN + TK) * IMG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  const int wm = uw / WNC, wn = uw % WNC;
  // bid_in runs (pixel split, tile) with the TILE fastest, over a range that one XCD executes contiguously (xcd_swizzle at the call site):
  // the tiles of a split -- the nine taps of a 3x3 filter read the same dZ rows and the same x rows at shifted positions -- share that XCD's
  // L2.  With the split fastest they were spread over all eight L2s and every operand row crossed HBM once per tile: 2.78 GB per grouped
  // tower launch for 0.36 GB of operands, i.e. the kernel ran at the HBM rate (profiles/r03_pmc_passes.txt).
  int bid = bid_in;
  const int ntile = p.tiles_n * p.tiles_k;
  const int split = bid / ntile; bid -= split * ntile;
  const int tile_k = bid % p.tiles_k, tile_n = bid / p.tiles_k;
  const int n0 = tile_n * (128 * TN), k0 = tile_k * (128 * TK);
  int ms = split * p.rows_per_split;
  int me = min(p.M, ms + p.rows_per_split);
  if (ms >= me) return;                                        // (never a planned split: splits = ceil(M / rows_per_split))
  constexpr int SLIST_CAP = WG_SLIST_BYTES / 2;
  const int nbt = (p.M + 63) >> 6;
  const bool deal = SPARSE && p.zmap && nbt <= 65535 && (nbt + p.splits - 1) / p.splits <= SLIST_CAP;
  if (deal) { ms = 0; me = p.M; }
  const auto rsrc_x = buf_rsrc(p.x, (int)p.x_bytes);
  const auto rsrc_z = buf_rsrc(p.dz, (int)p.z_bytes);
  const int prow = lane >> 4;                                  // pixel row inside the wave's 4-row group
  const int ch = (lane & 15) ^ ((prow << 2) | (uw & 3));       // source chunk of this lane (fixed)

  // per-lane constants of each sub-image: dZ column, and for X the byte offset of the lane's (tap, channel chunk) relative to a pixel's
  // top-left tap, its row offset and its mask bit
  unsigned zcol[TN];
  bool zok[TN];
#pragma unroll
  for (int h = 0; h < TN; ++h) {
    const int zn = n0 + 128 * h + ch * 8;
    zok[h] = zn < p.N;
    zcol[h] = (unsigned)(zn * 2);
  }
  unsigned cdx[TK];
  int dy[TK];
  unsigned long long tbit[TK];
#pragma unroll
  for (int h = 0; h < TK; ++h) {
    const int kk = k0 + 128 * h + ch * 8;
    const bool kok = kk < p.K;
    const int tap = kok ? kk / p.C : 0, c0 = kok ? kk - tap * p.C : 0;
    const int tr = tap / p.S, ts = tap - tr * p.S;
    dy[h] = tr * p.dil;
    cdx[h] = (unsigned)((ts * p.dil * p.C + c0) * 2);
    tbit[h] = kok ? (1ull << tap) : 0ull;
  }
  // Row records reach the lanes through LDS: waves 0 and 1 fetch the 64 records of a step with ONE LDS-DMA instruction each (two steps
  // ahead, into a two-slot ring behind the operand stages), every lane then picks its four with ds_read.  Fetching them into VGPRs
  // (global_load) beside the LDS-DMA operand loads made every K-step drain the whole vector-memory queue: 27 % of the kernel.
  const auto rsrc_t = buf_rsrc(p.tab, (int)p.tab_bytes);
  char* const stab = smem + 2 * STAGE;                        // [2][64] records
  auto tdma = [&](int mbase, int slot) {
    if (uw < 2) {
      const int m = mbase + 32 * uw + (lane >> 1);
      const unsigned off = (unsigned)min(m, p.M - 1) * 32u + (unsigned)(lane & 1) * 16u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_t, (__attribute__((address_space(3))) void*)(stab + slot * 2048 + uw * 1024), 16, off, 0, 0, 0);
    }
  };
  RowRec rec[PASSES];
  auto rread = [&](int slot) {
#pragma unroll
    for (int i = 0; i < PASSES; ++i) rec[i] = *reinterpret_cast<const RowRec*>(stab + slot * 2048 + (RPW * i + 4 * uw + prow) * 32);
  };
  auto gload = [&](int mbase, int buf) {
    char* sz = smem + buf * STAGE;
    char* sx = sz + TN * IMG;
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int m = mbase + RPW * i + 4 * uw + prow;
      const bool mok = m < me;
      const RowRec r = rec[i];
#pragma unroll
      for (int h = 0; h < TN; ++h) {
        const unsigned zoff = (mok && zok[h]) ? r.zoff + zcol[h] : BUF_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_z, (__attribute__((address_space(3))) void*)(sz + h * IMG + (RPW * i + 4 * uw) * 256), 16, zoff, 0, 0, 0);
      }
#pragma unroll
      for (int h = 0; h < TK; ++h) {
        const unsigned xoff = (mok && (r.mask & tbit[h])) ? r.xrow + (unsigned)dy[h] * r.wc2 + cdx[h] : BUF_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(sx + h * IMG + (RPW * i + 4 * uw) * 256), 16, xoff, 0, 0, 0);
      }
    }
  };

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  unsigned short* const slist = reinterpret_cast<unsigned short*>(stab + 4096);
  int nact = -1;                                                // -1: every step of the contiguous range
  if constexpr (SPARSE) {
    if (deal) {
      int base = 0;                                             // (every wave counts, wave 0 writes)
      for (int c = 0; c < nbt; c += 64) {
        const int b = c + lane;
        const bool on = b < nbt && p.zmap[b] != 0;
        const unsigned long long bm = __ballot(on);
        const int j = base + (int)__popcll(bm & ((1ull << lane) - 1ull));
        if (uw == 0 && on && j % p.splits == split) slist[j / p.splits] = (unsigned short)b;
        base += (int)__popcll(bm);
      }
      base = __builtin_amdgcn_readfirstlane(base);
      nact = base > split ? (base - split + p.splits - 1) / p.splits : 0;
      __syncthreads();
    }
  }
  const int nsteps = (SPARSE && nact >= 0) ? nact : (me - ms + BKM - 1) / BKM;
  auto mbase = [&](int stp) {
    if constexpr (SPARSE) {
      if (nact >= 0) return __builtin_amdgcn_readfirstlane((int)slist[stp]) * 64;
    }
    return ms + stp * BKM;
  };
  if (nsteps > 0) {
    tdma(mbase(0), 0);
    if (nsteps > 1) tdma(mbase(1), 1);
    __syncthreads();                                            // records of steps 0 and 1 are resident
    rread(0);
    gload(mbase(0), 0);
    __syncthreads();
  }
  // transposed-read lane roles: group g = lane>>4 covers k rows 8g..8g+7 of a 32-row sub-step; lane 4q+pp -> row q, cols 4pp..4pp+3
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
  // stagger (8-wave form): waves 4-7 run half a step behind waves 0-3, with which they share their SIMDs (see conv_igemm_kernel)
  const bool late = p.stagger && NW == 8 && uw >= 4;
  bool carried = false;
  // Fragment reads are ISSUED from inline asm: behind the ds_read_tr builtin hipcc (ROCm 7.2) waits vmcnt(0) ahead of the first read of
  // every step -- i.e. for the LDS-DMA of the NEXT stage issued just above -- which serialises load and compute inside each wave (the
  // plain ds_read_b128 of the forward kernel does not get that wait).  The asm reads are invisible to the compiler's counters; frag_wait()
  // is their s_waitcnt and makes every destination opaque, so no MFMA is scheduled above it.
  u32x2 alo[NI], ahi[NI], blo[NJ], bhi[NJ];
  auto tr_read = [&](u32x2& dst, const char* ptr) {
    const unsigned a = (unsigned)(unsigned long long)ptr;       // (the low half of a shared-aperture address is the LDS byte address)
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(a) : "memory");
  };
  auto frag_read = [&](const char* sz, const char* sx, int ks) {
    const int r0 = ks * 32 + 8 * g + q;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int col = wm * (16 * NI) + i * 16 + pp * 4;       // column of the dZ stage: sub-image col >> 7
      const char* im = sz + (col >> 7) * IMG;
      const int c = col & 127;
      tr_read(alo[i], im + tr_off(r0, c >> 3) + (c & 7) * 2);
      tr_read(ahi[i], im + tr_off(r0 + 4, c >> 3) + (c & 7) * 2);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = wn * (16 * NJ) + j * 16 + pp * 4;
      const char* im = sx + (col >> 7) * IMG;
      const int c = col & 127;
      tr_read(blo[j], im + tr_off(r0, c >> 3) + (c & 7) * 2);
      tr_read(bhi[j], im + tr_off(r0 + 4, c >> 3) + (c & 7) * 2);
    }
  };
  bf16x8 af[NI], bfr[NJ];
  auto frag_wait = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(alo[i]), "+v"(ahi[i]));
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(blo[j]), "+v"(bhi[j]));
#pragma unroll
    for (int i = 0; i < NI; ++i) af[i] = __builtin_bit_cast(bf16x8, (u32x4){alo[i][0], alo[i][1], ahi[i][0], ahi[i][1]});
#pragma unroll
    for (int j = 0; j < NJ; ++j) bfr[j] = __builtin_bit_cast(bf16x8, (u32x4){blo[j][0], blo[j][1], bhi[j][0], bhi[j][1]});
  };
  auto mfma_block = [&]() {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (X3 && (i & 3) >= 2 && (j & 3) >= 2) continue;       // tail x tail (16-row groups 2, 3 of every four = a tail band)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
  };
  for (int stp = 0; stp < nsteps; ++stp) {
    const int cur = stp & 1;
    if (late && carried) mfma_block();
    if (stp + 1 < nsteps) {
      rread((stp + 1) & 1);                                 // landed before the previous barrier
      gload(mbase(stp + 1), cur ^ 1);
    }
    // slot stp & 1 held this step's records; every wave read them one iteration ago (ahead of the barrier), so it can be refilled
    if (stp + 2 < nsteps) tdma(mbase(stp + 2), stp & 1);
    const char* sz = smem + cur * STAGE;
    const char* sx = sz + TN * IMG;
    frag_read(sz, sx, 0);
    frag_wait();
    mfma_block();
    frag_read(sz, sx, 1);
    frag_wait();                                            // (also in the late waves: their reads of this stage end before the barrier)
    if (!late) mfma_block(); else carried = true;
    __syncthreads();
  }
  if (late && carried) mfma_block();
  // slab mode: every pixel split owns a slab and STORES its partial tile (plain dword stores run at ~6 TB/s chip-wide, float atomics at
  // ~1.3 TB/s: 512 workgroups x 64 KB of atomics were a 25 us tail on every launch); the unpack kernel adds the slabs in split order,
  // so the weight gradient no longer depends on arrival order.  Otherwise: accumulate into dW[n][kk] with fp32 atomics (one dword per
  // lane, 16 consecutive columns per row group).
  float* const dwp = p.dw + (long long)split * p.slab_stride;
  const bool slab = p.slab_stride > 0;
  const int lr = lane & 15, lq = lane >> 4;
  if constexpr (X3) {
    // X3: the three bands of a logical entry sit in the SAME lane and register slot of three accumulators of this wave -- (zh, xh), (zh, xl)
    // and (zl, xh) -- and are added here, (hh + hl) + lh: the slab is the LOGICAL [N / 2][R][S][C / 2] partial gradient (a quarter of the
    // bytes of the band form) and the plain unpack kernel serves it
    const int KL = p.K >> 1;
#pragma unroll
    for (int I = 0; I < NI / 2; ++I)
#pragma unroll
      for (int J = 0; J < NJ / 2; ++J) {
        const int ih = (I >> 1) * 4 + (I & 1), jh = (J >> 1) * 4 + (J & 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + wm * (16 * NI) + ih * 16 + lq * 4 + r;        // physical column of the head of the entry's dZ channel
          const int k = k0 + wn * (16 * NJ) + jh * 16 + lr;                // ... and of its (tap, input channel)
          if (n < p.N && k < p.K) {
            const float v = (acc[ih][jh][r] + acc[ih][jh + 2][r]) + acc[ih + 2][jh][r];
            dwp[(long long)(((n >> 6) << 5) + (n & 31)) * KL + ((k >> 6) << 5) + (k & 31)] = v;
          }
        }
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wm * (16 * NI) + i * 16 + lq * 4 + r;
        const int k = k0 + wn * (16 * NJ) + j * 16 + lr;
#ifdef AOD_WGRAD_NO_EPI      // ablation build (tools/dbg): how much of the kernel is the atomic epilogue
        if (n < p.N && k < p.K && acc[i][j][r] == 12345.678f) p.dw[(long long)n * p.K + k] = 1.f;
#else
        if (n < p.N && k < p.K) {
          if (slab) dwp[(long long)n * p.K + k] = acc[i][j][r];
          else atomicAdd(p.dw + (long long)n * p.K + k, acc[i][j][r]);
        }
#endif
      }
}

// X3, WIDE form (the tower filters and every other layer whose X-layout dW is whole 512 x 512 tiles): a 256 x 256 LOGICAL tile per
// workgroup with ONE accumulator per entry -- zh*xh + zh*xl + zl*xh are summed in it, like the forward form sums its three products.  The
// band form above spends a 256 x 256 accumulator tile on 128 x 128 logical entries (a quarter of it on the tail x tail band it never
// computes) and issues 1.5 MFMAs per accumulator and 64-pixel step for 64 KB of staged operands; this form stages the same 64 KB per
// 32-pixel step -- eight 128-column sub-images: [zh32 | zl32] x 4 channel groups for each operand -- for 3 MFMAs per accumulator: twice the
// matrix work per staged byte, four times per LDS fragment read.  8 waves as 2 x 4, 128 x 64 logical entries per wave (32 accumulators);
// the head fragments of dZ are replaced by its tail fragments for the third product (the x fragments stay).
// NW = 8, T = 4: 512 x 512 physical columns = 256 x 256 logical entries, one workgroup per CU.  NW = 4, T = 2: 256 x 256 physical = 128 x 128
// logical (2 x 2 waves, 64 x 64 logical per wave, 16 accumulators; two workgroups per CU): the backbone layers whose dW is not whole
// 512-column tiles or whose pixel axis is too short to fill the chip with the big form.
// SPARSE (launches that carry a row-activity map of dZ, sparse backward): the active 64-row blocks of the WHOLE pixel axis are DEALT to the
// member's splits cyclically -- active block j goes to split j % splits -- and a workgroup compacts its share into an LDS list and runs its
// rings (row records, LDS-DMA stages) over that list instead of over the pixel steps of a contiguous range.  The positives sit at the end of
// the pyramid buffer (P4 - P7), so a contiguous split kept 45 - 64 % of its steps and the launch lasted as long as that split; the deal gives
// every split the same count.  A skipped step would have added dZ = 0 products only; what changes is WHICH slab a step's products land in,
// i.e. the fp32 summation order of the filter gradient (mapped launches only).  A split without a block stores a zero slab.  More blocks
// than the 16-bit list entries / the list can hold: the contiguous range, every step.
template <int NW, int T, bool SPARSE = false>
__device__ __forceinline__ void wgrad_tile_x3w(const WgradParams& p, int bid_in) {
  static_assert((NW == 8 && T == 4) || (NW == 4 && T == 2), "wide x3 wgrad forms");
  constexpr int TN = T, TK = T, BKM = 32;
  constexpr int RPW = 4 * NW, PASSES = BKM / RPW;      // pixel rows per pass of all waves
  constexpr int IMG = BKM * 256;              // one 128-column sub-image: 8 KB
  constexpr int STAGE = (TN + TK) * IMG;      // 64 KB
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  constexpr int WNC = NW / 2;                           // waves along the (tap, channel) axis
  const int wm = uw / WNC, wn = uw % WNC;
  int bid = bid_in;
  const int ntile = p.tiles_n * p.tiles_k;
  const int split = bid / ntile; bid -= split * ntile;
  const int tile_k = bid % p.tiles_k, tile_n = bid / p.tiles_k;
  const int n0 = tile_n * (128 * T), k0 = tile_k * (128 * T);       // physical columns
  int ms = split * p.rows_per_split;
  int me = min(p.M, ms + p.rows_per_split);
  if (ms >= me) return;                                        // (never a planned split: both plans set splits = ceil(M / rows_per_split), so no dealt share is lost here)
  constexpr int SLIST_CAP = (2048 + WG_SLIST_BYTES) / 2;
  const int nbt = (p.M + 63) >> 6;                             // 64-row blocks of the whole pixel axis
  const bool deal = SPARSE && p.zmap && nbt <= 65535 && (nbt + p.splits - 1) / p.splits <= SLIST_CAP;
  if (deal) { ms = 0; me = p.M; }                              // the workgroup's rows come from all over the axis
  const auto rsrc_x = buf_rsrc(p.x, (int)p.x_bytes);
  const auto rsrc_z = buf_rsrc(p.dz, (int)p.z_bytes);
  const auto rsrc_t = buf_rsrc(p.tab, (int)p.tab_bytes);
  const int prow = lane >> 4;                                  // pixel row inside the wave's 4-row group
  const int ch = (lane & 15) ^ ((prow << 2) | (uw & 3));       // source chunk of this lane (fixed; tr_off's key of row RPW * i + 4 * uw + prow)
  unsigned zcol[TN];
  bool zok[TN];
#pragma unroll
  for (int h = 0; h < TN; ++h) {
    const int zn = n0 + 128 * h + ch * 8;
    zok[h] = zn < p.N;
    zcol[h] = (unsigned)(zn * 2);
  }
  unsigned cdx[TK];
  int dy[TK];
  unsigned long long tbit[TK];
#pragma unroll
  for (int h = 0; h < TK; ++h) {
    const int kk = k0 + 128 * h + ch * 8;
    const bool kok = kk < p.K;
    const int tap = kok ? kk / p.C : 0, c0 = kok ? kk - tap * p.C : 0;
    const int tr = tap / p.S, ts = tap - tr * p.S;
    dy[h] = tr * p.dil;
    cdx[h] = (unsigned)((ts * p.dil * p.C + c0) * 2);
    tbit[h] = kok ? (1ull << tap) : 0ull;
  }
  char* const stab = smem + 2 * STAGE;                        // [2][32] row records
  auto tdma = [&](int mbase, int slot) {
    if (uw == 0) {
      const int m = mbase + (lane >> 1);
      const unsigned off = (unsigned)min(m, p.M - 1) * 32u + (unsigned)(lane & 1) * 16u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_t, (__attribute__((address_space(3))) void*)(stab + slot * 1024), 16, off, 0, 0, 0);
    }
  };
  RowRec rec[PASSES];
  auto rread = [&](int slot) {
#pragma unroll
    for (int i = 0; i < PASSES; ++i) rec[i] = *reinterpret_cast<const RowRec*>(stab + slot * 1024 + (RPW * i + 4 * uw + prow) * 32);
  };
  auto gload = [&](int mbase, int buf) {
    char* sz = smem + buf * STAGE;
    char* sx = sz + TN * IMG;
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int m = mbase + RPW * i + 4 * uw + prow;
      const bool mok = m < me;
      const RowRec r = rec[i];
#pragma unroll
      for (int h = 0; h < TN; ++h) {
        const unsigned zoff = (mok && zok[h]) ? r.zoff + zcol[h] : BUF_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_z, (__attribute__((address_space(3))) void*)(sz + h * IMG + (RPW * i + 4 * uw) * 256), 16, zoff, 0, 0, 0);
      }
#pragma unroll
      for (int h = 0; h < TK; ++h) {
        const unsigned xoff = (mok && (r.mask & tbit[h])) ? r.xrow + (unsigned)dy[h] * r.wc2 + cdx[h] : BUF_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(sx + h * IMG + (RPW * i + 4 * uw) * 256), 16, xoff, 0, 0, 0);
      }
    }
  };
  // 16-entry groups per wave: NW = 8: 128 logical dZ channels x 64 logical (tap, channel) columns; NW = 4: 64 x 64
  constexpr int NI = 32 * T / 16, NJ = 4;
  constexpr int WML = 16 * NI, WNL = 16 * NJ;
  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // this split's share of the active blocks: the j-th active block of the axis (ascending) belongs to split j % splits, at list slot j / splits
  constexpr int SPB = 64 / BKM;                                 // pixel steps per block
  unsigned short* const slist = reinterpret_cast<unsigned short*>(stab + 2048);
  int nact = -1;                                                // -1: every step of the contiguous range (no map, or too many blocks)
  if constexpr (SPARSE) {
    if (deal) {
      int base = 0;                                             // (every wave counts, wave 0 writes: the count needs no LDS word)
      for (int c = 0; c < nbt; c += 64) {
        const int b = c + lane;
        const bool on = b < nbt && p.zmap[b] != 0;
        const unsigned long long bm = __ballot(on);
        const int j = base + (int)__popcll(bm & ((1ull << lane) - 1ull));
        if (uw == 0 && on && j % p.splits == split) slist[j / p.splits] = (unsigned short)b;
        base += (int)__popcll(bm);
      }
      base = __builtin_amdgcn_readfirstlane(base);
      nact = base > split ? (base - split + p.splits - 1) / p.splits : 0;
      __syncthreads();
    }
  }
  const int nsteps = (SPARSE && nact >= 0) ? SPB * nact : (me - ms + BKM - 1) / BKM;
  auto mbase = [&](int stp) {
    if constexpr (SPARSE) {
      if (nact >= 0) return ms + __builtin_amdgcn_readfirstlane((int)slist[stp / SPB]) * 64 + (stp % SPB) * BKM;
    }
    return ms + stp * BKM;
  };
  if (nsteps > 0) {
    tdma(mbase(0), 0);
    if (nsteps > 1) tdma(mbase(1), 1);
    __syncthreads();
    rread(0);
    gload(mbase(0), 0);
    __syncthreads();
  }
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
  auto tr_read = [&](u32x2& dst, const char* ptr) {
    const unsigned a = (unsigned)(unsigned long long)ptr;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(a) : "memory");
  };
  // fragment of the 16 physical columns [col, col + 16) of an operand stage: pixel rows 8g + q (+4), 4 columns per lane
  auto frag = [&](u32x2& lo, u32x2& hi, const char* base, int col) {
    const char* im = base + (col >> 7) * IMG;
    const int c = (col & 127) + pp * 4;
    tr_read(lo, im + tr_off(8 * g + q, c >> 3) + (c & 7) * 2);
    tr_read(hi, im + tr_off(8 * g + q + 4, c >> 3) + (c & 7) * 2);
  };
  u32x2 alo[NI], ahi[NI], bhlo[NJ], bhhi[NJ], bllo[NJ], blhi[NJ];
  bf16x8 af[NI], bh[NJ], bl[NJ];
  for (int stp = 0; stp < nsteps; ++stp) {
    const int cur = stp & 1;
    if (stp + 1 < nsteps) {
      rread((stp + 1) & 1);                                 // landed before the previous barrier
      gload(mbase(stp + 1), cur ^ 1);
    }
    if (stp + 2 < nsteps) tdma(mbase(stp + 2), stp & 1);
    const char* sz = smem + cur * STAGE;
    const char* sx = sz + TN * IMG;
    // heads of dZ, heads and tails of x
#pragma unroll
    for (int i = 0; i < NI; ++i) { const int nl = wm * WML + i * 16; frag(alo[i], ahi[i], sz, ((nl >> 5) << 6) + (nl & 31)); }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int kl = wn * WNL + j * 16, col = ((kl >> 5) << 6) + (kl & 31);
      frag(bhlo[j], bhhi[j], sx, col);
      frag(bllo[j], blhi[j], sx, col + 32);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NI; ++i) { asm volatile("" : "+v"(alo[i]), "+v"(ahi[i])); af[i] = __builtin_bit_cast(bf16x8, (u32x4){alo[i][0], alo[i][1], ahi[i][0], ahi[i][1]}); }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      asm volatile("" : "+v"(bhlo[j]), "+v"(bhhi[j]), "+v"(bllo[j]), "+v"(blhi[j]));
      bh[j] = __builtin_bit_cast(bf16x8, (u32x4){bhlo[j][0], bhlo[j][1], bhhi[j][0], bhhi[j][1]});
      bl[j] = __builtin_bit_cast(bf16x8, (u32x4){bllo[j][0], bllo[j][1], blhi[j][0], blhi[j][1]});
    }
    // tails of dZ requested now, consumed after the two head products
    u32x2 tlo[NI], thi[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) { const int nl = wm * WML + i * 16; frag(tlo[i], thi[i], sz, ((nl >> 5) << 6) + (nl & 31) + 32); }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bh[j], acc[i][j], 0, 0, 0);       // zh * xh
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bl[j], acc[i][j], 0, 0, 0);       // zh * xl
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NI; ++i) { asm volatile("" : "+v"(tlo[i]), "+v"(thi[i])); af[i] = __builtin_bit_cast(bf16x8, (u32x4){tlo[i][0], tlo[i][1], thi[i][0], thi[i][1]}); }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bh[j], acc[i][j], 0, 0, 0);         // zl * xh
    __syncthreads();
  }
  // logical slab [N / 2][K / 2] of this pixel split
  float* const dwp = p.dw + (long long)split * p.slab_stride;
  const int lr = lane & 15, lq = lane >> 4;
  const int NL = p.N >> 1, KL = p.K >> 1;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = (n0 >> 1) + wm * WML + i * 16 + lq * 4 + r;
        const int k = (k0 >> 1) + wn * WNL + j * 16 + lr;
        if (n < NL && k < KL) dwp[(long long)n * KL + k] = acc[i][j][r];
      }
}
template <int NW, int T, bool SPARSE = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_wgrad_x3w_kernel(const WgradParams p) {
  wgrad_tile_x3w<NW, T, SPARSE>(p, p.xcd_order ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x);
}

// split of the pixel axis over workgroups: all workgroups co-resident (<= 2 per CU, no ragged second round); cost model (measured on
// MI355X): one 64-pixel step costs ~1.45 us with one workgroup per CU and ~1.7 us with two (both share the CU); every workgroup ends with
// 64 KB of output -- fp32 atomics at ~1.3 TB/s chip-wide (0.05 us per workgroup) or, in slab mode, plain stores at ~5.5 TB/s (0.012 us)
// plus the unpack kernel's read of one more slab per split.
template <int NW, int TN, int TK, bool X3 = false, bool SPARSE = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(TN * TK > 1 ? 2 : NW / 2, TN * TK > 1 ? 2 : NW / 2))) void conv_wgrad_kernel(const WgradParams p) {
  wgrad_tile<NW, TN, TK, X3, SPARSE>(p, p.xcd_order ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x);
}
// Grouped launch: up to WG_MAXG weight gradients (ANY geometries, one tile form) share one grid.  Alone a backbone layer needs 100+ pixel
// splits of its few 128 x 128 tiles to fill the chip -- a 512 x 128 filter (256 KB) leaves 30 MB of partial slabs for the unpack; three
// layers together need a third of the splits each (longer pixel runs per workgroup, a third of the slab traffic, one launch).
struct WgradGroups { WgradParams g[WG_MAXG]; int wg0[WG_MAXG + 1]; int n; };
template <int NW, int TN, int TK, bool X3 = false, bool SPARSE = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(TN * TK > 1 ? 2 : NW / 2, TN * TK > 1 ? 2 : NW / 2))) void conv_wgrad_grouped_kernel(const WgradGroups gp) {
  const int b = gp.g[0].xcd_order ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
  // (selects, not an indexed read of the argument block: a run-time index would move the whole array to scratch memory)
  if (b < gp.wg0[1]) wgrad_tile<NW, TN, TK, X3, SPARSE>(gp.g[0], b);
  else if (b < gp.wg0[2]) wgrad_tile<NW, TN, TK, X3, SPARSE>(gp.g[1], b - gp.wg0[1]);
  else if (b < gp.wg0[3]) wgrad_tile<NW, TN, TK, X3, SPARSE>(gp.g[2], b - gp.wg0[2]);
  else wgrad_tile<NW, TN, TK, X3, SPARSE>(gp.g[3], b - gp.wg0[3]);
}

template <int NW, int T, bool SPARSE = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_wgrad_grouped_x3w_kernel(const WgradGroups gp) {
  const int b = gp.g[0].xcd_order ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
  if (b < gp.wg0[1]) wgrad_tile_x3w<NW, T, SPARSE>(gp.g[0], b);
  else if (b < gp.wg0[2]) wgrad_tile_x3w<NW, T, SPARSE>(gp.g[1], b - gp.wg0[1]);
  else if (b < gp.wg0[3]) wgrad_tile_x3w<NW, T, SPARSE>(gp.g[2], b - gp.wg0[2]);
  else wgrad_tile_x3w<NW, T, SPARSE>(gp.g[3], b - gp.wg0[3]);
}

// =====================================================================================
// dispatch:  wgrad_fill -> wgrad_make_plan -> wgrad_run   (DESIGN.md "How a weight gradient picks its kernel")
// =====================================================================================
typedef aod_wgrad_plan_t WgradPlan;      // what wgrad_make_plan() decides and wgrad_run() follows (include/aod_hip.h: aod_conv2d_wgrad_plan reports it)

// Cost model of a SINGLE launch.
// `big`: tile form -- 0 = 128 x 128, 1 = 256 x 256, 2 = the WIDE x3 form of 8 waves (512 x 512 physical columns = 256 x 256 logical entries,
// wgrad_tile_x3w<8, 4>), 3 = the wide x3 form of 4 waves (256 x 256 physical = 128 x 128 logical, wgrad_tile_x3w<4, 2>)
static void wgrad_plan(int M, int N, int K, bool slabs, int& tiles_n, int& tiles_k, int& splits, int& rps, int& big, int big_min_m = 49152, int x3 = 0) {
  const ConvKnobs::Once& k1 = ConvKnobs::once();
  // the 256 x 256 tile (one workgroup per CU): deep layers whose dW is whole tiles of it and whose pixel axis gives every CU a long run
  const bool no_big = knob_is(k1.wgrad_256, '0');
  // (measured, single launches: 16 x 32 x 32 pixels lose 15 % with the big tile, 16 x 64 x 64 gain 10 %; members of a GROUP get longer pixel
  // runs per workgroup and take it from 16 384 pixels on: -0.11 ms per step, AOD_WGRAD_BIG_MINM overrides the group threshold)
  big = (N % 256 == 0 && K % 256 == 0 && M >= big_min_m) ? 1 : 0;
  if (no_big) big = 0;
  if (x3 && !knob_is(k1.wgrad_x3_wide, '0')) {
    if (N % 512 == 0 && K % 512 == 0 && M >= big_min_m && !no_big) big = 2;
    else if (N % 256 == 0 && K % 256 == 0) big = 3;
    else {
      // narrow dZ (the prediction convs: 384 / 128 / 64 physical columns) on a long pixel axis: the wide 4-wave form with a ragged column
      // tile (its loads of columns >= N return zeros, its stores are bounds-checked) -- 128 FLOP per staged byte instead of 64, which is what
      // bounds the 128 x 128 form.  AOD_WGRAD_X3_RAGGED=0: the 128 x 128 form.
      // (64 columns -- retina_L -- stay on the 128 x 128 form: 118 vs 137 us; the 8-wave wide form for the 384-column retina_cls measured the
      // same as this one, profiles/r05_x3_tile_ab.txt)
      if (!knob_is(k1.wgrad_x3_ragged, '0') && N % 64 == 0 && N >= 128 && K % 256 == 0 && M >= 16384) big = 3;
    }
  }
  const int T = big == 2 ? 512 : (big ? 256 : 128);
  tiles_n = (N + T - 1) / T;
  tiles_k = (K + T - 1) / T;
  const int tiles = tiles_n * tiles_k;
  int best = 1;
  double best_cost = 1e30;
  const int slots = (big == 1 || big == 2) ? 256 : 512;
  const int max_s = slots / tiles > 0 ? slots / tiles : 1;
  for (int sp = 1; sp <= max_s; ++sp) {
    const int rows = ((M + sp - 1) / sp + 63) / 64 * 64;
    const int nsp = (M + rows - 1) / rows;
    const int wgs = tiles * nsp;
    double cost = (rows / 64) * (big == 2 ? 4.5 : (big == 3 ? (wgs > 256 ? 2.6 : 2.2) : (big ? 2.9 : (wgs > 256 ? 1.7 : 1.45))));
    cost += slabs ? wgs * 0.012 * (big ? 4 : 1) + nsp * ((double)N * K * (x3 ? 1.0 : 4.0)) / 2.5e6 : wgs * 0.05 * (big ? 4 : 1);
    if (cost < best_cost) { best_cost = cost; best = sp; }
  }
  rps = ((M + best - 1) / best + 63) / 64 * 64;
  splits = (M + rps - 1) / rps;
}

// Split plan of a GROUP (slab form): every workgroup of the launch runs the same number T of 64-pixel steps (the groups' tiles are the same
// size, so that equalises their durations); T = the smallest for which the grid fits the chip's slots -- group g then gets ceil(steps_g / T)
// splits.  All members must take the same tile form (`big` of wgrad_plan); returns that form, or -1 when they do not.
static int wgrad_plan_group(int n, const int* M, const int* N, const int* K, int* tiles_n, int* tiles_k, int* splits, int* rps, int x3 = 0) {
  const ConvKnobs::Once& k1 = ConvKnobs::once();
  int big = -1;
  long long tiles[WG_MAXG];
  int steps[WG_MAXG], max_steps = 1;
  for (int g = 0; g < n; ++g) {
    int sp, r, b;
    wgrad_plan(M[g], N[g], K[g], true, tiles_n[g], tiles_k[g], sp, r, b, n > 1 ? (k1.wgrad_big_minm ? atoi(k1.wgrad_big_minm) : 16384) : 49152, x3);
    if (big >= 0 && b != big) return -1;
    big = b;
    tiles[g] = (long long)tiles_n[g] * tiles_k[g];
    steps[g] = (M[g] + 63) / 64;
    if (steps[g] > max_steps) max_steps = steps[g];
  }
  const int slots = (big == 1 || big == 2) ? 256 : (k1.wgrad_slots ? atoi(k1.wgrad_slots) : 512);
  int T = 1;
  bool fits = false;
  for (; T <= max_steps; ++T) {
    long long tot = 0;
    for (int g = 0; g < n; ++g) tot += tiles[g] * ((steps[g] + T - 1) / T);
    if (tot <= slots) { fits = true; break; }
  }
  // more tiles than workgroup slots even with ONE split each (the X-layout tiles of the x3 mode are four times as many): a group would run
  // as several rounds of workgroups that each walk the whole pixel axis -- its members are better off alone, with their own splits
  if (!fits) { if (n > 1) return -1; T = max_steps; }
  if (x3 && n > 1) {
    // x3: a member often has so many tiles that the group gets one or two splits and fills the slots badly (4 tower filters = 144 big tiles:
    // one split each, 144 of 256 workgroup slots, 1 364 steps; alone each: 36 tiles x 7 splits = 252 slots, 195 steps).  Estimated duration
    // = rounds of the slots x steps per workgroup; group only if that does not lose against the members launched one by one.
    auto cost = [&](int g0, int g1) {
      long long best = -1;
      for (int t = 1; t <= max_steps; ++t) {
        long long tot = 0;
        for (int g = g0; g < g1; ++g) tot += tiles[g] * ((steps[g] + t - 1) / t);
        const long long c = ((tot + slots - 1) / slots) * t;
        if (best < 0 || c < best) best = c;
        if (tot <= slots / 2) break;         // (fewer workgroups than half the slots from here on: longer t only costs)
      }
      return best;
    };
    long long alone = 0;
    for (int g = 0; g < n; ++g) alone += cost(g, g + 1);
    const long long grouped = (long long)T;    // (one round by construction)
    if (grouped * 10 > alone * 11) return -1;
  }
  for (int g = 0; g < n; ++g) {
    rps[g] = T * 64;
    splits[g] = (M[g] + rps[g] - 1) / rps[g];
  }
  return big;
}

// dynamic LDS of an instance: two stages of 2 * tile sub-images (128 columns x 64 pixel rows, the wide forms 32, of 256 B), the 4096-byte ring
// of row records and, behind it, the block list of a SPARSE instance
constexpr int wgrad_lds_bytes(bool wide, int tile, bool sparse) {
  return 2 * (2 * tile) * (wide ? 32 : 64) * 256 + 4096 + (sparse ? WG_SLIST_BYTES : 0);
}
static_assert(wgrad_lds_bytes(false, 1, false) == 65536 + 4096 && wgrad_lds_bytes(true, 2, false) == 65536 + 4096 &&
              wgrad_lds_bytes(false, 1, true) == 65536 + 4096 + 8192 && wgrad_lds_bytes(true, 2, true) == 65536 + 4096 + 8192, "LDS of the 4-wave forms");
static_assert(wgrad_lds_bytes(false, 2, false) == 131072 + 4096 && wgrad_lds_bytes(true, 4, false) == 131072 + 4096 &&
              wgrad_lds_bytes(false, 2, true) == 131072 + 4096 + 8192 && wgrad_lds_bytes(true, 4, true) == 131072 + 4096 + 8192, "LDS of the big forms");

// THE decision: n members of (M, N, K) physical columns, all x3 or none; slabs = slab form (0: fp32 atomics, single launches only); grouped
// = the grouped launch and its cost model (which is not n > 1: one member may go through the group planner, with other splits than alone);
// has_map bit g = member g carries a usable row-activity map (wgrad_map).  Returns 1 when the members cannot share a grid.
static int wgrad_make_plan(int n, const int* M, const int* N, const int* K, int x3, bool slabs, bool grouped, unsigned has_map, WgradPlan& pl) {
  AOD_CHECK_ARG(slabs || !grouped, "wgrad: grouped launches exist in the slab form only");
  AOD_CHECK_ARG(slabs || !x3, "wgrad (x3): slab form only");
  memset(&pl, 0, sizeof(pl));
  int form;
  if (grouped) {
    form = wgrad_plan_group(n, M, N, K, pl.tiles_n, pl.tiles_k, pl.splits, pl.rows_per_split, x3);
    if (form < 0) return 1;
  } else wgrad_plan(M[0], N[0], K[0], slabs, pl.tiles_n[0], pl.tiles_k[0], pl.splits[0], pl.rows_per_split[0], form, 49152, x3);
  pl.form = form; pl.x3 = x3 ? 1 : 0; pl.grouped = grouped ? 1 : 0;
  pl.wide = form >= 2 ? 1 : 0;
  pl.tile = form == 2 ? 4 : (form ? 2 : 1);
  // waves: the big forms 8, the small x3 forms 4; the bf16 128 x 128 form 8, or 4 under AOD_WGRAD_W8=0 -- in SINGLE launches only: the
  // grouped wrapper has no 4-wave bf16 instance and always takes 8 (kept as it was)
  pl.waves = (form == 1 || form == 2) ? 8 : ((x3 || (!grouped && knob_is(ConvKnobs::once().wgrad_w8, '0'))) ? 4 : 8);
  // a map is followed by the x3 forms that have a SPARSE instance (all but the 256 x 256 form, reachable under AOD_WGRAD_X3_WIDE=0 only); a
  // group is sparse when any member has one -- the others pass a null zmap to the sparse instance
  pl.sparse = (x3 && form != 1 && has_map) ? 1 : 0;
  pl.threads = 64 * pl.waves;
  pl.lds_bytes = wgrad_lds_bytes(pl.wide, pl.tile, pl.sparse);
  for (int g = 0; g < n; ++g) pl.grid += pl.tiles_n[g] * pl.tiles_k[g] * pl.splits[g];
  return 0;
}

// every tile instance: (wide, NW, tile, X3, SPARSE, has a grouped wrapper) -- wide 0: conv_wgrad(_grouped)_kernel<NW, tile, tile, X3, SPARSE>,
// wide 1 (x3 only): conv_wgrad(_grouped)_x3w_kernel<NW, tile, SPARSE>.  The list is the launch switch.
#define WGRAD_INSTANCES(X)                                                                                                             \
  X(0, 4, 1, false, false, 0) /* bf16, AOD_WGRAD_W8=0: single launches only */                                                         \
  X(0, 8, 1, false, false, 1) X(0, 8, 2, false, false, 1)                                                                              \
  X(0, 4, 1, true, false, 1) X(0, 4, 1, true, true, 1) X(0, 8, 2, true, false, 1)                                                      \
  X(1, 4, 2, true, false, 1) X(1, 4, 2, true, true, 1) X(1, 8, 4, true, false, 1) X(1, 8, 4, true, true, 1)

// one instance through the single (P = WgradParams) or the grouped (P = WgradGroups) wrapper; its LDS attribute on first use per device
template <bool GROUPED, bool WIDE, int NW, int T, bool X3, bool SP, class P>
static int wgrad_launch_instance(const WgradPlan& pl, const P& p, hipStream_t st) {
  auto kernel = [] {
    if constexpr (WIDE && GROUPED) return &conv_wgrad_grouped_x3w_kernel<NW, T, SP>;
    else if constexpr (WIDE) return &conv_wgrad_x3w_kernel<NW, T, SP>;
    else if constexpr (GROUPED) return &conv_wgrad_grouped_kernel<NW, T, T, X3, SP>;
    else return &conv_wgrad_kernel<NW, T, T, X3, SP>;
  }();
  static unsigned long long attr_done = 0;
  if (aod_first_on_device(&attr_done))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, wgrad_lds_bytes(WIDE, T, SP));
  hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(pl.threads), pl.lds_bytes, st, p);
  AOD_LAUNCH_CHECK();
  return 0;
}

// plan -> launch.  A plan without an instance (in this wrapper) is an error, never another kernel.
template <bool GROUPED, class P>
static int wgrad_run(const WgradPlan& pl, const P& p, hipStream_t st) {
#define X(WIDE, NW, T, X3, SP, GRP)                                                                                                    \
  if constexpr (!GROUPED || GRP)                                                                                                       \
    if (pl.wide == WIDE && pl.waves == NW && pl.tile == T && (pl.x3 != 0) == X3 && (pl.sparse != 0) == SP)                             \
      return wgrad_launch_instance<GROUPED, WIDE, NW, T, X3, SP>(pl, p, st);
  WGRAD_INSTANCES(X)
#undef X
  AOD_CHECK_ARG(false, "wgrad: no kernel instance for the plan wide %d, %d waves, tile %d, x3 %d, sparse %d, grouped %d", pl.wide, pl.waves, pl.tile,
                pl.x3, pl.sparse, pl.grouped);
  return -1;
}

// the row-activity map of dZ a launch may follow (sparse backward), or nullptr: x3, dense dZ segments (GEMM row m IS dZ row m, which is how
// the map is indexed) and AOD_SPARSE_BWD not 0 (a per-call read: tests flip it in-process)
static const unsigned char* wgrad_map(const aod_conv_desc_t* d, const void* dz_map) {
  if (!dz_map || !d->x3) return nullptr;
  long long m = 0;
  for (int i = 0; i < d->nseg; ++i) {
    if (d->seg[i].dst_row0 != m) return nullptr;
    m += (long long)d->seg[i].B * d->seg[i].OH * d->seg[i].OW;
  }
  ConvKnobs kn;
  if (kn.is(ConvKnobs::SPARSE_BWD, '0')) return nullptr;
  return (const unsigned char*)dz_map;
}

// operands + geometry + map of one weight gradient (everything but the split plan)
static int wgrad_fill(const aod_conv_desc_t* d, const void* x, const void* dz, float* dw, const void* row_table, const void* dz_map, WgradParams& p) {
  AOD_CHECK_ARG(d && x && dz && dw && row_table, "wgrad: null pointer");
  AOD_CHECK_ARG(!d->transposed, "wgrad: descriptor must be the forward descriptor");
  AOD_CHECK_ARG(d->N % 8 == 0, "wgrad: N %d must be a multiple of 8 (pad dZ)", d->N);
  ConvKParams cp;
  memset(&cp, 0, sizeof(cp));
  int rc = fill_params(d, cp);
  if (rc) return rc;
  memset(&p, 0, sizeof(p));
  p.x = (const bf16_t*)x; p.dz = (const bf16_t*)dz; p.dw = dw; p.tab = (const RowRec*)row_table;
  p.C = cp.C; p.N = cp.N; p.K = cp.K; p.R = cp.R; p.S = cp.S; p.dil = cp.dil; p.M = cp.M; p.x3 = cp.x3;
  if (p.x3) AOD_CHECK_ARG(p.N % 64 == 0 && p.C % 64 == 0, "wgrad (x3): X-layout widths (dZ %d, x %d) must be multiples of 64", p.N, p.C);
  long long xrows = 0, zrows = 0;
  for (int i = 0; i < d->nseg; ++i) {
    const aod_conv_seg_t& sg = d->seg[i];
    AOD_CHECK_ARG(sg.src_row0 >= 0 && sg.dst_row0 >= 0, "wgrad: negative row offset");
    const long long e = sg.src_row0 + (long long)sg.B * sg.H * sg.W, ez = sg.dst_row0 + (long long)sg.B * sg.OH * sg.OW;
    if (e > xrows) xrows = e;
    if (ez > zrows) zrows = ez;
  }
  p.x_bytes = xrows * p.C * 2;
  p.z_bytes = zrows * p.N * 2;
  p.tab_bytes = (long long)p.M * (long long)sizeof(RowRec);
  AOD_CHECK_ARG(p.x_bytes < 0xe0000000ll && p.z_bytes < 0xe0000000ll, "wgrad: operand larger than 3.5 GiB (32-bit buffer offsets)");
  const ConvKnobs::Once& k1 = ConvKnobs::once();
  p.stagger = knob_is(k1.stagger, '0') ? 0 : 1;
  p.xcd_order = knob_is(k1.wgrad_xcd, '0') ? 0 : 1;
  p.zmap = p.M ? wgrad_map(d, dz_map) : nullptr;
  return 0;
}

// fill -> plan -> launch of n members: grouped = the grouped wrapper and its planner, else ONE member through the single wrapper (its
// slab_stride 0: fp32 atomics).  dz_map: null, or null entries, = dense members.
static int wgrad_launch(const aod_conv_desc_t* const* descs, int n, bool grouped, const void* const* x, const void* const* dz, float* const* dw,
                        const int32_t* nslabs, const int64_t* slab_stride, const void* const* row_table, const void* const* dz_map,
                        aod_stream_t stream) {
  WgradGroups gp;
  memset(&gp, 0, sizeof(gp));
  int M[WG_MAXG], N[WG_MAXG], K[WG_MAXG];
  unsigned has_map = 0;
  for (int g = 0; g < n; ++g) {
    int rc = wgrad_fill(descs[g], x[g], dz[g], dw[g], row_table[g], dz_map ? dz_map[g] : nullptr, gp.g[g]);
    if (rc) return rc;
    if (!grouped && gp.g[g].M == 0) return 0;
    AOD_CHECK_ARG(gp.g[g].M > 0, "wgrad_grouped: empty member");
    AOD_CHECK_ARG(gp.g[g].x3 == gp.g[0].x3, "wgrad_grouped: members of different precision modes");
    M[g] = gp.g[g].M; N[g] = gp.g[g].N; K[g] = gp.g[g].K;
    if (gp.g[g].zmap) has_map |= 1u << g;
  }
  const bool slabs = grouped || slab_stride[0] > 0;
  WgradPlan pl;
  int rc = wgrad_make_plan(n, M, N, K, gp.g[0].x3, slabs, grouped, has_map, pl);
  if (rc < 0) return rc;
  AOD_CHECK_ARG(rc == 0, "wgrad_grouped: the members take different tile forms (aod_conv2d_wgrad_group_plan tells)");
  int wg = 0;
  for (int g = 0; g < n; ++g) {
    WgradParams& p = gp.g[g];
    if (slabs) {
      AOD_CHECK_ARG(pl.splits[g] <= nslabs[g], "wgrad: member %d needs %d slabs, %d provided (aod_conv2d_wgrad_splits / _group_plan)", g, pl.splits[g], nslabs[g]);
      AOD_CHECK_ARG(slab_stride[g] >= (long long)p.N * p.K / (p.x3 ? 4 : 1), "wgrad: slab stride smaller than N*K (x3: the logical N/2 * K/2)");
    }
    p.tiles_n = pl.tiles_n[g]; p.tiles_k = pl.tiles_k[g]; p.splits = pl.splits[g]; p.rows_per_split = pl.rows_per_split[g];
    p.slab_stride = slab_stride[g];
    gp.wg0[g] = wg;
    wg += pl.tiles_n[g] * pl.tiles_k[g] * pl.splits[g];
  }
  for (int g = n; g <= WG_MAXG; ++g) gp.wg0[g] = g == n ? wg : 0x7fffffff;
  gp.n = n;
  return grouped ? wgrad_run<true>(pl, gp, (hipStream_t)stream) : wgrad_run<false>(pl, gp.g[0], (hipStream_t)stream);
}

// aod_conv2d_wgrad_grouped with the row-activity maps of the members' dZ (dz_map: n pointers, null entries = dense members; null: none)
extern "C" int aod_conv2d_wgrad_grouped_map(const aod_conv_desc_t* const* descs, int n, const void* const* x, const void* const* dz,
                                            float* const* slabs, const int32_t* nslabs, const int64_t* slab_stride,
                                            const void* const* row_table, const void* const* dz_map, aod_stream_t stream) {
  AOD_CHECK_ARG(descs && x && dz && slabs && nslabs && slab_stride && row_table && n >= 1 && n <= WG_MAXG, "wgrad_grouped: 1..4 members");
  return wgrad_launch(descs, n, true, x, dz, slabs, nslabs, slab_stride, row_table, dz_map, stream);
}

extern "C" int aod_conv2d_wgrad_grouped(const aod_conv_desc_t* const* descs, int n, const void* const* x, const void* const* dz,
                                        float* const* slabs, const int32_t* nslabs, const int64_t* slab_stride,
                                        const void* const* row_table, aod_stream_t stream) {
  return aod_conv2d_wgrad_grouped_map(descs, n, x, dz, slabs, nslabs, slab_stride, row_table, nullptr, stream);
}

// ... following the row-activity map of dZ (sparse backward; the x3 forms with a SPARSE instance -- other launches ignore it; null: aod_conv2d_wgrad_slabs)
extern "C" int aod_conv2d_wgrad_slabs_map(const aod_conv_desc_t* d, const void* x, const void* dz, float* slabs, int nslabs, int64_t slab_stride,
                                          const void* row_table, const void* dz_map, aod_stream_t stream) {
  AOD_CHECK_ARG(nslabs >= 1 && slab_stride > 0, "wgrad_slabs: nslabs / slab_stride");
  const int32_t ns = nslabs;
  return wgrad_launch(&d, 1, false, &x, &dz, &slabs, &ns, &slab_stride, &row_table, &dz_map, stream);
}

extern "C" int aod_conv2d_wgrad_slabs(const aod_conv_desc_t* d, const void* x, const void* dz, float* slabs, int nslabs, int64_t slab_stride,
                                      const void* row_table, aod_stream_t stream) {
  return aod_conv2d_wgrad_slabs_map(d, x, dz, slabs, nslabs, slab_stride, row_table, nullptr, stream);
}

extern "C" int aod_conv2d_wgrad(const aod_conv_desc_t* d, const void* x, const void* dz, float* dw, const void* row_table,
                                aod_stream_t stream) {
  const int32_t ns = 0;
  const int64_t atomics = 0;
  return wgrad_launch(&d, 1, false, &x, &dz, &dw, &ns, &atomics, &row_table, nullptr, stream);
}

// The plan as data (host logic, no device): what the launch of these descriptors with these flags would decide.  Every exported plan function
// goes through here (`who`: its name in the error texts).  Returns 1 when the members cannot share a grid (mixed precision modes or tile
// forms, or the cost rule prefers single launches).
static int wgrad_plan_descs(const aod_conv_desc_t* const* descs, int n, unsigned flags, const char* who, WgradPlan& pl) {
  AOD_CHECK_ARG(descs && n >= 1 && n <= WG_MAXG, "%s: 1..4 descriptors", who);
  int M[WG_MAXG], N[WG_MAXG], K[WG_MAXG];
  unsigned has_map = 0;
  static const char a_map = 0;          // stands for every map that is present: the plan looks at the pointer, never through it
  for (int g = 0; g < n; ++g) {
    AOD_CHECK_ARG(descs[g] && !descs[g]->transposed, "%s: forward descriptors", who);
    ConvKParams cp;
    memset(&cp, 0, sizeof(cp));
    int rc = fill_params(descs[g], cp);
    if (rc) return rc;
    AOD_CHECK_ARG(cp.M > 0, "%s: empty member", who);
    M[g] = cp.M; N[g] = cp.N; K[g] = cp.K;
    if (descs[g]->x3 != descs[0]->x3) return 1;      // (mixed precision modes never share a grid)
    if ((flags & AOD_WGRAD_HAS_MAP(g)) && wgrad_map(descs[g], &a_map)) has_map |= 1u << g;
  }
  return wgrad_make_plan(n, M, N, K, descs[0]->x3, !(flags & AOD_WGRAD_ATOMIC), n > 1 || (flags & AOD_WGRAD_GROUPED), has_map, pl);
}

extern "C" int aod_conv2d_wgrad_plan_ex(const aod_conv_desc_t* const* descs, int n, unsigned flags, aod_wgrad_plan_t* out) {
  AOD_CHECK_ARG(out, "wgrad_plan: null pointer");
  return wgrad_plan_descs(descs, n, flags, "wgrad_plan", *out);
}

// (the form of the plan before it carried the instance: n = 1 the single slab launch, n > 1 the group; kept for its callers)
extern "C" int aod_conv2d_wgrad_plan(const aod_conv_desc_t* const* descs, int n, int32_t* form, int32_t* splits_out, int32_t* rows_per_split) {
  AOD_CHECK_ARG(form && splits_out && rows_per_split, "wgrad_plan: null pointer");
  WgradPlan pl;
  const int rc = wgrad_plan_descs(descs, n, 0, "wgrad_plan", pl);
  if (rc) return rc;
  *form = pl.form;
  for (int g = 0; g < n; ++g) { splits_out[g] = pl.splits[g]; rows_per_split[g] = pl.rows_per_split[g]; }
  return 0;
}

extern "C" int aod_conv2d_wgrad_splits(const aod_conv_desc_t* d) {
  WgradPlan pl;
  if (!d || d->transposed || wgrad_plan_descs(&d, 1, 0, "wgrad_splits", pl)) return 0;
  return pl.splits[0];
}

extern "C" int aod_conv2d_wgrad_group_plan(const aod_conv_desc_t* const* descs, int n, int32_t* splits_out) {
  AOD_CHECK_ARG(splits_out, "wgrad_group_plan: 1..4 descriptors");
  WgradPlan pl;
  const int rc = wgrad_plan_descs(descs, n, AOD_WGRAD_GROUPED, "wgrad_group_plan", pl);
  if (rc) return rc;                           // (1: launch the members one by one)
  for (int g = 0; g < n; ++g) splits_out[g] = pl.splits[g];
  return 0;
}
