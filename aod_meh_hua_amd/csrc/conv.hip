// NHWC bf16 implicit-GEMM convolution for gfx950 (MI355X): forward, dgrad (same kernel,
// transposed tap map).  fp32 accumulate on v_mfma_f32_16x16x32_bf16.
//
// Forward / dgrad   D[m][n] = sum_k A[m][k] * Wp[n][k],  m = (segment, b, oy, ox) pixel of the
//   destination, k = (r, s, c) tap-major, A gathered on the fly from the NHWC source (im2col is
//   never materialised), Wp = packed [N][R][S][C] bf16.  256 threads = 4 waves (2x2); tile
//   BM x BN x 64; operands staged global -> VGPR -> LDS (XOR-swizzled 16-B chunks, conflict-free
//   ds_read_b128), double-buffered, one barrier per K-step; epilogue goes through LDS so that
//   every global store is a full 16-B-per-lane row segment (scale/shift/residual/mask/ReLU fused).
// Wgrad: conv_wgrad.hip (the weight packing, the unpack of its slabs and param_prep stay here).
#include "common.h"
#include "pointwise.h"
#include "conv_x3p.h"
#include "conv_params.h"

#ifdef AOD_TILE_TIMING
// debug build only (tools/dbg/tile_timing.py): per-workgroup wall-clock stamps (100 MHz) at the phase boundaries of the tile
__device__ unsigned long long* g_tile_stamps = nullptr;
extern "C" int aod_dbg_set_tile_stamps(void* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tile_stamps), &buf, sizeof(buf)); }
#define TSTAMP(k) do { if (g_tile_stamps && threadIdx.x == 0) g_tile_stamps[(size_t)blockIdx.x * 16 + (k)] = wall_clock64(); } while (0)
#else
#define TSTAMP(k) do {} while (0)
#endif

// block -> (tile, member) of a grouped launch of `ngroups` members of `nwg` tiles each; a bijection of [0, nwg * ngroups).
// mapped = 0 (no member carries a row-activity map): member-major over xcd_swizzle -- every XCD a contiguous range of tiles.
// mapped = 1: a member's LIVE tiles cluster (the positives sit on the coarse levels, the last quarter of the tile range), and a contiguous
// range per XCD hands them all to two of the eight XCDs, which then run as many rounds as the dense launch while the other six idle.  So the
// blocks are dealt (tile, member) with the member fastest and NO swizzle: consecutive tiles of one member then sit `ngroups` blocks apart,
// which walks all eight bid % 8 classes when ngroups is odd; when it is even they would stay on every other class (with two members: the dense
// member on the even classes only), so the member order turns by one with every eight blocks.  Any 64 consecutive tiles of a member put 8 +- 1
// on each class.  Placement only (which XCD runs a block is a speed heuristic): nothing depends on it for correctness.  (Measured, docs/LAB_NOTES.md
// section 22: the mapped forward runs in two thirds of the dense time; the paired dgrad stays within 4 % of its dense time under either order.)
// Since the list below this is the FALLBACK of mapped launches (AOD_TILE_ORDER=0, callers without a list): it levels the live blocks per XCD,
// not per CU -- a dead block takes a CU in dispatch order and leaves it empty behind it (section 23).
__host__ __device__ __forceinline__ void conv_grouped_deal(int bid, int nwg, int ngroups, int mapped, int& tile, int& group) {
  if (!mapped) {
    const int wg = xcd_swizzle(bid, nwg * ngroups);
    tile = wg % nwg; group = wg / nwg;
    return;
  }
  tile = bid / ngroups;
  const int turn = (ngroups & 1) ? 0 : (tile * ngroups) >> 3;
  group = (bid - tile * ngroups + turn) % ngroups;
}

// ---- the block order of a mapped grouped launch as a LIST (ConvKParams.order): which tiles are live is device data, so a small launch that
// reads the maps (tile_order_kernel, next to where they are written) builds, per launch, a permutation of the ngroups * nwg entries
// member * nwg + tile.  The entries are ranked member-major (member, then tile), the live ones (a member without a map: all of them) and
// the dead ones apart; conv_tile_order_slot is the rule that places them:
//   live entry of rank k  -> the block b with xcd_swizzle(b, nlive) = k: the live entries fill the blocks [0, nlive), every blockIdx % 8 class
//                            (XCD) takes a CONTIGUOUS range of the member-major ranking, nlive / 8 of them +- 1 -- one member's tiles follow
//                            each other inside a class, so an XCD is through with one packed filter before it touches the next
//   dead entry of rank k  -> block nlive + k: behind every live one, where its zero stores no longer stand in the dispatch order between them
__host__ __device__ __forceinline__ int conv_tile_live(const unsigned char* map, int tile_m, int bm, int M) {
  if (!map) return 1;
  const int m0 = tile_m * bm, mend = m0 + bm < M ? m0 + bm : M;
  int any = 0;
  for (int b = m0 >> 6; b <= (mend - 1) >> 6; ++b) any |= map[b];
  return any ? 1 : 0;
}
__host__ __device__ __forceinline__ int conv_tile_order_slot(int live, int rank, int nlive) {
  if (!live) return nlive + rank;
  const int q = nlive >> 3, r = nlive & 7, head = r * (q + 1);      // (the inverse of xcd_swizzle(., nlive))
  if (rank < head) { const int c = rank / (q + 1); return c + 8 * (rank - c * (q + 1)); }
  const int c = (rank - head) / q;                                   // (rank >= head with rank < nlive: q >= 1)
  return r + c + 8 * (rank - head - c * q);
}

// OPS: which optional epilogue operands the instance supports -- 0 none, 1 ReLU mask only, 2 residual and mask (their prefetch registers
// are what pushes the 8-wave form into spills, so it exists without them)
// X3: the REFERENCE-PRECISION form (fp32-equivalent products on the bf16 matrix pipe).  Every fp32 value v travels as a bf16 head and a
// bf16 tail, v ~= h + l (h = bf16(v), l = bf16(v - h): 16 significant bits), in the X-LAYOUT: a tensor of C logical channels has
// 2 * ceil32(C) bf16 columns, [h(0..31) | l(0..31) | h(32..63) | l(32..63) | ...].  A 64-column K-step of such an operand is then 32
// channels whose heads are k-block 0 and whose tails are k-block 1, for the activations and for the packed filters alike, and
//     x * w ~= xh * wh + xl * wh + xh * wl            (the dropped xl * wl is 2^-16 of the product)
// is THREE MFMAs on fragments the unmodified staging already put into the LDS (the plain form issues two per K-step): same tiles, same
// LDS-DMA gather, same barriers.  The epilogue computes in fp32 as before (BN / bias / residual = head + tail / mask / ReLU / column
// sums) and writes head and tail of each value, 64 B apart.  p.N stays the LOGICAL output channel count (vector operands, fp32
// destinations); p.C / p.K are the physical (X-layout) widths of the source and of the packed filter rows.
template <int BM, int BN, int NT, int OPS, bool GROUPED, int ST, bool X3>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(BM >= 192 ? 2 : (NT == 512 ? 4 : 1), BM >= 192 ? 2 : (NT == 512 ? 4 : 8)))) void conv_igemm_kernel(const ConvKParams p) {
  static_assert(NT == 256 || NT == 512, "4 or 8 waves");
  static_assert(ST == 2 || (ST == 3 && NT == 256), "LDS stages: 2, or 3 for the 4-wave forms");
  static_assert(!X3 || NT == 256 || (NT == 512 && (BM == 256 || BM == 192)), "X3: the 4-wave forms and the 8-wave 256 x 256 / 192 x 192 tiles");
  constexpr int BK = 64;
  constexpr int CPR = BK / 8;        // 16-B chunks per tile row
  constexpr int RPP = NT / CPR;      // tile rows covered per pass of the NT threads
  constexpr int A_IT = BM / RPP, B_IT = BN / RPP;
  constexpr int ROWB = BK * 2;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
  constexpr int WAVES_M = NT / 128;        // waves are laid out WAVES_M x 2
  constexpr int WM = BM / WAVES_M, WN = BN / 2;  // wave tile
  constexpr int MI = WM / 16, NI = WN / 16;
  constexpr int CP = BN + 4;               // fp32 epilogue pitch
  // the fp32 epilogue image of a 256 x 256 tile (266 KB) does not fit the LDS: it is written and stored in EP passes of EBM rows
  constexpr int EP = (BM * CP * 4 > 144 * 1024) ? 2 : 1;
  constexpr int EBM = BM / EP;
  constexpr bool PREFETCH = EP == 1 && !X3;       // residual / mask rows prefetched into registers before the K loop (not for the big tile: 16 x 8 regs; not in X3: twice the pieces)
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x;
  TSTAMP(0);
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = p.tiles_m * p.tiles_n;
  // class-major launches keep the round-robin block -> XCD assignment: the classes differ in work (1 / 2 / 2 / 4 taps of a 3x3, 1 / 0 / 0 / 0
  // of a 1x1) and contiguous per-XCD tile ranges would hand whole classes to single XCDs
  int wg;
  if (GROUPED && p.order) {
    // mapped grouped launch with a device-built order (conv_tile_order_slot): one scalar load; the entry decodes like a swizzled index below
    // (clamped: a list the builder has not written must not send a block outside the tensors)
    const unsigned e = (unsigned)p.order[blockIdx.x], last = (unsigned)(nwg * p.ngroups - 1);
    wg = (int)(e < last ? e : last);
  }
  else if (!p.perm) wg = xcd_swizzle(blockIdx.x, nwg * (GROUPED ? p.ngroups : p.ksplit));
  else if ((nwg & 31) == 0) {
    // ... but inside each quarter of the tile range (~ one class) every XCD still takes a contiguous chunk (neighbouring column tiles
    // share their A rows in that XCD's L2), and the quarters are interleaved in launch order
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3, q = j & 3, k = j >> 2, tq = nwg >> 2;
    wg = q * tq + x * (tq >> 3) + k;
  } else wg = blockIdx.x;
  // (grouped launches with a row-activity map, forward or dgrad: the even deal of conv_grouped_deal instead)
  int tile = wg % nwg, zz = wg / nwg;
  if (GROUPED && p.interleave && !p.order) conv_grouped_deal(blockIdx.x, nwg, p.ngroups, 1, tile, zz);
  const int kz = GROUPED ? 0 : zz;           // kz: which slice of the K-steps (split-K launches)
  // grouped launch: `ngroups` convolutions of identical geometry (the cls / reg / evidence towers at one depth) share one grid, so
  // that their tiles fill whole rounds of the CUs together; group = which operand set this workgroup uses
  const int gi = GROUPED ? zz : 0;
  // (constant indices only: a run-time index into the by-value argument struct would move the whole struct to scratch memory; the
  // selection exists in the GROUPED instances only -- in the 256 x 256 tile, which sits at the register cap, it costs ~15 %)
#define AOD_GSEL(f, dflt) (GROUPED ? (gi == 0 ? p.grp[0].f : (gi == 1 ? p.grp[1].f : (gi == 2 ? p.grp[2].f : p.grp[3].f))) : (dflt))
  const bf16_t* const g_x = AOD_GSEL(x, p.x);
  const bf16_t* const g_w = AOD_GSEL(w, p.w);
  const float* const g_shift = AOD_GSEL(pre_shift, p.pre_shift);
#define g_y AOD_GSEL(y, p.y)
#define g_mask AOD_GSEL(mask, p.mask)
#define g_colsum AOD_GSEL(colsum, p.colsum)
  const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  if constexpr (X3 && (GROUPED || NT == 256)) {      // (the towers' grouped big tile and the 4-wave forms: the plain 8-wave tiles never carry a map)
    // sparse backward: a tile that nothing but zero dZ rows can reach (the launcher: dense stride-1 dgrad, destination row = GEMM row, no bias /
    // residual, atomic column sums -- a zero tile adds nothing to them) loads no operand and runs no K-step: it stores its zero rows, heads and
    // tails, which the next dgrad reads as halo, and returns.  Workgroup-uniform: scalar loads of at most BM / 64 map bytes, one branch.
    // sparse forward (conv_fwd_map_setup): the same block with a map of where the OUTPUT is needed.  A dead tile stores ZERO rows, not
    // relu(bias): the wgrad and the next layer's halo read them against exact-zero gradients, and those rows must be finite.
    const unsigned char* const om = AOD_GSEL(omap, p.omap);
    if (om) {
      const int mend = m0 + BM < p.M ? m0 + BM : p.M;
      int any = 0;
      for (int b = m0 >> 6; b <= (mend - 1) >> 6; ++b) any |= om[b];
      if (!any) {
        const int NPz = ((p.N + 31) >> 5) << 6;
        const int c0 = 2 * n0, c1 = 2 * (n0 + BN) < NPz ? 2 * (n0 + BN) : NPz;      // (BN % 32 == 0: whole head | tail bands)
        const int cpr = (c1 - c0) >> 3, nch = (mend - m0) * cpr;
        bf16_t* const yz = reinterpret_cast<bf16_t*>(g_y) + (long long)m0 * NPz + c0;
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.f;
        for (int i = (int)threadIdx.x; i < nch; i += NT) {
          const int r = i / cpr, c = i - r * cpr;
          *reinterpret_cast<bf16x8*>(yz + (long long)r * NPz + c * 8) = z;
        }
#ifdef AOD_TILE_TIMING
        // a dead block: end stamp behind its acknowledged stores, where it ran, what it was (11: dead flag, 14: tile | member << 32)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        TSTAMP(6);
        if (g_tile_stamps && threadIdx.x == 0) {
          g_tile_stamps[(size_t)blockIdx.x * 16 + 7] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492);
          g_tile_stamps[(size_t)blockIdx.x * 16 + 11] = 1ull;
          g_tile_stamps[(size_t)blockIdx.x * 16 + 14] = ((unsigned long long)gi << 32) | (unsigned)tile;
          g_tile_stamps[(size_t)blockIdx.x * 16 + 15] = wall_clock64();
        }
#endif
        return;
      }
    }
  }
#ifdef AOD_TILE_TIMING
  if (m0 < 0) return;      // (forces the argument loads ahead of the stamp)
  TSTAMP(8);
#endif

  // ---- operand staging: LDS-DMA (buffer_load_dwordx4 ... lds), no VGPR round trip, no ds_write.
  // One wave-instruction fills 1 KiB = 8 tile rows x 8 chunks LINEARLY (lane l -> row l>>3, slot l&7); the
  // XOR swizzle that makes the ds_read_b128 fragment reads conflict-free is applied on the SOURCE side:
  // slot s of row r holds k-chunk s ^ ((r>>1)&7).  Out-of-image taps / K,N tails use an out-of-range
  // buffer offset, for which the hardware range check returns zeros (no select, no predication).
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  const int prow = lane >> 3;                       // row inside the wave's 8-row group
  const int kc = (lane & 7) ^ ((4 * uw + (lane >> 4)) & 7);   // k-chunk this lane fetches (same for every pass)
  const int C8 = p.C >> 3;
  const auto rsrc_x = buf_rsrc(g_x, (int)p.x_bytes);
  const auto rsrc_w = buf_rsrc(g_w, (int)p.w_bytes);
  constexpr unsigned OOB = 0xfffffff0u;

  unsigned rbase[A_IT];                             // byte offset of pixel (b, 0, 0) of the row's source block
  int ry0[A_IT], rx0[A_IT], rH[A_IT], rW[A_IT];
  // segment of a row: seg_mend[] is padded with M, so counting the boundaries <= m needs no loop.  Nearly every tile lies inside ONE
  // segment: its index is then workgroup-uniform and the geometry comes from scalar loads; only tiles that straddle a segment boundary
  // take the per-lane path, whose indexed loads from the argument buffer are a serial chain of vector-memory round trips
  auto seg_of = [&](int m) {
    int sg = 0;
    if (p.nseg > 1) {
#pragma unroll
      for (int q = 0; q < 7; ++q) sg += (m >= p.seg_mend[q]) ? 1 : 0;
    }
    return sg;
  };
  const int m_last = (m0 + BM < p.M ? m0 + BM : p.M) - 1;
  const int sg_first = seg_of(m0);
  const bool one_seg = sg_first == seg_of(m_last);
  struct Geo { unsigned mstart, OW, OH, ohw, B, H, W, src0b, imgb; };
  auto load_geo = [&](int sg) {
    Geo g;
    g.mstart = sg ? (unsigned)p.seg_mend[sg - 1] : 0u;
    g.OW = (unsigned)p.segOW[sg]; g.OH = (unsigned)p.segOH[sg]; g.ohw = g.OH * g.OW; g.B = (unsigned)p.segB[sg];
    g.H = (unsigned)p.segH[sg]; g.W = (unsigned)p.segW[sg];
    // byte offsets fit 32 bits (x_bytes < 3.5 GiB is checked on the host), so the arithmetic may wrap on the way
    g.src0b = (unsigned)((unsigned long long)p.seg_src0[sg] * (unsigned)(p.C * 2));
    g.imgb = g.H * g.W * (unsigned)(p.C * 2);
    return g;
  };
  const Geo gu = load_geo(sg_first);          // workgroup-uniform: scalar loads, once
  auto udiv = [&](unsigned n, unsigned d) { return p.bigrows ? n / d : udiv_small(n, d); };
  // (image, y, x) of the destination pixel with index ml inside its segment; `cls` = its (y & 1) * 2 + (x & 1) class in a class-major
  // launch (p.perm), where the segment's rows are ordered class 0 | class 1 | class 2 | class 3, each class image-major
  auto rowpos = [&](unsigned ml, const Geo& g, unsigned& b, unsigned& oy, unsigned& ox, int& cls) {
    if (!p.perm) {
      b = udiv(ml, g.ohw);
      const unsigned rem = ml - b * g.ohw;
      oy = udiv(rem, g.OW); ox = rem - oy * g.OW; cls = 0;
    } else {
      const unsigned H0 = (g.OH + 1) >> 1, H1 = g.OH >> 1, W0 = (g.OW + 1) >> 1, W1 = g.OW >> 1;
      const unsigned e0 = g.B * H0 * W0, e1 = e0 + g.B * H0 * W1, e2 = e1 + g.B * H1 * W0;
      cls = (ml >= e0 ? 1 : 0) + (ml >= e1 ? 1 : 0) + (ml >= e2 ? 1 : 0);
      const unsigned start = cls == 0 ? 0u : (cls == 1 ? e0 : (cls == 2 ? e1 : e2));
      const unsigned Hc = (cls & 2) ? H1 : H0, Wc = (cls & 1) ? W1 : W0, hw = Hc * Wc;
      const unsigned r = ml - start;
      b = udiv(r, hw);
      const unsigned rem = r - b * hw, yy = udiv(rem, Wc);
      oy = 2 * yy + (unsigned)(cls >> 1); ox = 2 * (rem - yy * Wc) + (unsigned)(cls & 1);
    }
  };
  const bool linear = one_seg && !p.perm && !p.up_w;       // destination rows of the tile are consecutive: drow = m + const
  // destination row of every tile row, parked in LDS behind the staging / epilogue area (read by the general epilogue, and by the
  // fast one on tiles that straddle a segment boundary)
  constexpr int EPI_BYTES = EBM * CP * 4;
  constexpr int DROW_OFF = (ST * STAGE > EPI_BYTES ? ST * STAGE : EPI_BYTES);
  long long* s_drow = reinterpret_cast<long long*>(smem + DROW_OFF);
  if (t < BM) {
    const int m = m0 + t;
    if (linear) s_drow[t] = p.seg_dst0[sg_first] + (long long)((unsigned)m - gu.mstart);
    else if (p.up_w) {          // (one segment: conv_params)
      unsigned b, oy, ox; int cls;
      rowpos((unsigned)m, gu, b, oy, ox, cls);
      s_drow[t] = p.seg_dst0[0] + (long long)b * p.up_hw + (long long)(2 * oy) * p.up_w + 2 * ox;
    }
    else if (!p.perm) { const int sg = m < p.M ? seg_of(m) : 0; s_drow[t] = p.seg_dst0[sg] + (m - (sg ? p.seg_mend[sg - 1] : 0)); }
    else {
      const int sg = one_seg ? sg_first : (m < p.M ? seg_of(m) : 0);
      const Geo g = one_seg ? gu : load_geo(sg);
      unsigned b, oy, ox; int cls;
      rowpos((unsigned)m - g.mstart, g, b, oy, ox, cls);
      s_drow[t] = p.seg_dst0[sg] + (long long)(b * g.ohw + oy * g.OW + ox);
    }
  }
  TSTAMP(10);
  // tap state of this lane's k-chunk
  const int nk_all = (p.K + BK - 1) / BK;
  const int kt_begin = (int)((long long)kz * nk_all / p.ksplit), kt_end = (int)((long long)(kz + 1) * nk_all / p.ksplit);
  int c8 = kc + kt_begin * CPR, tr = 0, ts = 0;
  if (c8 >= C8) { const int taps = c8 / C8; c8 -= taps * C8; tr = taps / p.S; ts = taps - tr * p.S; }

  unsigned wbase[B_IT];
#pragma unroll
  for (int i = 0; i < B_IT; ++i) {
    const int n = n0 + RPP * i + 8 * uw + prow;
    wbase[i] = n < p.N ? (unsigned)(((long long)n * p.K + kc * 8 + (long long)kt_begin * BK) * 2) : OOB;
  }

  // A-operand byte offsets are kept incrementally: inside one filter tap consecutive K-steps only advance the
  // channel offset by BK elements (and the validity of the tap does not change), so the full coordinate / bounds
  // computation runs once per tap instead of once per K-step.  Invalid rows park at BUF_OOB, which stays out of
  // range under the increments (x_bytes < BUF_OOB is checked on the host).
  const bool fast_tap = (C8 % CPR) == 0;          // then every lane of the block changes tap at the same K-step
  unsigned aoff[A_IT];
  unsigned woff[B_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) aoff[i] = BUF_OOB;
#pragma unroll
  for (int i = 0; i < B_IT; ++i) woff[i] = wbase[i] == OOB ? BUF_OOB : wbase[i];
  const int steps_per_tap = fast_tap ? C8 / CPR : 1;
  // taps that can reach this tile at all (class-major dgrad of a stride-2 conv: tap (r, s) only hits destination pixels with
  // y = r * dil - pad and x = s * dil - pad modulo 2); the others are skipped whole -- 5 to 8 of the 9 taps of a 3x3, 3 of 4 tiles
  // of a 1x1.  Rows are still checked one by one, so a tile that straddles two classes simply keeps every tap.
  unsigned long long tapmask = ~0ull;
  if (p.perm && fast_tap && one_seg) {
    unsigned b_, y_, x_; int c_first, c_last;
    rowpos((unsigned)m0 - gu.mstart, gu, b_, y_, x_, c_first);
    rowpos((unsigned)m_last - gu.mstart, gu, b_, y_, x_, c_last);
    if (c_first == c_last) {
      tapmask = 0ull;
      for (int r = 0; r < p.R; ++r)
        for (int q = 0; q < p.S; ++q)
          if ((((c_first >> 1) + p.pad - r * p.dil) & 1) == 0 && (((c_first & 1) + p.pad - q * p.dil) & 1) == 0) tapmask |= 1ull << (r * p.S + q);
    }
  }
  const bool skipping = tapmask != ~0ull;
  int kt_ld = kt_begin;                          // K-step the loaders fetch next
  // X3, TAPS INNERMOST.  In (tap, channel chunk) order a tile re-reads its pixel rows -- shifted by a pixel or a line -- once per tap,
  // C / 64 K-steps apart: 8 steps x 32 KB x 32 workgroups per XCD is twice the 4 MB L2, so every tap's re-read went out to the fabric (PMC:
  // 2 193 MB per grouped tower launch for 268 MB of activations, 8.2x).  In (channel chunk, tap) order the nine taps of a chunk follow each
  // other: the re-use distance is one K-step and the shifted rows are L2 / L1 hits.  Every K-step then changes the tap, so the incremental
  // offsets of the plain order do not apply: a row keeps its offset at tap (0, 0) and a validity bit per tap, a K-step adds the tap's
  // (workgroup-uniform per segment) displacement.  All x3 instances take this order (stride-1 forward / dgrad and strided forward; the
  // class-major stride-2 dgrad keeps the plain order with its tap skipping), so grouped and separate launches still agree bit for bit.
  const int ntaps = p.R * p.S;
  // (deep layers only: with C < 256 columns a tap is at most 3 K-steps long -- the re-reads are L2 hits already -- and the per-step offset
  // arithmetic shows: the 16-tap stem ran 13 % slower in this order)
  const bool tapin = X3 && p.tap_inner && !p.perm && !(p.transposed && p.stride != 1) && ntaps > 1 && ntaps <= 32 && p.C >= 256;
  int tp_tap = X3 ? kt_begin % ntaps : 0, tp_cc = X3 ? kt_begin / ntaps : 0;
  unsigned tbase[X3 ? A_IT : 1], tvm[X3 ? A_IT : 1], wb0[X3 ? B_IT : 1];
  int ksteps_in_tap = fast_tap ? kt_begin % steps_per_tap : 0;     // (a split-K slice may start inside a tap)
  bool new_tap = true;

  auto load_a = [&](int buf) {
    char* sa = smem + buf * STAGE;
    if constexpr (X3) {
      if (tapin) {
        const int trr = tp_tap / p.S, tss = tp_tap - trr * p.S;
        const int dy = trr * p.dil, dx = tss * p.dil;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
          const int d = (dy * rW[i] + dx) * p.C * 2;
          const unsigned off = ((tvm[i] >> tp_tap) & 1u) ? tbase[i] + (unsigned)(p.transposed ? -d : d) + (unsigned)tp_cc * (BK * 2) : BUF_OOB;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(sa + (RPP * i + 8 * uw) * ROWB), 16, off, 0, 0, 0);
        }
        return;
      }
    }
    if (new_tap) {
      const bool tapok = tr < p.R;
      const int dy = tr * p.dil, dx = ts * p.dil;
#pragma unroll
      for (int i = 0; i < A_IT; ++i) {
        int y, x;
        bool ok = tapok;
        if (p.transposed) {
          const int ty = ry0[i] - dy, tx = rx0[i] - dx;
          if (p.stride == 1) { y = ty; x = tx; }
          else { ok = ok && ((ty | tx) >= 0) && (ty % p.stride == 0) && (tx % p.stride == 0); y = ty / p.stride; x = tx / p.stride; }
        } else { y = ry0[i] + dy; x = rx0[i] + dx; }
        ok = ok && (unsigned)y < (unsigned)rH[i] && (unsigned)x < (unsigned)rW[i];
        aoff[i] = ok ? rbase[i] + (unsigned)(((y * rW[i] + x) * p.C + c8 * 8) * 2) : BUF_OOB;
      }
      new_tap = false;
    }
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const unsigned off = aoff[i];     // (a plain local: a subscript of a template-sized array is type-dependent and the host pass rejects it as a builtin argument)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (__attribute__((address_space(3))) void*)(sa + (RPP * i + 8 * uw) * ROWB), 16, off, 0, 0, 0);
    }
  };
  auto load_b = [&](int buf) {
    char* sb = smem + buf * STAGE + A_BYTES;
    if constexpr (X3) {
      if (tapin) {
        const unsigned kofs = (unsigned)((tp_tap * p.C + tp_cc * BK) * 2);
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
          const unsigned off = wb0[i] == OOB ? BUF_OOB : wb0[i] + kofs;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(sb + (RPP * i + 8 * uw) * ROWB), 16, off, 0, 0, 0);
        }
        return;
      }
    }
    const bool kok = (kt_ld * BK + kc * 8) < p.K;
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const unsigned off = kok ? woff[i] : BUF_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (__attribute__((address_space(3))) void*)(sb + (RPP * i + 8 * uw) * ROWB), 16, off, 0, 0, 0);
    }
  };
  auto skip_dead_taps = [&]() {      // (at a tap boundary) hop over the taps that cannot reach this tile
    while (tr < p.R && !((tapmask >> (tr * p.S + ts)) & 1ull)) {
      if (++ts == p.S) { ts = 0; ++tr; }
      kt_ld += steps_per_tap;
#pragma unroll
      for (int i = 0; i < B_IT; ++i) woff[i] += (unsigned)(p.C * 2);
    }
  };
  auto advance = [&]() {      // state of the next K-step
    if constexpr (X3) {
      if (tapin) {
        ++kt_ld;
        if (++tp_tap == ntaps) { tp_tap = 0; ++tp_cc; }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) woff[i] += BK * 2;
    c8 += CPR;
    ++kt_ld;
    if (fast_tap && ++ksteps_in_tap < steps_per_tap) {
#pragma unroll
      for (int i = 0; i < A_IT; ++i) aoff[i] += BK * 2;
    } else {
      ksteps_in_tap = 0;
      while (c8 >= C8) { c8 -= C8; if (++ts == p.S) { ts = 0; ++tr; } }
      new_tap = true;
      if (skipping) skip_dead_taps();
    }
  };
  auto gload = [&](int buf) { load_a(buf); load_b(buf); advance(); };
  if (skipping) skip_dead_taps();

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  TSTAMP(1);
  // epilogue operands (bias / scale vectors of this thread's 8 columns; residual and ReLU mask of its E_IT row segments): issued
  // together with the first operand tile and consumed after the main loop -- a load-use chain per store iteration would expose one
  // memory latency per 16 B and cap memory-bound layers at a third of the bandwidth
  constexpr int NCH = BN / 8;              // 8-column chunks per tile row
  // (thread -> chunk mapping over a power-of-two chunk count: the 192-column tile leaves a quarter of its epilogue lanes idle)
  constexpr int NCHT = (NCH & (NCH - 1)) == 0 ? NCH : (NCH <= 32 ? 32 : 64);
  static_assert((EBM * NCHT) % NT == 0 && NT % NCHT == 0, "epilogue mapping");
  constexpr int E_IT = EBM * NCHT / NT;    // row segments per thread and epilogue pass
  const int ec = t % NCHT, er = t / NCHT;
  const bool ecok = NCHT == NCH || ec < NCH;
  float cs1[8], cb1[8], cs2[8];
  bf16x8 pres[PREFETCH ? E_IT : 1], pmask[PREFETCH ? E_IT : 1];
  // LATE (the 4-wave X3 forms, which cannot spare the registers during the K loop): the same operands are fetched once the accumulators
  // sit in LDS, all E_IT row segments at once, ahead of the barrier.  Fetched inside the store loop, every iteration's load waited behind the
  // previous iteration's store (the two may alias as far as the compiler knows): one exposed memory latency per 16-B segment, 9.4 us of
  // a 22 us tile on the residual convs of the X3 backbone.  (Not the 256 x 256 tile: its second-pass accumulators are still live, it spills.)
  constexpr bool LATE = X3 && EP == 1;
  bf16x8 lres[LATE ? E_IT : 1], lrl[(LATE && X3) ? E_IT : 1], lmask[LATE ? E_IT : 1];
  // interior tiles of the common configuration (bf16 destination, N % 8 == 0, no post-scale / raw copy) take an epilogue without per-thread
  // predicates; inside one segment the destination rows are also linear in m (drow = m + drow_lin)
  const bool fast = !p.out_f32 && !p.zraw && !p.post_scale && (p.N & 7) == 0 && n0 + BN <= p.N && m0 + BM <= p.M;
  // destination row pitch and column of logical channel n (elements): X-layout for the bf16 destinations of an X3 launch
  const bool xout = X3 && !p.out_f32;
  const int NP = xout ? ((p.N + 31) >> 5) << 6 : p.N;
  auto xcol = [&](int n) { return xout ? ((n >> 5) << 6) + (n & 31) : n; };
  const long long drow_lin = linear ? p.seg_dst0[sg_first] - (long long)gu.mstart : 0;
  const long long lin_off = (drow_lin + m0 + er) * NP + xcol(n0 + ec * 8);     // element offset of this thread's first row segment
  const long long lin_step = (long long)(NT / NCHT) * NP;                // ... and the distance to its next one
  auto prefetch_epilogue = [&](bool from_table) {
    const int n = n0 + ec * 8;
    if (fast) {
      {
        // bias through a buffer descriptor that is EMPTY when there is no bias: the range check then returns zeros and the load needs
        // no branch (a branch would make the compiler wait for the loaded values where the two paths merge, i.e. right here)
        const auto rsrc_b = buf_rsrc(g_shift, g_shift ? p.N * 4 : 0);
        const auto rsrc_s = buf_rsrc(p.pre_scale, p.pre_scale ? p.N * 4 : 0);
        const u32x4 b0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, n * 4, 0, 0), b1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, n * 4 + 16, 0, 0);
        const u32x4 s0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc_s, n * 4, 0, 0), s1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc_s, n * 4 + 16, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cb1[j] = __uint_as_float(b0[j]); cb1[4 + j] = __uint_as_float(b1[j]);
          cs1[j] = __uint_as_float(s0[j]); cs1[4 + j] = __uint_as_float(s1[j]);       // (zeros without a scale vector: not used then)
        }
      }
      if (!from_table) {
        if (PREFETCH && OPS > 1 && p.res) {
#pragma unroll
          for (int it = 0; it < E_IT; ++it) pres[it] = *reinterpret_cast<const bf16x8*>(p.res + lin_off + it * lin_step);
        }
        if (PREFETCH && OPS > 0 && g_mask) {
#pragma unroll
          for (int it = 0; it < E_IT; ++it) pmask[it] = *reinterpret_cast<const bf16x8*>(g_mask + lin_off + it * lin_step);
        }
        return;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = n + j < p.N;
        cs1[j] = (p.pre_scale && ok) ? p.pre_scale[n + j] : 1.f;
        cb1[j] = (g_shift && ok) ? g_shift[n + j] : 0.f;
        cs2[j] = (p.post_scale && ok) ? p.post_scale[n + j] : 1.f;
      }
    }
    if (PREFETCH && OPS > 0 && (p.res || g_mask)) {
#pragma unroll
      for (int it = 0; it < E_IT; ++it) {
        const int row = er + it * (NT / NCHT);
        const bool ok = (m0 + row < p.M) && (n + 8 <= p.N);
        const long long drow = from_table ? s_drow[row] : drow_lin + m0 + row;
        const long long off = ok ? drow * NP + xcol(n) : 0;
        if (OPS > 1 && p.res && ok) pres[it] = *reinterpret_cast<const bf16x8*>(p.res + off);
        if (OPS > 0 && g_mask && ok) pmask[it] = *reinterpret_cast<const bf16x8*>(g_mask + off);
      }
    }
  };
  // first stage: the weight tile and the epilogue operands do not depend on the row decode -- they go out first and are in flight
  // while the rows are resolved
  bool have = __builtin_amdgcn_readfirstlane(kt_ld) < kt_end;     // (kt_ld is the same in every lane; say so, or the loop control goes through EXEC)                    // (a class without a reachable tap has no K-step at all: its dX is the epilogue of zero)
  if constexpr (X3) {
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int n = n0 + RPP * i + 8 * uw + prow;
      wb0[i] = n < p.N ? (unsigned)(((long long)n * p.K + kc * 8) * 2) : OOB;
    }
  }
  if (have) load_b(0);
  if (linear && p.ksplit == 1 && PREFETCH) prefetch_epilogue(false);
  {
    // Row decode: lane j of a wave resolves the wave's row j & 31 ONCE (source block, top-left tap, image size); the 8 lanes that
    // gather the 8 k-chunks of a row then pick the record up with a lane shuffle (decoding per lane repeated the two divisions of a
    // row 8 times, four rows per lane)
    const int j = lane & 31;
    const int m = m0 + RPP * (j >> 3) + 8 * uw + (j & 7);
    const int sg = one_seg ? sg_first : (m < p.M ? seg_of(m) : 0);
    const Geo gl = one_seg ? gu : load_geo(sg);
    unsigned b, oy, ox; int cls;
    rowpos((unsigned)m - gl.mstart, gl, b, oy, ox, cls);
    const int d_hw = m < p.M ? (int)(gl.H | (gl.W << 16)) : 0;     // rows past M keep H = W = 0: every tap of theirs is out of the image
    const int d_base = (int)(gl.src0b + b * gl.imgb);
    const int d_y = p.transposed ? (int)oy + p.pad : (int)oy * p.stride - p.pad;
    const int d_x = p.transposed ? (int)ox + p.pad : (int)ox * p.stride - p.pad;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int src = i * 8 + prow;
      const int hw = __shfl(d_hw, src);
      rbase[i] = (unsigned)__shfl(d_base, src); ry0[i] = __shfl(d_y, src); rx0[i] = __shfl(d_x, src);
      rH[i] = hw & 0xffff; rW[i] = (int)((unsigned)hw >> 16);
    }
    if constexpr (X3) {
      if (tapin) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
          tbase[i] = rbase[i] + (unsigned)(((ry0[i] * rW[i] + rx0[i]) * p.C + kc * 8) * 2);      // (modular: only used where the tap is valid)
          unsigned vm = 0;
          for (int tq = 0; tq < ntaps; ++tq) {
            const int r_ = tq / p.S, s_ = tq - r_ * p.S;
            const int y = p.transposed ? ry0[i] - r_ * p.dil : ry0[i] + r_ * p.dil, x = p.transposed ? rx0[i] - s_ * p.dil : rx0[i] + s_ * p.dil;
            vm |= ((unsigned)y < (unsigned)rH[i] && (unsigned)x < (unsigned)rW[i]) ? (1u << tq) : 0u;
          }
          tvm[i] = vm;
        }
      }
    }
  }
  TSTAMP(9);
  if (have) { load_a(0); advance(); }
  __syncthreads();
  if (!linear && p.ksplit == 1 && PREFETCH) prefetch_epilogue(true);     // destination rows are not consecutive: they come from the LDS table
  TSTAMP(2);
#ifdef AOD_TILE_TIMING
  if (g_tile_stamps && threadIdx.x == 0) g_tile_stamps[(size_t)blockIdx.x * 16 + 12] = __builtin_amdgcn_s_memtime();     // shader clock around the K loop
#endif
  const int lr = lane & 15, lq = lane >> 4;
  // STAGGER (8-wave forms): waves 4-7 share their SIMDs with waves 0-3 and run the same program -- in lockstep both waves of a SIMD issue
  // their LDS-DMA, then both read fragments, then both want the matrix pipe.  Waves 4-7 therefore run half a K-step late: the MFMAs
  // of the second k-block are carried across the barrier (their fragments are already in registers) and issued at the top of the next
  // iteration, while waves 0-3 issue their loads and fragment reads (MI355X_MICROARCH.md 'Two waves per SIMD', item 9).
  const bool late = p.stagger && NT == 512 && uw >= 4;
  bool carried = false;
  bf16x8 af[MI], bfr[NI];
  auto frag_read = [&](const char* sa, const char* sb, int ks) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = wm * WM + i * 16 + lr;
      af[i] = *reinterpret_cast<const bf16x8*>(sa + row * ROWB + (((ks * 4 + lq) ^ ((row >> 1) & 7)) << 4));
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int row = wn * WN + j * 16 + lr;
      bfr[j] = *reinterpret_cast<const bf16x8*>(sb + row * ROWB + (((ks * 4 + lq) ^ ((row >> 1) & 7)) << 4));
    }
  };
  auto mfma_block = [&]() {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
  };
  // one K-step.  Plain: the two 32-deep k-blocks.  X3: k-block 0 = heads, k-block 1 = tails of the same 32 channels -> xh*wh, xl*wh, xh*wl
  // (the tails of the activations are read while the head fragments stay in registers; the weight fragments are replaced last)
  // (`defer`: a late wave of the staggered 8-wave form leaves the LAST product of the step to the top of the next iteration, like the
  // plain form leaves its second k-block)
  auto kstep = [&](const char* sa, const char* sb, bool defer) {
    frag_read(sa, sb, 0);
    mfma_block();
    if constexpr (X3) {
      bf16x8 al[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wm * WM + i * 16 + lr;
        al[i] = *reinterpret_cast<const bf16x8*>(sa + row * ROWB + (((4 + lq) ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bfr[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int row = wn * WN + j * 16 + lr;
        bfr[j] = *reinterpret_cast<const bf16x8*>(sb + row * ROWB + (((4 + lq) ^ ((row >> 1) & 7)) << 4));
      }
      if (!defer) mfma_block();
    } else {
      frag_read(sa, sb, 1);
      if (!defer) mfma_block();
    }
  };
  if (ST == 3) {
    // Three-stage ring (4-wave forms whose K-step is shorter than a load: one stage ahead, every K-step waits out the rest of a
    // load latency).  Stage s + 2 is issued at step s, the wait before the barrier names how many younger LDS-DMA instructions may
    // stay in flight (stage s + 2's: A_IT + B_IT per wave; loads, stores and LDS-DMA complete in issue order), and the barrier is a raw
    // s_barrier -- a __syncthreads() drains the queue.  The barrier also says that every wave is done reading stage s, whose buffer
    // stage s + 3 overwrites one step later.  Same K order as the two-stage loop: identical results.
    constexpr int LPS = A_IT + B_IT;
    bool have1 = have && __builtin_amdgcn_readfirstlane(kt_ld) < kt_end;
    if (have1) gload(1);
    int cur = 0;
    while (have) {
      const bool more2 = have1 && __builtin_amdgcn_readfirstlane(kt_ld) < kt_end;
      if (more2) gload(cur == 0 ? 2 : cur - 1);
      const char* sa = smem + cur * STAGE;
      const char* sb = sa + A_BYTES;
      kstep(sa, sb, false);
      if (!have1) break;
      __builtin_amdgcn_sched_barrier(0);
      if (more2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      cur = cur == 2 ? 0 : cur + 1;
      have1 = more2;
    }
    __syncthreads();      // the epilogue image overlays the ring
  } else {
  for (int cur = 0; have; cur ^= 1) {
    const bool more = __builtin_amdgcn_readfirstlane(kt_ld) < kt_end;
    if (late && carried) mfma_block();
    if (more) gload(cur ^ 1);
    have = more;
    const char* sa = smem + cur * STAGE;
    const char* sb = sa + A_BYTES;
    static_assert(BK == 64, "two 32-deep k-blocks per K-step");
    if constexpr (X3) { kstep(sa, sb, late); carried = late; }
    else {
      frag_read(sa, sb, 0);
      mfma_block();
      frag_read(sa, sb, 1);
      if (!late) mfma_block(); else carried = true;
    }
    __syncthreads();   // hipcc drains the LDS-DMA (vmcnt(0)) ahead of the barrier: next tile is resident afterwards
  }
  if (late && carried) mfma_block();
  }

  if (p.ksplit > 1) {
    // split-K: this slice's fp32 partial tile goes to its own slab, straight from the accumulators (one dword per lane, 16
    // consecutive columns per row group); no atomics, so the finalize pass can add the slabs in a fixed order
    float* const slab = p.ws + (long long)kz * p.M * p.N;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * WM + i * 16 + lq * 4 + r, n = n0 + wn * WN + j * 16 + lr;
          if (m < p.M && n < p.N) slab[(long long)m * p.N + n] = acc[i][j][r];
        }
    return;
  }
  // ---- epilogue: accumulators -> LDS (fp32, [BM][CP]) -> row-major vector stores
#ifdef AOD_TILE_TIMING
  if (g_tile_stamps && threadIdx.x == 0) g_tile_stamps[(size_t)blockIdx.x * 16 + 13] = __builtin_amdgcn_s_memtime();
#endif
  TSTAMP(3);
  if (!PREFETCH) prefetch_epilogue(!linear);     // big tile: the bias / scale vectors are fetched after the K loop (16-24 registers it cannot spare)
  float* sc = reinterpret_cast<float*>(smem);
  float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ep = 0; ep < EP; ++ep) {
  const int r0e = ep * EBM;                  // first tile row of this pass
  if (EP > 1 && ep > 0) __syncthreads();     // the previous pass's image has been stored
  if (EP == 1 || (wm * WM) / EBM == ep) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sc[(wm * WM - r0e + i * 16 + lq * 4 + r) * CP + wn * WN + j * 16 + lr] = acc[i][j][r];
  }
  if (LATE && fast && OPS > 0 && ecok) {
#pragma unroll
    for (int it = 0; it < E_IT; ++it) {
      const long long eoff = linear ? lin_off + (long long)r0e * NP + it * lin_step : s_drow[r0e + er + it * (NT / NCHT)] * NP + xcol(n0 + ec * 8);
      if (OPS > 1 && p.res) {
        lres[it] = *reinterpret_cast<const bf16x8*>(p.res + eoff);
        if constexpr (X3) lrl[it] = *reinterpret_cast<const bf16x8*>(p.res + eoff + 32);
      }
      if (g_mask) lmask[it] = *reinterpret_cast<const bf16x8*>(g_mask + eoff);
    }
  }
  __syncthreads();
  TSTAMP(4);

  // fast tiles: no per-thread predicates at all, only workgroup-uniform branches -- the general loop below costs ~500 instructions
  // per 16-B store, this one under 100
  if (fast) {
    if (ecok) {
    bf16_t* const yb = reinterpret_cast<bf16_t*>(g_y) + xcol(n0 + ec * 8);
    bf16_t* const yl = reinterpret_cast<bf16_t*>(g_y) + lin_off + (long long)r0e * NP;
#pragma unroll
    for (int it = 0; it < E_IT; ++it) {
      const int row = er + it * (NT / NCHT);
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(sc + row * CP + ec * 8);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(sc + row * CP + ec * 8 + 4);
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = v0[j]; v[4 + j] = v1[j]; }
      if (p.pre_scale) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= cs1[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += cb1[j];
      const long long eoff = linear ? lin_off + (long long)r0e * NP + it * lin_step : s_drow[r0e + row] * NP + xcol(n0 + ec * 8);
      if (OPS > 1 && p.res) {
        const bf16x8 rv = PREFETCH ? pres[it] : (LATE ? lres[it] : *reinterpret_cast<const bf16x8*>(p.res + eoff));
        if constexpr (X3) {
          const bf16x8 rl = LATE ? lrl[it] : *reinterpret_cast<const bf16x8*>(p.res + eoff + 32);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += (float)rv[j] + (float)rl[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += (float)rv[j];
        }
      }
      if (OPS > 0 && g_mask) {
        const bf16x8 mv = PREFETCH ? pmask[it] : (LATE ? lmask[it] : *reinterpret_cast<const bf16x8*>(g_mask + eoff));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ((float)mv[j] > 0.f) ? v[j] : 0.f;
      }
      if (p.relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
      }
      bf16x8 ov;
#pragma unroll
      for (int j = 0; j < 8; ++j) { csum[j] += v[j]; ov[j] = (bf16_t)v[j]; }
      bf16_t* const yo = linear ? yl + it * lin_step : yb + s_drow[r0e + row] * NP;
      *reinterpret_cast<bf16x8*>(yo) = ov;
      if constexpr (X3) {
        bf16x8 ol;
#pragma unroll
        for (int j = 0; j < 8; ++j) ol[j] = (bf16_t)(v[j] - (float)ov[j]);
        *reinterpret_cast<bf16x8*>(yo + 32) = ol;
      }
    }
    }
  } else if (p.out_f32 && !p.res && !g_mask && !p.zraw && !p.post_scale && !p.pre_scale && (p.N & 3) == 0) {
    // fp32 destinations of the prediction convs (bias, optional ReLU, no other operand; N = 180 / 36 / 720 ...): rows and 4-column halves are
    // the only predicates -- the general loop below spends ~500 instructions per 16-B store on operands these launches do not have.
    // (v * 1 + bias of the general loop = v + bias: the same bits)
    const int n = n0 + ec * 8;
    if (ecok && n < p.N) {
      const bool hi = n + 8 <= p.N;                 // else columns n .. n + 3 only (N % 4 == 0)
      float* const yo = reinterpret_cast<float*>(g_y) + n;
#pragma unroll
      for (int it = 0; it < E_IT; ++it) {
        const int row = er + it * (NT / NCHT);
        if (m0 + r0e + row >= p.M) continue;
        f32x4 v0 = *reinterpret_cast<const f32x4*>(sc + row * CP + ec * 8);
        f32x4 v1 = *reinterpret_cast<const f32x4*>(sc + row * CP + ec * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v0[j] = v0[j] * 1.0f + cb1[j]; v1[j] = v1[j] * 1.0f + cb1[4 + j]; }
        if (p.relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { v0[j] = fmaxf(v0[j], 0.f); v1[j] = fmaxf(v1[j], 0.f); }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { csum[j] += v0[j]; if (hi) csum[4 + j] += v1[j]; }
        float* const o = yo + s_drow[r0e + row] * p.N;
        *reinterpret_cast<f32x4*>(o) = v0;
        if (hi) *reinterpret_cast<f32x4*>(o + 4) = v1;
      }
    }
  } else
#pragma unroll
  for (int it = 0; it < E_IT; ++it) {
    const int row = er + it * (NT / NCHT);
    const int m = m0 + r0e + row;
    const int n = n0 + ec * 8;
    if (m >= p.M || n >= p.N || !ecok) continue;
    const long long drow = s_drow[r0e + row];
    float v[8], raw[8];
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(sc + row * CP + ec * 8);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(sc + row * CP + ec * 8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = v0[j]; v[4 + j] = v1[j]; }
    const bool full = (n + 8 <= p.N);
#pragma unroll
    for (int j = 0; j < 8; ++j) raw[j] = v[j];
    if (full) {
      const long long off = drow * NP + xcol(n);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] * cs1[j] + cb1[j];
      if (OPS > 1 && p.res) {
        const bf16x8 rv = PREFETCH ? pres[it] : *reinterpret_cast<const bf16x8*>(p.res + off);
        if (xout) {
          // v + (head + tail), the association of the fast path above (and of the fused bottleneck kernels): a ragged tile must not round an
          // element differently from an interior one -- (v + head) + tail differs in the last bit for ~0.2 % of the elements, which made a
          // row's bits depend on where the tile boundaries fall (i.e. on the batch size)
          const bf16x8 rl = *reinterpret_cast<const bf16x8*>(p.res + off + 32);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += (float)rv[j] + (float)rl[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += (float)rv[j];
        }
      }
      if (OPS > 0 && g_mask) {
        const bf16x8 mv = PREFETCH ? pmask[it] : *reinterpret_cast<const bf16x8*>(g_mask + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ((float)mv[j] > 0.f) ? v[j] : 0.f;
      }
      if (p.post_scale) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= cs2[j];
      }
      if (p.relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) csum[j] += v[j];
      if (p.out_f32) {
        float* o = reinterpret_cast<float*>(g_y) + off;
        if ((p.N & 3) == 0) {
          *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(o + 4) = (f32x4){v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = v[j];
        }
      } else {
        bf16x8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[j] = (bf16_t)v[j];
        *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(g_y) + off) = ov;
        if (xout) {
          bf16x8 ol;
#pragma unroll
          for (int j = 0; j < 8; ++j) ol[j] = (bf16_t)(v[j] - (float)ov[j]);
          *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(g_y) + off + 32) = ol;
        }
      }
      if (p.zraw) {
        bf16x8 zv;
#pragma unroll
        for (int j = 0; j < 8; ++j) zv[j] = (bf16_t)raw[j];
        *reinterpret_cast<bf16x8*>(p.zraw + off) = zv;
      }
    } else {
      for (int j = 0; j < 8 && n + j < p.N; ++j) {
        const long long off = drow * p.N + n + j;
        float u = v[j];
        if (p.pre_scale) u *= p.pre_scale[n + j];
        if (g_shift) u += g_shift[n + j];
        if (p.res) u += (float)p.res[off];
        if (g_mask) u = ((float)g_mask[off] > 0.f) ? u : 0.f;
        if (p.post_scale) u *= p.post_scale[n + j];
        if (p.relu) u = fmaxf(u, 0.f);
        csum[j] += u;
        if (p.out_f32) reinterpret_cast<float*>(g_y)[off] = u;
        else reinterpret_cast<bf16_t*>(g_y)[off] = (bf16_t)u;
        if (p.zraw) p.zraw[off] = (bf16_t)raw[j];
      }
    }
  }
  }    // epilogue passes
  TSTAMP(5);
#ifdef AOD_TILE_TIMING
  __builtin_amdgcn_s_waitcnt(0);      // vmcnt/lgkmcnt 0: stores acknowledged
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TSTAMP(6);
  if (g_tile_stamps && threadIdx.x == 0)
    g_tile_stamps[(size_t)blockIdx.x * 16 + 7] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492);
#endif
  if (g_colsum) {
    // column sums of this tile: per-thread partials -> LDS [NT / NCHT][BN] -> one fp32 atomic per column
    __syncthreads();
    float* sr = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int j = 0; j < 8; ++j) if (ecok) sr[er * BN + ec * 8 + j] = csum[j];
    __syncthreads();
    if (t < BN && n0 + t < p.N) {
      float s = 0.f;
      for (int r = 0; r < NT / NCHT; ++r) s += sr[r * BN + t];
      if (p.cs_ws) p.cs_ws[((long long)gi * p.tiles_m + tile_m) * p.N + n0 + t] = s;
      else atomicAdd(g_colsum + n0 + t, s);
    }
  }
#ifdef AOD_TILE_TIMING
  // the block's last stamp, behind the column sums (15), and what it was (14: tile | member << 32)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (g_tile_stamps && threadIdx.x == 0) g_tile_stamps[(size_t)blockIdx.x * 16 + 14] = ((unsigned long long)gi << 32) | (unsigned)tile;
  TSTAMP(15);
#endif
}

#undef g_y
#undef g_mask
#undef g_colsum
#undef AOD_GSEL

template <int BM, int BN, int NT = 256, int OPS = 2, bool GROUPED = false, int ST = 2, bool X3 = false>
static int launch_conv(const ConvKParams& p, hipStream_t st) {
  ConvKParams q = p;
  q.tiles_m = (p.M + BM - 1) / BM;
  q.tiles_n = (p.N + BN - 1) / BN;
  const size_t stage = (size_t)(BM + BN) * 128 * ST;
  const size_t epi_full = (size_t)BM * (BN + 4) * 4;
  const size_t epi = epi_full > 144 * 1024 ? epi_full / 2 : epi_full;      // (two epilogue passes for the 256 x 256 tile)
  const size_t lds = (stage > epi ? stage : epi) + (size_t)BM * 8;     // staging | fp32 epilogue image, then the destination-row table
  static unsigned long long attr_done = 0;
  if (aod_first_on_device(&attr_done)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_kernel<BM, BN, NT, OPS, GROUPED, ST, X3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  // deterministic mode: partial column sums per (group, row tile) into the scratch, added in order below (a split-K launch has no epilogue
  // of its own: conv_splitk_finalize_kernel takes the scratch)
  bool any_cs = q.colsum != nullptr;
  if (GROUPED) for (int g = 0; g < q.ngroups; ++g) any_cs = any_cs || q.grp[g].colsum;
  const int ng = GROUPED ? q.ngroups : 1;
  if (q.ksplit == 1) q.cs_ws = any_cs ? aod_det_scratch((size_t)ng * q.tiles_m * q.N) : nullptr;
  hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, NT, OPS, GROUPED, ST, X3>), dim3(q.tiles_m * q.tiles_n * (q.ngroups > 1 ? q.ngroups : q.ksplit)), dim3(NT), lds, st, q);
  if (q.ksplit == 1 && q.cs_ws) {
    for (int g = 0; g < ng; ++g) {
      float* dst = GROUPED ? q.grp[g].colsum : q.colsum;
      if (dst) { const int rc = aod_colsum_finalize(q.cs_ws + (size_t)g * q.tiles_m * q.N, q.tiles_m, q.N, q.N, dst, nullptr, 0, st); if (rc) return rc; }
    }
  }
  return 0;
}

// Split-K second pass: the epilogue of conv_igemm_kernel applied to the fp32 sums in the workspace.  A block takes 8 GEMM rows x 256
// columns (thread -> one 8-column chunk of one row; the outputs are tiny, the grid has to be wide), column sums need one LDS
// reduction and 256 atomics per block.
__global__ __launch_bounds__(256) void conv_splitk_finalize_kernel(const ConvKParams p) {
  __shared__ float sr[8][256];
  const int t = threadIdx.x, ec = t & 31, er = t >> 5;
  const int n = (blockIdx.y * 32 + ec) * 8;
  float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float cs1[8], cb1[8], cs2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool ok = n + j < p.N;
    cs1[j] = (p.pre_scale && ok) ? p.pre_scale[n + j] : 1.f;
    cb1[j] = (p.pre_shift && ok) ? p.pre_shift[n + j] : 0.f;
    cs2[j] = (p.post_scale && ok) ? p.post_scale[n + j] : 1.f;
  }
  const bool vec = (p.N & 7) == 0 && n + 8 <= p.N;
  if (n < p.N) {
    for (int k = 0; k < 1; ++k) {
      const int m = blockIdx.x * 8 + er;
      if (m >= p.M) break;
      int sg = 0;
      if (p.nseg > 1) {
#pragma unroll
        for (int q = 0; q < 7; ++q) sg += (m >= p.seg_mend[q]) ? 1 : 0;
      }
      const long long drow = p.seg_dst0[sg] + (m - (sg ? p.seg_mend[sg - 1] : 0));
      const float* w = p.ws + (long long)m * p.N + n;
      float raw[8], v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[j] = 0.f;
      const long long slab = (long long)p.M * p.N;
      for (int z = 0; z < p.ksplit; ++z) {           // fixed order: the sum does not depend on which slice finished first
        if (vec) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(w + z * slab), b = *reinterpret_cast<const f32x4*>(w + z * slab + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { raw[j] += a[j]; raw[4 + j] += b[j]; }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) raw[j] += n + j < p.N ? w[z * slab + j] : 0.f;
        }
      }
      // (X3 launches with a bf16 destination: X-layout rows, heads and tails 32 columns apart)
      const bool xout = p.x3 && !p.out_f32;
      const int NP = xout ? ((p.N + 31) >> 5) << 6 : p.N;
      const long long off = drow * NP + (xout ? ((n >> 5) << 6) + (n & 31) : n);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (n + j >= p.N) { v[j] = 0.f; continue; }
        float u = raw[j] * cs1[j] + cb1[j];
        if (p.res) u += xout ? (float)p.res[off + j] + (float)p.res[off + 32 + j] : (float)p.res[off + j];
        if (p.mask) u = ((float)p.mask[off + j] > 0.f) ? u : 0.f;
        if (p.post_scale) u *= cs2[j];
        if (p.relu) u = fmaxf(u, 0.f);
        v[j] = u;
        csum[j] += u;
      }
      if (vec && !p.out_f32) {
        bf16x8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[j] = (bf16_t)v[j];
        *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(p.y) + off) = ov;
        if (xout) {
          bf16x8 ol;
#pragma unroll
          for (int j = 0; j < 8; ++j) ol[j] = (bf16_t)(v[j] - (float)ov[j]);
          *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16_t*>(p.y) + off + 32) = ol;
        }
      } else {
        for (int j = 0; j < 8 && n + j < p.N; ++j) {
          if (p.out_f32) reinterpret_cast<float*>(p.y)[off + j] = v[j];
          else reinterpret_cast<bf16_t*>(p.y)[off + j] = (bf16_t)v[j];
        }
      }
      if (p.zraw)
        for (int j = 0; j < 8 && n + j < p.N; ++j) p.zraw[off + j] = (bf16_t)raw[j];
    }
  }
  if (p.colsum) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sr[er][ec * 8 + j] = csum[j];
    __syncthreads();
    const int c = blockIdx.y * 256 + t;
    if (c < p.N) {
      float s2 = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) s2 += sr[r][t];
      if (p.cs_ws) p.cs_ws[(long long)blockIdx.x * p.N + c] = s2;
      else atomicAdd(p.colsum + c, s2);
    }
  }
}

// =====================================================================================
// forward / dgrad dispatch:  conv_params -> conv_plan -> conv_launch   (DESIGN.md "How a conv picks its kernel")
// =====================================================================================

// CU count of the current device, resolved once per device; 256 (the MI355X) when there is no device or the query fails
static int xp_cus() {
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return 256;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

// Split-K pays when the output is so small that whole tiles cannot fill the device: few tiles x very many K-steps (pyramid level P6:
// a stride-2 3x3 on the 2048-channel C5, 8 x 8 outputs per image; the 3x3 convs of the 16 x 16 backbone stage, K = 4608).  The decision and the slice boundaries depend on the PER-IMAGE
// geometry and on K only, never on the batch size: the fp32 summation order of an output element -- and so the score of an image --
// must not change with how the pool is batched.  Returns the number of K slices (1 = direct launch).
static int choose_ksplit(const ConvKParams& p) {
  const ConvKnobs::Once& k1 = ConvKnobs::once();
  const int nk = (p.K + 63) / 64;
  if (nk < 64) return 1;
  const long long maxhw = k1.ksplit_maxhw ? atoll(k1.ksplit_maxhw) : 256;
  long long rows16 = 0;                 // GEMM rows of a NOMINAL batch of 16 images (the batch size itself must not enter: see above)
  for (int i = 0; i < p.nseg; ++i) {
    if (p.segB[i] <= 0) continue;
    if ((long long)p.segOH[i] * p.segOW[i] > maxhw) return 1;
    rows16 += 16ll * p.segOH[i] * p.segOW[i];
  }
  if (k1.ksplit_steps) { const int per = atoi(k1.ksplit_steps); return nk / per > 1 ? nk / per : 1; }
  // as many slices as fill ONE round of two workgroups per CU with the split launch's 128-row tiles -- one slice more starts a second,
  // nearly empty round (P6 at 16 x 8 x 8: 36 slices 66.7 us, 24 slices 54.4 us) -- but no slice shorter than 8 K-steps
  const long long tiles = ((rows16 + 127) / 128) * ((p.N + 127) / 128);
  long long ks = 512 / (tiles > 0 ? tiles : 1);
  if (ks > nk / 8) ks = nk / 8;
  return ks > 1 ? (int)ks : 1;
}

static int conv_params(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst, const float* pre_scale,
                       const float* pre_shift, const void* res, const void* mask, const float* post_scale, void* zraw, float* colsum,
                       ConvKParams& p) {
  AOD_CHECK_ARG(desc && src && w_packed && dst, "conv: null pointer");
  memset(&p, 0, sizeof(p));
  int rc = fill_params(desc, p);
  if (rc) return rc;
  AOD_CHECK_ARG(!(desc->out_f32 && zraw), "conv: zraw needs a bf16 destination");
  if (desc->x3) {
    AOD_CHECK_ARG(!zraw && !post_scale, "conv (x3): zraw / post_scale are not supported");
    AOD_CHECK_ARG(desc->out_f32 || desc->N % 32 == 0, "conv (x3): a bf16 (X-layout) destination needs N %% 32 == 0, got %d", desc->N);
    AOD_CHECK_ARG(!(desc->out_f32 && (res || mask)), "conv (x3): residual / mask operands need an X-layout destination");
  }
  const ConvKnobs::Once& k1 = ConvKnobs::once();
  p.x = (const bf16_t*)src; p.w = (const bf16_t*)w_packed; p.y = dst;
  p.pre_scale = pre_scale; p.pre_shift = pre_shift; p.res = (const bf16_t*)res; p.mask = (const bf16_t*)mask;
  p.post_scale = post_scale; p.zraw = (bf16_t*)zraw; p.colsum = colsum;
  p.ksplit = 1;
  p.stagger = knob_is(k1.stagger, '0') ? 0 : 1;
  p.tap_inner = knob_is(k1.x3_taps_inner, '0') ? 0 : 1;
  p.perm = (desc->transposed && desc->stride == 2 && desc->R * desc->S > 1 && desc->R * desc->S <= 64) ? 1 : 0;     // (no gain measured for 1x1)
  // The dgrad of a 1x1 / stride-2 conv ACCUMULATED IN PLACE (res == dst, nothing else in the epilogue: the running sum of a gradient
  // junction, functional.GradAcc) only changes the (even, even) pixels of the destination: dX[b, 2y, 2x] += dZ[b, y, x] . W.  As a general
  // transposed launch it walks K for all four pixel classes and rewrites 4 x the rows (206 us for the layer-3 entry at 16 x 64 x 64 x 512
  // in the reference-precision mode); as a LATTICE launch it is a plain GEMM over the dZ pixels whose rows are stored two apart.
  if (desc->transposed && desc->stride == 2 && desc->R == 1 && desc->S == 1 && desc->pad == 0 && desc->nseg == 1 && res && res == dst &&
      !mask && !colsum && !pre_scale && !pre_shift && !post_scale && !zraw && !desc->relu && !desc->out_f32 && p.M > 0 &&
      !knob_is(k1.dgrad_lattice, '0')) {
    p.up_w = p.segOW[0]; p.up_hw = p.segOH[0] * p.segOW[0];
    p.segOH[0] = p.segH[0]; p.segOW[0] = p.segW[0];
    p.stride = 1;
    const long long m = (long long)p.segB[0] * p.segH[0] * p.segW[0];
    p.M = (int)m;
    for (int i = 0; i < 8; ++i) p.seg_mend[i] = (int)m;
    p.bigrows = m >= (1ll << 22) ? 1 : 0;
  }
  if (knob_is(k1.dgrad_classes, '0')) p.perm = 0;
  long long xrows = 0;
  for (int i = 0; i < desc->nseg; ++i) {
    const aod_conv_seg_t& sg = desc->seg[i];
    AOD_CHECK_ARG(sg.src_row0 >= 0, "conv: negative src_row0");
    const long long e = sg.src_row0 + (long long)sg.B * sg.H * sg.W;
    if (e > xrows) xrows = e;
  }
  p.x_bytes = xrows * p.C * 2;
  p.w_bytes = (long long)p.N * p.K * 2;
  AOD_CHECK_ARG(p.x_bytes < 0xe0000000ll && p.w_bytes < 0xe0000000ll, "conv: operand larger than 3.5 GiB (32-bit buffer offsets)");
  return 0;
}

// ... of a grouped launch (aod_conv2d_grouped): the descriptor with the operands of group 0, then grp[]
static int conv_params_grouped(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed, void* const* dst,
                               const float* const* pre_shift, const void* const* mask, float* const* colsum, ConvKParams& p) {
  AOD_CHECK_ARG(desc && src && w_packed && dst && ngroups >= 1 && ngroups <= 4, "conv_grouped: 1..4 groups");
  AOD_CHECK_ARG(!desc->out_f32, "conv_grouped: bf16 destinations only");
  AOD_CHECK_ARG(!desc->x3 || (desc->N % 256 == 0 && desc->R * desc->S * desc->C >= 2048), "conv_grouped (x3): N %% 256 == 0 and a deep K required");
  int rc = conv_params(desc, src[0], w_packed[0], dst[0], nullptr, pre_shift ? pre_shift[0] : nullptr, nullptr, mask ? mask[0] : nullptr, nullptr,
                       nullptr, colsum ? colsum[0] : nullptr, p);
  if (rc) return rc;
  AOD_CHECK_ARG(!p.perm, "conv_grouped: class-major stride-2 dgrad launches are not grouped");
  p.ngroups = ngroups;
  for (int g = 0; g < ngroups; ++g) {
    AOD_CHECK_ARG(src[g] && w_packed[g] && dst[g], "conv_grouped: null operand in group %d", g);
    p.grp[g].x = (const bf16_t*)src[g]; p.grp[g].w = (const bf16_t*)w_packed[g]; p.grp[g].y = dst[g];
    p.grp[g].pre_shift = pre_shift ? pre_shift[g] : nullptr;
    p.grp[g].mask = mask ? (const bf16_t*)mask[g] : nullptr;
    p.grp[g].colsum = colsum ? colsum[g] : nullptr;
  }
  return 0;
}

// ---- sparse backward: row-activity maps (one byte per 64 rows of a gradient row tensor; 0 = every row of the block is exactly zero).
// out[b] = OR of in[] over the dZ rows that the destination rows of block b can reach through the filter taps of a dense stride-1 dgrad: the
// linear range [first - up W - left, last + down W + right] of the segment, cut to the whole image rows and to the images the block touches.
struct MapGeo { int nseg, M, R, S, pad, dil; int segH[8], segW[8], seg_mend[8]; };
__device__ __forceinline__ unsigned char row_map_dilate_at(const unsigned char* in, int b, const MapGeo& g) {
  const int r0 = b << 6, r1 = r0 + 63 < g.M ? r0 + 63 : g.M - 1;
  const int up = (g.R - 1) * g.dil - g.pad, dn = g.pad, lf = (g.S - 1) * g.dil - g.pad, rt = g.pad;
  int any = 0;
  for (int sg = 0; sg < g.nseg; ++sg) {
    const int s0 = sg ? g.seg_mend[sg - 1] : 0, s1 = g.seg_mend[sg];
    const int lo = (r0 > s0 ? r0 : s0) - s0, hi = (r1 < s1 - 1 ? r1 : s1 - 1) - s0;
    if (lo > hi) continue;
    const int W = g.segW[sg], hw = g.segH[sg] * W;
    int a = lo - up * W - lf, z = hi + dn * W + rt;
    const int qa = (lo / W - up) * W, qz = (hi / W + dn + 1) * W - 1;
    a = a > qa ? a : qa; z = z < qz ? z : qz;
    const int ia = (lo / hw) * hw, iz = (hi / hw + 1) * hw - 1;
    a = a > ia ? a : ia; z = z < iz ? z : iz;
    for (int k = (s0 + a) >> 6; k <= (s0 + z) >> 6; ++k) any |= in[k];
  }
  return any ? 1 : 0;
}
__global__ __launch_bounds__(256) void row_map_dilate_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const MapGeo g) {
  const int b = (int)(blockIdx.x * 256 + threadIdx.x);
  if (b >= (g.M + 63) >> 6) return;
  out[b] = row_map_dilate_at(in, b, g);
}

// ---- sparse forward: the same maps, read the other way -- byte b = 1: some row of block b of a tower activation is NEEDED.  The box-regression
// and the MEH loss multiply by bbox_weights, which the assigner writes before the head runs and which is exactly 0 at every anchor that is not
// positive: level 0 of the chain marks the pixel blocks that hold a weighted anchor (pixel row p owns the A anchors A p .. A p + A - 1 of the
// level-major target rows), and every further level is the dilation above of the one before -- the MapGeo of a 3 x 3 / pad 1 conv is
// symmetric, so "the rows a dgrad reaches from block b" is also "the rows whose forward reads block b".  maps[k] = D^k(maps[0]).
struct FwdMapChain { unsigned char* m[8]; int n; };
__global__ __launch_bounds__(256) void fwd_row_map_kernel(const float* __restrict__ bw, unsigned char* __restrict__ out, long long rows, int fpr) {
  // one workgroup per block of 64 pixel rows: 64 * fpr contiguous floats (fpr = floats per pixel row, 4 * anchors: whole 16-B vectors)
  const long long r0 = (long long)blockIdx.x * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  const float4* const src = reinterpret_cast<const float4*>(bw + r0 * fpr);
  const int n4 = (int)((r1 - r0) * (fpr >> 2));
  int any = 0;
  for (int i = (int)threadIdx.x; i < n4; i += 256) {
    const float4 v = src[i];
    any |= (v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f) ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) out[blockIdx.x] = any ? 1 : 0;
}
// ONE workgroup walks the whole chain: level k reads level k - 1 behind a barrier.  LDS_BLOCKS > 0: the two levels in flight live in the LDS
// (a pyramid has ~1 400 blocks; a dependent global load per neighbour block and level made this launch 70 us), and every level is copied out
// as it completes; 0: maps of more than LDS_BLOCKS bytes, level by level through global memory.
template <int LDS_BLOCKS>
__global__ __launch_bounds__(1024) void fwd_map_chain_kernel(const FwdMapChain c, const MapGeo g) {
  const int nblk = (g.M + 63) >> 6;
  if constexpr (LDS_BLOCKS > 0) {
    __shared__ unsigned char buf[2][LDS_BLOCKS];
    for (int b = (int)threadIdx.x; b < nblk; b += 1024) buf[0][b] = c.m[0][b];
    __syncthreads();
    for (int k = 1; k < c.n; ++k) {
      const unsigned char* const in = buf[(k - 1) & 1];
      unsigned char* const out = buf[k & 1];
      for (int b = (int)threadIdx.x; b < nblk; b += 1024) {
        const unsigned char v = row_map_dilate_at(in, b, g);
        out[b] = v;
        c.m[k][b] = v;
      }
      __syncthreads();
    }
  } else {
    for (int k = 1; k < c.n; ++k) {
      for (int b = (int)threadIdx.x; b < nblk; b += 1024) c.m[k][b] = row_map_dilate_at(c.m[k - 1], b, g);
      __threadfence_block();
      __syncthreads();
    }
  }
}

// ---- the list of a mapped grouped launch (ConvKParams.order, conv_tile_order_slot).  ONE workgroup: (dgrad launches) first the dilation of
// every member's incoming map, in place of the row_map_dilate_kernel launches; then, over the entries e = member * tiles + tile in
// member-major order, the live count, and a block-wide scan that gives every entry its rank among the live or the dead ones.
struct TileOrderArgs {
  const unsigned char* omap[4];      // per member: the map that decides its tiles (null: every tile is live)
  const unsigned char* dil_in[4];    // per member, optional: dil_out = dilation of dil_in, written before the list
  unsigned char* dil_out[4];
  int* order;
  int ngroups, tiles_m, tiles_n, bm, M;
  int items;      // 1: the ITEM list of a mapped launch of the persistent kernel (conv_x3p.h): the ranking itself, live entries first -- the deal over
                  // the blockIdx % 8 classes is the kernel's slot rule (x3p_item_slot), not a property of the list
};
__host__ __device__ __forceinline__ int tile_order_place(const TileOrderArgs& a, int live, int rank, int nlive) {
  return a.items ? (live ? rank : nlive + rank) : conv_tile_order_slot(live, rank, nlive);
}
__host__ __device__ __forceinline__ int tile_order_live(const TileOrderArgs& a, int e) {
  const int nwg = a.tiles_m * a.tiles_n, g = e / nwg, tile_m = (e - g * nwg) / a.tiles_n;
  const unsigned char* const m = g == 0 ? a.omap[0] : (g == 1 ? a.omap[1] : (g == 2 ? a.omap[2] : a.omap[3]));
  return conv_tile_live(m, tile_m, a.bm, a.M);
}
__global__ __launch_bounds__(1024) void tile_order_kernel(const TileOrderArgs a, const MapGeo g) {
  __shared__ int wcnt[16];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nblk = (g.M + 63) >> 6;
  bool dilated = false;
  for (int m = 0; m < a.ngroups; ++m) {
    const unsigned char* const in = m == 0 ? a.dil_in[0] : (m == 1 ? a.dil_in[1] : (m == 2 ? a.dil_in[2] : a.dil_in[3]));
    unsigned char* const out = m == 0 ? a.dil_out[0] : (m == 1 ? a.dil_out[1] : (m == 2 ? a.dil_out[2] : a.dil_out[3]));
    if (!in) continue;
    dilated = true;
    for (int b = t; b < nblk; b += 1024) out[b] = row_map_dilate_at(in, b, g);
  }
  if (dilated) { __threadfence_block(); __syncthreads(); }
  const int total = a.ngroups * a.tiles_m * a.tiles_n;
  int nlive = 0;
  for (int base = 0; base < total; base += 1024) {
    const int e = base + t;
    nlive += __syncthreads_count(e < total && tile_order_live(a, e));
  }
  int live_before = 0;            // live entries in the chunks behind us
  for (int base = 0; base < total; base += 1024) {
    const int e = base + t;
    const int live = (e < total && tile_order_live(a, e)) ? 1 : 0;
    const unsigned long long bal = __ballot(live);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull)), chunk = 0;
    for (int w = 0; w < 16; ++w) { before += w < wave ? wcnt[w] : 0; chunk += wcnt[w]; }
    if (e < total) {
      const int rank = live ? live_before + before : (base - live_before) + (t - before);
      a.order[tile_order_place(a, live, rank, nlive)] = e;
    }
    live_before += chunk;
    __syncthreads();
  }
}
// the same list on the host (maps in host memory): aod_conv2d_tile_order
static void tile_order_host(const TileOrderArgs& a, int* order) {
  const int total = a.ngroups * a.tiles_m * a.tiles_n;
  int nlive = 0;
  for (int e = 0; e < total; ++e) nlive += tile_order_live(a, e);
  int nl = 0, nd = 0;
  for (int e = 0; e < total; ++e) {
    const int live = tile_order_live(a, e);
    order[tile_order_place(a, live, live ? nl : nd, nlive)] = e;
    (live ? nl : nd) += 1;
  }
}
// whether the launch takes a list: a caller's buffer, a map on some member, the 256 x 256 grouped tile, and not AOD_TILE_ORDER=0
static bool tile_order_applies(const ConvKParams& p, const ConvPlan& pl, const void* order) {
  if (!order || !p.interleave || pl.kind != AOD_CONV_PLAN_IGEMM || !pl.grouped || !pl.x3 || pl.bm != 256 || pl.bn != 256) return false;
  ConvKnobs kn;
  return !kn.is(ConvKnobs::TILE_ORDER, '0');
}
static int tile_order_launch(ConvKParams& p, const MapGeo& mg, int ngroups, const void* const* dil_in, void* const* dil_out, int* order, hipStream_t st) {
  TileOrderArgs a;
  memset(&a, 0, sizeof(a));
  for (int g = 0; g < ngroups; ++g) {
    a.omap[g] = p.grp[g].omap;
    if (dil_in && dil_in[g]) { a.dil_in[g] = (const unsigned char*)dil_in[g]; a.dil_out[g] = (unsigned char*)dil_out[g]; }
  }
  a.order = order; a.ngroups = ngroups; a.bm = 256; a.M = p.M;
  a.tiles_m = (p.M + 255) / 256; a.tiles_n = (p.N + 255) / 256;
  AOD_CHECK_ARG(((uintptr_t)order & 3) == 0, "conv (tile order): the list must be 4-byte aligned");
  hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, st, a, mg);
  AOD_LAUNCH_CHECK();
  p.order = order;
  return 0;
}

// ---- the mapped form of the persistent kernel (conv_x3p.hip): a PLAIN 3x3 dgrad that carries a map runs 128-column tiles -- a live row tile
// is N / 128 items of half a 256-column tile's matrix work -- in the order of an item list that the launch which dilates the map writes
// (tile_order_kernel, TileOrderArgs.items).  With 0.15 % of the anchors positive ~100 - 150 of the 682 row tiles of the bench's pyramid are
// live: the static walk of 256-column tiles gave a quarter of the workgroups one to three of them and the launch lasted as long as the
// unluckiest one; the list gives every workgroup ceil(live / G) items or one fewer.  AOD_X3P_MAPPED=0: the launch stays as planned.
static bool x3p_mapped_applies(const ConvKParams& p, const ConvPlan& pl, const void* order, int& grid) {
  if (!order || !p.omap || pl.kind != AOD_CONV_PLAN_X3P || pl.grouped || pl.taps != 9 || pl.lat != 0 || pl.pre != 0 || p.N % 128 != 0) return false;
  ConvKnobs kn;
  if (kn.is(ConvKnobs::X3P_MAPPED, '0')) return false;
  const int tiles_n = p.N / 128;
  grid = x3p_mapped_grid((long long)((p.M + XP_BM - 1) / XP_BM) * tiles_n, tiles_n, xp_cus());
  return grid > 0;
}
static int x3p_mapped_launch(ConvKParams& p, ConvPlan& pl, int grid, const MapGeo& mg, const void* dil_in, void* dil_out, int* order, hipStream_t st) {
  TileOrderArgs a;
  memset(&a, 0, sizeof(a));
  a.omap[0] = p.omap; a.dil_in[0] = (const unsigned char*)dil_in; a.dil_out[0] = (unsigned char*)dil_out;
  a.order = order; a.ngroups = 1; a.bm = XP_BM; a.M = p.M; a.items = 1;
  a.tiles_m = (p.M + XP_BM - 1) / XP_BM; a.tiles_n = p.N / 128;
  AOD_CHECK_ARG(((uintptr_t)order & 3) == 0, "conv (item list): the list must be 4-byte aligned");
  hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, st, a, mg);
  AOD_LAUNCH_CHECK();
  p.order = order;
  pl.wide = 0; pl.grid = grid;
  return 0;
}

// in_map[g] / out_map[g] of a (grouped) dgrad launch: writes every out_map from its in_map (a small launch of its own, ahead of the conv) and
// hands the conv kernel the OUT map of each member whose zero tiles are safe to skip.  ngroups = 0: the plain launch (p.omap).
// order (grouped launches of the 256 x 256 tile, optional): the list of the launch is built by the same small launch (tile_order_kernel).
static int conv_map_setup(ConvKParams& p, int ngroups, const void* const* in_map, void* const* out_map, hipStream_t st,
                          ConvPlan* pl = nullptr, int* order = nullptr) {
  const int ng = ngroups ? ngroups : 1;
  bool any = false;
  for (int g = 0; g < ng; ++g) {
    AOD_CHECK_ARG(!in_map[g] == !out_map[g], "conv (map): member %d needs both its incoming and its outgoing map, or neither", g);
    any = any || in_map[g];
  }
  if (!any || p.M == 0) return 0;
  AOD_CHECK_ARG(p.x3 && p.transposed && p.stride == 1 && !p.out_f32 && !p.perm && !p.up_w, "conv (map): row-activity maps exist for the x3 stride-1 dgrad with X-layout rows only");
  AOD_CHECK_ARG((p.R - 1) * p.dil >= p.pad && (p.S - 1) * p.dil >= p.pad, "conv (map): padding beyond the filter");
  MapGeo mg;
  memset(&mg, 0, sizeof(mg));
  mg.nseg = p.nseg; mg.M = p.M; mg.R = p.R; mg.S = p.S; mg.pad = p.pad; mg.dil = p.dil;
  for (int i = 0; i < p.nseg; ++i) {
    const long long m0 = i ? p.seg_mend[i - 1] : 0;
    AOD_CHECK_ARG(p.segH[i] == p.segOH[i] && p.segW[i] == p.segOW[i] && p.seg_src0[i] == m0 && p.seg_dst0[i] == m0,
                  "conv (map): segment %d is not a dense same-size map (dZ and dX rows must both be GEMM rows)", i);
    mg.segH[i] = p.segH[i]; mg.segW[i] = p.segW[i]; mg.seg_mend[i] = p.seg_mend[i];
  }
  const int nblk = (p.M + 63) >> 6;
  ConvKnobs kn;
  const bool dense = kn.is(ConvKnobs::SPARSE_BWD, '0');      // AOD_SPARSE_BWD=0: the maps are still written, no tile is skipped
  for (int g = 0; g < ng; ++g) {
    if (!in_map[g]) continue;
    // a skipped tile stores zeros and sends no column sums: only where the epilogue of a zero accumulator IS zero (no bias / scale / residual)
    // and the column sums are atomics (deterministic mode expects a partial row from every tile: it stays dense)
    const float* const shift = ngroups ? p.grp[g].pre_shift : p.pre_shift;
    float* const cs = ngroups ? p.grp[g].colsum : p.colsum;
    const bool skip_ok = !dense && !shift && !p.pre_scale && !p.res && !p.post_scale && !p.zraw && !(cs && aod_get_deterministic());
    if (!skip_ok) continue;
    if (ngroups) { p.grp[g].omap = (const unsigned char*)out_map[g]; p.interleave = 1; }
    else p.omap = (const unsigned char*)out_map[g];
  }
  // the maps themselves: one launch with the list of the conv launch behind them, or a launch per mapped member
  if (ngroups && pl && tile_order_applies(p, *pl, order)) return tile_order_launch(p, mg, ngroups, in_map, out_map, order, st);
  // (plain launch on the persistent kernel: the same launch writes the item list, and the plan becomes the 128-column form)
  int mgrid = 0;
  if (!ngroups && pl && x3p_mapped_applies(p, *pl, order, mgrid)) return x3p_mapped_launch(p, *pl, mgrid, mg, in_map[0], out_map[0], order, st);
  for (int g = 0; g < ng; ++g) {
    if (!in_map[g]) continue;
    hipLaunchKernelGGL(row_map_dilate_kernel, dim3((nblk + 255) / 256), dim3(256), 0, st, (const unsigned char*)in_map[g], (unsigned char*)out_map[g], mg);
    AOD_LAUNCH_CHECK();
  }
  return 0;
}

// the geometry the maps are defined on: x3, stride 1, same-size segments whose destination rows ARE the GEMM rows (a forward launch may
// gather its source levels from anywhere: only the rows it stores are skipped by map)
static int conv_map_geo(const ConvKParams& p, MapGeo& mg, bool dense_src) {
  AOD_CHECK_ARG(p.x3 && p.stride == 1 && !p.out_f32 && !p.perm && !p.up_w, "conv (map): row-activity maps exist for x3 stride-1 launches with X-layout rows only");
  AOD_CHECK_ARG((p.R - 1) * p.dil >= p.pad && (p.S - 1) * p.dil >= p.pad, "conv (map): padding beyond the filter");
  memset(&mg, 0, sizeof(mg));
  mg.nseg = p.nseg; mg.M = p.M; mg.R = p.R; mg.S = p.S; mg.pad = p.pad; mg.dil = p.dil;
  for (int i = 0; i < p.nseg; ++i) {
    const long long m0 = i ? p.seg_mend[i - 1] : 0;
    AOD_CHECK_ARG(p.segH[i] == p.segOH[i] && p.segW[i] == p.segOW[i] && (!dense_src || p.seg_src0[i] == m0) && p.seg_dst0[i] == m0,
                  "conv (map): segment %d is not a dense same-size map (the destination rows must be the GEMM rows)", i);
    mg.segH[i] = p.segH[i]; mg.segW[i] = p.segW[i]; mg.seg_mend[i] = p.seg_mend[i];
  }
  return 0;
}

// omap[g] of a grouped FORWARD launch (sparse forward): the READY-MADE map of where member g's output is needed (aod_fwd_row_maps; null = a
// dense member).  A dead tile stores zero rows whatever its bias.  The grouped forward has no residual, raw-sum (zraw) or fp32 destination,
// and a mapped launch may carry neither a mask nor column sums (both belong to dgrad epilogues): those stay forbidden here.
static int conv_fwd_map_setup(ConvKParams& p, int ngroups, const void* const* omap, hipStream_t st, const ConvPlan& pl, int* order) {
  bool any = false;
  for (int g = 0; g < ngroups; ++g) any = any || omap[g];
  if (!any || p.M == 0) return 0;
  AOD_CHECK_ARG(!p.transposed, "conv_grouped (forward map): a dgrad descriptor -- its maps go through aod_conv2d_grouped_map");
  AOD_CHECK_ARG(!p.pre_scale && !p.res && !p.post_scale && !p.zraw, "conv_grouped (forward map): scale / residual / raw-sum operands are not supported");
  for (int g = 0; g < ngroups; ++g)
    AOD_CHECK_ARG(!p.grp[g].mask && !p.grp[g].colsum, "conv_grouped (forward map): member %d carries a mask or column sums", g);
  MapGeo mg;
  const int rc = conv_map_geo(p, mg, false);
  if (rc) return rc;
  ConvKnobs kn;
  if (kn.is(ConvKnobs::SPARSE_FWD, '0')) return 0;      // AOD_SPARSE_FWD=0: the maps exist, no tile is skipped (and the launch keeps the unmapped deal)
  for (int g = 0; g < ngroups; ++g) p.grp[g].omap = (const unsigned char*)omap[g];
  p.interleave = 1;
  if (tile_order_applies(p, pl, order)) return tile_order_launch(p, mg, ngroups, nullptr, nullptr, order, st);
  return 0;
}

extern "C" size_t aod_conv2d_ws_bytes(const aod_conv_desc_t* desc) {
  ConvKParams p;
  memset(&p, 0, sizeof(p));
  if (!desc || fill_params(desc, p) != 0 || p.M == 0) return 0;
  const int ks = choose_ksplit(p);
  return ks > 1 ? (size_t)ks * p.M * p.N * 4 : 0;
}

// a 1x1 / stride-1 launch as the plain GEMM over consecutive rows that the streaming kernel (pointwise.hip) runs
static void pw_args(const ConvKParams& p, PwArgs& a) {
  const long long s0 = p.seg_src0[0], d0 = p.seg_dst0[0];
  a.x = p.x + s0 * p.C; a.w = p.w; a.y = reinterpret_cast<bf16_t*>(p.y) + d0 * p.N;
  a.pre_scale = p.pre_scale; a.pre_shift = p.pre_shift;
  a.res = p.res ? p.res + d0 * p.N : nullptr; a.mask = p.mask ? p.mask + d0 * p.N : nullptr; a.colsum = p.colsum;
  a.M = p.M; a.N = p.N; a.K = p.C; a.relu = p.relu;
}

// The persistent producer / consumer kernel's rules (conv_x3p.hip): true and out.taps / wide / pre / lat / grid filled when it takes the launch.
// ngroups = 0: a plain launch; det_colsum: a column-sum operand in deterministic mode.
static bool plan_x3p(const ConvKParams& p, int ngroups, bool det_colsum, ConvKnobs& kn, ConvPlan& out) {
  if (kn.is(ConvKnobs::X3P, '0')) return false;                      // AOD_X3P=0 keeps every launch on the general kernel
  const int taps = p.R * p.S, ng = ngroups > 1 ? ngroups : 1;
  if (taps != 1 && taps != 9) return false;
  if (taps == 9 && p.S != 3) return false;
  if (p.N % 128 != 0 || p.C % 64 != 0 || p.M <= 0) return false;
  // AOD_X3P_DGRAD=0 (parallel.GradSync sets it when gradients are all-reduced under the backward pass): backward launches stay with the general
  // kernel.  A persistent grid of one 160-KB-LDS workgroup per CU assumes every CU is free; RCCL's channel workgroups hold some for milliseconds,
  // and the workgroups that cannot start then run AFTER the others -- a one-round launch takes twice as long -- where the general kernel's many
  // small workgroups just lose those CUs' share.  Forward and scoring launches never run beside a collective.
  if (p.transposed && kn.is(ConvKnobs::X3P_DGRAD, '0')) return false;
  // (the class-major stride-2 dgrad and the in-place 1x1 / stride-2 dgrad as lattice launches of the persistent kernel: X3PArgs.lat)
  const int lat = ngroups ? 0 : (p.perm ? 1 : (p.up_w ? 2 : 0));
  if (lat && kn.is(ConvKnobs::X3P_LATTICE, '0')) return false;
  if (lat == 1) {
    // class-major stride-2 dgrad: 3x3, pad 1, no dilation, one segment with an even map whose halves are the dZ map
    if (!(p.transposed && p.stride == 2 && taps == 9 && p.pad == 1 && p.dil == 1 && p.nseg == 1)) return false;
    if ((p.segOH[0] & 1) || (p.segOW[0] & 1) || p.segH[0] * 2 != p.segOH[0] || p.segW[0] * 2 != p.segOW[0]) return false;
  } else if (lat == 2) {
    if (!(p.transposed && p.stride == 1 && taps == 1 && p.pad == 0 && p.nseg == 1 && p.up_w > 0)) return false;
  } else if (p.transposed && p.stride != 1) return false;
  if (det_colsum) return false;                        // ordered column sums stay with the general kernel (determinism.hip)
  if ((long long)p.K * 2 * p.N >= 0x7fffffffll) return false;
  // GEMM rows the launch tiles: the destination pixels, or (class-major form) the pixels of ONE of the four classes
  const long long rows = lat == 1 ? (long long)p.segB[0] * (p.segOH[0] / 2) * (p.segOW[0] / 2) : p.M;
  const long long tiles_m = (rows + XP_BM - 1) / XP_BM, reps = (long long)ng * (lat == 1 ? 4 : 1);
  // Operand-prefetch form (conv_x3p_kernel PRE): dense 1x1 launches with EXACTLY one of residual (-> 1) / ReLU mask (-> 2), else 0.
  // AOD_X3P_PRE=0 disables.
  int pre = 0;
  if (taps == 1 && lat == 0 && ngroups <= 1 && p.stride == 1 && (p.res != nullptr) != (p.mask != nullptr) && !kn.is(ConvKnobs::X3P_PRE, '0'))
    pre = p.res ? 1 : 2;
  // 256-column tiles (half the pixel bytes per MFMA, twice the MFMAs per barrier) when they still give at least three quarters of the CUs a
  // tile; AOD_X3P_BN=128 / 256 forces.  (Not with the prefetch form, which exists for the 128-column tile: 64 accumulators leave room for the operand)
  const int ncu = xp_cus();
  bool wide = false;
  if (!pre && p.N % 256 == 0) {
    const char* fbn = kn.call(ConvKnobs::X3P_BN);
    wide = fbn ? atoi(fbn) == 256 : tiles_m * (p.N / 256) * reps >= (long long)ncu * 3 / 4;
  }
  // a tile needs a K loop long enough to amortise the one-workgroup-per-CU structure (its epilogue runs beside nothing but the loaders' next
  // stages): from ~24 K-steps of a 128-column tile on the persistent form wins -- every 3x3 layer (36+ steps), the 1024 -> 256 reduce / lateral
  // 1x1 convs (32 steps: 37.0 -> 28.7 us), retina_cls' dgrad (54: 243 -> 230 us) -- and a 256-column tile's K-step carries twice the matrix
  // work per barrier, so 12 of those do (the 512 -> 256 lateral and the 512 -> 1024 stride-2 downsample conv: 57.7 -> 55.0, 57.0 -> 54.3 us).
  // Below that the general kernel's two workgroups per CU win (the expand 1x1 convs with their residual, 4 - 16 steps: 45.5 vs 49.9,
  // 34.0 vs 36.8 us; retina_reg / retina_L dgrads with 18 / 9 steps of a 128-column tile: 106 vs 116, 76 vs 88 us) -- a residual epilogue is
  // only taken from 24 steps on.  The class-major form is judged by its average class (9 taps over 4 classes).
  // profiles/r06_x3p_micro.txt; AOD_X3P_MIN_STEPS overrides the threshold.
  {
    const char* ms = kn.call(ConvKnobs::X3P_MIN_STEPS);
    const int thr = ms ? atoi(ms) : 24;
    const int steps = lat == 1 ? 9 * (p.C >> 6) / 4 : taps * (p.C >> 6);
    // (the operand-prefetch form does not change this: with the residual requested before the K loop the 8-step expand conv of
    // layer 3 still takes 49.5 us against the general kernel's 44.9 -- its K loop is bound by what 96 KB of ring can keep in flight against
    // the memory latency under the residual / store traffic, 1.08 us per K-step by the stamps -- and only the 4-step layer-2 expand conv wins,
    // 73.8 against 80.0 us; AOD_X3P_PRE_MIN_STEPS lowers the threshold for launches that qualify for the form)
    const char* pms = kn.call(ConvKnobs::X3P_PRE_MIN_STEPS);
    if (pms && pre) { if (steps < atoi(pms)) return false; }
    else if (lat != 1 && (steps * (wide ? 2 : 1) < thr || (p.res && steps < thr))) return false;
    if (lat == 1 && steps * (wide ? 2 : 1) < thr / 2) return false;          // (the general kernel's class-major launches are its slowest: 86 - 127 TFLOP/s)
  }
  long long prev = 0;
  for (int i = 0; i < p.nseg; ++i) {
    const long long r = p.seg_mend[i] - prev;
    prev = p.seg_mend[i];
    if (r >= (1ll << 22)) return false;                              // float-reciprocal row decode
    if (i + 1 < p.nseg && r % XP_BM != 0) return false;              // a tile must not straddle two segments
    if (p.seg_dst0[i] + r >= (1ll << 31)) return false;
  }
  // one 8-wave workgroup per CU: worth it from ~ a round of the chip on; below that the general kernel's smaller tiles fill more CUs
  const char* mint = kn.call(ConvKnobs::X3P_MIN_TILES);
  if (tiles_m * (p.N / 128) * reps < (mint ? atoll(mint) : 192)) return false;
  const long long ntiles = tiles_m * (p.N / (wide ? 256 : 128)) * reps;
  out.kind = AOD_CONV_PLAN_X3P;
  out.taps = lat == 1 ? 4 : taps;          // (the kernel's TAPS: the most taps a class of the class-major form has)
  out.wide = wide; out.pre = pre; out.lat = lat; out.x3 = 1; out.grouped = ngroups ? 1 : 0;
  out.grid = (int)(ntiles < ncu ? ntiles : ncu);
  return true;
}

// Which kernel a launch runs on.  Pure host logic: reads p (geometry, which operands are present, res == dst through up_w), the knobs, the
// deterministic flag, the pointwise mode and the CU count; enqueues and allocates nothing.  ngroups = 0: aod_conv2d(_ws); 1 .. 4:
// aod_conv2d_grouped (p.grp[] filled).
static int conv_plan(const ConvKParams& p, int ngroups, bool has_workspace, ConvPlan& out) {
  memset(&out, 0, sizeof(out));
  const ConvKnobs::Once& k1 = ConvKnobs::once();
  ConvKnobs kn;
  bool any_mask = p.mask != nullptr, any_cs = p.colsum != nullptr;
  for (int g = 0; g < ngroups; ++g) { any_mask = any_mask || p.grp[g].mask; any_cs = any_cs || p.grp[g].colsum; }
  auto igemm = [&](int bm, int bn, int nt, int ops, int stages) {
    out.kind = AOD_CONV_PLAN_IGEMM; out.bm = bm; out.bn = bn; out.nt = nt; out.ops = ops; out.stages = stages; out.x3 = p.x3; out.grouped = ngroups ? 1 : 0;
    return 0;
  };
  auto w8 = [&](int bm, int bn) { return igemm(bm, bn, 512, any_mask ? 1 : 0, 2); };      // the 8-wave forms: no residual, own instance with the mask
  auto ntiles = [&](int bm, int bn) { return (long long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  // The 256 x 256 tile (one 8-wave workgroup per CU, 128 FLOP per staged byte instead of 64, two epilogue passes) runs deep-K layers
  // 15-18 % faster per tile (tools/dbg/tile256.py: 794 -> 934 TFLOP/s on the FPN P3 shape) but one workgroup per CU quantises hard: it
  // is chosen only when its tiles fill whole rounds of the 256 CUs to >= 92 % (AOD_TILE_256=1 forces it in the plain form, =0 disables it).
  // X3: a K-step of the 128 x 128 tile asks the L2 -> LDS path for 64 KB per 1 536 matrix-pipe cycles per CU -- more than it delivers --, the
  // big tile for half of that.
  const long long t256 = ntiles(256, 256);
  const bool fits256 = t256 >= 240 && t256 * 100 >= ((t256 + 255) / 256) * 256 * 92;
  const bool shape256 = !p.res && !p.out_f32 && p.N % 256 == 0 && p.K >= (p.x3 ? 2048 : 1024);
  const long long want = k1.tile_want ? atoll(k1.tile_want) : 512;      // tiles that fill the device: >= 2 workgroups per CU (2 x 256)

  if (ngroups) {
    // the head towers' grouped launches CAN run on the persistent producer / consumer kernel (conv_x3p.hip, 128 x 256 tiles; identical bits):
    // AOD_X3P_GROUPED=1.  Not the default -- launch by launch the two forms are level (671 vs 689 us forward, 729 vs 725 us dgrad for three
    // groups at 16 x 512^2, profiles/r06_x3p_micro.txt; interleaved A/Bs: tools/dbg/x3p_grouped_micro.py) and inside the step the 256 x 256
    // tile is 0.3 - 0.5 ms ahead
    if (p.x3 && p.R == p.S && !p.bigrows && kn.is(ConvKnobs::X3P_GROUPED, '1') && plan_x3p(p, ngroups, any_cs && aod_get_deterministic(), kn, out)) return 0;
    if (p.x3) return w8(256, 256);          // x3 groups take the big tile (the 4-wave forms have no grouped instances)
    // the tile whose grouped tile count fills the CU rounds best: 256 x 256 at one workgroup per CU, else 128 x 128 on 8 waves at two
    auto fill = [&](int bm, int bn, int slots) {
      const long long t = ntiles(bm, bn) * ngroups;
      return (double)t / (double)(((t + slots - 1) / slots) * slots);
    };
    const bool ok256 = !knob_is(k1.tile_256, '0') && p.N % 256 == 0 && p.K >= 1024;
    if (ok256 && fill(256, 256, 256) * 1.12 >= fill(128, 128, 512)) return w8(256, 256);        // (the big tile is ~15 % faster per FLOP when its rounds are full)
    AOD_CHECK_ARG(p.N >= 128, "conv_grouped: N >= 128 required");
    return w8(128, 128);
  }

  // 1x1, stride 1: a plain GEMM over consecutive rows -- the persistent streaming kernel (pointwise.hip) when its launch heuristic wants it.
  // (aod_pw_wants asks aod_det_scratch(1), not the deterministic FLAG: the two differ when the mode is on and the scratch could not be
  // allocated -- the streaming kernel's atomics are then as good as the general kernel's fallback -- so the call stays as it is.)
  if (!p.x3 && !p.up_w && p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0 && p.nseg == 1 && !p.out_f32 && !p.zraw && !p.post_scale) {
    PwArgs a;
    pw_args(p, a);
    if (aod_pw_wants(a)) { out.kind = AOD_CONV_PLAN_PW_STREAM; return 0; }
  }
  const int ks = (has_workspace && !p.perm && !p.up_w) ? choose_ksplit(p) : 1;
  if (ks > 1) {
    igemm(128, p.N > 64 ? 128 : 64, 256, 2, 2);
    out.kind = AOD_CONV_PLAN_SPLIT_K; out.ksplit = ks;
    return 0;
  }
  if (p.x3) {
    // the persistent producer / consumer kernel (conv_x3p.hip) for the 128-column-tileable 1x1 / 3x3 layers that fill at least ~ a round of
    // the CUs with 128 x 128 tiles and do NOT qualify for the 256 x 256 tile (the head towers, FPN P3): identical bits, AOD_X3P=0 disables
    // (AOD_X3P_OVER_256=1, A/B: also take the launches of the 256 x 256 tile)
    if (!p.out_f32 && !p.zraw && !p.post_scale && !p.bigrows && p.R == p.S && (!(shape256 && fits256) || kn.is(ConvKnobs::X3P_OVER_256, '1')) &&
        plan_x3p(p, 0, any_cs && aod_get_deterministic(), kn, out)) return 0;
    if (!knob_is(k1.tile_256, '0') && shape256 && fits256) return w8(256, 256);
    // 129 .. 192 output columns without epilogue operands (retina_cls, 180 columns, fp32 destination): a 192 x 192 tile on eight waves, one
    // workgroup per CU like the 256 x 256 tile (96 FLOP per staged byte; 64-wide tiles: 43, and the L2 -> LDS path bounds the 4-wave x3
    // forms), same K order -> same bits.  AOD_X3_TILE_192=0: the 128 x 64 tile.
    if (p.N > 128 && p.N <= 192 && !p.res && !p.mask && !p.zraw && p.K >= 2048 && ntiles(192, 192) >= 240 && !kn.is(ConvKnobs::X3_TILE_192, '0'))
      return igemm(192, 192, 512, 0, 2);
  } else {
    if (!knob_is(k1.tile_256, '0') && shape256 && ((knob_is(k1.tile_256, '1') && t256 >= 128) || fits256)) return w8(256, 256);
    // deep convs without a residual operand (forward and dgrad of the head towers, the 3x3 of the backbone): the 128 x 128 tile on 8
    // waves -- four waves per SIMD hide more of the K loop's waits than two (-4 % on the head-tower shape); with the residual's prefetch
    // registers as well the 8-wave form spills and loses
    if (!knob_is(k1.tile_w8, '0') && !p.res && p.N >= 128 && p.K >= 1024 && ntiles(128, 128) >= want) return w8(128, 128);
  }
  // the 4-wave forms: the largest tile that still fills the device; else the most workgroups
  // a ragged last column tile (N = 180 -> 128 + 52) wastes MFMA work; 64-wide tiles trim it (192 instead of 256 columns)
  const int pad128 = (p.N + 127) / 128 * 128, pad64 = (p.N + 63) / 64 * 64;
  const bool ragged = p.N > 128 && (pad128 - pad64) * 5 >= pad128;
  // (three LDS stages for the 64-row tiles -- x3: always; plain: when the K loop is long enough to matter, AOD_RING3=0 disables; the 128 x 64
  // tile keeps two -- three stages cost it its third workgroup per CU: 61 -> 69 us on the narrow prediction convs; the 128 x 128 tile too --
  // three stages = 96 KB = one workgroup per CU: measured +0.55 ms per step; 64 x 128 x 3 stages instead: +0.3 ms)
  const int st64 = (p.x3 || (!knob_is(k1.ring3, '0') && p.K >= 256)) ? 3 : 2;
  if (ragged && ntiles(128, 64) >= want) return igemm(128, 64, 256, 2, 2);
  if (p.N > 64 && ntiles(128, 128) >= want) return igemm(128, 128, 256, 2, 2);
  if (p.N > 64 && ntiles(64, 128) >= want) return igemm(64, 128, 256, 2, st64);
  if (p.N <= 64 && ntiles(128, 64) >= want) return igemm(128, 64, 256, 2, 2);
  if (p.N > 64 && ntiles(128, 64) >= want && p.N % 128 != 0) return igemm(128, 64, 256, 2, 2);
  return igemm(64, 64, 256, 2, st64);
}

// operands / geometry of a launch in the persistent kernel's terms (conv_x3p.hip)
static void x3p_args(const ConvKParams& p, const ConvPlan& plan, X3PArgs& a) {
  memset(&a, 0, sizeof(a));
  a.x = p.x; a.w = p.w; a.y = reinterpret_cast<bf16_t*>(p.y); a.pre_scale = p.pre_scale; a.pre_shift = p.pre_shift; a.res = p.res; a.mask = p.mask;
  a.colsum = p.colsum; a.C = p.C; a.N = p.N; a.K = p.K; a.taps = p.R * p.S; a.S = p.S; a.stride = p.stride; a.pad = p.pad; a.dil = p.dil;
  a.transposed = p.transposed; a.relu = p.relu; a.nseg = p.nseg; a.M = p.M; a.x_bytes = p.x_bytes; a.w_bytes = p.w_bytes;
  a.tapin = (p.tap_inner && a.taps > 1 && p.C >= 256) ? 1 : 0;      // the general kernel's K order for this shape (see `tapin` there)
  for (int i = 0; i < 8; ++i) {
    a.segH[i] = p.segH[i]; a.segW[i] = p.segW[i]; a.segOH[i] = p.segOH[i]; a.segOW[i] = p.segOW[i]; a.segB[i] = p.segB[i];
    a.seg_src0[i] = p.seg_src0[i]; a.seg_dst0[i] = p.seg_dst0[i]; a.seg_mend[i] = p.seg_mend[i];
  }
  // the kernel reads its operands from grp[]: the groups of a grouped launch, else the one set above
  a.ngroups = p.ngroups > 1 ? p.ngroups : 1;
  a.grp[0].x = a.x; a.grp[0].w = a.w; a.grp[0].y = a.y; a.grp[0].shift = a.pre_shift; a.grp[0].mask = a.mask; a.grp[0].colsum = a.colsum;
  // maps: the 256-column 3x3 instance follows them under its static walk; the 128-column one only as the mapped form, with its item list
  // (x3p_mapped_launch) -- a 128-column launch without a list stays dense
  a.order = (!plan.wide && p.ngroups <= 1) ? p.order : nullptr;
  const bool maps = plan.wide || a.order;
  a.grp[0].omap = maps ? p.omap : nullptr;
  for (int g = 0; g < p.ngroups; ++g) {
    a.grp[g].x = p.grp[g].x; a.grp[g].w = p.grp[g].w; a.grp[g].y = reinterpret_cast<bf16_t*>(p.grp[g].y); a.grp[g].shift = p.grp[g].pre_shift;
    a.grp[g].mask = p.grp[g].mask; a.grp[g].colsum = p.grp[g].colsum; a.grp[g].omap = maps ? p.grp[g].omap : nullptr;
  }
  a.lat = plan.lat; a.up_w = p.up_w; a.up_hw = p.up_hw;
  const long long rows = a.lat == 1 ? (long long)a.segB[0] * (a.segOH[0] / 2) * (a.segOW[0] / 2) : a.M;
  a.tiles_m = (int)((rows + XP_BM - 1) / XP_BM);
  a.tiles_n = a.N / (plan.wide ? 256 : 128);
}

// every instance of conv_igemm_kernel: (BM, BN, NT, OPS, GROUPED, ST, X3) -- the list is the launch switch
#define CONV_IGEMM_INSTANCES(X)                                                                                                       \
  X(256, 256, 512, 0, false, 2, false) X(256, 256, 512, 1, false, 2, false) X(128, 128, 512, 0, false, 2, false) X(128, 128, 512, 1, false, 2, false) \
  X(128, 128, 256, 2, false, 2, false) X(128, 64, 256, 2, false, 2, false) X(64, 128, 256, 2, false, 2, false) X(64, 128, 256, 2, false, 3, false)   \
  X(64, 64, 256, 2, false, 2, false) X(64, 64, 256, 2, false, 3, false)                                                               \
  X(256, 256, 512, 0, true, 2, false) X(256, 256, 512, 1, true, 2, false) X(128, 128, 512, 0, true, 2, false) X(128, 128, 512, 1, true, 2, false)    \
  X(256, 256, 512, 0, false, 2, true) X(256, 256, 512, 1, false, 2, true) X(192, 192, 512, 0, false, 2, true)                          \
  X(128, 128, 256, 2, false, 2, true) X(128, 64, 256, 2, false, 2, true) X(64, 128, 256, 2, false, 3, true) X(64, 64, 256, 2, false, 3, true)      \
  X(256, 256, 512, 0, true, 2, true) X(256, 256, 512, 1, true, 2, true)

static int launch_igemm(const ConvPlan& pl, const ConvKParams& p, hipStream_t st) {
#define X(BM, BN, NT, OPS, GROUPED, ST, X3)                                                                                           \
  if (pl.bm == BM && pl.bn == BN && pl.nt == NT && pl.ops == OPS && (pl.grouped != 0) == GROUPED && pl.stages == ST && (pl.x3 != 0) == X3) \
    return launch_conv<BM, BN, NT, OPS, GROUPED, ST, X3>(p, st);
  CONV_IGEMM_INSTANCES(X)
#undef X
  AOD_CHECK_ARG(false, "conv: no kernel instance for the plan %d x %d, %d threads, ops %d, %d stages, x3 %d, grouped %d", pl.bm, pl.bn, pl.nt, pl.ops,
                pl.stages, pl.x3, pl.grouped);
  return -1;
}

// plan -> launch(es).  A plan without a kernel instance is an error, never another kernel.
static int conv_launch(const ConvPlan& pl, ConvKParams& p, void* workspace, size_t workspace_bytes, hipStream_t st) {
  switch (pl.kind) {
    case AOD_CONV_PLAN_PW_STREAM: {
      PwArgs a;
      pw_args(p, a);
      return aod_pw_gemm(a, st);
    }
    case AOD_CONV_PLAN_X3P: {
      X3PArgs a;
      x3p_args(p, pl, a);
      ConvKnobs kn;
      const char* r = kn.call(ConvKnobs::X3P_ROT);
      a.rot = r ? atoi(r) : 0;
      return aod_conv_x3p_launch(a, pl, st);
    }
    case AOD_CONV_PLAN_SPLIT_K: {
      const size_t need = (size_t)pl.ksplit * p.M * p.N * 4;
      AOD_CHECK_ARG(workspace && workspace_bytes >= need, "conv: split-K workspace of %zu bytes, need %zu (aod_conv2d_ws_bytes)", workspace_bytes, need);
      p.ksplit = pl.ksplit; p.ws = (float*)workspace;
      p.omap = nullptr;                    // (a K slice has no epilogue of its own: split launches stay dense)
      int rc = launch_igemm(pl, p, st);
      if (rc) return rc;
      AOD_LAUNCH_CHECK();
      p.cs_ws = p.colsum ? aod_det_scratch((size_t)((p.M + 7) / 8) * p.N) : nullptr;
      hipLaunchKernelGGL(conv_splitk_finalize_kernel, dim3((p.M + 7) / 8, (p.N + 255) / 256), dim3(256), 0, st, p);
      AOD_LAUNCH_CHECK();
      if (p.cs_ws) return aod_colsum_finalize(p.cs_ws, (p.M + 7) / 8, p.N, p.N, p.colsum, nullptr, 0, st);
      return 0;
    }
    case AOD_CONV_PLAN_IGEMM: {
      int rc = launch_igemm(pl, p, st);
      if (rc) return rc;
      AOD_LAUNCH_CHECK();
      return 0;
    }
  }
  AOD_CHECK_ARG(false, "conv: plan of unknown kind %d", pl.kind);
  return -1;
}

// aod_conv2d_ws with the row-activity maps of the sparse backward (x3 stride-1 dgrad; both null: the plain launch)
// order (optional): int32 [ceil(rows / 128) * N / 128], device memory -- a mapped 3x3 launch of the persistent kernel then takes its
// 128-column form and follows the item list that the map's launch writes there (x3p_mapped_launch); null, or AOD_X3P_MAPPED=0: as planned
extern "C" int aod_conv2d_ws_map_order(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst,
                                       const float* pre_scale, const float* pre_shift, const void* res, const void* mask,
                                       const float* post_scale, void* zraw, float* colsum, void* workspace, size_t workspace_bytes,
                                       const void* in_map, void* out_map, void* order, aod_stream_t stream) {
  ConvKParams p;
  ConvPlan pl;
  int rc = conv_params(desc, src, w_packed, dst, pre_scale, pre_shift, res, mask, post_scale, zraw, colsum, p);
  if (rc) return rc;
  if (p.M == 0) return 0;
  rc = conv_plan(p, 0, workspace != nullptr, pl);
  if (rc) return rc;
  rc = conv_map_setup(p, 0, &in_map, &out_map, (hipStream_t)stream, &pl, (int*)order);
  if (rc) return rc;
  return conv_launch(pl, p, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int aod_conv2d_ws_map(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst,
                                 const float* pre_scale, const float* pre_shift, const void* res, const void* mask,
                                 const float* post_scale, void* zraw, float* colsum, void* workspace, size_t workspace_bytes,
                                 const void* in_map, void* out_map, aod_stream_t stream) {
  return aod_conv2d_ws_map_order(desc, src, w_packed, dst, pre_scale, pre_shift, res, mask, post_scale, zraw, colsum, workspace, workspace_bytes,
                                 in_map, out_map, nullptr, stream);
}

// The item list of a mapped launch of the persistent kernel as data (host logic only; the ranking is the one tile_order_kernel runs, the deal
// the kernel's x3p_item_slot): `rows` GEMM rows, `tiles_n` = N / 128 column tiles, a grid of `grid` workgroups (x3p_mapped_grid), map = a HOST
// copy of the row-activity map ((rows + 63) / 64 bytes).  item[pos] = tile_m * tiles_n + tile_n of list position pos, block[pos] / round[pos] =
// the workgroup that runs it and as which of its items, pos < ceil(rows / 128) * tiles_n.
extern "C" int aod_conv2d_x3p_item_order(int rows, int tiles_n, int grid, const void* map, int32_t* item, int32_t* block, int32_t* round) {
  AOD_CHECK_ARG(rows >= 1 && tiles_n >= 1 && map && item && block && round, "conv_x3p_item_order: rows %d, tiles_n %d", rows, tiles_n);
  const int tiles_m = (rows + XP_BM - 1) / XP_BM, ntiles = tiles_m * tiles_n;
  AOD_CHECK_ARG(grid >= 1 && grid <= ntiles && grid % (8 * tiles_n) == 0, "conv_x3p_item_order: a grid of %d for %d tiles in %d columns", grid, ntiles, tiles_n);
  TileOrderArgs a;
  memset(&a, 0, sizeof(a));
  a.omap[0] = (const unsigned char*)map;
  a.ngroups = 1; a.bm = XP_BM; a.M = rows; a.tiles_m = tiles_m; a.tiles_n = tiles_n; a.items = 1;
  tile_order_host(a, item);
  for (int pos = 0; pos < ntiles; ++pos) { block[pos] = x3p_slot_block(pos % grid, tiles_n); round[pos] = pos / grid; }
  return 0;
}
// ... and the grid of that launch on a device of `cus` compute units (0: too few tiles for the deal, the launch keeps its planned form)
extern "C" int aod_conv2d_x3p_mapped_grid(int rows, int tiles_n, int cus) {
  AOD_CHECK_ARG(rows >= 1 && tiles_n >= 1 && cus >= 1, "conv_x3p_mapped_grid: rows %d, tiles_n %d, cus %d", rows, tiles_n, cus);
  return x3p_mapped_grid((long long)((rows + XP_BM - 1) / XP_BM) * tiles_n, tiles_n, cus);
}

extern "C" int aod_conv2d_ws(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst,
                             const float* pre_scale, const float* pre_shift, const void* res, const void* mask,
                             const float* post_scale, void* zraw, float* colsum, void* workspace, size_t workspace_bytes,
                             aod_stream_t stream) {
  return aod_conv2d_ws_map(desc, src, w_packed, dst, pre_scale, pre_shift, res, mask, post_scale, zraw, colsum, workspace, workspace_bytes, nullptr,
                           nullptr, stream);
}

// aod_conv2d_grouped with per-member row-activity maps (in_map / out_map: arrays of ngroups pointers, null entries = dense members; both
// arrays null: the plain launch)
// order (optional): int32 [ngroups * tiles of 256 rows * tiles of 256 columns], device memory -- where the launch carries a map and runs the
// 256 x 256 tile, the small launch that writes the maps also writes the block order of the launch there (conv_tile_order_slot) and the
// kernel follows it; null, or AOD_TILE_ORDER=0: the fixed deal (conv_grouped_deal)
extern "C" int aod_conv2d_grouped_map_order(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed,
                                            void* const* dst, const float* const* pre_shift, const void* const* mask, float* const* colsum,
                                            const void* const* in_map, void* const* out_map, void* order, aod_stream_t stream) {
  ConvKParams p;
  ConvPlan pl;
  int rc = conv_params_grouped(desc, ngroups, src, w_packed, dst, pre_shift, mask, colsum, p);
  if (rc) return rc;
  if (p.M == 0) return 0;
  rc = conv_plan(p, ngroups, false, pl);
  if (rc) return rc;
  AOD_CHECK_ARG(!in_map == !out_map, "conv_grouped (map): incoming and outgoing maps come together");
  if (in_map) {
    rc = conv_map_setup(p, ngroups, in_map, out_map, (hipStream_t)stream, &pl, (int*)order);
    if (rc) return rc;
  }
  return conv_launch(pl, p, nullptr, 0, (hipStream_t)stream);
}

extern "C" int aod_conv2d_grouped_map(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed,
                                      void* const* dst, const float* const* pre_shift, const void* const* mask, float* const* colsum,
                                      const void* const* in_map, void* const* out_map, aod_stream_t stream) {
  return aod_conv2d_grouped_map_order(desc, ngroups, src, w_packed, dst, pre_shift, mask, colsum, in_map, out_map, nullptr, stream);
}

extern "C" int aod_conv2d_grouped(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed,
                                  void* const* dst, const float* const* pre_shift, const void* const* mask, float* const* colsum,
                                  aod_stream_t stream) {
  return aod_conv2d_grouped_map(desc, ngroups, src, w_packed, dst, pre_shift, mask, colsum, nullptr, nullptr, stream);
}

// aod_conv2d_grouped, forward, with a ready-made row-activity map per member (omap: ngroups pointers, null entries = dense members)
// (order: as in aod_conv2d_grouped_map_order; the list is built by a small launch ahead of the conv)
extern "C" int aod_conv2d_grouped_fwd_map_order(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed,
                                                void* const* dst, const float* const* pre_shift, const void* const* omap, void* order,
                                                aod_stream_t stream) {
  ConvKParams p;
  ConvPlan pl;
  int rc = conv_params_grouped(desc, ngroups, src, w_packed, dst, pre_shift, nullptr, nullptr, p);
  if (rc) return rc;
  if (p.M == 0) return 0;
  rc = conv_plan(p, ngroups, false, pl);
  if (rc) return rc;
  if (omap && pl.kind == AOD_CONV_PLAN_IGEMM && pl.x3) {      // (the persistent kernel, AOD_X3P_GROUPED=1, skips bias-free dgrad tiles only: dense there)
    rc = conv_fwd_map_setup(p, ngroups, omap, (hipStream_t)stream, pl, (int*)order);
    if (rc) return rc;
  }
  return conv_launch(pl, p, nullptr, 0, (hipStream_t)stream);
}

extern "C" int aod_conv2d_grouped_fwd_map(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed,
                                          void* const* dst, const float* const* pre_shift, const void* const* omap, aod_stream_t stream) {
  return aod_conv2d_grouped_fwd_map_order(desc, ngroups, src, w_packed, dst, pre_shift, omap, nullptr, stream);
}

// The row-activity maps of the sparse forward: maps[0] from the assigner's bbox_weights (fp32 [rows * anchors][4], level-major like the rows
// of `desc`), maps[k] = the dilation of maps[k - 1] by the filter of `desc`, k < nmaps <= 8.  (rows + 63) / 64 bytes each.
extern "C" int aod_fwd_row_maps(const aod_conv_desc_t* desc, const float* bbox_weights, int anchors, int nmaps, void* const* maps,
                                aod_stream_t stream) {
  AOD_CHECK_ARG(desc && bbox_weights && maps && anchors >= 1 && nmaps >= 1 && nmaps <= 8, "fwd_row_maps: null argument, or nmaps %d outside 1 .. 8", nmaps);
  ConvKParams p;
  memset(&p, 0, sizeof(p));
  int rc = fill_params(desc, p);
  if (rc) return rc;
  AOD_CHECK_ARG(!p.transposed, "fwd_row_maps: a forward descriptor is expected");
  MapGeo mg;
  rc = conv_map_geo(p, mg, true);
  if (rc) return rc;
  if (p.M == 0) return 0;
  FwdMapChain c;
  memset(&c, 0, sizeof(c));
  c.n = nmaps;
  for (int k = 0; k < nmaps; ++k) {
    AOD_CHECK_ARG(maps[k], "fwd_row_maps: map %d is null", k);
    c.m[k] = (unsigned char*)maps[k];
  }
  AOD_CHECK_ARG(((uintptr_t)bbox_weights & 15) == 0, "fwd_row_maps: bbox_weights must be 16-byte aligned");
  hipLaunchKernelGGL(fwd_row_map_kernel, dim3((p.M + 63) >> 6), dim3(256), 0, (hipStream_t)stream, bbox_weights, c.m[0], (long long)p.M, 4 * anchors);
  AOD_LAUNCH_CHECK();
  if (nmaps > 1) {
    constexpr int LB = 16384;      // 2 x 16 KB of LDS: pyramids of up to 2^20 rows
    if (((p.M + 63) >> 6) <= LB) hipLaunchKernelGGL(fwd_map_chain_kernel<LB>, dim3(1), dim3(1024), 0, (hipStream_t)stream, c, mg);
    else hipLaunchKernelGGL(fwd_map_chain_kernel<0>, dim3(1), dim3(1024), 0, (hipStream_t)stream, c, mg);
    AOD_LAUNCH_CHECK();
  }
  return 0;
}

// conv_grouped_deal as data (host logic only): tile[b] / group[b] of block b of a grouped launch of `ngroups` members of `nwg` tiles each,
// b < nwg * ngroups; mapped: whether a member carries a row-activity map.
extern "C" int aod_conv2d_grouped_deal(int nwg, int ngroups, int mapped, int32_t* tile, int32_t* group) {
  AOD_CHECK_ARG(nwg >= 1 && ngroups >= 1 && ngroups <= 4 && tile && group, "conv_grouped_deal: nwg %d, ngroups %d", nwg, ngroups);
  for (int b = 0; b < nwg * ngroups; ++b) {
    int t, g;
    conv_grouped_deal(b, nwg, ngroups, mapped ? 1 : 0, t, g);
    tile[b] = t; group[b] = g;
  }
  return 0;
}

// The list of a mapped grouped launch as data (host logic only; the rule and the walk are the ones tile_order_kernel runs): `ngroups` members
// of `rows` GEMM rows and `tiles_n` column tiles each, maps[g] = a HOST copy of member g's row-activity map ((rows + 63) / 64 bytes) or null
// for a member without one.  tile[b] / group[b] of block b, b < ngroups * ceil(rows / 256) * tiles_n.
extern "C" int aod_conv2d_tile_order(int rows, int tiles_n, int ngroups, const void* const* maps, int32_t* tile, int32_t* group) {
  AOD_CHECK_ARG(rows >= 1 && tiles_n >= 1 && ngroups >= 1 && ngroups <= 4 && maps && tile && group, "conv_tile_order: rows %d, tiles_n %d, ngroups %d", rows, tiles_n, ngroups);
  TileOrderArgs a;
  memset(&a, 0, sizeof(a));
  for (int g = 0; g < ngroups; ++g) a.omap[g] = (const unsigned char*)maps[g];
  a.ngroups = ngroups; a.bm = 256; a.M = rows; a.tiles_m = (rows + 255) / 256; a.tiles_n = tiles_n;
  const int nwg = a.tiles_m * tiles_n;
  tile_order_host(a, tile);
  for (int b = 0; b < nwg * ngroups; ++b) { const int e = tile[b]; tile[b] = e % nwg; group[b] = e / nwg; }
  return 0;
}

extern "C" int aod_conv2d(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst,
                          const float* pre_scale, const float* pre_shift, const void* res, const void* mask,
                          const float* post_scale, void* zraw, float* colsum, aod_stream_t stream) {
  return aod_conv2d_ws(desc, src, w_packed, dst, pre_scale, pre_shift, res, mask, post_scale, zraw, colsum, nullptr, 0, stream);
}

// The plan of aod_conv2d_ws (ngroups = 0) / aod_conv2d_grouped (1 .. 4) for this descriptor and these operands: host logic, no device needed
extern "C" int aod_conv2d_plan(const aod_conv_desc_t* desc, int ngroups, unsigned operand_flags, aod_conv_plan_t* out) {
  AOD_CHECK_ARG(desc && out && ngroups >= 0 && ngroups <= 4, "conv_plan: null pointer or ngroups outside 0..4");
  static char operand[16];                      // stands for every operand that is present: the plan looks at pointers, never through them
  char* const dst = operand + 8;
  auto has = [&](unsigned f) { return (operand_flags & f) ? (void*)operand : nullptr; };
  void* const res = (operand_flags & AOD_CONV_RES_IS_DST) ? (void*)dst : has(AOD_CONV_HAS_RES);
  ConvKParams p;
  int rc;
  if (ngroups) {
    const void* in[4] = {operand, operand, operand, operand};
    void* outs[4] = {dst, dst, dst, dst};
    const float* shift[4] = {};
    const void* mask[4] = {has(AOD_CONV_HAS_MASK)};
    float* colsum[4] = {(float*)has(AOD_CONV_HAS_COLSUM)};
    shift[0] = (const float*)has(AOD_CONV_HAS_PRE_SHIFT);
    rc = conv_params_grouped(desc, ngroups, in, in, outs, shift, mask, colsum, p);
  } else {
    rc = conv_params(desc, operand, operand, dst, (const float*)has(AOD_CONV_HAS_PRE_SCALE), (const float*)has(AOD_CONV_HAS_PRE_SHIFT), res,
                     has(AOD_CONV_HAS_MASK), (const float*)has(AOD_CONV_HAS_POST_SCALE), has(AOD_CONV_HAS_ZRAW), (float*)has(AOD_CONV_HAS_COLSUM), p);
  }
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  if (p.M == 0) return 0;
  return conv_plan(p, ngroups, (operand_flags & AOD_CONV_HAS_WORKSPACE) != 0, *out);
}

// =====================================================================================
// weight re-packing
// =====================================================================================
__global__ void pack_w_fwd_kernel(const float* __restrict__ w, bf16_t* __restrict__ o, int O, int I, int RS, int Ipad) {
  const long long n = (long long)O * RS * Ipad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = i % Ipad; const long long r1 = i / Ipad; const int rs = r1 % RS; const int oo = r1 / RS;
    o[i] = (c < I) ? (bf16_t)w[((long long)oo * I + c) * RS + rs] : (bf16_t)0.f;
  }
}
__global__ void pack_w_dgrad_kernel(const float* __restrict__ w, const float* __restrict__ scale, bf16_t* __restrict__ o, int O, int I, int RS,
                                    int Opad) {
  const long long n = (long long)Opad * RS * I;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int oo = i % Opad; const long long r1 = i / Opad; const int rs = r1 % RS; const int c = r1 / RS;
    o[i] = (oo < O) ? (bf16_t)(w[((long long)oo * I + c) * RS + rs] * (scale ? scale[oo] : 1.f)) : (bf16_t)0.f;
  }
}
// One block per output channel o: g[o][c][rs] (+)= scale[o] * dw[o][rs][c], and wdot[o] = <w[o], dw[o]>.
// With y = (z - mean) * invstd * gamma + beta and z = <w[o], patch>, the BN-scale gradient needs sum_m gm[m,o] * z[m,o]
// = <w[o], sum_m gm[m,o] * patch(m)> = <w[o], dW_gm[o]>: the pre-BN activations never have to be stored or re-read.
__global__ __launch_bounds__(256) void unpack_wgrad_kernel(float* __restrict__ dw, float* __restrict__ g, const float* __restrict__ scale,
                                                          const float* __restrict__ w, float* __restrict__ wdot, const float* __restrict__ bn_s1,
                                                          const float* __restrict__ bn_mean, const float* __restrict__ bn_invstd, int O, int I,
                                                          int RS, int Ipad, int accumulate, int clear) {
  __shared__ float red[4];
  const int oo = blockIdx.x;
  const int n = I * RS;
  const float sc = scale ? scale[oo] : 1.f;
  float dot = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int rs = i % RS, c = i / RS;
    const long long si = ((long long)oo * RS + rs) * Ipad + c;
    const long long gi = (long long)oo * n + i;
    const float v = dw[si];
    if (clear) dw[si] = 0.f;          // hand the accumulator back all-zero: no separate memset launch per conv
    if (w) dot += w[gi] * v;
    g[gi] = accumulate ? g[gi] + v * sc : v * sc;
  }
  if (wdot) {
    dot = wave_sum(dot);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float d = red[0] + red[1] + red[2] + red[3];
      wdot[oo] = bn_s1 ? bn_invstd[oo] * (d - bn_mean[oo] * bn_s1[oo]) : d;      // BN weight gradient when the statistics are given
    }
  }
}
// Slab form: dw = [nslabs][Opad][RS][Ipad] partial sums written by conv_wgrad_kernel's splits; one block per output channel adds the
// slabs IN ORDER (deterministic), reading each slab row with consecutive lanes on consecutive channels, transposes [rs][c] -> [c][rs]
// through LDS and writes the OIHW gradient with consecutive lanes on consecutive elements.
constexpr int UNP_CH = 1024;      // channels per LDS chunk at RS <= 9 taps (9 216 tile entries; fewer channels per chunk for 10 .. 16 taps)
constexpr int UNP_T = 1024;       // threads: 16 waves per block keep enough slab loads in flight (one block per output channel)
struct UnpackArgs {
  const float* dw; float* g; const float* scale; const float* w; float* wdot; const float* bn_s1; const float* bn_mean; const float* bn_invstd;
  long long slab_stride;
  int nslabs, O, I, RS, Ipad, accumulate;
  int x3;      // (unused: x3 wgrad launches write LOGICAL slabs -- the three bands of an entry are added in the wgrad epilogue)
};
__device__ __forceinline__ void unpack_row(const UnpackArgs& a, int oo, float* tile, float* red) {
  const float* __restrict__ dw = a.dw;
  float* __restrict__ g = a.g;
  const float* __restrict__ w = a.w;
  const int nslabs = a.nslabs, I = a.I, RS = a.RS, Ipad = a.Ipad, accumulate = a.accumulate;
  const long long slab_stride = a.slab_stride;
  const float sc = a.scale ? a.scale[oo] : 1.f;
  float dot = 0.f;
  const int CH = RS <= 9 ? UNP_CH : (UNP_CH * 9) / RS;            // (filters of 10 .. 16 taps -- SSD512's 4 x 4 extra conv -- take narrower chunks of the same tile)
  for (int c0 = 0; c0 < I; c0 += CH) {
    const int nc = min(CH, I - c0);
    for (int i = threadIdx.x; i < nc * RS; i += UNP_T) {
      const int rs = i / nc, c = i - rs * nc;                       // consecutive lanes on consecutive channels of one slab row
      float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;                 // fixed association: ((s0+s4+..)+(s1+s5+..))+((s2+..)+(s3+..))
      {
      const float* src = dw + ((long long)oo * RS + rs) * Ipad + c0 + c;
      int sl = 0;
      for (; sl + 4 <= nslabs; sl += 4) {
        const float a0 = src[(long long)sl * slab_stride], a1 = src[(long long)(sl + 1) * slab_stride];
        const float a2 = src[(long long)(sl + 2) * slab_stride], a3 = src[(long long)(sl + 3) * slab_stride];
        v0 += a0; v1 += a1; v2 += a2; v3 += a3;
      }
      for (; sl < nslabs; ++sl) v0 += src[(long long)sl * slab_stride];
      }
      tile[c * RS + rs] = (v0 + v1) + (v2 + v3);
    }
    __syncthreads();
    const long long g0 = ((long long)oo * I + c0) * RS;
    for (int i = threadIdx.x; i < nc * RS; i += UNP_T) {
      const float v = tile[i];
      if (w) dot += w[g0 + i] * v;
      g[g0 + i] = accumulate ? g[g0 + i] + v * sc : v * sc;
    }
    __syncthreads();
  }
  if (a.wdot) {
    dot = wave_sum(dot);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) {
      float d = 0.f;
      for (int k = 0; k < UNP_T / 64; ++k) d += red[k];
      a.wdot[oo] = a.bn_s1 ? a.bn_invstd[oo] * (d - a.bn_mean[oo] * a.bn_s1[oo]) : d;
    }
  }
}
__global__ __launch_bounds__(UNP_T) void unpack_wgrad_slabs_kernel(const UnpackArgs a) {
  __shared__ float tile[UNP_CH * 9 + 1];
  __shared__ float red[UNP_T / 64];
  unpack_row(a, blockIdx.x, tile, red);
}
// the unpacks of a grouped wgrad launch in one grid: block -> (member, output channel)
struct UnpackGroups { UnpackArgs g[WG_MAXG]; int blk0[WG_MAXG + 1]; };
__global__ __launch_bounds__(UNP_T) void unpack_wgrad_slabs_grouped_kernel(const UnpackGroups gp) {
  __shared__ float tile[UNP_CH * 9 + 1];
  __shared__ float red[UNP_T / 64];
  const int b = blockIdx.x;
  if (b < gp.blk0[1]) unpack_row(gp.g[0], b, tile, red);
  else if (b < gp.blk0[2]) unpack_row(gp.g[1], b - gp.blk0[1], tile, red);
  else if (b < gp.blk0[3]) unpack_row(gp.g[2], b - gp.blk0[2], tile, red);
  else unpack_row(gp.g[3], b - gp.blk0[3], tile, red);
}
// ---- batched parameter preparation: ONE launch re-derives, for every registered conv layer, the folded eval-BN vectors
// (scale = gamma * rsqrt(var + eps), shift = beta - mean * scale, invstd) and both packed bf16 weight images (forward
// [O][R][S][Ipad]; dgrad [I][R][S][Opad] with the BN scale folded in).  After an optimizer step every trainable layer is stale; doing
// this per layer costs ~270 launches of a few microseconds each per iteration.
struct PrepItem {            // 16 x 8 bytes, filled by the host into a device table
  const float* w; const float* gamma; const float* beta; const float* mean; const float* var;
  bf16_t* wf; bf16_t* wd; float* scale; float* shift; float* invstd;
  int O, I, RS, Ipad, Opad, blk0;      // blk0: first block of this item
  float eps; int flags;                // flags bit 0: X3 images (X-layout along the packed channel axis: Ipad / Opad are then the PHYSICAL
  long long pad2_[2];                  // widths 2 * ceil32(I) / 2 * ceil32(O); head = bf16(v), tail = bf16(v - head), v = w (* BN scale, dgrad))
};
// One block = one 32 (out channels) x 32 (in channels) tile of one layer, all R*S taps: the fp32 master weights are read ONCE, coalesced
// (for a fixed output channel the (c, tap) run is contiguous), staged in LDS and written out as both packed images in 64-byte runs.
// Layers with more than 9 taps (the frozen 7x7 stem) take the element-wise path.
constexpr int PREP_T = 32, PREP_RS = 9;
__global__ __launch_bounds__(256) void param_prep_kernel(const PrepItem* __restrict__ items, int nitems) {
  __shared__ float tile[PREP_RS][PREP_T][PREP_T + 1];     // used as a linear [32][32*RS | 1] array
  int lo = 0, hi = nitems - 1;
  while (lo < hi) {      // block -> item: binary search over blk0 (items are in block order)
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const PrepItem it = items[lo];
  const int lb = blockIdx.x - it.blk0;
  const int t = threadIdx.x;
  if (it.RS > PREP_RS) {
    const long long nf = (long long)it.O * it.RS * it.Ipad, nd = it.wd ? (long long)it.I * it.RS * it.Opad : 0;
    for (int u = 0; u < 8; ++u) {
      const long long i = (long long)lb * 2048 + u * 256 + t;
      const bool x3 = it.flags & 1;
      if (i < nf) {
        const int cp = i % it.Ipad; const long long r1 = i / it.Ipad; const int rs = r1 % it.RS; const int oo = r1 / it.RS;
        const int c = x3 ? ((cp >> 6) << 5) + (cp & 31) : cp;              // logical channel of physical column cp
        const float v = (c < it.I) ? it.w[((long long)oo * it.I + c) * it.RS + rs] : 0.f;
        const bf16_t h = (bf16_t)v;
        it.wf[i] = (x3 && (cp & 32)) ? (bf16_t)(v - (float)h) : h;
      }
      if (i < nd) {
        const int op = i % it.Opad; const long long r1 = i / it.Opad; const int rs = r1 % it.RS; const int c = r1 / it.RS;
        const int oo = x3 ? ((op >> 6) << 5) + (op & 31) : op;
        float v = 0.f;
        if (oo < it.O) { v = it.w[((long long)oo * it.I + c) * it.RS + rs]; if (it.gamma) v *= it.gamma[oo] * rsqrtf(it.var[oo] + it.eps); }
        const bf16_t h = (bf16_t)v;
        it.wd[i] = (x3 && (op & 32)) ? (bf16_t)(v - (float)h) : h;
      }
      if (it.gamma && i < it.O) {
        const float inv = rsqrtf(it.var[i] + it.eps), sc = it.gamma[i] * inv;
        it.invstd[i] = inv; it.scale[i] = sc; it.shift[i] = it.beta[i] - it.mean[i] * sc;
      }
    }
    return;
  }
  const bool x3 = it.flags & 1;
  const int Il = x3 ? it.Ipad >> 1 : it.Ipad, Ol = x3 ? it.Opad >> 1 : it.Opad;      // logical (padded) channel counts of the two images
  const int tiles_c = (Il + PREP_T - 1) / PREP_T;
  const int to = lb / tiles_c, tc = lb - to * tiles_c;
  const int o0 = to * PREP_T, c0 = tc * PREP_T;
  const int RS = it.RS;
  const int run = PREP_T * RS;                 // floats of one output channel inside the tile: (c0 .. c0+32) x taps, contiguous in OIHW
  const int pitch = run | 1;                   // odd LDS pitch: column reads (dgrad image) stay conflict-free
  float* tl = &tile[0][0][0];                  // linear [32][pitch]
  const int cvalid = it.I - c0 < PREP_T ? it.I - c0 : PREP_T;     // real input channels in this tile (may be <= 0)
  {
    // the whole 32 x run tile as ONE flat index space of 16-B pieces (run = 32 RS floats is a multiple of 4, so a piece never straddles
    // two output channels): exactly RS pieces per thread, ALL requested before the first one is used (four 4-B loads in flight per thread
    // made every block a chain of nine memory round trips: 118 us per training step for 312 MB)
    const int lim = cvalid * RS;
    const float* src0 = it.w + ((long long)o0 * it.I + c0) * RS;
    const long long ostride = (long long)it.I * RS;
    const bool al = ((((size_t)src0) | ((size_t)ostride * 4)) & 15) == 0;
    f32x4 v[PREP_RS];
    int ol[PREP_RS], idx[PREP_RS];
    const bool full = al && cvalid == PREP_T && o0 + PREP_T <= it.O;      // (block-uniform: no per-thread predicate around the loads)
#pragma unroll
    for (int k = 0; k < PREP_RS; ++k) {
      v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (k < RS) {
        const int e = 4 * (t + k * 256);
        ol[k] = e / run; idx[k] = e - ol[k] * run;
        const float* sp = src0 + ol[k] * ostride + idx[k];
        if (full) v[k] = *reinterpret_cast<const f32x4*>(sp);
        else if (o0 + ol[k] < it.O) {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (idx[k] + j < lim) v[k][j] = sp[j];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PREP_RS; ++k)
      if (k < RS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) tl[ol[k] * pitch + idx[k] + j] = v[k][j];
      }
  }
  __syncthreads();
  // both images leave the tile as 16-B stores (8 consecutive channels per lane; 2-B stores -- one channel per lane -- held the launch at
  // 2.5 TB/s: 126 us per training step for 312 MB)
  // forward image [O][RS][Ipad]: runs of 32 input channels = 4 octets
  for (int u = t; u < PREP_T * RS * 4; u += 256) {
    const int oct = u & 3, q = u >> 2, ol = q / RS, rs = q - ol * RS;
    const int o = o0 + ol, c = c0 + oct * 8;
    if (o < it.O && c < Il) {
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (bf16_t)tl[ol * pitch + (oct * 8 + j) * RS + rs];
      if (!x3) *reinterpret_cast<bf16x8*>(it.wf + ((long long)o * RS + rs) * it.Ipad + c) = v;
      else {         // this tile's 32 channels = one head band + one tail band of the X-layout
        bf16x8 l;
#pragma unroll
        for (int j = 0; j < 8; ++j) l[j] = (bf16_t)(tl[ol * pitch + (oct * 8 + j) * RS + rs] - (float)v[j]);
        bf16_t* d = it.wf + ((long long)o * RS + rs) * it.Ipad + 2 * c0 + oct * 8;
        *reinterpret_cast<bf16x8*>(d) = v;
        *reinterpret_cast<bf16x8*>(d + 32) = l;
      }
    }
  }
  // dgrad image [I][RS][Opad] (x BN scale): runs of 32 output channels = 4 octets
  if (it.wd) {
    __shared__ float s_sc[PREP_T];
    if (t < PREP_T) {
      const int o = o0 + t;
      s_sc[t] = (it.gamma && o < it.O) ? it.gamma[o] * rsqrtf(it.var[o] + it.eps) : 1.f;
    }
    __syncthreads();
    for (int u = t; u < PREP_T * RS * 4; u += 256) {
      const int oct = u & 3, q = u >> 2, cl = q / RS, rs = q - cl * RS;
      const int c = c0 + cl, o = o0 + oct * 8;
      if (c < it.I && o < Ol) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (bf16_t)(tl[(oct * 8 + j) * pitch + cl * RS + rs] * s_sc[oct * 8 + j]);
        if (!x3) *reinterpret_cast<bf16x8*>(it.wd + ((long long)c * RS + rs) * it.Opad + o) = v;
        else {
          bf16x8 l;
#pragma unroll
          for (int j = 0; j < 8; ++j) l[j] = (bf16_t)(tl[(oct * 8 + j) * pitch + cl * RS + rs] * s_sc[oct * 8 + j] - (float)v[j]);
          bf16_t* d = it.wd + ((long long)c * RS + rs) * it.Opad + 2 * o0 + oct * 8;
          *reinterpret_cast<bf16x8*>(d) = v;
          *reinterpret_cast<bf16x8*>(d + 32) = l;
        }
      }
    }
  }
  if (it.gamma && tc == 0 && t < PREP_T && o0 + t < it.O) {
    const int o = o0 + t;
    const float inv = rsqrtf(it.var[o] + it.eps), sc = it.gamma[o] * inv;
    it.invstd[o] = inv; it.scale[o] = sc; it.shift[o] = it.beta[o] - it.mean[o] * sc;
  }
}
extern "C" int aod_param_prep(const void* items_dev, int nitems, int total_blocks, aod_stream_t stream) {
  AOD_CHECK_ARG(items_dev && nitems >= 0 && total_blocks >= 0, "param_prep: bad args");
  if (nitems == 0 || total_blocks == 0) return 0;
  hipLaunchKernelGGL(param_prep_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const PrepItem*)items_dev, nitems);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_param_prep_item_bytes(void) { return (int)sizeof(PrepItem); }


extern "C" int aod_pack_weight_fwd(const float* w, void* o, int O, int I, int R, int S, int Ipad, aod_stream_t stream) {
  AOD_CHECK_ARG(w && o && Ipad >= I && Ipad % 8 == 0, "pack_weight_fwd: bad args");
  hipLaunchKernelGGL(pack_w_fwd_kernel, dim3(grid_for<4096>((long long)O * R * S * Ipad)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)o, O, I, R * S, Ipad);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_pack_weight_dgrad(const float* w, void* o, int O, int I, int R, int S, int Opad, const float* scale, aod_stream_t stream) {
  AOD_CHECK_ARG(w && o && Opad >= O && Opad % 8 == 0, "pack_weight_dgrad: Opad must be a multiple of 8 and >= O");
  hipLaunchKernelGGL(pack_w_dgrad_kernel, dim3(grid_for<4096>((long long)Opad * R * S * I)), dim3(256), 0, (hipStream_t)stream, w, scale, (bf16_t*)o, O, I, R * S, Opad);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_unpack_wgrad_slabs(const float* dw_slabs, int nslabs, int64_t slab_stride, float* g, int O, int I, int R, int S, int Ipad,
                                      int accumulate, const float* scale, const float* w_oihw, float* wdot, const float* bn_s1,
                                      const float* bn_mean, const float* bn_invstd, aod_stream_t stream) {
  AOD_CHECK_ARG(dw_slabs && g && nslabs >= 1 && slab_stride > 0, "unpack_wgrad_slabs: null / empty");
  AOD_CHECK_ARG(R * S <= 16, "unpack_wgrad_slabs: at most 16 taps (larger filters take aod_unpack_wgrad)");
  AOD_CHECK_ARG(!wdot || w_oihw, "unpack_wgrad_slabs: wdot needs the weights");
  AOD_CHECK_ARG(!bn_s1 || (wdot && bn_mean && bn_invstd), "unpack_wgrad_slabs: BN mode needs wdot, mean and invstd");
  if (O == 0) return 0;
  UnpackArgs a;
  a.dw = dw_slabs; a.g = g; a.scale = scale; a.w = w_oihw; a.wdot = wdot; a.bn_s1 = bn_s1; a.bn_mean = bn_mean; a.bn_invstd = bn_invstd;
  a.slab_stride = slab_stride; a.nslabs = nslabs; a.O = O; a.I = I; a.RS = R * S; a.Ipad = Ipad; a.accumulate = accumulate & 1; a.x3 = (accumulate >> 1) & 1;
  hipLaunchKernelGGL(unpack_wgrad_slabs_kernel, dim3(O), dim3(UNP_T), 0, (hipStream_t)stream, a);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_unpack_wgrad_slabs_grouped(int n, const float* const* dw_slabs, const int32_t* nslabs, const int64_t* slab_stride,
                                              float* const* g, const int32_t* O, const int32_t* I, const int32_t* R, const int32_t* S,
                                              const int32_t* Ipad, const int32_t* accumulate, const float* const* scale,
                                              const float* const* w_oihw, float* const* wdot, const float* const* bn_s1,
                                              const float* const* bn_mean, const float* const* bn_invstd, aod_stream_t stream) {
  AOD_CHECK_ARG(n >= 1 && n <= WG_MAXG && dw_slabs && nslabs && slab_stride && g && O && I && R && S && Ipad && accumulate && scale &&
                w_oihw && wdot && bn_s1 && bn_mean && bn_invstd, "unpack_wgrad_slabs_grouped: 1..4 members, no null arrays");
  UnpackGroups gp;
  memset(&gp, 0, sizeof(gp));
  int blk = 0;
  for (int i = 0; i < n; ++i) {
    AOD_CHECK_ARG(dw_slabs[i] && g[i] && nslabs[i] >= 1 && slab_stride[i] > 0 && O[i] >= 1, "unpack_wgrad_slabs_grouped: null / empty member");
    AOD_CHECK_ARG(R[i] * S[i] <= 16, "unpack_wgrad_slabs_grouped: at most 16 taps");
    AOD_CHECK_ARG(!wdot[i] || w_oihw[i], "unpack_wgrad_slabs_grouped: wdot needs the weights");
    AOD_CHECK_ARG(!bn_s1[i] || (wdot[i] && bn_mean[i] && bn_invstd[i]), "unpack_wgrad_slabs_grouped: BN mode needs wdot, mean and invstd");
    UnpackArgs& a = gp.g[i];
    a.dw = dw_slabs[i]; a.g = g[i]; a.scale = scale[i]; a.w = w_oihw[i]; a.wdot = wdot[i]; a.bn_s1 = bn_s1[i]; a.bn_mean = bn_mean[i];
    a.bn_invstd = bn_invstd[i];
    a.slab_stride = slab_stride[i]; a.nslabs = nslabs[i]; a.O = O[i]; a.I = I[i]; a.RS = R[i] * S[i]; a.Ipad = Ipad[i]; a.accumulate = accumulate[i] & 1; a.x3 = (accumulate[i] >> 1) & 1;
    gp.blk0[i] = blk;
    blk += O[i];
  }
  for (int i = n; i <= WG_MAXG; ++i) gp.blk0[i] = i == n ? blk : 0x7fffffff;
  hipLaunchKernelGGL(unpack_wgrad_slabs_grouped_kernel, dim3(blk), dim3(UNP_T), 0, (hipStream_t)stream, gp);
  AOD_LAUNCH_CHECK();
  return 0;
}
extern "C" int aod_unpack_wgrad(float* dw, float* g, int O, int I, int R, int S, int Ipad, int accumulate, int clear_src, const float* scale,
                                const float* w_oihw, float* wdot, const float* bn_s1, const float* bn_mean, const float* bn_invstd,
                                aod_stream_t stream) {
  AOD_CHECK_ARG(dw && g, "unpack_wgrad: null");
  AOD_CHECK_ARG(!wdot || w_oihw, "unpack_wgrad: wdot needs the weights");
  AOD_CHECK_ARG(!bn_s1 || (wdot && bn_mean && bn_invstd), "unpack_wgrad: BN mode needs wdot, mean and invstd");
  if (O == 0) return 0;
  hipLaunchKernelGGL(unpack_wgrad_kernel, dim3(O), dim3(256), 0, (hipStream_t)stream, dw, g, scale, w_oihw, wdot, bn_s1, bn_mean, bn_invstd, O, I,
                     R * S, Ipad, accumulate, clear_src);
  AOD_LAUNCH_CHECK();
  return 0;
}
