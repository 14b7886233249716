// What the two halves of the convolution share: conv.hip (forward / dgrad) and conv_wgrad.hip (weight gradient) both turn an aod_conv_desc_t
// into ConvKParams with fill_params(), read the environment switches of the dispatch from ConvKnobs and place workgroups with xcd_swizzle()
// (tile_prims.h).
#pragma once
#include "tile_prims.h"

constexpr int WG_MAXG = 4;      // members of a grouped weight-gradient launch (conv_wgrad.hip) and of its grouped unpack (conv.hip)

struct ConvGroup { const bf16_t* x; const bf16_t* w; void* y; const float* pre_shift; const bf16_t* mask; float* colsum; const unsigned char* omap; };
struct ConvKParams {
  const bf16_t* x;
  const bf16_t* w;
  void* y;
  const float* pre_scale;
  const float* pre_shift;
  const bf16_t* res;
  const bf16_t* mask;
  const float* post_scale;
  bf16_t* zraw;
  float* colsum;      // optional fp32 [N]: += column sums of the stored values (fused bias / BN-shift gradient in dgrad launches)
  int C, N, K, R, S, stride, pad, dil, transposed, relu, out_f32;
  int nseg, M;
  int tiles_m, tiles_n;
  int ksplit;         // > 1: split-K launch -- K-steps are divided over ksplit workgroups per tile, each stores its fp32 partial tile
  float* ws;          // split-K workspace, fp32 [ksplit][M][N] in GEMM-row order; conv_splitk_finalize sums the slabs IN ORDER (deterministic)
  int perm;           // dgrad of a stride-2 conv: GEMM rows run CLASS-MAJOR inside a segment (the four (y & 1, x & 1) classes of the
                      // destination pixels one after the other), so a tile is one class and the filter taps that can never hit it are skipped
  int ngroups;        // > 1: grouped launch (aod_conv2d_grouped): grp[] replaces x / w / y / pre_shift / mask / colsum
  int interleave;     // grouped launch that carries a map: workgroup -> (tile, group) with the GROUP fastest (see conv_igemm_kernel in conv.hip)
  const int* order;   // mapped grouped launch of the 256 x 256 tile, optional: block b runs entry order[b] = member * tiles + tile, a permutation that
                      // tile_order_kernel (conv.hip) writes from the maps ahead of the launch -- live tiles first, dealt evenly over the blockIdx % 8
                      // classes.  nullptr: conv_grouped_deal (AOD_TILE_ORDER=0, or a caller without a list)
                      // Plain mapped 3x3 dgrad on the persistent kernel: the ITEM list of its 128-column form (conv_x3p.h, X3PArgs.order)
  const unsigned char* omap;   // X3 stride-1 dgrad, optional (sparse backward, conv_map_setup): ROW-ACTIVITY MAP of the DESTINATION -- byte b = 0: no
                      // row of 64 b .. 64 b + 63 can receive anything but zeros (every dZ row the filter taps reach from there is zero); a tile whose
                      // blocks are all 0 stores zero rows and leaves.  nullptr: every tile is computed.  Grouped launches: grp[].omap
  ConvGroup grp[4];
  int stagger;        // 8-wave forms: waves 4-7 run half a K-step behind waves 0-3 (see the K loop of conv_igemm_kernel, conv.hip)
  int x3;             // reference-precision mode (aod_conv_desc_t.x3): operands in the X-layout, three MFMAs per 32 channels (see X3 in conv.hip)
  int tap_inner;      // X3: K-steps run (channel chunk, tap) with the TAP innermost (see the loaders of conv_igemm_kernel, conv.hip)
  int bigrows;        // some segment has >= 2^22 rows: the float-reciprocal row decode is not exact, use integer division
  float* cs_ws;       // deterministic mode (determinism.hip): partial column sums go to row (group * tiles_m + tile_m) of this scratch [..][N]
                      // (split-K finalize: row = its row block) instead of into fp32 atomics; the launcher adds the rows in order afterwards
  int up_w, up_hw;    // > 0: LATTICE launch (conv_params): the GEMM rows are the pixels (b, y, x) of the source map and row (b, y, x) is stored
                      // at row b * up_hw + 2y * up_w + 2x of the destination -- the in-place 1x1 / stride-2 dgrad, whose other rows do not change
  long long x_bytes, w_bytes;
  int segH[8], segW[8], segOH[8], segOW[8], segB[8];
  long long seg_src0[8], seg_dst0[8];
  int seg_mend[8];
};

static inline int fill_params(const aod_conv_desc_t* d, ConvKParams& p) {
  AOD_CHECK_ARG(d->nseg >= 1 && d->nseg <= 8, "conv: nseg %d out of range", d->nseg);
  AOD_CHECK_ARG(d->C % 8 == 0, "conv: source channels %d must be a multiple of 8", d->C);
  AOD_CHECK_ARG(d->stride >= 1 && d->dil >= 1 && d->R >= 1 && d->S >= 1, "conv: bad geometry");
  AOD_CHECK_ARG(d->x3 == 0 || d->x3 == 1, "conv: aod_conv_desc_t.x3 = %d (0 or 1; descriptors must be zero-initialised -- the field took the place of padding in aod_version() 2)", d->x3);
  p.C = d->C; p.N = d->N; p.R = d->R; p.S = d->S; p.K = d->R * d->S * d->C;
  p.stride = d->stride; p.pad = d->pad; p.dil = d->dil; p.transposed = d->transposed;
  p.relu = d->relu; p.out_f32 = d->out_f32; p.nseg = d->nseg; p.x3 = d->x3 ? 1 : 0;
  if (p.x3) AOD_CHECK_ARG(d->C % 64 == 0, "conv (x3): X-layout source width %d must be a multiple of 64", d->C);
  long long m = 0;
  for (int i = 0; i < d->nseg; ++i) {
    const aod_conv_seg_t& s = d->seg[i];
    if (!d->transposed) {
      const int eh = (s.H + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1;
      const int ew = (s.W + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1;
      // (a destination smaller than the natural output is its top-left part: the space-to-depth stem computes 256 of the 257 rows /
      // columns a 4x4 / pad-2 filter would give)
      AOD_CHECK_ARG(s.OH >= 1 && s.OW >= 1 && s.OH <= eh && s.OW <= ew, "conv: segment %d output %dx%d exceeds the expected %dx%d", i, s.OH, s.OW, eh, ew);
    } else {
      const int eh = (s.OH + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1;
      const int ew = (s.OW + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1;
      AOD_CHECK_ARG(eh == s.H && ew == s.W, "dgrad: segment %d dZ %dx%d != expected %dx%d", i, s.H, s.W, eh, ew);
    }
    AOD_CHECK_ARG(s.H < 65536 && s.W < 65536 && s.OH < 65536 && s.OW < 65536, "conv: segment %d image side >= 65536", i);
    p.segB[i] = s.B; p.segH[i] = s.H; p.segW[i] = s.W; p.segOH[i] = s.OH; p.segOW[i] = s.OW;
    p.seg_src0[i] = s.src_row0; p.seg_dst0[i] = s.dst_row0;
    m += (long long)s.B * s.OH * s.OW;
    AOD_CHECK_ARG(m < (1ll << 31), "conv: too many rows");
    p.seg_mend[i] = (int)m;
  }
  for (int i = d->nseg; i < 8; ++i) { p.segB[i] = p.segH[i] = p.segW[i] = p.segOH[i] = p.segOW[i] = 0; p.seg_src0[i] = p.seg_dst0[i] = 0; p.seg_mend[i] = (int)m; }
  p.M = (int)m;
  p.bigrows = 0;
  for (int i = 0; i < d->nseg; ++i)
    if ((long long)d->seg[i].B * d->seg[i].OH * d->seg[i].OW >= (1ll << 22)) p.bigrows = 1;
  return 0;
}

// The environment switches of the dispatch.  FIRST HALF: read once per process (the first launch or plan).  SECOND HALF: consulted by the plan
// of every launch, because tests and parallel.GradSync change them in-process -- read lazily, at most once per launch and only by a rule
// that gets as far as asking, so that a launch never calls getenv more often than the rule ladder it replaces did (plain-bf16 launches: never).
struct ConvKnobs {
  struct Once {
    const char* ksplit_maxhw = getenv("AOD_KSPLIT_MAXHW");      // (debug: the largest per-image output that is still split)
    const char* ksplit_steps = getenv("AOD_KSPLIT_STEPS");      // (debug: a fixed number of K-steps per slice, the rule of the earlier rounds at 16)
    const char* stagger = getenv("AOD_STAGGER");
    const char* x3_taps_inner = getenv("AOD_X3_TAPS_INNER");    // (debug: 0 = the plain K order)
    const char* dgrad_lattice = getenv("AOD_DGRAD_LATTICE");
    const char* dgrad_classes = getenv("AOD_DGRAD_CLASSES");
    const char* tile_want = getenv("AOD_TILE_WANT");            // (debug: the tile count that counts as 'fills the device')
    const char* tile_256 = getenv("AOD_TILE_256");              // (1 forces the plain 256 x 256 tile, 0 disables it in every form)
    const char* tile_w8 = getenv("AOD_TILE_W8");
    const char* ring3 = getenv("AOD_RING3");
    // the weight-gradient plan (conv_wgrad.hip).  No test or tool sets an AOD_WGRAD_* variable in-process, so reading them here, at the first
    // dispatch of either half, instead of where a plan first reaches the rule changes nothing observable
    const char* wgrad_256 = getenv("AOD_WGRAD_256");            // (0 = never the 256 x 256 tile, nor the 8-wave wide x3 form)
    const char* wgrad_x3_wide = getenv("AOD_WGRAD_X3_WIDE");    // (debug: 0 = never the wide x3 form)
    const char* wgrad_x3_ragged = getenv("AOD_WGRAD_X3_RAGGED");   // (0 = narrow dZ stays on the 128 x 128 form)
    const char* wgrad_big_minm = getenv("AOD_WGRAD_BIG_MINM");  // (the rows from which a member of a GROUP takes the big tile, default 16 384)
    const char* wgrad_slots = getenv("AOD_WGRAD_SLOTS");        // (debug: grid size the group plan aims at, small-tile form)
    const char* wgrad_w8 = getenv("AOD_WGRAD_W8");              // (debug: 0 = the 4-wave bf16 128 x 128 form, single launches only)
    const char* wgrad_xcd = getenv("AOD_WGRAD_XCD");            // (debug: 0 = launch order)
  };
  static const Once& once() { static const Once k{}; return k; }

  enum Call { X3P_OVER_256, X3_TILE_192, X3P_GROUPED, X3P, X3P_PRE, X3P_BN, X3P_DGRAD, X3P_LATTICE, X3P_MIN_STEPS, X3P_PRE_MIN_STEPS, X3P_MIN_TILES,
              X3P_ROT, SPARSE_BWD, SPARSE_FWD, TILE_ORDER, X3P_MAPPED, NCALL };
  const char* val[NCALL];
  unsigned seen = 0;
  const char* call(Call k) {
    static const char* const names[NCALL] = {"AOD_X3P_OVER_256", "AOD_X3_TILE_192", "AOD_X3P_GROUPED", "AOD_X3P", "AOD_X3P_PRE", "AOD_X3P_BN",
                                             "AOD_X3P_DGRAD", "AOD_X3P_LATTICE", "AOD_X3P_MIN_STEPS", "AOD_X3P_PRE_MIN_STEPS", "AOD_X3P_MIN_TILES",
                                             "AOD_X3P_ROT", "AOD_SPARSE_BWD", "AOD_SPARSE_FWD", "AOD_TILE_ORDER", "AOD_X3P_MAPPED"};
    if (!((seen >> k) & 1u)) { val[k] = getenv(names[k]); seen |= 1u << k; }
    return val[k];
  }
  bool is(Call k, char c) { const char* v = call(k); return v && v[0] == c; }
};
static inline bool knob_is(const char* v, char c) { return v && v[0] == c; }
