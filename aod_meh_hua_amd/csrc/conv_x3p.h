// Persistent producer / consumer form of the reference-precision (x3) convolution: csrc/conv_x3p.hip.  conv.hip's conv_plan() decides whether
// a launch takes it and in which form (ConvPlan: taps, wide, pre, lat, grid); conv_launch() fills X3PArgs from its own parameter block.
#pragma once
#include "common.h"

typedef aod_conv_plan_t ConvPlan;      // what conv_plan() decides and conv_launch() follows (include/aod_hip.h: aod_conv2d_plan reports it)
constexpr int XP_BM = 128;             // pixel rows of a tile of the persistent kernel

struct X3PArgs {
  const bf16_t* x;          // source rows, X-layout, p.C physical columns
  const bf16_t* w;          // packed filter [N][R][S][C] (physical columns), forward or dgrad image
  bf16_t* y;                // destination rows, X-layout (2 * ceil32(N) columns)
  const float* pre_scale;   // optional fp32 [N]
  const float* pre_shift;   // optional fp32 [N]
  const bf16_t* res;        // optional residual, destination layout
  const bf16_t* mask;       // optional ReLU mask (the producer's saved output), destination layout
  float* colsum;            // optional fp32 [N]: += column sums of the stored values (fp32 atomics)
  int C, N, K, taps, S, stride, pad, dil, transposed, relu, tapin;
  int nseg, M, tiles_m, tiles_n;
  int rot;                  // debug (AOD_X3P_ROT): tile-dependent start chunk of the K loop / dropped operand loads (timing experiments)
  int lat;                  // destination lattice: 0 dense; 1 CLASS-MAJOR stride-2 dgrad of a 3x3 / pad-1 conv (one segment, even OH / OW): the
                            // tiles walk the four (y & 1, x & 1) classes of the destination pixels, a class's tile multiplies only the 1 / 2 / 2 / 4
                            // taps that reach it; 2 the IN-PLACE 1x1 / stride-2 dgrad (conv.hip `up_w`): a plain GEMM over the dZ pixels whose row
                            // (b, y, x) is stored at destination row b * up_hw + 2y * up_w + 2x
  int up_w, up_hw;
  int ngroups;              // >= 1: grp[] holds the operands (grp[0] repeats the fields above for a plain launch)
  // omap (optional, the 3x3 / 256-column dense form): row-activity map of the DESTINATION rows, one byte per 64 (conv.hip, conv_map_setup) -- a tile
  // whose two blocks are 0 issues and consumes no stage and stores zero rows
  struct { const bf16_t* x; const bf16_t* w; bf16_t* y; const float* shift; const bf16_t* mask; float* colsum; const unsigned char* omap; } grp[4];
  // order (optional, the mapped 3x3 / 128-column form, plain launches): the ITEM LIST of the launch -- a permutation of the tiles tile_m * tiles_n +
  // tile_n that tile_order_kernel (conv.hip) writes from the map ahead of the launch, every live tile ahead of every dead one; the workgroup
  // whose slot is s = x3p_item_slot(blockIdx.x, tiles_n) runs order[s], order[s + G], ... (G = gridDim.x, a multiple of 8 * tiles_n)
  const int* order;
  long long x_bytes, w_bytes;
  int segH[8], segW[8], segOH[8], segOW[8], segB[8];
  long long seg_src0[8], seg_dst0[8];
  int seg_mend[8];
};

// ---- the deal of a mapped launch (X3PArgs.order).  The list ranks the items (a row tile's tiles_n column tiles follow each other) live first;
// position pos is item (pos / G) of the workgroup whose slot is pos % G.  Slots are dealt to the blocks in groups of tiles_n -- one row tile --
// round-robin over the eight blockIdx % 8 classes (XCDs): group u = slot / tiles_n goes to class u % 8, so the column tiles of a row tile, which
// read the same pixel rows, share an L2, consecutive live row tiles spread over the XCDs, and with the live items in positions [0, nlive) every
// workgroup owns ceil(nlive / G) of them or one fewer, ahead of its dead ones.  G % (8 * tiles_n) == 0 makes the deal a bijection per round.
__host__ __device__ __forceinline__ int x3p_item_slot(int bid, int tiles_n) {
  const int c = bid & 7, k = bid >> 3, i = k / tiles_n, tn = k - i * tiles_n;
  return (8 * i + c) * tiles_n + tn;
}
__host__ __device__ __forceinline__ int x3p_slot_block(int slot, int tiles_n) {      // the inverse
  const int u = slot / tiles_n, tn = slot - u * tiles_n;
  return (u & 7) + 8 * ((u >> 3) * tiles_n + tn);
}
// grid of a mapped launch: the largest multiple of 8 * tiles_n within min(tiles, CUs); 0 = too few tiles for the deal (the launch stays as it is)
static inline int x3p_mapped_grid(long long ntiles, int tiles_n, int ncu) {
  const long long cap = ntiles < ncu ? ntiles : ncu, unit = 8ll * tiles_n;
  return (int)(cap / unit * unit);
}

// launches the instance plan.taps / wide / lat / pre name on plan.grid workgroups (a combination without an instance is an error)
int aod_conv_x3p_launch(const X3PArgs& a, const ConvPlan& plan, hipStream_t st);
