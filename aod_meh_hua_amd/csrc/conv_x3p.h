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
  long long x_bytes, w_bytes;
  int segH[8], segW[8], segOH[8], segOW[8], segB[8];
  long long seg_src0[8], seg_dst0[8];
  int seg_mend[8];
};

// launches the instance plan.taps / wide / lat / pre name on plan.grid workgroups (a combination without an instance is an error)
int aod_conv_x3p_launch(const X3PArgs& a, const ConvPlan& plan, hipStream_t st);
