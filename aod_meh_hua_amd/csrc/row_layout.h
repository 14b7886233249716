// The two layouts of an activation row and the one place that knows them.  Unit of work in both: one OCTET = 8 consecutive logical channels.
//   bf16 NHWC rows   channel c of a pixel is bf16 column c: an octet is ONE 16-B piece.
//   X rows           (reference-precision mode) an fp32 value v travels as head h = bf16(v) and tail l = bf16(v - h); C logical channels are
//                    a bf16 row of 2 * ceil32(C) columns [h(0..31) | l(0..31) | h(32..63) | l(32..63) | ...]: an octet is a 16-B head piece
//                    (column xoct(q), tile_prims.h) and the 16-B tail piece 64 B behind it.
// A row kernel that exists for both layouts is ONE template over a policy below: it computes on the eight fp32 values of an octet and leaves
// addressing, loading and storing to the policy.  Kernels that take the mode as an argument (`int x3`) use the run-time form at the end.
//   at(pix, q, Q)      element offset of octet q of pixel `pix` in rows of Q octets.
//   col(q)             column of octet q in its row: at(pix, q, Q) == at(pix, 0, Q) + col(q).
//   load / store       the octet at p <-> eight fp32 values.
#pragma once
#include "tile_prims.h"

struct Bf16Rows {
  static __device__ __forceinline__ long long at(long long pix, int q, int Q) { return (pix * Q + q) * 8; }
  static __device__ __forceinline__ int col(int q) { return q * 8; }
  static __device__ __forceinline__ void load(const bf16_t* __restrict__ p, float (&v)[8]) {
    const bf16x8 h = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
  }
  static __device__ __forceinline__ void store(bf16_t* __restrict__ p, const float (&v)[8]) {
    bf16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (bf16_t)v[j];
    *reinterpret_cast<bf16x8*>(p) = h;
  }
};

struct XRows {
  static __device__ __forceinline__ int pitch(int Q) { return (Q >> 2) * 64; }      // bf16 columns of a row of Q octets
  static __device__ __forceinline__ long long at(long long pix, int q, int Q) { return pix * pitch(Q) + xoct(q); }
  static __device__ __forceinline__ int col(int q) { return xoct(q); }
  static __device__ __forceinline__ void load(const bf16_t* __restrict__ p, float (&v)[8]) {
    const bf16x8 h = *reinterpret_cast<const bf16x8*>(p), l = *reinterpret_cast<const bf16x8*>(p + 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j] + (float)l[j];
  }
  static __device__ __forceinline__ void store(bf16_t* __restrict__ p, const float (&v)[8]) {
    bf16x8 h, l;
    split8(v, h, l);
    *reinterpret_cast<bf16x8*>(p) = h;
    *reinterpret_cast<bf16x8*>(p + 32) = l;
  }
};

// ---------------------------------------------------------------- run-time form: column of octet q in its row, and the load at it
__device__ __forceinline__ int row_col(int x3, int q) { return x3 ? xoct(q) : q * 8; }
// (not `x3 ? XRows::load : Bf16Rows::load`: one shared head load in front of the branch is what coreset.hip and ccms.hip were compiled from,
// and the two-call form reorders several hundred of their instructions)
__device__ __forceinline__ void row_load(const bf16_t* __restrict__ p, int x3, float (&v)[8]) {
  const bf16x8 h = *reinterpret_cast<const bf16x8*>(p);
  if (x3) {
    const bf16x8 l = *reinterpret_cast<const bf16x8*>(p + 32);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j] + (float)l[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
  }
}
