// The small primitives every hand-written kernel file shares: workgroup placement, the LDS swizzles and row permutation of the MFMA tiles,
// vmcnt waits, buffer descriptors, the X-layout column map and the grid of the row kernels.  Several are CONTRACTS between files (the code
// that packs or stages an image and every kernel that reads fragments from it must use the same function): one definition, here.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- workgroup placement
// XCD remap of a block index, a bijection of [0, nwg): the hardware deals blocks round-robin over the 8 XCDs, so blocks that share an XCD
// (bid % 8) take a CONTIGUOUS range of tiles and neighbouring tiles meet in one L2.  Placement only: nothing depends on it for correctness.
__host__ __device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, j = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// n / d for n < 2^22 (the float product is within 1 of the quotient; one correction step makes it exact)
__device__ __forceinline__ unsigned udiv_small(unsigned n, unsigned d) {
  unsigned q = (unsigned)((float)n * __builtin_amdgcn_rcpf((float)d));
  const int r = (int)(n - q * d);
  q = r < 0 ? q - 1 : ((unsigned)r >= d ? q + 1 : q);
  return q;
}

// ---------------------------------------------------------------- LDS images of 128-B rows (64 bf16), byte offset of 16-B chunk `chunk` of `row`
// pixel tiles: the XOR swizzle of conv.hip (slot s of row r holds chunk s ^ ((r >> 1) & 7)): conflict-free ds_read_b128 fragment reads.
// The LDS-DMA lane roles that fill an image apply the same key on the source side.
__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// filter images: the paired-block row permutation (wrow) makes the 16 lanes of a fragment read rows {0-3, 8-11, 16-19, 24-27} (+4): rows r and
// r + 16 share (r >> 1) & 7 and lie 2048 B apart -- the same banks.  One more row bit in the XOR key separates them (PMC before: 35 % of
// the LDS cycles of the kernel were bank conflicts).  The code that stages a filter image and every fragment read of it must agree on this key.
__device__ __forceinline__ int wswz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7) ^ (((row >> 4) & 1) << 1)) << 4); }
// Which output channel sits in MFMA row `lr` of 16-row block j.  The blocks are PAIRED: rows 4q .. 4q + 3 of block 2p are channels
// 32p + 8q + 0..3 and of block 2p + 1 channels 32p + 8q + 4..7, so that in the transposed accumulators lane group q holds the 8
// CONSECUTIVE channels 32p + 8q .. + 7 across the pair: intermediates, residual and output move in 16-B pieces.
__device__ __forceinline__ int wrow(int j, int lr) { return (j >> 1) * 32 + (lr >> 2) * 8 + (j & 1) * 4 + (lr & 3); }

// ---------------------------------------------------------------- vmcnt waits
// wait until at most N / n vector memory operations of this wave are outstanding (loads, stores and LDS-DMA complete in issue order)
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// n is wave-uniform; beyond the table: vmcnt(0), waiting for more than asked is always safe.  The macro stays defined: pointwise.hip, whose
// ring runs 48 operations deep, keeps a longer switch of its own.
#define AOD_VMCASE(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
__device__ __forceinline__ void wait_vm_dyn(int n) {
  switch (n) {
    AOD_VMCASE(0) AOD_VMCASE(1) AOD_VMCASE(2) AOD_VMCASE(3) AOD_VMCASE(4) AOD_VMCASE(5) AOD_VMCASE(6) AOD_VMCASE(7) AOD_VMCASE(8)
    AOD_VMCASE(9) AOD_VMCASE(10) AOD_VMCASE(11) AOD_VMCASE(12) AOD_VMCASE(13) AOD_VMCASE(14) AOD_VMCASE(15) AOD_VMCASE(16)
    AOD_VMCASE(17) AOD_VMCASE(18) AOD_VMCASE(19) AOD_VMCASE(20) AOD_VMCASE(21) AOD_VMCASE(22) AOD_VMCASE(23) AOD_VMCASE(24)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// ---------------------------------------------------------------- buffer descriptors
// word 3 of a raw buffer descriptor (DATA_FORMAT = 32 bit, nothing else set: raw byte offsets checked against `bytes`) and the descriptor
// of `bytes` at p.  An access past the end reads zeros / stores nothing, so an EMPTY descriptor (bytes = 0) stands for an absent operand
// without a branch.
constexpr unsigned BUF_RSRC_FLAGS = 0x00020000u;
__device__ __forceinline__ auto buf_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, BUF_RSRC_FLAGS);
}
// the offset of a lane that must not touch memory: out of range of every descriptor, and it stays so under the per-step increments the
// loaders add to it (operands < 3.5 GiB: checked on the host)
constexpr unsigned BUF_OOB = 0xf0000000u;

// ---------------------------------------------------------------- accumulator pieces
// fp32 x 8 -> head h = bf16(v) and tail l = bf16(v - h) pieces of the X layout
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& h, bf16x8& l) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { h[j] = (bf16_t)v[j]; l[j] = (bf16_t)(v[j] - (float)h[j]); }
}
// bit j of the result: element j of the 16-B piece (8 bf16; X rows: 8 heads) is > 0 -- the ReLU mask of 8 channels in 8 bits
__device__ __forceinline__ unsigned pos_bits(const u32x4 q) {
  unsigned m = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    m |= (__uint_as_float(q[w] << 16) > 0.f ? 1u : 0u) << (2 * w);
    m |= (__uint_as_float(q[w] & 0xffff0000u) > 0.f ? 1u : 0u) << (2 * w + 1);
  }
  return m;
}
// sum over the 16 lanes that share lq (the lanes of one pixel block that hold the same 8 channels) = one DPP row: four rotate-and-add steps
// on the vector ALU, every lane ends up with the total (__shfl_xor would be four ds_bpermute round trips through the LDS pipe per value)
template <int N> __device__ __forceinline__ float row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false));
}
__device__ __forceinline__ float sum_lr(float v) {
  v += row_ror<8>(v); v += row_ror<4>(v); v += row_ror<2>(v); v += row_ror<1>(v);
  return v;
}

// ---------------------------------------------------------------- X layout (row_layout.h)
// physical column (elements) of logical octet q: 8 logical channels = a 16-B head piece and the 16-B tail piece 64 B behind it.  The row
// kernels, the dropout pass and the conv epilogues all address X rows through this map.
__device__ __forceinline__ int xoct(int q) { return ((q >> 2) << 6) + ((q & 3) << 3); }

// ---------------------------------------------------------------- grid of a grid-stride row kernel: 256-thread blocks over n items, at most CAP
template <int CAP>
static inline int grid_for(long long n) {
  const long long b = (n + 255) / 256;
  return (int)(b > CAP ? CAP : (b < 1 ? 1 : b));
}
