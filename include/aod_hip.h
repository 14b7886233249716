/* libaodhip.so -- C ABI of the MI355X (gfx950) kernels behind the MEH/HUA hot path.
 *
 * The reference (MoonLab-YH/AOD_MEH_HUA) is pure Python; its native work is dispatched to
 * third-party libraries (cuDNN via torch, mmcv-full 1.3.8 CUDA ops, torch.distributions).
 * Each entry point below names the reference call site (file:line under /root/reference)
 * whose native dispatch it replaces.  INTEGRATION.md shows the Python (ctypes) binding a
 * maintainer of the reference would add at each site.
 *
 * Conventions (every entry point):
 *   - returns 0 on success, -1 bad argument/shape, -2 workspace too small, -3 HIP error
 *     (message via aod_last_error());
 *   - caller owns all memory (device pointers, pre-allocated outputs); no internal
 *     allocation, no host sync; kernels are enqueued on `stream` (a hipStream_t);
 *   - activations are NHWC ("channels-last") bf16 unless stated; weights are handed over in
 *     the reference's OIHW fp32 master layout and re-packed by aod_pack_weight_*;
 *   - int64 label / index tensors keep the reference's dtypes.
 */
#ifndef AOD_HIP_H
#define AOD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* aod_stream_t; /* hipStream_t */

const char* aod_last_error(void);
int aod_version(void); /* 3 removed the fragment-major filter pack and the register-streamed 256-plane bottleneck entries that version 2 exported */

/* ------------------------------------------------------------------ convolution (K1-K3, K5)
 * One pyramid segment = one [B, H, W, C] NHWC block inside a flat [rows, C] buffer.  A launch may
 * cover up to 8 segments that share weights (the five FPN levels of the head towers,
 * mmdet/models/dense_heads/Lambda_L2.py:79-103 multi_apply over levels). */
typedef struct {
  int32_t B, H, W;        /* source block geometry (input of fwd; dZ of dgrad)                */
  int32_t OH, OW;         /* destination block geometry (output of fwd; dX of dgrad)          */
  int64_t src_row0;       /* first row of this block in the source buffer                     */
  int64_t dst_row0;       /* first row of this block in the destination buffer                */
} aod_conv_seg_t;

typedef struct {
  int32_t C, N;           /* GEMM K-side channels (source channels), output channels          */
  int32_t R, S;           /* filter taps                                                      */
  int32_t stride, pad, dil;
  int32_t transposed;     /* 0: y = conv(x, w).  1: dgrad (dX = conv_transpose(dZ, w)); `w`
                             must then be the [C_in][R][S][C_out] packing (aod_pack_weight_dgrad) */
  int32_t relu;           /* apply max(v, 0) last                                             */
  int32_t out_f32;        /* destination dtype: 0 bf16, 1 fp32                                */
  int32_t nseg;
  int32_t x3;             /* 1: reference-precision mode.  bf16 operands are in the X-LAYOUT: a tensor of c logical channels has
                             2*ceil32(c) bf16 columns [h(0..31) | l(0..31) | h(32..63) | ...], value = head + tail (h = bf16(v),
                             l = bf16(v - h)); three MFMAs per 32 channels (xh*wh + xl*wh + xh*wl) give fp32-grade products.  C is then
                             the PHYSICAL source width (multiple of 64), N the LOGICAL output channel count; a bf16 destination,
                             res and mask are X-layout rows of 2*ceil32(N) columns, an fp32 destination has N columns.  (Fills the
                             padding the struct had in front of seg[]: the layout of the other fields is unchanged.  aod_version() >= 2.
                             Descriptors MUST be zero-initialised (memset / = {0}); any value other than 0 or 1 is rejected.) */
  aod_conv_seg_t seg[8];
} aod_conv_desc_t;

/* replaces: F.conv2d dispatched by mmcv ConvModule / nn.Conv2d in
 *   mmdet/models/backbones/resnet.py:165-205,262-301,598-610 (+ frozen-stat BN :647-656 folded
 *   into pre_scale/pre_shift), mmdet/models/necks/fpn.py:156-202,
 *   mmdet/models/dense_heads/Lambda_L2.py:85-103.
 * v = acc * pre_scale[n] + pre_shift[n] + res[m][n]; if (mask) v = mask[m][n] > 0 ? v : 0;
 * v *= post_scale[n]; if (relu) v = max(v, 0); dst[m][n] = v; optional zraw[m][n] = acc (bf16);
 * optional colsum[n] += sum_m v (fp32 atomics).  In a dgrad launch res / mask / colsum fuse the ACTIVATION backward
 * of the layer below into the epilogue: dst = (dX + res) * [mask > 0] is the masked gradient w.r.t. that layer's
 * pre-activation output and colsum its bias / BN-shift gradient (the autograd chain of Lambda_L2.py:85-94 and
 * resnet.py:262-301 without a separate elementwise pass).
 * Any of pre_scale/pre_shift/res/mask/post_scale/zraw/colsum may be NULL. */
int aod_conv2d(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst,
               const float* pre_scale, const float* pre_shift, const void* res, const void* mask,
               const float* post_scale, void* zraw, float* colsum, aod_stream_t stream);

/* Same operation with a caller-provided scratch buffer, which lets small-output / deep-reduction convolutions (at most 16 x 16
 * outputs per image and K >= 4096: the stride-2 3x3 on C5 that makes pyramid level P6, fpn.py:156-202 -- 1 024 output pixels,
 * K = 18 432 -- and the 3x3 convs of the last backbone stage, resnet.py:262-301) run split-K: the K-steps of a tile are divided over
 * several workgroups, each stores its fp32 partial tile into its own slab of `workspace` ([slices][M][N] fp32, need not be
 * initialised) and a second small kernel adds the slabs IN ORDER and applies the epilogue above -- deterministic, no atomics.
 * Whether and how K is sliced depends on K and on the per-image output size only, not on the batch: the summation order of an output
 * element never changes with the batching of the pool.
 * aod_conv2d_ws_bytes() is the size the launch heuristic wants for this descriptor (0: the direct kernel is used and workspace may
 * be NULL).  aod_conv2d() == aod_conv2d_ws() with workspace NULL. */
size_t aod_conv2d_ws_bytes(const aod_conv_desc_t* desc);
int aod_conv2d_ws(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst,
                  const float* pre_scale, const float* pre_shift, const void* res, const void* mask,
                  const float* post_scale, void* zraw, float* colsum, void* workspace, size_t workspace_bytes,
                  aod_stream_t stream);

/* Which kernel a launch would run on -- the decision aod_conv2d_ws (ngroups = 0) or aod_conv2d_grouped (ngroups = 1 .. 4, below) takes for
 * this descriptor, as data.  Host logic only: nothing is enqueued and no device is needed (without one the CU count counts as 256).
 * operand_flags: which optional operands the launch would carry (grouped: whether ANY group has the mask / column sum);
 * AOD_CONV_RES_IS_DST: a residual that is the destination itself (the in-place gradient accumulation).  The plan follows the same
 * environment switches, aod_set_deterministic and aod_set_pointwise_mode as the launch.  kind 0: an empty launch (no rows). */
enum { AOD_CONV_PLAN_PW_STREAM = 1,   /* the streaming 1x1 GEMM (csrc/pointwise.hip); no further fields                                  */
       AOD_CONV_PLAN_SPLIT_K = 2,     /* conv_igemm_kernel<bm, bn, nt, ops, grouped, stages, x3> over ksplit K slices + the finalize pass */
       AOD_CONV_PLAN_X3P = 3,         /* conv_x3p_kernel<taps, wide ? 8 : 4, lat, pre> on grid workgroups (csrc/conv_x3p.hip)             */
       AOD_CONV_PLAN_IGEMM = 4 };     /* conv_igemm_kernel<bm, bn, nt, ops, grouped, stages, x3>                                          */
enum { AOD_CONV_HAS_PRE_SCALE = 1, AOD_CONV_HAS_PRE_SHIFT = 2, AOD_CONV_HAS_RES = 4, AOD_CONV_RES_IS_DST = 8, AOD_CONV_HAS_MASK = 16,
       AOD_CONV_HAS_POST_SCALE = 32, AOD_CONV_HAS_ZRAW = 64, AOD_CONV_HAS_COLSUM = 128, AOD_CONV_HAS_WORKSPACE = 256 };
typedef struct {
  int32_t kind;
  int32_t bm, bn, nt, ops, stages, x3, grouped;   /* tile rows x columns, threads, epilogue operands (0 none, 1 mask, 2 residual + mask), LDS stages */
  int32_t ksplit;
  int32_t taps, wide, pre, lat, grid;             /* the kernel's TAPS (4: class-major form), 256-column tiles, operand prefetch 0 / 1 (residual) /
                                                     2 (mask), lattice 0 / 1 (class-major stride-2 dgrad) / 2 (in-place 1x1 stride-2 dgrad), workgroups */
} aod_conv_plan_t;
int aod_conv2d_plan(const aod_conv_desc_t* desc, int ngroups, unsigned operand_flags, aod_conv_plan_t* out);

/* Reference-precision (x3) launches of aod_conv2d(_ws) with an X-layout destination, N % 128 == 0, a 1x1 or 3x3 filter (forward at any
 * stride, dgrad at stride 1), segments that are whole multiples of 128 rows (but the last), at least ~192 tiles of 128 x 128 and at least
 * 24 K-steps (of 32 channels x 1 tap) per tile -- the 3x3 convs and the deep reduce / lateral 1x1 convs of the trainable backbone stages and
 * of the neck (mmdet/models/backbones/resnet.py:262-301, necks/fpn.py:151-202), their dgrads, and the dgrad of retina_cls
 * (dense_heads/Lambda_L2.py:52) -- run on a persistent producer / consumer kernel
 * (csrc/conv_x3p.hip: loader waves stream the operand tiles through a four-slot LDS ring, consumer waves only issue MFMAs and finish the
 * tile from registers).  Results are bit-identical to the general kernel (the optional column sums are fp32 atomics in both).  Environment
 * AOD_X3P=0 keeps every launch on the general kernel, AOD_X3P_MIN_TILES / AOD_X3P_MIN_STEPS override the two thresholds, AOD_X3P_GROUPED=1
 * also sends the grouped tower launches of aod_conv2d_grouped there (128 x 256 tiles; level with the 256 x 256 tile); with aod_set_deterministic(1) launches
 * that carry column sums stay on the general kernel (ordered sums).  The class-major stride-2 dgrad of a 3x3 / pad-1 conv on an even map and the
 * in-place 1x1 / stride-2 dgrad (res == dst) run there as lattice launches (AOD_X3P_LATTICE=0: general kernel).  aod_conv_x3p_count(): launches the persistent kernel has taken in this
 * process (tests / bench bookkeeping). */
int64_t aod_conv_x3p_count(void);

/* 1x1 / stride-1 / one-segment launches of aod_conv2d(_ws) without zraw / post_scale / fp32 destination are plain GEMMs over consecutive
 * rows (the conv1 / conv3 of every bottleneck, mmdet/models/backbones/resnet.py:260-290, and their dgrads): a persistent streaming
 * kernel (csrc/pointwise.hip) takes them when its tiles fill the CUs.  mode -1 (default): that heuristic (environment AOD_PW_STREAM=0/1
 * overrides), 0: always the general implicit-GEMM kernel, 1: the streaming kernel whenever the shape allows (K % 64 == 0, N % 64 == 0,
 * N <= 2048).  Process-wide; results of the two kernels are bit-identical (tests/test_gpu_kernels.py).  Returns the previous mode. */
int aod_set_pointwise_mode(int mode);

/* Deterministic mode (the reference's `--deterministic`, tools/train_RetinaNet.py:56-68 -> cudnn.deterministic): on = 1 makes the bias /
 * BN-shift column sums of the dgrad epilogues and of the activation-backward / pad-cast passes -- the only order-dependent reduction of
 * the training path (fp32 atomics otherwise) -- sums of per-workgroup partials in a fixed order (csrc/determinism.hip; one small extra
 * launch per vector).  Two runs from the same state are then bit-identical.  Allocates a 32 MB scratch on the CURRENT device the first time
 * it is switched on there (call it outside a graph capture, once per device).  Process-wide; returns the previous setting. */
int aod_set_deterministic(int on);
int aod_get_deterministic(void);

/* A whole 64-channel ResNet bottleneck, forward only (mmdet/models/backbones/resnet.py:262-301 with eval-mode BN; layer1 is frozen,
 * resnet.py:612-628, so nothing of it is needed by the backward pass either):
 *   y = relu(bn3(conv3_1x1(relu(bn2(conv2_3x3(relu(bn1(conv1_1x1(x)))))))) + res)
 * x [B*H*W][Cin] bf16 NHWC rows (Cin % 64 == 0), w1 [64][Cin], w2 [64][3][3][64], w3 [256][64] packed forward weights, s* / b* the
 * folded BN scale / shift vectors (fp32), res and y [B*H*W][256] bf16 (res may be x).  One kernel: the two 64-channel intermediates
 * stay in LDS, x and y cross HBM once (csrc/bottleneck.hip). */
int aod_bottleneck64_fwd(const void* x, int Cin, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                         const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, const void* res, void* y,
                         aod_stream_t stream);
/* ... for the stage's FIRST block (Cin = 64; resnet.py:291-292): the residual is bn_d(conv_d_1x1(x)), computed inside the launch from the packed
 * [256][64] filter of the downsample conv and its folded BN -- the bits a separate aod_conv2d launch would have stored and this one read back. */
int aod_bottleneck64_ds_fwd(const void* x, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                            const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, const void* wd,
                            const float* sd, const float* bd, void* y, aod_stream_t stream);
/* The same for an IDENTITY bottleneck of the 128-plane stage (layer2: 512 -> 128 -> 128 -> 512, residual = x): the conv2 / conv3 filters are
 * streamed through LDS rings (csrc/bottleneck_wide.hip).  t1 / t2 (optional, [B*H*W][128] bf16): the block's two intermediates for the
 * pixels of the image -- with them the launch is also the forward of a TRAINING step (the backward pass reads them); NULL: inference. */
int aod_bottleneck128_fwd(const void* x, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                          const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, void* y, void* t1, void* t2,
                          aod_stream_t stream);
/* ... and of the 256-plane stage (layer3: 1024 -> 256 -> 256 -> 1024; t1 / t2 [B*H*W][256]): 4 x 16 pixel tiles, the eight waves split the
 * output channels, all three filters streamed in 32-KB slices. */
int aod_bottleneck256_fwd(const void* x, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                          const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, void* y, void* t1, void* t2,
                          aod_stream_t stream);
/* The DGRAD chain of the same identity blocks (planes = 128 / 256) in one launch -- the three dgrad launches of conv3, conv2, conv1 with
 * their fused epilogues (aod_conv2d: mask / res / colsum) back to back, the two intermediates staying in LDS:
 *   gt2 = [act_t2 > 0] * conv3_T(g)        gt1 = [act_t1 > 0] * conv2_T(gt2)        gx = [act_x > 0] * (conv1_T(gt1) + g)
 * g [B*H*W][4*planes]: the finished gradient w.r.t. the block's pre-ReLU output (it is also the skip branch's gradient); wd3 [planes][4*planes],
 * wd2 [planes][3][3][planes], wd1 [4*planes][planes]: the packed dgrad filters (BN scale folded in, aod_pack_weights_dgrad); act_*: the
 * activations the forward pass saved; colsum_*: fp32 [planes] [planes] [4*planes], += column sums of the three results (the BN-shift
 * gradients of conv2, conv1 and of the previous block's conv3).  Gradients equal those of the three launches bit for bit. */
int aod_bottleneck_bwd(int planes, const void* g, int B, int H, int W, const void* wd3, const void* wd2, const void* wd1, const void* act_t2,
                       const void* act_t1, const void* act_x, void* gx, void* gt2, void* gt1, float* colsum_t2, float* colsum_t1,
                       float* colsum_x, aod_stream_t stream);

/* Grouped launch: `ngroups` (<= 4) convolutions with IDENTICAL descriptor (geometry, C, N, filter) but their own operands share one
 * grid -- the cls / reg / evidence towers at one depth (Lambda_L2.py:85-103: three independent 4-conv stacks over the same pyramid).
 * Alone each tower conv leaves a third of its last round of workgroups idle; together their tiles fill whole rounds (3 x 341 tiles of
 * 256 x 256 = 3.996 rounds of the 256 CUs).  bf16 destinations; pre_shift / mask / colsum arrays (or their entries) may be NULL; a
 * dgrad descriptor (transposed = 1, stride 1) is accepted.  Results are bit-identical to `ngroups` aod_conv2d calls. */
int aod_conv2d_grouped(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed, void* const* dst,
                       const float* const* pre_shift, const void* const* mask, float* const* colsum, aod_stream_t stream);

/* Sparse backward (reference-precision mode, stride-1 dgrad between dense same-size maps -- the head towers).  A ROW-ACTIVITY MAP is one byte
 * per 64 rows of a gradient row tensor, (rows + 63) / 64 bytes: 0 = every row of the block is exactly zero, 1 = the block may hold
 * something; a NULL map = everything may.  The box-regression and MEH gradients are zero at every anchor that is not positive, i.e. in
 * ~99 % of the pyramid rows.  in_map describes dZ; the launch writes out_map, the map of dX (block b is 1 when a dZ block that the filter
 * taps reach from its rows is: never 0 for a block that receives a non-zero value, never looser than the linear row range
 * [first - W - 1, last + W + 1] of a 3x3), and a tile of the convolution whose dX blocks are all 0 loads nothing, multiplies nothing and stores
 * zero rows (heads and tails).  Active tiles run the dense code: same bits.  Members with a bias / scale / residual operand, split-K launches,
 * launches on kernels without the check and column sums in deterministic mode are computed densely (out_map is still written).
 * in_map and out_map come together (grouped: per member; a member without maps is dense). */
int aod_conv2d_ws_map(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst, const float* pre_scale,
                      const float* pre_shift, const void* res, const void* mask, const float* post_scale, void* zraw, float* colsum,
                      void* workspace, size_t workspace_bytes, const void* in_map, void* out_map, aod_stream_t stream);
int aod_conv2d_grouped_map(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed, void* const* dst,
                           const float* const* pre_shift, const void* const* mask, float* const* colsum, const void* const* in_map,
                           void* const* out_map, aod_stream_t stream);
/* The mapped form of the persistent kernel.  `order`: int32 [ceil(rows / 128) * N / 128], device memory.  A 3x3 launch of aod_conv2d_ws_map
 * that the persistent kernel takes and whose map may skip tiles then runs 128-column tiles -- a live 128-row tile is N / 128 ITEMS -- in the
 * order of a list that the launch which writes out_map also writes there: a permutation of the items tile_m * (N / 128) + tile_n, ranked in
 * that order, every live one ahead of every dead one.  List position pos is item pos / G of the workgroup whose slot is pos % G (G = the grid,
 * a multiple of 8 * N / 128); slots go to the blocks one row tile at a time, round-robin over the blockIdx % 8 classes, so a row tile's column
 * tiles share a class and every workgroup owns ceil(live / G) live items or one fewer, ahead of its dead ones (which still store their zero
 * rows).  Same bits per row as aod_conv2d_ws_map.  order = NULL, AOD_X3P_MAPPED=0 (read per call), fewer than 8 * N / 128 items, or a launch
 * the form does not apply to: aod_conv2d_ws_map unchanged.  aod_conv2d_x3p_item_order applies the rule to a HOST copy of the map (item, block
 * and round of every list position for a grid of `grid` workgroups); aod_conv2d_x3p_mapped_grid is the grid on a device of `cus` compute
 * units (0: the form is not taken); aod_conv_x3p_mapped_count() counts the launches that took the form in this process. */
int aod_conv2d_ws_map_order(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst, const float* pre_scale,
                            const float* pre_shift, const void* res, const void* mask, const float* post_scale, void* zraw, float* colsum,
                            void* workspace, size_t workspace_bytes, const void* in_map, void* out_map, void* order, aod_stream_t stream);
int aod_conv2d_x3p_item_order(int rows, int tiles_n, int grid, const void* map, int32_t* item, int32_t* block, int32_t* round);
int aod_conv2d_x3p_mapped_grid(int rows, int tiles_n, int cus);
int64_t aod_conv_x3p_mapped_count(void);

/* Sparse forward (reference-precision mode, the reg and MEH towers in training).  The box-regression and the MEH loss multiply by the assigner's
 * bbox_weights, 0 at every anchor that is not positive, so those towers' activations are read only inside the receptive field of the positives.
 * aod_fwd_row_maps writes the chain: maps[0] byte b = 1 when a pixel row of 64 b .. 64 b + 63 owns an anchor with a non-zero weight (pixel row p
 * owns rows anchors * p .. anchors * p + anchors - 1 of bbox_weights, fp32 [.][4], level-major like the rows of `desc`), maps[k] = the dilation
 * of maps[k - 1] by the rule of aod_conv2d_ws_map (desc: a forward x3 stride-1 descriptor between dense same-size maps; nmaps <= 8).
 * aod_conv2d_grouped_fwd_map is aod_conv2d_grouped (forward) with a READY-MADE map per member (NULL entries: dense members): a 256-row tile
 * whose blocks are all 0 loads nothing, multiplies nothing and stores ZERO rows -- not relu(bias) --; live tiles run the dense code on the
 * same operands: same bits.  AOD_SPARSE_FWD=0: no tile is skipped.  Launches on the persistent kernel (AOD_X3P_GROUPED=1) stay dense.
 * aod_conv2d_grouped_deal gives the block -> (tile, member) assignment of a grouped launch as data: mapped = 0 the member-major XCD-contiguous
 * order, mapped = 1 (some member carries a map, forward or dgrad) the even deal over the eight blockIdx % 8 classes. */
int aod_fwd_row_maps(const aod_conv_desc_t* desc, const float* bbox_weights, int anchors, int nmaps, void* const* maps, aod_stream_t stream);
int aod_conv2d_grouped_fwd_map(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed, void* const* dst,
                               const float* const* pre_shift, const void* const* omap, aod_stream_t stream);
int aod_conv2d_grouped_deal(int nwg, int ngroups, int mapped, int32_t* tile, int32_t* group);

/* The block order of a mapped grouped launch as a device-built LIST.  `order`: int32 [ngroups * tiles], device memory, tiles = ceil(rows / 256)
 * * ceil(N / 256).  Where the launch carries a map and runs the 256 x 256 tile, the small launch that writes the maps (dgrad) or one ahead of
 * the conv (forward) writes a permutation of the entries member * tiles + tile there, and block b of the conv runs entry order[b]: every live
 * entry (a member without a map: all its tiles) before every dead one; the live ones, ranked member-major, dealt so that each blockIdx % 8
 * class takes a contiguous range of the ranking, the same number +- 1.  Which block runs a tile is placement only: same bits per row.
 * order = NULL, AOD_TILE_ORDER=0, or a launch the list does not apply to: aod_conv2d_grouped_map / aod_conv2d_grouped_fwd_map unchanged.
 * aod_conv2d_tile_order applies the same rule to HOST copies of the maps (NULL entries: members without a map; tiles_n = ceil(N / 256)). */
int aod_conv2d_grouped_map_order(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed, void* const* dst,
                                 const float* const* pre_shift, const void* const* mask, float* const* colsum, const void* const* in_map,
                                 void* const* out_map, void* order, aod_stream_t stream);
int aod_conv2d_grouped_fwd_map_order(const aod_conv_desc_t* desc, int ngroups, const void* const* src, const void* const* w_packed,
                                     void* const* dst, const float* const* pre_shift, const void* const* omap, void* order, aod_stream_t stream);
int aod_conv2d_tile_order(int rows, int tiles_n, int ngroups, const void* const* maps, int32_t* tile, int32_t* group);

/* replaces: the weight-gradient half of autograd's conv backward (cuDNN wgrad) for the same
 * call sites.  dw_f32 is [N][R][S][C] fp32 and is ACCUMULATED into (caller zeroes it);
 * x: forward input [rows, C] bf16; dz: [rows_out, N] bf16. */
int aod_conv2d_wgrad(const aod_conv_desc_t* desc, const void* x, const void* dz, float* dw_f32,
                     const void* row_table, aod_stream_t stream);
/* Deterministic form of the same operation (no float atomics): the kernel splits the pixel axis over aod_conv2d_wgrad_splits(desc)
 * workgroup groups; split s STORES its partial result into slabs + s * slab_stride ([N][R][S][C] fp32 each, need not be initialised;
 * slab_stride >= N*R*S*C elements) and aod_unpack_wgrad_slabs adds the slabs in split order.  Plain stores run at ~6 TB/s where float
 * atomics run at ~1.3 TB/s chip-wide, and the weight gradient becomes bit-reproducible run to run (1-GPU vs N-GPU traces comparable). */
int aod_conv2d_wgrad_splits(const aod_conv_desc_t* desc);
int aod_conv2d_wgrad_slabs(const aod_conv_desc_t* desc, const void* x, const void* dz, float* slabs, int nslabs, int64_t slab_stride,
                           const void* row_table, aod_stream_t stream);
/* Grouped form: the weight gradients of n (<= 4) convolutions of ANY geometries in one grid -- e.g. the three convs of a bottleneck once
 * its dgrad chain has produced all three gradients.  Alone a backbone layer needs 100+ pixel splits of its few tiles to fill the chip and
 * leaves that many partial slabs; together each needs a fraction of them.  aod_conv2d_wgrad_group_plan: splits_out[i] = slabs member i
 * needs; returns 1 (nothing written) when the members do not share a tile form -- launch them one by one then.  All arrays are HOST
 * arrays of n entries.  Results differ from the single launches by the association of the pixel sum only (other split boundaries). */
int aod_conv2d_wgrad_group_plan(const aod_conv_desc_t* const* descs, int n, int32_t* splits_out);
int aod_conv2d_wgrad_grouped(const aod_conv_desc_t* const* descs, int n, const void* const* x, const void* const* dz, float* const* slabs,
                             const int32_t* nslabs, const int64_t* slab_stride, const void* const* row_table, aod_stream_t stream);
/* Sparse backward (see aod_conv2d_ws_map): the same launches following the row-activity map of each member's dZ.  The x3 forms with a SPARSE
 * instance (the two wide forms and the 4-wave 128 x 128 form) deal the active 64-row blocks of the pixel axis to the member's splits
 * cyclically -- active block j goes to split j mod splits -- and a workgroup walks only its share.  A skipped step would have added
 * products of dZ = 0 only; the slabs hold OTHER partial sums than those of the launch without a map, their total is the same gradient in
 * another fp32 summation order.  Other tile forms, non-dense dZ segments and AOD_SPARSE_BWD=0 ignore the map.
 * dz_map: (rows + 63) / 64 bytes per member; NULL (or NULL entries): dense. */
int aod_conv2d_wgrad_grouped_map(const aod_conv_desc_t* const* descs, int n, const void* const* x, const void* const* dz, float* const* slabs,
                                 const int32_t* nslabs, const int64_t* slab_stride, const void* const* row_table, const void* const* dz_map,
                                 aod_stream_t stream);
/* The plan of a weight-gradient launch as data -- the decision the launch itself follows.  Host logic only: nothing is enqueued and no device
 * is needed.  flags: AOD_WGRAD_ATOMIC -- aod_conv2d_wgrad (one member, fp32 atomics) instead of the slab form; AOD_WGRAD_GROUPED -- the
 * grouped launch and its planner (implied for n > 1; one member goes through it as well, with other splits than aod_conv2d_wgrad_slabs);
 * AOD_WGRAD_HAS_MAP(g) -- member g carries a row-activity map of its dZ (the plan drops it where the launch would: not x3, non-dense dZ
 * segments, AOD_SPARSE_BWD=0).
 * form: 0 = 128 x 128 tile, 1 = 256 x 256, 2 / 3 = the wide x3 forms of 8 / 4 waves.  The kernel instance: wide 0 conv_wgrad(_grouped)_kernel
 * <waves, tile, tile, x3, sparse>, wide 1 conv_wgrad(_grouped)_x3w_kernel<waves, tile, sparse> (tile in units of 128 columns), on `grid`
 * workgroups of `threads` threads with lds_bytes of dynamic LDS.  Member g: tiles_n[g] x tiles_k[g] tiles, each over splits[g] splits;
 * split s covers GEMM rows [s * rows_per_split[g], (s + 1) * rows_per_split[g]).
 * Returns 1 (plan not valid) when the members cannot share a grid, -1 on argument errors.
 * aod_conv2d_wgrad_splits, aod_conv2d_wgrad_group_plan and aod_conv2d_wgrad_plan report parts of this plan; aod_conv2d_wgrad_splits still
 * returns 0 for a descriptor without rows and now leaves "empty member" in aod_last_error when it does. */
enum { AOD_WGRAD_ATOMIC = 1, AOD_WGRAD_GROUPED = 2 };
#define AOD_WGRAD_HAS_MAP(g) (16u << (g))
typedef struct {
  int32_t form;
  int32_t wide, waves, tile, x3, sparse, grouped;
  int32_t threads, lds_bytes, grid;
  int32_t tiles_n[4], tiles_k[4], splits[4], rows_per_split[4];
} aod_wgrad_plan_t;
int aod_conv2d_wgrad_plan_ex(const aod_conv_desc_t* const* descs, int n, unsigned flags, aod_wgrad_plan_t* out);
/* The earlier, shorter report of the same plan (flags 0), kept with its signature for its callers: form, and per member splits and
 * rows_per_split.  n = 1 -- aod_conv2d_wgrad_slabs(_map); n = 2 .. 4 -- the grouped launch.  Same return values. */
int aod_conv2d_wgrad_plan(const aod_conv_desc_t* const* descs, int n, int32_t* form, int32_t* splits, int32_t* rows_per_split);
int aod_conv2d_wgrad_slabs_map(const aod_conv_desc_t* desc, const void* x, const void* dz, float* slabs, int nslabs, int64_t slab_stride,
                               const void* row_table, const void* dz_map, aod_stream_t stream);
/* Row table of a forward descriptor (32 B per destination pixel: source block origin, top-left tap, extents,
 * dZ row).  Depends only on segment geometry / stride / pad / filter size: build once, reuse for every wgrad
 * launch with that geometry. */
size_t aod_conv_row_table_bytes(const aod_conv_desc_t* desc);
int aod_conv_row_table(const aod_conv_desc_t* desc, void* table, aod_stream_t stream);

/* OIHW fp32 -> [O][R][S][Ipad] bf16 (forward) / [I][R][S][Opad] bf16 (dgrad); pads zero-filled, multiples of 8.
 * dgrad: `scale` (nullable, fp32 [O]) multiplies output channel o -- the eval-BN scale gamma*rsqrt(var+eps) of
 * resnet.py:647-656 folded into the weights, so that dX = conv_T(gm, scale*W) needs no scaled copy of the gradient. */
int aod_pack_weight_fwd(const float* w_oihw, void* w_packed, int O, int I, int R, int S, int Ipad, aod_stream_t stream);
int aod_pack_weight_dgrad(const float* w_oihw, void* w_packed, int O, int I, int R, int S, int Opad, const float* scale,
                          aod_stream_t stream);
/* [Opad][R][S][Ipad] fp32 (wgrad result) -> OIHW fp32 gradient (first O rows / I channels), times scale[o] when given;
 * accumulate != 0 adds; clear_src != 0 zeroes every element it reads, so a persistent accumulator is all-zero again.
 * wdot (nullable, fp32 [O], overwritten) receives <w_oihw[o], dw[o]> = sum_m gm[m,o] * z[m,o]; with bn_s1 (= sum_m gm[m,o]),
 * bn_mean and bn_invstd it receives invstd * (that - mean * s1) instead: the weight gradient of the eval-mode BatchNorm behind
 * the conv (resnet.py:262-301) without keeping the pre-BN activations z. */
int aod_unpack_wgrad(float* dw_orsi, float* grad_oihw, int O, int I, int R, int S, int Ipad, int accumulate, int clear_src,
                     const float* scale, const float* w_oihw, float* wdot, const float* bn_s1, const float* bn_mean,
                     const float* bn_invstd, aod_stream_t stream);

/* Slab form (aod_conv2d_wgrad_slabs): dw_slabs = [nslabs][Opad][R][S][Ipad] partial sums, added in slab order; at most 16 taps (the product uses it for 10 .. 16 taps in the reference-precision mode only).
 * The slabs of an x3 launch (aod_conv_desc_t.x3) are LOGICAL -- [N/2][R][S][C/2] for the physical widths N, C of the descriptor, slab_stride
 * >= N*R*S*C/4: the (head, head) + (head, tail) + (tail, head) bands of an entry are added in the wgrad epilogue -- and unpack like any
 * other: Opad = N/2, Ipad = C/2. */
int aod_unpack_wgrad_slabs(const float* dw_slabs, int nslabs, int64_t slab_stride, float* grad_oihw, int O, int I, int R, int S, int Ipad,
                           int accumulate, const float* scale, const float* w_oihw, float* wdot, const float* bn_s1,
                           const float* bn_mean, const float* bn_invstd, aod_stream_t stream);

/* ... and the unpacks of a grouped launch in one grid (arrays of n <= 4 entries; entries of scale / w_oihw / wdot / bn_* may be NULL). */
int aod_unpack_wgrad_slabs_grouped(int n, const float* const* dw_slabs, const int32_t* nslabs, const int64_t* slab_stride, float* const* g,
                                   const int32_t* O, const int32_t* I, const int32_t* R, const int32_t* S, const int32_t* Ipad,
                                   const int32_t* accumulate, const float* const* scale, const float* const* w_oihw, float* const* wdot,
                                   const float* const* bn_s1, const float* const* bn_mean, const float* const* bn_invstd,
                                   aod_stream_t stream);
/* Batched re-derivation of everything the conv launches read from the parameters, for ALL layers in one launch (after an optimizer
 * step every trainable layer is stale): items_dev = device array of `nitems` records of aod_param_prep_item_bytes() bytes,
 *   { const float* w_oihw, gamma, beta, mean, var;  void* w_fwd_packed, w_dgrad_packed;  float* scale, shift, invstd;
 *     int32 O, I, RS, Ipad, Opad, blk0;  float eps;  int32 flags;  int64 pad[2] }
 * flags bit 0: X3 images for aod_conv_desc_t.x3 launches -- the packed channel axis of both images is in the X-layout (Ipad / Opad =
 * the physical widths 2*ceil32(I) / 2*ceil32(O); head = bf16(v), tail = bf16(v - head)) and an item owns ceil32(O)/32 * ceil32(I)/32 blocks.
 * gamma == NULL: conv without BatchNorm (plain packs); w_dgrad_packed == NULL: no dgrad image.  With BN the dgrad image carries
 * scale[o] = gamma*rsqrt(var+eps) (see aod_pack_weight_dgrad) and scale/shift/invstd receive the folded eval-mode BN vectors
 * (resnet.py:647-656).  blk0 = first block of the item; an item owns ceil(Opad/32)*ceil(Ipad/32) blocks (32 x 32 channel tiles), or
 * ceil(max(O*RS*Ipad, I*RS*Opad, O)/2048) blocks when RS > 9. */
int aod_param_prep(const void* items_dev, int nitems, int total_blocks, aod_stream_t stream);
int aod_param_prep_item_bytes(void);

/* ------------------------------------------------------------------ layout / elementwise
 * NCHW fp32 image -> NHWC bf16 with channels zero-padded to Cpad (stem input). replaces the
 * implicit layout of `img` in SSL_L_single_stage.py:45-49 extract_feat. */
int aod_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int B, int C, int H, int W, int Cpad, aod_stream_t stream);
/* Stem input in space-to-depth form: fp32 [B][C <= 4][H][W] (H, W even) -> bf16 [B][H/2][W/2][16], channel slot (dy * 2 + dx) * C + c =
 * pixel (2Y + dy, 2X + dx), remaining slots zero.  The 7x7 / stride-2 / pad-3 stem conv (mmdet/models/backbones/resnet.py:575-600)
 * over the image equals a 4x4 / stride-1 / pad-2 conv over this tensor with the filter taps regrouped the same way. */
int aod_nchw_f32_to_s2d_bf16(const float* src, void* dst, int B, int C, int H, int W, aod_stream_t stream);
/* The frozen stem in one launch on the space-to-depth image: y = max_pool_3x3_s2_p1(relu(bn1(conv1(x)))) (resnet.py:630-637; conv1 as the
 * 4x4 / stride-1 / pad-2 filter [64][4][4][16] over x_s2d [B][H2][W2][16]).  y [B][H4][W4][64] bf16 with H4 = (H2 - 1) / 2 + 1; the
 * 64-channel conv output never leaves LDS (csrc/stem.hip). */
int aod_stem_pool_fwd(const void* x_s2d, const void* w_packed, const float* scale, const float* shift, void* y, int B, int H2, int W2,
                      aod_stream_t stream);
/* MaxPool 3x3 s2 p1, NHWC bf16 (resnet.py:610). */
int aod_maxpool3x3s2(const void* src, void* dst, int B, int H, int W, int C, aod_stream_t stream);
/* FPN top-down: dst[b,y,x,c] += src[b,y/2,x/2,c] (nearest 2x, fpn.py:163-172) and its adjoint */
int aod_upsample2x_add(const void* src, void* dst, int B, int h, int w, int C, int H, int W, aod_stream_t stream);
int aod_upsample2x_add_bwd(const void* g_dst, void* g_src_accum, int B, int h, int w, int C, int H, int W, aod_stream_t stream);
/* out = lateral + nearest_upsample(top) without touching the lateral (fpn.py:163-172: `laterals[i-1] += F.interpolate(laterals[i])`
 * whose in-place add autograd turns into a copy), and the adjoint that WRITES g_top (no zero fill of the destination). */
int aod_upsample2x_add_to(const void* top, const void* lateral, void* out, int B, int h, int w, int C, int H, int W, aod_stream_t stream);
int aod_upsample2x_add_bwd_set(const void* g_dst, void* g_src, int B, int h, int w, int C, int H, int W, aod_stream_t stream);
/* Backward of y = act(z*scale+shift [+res]) in eval-mode BN (resnet.py:262-301):
 * gm = g * (a > 0 if relu);  dz = gm * scale[n];  dbeta[n] += sum_m gm;  dgamma[n] += sum_m gm * (z - mean[n]) * invstd[n].
 * gmask_out (optional) receives gm (gradient for the residual branch); z/mean/invstd NULL -> bias-only mode
 * (ConvModule bias+ReLU, Lambda_L2.py:44-51): dz = gm, dbeta = column sum.  dbeta/dgamma are fp32, accumulated. */
int aod_act_bwd(const void* g, const void* a, const void* z, const float* scale, const float* mean, const float* invstd,
                void* dz, void* gmask_out, float* dbeta, float* dgamma, int64_t M, int N, int relu, int g_is_f32,
                aod_stream_t stream);
/* dz[M,Npad] (bf16) = pad(g[M,N] * (relu_out > 0 if given));  colsum[n] += sum_m of the same
 * (gradients of the N = 180/36/9 prediction convs; relu_out_f32 = retina_L's fp32 output, Lambda_L2.py:101) */
int aod_pad_cast_colsum(const void* g, const float* relu_out_f32, void* dz, float* colsum, int64_t M, int N, int Npad,
                        int g_is_f32, aod_stream_t stream);
/* out = relu(a + b) bf16 and backward mask (bottleneck join, resnet.py:292-299) */
int aod_add_relu(const void* a, const void* b, void* out, int64_t n, aod_stream_t stream);

/* 3x3 / stride-1 / pad-1 conv with the input halo tile resident in LDS (csrc/halo_conv.hip) for the layers whose output is narrow next to
 * their input: the prediction convs retina_cls / retina_reg / retina_L over all pyramid levels (mmdet/models/dense_heads/Lambda_L2.py:52-54,
 * 92-103) and their dgrads (desc->transposed = 1 with the aod_pack_weight_dgrad packing: taps mirrored).  Same descriptor as aod_conv2d;
 * v = acc + pre_shift[n]; if (mask) v = mask[m][n] > 0 ? v : 0; if (relu) v = max(v, 0); colsum[n] += sum_m v.  desc->C <= 256, N <= 256.
 * aod_halo_conv3x3_applies() tells whether a descriptor qualifies. */
int aod_halo_conv3x3_applies(const aod_conv_desc_t* desc);
int aod_halo_conv3x3(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst, const float* pre_shift,
                     const void* mask, float* colsum, aod_stream_t stream);

/* ------------------------------------------------------------------ losses (K6-K8)
 * replaces: mmcv.ops.sigmoid_focal_loss fwd/bwd CUDA kernels + softmax/log chain at
 *   mmdet/models/losses/EDL_Softmax_FocalLoss.py:9-27,51-69, L1 at smooth_l1_loss.py:33-45,
 *   reductions at losses/utils.py:28-54, called from Lambda_L2.py:112-121.
 * cls [Nrows, C] fp32 logits, labels int64 (C == background), label_w fp32, bbox_* [Nrows,4] fp32.
 * Outputs: loss_noR[Nrows]; sums[0] += sum(l*w), sums[1] += sum(|p-t|*bw), sums[2] += sum(loss_noR)
 * (deterministic two-stage reduction; `partials` is a caller workspace of aod_loss_partials_len floats). */
size_t aod_loss_partials_len(int64_t nrows);
int aod_edl_focal_l1_fwd(const float* cls, const int64_t* labels, const float* label_w,
                         const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                         int64_t nrows, int C, float gamma, float alpha,
                         float* loss_noR, float* sums3, float* partials, aod_stream_t stream);
/* grad_cls = d(sum(l*w))*g_cls + d(sum_rows loss_noR * g_noR[row]);  grad_bbox = sign(p-t)*bw*g_bbox.
 * g_cls, g_bbox: device scalars (already divided by avg_factor); g_noR: device [Nrows] -- or ONE device scalar applied to every row when
 * g_noR_is_scalar != 0 (the gradient of mean(loss_noR), Lambda_L2.py:112-121 + SSL_Lambda.py:136-141, without materialising it) -- or NULL,
 * g_noR_scalar: host scalar used when g_noR is NULL.  Output element (row r, col c) is written at
 * (r / A) * pitch + (r % A) * C + c -- i.e. straight into the prediction conv's [pixels, pitch] dZ
 * buffer (pitch = A*C rounded up to 8, pad columns pre-zeroed by the caller) -- as bf16 or fp32. */
int aod_edl_focal_l1_bwd(const float* cls, const int64_t* labels, const float* label_w,
                         const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                         int64_t nrows, int C, float gamma, float alpha,
                         const float* g_cls, const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar,
                         void* grad_cls, void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box,
                         aod_stream_t stream);
/* Elementwise form [Nrows, C] of the same loss: what EDL_Softmax_FocalLoss.forward(reduction='none') returns
 * (EDL_Softmax_FocalLoss.py:51-69 -> mmcv.ops.sigmoid_focal_loss(..., 'none'), :17).  grad_out == NULL: out[r][c] = l_c (forward);
 * grad_out = upstream gradient [Nrows, C]: out = gradient w.r.t. the logits (backward through softmax -> logit -> focal term). */
int aod_edl_focal_elem(const float* cls, const int64_t* labels, int64_t nrows, int C, float gamma, float alpha,
                       const float* grad_out, float* out, aod_stream_t stream);
/* MEH loss (Lambda_L2.py:235-241): out_sum[0] += sum(((|lam+1e-9-loss|)*w)^2), w = bbox_w4[i*4];
 * grad = g[0]*2*w^2*(lam+1e-9-loss) written at (i / A) * pitch + i % A.  partials: >= aod_loss_partials_len(n) floats */
int aod_meh_loss_fwd(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n,
                     float* out_sum, float* partials, aod_stream_t stream);
int aod_meh_loss_bwd(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n,
                     const float* g, void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream);
/* The same four passes over ALL pyramid levels in one launch each (the reference runs loss_single / loss_single_L once per level through
 * multi_apply: L_anchor_head.py:306-314,322-327, Lambda_L2.py:105-121,235-241).  The levels' anchor rows are adjacent row ranges of every
 * operand (level l = rows [sum(level_rows[:l]), + level_rows[l]), what the level-batched prediction convs and the level-major targets of
 * aod_max_iou_assign produce); level_rows: HOST array of nlevels <= 8 row counts.  Blocks never straddle a level and every sum runs in the
 * order of a per-level call: loss_noR, the sums and the gradients are bit-identical to nlevels separate calls.
 *   sums [3][nlevels]  (written, not accumulated): row 0 = sum(l*w), row 1 = sum(|p-t|*bw), row 2 = sum(loss_noR) of each level
 *   num_pos (optional, device int32 [num_images], aod_max_iou_assign's per-image positive counts): the sums are then DIVIDED in place --
 *     rows 0, 1 by num_total_samples = sum_b max(num_pos[b], 1) (L_anchor_head.py:300-303, what loss_single divides by at :266-288), row 2 by
 *     the level's row count (the mean of SSL_Lambda.py:136-141) -- with IEEE divisions; divisors [3][nlevels] and num_total [1] are written
 *   g_sums [3][nlevels]: their gradients (device) -- of the divided sums when the forward's `divisors` are passed (else NULL);
 *   g_noR_rows: optional per-row gradient of loss_noR, then used INSTEAD of row 2
 *   out_sums [nlevels] / g [nlevels]: the MEH sums and their gradients.  partials: >= aod_loss_levels_partials_len floats. */
size_t aod_loss_levels_partials_len(int nlevels, const int64_t* level_rows);
int aod_edl_focal_l1_levels_fwd(const float* cls, const int64_t* labels, const float* label_w,
                                const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                                int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                                float* loss_noR, float* sums, float* partials, const int32_t* num_pos, int num_images,
                                float* divisors, float* num_total, aod_stream_t stream);
int aod_edl_focal_l1_levels_bwd(const float* cls, const int64_t* labels, const float* label_w,
                                const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                                int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                                const float* g_sums, const float* divisors, const float* g_noR_rows, void* grad_cls, void* grad_bbox, int out_bf16,
                                int A, int pitch_cls, int pitch_box, aod_stream_t stream);
/* The plain RetinaNet baseline's loss (MyRetinaHead.py:91-109 -> FocalLoss, mmdet/models/losses/focal_loss.py:85 -> mmcv.ops.sigmoid_focal_loss)
 * + the same L1 box term: mmcv-full 1.3.8's focal term applied to the RAW logits, per class, no softmax in front of it:
 *   q = 1 / (1 + exp(-x_c));  target class: -alpha (1-q)^gamma log(max(q, FLT_MIN));  others: -(1-alpha) q^gamma log(max(1-q, FLT_MIN))
 * (a label of C = background makes every column negative).  The gradient is that expression's derivative per class, clamps as written.
 * Each entry takes exactly the arguments of its aod_edl_focal_l1_* / aod_edl_focal_elem counterpart above -- sums, partials, num_pos /
 * divisors, g_noR_rows, the (A, pitch) dZ layout in bf16 or fp32 -- and is the same kernel with another compile-time form: same blocks,
 * same summation orders, the level-fused launches bit-identical to per-level ones. */
int aod_sigmoid_focal_l1_fwd(const float* cls, const int64_t* labels, const float* label_w,
                             const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                             int64_t nrows, int C, float gamma, float alpha,
                             float* loss_noR, float* sums3, float* partials, aod_stream_t stream);
int aod_sigmoid_focal_l1_bwd(const float* cls, const int64_t* labels, const float* label_w,
                             const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                             int64_t nrows, int C, float gamma, float alpha,
                             const float* g_cls, const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar,
                             void* grad_cls, void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box,
                             aod_stream_t stream);
int aod_sigmoid_focal_l1_levels_fwd(const float* cls, const int64_t* labels, const float* label_w,
                                    const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                                    int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                                    float* loss_noR, float* sums, float* partials, const int32_t* num_pos, int num_images,
                                    float* divisors, float* num_total, aod_stream_t stream);
int aod_sigmoid_focal_l1_levels_bwd(const float* cls, const int64_t* labels, const float* label_w,
                                    const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                                    int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                                    const float* g_sums, const float* divisors, const float* g_noR_rows, void* grad_cls, void* grad_bbox,
                                    int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream);
/* The eight passes above with the focal form AND the box form as arguments; the entries above are box_form 0 and return the
 * same bits through these.  focal_form 0 = EDL softmax-focal, 1 = sigmoid focal.  The box term of a row (what enters sums row 1):
 *   box_form 0  l1    sum_j |pred_j - tgt_j| * bw_j on the encoded deltas; box_eps / box_linear / the coder are not read (may be NULL)
 *   box_form 1  iou   w * -log(max(IoU, box_eps)), or w * (1 - max(IoU, box_eps)) when box_linear   (mmdet IoULoss, iou_loss.py:14-36)
 *   box_form 2  giou  w * (1 - (IoU - (E - U) / E)), U = max(U, box_eps), E = max(E, box_eps)        (mmdet GIoULoss, iou_loss.py:87-102)
 * with w = (bw_0 + bw_1 + bw_2 + bw_3) / 4.  A row with w == 0 is not evaluated: it adds exactly 0 and its four gradients are +0, whatever
 * bbox_pred / bbox_tgt hold there (NaN and inf included).  Forms 1, 2 decode bbox_pred[r] and bbox_tgt[r] -- both encoded deltas, as for
 * form 0 -- in the anchor-normalised frame: t = delta * stds4 + means4 (HOST float[4] each, stds > 0), centre (t0, t1), size
 * (exp(clamp(t2)), exp(clamp(t3))), clamp to +-|ln(wh_ratio_clip)|, corners centre -+ size / 2; bbox_overlaps(is_aligned=True) of
 * iou2d_calculator.py:212-260 on the two boxes.  IoU, and (E - U) / E, do not change under the per-axis scaling and translation that takes
 * this frame to pixels, so no anchor is read.  Gradients: autograd's, through the decode; a tie of torch.max(a, b) / torch.min(a, b) hands
 * each side half, clamp(min=m) passes where x >= m, the size clamp passes on [-|ln clip|, |ln clip|].  Needs bbox_pred (non-NULL) and
 * 16-B aligned bbox_* for forms 1, 2. */
int aod_focal_box_fwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                         float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w,
                         const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                         int64_t nrows, int C, float gamma, float alpha,
                         float* loss_noR, float* sums3, float* partials, aod_stream_t stream);
int aod_focal_box_bwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                         float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w,
                         const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                         int64_t nrows, int C, float gamma, float alpha,
                         const float* g_cls, const float* g_bbox, const float* g_noR, float g_noR_scalar, int g_noR_is_scalar,
                         void* grad_cls, void* grad_bbox, int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream);
int aod_focal_box_levels_fwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                                float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w,
                                const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                                int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                                float* loss_noR, float* sums, float* partials, const int32_t* num_pos, int num_images,
                                float* divisors, float* num_total, aod_stream_t stream);
int aod_focal_box_levels_bwd_ex(int focal_form, int box_form, float box_eps, int box_linear, const float* means4, const float* stds4,
                                float wh_ratio_clip, const float* cls, const int64_t* labels, const float* label_w,
                                const float* bbox_pred, const float* bbox_tgt, const float* bbox_w,
                                int nlevels, const int64_t* level_rows, int C, float gamma, float alpha,
                                const float* g_sums, const float* divisors, const float* g_noR_rows, void* grad_cls, void* grad_bbox,
                                int out_bf16, int A, int pitch_cls, int pitch_box, aod_stream_t stream);
/* FocalLoss.forward(reduction='none') (focal_loss.py:85): out[r][c] = l_c, or with grad_out the gradient grad_out[r][c] * d l_c / d x_c */
int aod_sigmoid_focal_elem(const float* cls, const int64_t* labels, int64_t nrows, int C, float gamma, float alpha,
                           const float* grad_out, float* out, aod_stream_t stream);
int aod_meh_loss_levels_fwd(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                            float* out_sums, float* partials, aod_stream_t stream);
int aod_meh_loss_levels_bwd(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                            const float* g, void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream);
/* The four MEH passes with the loss FORM of the reference's ablation heads; the entries above are form = 0.  Per row, d = the form's
 * difference, w = bbox_w4[i*4], in fp32; same partial sums, same reduction order and the same gradient layout as above.
 *   form 0  L2    (Lambda_L2.py:235-241)    d = lam+1e-9 - loss                   term (|d|*w)^2   grad g*2*w^2*d
 *   form 1  L1    (Lambda_L1.py:236-241)    d = lam+1e-9 - loss                   term ||d|*w|     grad g*|w|*sign(d), 0 where d == 0
 *   form 2  MSLE  (Lambda_MSLE.py:236-242)  d = log(lam+1e-9+1) - log(loss+1)     term (|d|*w)^2   grad g*2*(|d|*w)*w*sign(d)/(lam+1e-9+1) */
int aod_meh_loss_fwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n, int form,
                        float* out_sum, float* partials, aod_stream_t stream);
int aod_meh_loss_bwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int64_t n, int form,
                        const float* g, void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream);
int aod_meh_loss_levels_fwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                               int form, float* out_sums, float* partials, aod_stream_t stream);
int aod_meh_loss_levels_bwd_ex(const float* lam, const float* loss_noR, const float* bbox_w4, int nlevels, const int64_t* level_rows,
                               int form, const float* g, void* grad_lam, int out_bf16, int A, int pitch, aod_stream_t stream);

/* ------------------------------------------------------------------ geometry (K9, K10)
 * replaces: AnchorGenerator.grid_anchors/valid_flags (core/anchor/anchor_generator.py:308-438),
 *   MaxIoUAssigner.assign (core/bbox/assigners/max_iou_assigner.py:60-210) + bbox_overlaps
 *   (iou2d_calculator.py:212-252) + PseudoSampler + bbox2delta (delta_xywh_bbox_coder.py:98-140)
 *   + unmap, as driven by L_anchor_head.py:155-257.  Bit-exact integer outputs.
 * anchors [A,4] fp32; valid [B,A] uint8; gts packed [B, Gmax, 4] fp32 with gt_count[B], gt_labels [B,Gmax] int64.
 * outputs: assigned [B,A] int64, labels [B,A] int64, label_w [B,A] f32, bbox_t [B,A,4], bbox_w [B,A,4],
 * num_pos [B] int32.  ws: workspace of aod_assign_ws_bytes(B, Gmax).  nlev > 0 with level_start_host[nlev+1]
 * (anchor offsets of the pyramid levels, HOST array) writes the outputs level-major [L][B][A_l] so that every
 * level's targets are one contiguous block (images_to_levels, anchor/utils.py:4-17, without a copy). */
size_t aod_assign_ws_bytes(int B, int Gmax);
int aod_max_iou_assign(const float* anchors, const uint8_t* valid, int64_t A, int B,
                       const float* gts, const int32_t* gt_count, const int64_t* gt_labels, int Gmax,
                       float pos_thr, float neg_thr, float min_pos_iou, int gt_max_assign_all, int num_classes,
                       const float* means4, const float* stds4,
                       int64_t* assigned, int64_t* labels, float* label_w, float* bbox_t, float* bbox_w,
                       int32_t* num_pos, void* ws, int nlev, const int64_t* level_start_host, aod_stream_t stream);

/* ------------------------------------------------------------------ scoring (K11-K13)
 * replaces Lambda_L2.py:264-304: alphas = softmax; scores = alphas / (sum(alphas) + 1e-20 + 1e-9); row max; level gate
 * (any anchor of the level with max alpha > fg_thr, Lambda_L2.py:497-502).  cls [B, rows_per_img, C] fp32 (one level);
 * rowmax [B, rows_per_img]; any_fg [B] int32 (OR-ed into; caller zeroes).  has_bg = 1 (SSD, My_L_ssd_head.py:331-345): plain softmax
 * over C logits whose last column is background, maxima over the C-1 foreground columns.  has_bg = 2 (the plain RetinaNet baseline,
 * anchor_head.py:535-554 with last_activation == 'sigmoid'): s_c = 1 / (1 + exp(-x_c)) per class, both maxima over all C columns. */
int aod_softmax_rowmax(const float* cls, int B, int64_t rows_per_img, int C, float fg_thr, float* rowmax, int32_t* any_fg,
                       int has_bg, aod_stream_t stream);
/* per image stable top-k (k <= 1024; descending score, ties -> lower index) of score [B, A] -> idx [B, out_pitch] int32
 * (torch.topk at Lambda_L2.py:290; its tie order is unspecified, pinned here) */
int aod_topk_stable(const float* score, int B, int64_t A, int k, int32_t* idx, int64_t out_pitch, aod_stream_t stream);
/* gather + decode ONE level into the concatenated candidate arrays (Lambda_L2.py:292-308,325-326; delta2bbox
 * delta_xywh_bbox_coder.py:144-262): for candidate j (anchor idx[b][j], or j itself when idx == NULL):
 * boxes [B, n_total, 4] (clipped to img_hw[b] = (H, W), divided by scale4[b] when given), scores [B, n_total, C+1]
 * (normalised softmax + zero background column), lam [B, n_total], cand_anchor [B, n_total] = anchor0 + anchor index,
 * written at candidate offset cand0.  normalize: 1 normalised evidence scores, 0 raw softmax (Entropy_ALL), 2 softmax incl. a
 * background logit (SSD: C logits -> C score columns, no padding column), 3 per-class sigmoid scores (anchor_head.py:535-536,592-596:
 * C score columns + the zero background column; aod_pre_nms_levels(normalize = 3) scans with has_bg = 2 itself and refuses has_bg != 0). */
int aod_gather_decode(const float* cls, const float* reg, const float* lam_map, const float* anchors, const int32_t* idx,
                      int B, int64_t A, int k, int C, int64_t idx_pitch, const float* img_hw, const float* scale4,
                      const float* means4, const float* stds4, float wh_ratio_clip, float* boxes, float* scores, float* lam,
                      int32_t* cand_anchor, int64_t n_total, int64_t cand0, int64_t anchor0, int normalize, aod_stream_t stream);
/* The three steps above for ALL L (<= 8) pyramid levels of a batch in two launches (the per-level loop of Lambda_L2.py:264-310 /
 * My_L_ssd_head.py:331-365): one scan of every level's logits, then one workgroup per (image, level) that selects the level's top-k[l]
 * (where k[l] < A[l]) and gathers + decodes its candidates.  cls / reg / lam_map / anchors / A / k: HOST arrays of L entries.
 * rowmax: [sum_l B*A[l]] level-major (level l = a [B, A[l]] block); any_fg [L, B] (zeroed by the caller); idx: level-major [B, k[l]]
 * blocks of the levels with k[l] < A[l] only (may be NULL when there is none); n_total = sum_l k[l].  Results are those of the
 * per-level entry points bit for bit. */
int aod_pre_nms_levels(int L, const float* const* cls, const float* const* reg, const float* const* lam_map, const float* const* anchors,
                       const int64_t* A, const int32_t* k, int B, int C, float fg_thr, int has_bg, int normalize, const float* img_hw,
                       const float* scale4, const float* means4, const float* stds4, float wh_ratio_clip, float* rowmax, int32_t* any_fg,
                       int32_t* idx, float* boxes, float* scores, float* lam, int32_t* cand_anchor, int64_t n_total, aod_stream_t stream);
/* multiclass_nms (core/post_processing/bbox_nms.py:7-93 -> mmcv batched_nms / nms_cpu semantics, both its <10000 and
 * per-class paths reduce to this class-aware greedy scan).  boxes [B,n,4], scores [B,n,C+1]; outputs dets [B,max_num,5],
 * det_labels [B,max_num] int64, keep [B,max_num] int64 (index into the score>thr list; -1 padded), num_det [B] int32. */
size_t aod_nms_ws_bytes(int B, int n, int C);
int aod_multiclass_nms(const float* boxes, const float* scores, int B, int n, int C, float score_thr, float iou_thr,
                       int max_num, float* dets, int64_t* det_labels, int64_t* keep, int32_t* num_det,
                       void* ws, aod_stream_t stream);
/* tpfp_default (mmdet/core/evaluation/mean_ap.py:154-239, area_ranges=None) for a whole batch, all classes and T (1..8) IoU thresholds in
 * one launch.  dets [B,M,5] / labels [B,M] int64 / num [B] int32: the outputs of aod_multiclass_nms (rows >= num[b] are never read;
 * M <= 2048).  gt_boxes [B,G,4], gt_labels [B,G] int32, gt_ignore [B,G] uint8, gt_num [B] int32: per image the real gts in annotation
 * order, THEN the ignored gts in annotation order (the host stacks gt_bboxes above gt_bboxes_ignore per class and argmax takes the first
 * maximum; the packed list filtered by class has that order).  iou_thr_host: HOST array of T thresholds, compared as fp32.
 * flags [T,B,M] uint8: 0 neither (best gt ignored, or row >= num[b]), 1 tp, 2 fp.  Claimants of one gt rank by descending score, ties by
 * lower row (stable); IoU is bbox_overlaps (bbox_overlaps.py:4-48) bit for bit in fp32.  No workspace, no host sync. */
int aod_eval_match(const float* dets, const int64_t* labels, const int32_t* num, const float* gt_boxes, const int32_t* gt_labels,
                   const uint8_t* gt_ignore, const int32_t* gt_num, int B, int M, int G, const float* iou_thr_host, int T,
                   uint8_t* flags, aod_stream_t stream);
/* COCO bbox matching (replaces the per-image loop of core/coco_eval.py evaluate_bbox: coco_eval.match_image once per image and
 * class) for a whole batch, all classes, A (1..4) area ranges and T (1..16) IoU thresholds in one launch.  dets / labels / num as for
 * aod_eval_match (M <= 1024).  gt_boxes [B,G,4] fp64 xywh, gt_area [B,G] fp64 (the annotation's area, which the range test reads),
 * gt_label [B,G] int32, gt_crowd [B,G] uint8, gt_num [B] int32: the image's gts in file order (G <= 512).  area_rng_host: HOST array of
 * A (lo, hi) pairs, inclusive; iou_thr_host: HOST array of T thresholds; both fp64.  states [A,T,B,M] uint8: 1 matched to a counted gt,
 * 0 unmatched and counted, 2 ignored (matched to an ignored gt, or unmatched with its own area outside the range); rows >= num[b] are 0.
 * Detections rank by descending score, ties by lower row; IoU is coco_eval.iou_matrix bit for bit in fp64.  No workspace, no host sync.
 * Scores must not be NaN: such rows have no rank, and some rows below num[b] are then left unwritten (the caller zeroes `states` first if
 * it cannot rule NaN out; core/coco_eval_device.py does). */
int aod_coco_match(const float* dets, const int64_t* labels, const int32_t* num, const double* gt_boxes, const double* gt_area,
                   const int32_t* gt_label, const uint8_t* gt_crowd, const int32_t* gt_num, int B, int M, int G,
                   const double* area_rng_host, int A, const double* iou_thr_host, int T, uint8_t* states, aod_stream_t stream);

/* ------------------------------------------------------------------ HUA (K13-K15)
 * replaces GetObjectIdx + ComputeObjUnc + AggregateObjScaleUnc (Lambda_L2.py:343-349,489-537,597-619;
 * torch._sample_dirichlet): per image, (candidate,object) pairs -> num_samples Dirichlet samples -> epistemic ->
 * (object, level, class) bins -> class/scale/object aggregation -> unc[B].
 * level_start_host[L+1]: candidate offsets of the concatenated levels (HOST array); level_any_fg [L][B] int32;
 * cand_anchor [B,n] global anchor id and image_ids [B] int64 key the counter RNG (partition invariant);
 * agg3_host = (class, scale, object) codes 0 Sum / 1 Avg / 2 Max (HOST array; NULL = Sum/Max/Sum).
 * scale_mode = 1: Entropy_ALL / ComputeScaleUnc + AggregateScaleUnc (Lambda_L2.py:539-569,636-691): every candidate whose max
 * score exceeds fg_thr is a pair of one pseudo object, lambda mean over ALL candidates of the level, scores = raw softmax.
 * dirichlet_cols: C (evidence head; 0 = default) or C+1 (SSD: the background probability is a Dirichlet component too).
 * pair_out (optional, [B, max_pairs, 4] f32: cand, obj, aleatoric, epistemic); pair_count [B] int32 (may exceed
 * max_pairs: then the excess pairs were dropped and the caller must retry with a larger workspace). */
size_t aod_hua_ws_bytes(int B, int max_pairs);
int aod_hua_score(const float* boxes, const float* scores, const float* lam, const int32_t* cand_anchor,
                  const float* dets, const int32_t* num_det, const int32_t* level_start_host, const int32_t* level_any_fg,
                  const int64_t* image_ids, int B, int n, int L, int C, int max_num, float obj_score_thr, float obj_iou_thr,
                  float fg_thr, int num_samples, uint64_t seed, const int32_t* agg3_host, int clsW, int scale_mode,
                  int dirichlet_cols, float* unc, float* pair_out, int max_pairs, int32_t* pair_count, void* ws, aod_stream_t stream);
/* aod_hua_score with two opt-in extensions (same reference call site: Lambda_L2.py:343-349,489-537,597-619); aod_hua_score is
 * aod_hua_score_ex(..., estimator = 0, obj_out = NULL, obj_pairs = NULL).
 * estimator: 0 = Monte-Carlo (num_samples Dirichlet draws, Philox stream keyed by seed / image_ids / cand_anchor);
 *            1 = closed form of the Monte-Carlo limit, per pair in fp32: S = sum a_c, m_c = a_c / S, total = -sum m_c ln m_c,
 *                aleatoric = psi(S+1) - sum m_c psi(a_c+1), epistemic = total - aleatoric (a_c == 0 contributes 0);
 *                num_samples, seed and image_ids are not read.
 * obj_out (optional, [B, max_num, 2] f32) / obj_pairs ([B, max_num] int32; NULL iff obj_out is NULL): per DETECTION ROW of dets[b],
 * (aleatoric, epistemic) after the class and scale folds -- the epistemic value is the term the object fold consumes -- and the number
 * of pairs the row's object owns; (NaN, NaN, 0) for rows with score <= obj_score_thr, rows >= num_det and objects without a pair.
 * Not offered with scale_mode = 1. */
int aod_hua_score_ex(const float* boxes, const float* scores, const float* lam, const int32_t* cand_anchor,
                     const float* dets, const int32_t* num_det, const int32_t* level_start_host, const int32_t* level_any_fg,
                     const int64_t* image_ids, int B, int n, int L, int C, int max_num, float obj_score_thr, float obj_iou_thr,
                     float fg_thr, int num_samples, uint64_t seed, const int32_t* agg3_host, int clsW, int scale_mode,
                     int dirichlet_cols, float* unc, float* pair_out, int max_pairs, int32_t* pair_count, int estimator,
                     float* obj_out, int32_t* obj_pairs, void* ws, aod_stream_t stream);
/* aod_hua_score_ex for the reference's ablation heads; aod_hua_score_ex is aod_hua_score_ex2(..., lam_mode = 0) with scale_mode 0 / 1.
 * lam_mode: 0 = alpha = score * mean(lambda) / (lambda + 1e-7) * 25 (Lambda_L2.py:513-516, 551-554);
 *           1 = alpha = score: Lambda_L2Net_NoL's ComputeObjUnc / ComputeScaleUnc (Lambda_L2_noL.py:526-532, 586-592), lam is not read.
 * scale_mode = 2: Entropy_Avg, ComputeAvgUnc + AggregateAvgUnc (Lambda_L2_noL.py:552-572, 631-640): the pairs of scale_mode = 1 (every
 *   candidate whose max score exceeds fg_thr, pseudo object 0, same Philox keying), no class bins: unc[b] = mean over the levels that own a
 *   pair of (mean of the level's per-pair epistemic values), 0 when no level owns one (the reference yields NaN there, and drops a level
 *   whose mean is exactly 0.0: neither is reproduced).  Fixed summation order, no atomics: an image's score does not depend on its batch.
 *   With num_samples = 50, lam_mode = 1, estimator = 0 this is the reference's pool; estimator = 1 is its n -> infinity limit, NOT its
 *   50-sample expectation (the `total` term, the entropy of the mean of n samples, is biased downwards at finite n).  agg3_host and clsW are not read. */
int aod_hua_score_ex2(const float* boxes, const float* scores, const float* lam, const int32_t* cand_anchor,
                      const float* dets, const int32_t* num_det, const int32_t* level_start_host, const int32_t* level_any_fg,
                      const int64_t* image_ids, int B, int n, int L, int C, int max_num, float obj_score_thr, float obj_iou_thr,
                      float fg_thr, int num_samples, uint64_t seed, const int32_t* agg3_host, int clsW, int scale_mode,
                      int dirichlet_cols, float* unc, float* pair_out, int max_pairs, int32_t* pair_count, int estimator, int lam_mode,
                      float* obj_out, int32_t* obj_pairs, void* ws, aod_stream_t stream);

/* ------------------------------------------------------------------ SSD300-VGG16 variant (BASELINE config 0)
 * generic NHWC bf16 max-pool fwd/bwd (mmcv VGG pools, ceil_mode, + the 3x3 s1 p1 pool5 of backbones/ssd_vgg.py:66-68) */
int aod_maxpool_fwd(const void* x, void* y, int B, int H, int W, int C, int OH, int OW, int k, int s, int p, aod_stream_t stream);
int aod_maxpool_bwd(const void* x, const void* g, void* gx, int B, int H, int W, int C, int OH, int OW, int k, int s, int p,
                    aod_stream_t stream);
/* L2Norm (necks/ssd_neck.py:105-128): y = w[c] * x / (||x||_2 + eps) per pixel; bwd accumulates gw (fp32) */
int aod_l2norm_fwd(const void* x, const float* w, void* y, int64_t rows, int C, float eps, aod_stream_t stream);
int aod_l2norm_bwd(const void* x, const float* w, const void* g, void* gx, float* gw, int64_t rows, int C, float eps, aod_stream_t stream);
/* SSD loss per image (My_L_ssd_head.py:182-215): ce[b][a] = CE(logits, label) * w (== loss_noR); sums3[b] = (sum_pos ce + sum of the
 * min(ratio * #pos, #neg) largest negative ce, sum smooth_l1 * w, mean ce); sel4[b] = selection record consumed by the backward. */
int aod_ssd_loss_fwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred, const float* bbox_tgt,
                     const float* bbox_w, int B, int A, int C1, int num_classes, int neg_pos_ratio, float beta, float* ce, float* sums3,
                     uint32_t* sel4, aod_stream_t stream);
int aod_ssd_loss_bwd(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred, const float* bbox_tgt,
                     const float* bbox_w, const float* ce, const uint32_t* sel4, int B, int A, int C1, int num_classes, float beta,
                     const float* g_cls, const float* g_box, const float* g_noR, float* grad_cls, float* grad_box, aod_stream_t stream);

/* ------------------------------------------------------------------ synthetic pool (bench harness; nothing to replace in the reference:
 * its pool is VOC images from disk, tools/train_RetinaNet.py:221-225).  dst [B, elems_per_image] fp32 ~ N(0,1), a pure function of
 * (seed, image_ids[b], element index): Philox4x32-10 keyed like the HUA sampler, so a sharded pool scores the same
 * images for any world size.  elems_per_image % 4 == 0. */
int aod_synth_normal_images(float* dst, int B, int64_t elems_per_image, uint64_t seed, const int64_t* image_ids, aod_stream_t stream);

/* ------------------------------------------------------------------ device-side image transforms (pipelines.py, device_transforms=True)
 * Replaces the host pixel work of mmdet/datasets/pipelines/transforms.py Resize (:26-317, bilinear), RandomFlip (:319-470),
 * Normalize (:566-635) and Pad (:637-722), and the bottom / right batch padding of mmcv's collate (mmcv/parallel/collate.py), for one
 * batch in one launch.  src_pack: the batch's decoded BGR HWC uint8 images, packed; items_dev: B records (device memory, 8-B aligned);
 * dst: float32 NCHW [B, 3, Hp, Wp].  Pixels inside img_shape (oh, ow) are bit-identical to pipelines.imresize -> flip -> imnormalize;
 * pixels in [img_shape, pad_shape) get pad_val; pixels beyond pad_shape get 0.  sy / sx are np.float32(h / oh) and np.float32(w / ow)
 * exactly as pipelines._lin_coords computes them; flip: bit 0 horizontal, bit 1 vertical (3 = diagonal). */
typedef struct {
  int64_t src_off;       /* byte offset of this image in src_pack                            */
  int32_t h, w;          /* source size                                                       */
  int32_t oh, ow;        /* resized size (img_shape)                                          */
  int32_t ph, pw;        /* pad_shape                                                         */
  float sy, sx;          /* source / destination scale per axis                               */
  int32_t flip;          /* 0 none, 1 horizontal, 2 vertical, 3 diagonal                      */
  int32_t to_rgb;        /* output channel c reads BGR channel 2 - c                          */
  float pad_val;
  float mean[3], std[3]; /* per OUTPUT channel                                                */
  int32_t reserved;
} aod_image_xform_item_t;  /* 80 bytes */
int aod_image_xform(const void* src_pack, const aod_image_xform_item_t* items_dev, int B, int Hp, int Wp, float* dst, aod_stream_t stream);

/* ------------------------------------------------------------------ optimizer (K16)
 * torch.optim.SGD semantics (apis/train_Lambda.py:54,59-61): d = g*grad_scale + wd*p; buf = first ? d : mom*buf + d;
 * p -= lr*buf, over HOST arrays of device pointers (params/grads/momentum buffers, fp32) and element counts.
 * lr_dev (nullable): device fp32 scalar that overrides `lr` -- lets a launch captured in a HIP graph follow the LR schedule. */
int aod_sgd_multi(void* const* params, void* const* grads, void* const* moms, const int64_t* sizes, int ntensors,
                  float lr, const float* lr_dev, float momentum, float weight_decay, int first_step, float grad_scale,
                  aod_stream_t stream);
/* aod_sgd_multi with a device-resident clip coefficient (nullable; state + 1 of aod_grad_norm_multi): the effective gradient scale is
 * grad_scale * *coef_dev.  A negative coefficient is the skip sentinel: the launch leaves params and momentum buffers untouched.
 * coef_dev == NULL is aod_sgd_multi, bit for bit. */
int aod_sgd_multi_clipped(void* const* params, void* const* grads, void* const* moms, const int64_t* sizes, int ntensors,
                          float lr, const float* lr_dev, float momentum, float weight_decay, int first_step, float grad_scale,
                          const float* coef_dev, aod_stream_t stream);
/* Gradient-norm clipping (mmcv OptimizerHook.clip_grads -> torch.nn.utils.clip_grad_norm_, norm_type 2) without a host round trip:
 * total_norm = sqrt(sum over all tensors of (g * grad_scale)^2), coef = min(1, max_norm / (total_norm + 1e-6)).  One launch per <= 48
 * tensors writes per-block fp32 partial sums to partials_ws (ws_capacity floats; 96 * ntensors always suffices), one workgroup adds them in
 * a fixed order in double: no atomics, the result does not depend on scheduling.  state (device, 4 fp32, zeroed once by the caller):
 * {total_norm, coef, skipped_steps, reserved}.  A non-finite norm gives coef = NaN (the update is non-finite, as with
 * clip_grad_norm_(error_if_nonfinite=False)) or, with flags bit 0 (skip_nonfinite), coef = -1 (aod_sgd_multi_clipped skips the update) and
 * skipped_steps += 1.  The gradients themselves are not modified. */
int aod_grad_norm_multi(void* const* grads, const int64_t* sizes, int ntensors, float grad_scale, float max_norm, int flags,
                        float* partials_ws, int64_t ws_capacity, float* state, aod_stream_t stream);

/* ------------------------------------------------------------------ ensemble / MC-dropout mutual information (csrc/ensemble_mi.hip)
 * Replaces mmdet/apis/CalEnsembleUnc.py:164-180 (ComputeMI) and mmdet/apis/CalMCDropoutUnc.py:183-199 (ComputeMCDropoutMI): the Python loop
 * over levels x images of a dozen torch ops each, ending in .tolist().  maps[k * L + l] = device pointer of member k's classification map of
 * level l: dense fp32, B x n_per_level[l] elements, batch outermost (NCHW-contiguous and channels_last both qualify: the score is a sum over
 * all elements; the class structure enters through rows_l = n_per_level[l] / n_cls only).  2 <= K <= 32 members, 1 <= L <= 8 levels.
 *   out[b] = mean_l ( sum_e [ -avg ln avg + (1/K) sum_k p_k ln p_k ] / rows_l ),   p_k = sigmoid(x_k), avg = mean_k p_k,   0 ln 0 = 0
 * (the reference yields NaN for an image once one sigmoid underflows).  partials_ws: aod_ensemble_mi_partials_len(L, n_per_level, B) floats
 * (ws_capacity = what the caller holds; -2 when too small).  Two launches, no atomics; the sums have a fixed order that does not depend on B
 * or on an image's position in the batch: same bits on every launch, and for an image scored alone or inside a batch. */
size_t aod_ensemble_mi_partials_len(int L, const int64_t* n_per_level, int B);
int aod_ensemble_mi(const void* const* maps, int K, int L, const int64_t* n_per_level, int B, int n_cls, float* out, float* partials_ws,
                    int64_t ws_capacity, aod_stream_t stream);

/* ------------------------------------------------------------------ MC-dropout baseline: Dropout2d factors and their application (csrc/dropout.hip)
 * The stochastic forward of mmdet/apis/CalMCDropoutUnc.py:137-163: one Dropout2d(rate) behind every ReLU (utils/functions.py:492-505), i.e.
 * one factor per (image, site, channel), 0 or 1 / (1 - rate), for the whole plane.  The conv kernels are untouched: the factors of one
 * forward are written into a dense fp32 table [B][T] (T = sum of the sites' channel counts) by ONE launch, and every ReLU output on the
 * path is multiplied in place by its site's slice of its image's row.
 *   aod_dropout2d_masks: table[b][site_offsets[s] + c] = u > rate ? 1 / (1 - rate) : 0 with u = u01(word c & 3 of Philox4x32-10 at counter
 *     (c >> 2, s, sample, (uint32) image_ids[b]), key ((uint32) seed ^ 0x44524F50, seed >> 32)), u01(w) = ((w >> 8) + 1) * 2^-24 in (0, 1]:
 *     rate = 0 writes ones.  image_ids [B] int64 and site_offsets [n_sites] int32 (ascending, site s spans up to the next offset, the last
 *     one up to T) are DEVICE arrays; sample is a plain argument.  A factor depends on (seed, sample, image id, site, channel) only.
 *   aod_dropout2d_apply: NHWC rows [B * HW, width(C)] *= table_row0[(row / HW) * row_stride_T + c], in place.  x3 = 0: bf16 rows of C columns
 *     (C % 8 == 0), value = bf16_rne((float) x * f).  x3 = 1: X-layout rows of 2 * ceil32(C) columns; head + tail are re-formed in fp32,
 *     multiplied and split again; pad columns stay zero.
 *   aod_dropout2d_apply_multi: the same for 1..8 row segments of one buffer `x` in one launch (the tower outputs of one depth: one segment
 *     per pyramid level): segment s = rows seg_row0[s] .. + B * seg_hw[s], factors table[b * row_stride_T + seg_off[s] + c].  The three
 *     seg_* arrays are HOST arrays. */
int aod_dropout2d_masks(float* table, const int64_t* image_ids, int B, const int32_t* site_offsets, int n_sites, int T, float rate,
                        uint64_t seed, uint32_t sample, aod_stream_t stream);
int aod_dropout2d_apply(void* x, const float* table_row0, int64_t row_stride_T, int B, int HW, int C, int x3, aod_stream_t stream);
int aod_dropout2d_apply_multi(void* x, const float* table, int64_t row_stride_T, int B, int nseg, const int64_t* seg_row0,
                              const int32_t* seg_hw, const int32_t* seg_off, int C, int x3, aod_stream_t stream);

/* ------------------------------------------------------------------ Core-set acquisition: pooled pyramid descriptors and k-center greedy
 * (csrc/coreset.hip: the descriptor; csrc/kcenter.hip: the selection).  No reference call site: O. Sener, S. Savarese, "Active Learning
 * for Convolutional Neural Networks: A Core-Set Approach", ICLR 2018, Algorithm 1 (k-Center-Greedy); the semantics are fixed in DESIGN 3i.
 *   aod_pool_descriptor: the descriptor of image b = concatenation over the nseg pyramid levels of the global average of the neck output:
 *     out[b * out_stride + s * C + c] = mean over the seg_hw[s] rows of image b in segment s of channel c, fp32.  Segment s = rows
 *     seg_row0[s] .. + B * seg_hw[s] of the row buffer `base` (1..8 segments, HOST arrays).  x3 = 0: bf16 rows of C columns; x3 = 1:
 *     X-layout rows of 2 * ceil32(C) columns, value = head + tail formed in fp32, pad columns are never read.  C % 8 == 0.  fp32
 *     accumulation, one division by seg_hw[s]; the order of a sum depends on seg_hw[s] only -- not on B, on the image's position in the
 *     batch or on another segment: an image has the same descriptor bits alone and in any batch.  16-B loads, a fixed LDS tree, no atomics.
 *   aod_kcenter_greedy: desc [N][D] fp32 (1 <= D <= 2048, 16-B aligned), labelled [n_labelled] int64 DEVICE indices (distinct, in [0, N):
 *     the caller validates; an index outside the matrix is skipped, never dereferenced), 1 <= budget <= N - n_labelled.
 *       d(i, c) = sum_k (x_ik - x_ck)^2 in the direct difference form, fp32; a function of the two rows and D alone
 *       mind[i] = min over labelled c of d(i, c) (+inf for an empty labelled set); labelled rows are selected
 *       step t  : picks[t] = the unselected row with the largest mind, the LOWEST index on a tie; radius[t] = that mind; the pick becomes
 *                 selected; every mind[i] takes min(mind[i], d(i, pick)).  A selected row never wins, also when every mind is 0.
 *     picks [budget] int64, radius [budget] fp32, mind [N] fp32 (on return: the distance to the nearest labelled or picked row), ws:
 *     aod_kcenter_ws_len(N) bytes, 8-B aligned.  All budget steps are enqueued on `stream` (one launch per pick, which first reduces the
 *     per-workgroup partials of the launch before it); no host sync, no cross-workgroup wait inside a launch, no atomics, no trip count
 *     that depends on data.  NaN descriptors are the caller's error.  aod_kcenter_chunk(): labelled centers per initialisation launch. */
int aod_pool_descriptor(const void* base, int nseg, const int64_t* seg_row0, const int32_t* seg_hw, int C, int x3, int B, float* out,
                        int64_t out_stride, aod_stream_t stream);
int aod_kcenter_chunk(void);
size_t aod_kcenter_ws_len(int64_t N);
int aod_kcenter_greedy(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                       float* radius, float* mind, void* ws, aod_stream_t stream);

/* ------------------------------------------------------------------ CDAL acquisition: class-mixture descriptors and the symmetrised-KL
 * k-center metric (csrc/cdal.hip, csrc/kcenter.hip).  No reference call site: S. Agarwal, H. Arora, S. Anand, C. Arora, "Contextual
 * Diversity for Active Learning", ECCV 2020, in its core-set form (CDAL-CS); the semantics are fixed in DESIGN 3j.
 *   aod_cdal_descriptor: maps = L HOST-array device pointers (1..8 levels; they travel as kernel arguments), level l = fp32 [B][rows_l][C]
 *     logits, the C classes of an anchor row contiguous (rows_per_level: HOST array), 1 <= C <= 32 (2 C^2 <= 2048 descriptor columns).
 *     Per row: p = softmax(x) as exp(x - max) / sum; a region iff max p > score_thr (strict), its class the argmax (lowest index on a
 *     tie), its weight w = H(p) + 2^-10 (0 ln 0 = 0).  Per image and class c: M[c] = sum w p / sum w over the regions of class c (1 / C
 *     for a class without one), P[c] = (1 - 2^-10) M[c] + 2^-10 / C;  out[b * out_stride + ...] = [P (C * C) | ln P (C * C)].
 *     Two launches (per-chunk partial accumulators into ws, then one workgroup per image and class), no atomics, no host sync; expf / log1pf /
 *     logf.  The association of every sum depends on a row's index inside its own image only: an image has the same descriptor bits
 *     alone, at any position of any batch, eager or replayed.  16-B loads where an image's base is 16-B aligned.
 *     ws: aod_cdal_ws_len(L, rows_per_level, C, B) floats (0: bad shape), ws_capacity = the floats it holds; aod_cdal_chunk(): rows per
 *     partial accumulator.
 *   aod_kcenter_greedy_ex: aod_kcenter_greedy with a metric.  0: the squared Euclidean distance (the same arithmetic and bits as
 *     aod_kcenter_greedy, which forwards here).  1: a row is [P | ln P], two halves of D / 2 columns (D even, else refused):
 *       d(i, j) = 1/2 sum_k max((P_ik - P_jk)(ln P_ik - ln P_jk), 0), the symmetrised KL divergence summed over the classes;
 *     the lane ownership, the four running sums per lane and the butterfly of metric 0 over the D / 2 columns of a half: a function of
 *     the two rows and D alone.  Every term is non-negative, so the 64-bit keys order it as they order metric 0. */
int aod_cdal_chunk(void);
size_t aod_cdal_ws_len(int L, const int64_t* rows_per_level, int C, int B);
int aod_cdal_descriptor(const void* const* maps, int L, const int64_t* rows_per_level, int C, int B, float score_thr, float* out,
                        int64_t out_stride, float* ws, int64_t ws_capacity, aod_stream_t stream);
int aod_kcenter_greedy_ex(const float* desc, int64_t N, int D, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                          float* radius, float* mind, void* ws, aod_stream_t stream, int metric);

/* ------------------------------------------------------------------ Posterior uncertainty pools: entropy, margin, least confidence of the
 * detector's own class posterior per detection, aggregated per image (csrc/det_unc.hip).  No reference call site ("Entropy" in the paper's
 * tables; margin / least confidence and the max / mean / sum aggregates: Brust et al., VISAPP 2019; Roy et al., BMVC 2018); the semantics are
 * fixed in DESIGN 3l.
 *   aod_det_uncertainty: boxes [B][n][4], scores [B][n][W] = the candidates of aod_pre_nms_levels / aod_gather_decode; dets [B][max_num][5],
 *     labels [B][max_num] int64, num [B] = the outputs of aod_multiclass_nms.  1 <= max_num <= 1024, n >= 1, W >= 2.
 *     layout: the columns of a score row that form the posterior -- 0 (cat) the first W - 1 as one categorical distribution (the EDL-normalised
 *     scores; the last column is the zero pad), 1 (cat_bg) all W (SSD's softmax, background last), 2 (sigmoid) the first W - 1 as independent
 *     Bernoulli posteriors.  Row j of image b is an object iff j < num[b] and dets[b][j][4] > score_thr (strict; rows >= num[b] are never
 *     read).  Its score row is the candidate of lowest index whose four box words equal dets[b][j][0..3] and whose score at labels[b][j]
 *     equals dets[b][j][4], bit for bit (the NMS kernel copies both); an object without one (or with a label outside [0, W)) is skipped and
 *     counted in missing[b].
 *     measure: 0 entropy (-sum s ln s; layout 2: sum_c -s ln s - (1 - s) log1pf(-s); 0 ln 0 = 0), 1 margin 1 - (s_(1) - s_(2)) (two used
 *     columns at least, else refused), 2 least confidence 1 - s_(1).  aggregate over the image's objects: 0 max, 1 mean, 2 sum; an image
 *     without an object scores 0.  unc [B]; obj_out [B][max_num] (nullable): the measure per detection row, NaN where the row is no object
 *     (or is missing); missing [B] int32 (nullable).
 *     One launch, one workgroup per image, no atomics, no workspace, no host sync; logf / log1pf.  The classes of a row are added in column
 *     order and the objects in a pairwise tree over the next power of two >= max_num: a function of j and max_num alone, so an image has the
 *     same score bits alone, at any position of any batch, eager or replayed. */
int aod_det_uncertainty(const float* boxes, const float* scores, const float* dets, const int64_t* labels, const int32_t* num, int B, int n,
                        int W, int max_num, int layout, int measure, int aggregate, float score_thr, float* unc, float* obj_out,
                        int32_t* missing, aod_stream_t stream);

/* ------------------------------------------------------------------ Localization-stability acquisition (csrc/loc_stability.hip): detect on
 * the clean image and on copies with Gaussian pixel noise of growing strength, score the image by how far its boxes move (Kao, Lee, Sen,
 * Liu, "Localization-Aware Active Learning for Object Detection", ACCV 2018: LS and LS+C).  No reference call site; the semantics are fixed
 * in DESIGN 3m.
 *   aod_pixel_noise: src, dst fp32 [B][C][Hp][Wp] (normalised, padded model input), out of place (dst == src or overlapping: refused),
 *     16-B aligned; C <= 4, Hp <= 65536, Wp <= 262144, Wp % 4 == 0.  hw [B][2] int32 (device): img_shape (h, w) per image; inv_std: C HOST
 *     floats, 1 / std_c of the normalisation in the tensor's channel order; sigma >= 0, finite, in 0..255 pixel units; 0 <= level < 16.
 *     dst[b][c][y][x] = src + (sigma * inv_std[c]) * z for y < h and x < w, src's bits elsewhere (and everywhere for sigma == 0); no
 *     clipping.  z = element x & 3 of the four normals (u01, two Box-Muller pairs: ra cos, ra sin, rb cos, rb sin -- the quad of
 *     aod_synth_normal_images) of the Philox4x32-10 block with counter (c0, c1, c2, c3) = ((y << 16) | (x >> 2), 0x80000000 | (level << 8) | c,
 *     id & 0xffffffff, id >> 32), id = image_ids[b] (device int64), key (seed & 0xffffffff, seed >> 32).  Bit 31 of c1 keeps the stream
 *     disjoint from the synthetic pool's.  z is a function of (seed, level, id, c, y, x) alone -- not of B, the batch position or Wp.
 *     One thread per 4 consecutive x (a 16-B load and a 16-B store).
 *   aod_loc_stability: the stacked slots dets [K+1][B][max_num][5], labels [K+1][B][max_num] int64,
 *     num [K+1][B]: slot 0 the clean detections, slot k + 1 those of noise level k; 1 <= K <= 16, 1 <= max_num <= 1024.  Reference row j of
 *     slot 0 is an object iff j < num[0][b] and dets[0][b][j][4] > score_thr (strict); w_j is that score.  m_jk = the largest IoU of box j
 *     over the rows < num[k+1][b] of slot k + 1 (same_class = 1: rows with j's label only), 0 for an empty slot;
 *       iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih likewise, ov = iw * ih, un = area_a + area_b - ov, IoU = ov / max(un, 1e-6)
 *     in fp32 with an IEEE division (aod_eval_match's form, no +1).  S_j = (m_j0 + ... + m_j,K-1) / K, added in level order;
 *     S_I = sum_j w_j S_j / sum_j w_j over the objects.  combine 0 (ls): unc[b] = 1 - S_I; 1 (ls+c): (1 - S_I) + (1 - max_j w_j); an image
 *     without an object scores 0.  stab_out [B][max_num] (nullable): S_j, NaN where the row is no object.  Rows >= num of any slot are never
 *     read.
 *     One launch, one workgroup per image, no atomics, no workspace, no host sync.  The sums over j run in a pairwise tree over the next
 *     power of two >= max_num: a function of j and max_num alone, so an image has the same score bits alone, at any position of any batch,
 *     eager or replayed. */
int aod_loc_stability_max_levels(void); /* 16: the largest K of aod_loc_stability, levels 0 .. 15 of aod_pixel_noise */
int aod_pixel_noise(const float* src, float* dst, int B, int C, int Hp, int Wp, const int32_t* hw, const float* inv_std, float sigma, int level,
                    uint64_t seed, const int64_t* image_ids, aod_stream_t stream);
int aod_loc_stability(const float* dets, const int64_t* labels, const int32_t* num, int K, int B, int max_num, float score_thr, int same_class,
                      int combine, float* unc, float* stab_out, aod_stream_t stream);

/* ------------------------------------------------------------------ CCMS acquisition (csrc/ccms.hip, csrc/kcenter.hip, csrc/det_unc.hip):
 * pre-select the most uncertain images, then spread the picks by k-center greedy under a distance that matches objects of the same class
 * between two images (PPAL: Yang, Huang, Crowley, "Plug and Play Active Learning for Object Detection", CVPR 2024; its class-difficulty
 * EMA: the next section).  No reference call site; the semantics are fixed in DESIGN 3o.
 *   aod_det_uncertainty_ex: aod_det_uncertainty (the same arithmetic and bits; it forwards here) with obj_cand [B][max_num] int32
 *     (nullable): the candidate row matched to detection row j, -1 where the row is no object or has no candidate.
 *   aod_object_descriptors: the objects of image b are its detection rows j < num[b] with dets[b][j][4] > score_thr (strict), in row
 *     order, the first max_obj of them (1 <= max_obj <= 64).  Object row j has class labels[b][j], weight dets[b][j][4], candidate row
 *     k = obj_cand[b][j], global anchor g = cand_anchor[b][k] (cand_anchor [B][n] int32), level l with anchor0_l <= g < anchor0_{l+1}
 *     (anchor0_{l+1} = anchor0_l + seg_hw[l] * seg_na[l]) and cell (g - anchor0_l) / seg_na[l].  Its raw feature v is row
 *     b * seg_hw[l] + cell of the level's neck output seg_base[l] (nseg <= 8 HOST pointers to DEVICE rows, 16-B aligned): C bf16 columns
 *     (x3 = 0) or X-layout rows of 2 * ceil32(C) columns, value = head + tail (x3 = 1); C % 8 == 0, C <= 1024; 16-B loads; pad columns
 *     and rows outside the levels are never read.  f = v / sqrt(sum_k v_k^2) (IEEE sqrt and division), all zeros when the sum is 0.  An
 *     object with obj_cand outside [0, n), a label outside int32 or an anchor outside every level is skipped -- it takes no slot -- and
 *     counted in missing[b] (all such rows of the image, beyond the max_obj cut too; expected 0).  1 <= max_num <= 1024.
 *     Outputs: feat [B][max_obj][C] fp32 (16-B aligned), cls [B][max_obj] int32, w [B][max_obj] fp32, cnt [B], missing [B] int32; slots
 *     >= cnt[b] hold (zeros, -1, 0).  One launch, one workgroup per image, no atomics, no host sync.  The sum of squares runs per lane in
 *     element order, then an xor butterfly: a function of the row alone, so an image has the same bits alone and inside any batch.
 *   aod_ccms_distance: feat [M][max_obj][C] fp32 (16-B aligned), cls, w [M][max_obj], cnt [M] as above (rows >= cnt[a] are never used);
 *     1 <= M <= aod_ccms_max_images() = 32768, 1 <= max_obj <= 64 (an image is one or two blocks of 32 objects), C % 8 == 0, C <= 256 (four
 *     blocks of 32 x C fp32 stay resident in the 160 KB LDS).  dist [M][M] fp32:
 *       m_i = max(0, max_{j in b, c_j = c_i} <f_i, f_j>) (0 if b has no object of that class), S(a->b) = sum_i w_i m_i / sum_i w_i
 *       (0 if a has no object), d(a, b) = max(0, 1 - (S(a->b) + S(b->a)) / 2) for a != b, d(a, a) = 0.
 *     All arithmetic fp32; the sums over i run in row order (separate multiply and add).  Every dot product is a k-ordered fmaf chain on
 *     v_mfma_f32_32x32x2_f32 with the channels in the order 0 4 1 5 2 6 3 7 8 12 ... (C padded with zeros to 64 / 128 / 256): a function of
 *     k alone.  No atomics.  An entry is a function of the two images alone -- not of M, its position or the tiling -- and dist[a][b] and
 *     dist[b][a] hold the same bits.  NaN features are the caller's error.
 *   aod_kcenter_greedy_matrix: aod_kcenter_greedy's selection (the same prepare / mark / keys / one-launch-per-pick scheme, tie rule, picks /
 *     radius / mind outputs and aod_kcenter_ws_len(N) workspace) on a precomputed dist [N][N] fp32 with non-negative entries: the sweeps read
 *     dist[p][i] of center p.  With n_labelled == 0 the first pick is row 0 with radius +inf. */
int aod_det_uncertainty_ex(const float* boxes, const float* scores, const float* dets, const int64_t* labels, const int32_t* num, int B, int n,
                           int W, int max_num, int layout, int measure, int aggregate, float score_thr, float* unc, float* obj_out,
                           int32_t* missing, int32_t* obj_cand, aod_stream_t stream);
int aod_object_descriptors(const void* const* seg_base, int nseg, const int32_t* seg_hw, const int32_t* seg_na, int C, int x3, int B,
                           const int32_t* cand_anchor, int n, const float* dets, const int64_t* labels, const int32_t* num,
                           const int32_t* obj_cand, int max_num, int max_obj, float score_thr, float* feat, int32_t* cls, float* w, int32_t* cnt,
                           int32_t* missing, aod_stream_t stream);
int aod_ccms_max_images(void);
int aod_ccms_distance(const float* feat, const int32_t* cls, const float* w, const int32_t* cnt, int M, int max_obj, int C, float* dist,
                      aod_stream_t stream);
int aod_kcenter_greedy_matrix(const float* dist, int64_t N, const int64_t* labelled, int64_t n_labelled, int64_t budget, int64_t* picks,
                              float* radius, float* mind, void* ws, aod_stream_t stream);

/* ------------------------------------------------------------------ class difficulty (csrc/difficulty.hip, csrc/det_unc.hip): the
 * training-side half of PPAL's Difficulty-Calibrated Uncertainty Sampling (Yang, Huang, Crowley, CVPR 2024).  No reference call site; the
 * semantics are fixed in DESIGN 3p.
 *   aod_class_difficulty_accum: over the loss operands of aod_*_focal_l1_*_fwd -- cls [nrows][C] fp32 logits, labels [nrows] int64,
 *     label_w [nrows], bbox_pred / bbox_tgt [nrows][4] fp32 deltas (16-B aligned) -- a positive is a row r with 0 <= labels[r] < C and
 *     label_w[r] > 0; cls / bbox_pred / bbox_tgt of every other row are never read (they may hold NaN).  With c = labels[r]:
 *       P    form 0: softmax(cls[r])[c], the maximum subtracted;  form 1: 1 / (1 + exp(-cls[r][c]))
 *       IoU  of the boxes (centre (t0, t1), size (exp(clamp(t2)), exp(clamp(t3)))), t = delta * stds4 + means4 (HOST float[4] each), clamp
 *            to +-|ln(wh_ratio_clip)|, for delta = bbox_pred[r] and bbox_tgt[r]:  ov / max(un, 1e-6) as in aod_loc_stability.  Both boxes
 *            are decoded from the same anchor and IoU is unchanged by translation and per-axis scaling: no anchor is read.
 *       q    1 - powf(P, xi) * powf(IoU, 1 - xi), 1 when P or IoU is 0, clamped to [0, 1];  0 <= xi <= 1
 *     acc [2C] fp32: acc[c] += sum of q, acc[C + c] += count over the call's positives of class c (the count is an fp32 integer).  Several
 *     calls add up (one per pyramid level; a rank may all-reduce acc before the update).  ws: aod_class_difficulty_ws_len(nrows, C) floats.
 *     1 <= C <= 128; nrows == 0 is a no-op.  Two launches (block partials; one block adds them in block order), no atomics; every sum's
 *     order depends on nrows and the row indices alone: the same inputs give the same bits on every run, eager or replayed.
 *   aod_class_difficulty_update: for c < C with acc[C + c] > 0: d[c] = momentum * d[c] + (1 - momentum) * (acc[c] / acc[C + c]); any other
 *     d[c] keeps its bits.  acc is zeroed.  0 <= momentum <= 1.  One launch.
 *   aod_det_uncertainty_w: aod_det_uncertainty_ex with class_w [W] fp32 (nullable): the measure of an object row with label l is multiplied
 *     by class_w[l] (one fp32 multiply) before it is written to obj_out and enters the aggregate.  NULL: aod_det_uncertainty_ex's bits (it
 *     forwards here). */
size_t aod_class_difficulty_ws_len(int64_t nrows, int C);
int aod_class_difficulty_accum(const float* cls, const int64_t* labels, const float* label_w, const float* bbox_pred, const float* bbox_tgt,
                               int64_t nrows, int C, int form, const float* means4, const float* stds4, float wh_ratio_clip, float xi, float* acc,
                               float* ws, aod_stream_t stream);
int aod_class_difficulty_update(float* acc, float* d, int C, float momentum, aod_stream_t stream);
int aod_det_uncertainty_w(const float* boxes, const float* scores, const float* dets, const int64_t* labels, const int32_t* num, int B, int n,
                          int W, int max_num, int layout, int measure, int aggregate, float score_thr, float* unc, float* obj_out,
                          int32_t* missing, int32_t* obj_cand, const float* class_w, aod_stream_t stream);

/* ------------------------------------------------------------------ Consistency acquisition (csrc/consistency.hip): detect on the image and
 * on mirrored copies, map the boxes back, score the image by how much the detection lists disagree in box position and in class posterior
 * (Elezi, Yu, Anandkumar, Leal-Taixe, Alvarez, "Not All Labels Are Equal: Rationalizing the Labeling Costs for Training Object Detection",
 * CVPR 2022; CALD: Yu, Zhu, Yang, Chen, "Consistency-based Active Learning for Object Detection", CVPR Workshops 2022).  No reference call
 * site; the semantics are fixed in DESIGN 3q.  Flip codes: bit 0 horizontal, bit 1 vertical (1 hflip, 2 vflip, 3 hvflip).
 *   aod_flip_images: src, dst fp32 [B][C][Hp][Wp] (the padded model input), out of place (dst == src or overlapping: refused); any Wp >= 1.
 *     hw [B][2] int32 (device): img_shape (h, w) per image, clamped to Hp / Wp.  dst[b][c][y][x] = src[b][c][fy ? h-1-y : y][fx ? w-1-x : x]
 *     for y < h and x < w, src's bits elsewhere (the pad stays where the collate put it): a bit copy, nothing is computed.  16-B stores when
 *     Wp % 4 == 0 and both buffers are 16-B aligned, one element per thread otherwise; the same bits either way.  flip in {1, 2, 3}.
 *   aod_det_posterior: scores [B][n][W] (the candidates' score rows), obj_cand [B][max_num] int32 (aod_det_uncertainty_ex's, called with
 *     score_thr = -inf so that every row j < num[b] is looked up), num [B].  post [B][max_num][W]: post[b][j][:] = scores[b][obj_cand[b][j]][:]
 *     for j < num[b] with a candidate row (0 <= obj_cand < n), zero rows elsewhere -- every word of post is written; missing [B] (nullable):
 *     the rows j < num[b] without one.
 *   aod_det_consistency: the stacked slots dets [V+1][B][max_num][5], labels [V+1][B][max_num] int64, num [V+1][B], post [V+1][B][max_num][W]:
 *     slot 0 the clean detections, slot v + 1 those of view v; flips: V HOST codes; ext [B][2] fp32 (device): the extent (w, h) of the frame
 *     the boxes lie in (rescaled detections: (w / scale_x, h / scale_y)).  1 <= V <= 3, 1 <= max_num <= 1024, W >= 2.
 *     Row j of slot 0 is an object iff j < num[0][b] and dets[0][b][j][4] > score_thr (strict).  A view box is un-flipped first:
 *     horizontal x1' = ext_w - x2, x2' = ext_w - x1, vertical likewise with ext_h (one fp32 subtraction each); scores and labels unchanged.
 *     match_jv = argmax of the IoU over the un-flipped rows i < num[v+1][b] (same_class = 1: rows with j's label only), lowest index on a tie,
 *       iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih likewise, ov = iw * ih, un = area_a + area_b - ov, IoU = ov / max(un, 1e-6)
 *     (aod_loc_stability's form).  No such row, or a best IoU of 0: match -1, iou_jv = 0, js_jv = 1.  Otherwise, with p = post[0][b][j] and
 *     q = post[v+1][b][match], t(a, b) = [a > 0] a (ln a - ln m) + [b > 0] b (ln b - ln m), m = (a + b) / 2 (>= 0; exactly 0 for equal bits; a
 *     term whose m rounds to 0 -- a + b = 2^-149 -- is taken as 0):
 *       layout 0 (cat: the first W - 1 columns) / 1 (cat_bg: all W): js = (sum_c t(p_c, q_c) / 2) / ln 2, the columns added in order;
 *       layout 2 (sigmoid: the first W - 1 columns, independent Bernoulli): js = (sum_c (t(p_c, q_c) + t(1 - p_c, 1 - q_c)) / 2 / used) / ln 2.
 *     mode 0 (box): u_jv = 1 - iou_jv; 1 (cls): js_jv; 2 (both): ((1 - iou_jv) + js_jv) / 2.  u_j = (u_j0 + ... + u_j,V-1) / V, the views
 *     added in order.  aggregate 0 / 1 / 2: unc[b] = max / mean / sum of u_j over the objects; an image without one scores 0.
 *     Nullable outputs: obj_out [B][max_num] (u_j), iou_out / js_out [V][B][max_num]: NaN where the row is no object; match_out
 *     [V][B][max_num] int32: -1 where unmatched or no object.  Rows >= num of any slot are never read.
 *     One launch, one workgroup per image, no atomics, no workspace, no host sync.  The aggregate runs in a pairwise tree over the next power
 *     of two >= max_num (rows that are no object hold 0): a function of j and max_num alone, so an image has the same score bits alone, at
 *     any position of any batch, eager or replayed. */
int aod_consistency_max_views(void); /* 3: the largest V of aod_det_consistency */
int aod_flip_images(const float* src, float* dst, int B, int C, int Hp, int Wp, const int32_t* hw, int flip, aod_stream_t stream);
int aod_det_posterior(const float* scores, const int32_t* obj_cand, const int32_t* num, int B, int n, int W, int max_num, float* post,
                      int32_t* missing, aod_stream_t stream);
int aod_det_consistency(const float* dets, const int64_t* labels, const int32_t* num, const float* post, int V, const int32_t* flips,
                        const float* ext, int B, int max_num, int W, int layout, int mode, int aggregate, float score_thr, int same_class,
                        float* unc, float* obj_out, float* iou_out, float* js_out, int32_t* match_out, aod_stream_t stream);

/* ------------------------------------------------------------------ ENMS + DivProto acquisition (csrc/divproto.hip): entropy summed over
 * the objects that survive a feature-similarity NMS, then a progressive pick that rejects images whose class prototypes repeat the picks so
 * far and favours the classes the picks hold least (Wu, Chen, Huang, "Entropy-based Active Learning for Object Detection with Progressive
 * Diversity Constraint", CVPR 2022).  No reference call site; the semantics are fixed in DESIGN 3s.
 * <a, b> is one fp32 product form everywhere: 16 lanes per product, lane q owns the channels 4q + 64m (+0..3) in ascending m, four running
 * sums (separate multiply and add), ((s0 + s1) + (s2 + s3)), an xor butterfly over the 16 lanes: bit-symmetric, a function of the two rows
 * and C alone.
 *   aod_object_measure: h [B][max_obj] fp32, slot-aligned with aod_object_descriptors' feat / cls / w: obj_out [B][max_num] (the per-object
 *     measure of aod_det_uncertainty*) at the detection rows j < num[b] with dets[b][j][4] > score_thr (strict) -- a row whose
 *     obj_cand[b][j] < 0 (nullable; expected never) takes no slot --, the first max_obj in row order; 0 behind them.
 *   aod_enms_prototypes: feat [B][max_obj][C] fp32 (16-B aligned), cls, w, h [B][max_obj], cnt [B] (rows >= cnt[b] are never read);
 *     1 <= max_obj <= 64, C % 8 == 0, 8 <= C <= 256.  One workgroup per image, rows resident in LDS.
 *       ENMS: all objects alive; repeat: k* = the alive object with the largest h (lowest index on a tie), E += h_k* (fp32, pick order),
 *         k* and every alive j with cls_j == cls_k* and <f_j, f_k*> > t_enms (strict) die.  enms [B] = E, kept [B] = picks,
 *         pick [B][max_obj] int32 (nullable) = the picked slots in pick order, -1 behind them.
 *       prototypes: for every class among ALL the image's objects, ascending: v = sum over its objects in ascending k of
 *         (h_k + 2^-10) * f_k, p = v / sqrt(sum v^2) (zeros when the sum is 0), conf = max w_k.  proto [B][max_obj][C] (16-B aligned),
 *         pcls [B][max_obj] (-1 pad), pconf [B][max_obj] (0 pad), pcnt [B].
 *       A threshold >= 1 switches its check off (t_enms: nothing is suppressed; t_intra below: no image is redundant): a cosine cannot
 *       exceed 1, the rounded product of a unit row with itself can.
 *     An image's outputs are a function of its rows alone: the same bits alone, in any batch, eager or replayed.
 *   aod_divproto_select: the progressive pick over order [M] int64 (DEVICE; distinct indices into the pool tensors proto [N][max_obj][C],
 *     pcls, pconf [N][max_obj], pcnt [N], in sweep order).  State: S empty, n_c = 0, free_used = 0.  Per position, until `budget` images
 *     are accepted:  m = min over the image's classes c of (max over the entries of c's list of <p_I,c, p_J,c>; 0 for an empty list);
 *     m > t_intra (strict) and at least one class: redundant.  Otherwise, class_balance != 0: class c is minor iff fewer than n_minor
 *     classes c' have n_c' < n_c or (n_c' == n_c and c' < c); the image serves iff it has a minor class with conf > t_inter and
 *     n_c < quota: accepted (stage 1); else free_used < n_free: accepted (stage 2), ++free_used; else deferred.  class_balance == 0:
 *     accepted (stage 1).  Accept: picks [t] = image, every class joins its list, ++n_c for the classes with conf > t_inter.  A sweep
 *     that ends short is filled with the deferred positions in sweep order, then the redundant ones (stage 3).  picks [budget] int64,
 *     stage [budget] int32.  A slot whose class lies outside [0, n_cls) is ignored.  1 <= n_cls <= 128, 1 <= budget <= M <= 2^31 - 1,
 *     1 <= n_minor <= n_cls, 1 <= quota <= budget, 0 <= n_free <= budget.  ws: aod_divproto_ws_len(M, n_cls, budget) bytes, 8-B
 *     aligned.  An init launch, ceil(M / chunk) launches of ONE workgroup (chunk = 0: aod_divproto_chunk() = 64 positions; a launch
 *     that finds the budget met exits at once), one fill launch; all state in ws, so the result does not depend on chunk.  No atomics,
 *     no cross-workgroup wait, no host sync. */
int aod_object_measure(const float* obj_out, const float* dets, const int32_t* num, const int32_t* obj_cand, int B, int max_num, int max_obj,
                       float score_thr, float* h, aod_stream_t stream);
int aod_enms_prototypes(const float* feat, const int32_t* cls, const float* w, const float* h, const int32_t* cnt, int B, int max_obj, int C,
                        float t_enms, float* enms, int32_t* kept, float* proto, int32_t* pcls, float* pconf, int32_t* pcnt, int32_t* pick,
                        aod_stream_t stream);
int aod_divproto_chunk(void);
size_t aod_divproto_ws_len(int64_t M, int n_cls, int64_t budget);
int aod_divproto_select(const int64_t* order, int64_t M, int64_t N, const float* proto, const int32_t* pcls, const float* pconf,
                        const int32_t* pcnt, int max_obj, int C, int n_cls, int64_t budget, float t_intra, float t_inter, int n_minor,
                        int64_t quota, int64_t n_free, int class_balance, int chunk, int64_t* picks, int32_t* stage, void* ws,
                        aod_stream_t stream);

/* ------------------------------------------------------------------ BADGE acquisition (csrc/badge.hip, csrc/kmeanspp.hip): gradient
 * embeddings whose length carries an image's uncertainty and whose direction its content, then k-means++ D^2 seeding on them (J. T. Ash,
 * C. Zhang, A. Krishnamurthy, J. Langford, A. Agarwal, "Deep Batch Active Learning by Diverse, Uncertain Gradient Lower Bounds", ICLR 2020;
 * the seeding: D. Arthur, S. Vassilvitskii, "k-means++: The Advantages of Careful Seeding", SODA 2007).  No reference call site; the
 * semantics are fixed in DESIGN 3t.
 *   aod_object_posterior: post [B][max_obj][W] fp32, slot-aligned with aod_object_descriptors' feat / cls: scores [B][n][W] (the candidate
 *     score rows) at row obj_cand[b][j] of the detection rows j < num[b] with dets[b][j][4] > score_thr (strict) and 0 <= obj_cand[b][j] < n
 *     (aod_object_measure's slot rule), the first max_obj in row order; zero rows behind them: every word is written.
 *   aod_badge_embedding: out[b * out_stride + c * Cf + j] = sum over the objects o < cnt[b] in ascending order of a_o[c] * f_o[j], fp32, a
 *     separate multiply and add per object; a_o[c] = post[b][o][c] - [c == cls[b][o]], c < n_cls <= W (the gradient of the cross-entropy with
 *     respect to the logits under the detection's own label), f_o = feat[b][o][:].  feat [B][K][Cf] (16-B aligned), post [B][K][W],
 *     cls [B][K], cnt [B]; K <= 64, Cf % 8 == 0, 8 <= Cf <= 256, n_cls <= 128; out 16-B aligned, out_stride % 4 == 0 and >= n_cls * Cf.
 *     Columns >= n_cls of post and rows >= cnt[b] are never read; cnt[b] = 0 writes the zero row.  One workgroup per image, no atomics: a
 *     row is a function of its image alone -- the same bits alone, in any batch, eager or replayed.
 *   aod_kmeanspp_seed: desc [N][D] fp32 (1 <= N <= 2^24, 1 <= D <= 32768, 16-B aligned), excluded [n_excluded] int64 DEVICE indices
 *     (distinct, in [0, N): the caller validates; an index outside the matrix is skipped, never dereferenced), 1 <= budget <=
 *     N - n_excluded, draws [budget] fp64 DEVICE values in [0, 1) (draws[0] is not read).  A row is eligible iff it is neither excluded nor
 *     picked; excluded rows are NOT centres.
 *       d(i, c)  = sum_k (x_ik - x_ck)^2 in aod_kcenter_greedy's arithmetic, continued past column 2048: the same bits for D <= 2048
 *       pick 0   : the eligible row with the largest |x_i|^2 = d(i, 0), the LOWEST index on a tie; weight[0] = that norm, total[0] = 0
 *       pick t   : w_i = min over the picks so far of d(i, pick) for an eligible row, else 0.  S_b = the fp64 sum of w_i over block b of
 *                  aod_kmeanspp_block() consecutive rows in row order, T = S_0 + S_1 + ... in block order.  T == 0: the lowest eligible
 *                  row.  Else target = draws[t] * T (one fp64 product) and the pick is the first row with w_i > 0 whose running sum -- the
 *                  blocks before it in order, then the rows of its block in order, fp64 -- exceeds target (strict); no such row (the
 *                  product rounded up to T): the last row with w_i > 0.  weight[t] = w_pick, total[t] = T.
 *     picks [budget] int64, weight [budget] fp32, total [budget] fp64, mind [N] fp32 (on return: the distance to the nearest picked row),
 *     ws: aod_kmeanspp_ws_len(N) bytes (0: N outside 1 .. 2^24), 8-B aligned.  All steps are enqueued on `stream`, one launch per pick, which
 *     first finds the pick from the per-block partials of the launch before it (every workgroup redundantly, in one fixed association that
 *     depends on N and aod_kmeanspp_block() alone); no host sync, no cross-workgroup wait inside a launch, no atomics, no trip count that
 *     depends on data.  NaN descriptors are the caller's error. */
int aod_object_posterior(const float* scores, const float* dets, const int32_t* num, const int32_t* obj_cand, int B, int n, int W, int max_num,
                         int max_obj, float score_thr, float* post, aod_stream_t stream);
int aod_badge_embedding(const float* feat, const float* post, const int32_t* cls, const int32_t* cnt, int B, int K, int Cf, int W, int n_cls,
                        float* out, int64_t out_stride, aod_stream_t stream);
int aod_kmeanspp_block(void);
size_t aod_kmeanspp_ws_len(int64_t N);
int aod_kmeanspp_seed(const float* desc, int64_t N, int D, const int64_t* excluded, int64_t n_excluded, int64_t budget, const double* draws,
                      int64_t* picks, float* weight, double* total, float* mind, void* ws, aod_stream_t stream);

/* ------------------------------------------------------------------ reference-precision mode (aod_conv_desc_t.x3): row kernels on
 * X-layout tensors (csrc/x3_ops.hip).  The reference computes every one of these in fp32 (README.md:13-25); here a value is the fp32 sum of
 * its bf16 head and tail and is written back as such a pair.  `C` = PHYSICAL width (bf16 columns, multiple of 64) unless stated. */
/* fp32 [M][C logical] <-> X rows [M][2*ceil32(C)] (pad channels zero) */
int aod_x3_split(const float* src, void* dst, int64_t M, int C, aod_stream_t stream);
int aod_x3_merge(const void* src, float* dst, int64_t M, int C, aod_stream_t stream);
/* out = a + b over n bf16 elements of X rows: autograd's gradient accumulation where a tensor feeds several consumers (fpn.py:163-202,
 * Lambda_L2.py:85-94) */
int aod_x3_add(const void* a, const void* b, void* out, int64_t n, aod_stream_t stream);
/* aod_nchw_f32_to_s2d_bf16 with X rows of 64 columns (the 16 slots as one 32-channel band) */
int aod_x3_nchw_f32_to_s2d(const float* src, void* dst, int B, int C, int H, int W, aod_stream_t stream);
/* aod_maxpool3x3s2 / aod_upsample2x_add_to / aod_upsample2x_add_bwd_set on X rows */
int aod_x3_maxpool3x3s2(const void* src, void* dst, int B, int H, int W, int C, aod_stream_t stream);
int aod_x3_upsample2x_add_to(const void* top, const void* lateral, void* out, int B, int h, int w, int C, int H, int W, aod_stream_t stream);
int aod_x3_upsample2x_add_bwd_set(const void* g_dst, void* g_src, int B, int h, int w, int C, int H, int W, aod_stream_t stream);
/* dz = g * [a > 0] (relu != 0; dz may be NULL), colsum[c] += sum_m of it over the C/2 logical channels (aod_act_bwd's masked-gradient part) */
int aod_x3_act_bwd(const void* g, const void* a, void* dz, float* colsum, int64_t M, int C, int relu, aod_stream_t stream);
/* aod_pad_cast_colsum: fp32 head gradients [M][N] (* [relu_out > 0]) -> X rows of 2*ceil32(N) columns + column sums fp32 [ceil32(N)] */
int aod_x3_pad_cast_colsum(const float* g, const float* relu_out_f32, void* dz, float* colsum, int64_t M, int N, aod_stream_t stream);
/* ... and the row-activity map of dz ((M + 63) / 64 bytes, see aod_conv2d_ws_map): a block is 1 when any of its values fails v == 0 (NaN counts,
 * -0 does not).  dz and the column sums are those of the call without a map.  map NULL: aod_x3_pad_cast_colsum. */
int aod_x3_pad_cast_colsum_map(const float* g, const float* relu_out_f32, void* dz, float* colsum, int64_t M, int N, void* map,
                               aod_stream_t stream);

/* aod_bottleneck64_fwd on X rows (reference-precision mode; csrc/bottleneck_x3.hip): x [B*H*W][2*Cin], w1 / w2 / w3 = the X filter images of
 * aod_param_prep (flags bit 0), res / y [B*H*W][512]; Cin = LOGICAL input channels (64 or 256). */
int aod_bottleneck64x3_fwd(const void* x, int Cin, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                           const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, const void* res, void* y,
                           aod_stream_t stream);

/* ... for the stage's FIRST block (Cin = 64; resnet.py:291-292): the residual is bn_d(conv_d_1x1(x)), computed inside the launch from wd = the X
 * filter image [256][128] of the downsample conv and its folded BN -- the bits a separate aod_conv2d launch would have stored and this one read back. */
int aod_bottleneck64x3_ds_fwd(const void* x, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                              const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, const void* wd,
                              const float* sd, const float* bd, void* y, aod_stream_t stream);

/* aod_bottleneck128_fwd on X rows (reference-precision mode; csrc/bottleneck128_x3.hip): the IDENTITY bottleneck of the 128-plane stage
 * (mmdet/models/backbones/resnet.py:262-301, layer2: 512 -> 128 -> 128 -> 512) in one launch.  x / y [B*H*W][1024], w1 [128][1024], w2
 * [128][9][256], w3 [512][256] = the X filter images of aod_param_prep (flags bit 0), s / b the folded BN vectors; t1 / t2 [B*H*W][256]
 * (both or neither; NULL: inference / frozen) receive the block's two intermediates -- the launch is then the forward of a training step, the
 * three convs being recorded as autograd nodes around its outputs.  Same bits as the three aod_conv2d launches it replaces.  y must not alias x. */
int aod_bottleneck128x3_fwd(const void* x, int B, int H, int W, const void* w1, const float* s1, const float* b1, const void* w2,
                            const float* s2, const float* b2, const void* w3, const float* s3, const float* b3, void* y, void* t1, void* t2,
                            aod_stream_t stream);

/* aod_bottleneck_bwd (planes = 128) on X rows: the DGRAD chain of the same block in one launch -- the three x3 dgrad launches of conv3, conv2,
 * conv1 with their fused epilogues (mask / res / colsum) back to back, the two intermediate gradients staying in LDS:
 *   gt2 = [act_t2 > 0] * conv3_T(g)        gt1 = [act_t1 > 0] * conv2_T(gt2)        gx = [act_x > 0] * (conv1_T(gt1) + g)
 * g / act_x / gx [B*H*W][1024], act_t2 / act_t1 / gt2 / gt1 [B*H*W][256] X rows; wd3 [128][1024], wd2 [128][3][3][256], wd1 [512][256]: the X dgrad
 * images of aod_param_prep (BN scale folded in before the split); colsum_*: fp32 [128] [128] [512], += column sums of the three results (atomics:
 * the launch stands aside in the deterministic mode).  Gradients equal those of the three launches bit for bit.  gx must not alias g. */
int aod_bottleneck128x3_bwd(const void* g, int B, int H, int W, const void* wd3, const void* wd2, const void* wd1, const void* act_t2,
                            const void* act_t1, const void* act_x, void* gx, void* gt2, void* gt1, float* colsum_t2, float* colsum_t1,
                            float* colsum_x, aod_stream_t stream);

/* The narrow prediction convs in the reference-precision mode (Lambda_L2.py:52-54,100-103: retina_reg 256 -> 36, retina_L 256 -> 9 over the five
 * pyramid levels; csrc/halo_x3.hip): x3 forward 3x3 / stride 1 / pad 1, fp32 destination of at most 48 channels, X-layout source rows and X
 * filter image [N][3][3][C].  A K-step is a whole 32-channel chunk (halo + the nine taps' filter slices resident in LDS together).  Same bits as
 * aod_conv2d with the same descriptor.  aod_halo_conv3x3_x3_applies() tells whether a descriptor qualifies. */
int aod_halo_conv3x3_x3_applies(const aod_conv_desc_t* desc);
int aod_halo_conv3x3_x3(const aod_conv_desc_t* desc, const void* src, const void* w_packed, void* dst, const float* pre_shift,
                        aod_stream_t stream);

/* Calibration only (bench.py `roofline.measured_peaks`; no reference call site): `workgroups` x 4 waves issue `iters` x 16 independent bf16
 * MFMAs each and write {shader cycles, 100-MHz ticks} per workgroup to out_u64_pairs -- the clock the chip holds under matrix load
 * (csrc/probe.hip).  sink: one float the kernel may write (keeps the work alive). */
int aod_mfma_clock_probe(int iters, int workgroups, void* out_u64_pairs, float* sink, aod_stream_t stream);

/* The frozen stem of the reference-precision mode in one launch (csrc/stem_x3.hip; resnet.py:630-637): fp32 NCHW image [B][3][H][W] (even
 * H, W) -> y = max_pool_3x3_s2_p1(relu(bn1(conv1_7x7_s2(img)))) as X rows [B][H4][W4][128], H4 = (H/2 - 1) / 2 + 1.  w_x = the X filter
 * image [64][4][4][64] of the space-to-depth form of conv1 (aod_param_prep, flags bit 0, of the [64][12][4][4] filter); replaces
 * aod_x3_nchw_f32_to_s2d + aod_conv2d + aod_x3_maxpool3x3s2 and agrees with them to fp32 summation order. */
int aod_stem_pool_x3_fwd(const float* img, const void* w_x, const float* scale, const float* shift, void* y, int B, int C, int H, int W,
                         aod_stream_t stream);

/* SSD300-VGG16 (BASELINE config 0) in the reference-precision mode: the image as ONE 32-channel band of X rows (64 columns; the first VGG
 * conv reads it), and aod_maxpool_fwd/bwd, aod_l2norm_fwd/bwd on X rows (C = the X-layout width; L2Norm's w has C/2 entries). */
int aod_x3_nchw_f32_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, aod_stream_t stream);
int aod_x3_maxpool_fwd(const void* x, void* y, int B, int H, int W, int C, int OH, int OW, int k, int s, int p, aod_stream_t stream);
int aod_x3_maxpool_bwd(const void* x, const void* g, void* gx, int B, int H, int W, int C, int OH, int OW, int k, int s, int p, aod_stream_t stream);
int aod_x3_l2norm_fwd(const void* x, const float* w, void* y, int64_t rows, int C, float eps, aod_stream_t stream);
int aod_x3_l2norm_bwd(const void* x, const float* w, const void* g, void* gx, float* gw, int64_t rows, int C, float eps, aod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
