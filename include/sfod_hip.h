/* libsfod_hip.so -- C ABI of the MI355X (gfx950) teacher-student Faster R-CNN hot path.
 *
 * The reference (EPFL-IMOS/simple-SFOD) has no FFI: its hot path is Python calling
 * Detectron2 / torchvision / torch device ops.  Each entry point below replaces the device op
 * the reference reaches at the cited site (paths relative to /root/reference; "d2:" / "tv:" =
 * upstream Detectron2 / torchvision semantics restated in SURVEY.md Appendix A).
 *
 * Conventions
 *   - every pointer is a BORROWED device pointer (tensor.data_ptr()); the caller keeps the
 *     memory alive until the stream is synchronised.  The library never allocates.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is enqueued on it,
 *     nothing synchronises.
 *   - return value: 0 on success, negative hipError_t otherwise, -1000 for bad arguments.
 *   - activations are NHWC ("pixel-major rows, channels contiguous"); `dt` selects the storage /
 *     MFMA input type: SFOD_F32 (v_mfma_f32_32x32x2_f32), SFOD_BF16 (reduced precision:
 *     v_mfma_f32_32x32x16_bf16, fp32 accumulate) or SFOD_BF16X3 (fp32-equivalent arithmetic on the
 *     bf16 matrix pipe, the default mode): every MFMA operand element v is stored as the pair
 *     hi = bf16(v), lo = bf16(v - hi) (|v - hi - lo| <= 2^-16 |v|) and a product is accumulated in fp32 as
 *     hi*hi + hi*lo + lo*hi (three v_mfma_f32_32x32x16_bf16; the dropped lo*lo term is <= 2^-16 relative).
 *     Storage of a SFOD_BF16X3 tensor [.., C] (C a multiple of 8): 4 bytes per logical element, every group
 *     of 8 consecutive channels is 32 bytes = 8 x bf16 hi followed by 8 x bf16 lo.  Convolutions / GEMMs take
 *     SFOD_BF16X3 operands and write fp32; the elementwise producers (preprocess, BatchNorm apply, BatchNorm
 *     backward, ROIAlign, cast) write the pairs.
 *     SFOD_F16X3: the same storage and the same three-MFMA product with IEEE half pairs, hi = f16(v),
 *     lo = f16(v - hi) (v_mfma_f32_32x32x16_f16; subnormal inputs are kept): 22 significand bits per operand for
 *     |v| in [2^-3, 65504], an absolute 2^-25 below, +-65504 saturation above -- the operand format of the FORWARD
 *     products of cfg.SFOD.COMPUTE_DTYPE = "f16x3" (activations and weights, whose magnitudes sit in that window;
 *     gradients do not, the backward products of that mode use SFOD_BF16X3).  Served by the forward convolution /
 *     GEMM entry points and by every producer of operand pairs; the weight-gradient entry points take SFOD_BF16X3.
 *   - per-image variable-length results live in fixed-capacity arrays plus an int32 count per
 *     image, so that no entry point needs a host round trip.
 */
#ifndef SFOD_HIP_H
#define SFOD_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SFOD_F32 0
#define SFOD_BF16 1
#define SFOD_BF16X3 2
#define SFOD_F16X3 3

int sfod_version(void);
/* last error text of the calling thread ("" if none) */
const char* sfod_last_error(void);

/* ---- K1: preprocess.  d2 GeneralizedRCNN.preprocess_image (normalise, pad) as called at
 * daod/modeling/meta_arch/source_free_adaptive_teacher_rcnn.py:212 ; uint8 CHW BGR -> NHWC.
 * img_ptrs: device array of B pointers to uint8 [3,h_i,w_i]; sizes: int32 [B,2] (h,w);
 * out: [B,Hp,Wp,Cpad] (channels >= 3 are zero, padding pixels are zero). */
int sfod_preprocess(const void* const* img_ptrs, const int32_t* sizes, int B, int Hp, int Wp,
                    int Cpad, const float* mean3, const float* std3, void* out, int dt,
                    void* stream);

/* horizontal flip of a uint8 [C,H,W] image: the RandomFlip(0.5, horizontal) of the weak augmentation
 * (d2 build_augmentation; daod/data/mappers/two_crop_augmentation_mapper.py:73-157), on device */
int sfod_hflip_u8(const void* src, void* dst, int C, int H, int W, void* stream);

/* ResizeShortestEdge on a uint8 [C,H,W] frame -> [C,h,w], bit-exact with Pillow's Image.resize(..., BILINEAR)
 * (what d2's ResizeTransform calls for uint8 images; detection_utils / two_crop_augmentation_mapper.py:73-157):
 * separable support-scaled triangle filter, 22-bit fixed-point coefficients, uint8 clip between the passes.
 * hbounds/vbounds: int32 [out][2] = (first source index, tap count); hcoef/vcoef: int32 [out][ksize] fixed-point
 * weights -- built on the host like Pillow's precompute_coeffs + normalize_coeffs_8bpc.  flip != 0 also mirrors
 * the result horizontally (RandomFlip follows the resize). */
int sfod_resize_bilinear_u8(const void* src, void* dst, int C, int H, int W, int h, int w,
                            const int32_t* hbounds, const int32_t* hcoef, int ksize_h,
                            const int32_t* vbounds, const int32_t* vcoef, int ksize_v, int flip,
                            void* stream);
/* the general form: the whole weak augmentation of one frame -- d2 RandomCrop (INPUT.CROP), ResizeShortestEdge over any
 * INPUT.MIN_SIZE_TRAIN, RandomFlip horizontal or vertical (d2 build_augmentation; two_crop_augmentation_mapper.py:35-48) --
 * in one launch and without an intermediate crop tensor:
 *   dst [C,h,w] = flip(PIL.resize(src[:, y0:y0+ch, x0:x0+cw], (w, h), BILINEAR)),  bit for bit.
 * src is the whole [C,H,W] frame; the window's rows keep the frame's pitch W.  hbounds/hcoef are the tables for cw -> w,
 * vbounds/vcoef those for ch -> h (layout as above).  flip_mode: 0 none, 1 horizontal (output column w-1-x), 2 vertical
 * (output row h-1-y).  h == ch && w == cw is a windowed copy (+ flip), as Pillow returns a copy there: the filter does not
 * run and the tables are not read.  The kernels' 8-byte tap loads may read bytes outside the window but inside the frame
 * (weight 0), never outside the frame.  Refused with SFOD_EBADARG before any launch: a window not inside the frame, a
 * non-positive extent, flip_mode outside {0, 1, 2}, a NULL image or (when the filter runs) table.
 * sfod_resize_bilinear_u8 is this call with the full window and flip_mode = (flip != 0). */
int sfod_resize_bilinear_u8_opt(const void* src, void* dst, int C, int H, int W, int y0, int x0, int ch, int cw,
                                int h, int w, const int32_t* hbounds, const int32_t* hcoef, int ksize_h,
                                const int32_t* vbounds, const int32_t* vcoef, int ksize_v, int flip_mode,
                                void* stream);

/* Mosaic composition of one training image in one launch (daod/data/mappers/mosaic.py:81-265, MosaicDetection.__getitem__):
 *   canvas [2*H0][2*W0] = fill;  for tile k in order:  canvas[ly1:ly2, lx1:lx2] = U_k[sy1:sy2, sx1:sx2]  with
 *   U_k = PIL.resize(tile_k [3,h0,w0], (w, h), BILINEAR), bit for bit (the arithmetic of sfod_resize_bilinear_u8);
 *   out [3,H0,W0][c][y][x] = (canvas[2y][2x] + canvas[2y][2x+1] + canvas[2y+1][2x] + canvas[2y+1][2x+1] + 2) >> 2.
 * Neither the canvas nor any U_k is written to memory.  tiles, tabs and geom are HOST arrays, read before the call returns
 * (the geometry travels in the launch arguments, nothing is uploaded):
 *   tiles [n_tiles]      device pointers to the uint8 [3,h0,w0] tiles
 *   tabs  [n_tiles][2]   device pointers to the horizontal (w0 -> w) and vertical (h0 -> h) table of each tile: int32 bounds
 *                        [out][2] = (first source index, tap count) immediately followed by int32 coefficients [out][ksize]
 *                        (the layout sfod_resize_bilinear_u8 takes as two pointers).  Both NULL: identity scale, the tile is
 *                        already at canvas scale (h == h0, w == w0) and is copied.
 *   geom  [n_tiles][14]  int32: h0, w0, h, w, lx1, ly1, lx2, ly2, sx1, sy1, sx2, sy2, ksize_h, ksize_v
 * Refused with SFOD_EBADARG before any launch (out untouched): n_tiles outside 1..4, fill outside 0..255, a NULL tile / out,
 * one table of a tile NULL, a paste rectangle that leaves the canvas, a source rectangle that leaves its up-scaled tile,
 * rectangles whose two sides differ in extent, a table-less tile that is not at canvas scale. */
int sfod_mosaic_u8(const void* const* tiles, const void* const* tabs, const int32_t* geom, int n_tiles, int fill,
                   void* out, int H0, int W0, void* stream);

/* ---- K2/K5/K14/K18: implicit-GEMM convolution / linear layer on MFMA.
 * y[m, n] = act( sum_{tap, c} x[pix(m) + tap][c] * w[n][tap][c] + bias[n] ),  m = (b, oy, ox)
 * x: [B,H,W,Cin] NHWC, w: packed [Cout][KH*KW][Cin] (K contiguous), y: [B,H,W,ldy] with ldy >=
 * Cout.  KH=KW=3 pad 1 (vgg.py:18 conv3x3; d2 StandardRPNHead.conv; dann.py:14-17) or KH=KW=1
 * (1x1 convs and nn.Linear: x [R,K] -> y [R,N]).  act: 0 none, 1 ReLU, 2 LeakyReLU(0.2).
 * stats (optional, fp32 [nblk][2][Cout] followed by [nblk] row counts, nblk from
 * sfod_conv_stats_blocks): per-row-block (sum, M2, count) of the pre-activation output for the
 * train-mode BatchNorm that follows (vgg.py:20).  out_dt may differ from dt (e.g. fp32
 * logits out of a bf16 head).  Also used for data-gradient (dgrad) with rotated weights. */
int sfod_conv_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W,
                  int Cin, int Cout, int ksize, int ldy, int act, float* stats, int dt, int out_dt,
                  void* stream);
/* the same for SFOD_F16X3 weights packed with their per-tensor power-of-two scale (sfod_pack_*_ws below): w_absmax is the
 * device word the packer published (bits of max|w|); the kernels multiply their accumulators by the inverse scale before
 * bias / statistics / activation (exact).  w_absmax == NULL: unscaled weights (= sfod_conv_fwd). */
int sfod_conv_fwd_ws(const void* x, const void* w, const uint32_t* w_absmax, const float* bias, void* y, int B, int H,
                     int W, int Cin, int Cout, int ksize, int ldy, int act, float* stats, int dt, int out_dt,
                     void* stream);
/* the same with device scratch the library may use (sfod_conv_fwd_scratch_bytes for the shape; 0 = none wanted, and the
 * call is then sfod_conv_fwd_ws).  Today: linear layers (ksize 1, fp32 output, no statistics) with so few rows that their
 * grid fills less than half the chip -- the ROI head's fc1 at one frame per GPU, 512 x 25088 -> 1024 -- run split along K;
 * the scratch holds the S partial outputs (S x rows x Cout floats), summed in index order with bias and activation by a
 * second launch (run-to-run identical; differs from the unsplit kernel by fp32 summation order).  scratch == NULL or too
 * small: the unsplit kernel.  SFOD_GEMM_SPLITK=0 in the environment switches the split form off (A/B runs). */
int64_t sfod_conv_fwd_scratch_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int dt, int out_dt, int with_stats);
int sfod_conv_fwd_scratch(const void* x, const void* w, const uint32_t* w_absmax, const float* bias, void* y, int B, int H,
                          int W, int Cin, int Cout, int ksize, int ldy, int act, float* stats, int dt, int out_dt,
                          void* scratch, int64_t scratch_bytes, void* stream);
/* number of statistics blocks nblk sfod_conv_fwd writes for this layer shape; `stats` holds
 * nblk * (2*Cout + 1) floats.  The query sees neither ldy nor out_dt: it answers for dense rows (ldy = Cout) and the
 * operands' own output type (fp32 for operand pairs).  A launch with stats != NULL whose real ldy / out_dt select a kernel
 * that writes another number of blocks -- a bf16 first layer (Cin 8 -> 64) written as fp32 or with ldy % 8 != 0 runs the
 * generic kernel instead of the first-layer one -- returns SFOD_EBADARG before anything is launched, with a
 * sfod_last_error text that names sfod_conv_stats_blocks. */
int sfod_conv_stats_blocks(int B, int H, int W, int Cin, int Cout, int ksize, int dt);
/* kernel selection for 3x3 bf16 convolutions: 0 auto, 1 generic implicit GEMM (im2col chunks
 * DMA'd per tap), 2 halo-patch kernel (input patch staged once per 32-channel slice and reused by
 * all nine taps) whenever the shape allows.  3 / 4: auto for everything but the generic bf16x3 weight
 * gradient (1x1 / linear layers, 3x3 layers the halo-patch kernel does not take), which then ALWAYS runs
 * its 64 x 64 kernel (3: k_conv_wgrad<bf16_t,2,2,1>) / its wide 128 x 256 kernel wherever the operands
 * allow it, i.e. Cout >= 128 and ksize^2 * Cin >= 256 (4: k_conv_wgrad_x3w), instead of choosing by the
 * size of the output.  Any other value means 0.  For A/B tests and benchmarks. */
int sfod_set_conv_algo(int algo);
/* Data gradient of a 3x3 convolution with the BatchNorm-backward REDUCTION of the layer below folded into its epilogue
 * (the hand-written backward of vgg.py's conv-BN-ReLU chain; torch autograd runs these as separate kernels).
 * x: the upper layer's dy [B,H,W,Cin] (operand dtype dt), w: its rotated weights, dz [B,H,W,Cout] fp32 (dense): the
 * gradient w.r.t. the lower layer's activated output.  y / mean / invstd / gamma / beta: the lower layer's saved
 * pre-BatchNorm output (fp32 [B,H,W,Cout]) and BatchNorm inputs; red_ws receives sfod_conv_dgrad_bnred_blocks(...) rows
 * of 2 * Cout partial sums for sfod_bn_relu_pool_bwd(reduced_blocks = that count).  _blocks returns 0 when the shape /
 * dtype is not served by the halo-patch kernel: use sfod_conv_fwd and the unfused BatchNorm backward then. */
int sfod_conv_dgrad_bnred_blocks(int B, int H, int W, int Cin, int Cout, int dt);
int sfod_conv_dgrad_bnred(const void* x, const void* w, void* dz, int B, int H, int W, int Cin, int Cout, int dt,
                          const float* y, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, float* red_ws, void* stream);
/* K2 with the PRODUCER's BatchNorm + ReLU folded into the operand path (vgg.py:18-20: conv -> BatchNorm2d -> ReLU -> conv, the
 * activated tensor consumed by nobody else: forward-only passes such as the teacher's, source_free_adaptive_teacher.py:385-390).
 * x_pre: the producer's pre-BatchNorm output, fp32 [B,H,W,Cin]; in_mean / in_invstd / in_gamma / in_beta [Cin]: its batch
 * statistics and affine parameters.  The kernel computes relu((x - mean) * (invstd * gamma) + beta) and the (hi, lo) split of
 * SFOD_BF16X3 -- the arithmetic of sfod_bn_relu_pool_fwd, bit for bit -- on each patch slice in LDS; w / bias / y / stats / act
 * as in sfod_conv_fwd (3x3, y fp32).  _supported: 1 when the shape is served (dt SFOD_BF16X3, Cin % 32 == 0, the halo-patch
 * kernel's 256 x 128 shape); otherwise run sfod_bn_relu_pool_fwd + sfod_conv_fwd.  It also answers 0 -- process-wide
 * settings, not properties of the shape -- when the generic implicit-GEMM path is forced (sfod_set_conv_algo(1)), when the
 * 16x16x32 form is switched off (sfod_set_conv3x3_m16(0) / SFOD_P3_M16=0: the fold exists on that form only) and when a
 * workgroup-shape variant other than auto / 2 / 5 / 6 is forced (sfod_set_conv3x3_variant).  The caller decides WHETHER to
 * use it (the in-LDS transform costs the convolution 12-15 %; backbone_vgg.py takes it in forward-only train-mode passes
 * for producers whose fp32 output is >= 256 MB: conv2_1 from 3 frames per GPU at 600 x 1200, conv3_1 / conv3_2 from 6;
 * conv4_x never, see profiles/r4_bnin_layers.txt). */
int sfod_conv_fwd_bnin_supported(int B, int H, int W, int Cin, int Cout, int dt);
int sfod_conv_fwd_bnin(const float* x_pre, const float* in_mean, const float* in_invstd, const float* in_gamma,
                       const float* in_beta, const void* w, const float* bias, float* y, int B, int H, int W, int Cin,
                       int Cout, int ldy, int act, float* stats, int dt, void* stream);
/* Tile shape of the generic implicit-GEMM kernel behind sfod_conv_fwd (1x1 / linear / first layer), 0..8 (other values: 0):
 * 0 = the planner's choice (environment SFOD_GEMM_TILE), 1 = 128 x 64, 2 = 128 x 128, 3 = 256 x 128, 4 = 256 x 64, 5 = 256 x 256 (pairs, fp32 out),
 * 6 / 7 / 8 = 256 x 128 / 128 x 128 / 256 x 128 (four stages) with 64-byte K stages (pairs, fp32 out: two or three
 * workgroups per CU); shapes a layer cannot take fall back to the planner's.  Every shape computes the same values.  For
 * A/B runs and parity tests. */
int sfod_set_gemm_tile(int tile);
/* workgroup shape of the halo-patch kernel, 0..9: 0 auto, 1 = 512 px x 128 ch, 2 = 256 x 128, 3 = 256 x 64,
 * 4 = 512 x 64 (3 / 4 need physical Cin % 64 == 0, else they run as 2 / 1), 5 = 256 x 128 on v_mfma_f32_16x16x32 (operand
 * pairs with logical Cin % 32 == 0; otherwise as 2: 8 waves x (64 px x 64 ch), four waves per SIMD), 6 = the same with 4
 * waves x (128 px x 64 ch), two per SIMD (leaves registers for a co-resident kernel; tools/experiments/corun_conv_bn.py),
 * 7 / 8 = shapes 3 / 4 on v_mfma_f32_16x16x32 (4 waves x (64 px x 64 ch) / 8 waves of them), 9 = shape 3 on it with 8 waves
 * x (32 px x 64 ch), two workgroups = 16 waves per CU.  7 / 8 / 9 need operand pairs with physical Cin % 64 == 0 (logical
 * Cin % 32 == 0); with fewer channels they run as the 32x32x16 kernel of shape 2 / 1 / 2, on other operands as 3 / 4 / 3.
 * Any value outside 1..9 means auto.  sfod_last_conv_kernel names the kernel a launch ran.  For A/B runs and parity tests. */
int sfod_set_conv3x3_variant(int variant);
/* the kernel instantiation the calling thread's last convolution launch ran (halo-patch forward / data gradient, generic
 * implicit GEMM incl. split-K, halo-patch and generic weight gradient), e.g. "k_conv3x3_m16<8,2,1,0,0,1>": copied into buf
 * (NUL-terminated, truncated to n - 1 characters); returns the full length, 0 if nothing was launched yet, -1000 for a NULL
 * buf or n <= 0.  A host-side record set where the launch is issued; it says which code ran, not whether it finished. */
int sfod_last_conv_kernel(char* buf, int n);
/* Deterministic gradients (default 0; environment SFOD_DETERMINISTIC, config SFOD.DETERMINISTIC): the generic weight-gradient
 * kernels (1x1 / linear / first layer / fp32) store every pixel split's partial tile into a slab of the workspace
 * (sfod_conv_wgrad_ws_bytes grows accordingly) and sum the slabs in split order instead of combining them with float atomics,
 * the bias gradient runs one workgroup per 64 columns: bit-identical results from run to run (the halo-patch 3x3 weight
 * gradient, BatchNorm and ROIAlign backward are always order-fixed).  sfod_get_deterministic: the current setting. */
int sfod_set_deterministic(int on);
int sfod_get_deterministic(void);
/* whether the automatic choice runs shape 2 as shape 5 (default 1; environment SFOD_P3_M16).  Same tiles, same products,
 * another fp32 summation order inside a 32-deep k-step. */
int sfod_set_conv3x3_m16(int on);
/* A/B knob of the bf16x3 halo-patch weight gradient (environment SFOD_W3_PIPE): 2 (default) the 64 co x 64 ci block on
 * 128-pixel tiles (k_wgrad3x3_w64; layers with Cin >= 64, else as 1), 1 the pipelined 64 x 32-block loop
 * (k_wgrad3x3_patch<4, true, true>), 0 the round-2 loop.  0 and 1 give bit-identical results, 2 sums the same products over
 * other pixel tiles (equal to fp32 summation order). */
int sfod_set_wgrad3x3_pipe(int on);
/* which kernel sfod_conv_fwd runs for this shape (dense rows, the operands' own output type, the current
 * sfod_set_conv_algo / sfod_set_gemm_tile settings): 0 extents not served, 1 generic implicit GEMM, 2 halo-patch, 3
 * first-layer kernel (Cin = one padded 8-channel chunk, Cout = 64), 4 generic implicit GEMM on its 256 x 256 tile (bf16x3
 * linear layers / 1x1 convolutions with wide outputs) */
int sfod_conv_fwd_algo(int B, int H, int W, int Cin, int Cout, int ksize, int dt);

/* dt: SFOD_BF16 (x, w, y bf16) or SFOD_BF16X3 (x, w operand pairs; y: the activated operand pairs of the next layer).
 * First VGG layer (3 real channels in one 8-wide chunk -> 64, bf16) with the train-mode BatchNorm + ReLU folded in
 * by recomputation -- the layer's K is 27, its cost is writing 64 channels per pixel: pass 1 (y = NULL) produces
 * only the BatchNorm partial statistics (nothing stored), pass 2 (scale = gamma * invstd, shift = beta - mean *
 * scale, act = 1) recomputes the convolution and stores z = relu(scale * (conv + bias) + shift) directly, so
 * neither y nor a separate BatchNorm pass exist.  For forward-only use (the teacher: vgg.py:15-20 under no_grad;
 * a backward needs y).  stats layout / count as sfod_conv_fwd for this shape (sfod_conv_stats_blocks). */
int sfod_conv_first_supported(int B, int H, int W, int Cin, int Cout, int dt, int ldy);
int sfod_conv_first_fused(const void* x, const void* w, const float* bias, const float* scale,
                          const float* shift, void* y, float* stats, int B, int H, int W, int ldy,
                          int act, int dt, void* stream);
int sfod_conv_first_fused_ws(const void* x, const void* w, const uint32_t* w_absmax, const float* bias,
                             const float* scale, const float* shift, void* y, float* stats, int B, int H, int W,
                             int ldy, int act, int dt, void* stream);
/* The two entry points above run the first-layer kernel at ANY extent (sfod_conv_first_supported says where sfod_conv_fwd
 * itself picks it, and only there does sfod_conv_stats_blocks give this kernel's count); its statistics are one block per
 * 8 x 32-pixel tile: sfod_conv_first_stats_blocks (0 for hostile extents).
 * A/B knobs of the SFOD_BF16X3 / SFOD_F16X3 kernel, same bits at every setting: sfod_set_conv_first_pipe (environment
 * SFOD_F1_PIPE, default 1) 1 = the pipelined tile loop (next tile's patch in flight, one barrier less per tile, no masks on
 * full tiles), 0 = the plain loop; sfod_set_conv_first_grid (SFOD_F1_GRID, default 0) n > 0 caps the persistent grid at n
 * workgroups (tests: several tiles per workgroup on small images), 0 = one workgroup per resident slot. */
int sfod_conv_first_stats_blocks(int B, int H, int W);
int sfod_set_conv_first_pipe(int on);
int sfod_set_conv_first_grid(int n);
/* Student conv1_1, pass 2 by recomputation: z = relu(bn(conv(x) + bias)) as SFOD_BF16X3 pairs [B,H,W,ldz], BIT-IDENTICAL to
 * sfod_conv_fwd (fp32 y) followed by sfod_bn_relu_pool_fwd(y, mean, invstd, gamma, beta -> SFOD_BF16X3, ReLU, no pooling):
 * the same kernel recomputes the K = 27 convolution (reads the 8-channel input instead of the 64-channel y) and its
 * epilogue is that pass's arithmetic, operation for operation.  y itself still comes from sfod_conv_fwd (the backward
 * reads it).  _supported: 1 only for Cin = 8, Cout = 64, pool_flags = 0 (no pooling, ReLU: the flags of
 * sfod_bn_relu_pool_fwd), dt = SFOD_BF16X3, y_dt = SFOD_F32, a shape for which sfod_conv_fwd runs the first-layer kernel,
 * and the knob below at 1; elsewhere the caller runs sfod_bn_relu_pool_fwd.
 * sfod_set_first_apply_recompute (environment SFOD_FIRST_APPLY_RECOMPUTE, default 1): A/B knob, 0 = the query refuses. */
int sfod_conv_first_bn_apply_supported(int B, int H, int W, int Cin, int Cout, int pool_flags, int dt, int y_dt);
int sfod_conv_first_bn_apply(const void* x, const void* w, const float* bias, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, void* z, int B, int H, int W, int ldz, int dt,
                             void* stream);
int sfod_set_first_apply_recompute(int on);

/* weight gradient: dw[n][tap][c] += sum_m dy[m][n] * x[pix(m)+tap][c]  (fp32, packed layout, added
 * into the caller's (zero-initialised) buffer).  3x3 bf16 layers run the halo-patch kernel: pixel
 * splits write fp32 slabs into `ws` (sfod_conv_wgrad_ws_bytes, may be 0 -> ws unused) and are summed
 * in a fixed order; other shapes use the generic kernel (split over row chunks, float atomics).
 * A batch whose x or dy passes the kernel's 32-bit byte offsets is walked in sub-batches inside the one
 * call; sfod_conv_wgrad_ws_bytes is the LARGEST need of any sub-batch (a smaller remainder can want more
 * slabs than a full one), and a smaller workspace is refused before anything is launched.  0 for hostile
 * extents and for an empty gradient (no pixels, no input or output channels, ksize 0). */
int64_t sfod_conv_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int lddy, int dt);
int sfod_conv_wgrad(const void* x, const void* dy, float* dw, int B, int H, int W, int Cin,
                    int Cout, int ksize, int lddy, int dt, void* ws, int64_t ws_bytes, void* stream);
/* the same gradient written straight in the state-dict layout OIHW [Cout][Cin][3][3] (fp32): overwritten
 * (accumulate 0) or added into (accumulate 1, e.g. the parameter's slice of the flat gradient buffer).
 * Only for shapes the halo-patch kernel serves (sfod_conv_wgrad_oihw_supported != 0): its slab
 * reduction does the layout change, so neither a packed temporary nor its zero fill exist. */
int sfod_conv_wgrad_oihw_supported(int B, int H, int W, int Cin, int Cout, int ksize, int lddy, int dt);
int sfod_conv_wgrad_oihw(const void* x, const void* dy, float* dw_oihw, int B, int H, int W, int Cin,
                         int Cout, int ksize, int lddy, int dt, int accumulate, void* ws,
                         int64_t ws_bytes, void* stream);
/* First VGG layer (conv1_1: x operand pairs with Cin = one 8-channel group, Cout = 64, no data gradient): the weight gradient
 * straight from the INPUTS of its BatchNorm + ReLU backward.  dz (gradient of the activated output) and y (saved
 * pre-BatchNorm output) are fp32 [B,H,W,64]; dgamma / dbeta are the FINALIZED sums of this layer (sfod_bn_relu_pool_bwd with
 * dy = NULL produces them without the apply pass).  The kernel (k_first_wgrad_bn) forms every dy pair in registers with the
 * expression and the (hi, lo) split of sfod_bn_relu_pool_bwd's apply pass and sums the products in the order of
 * sfod_conv_wgrad's / sfod_conv_wgrad_oihw's kernel: dw is BIT-IDENTICAL to sfod_bn_relu_pool_bwd(dy as SFOD_BF16X3)
 * followed by sfod_conv_wgrad (oihw = 0: dw packed [64][9][8], added into; `accumulate` ignored) or sfod_conv_wgrad_oihw
 * (oihw = 1: dw [64][8][3][3], overwritten or, accumulate = 1, added into), and dy (4 bytes x B*H*W*64, written and read
 * back once) never exists.  ws: sfod_conv_wgrad_ws_bytes of (B, H, W, 8, 64, 3, 64, SFOD_BF16X3).
 * _supported: 1 only for Cin = 8, Cout = 64, pool = 0 (no pooling, ReLU: the `pool` flags of sfod_bn_relu_pool_bwd), dt =
 * SFOD_BF16X3 (x), y_dt = SFOD_F32, a shape sfod_conv_wgrad_oihw serves with its halo-patch kernel in ONE sub-batch (tensors
 * below 2 GiB), and the knob below at 1; elsewhere the caller runs the two launches.
 * sfod_set_first_wgrad_fused (environment SFOD_FIRST_WGRAD_FUSED, default 1): A/B knob, 0 = the query refuses. */
int sfod_conv_first_wgrad_bn_supported(int B, int H, int W, int Cin, int Cout, int pool, int dt, int y_dt);
int sfod_conv_first_wgrad_bn(const void* x, const void* dz, const void* y, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, const float* dgamma, const float* dbeta,
                             float* dw, int B, int H, int W, int Cin, int Cout, int dt, int oihw, int accumulate,
                             void* ws, int64_t ws_bytes, void* stream);
int sfod_set_first_wgrad_fused(int on);

/* weight (re)packing between the reference's state-dict layouts and the kernel layouts.
 * OIHW fp32 [Cout][Cin][KH][KW] -> packed [Cout][KH*KW][CinPad] (dt); rot180=1 additionally
 * swaps in/out channels and flips the taps: the dgrad weight [Cin][KH*KW][Cout]. */
int sfod_pack_conv_weight(const float* w_oihw, void* w_packed, int Cout, int Cin, int ksize,
                          int CinPad, int rot180, int dt, void* stream);
/* SFOD_F16X3 weights with a per-tensor scale: half pairs keep 22 bits only for |v| >= 2^-3 and weights are uniformly
 * small, so the `_ws` packers first reduce max|w| of the fp32 source into the device word(s) `absmax` (bit pattern of a
 * non-negative float; one word per tensor), then store w * s with s the power of two that puts max|w| * s into
 * [2^13, 2^14).  The forward entry points (`sfod_conv_fwd_ws`, `sfod_conv_first_fused_ws`) take the same word and undo
 * the scale on their accumulators.  absmax == NULL: unscaled (any dt). */
int sfod_pack_conv_weight_ws(const float* w_oihw, void* w_packed, uint32_t* absmax, int Cout, int Cin, int ksize,
                             int CinPad, int rot180, int dt, void* stream);
/* every conv weight of a model in one launch.  desc (device, int64): n entries of 8 values
 * {src fp32 OIHW pointer, dst packed pointer, Cout, Cin, ksize, innerPad, rot180, first_block}, where
 * first_block is the running sum of sfod_pack_conv_weights_blocks over the preceding entries;
 * total_blocks = the sum over all entries.  Same layouts as sfod_pack_conv_weight. */
int sfod_pack_conv_weights_blocks(int Cout, int Cin, int ksize, int innerPad, int rot180);
int sfod_pack_conv_weights_multi(const int64_t* desc, int n, int total_blocks, int dt, void* stream);
int sfod_pack_conv_weights_multi_ws(const int64_t* desc, int n, int total_blocks, int dt, uint32_t* absmax /* [n] */,
                                    void* stream);
/* packed fp32 grad [Cout][taps][CinPad] -> OIHW fp32 grad (accumulate=0: overwrite) */
int sfod_unpack_conv_wgrad(const float* dw_packed, float* dw_oihw, int Cout, int Cin, int ksize,
                           int CinPad, int accumulate, void* stream);
/* nn.Linear weight [N][K] fp32 -> [N][Kperm] (dt) where, if chw_c > 0, the K axis is permuted
 * from (c, p) (flatten of [C,7,7], d2 FastRCNNConvFCHead) to (p, c) (our ROIAlign layout);
 * transpose=1 writes [K][N] instead (the dgrad operand).  out[n][p * C + c] = w[n][c * PP + p] with C = chw_c,
 * PP = K / C; chw_c > 0 with K % chw_c != 0 is refused with SFOD_EBADARG before any launch (pack and unpack). */
int sfod_pack_fc_weight(const float* w, void* out, int N, int K, int chw_c, int transpose, int dt,
                        void* stream);
int sfod_unpack_fc_wgrad(const float* dw_packed, float* dw, int N, int K, int chw_c,
                         int accumulate, void* stream);
/* same with an explicit leading dimension `ld` of the packed matrix (zero-padded inner axis, so
 * that every row is a whole number of 16-byte chunks, e.g. the 41 predictor outputs -> 48) */
int sfod_pack_fc_weight_ld(const float* w, void* out, int N, int K, int chw_c, int transpose, int ld,
                           int dt, void* stream);
int sfod_pack_fc_weight_ld_ws(const float* w, void* out, uint32_t* absmax, int N, int K, int chw_c, int transpose,
                              int ld, int dt, void* stream);
int sfod_unpack_fc_wgrad_ld(const float* dw_packed, float* dw, int N, int K, int chw_c, int ld,
                            int accumulate, void* stream);
/* column sums of a [M, ld] matrix's first N columns: bias gradients.  db[n] (+)= sum_m dy[m][n].  Held per column to the
 * fp64 sum within 8 sqrt(M) 2^-24 sum_m |dy[m][n]| (+ 2^-24 |db| when accumulating), in the sliced and the deterministic form
 * (tests/test_gpu_pointwise_definition.py); columns [N, ld) are never read. */
int sfod_bias_grad(const void* dy, float* db, int M, int N, int ld, int accumulate, int dt,
                   void* stream);

/* ---- K3/K4: train-mode BatchNorm2d + ReLU (+ 2x2 max-pool), NHWC.  vgg.py:15,20; torch
 * BatchNorm2d semantics of SURVEY.md A.14 (biased var to normalise, unbiased var into
 * running_var, momentum 0.1, eps 1e-5).  This is also the AdaBN running-stat refresh
 * (daod/engine/trainers/base.py:270-337): it runs identically under no_grad. */
int sfod_bn_finalize(const float* stats, int nblocks, int M, int C,
                     float* mean, float* invstd, float* running_mean, float* running_var,
                     float momentum, float eps, int update_running, int64_t* num_batches_tracked,
                     float* ws, void* stream);
/* update_running: 0 = leave the running statistics alone; k >= 1 = apply k momentum updates with this batch's
 * statistics (k forward passes over the same batch between two optimiser steps -- the reference's student runs its
 * backbone three times per step when its zero-weighted domain branch is on, source_free_adaptive_teacher.py:527-537).
 * num_batches_tracked: the BatchNorm buffer of that name (device int64 scalar), incremented by k; may be NULL. */
/* `stats` (written by the convolution's epilogue, nblocks * (2 * C + 1) floats): stats[blk][0][c] = the block's sum over its
 * rows, stats[blk][1][c] = the block's sum of squared deviations from ITS mean, then -- behind all the sums, at
 * stats + nblocks * 2 * C -- counts[blk] = the block's rows as a float; a block with count 0 is skipped. */
/* Population statistics (TEST.PRECISE_BN, AdaBN with precise=True): sfod_bn_finalize with one more operand.  `pop` is the
 * layer's accumulator, three rows of fp64 `pop_stride` doubles apart -- pop[c] = n, pop[pop_stride + c] = mean,
 * pop[2 * pop_stride + c] = M2 = sum (x - mean)^2 over everything seen so far -- so that all layers of a model can be columns
 * of one [3][sum C] tensor.  With pop != NULL the SAME launch that writes mean / invstd (bit-identical to sfod_bn_finalize's)
 * merges this batch (M, mu_b = sum x / M, tot = sum (x - mu_b)^2, both already held in fp64) by Chan's update
 *   d = mu_b - mean;  n' = n + M;  mean += d M / n';  M2 += tot + d^2 n M / n'
 * leaves running_mean / running_var alone and adds 1 to num_batches_tracked (whatever update_running says).  No further
 * launch, no atomics: one thread owns a channel.  pop == NULL is sfod_bn_finalize.  SFOD_EBADARG before any launch: pop not
 * 8-byte aligned, pop_stride <= 0 or < C. */
int sfod_bn_finalize_pop(const float* stats, int nblocks, int M, int C,
                         float* mean, float* invstd, float* running_mean, float* running_var,
                         float momentum, float eps, int update_running, int64_t* num_batches_tracked,
                         float* ws, double* pop, int64_t pop_stride, void* stream);
/* The accumulated statistics of every layer into their running buffers in ONE launch: running_mean = fp32(mean),
 * running_var = fp32(M2 / n) (biased; fp64 with one rounding).  `table` (device, int64) and `table_host` (the same values
 * on the host, read by the checks only): n <= 1024 entries of 4 values {first column, C, running_mean pointer,
 * running_var pointer}.  A layer with n = 0 (it never ran) keeps its buffers.  SFOD_EBADARG before any launch: pop NULL
 * or misaligned, pop_stride <= 0, an entry with first column + C > pop_stride or a NULL / misaligned buffer. */
int sfod_bn_pop_commit(const double* pop, int64_t pop_stride, const int64_t* table, const int64_t* table_host, int n,
                       void* stream);
/* dst <- Chan merge of two contiguous [3][columns] accumulators, column by column (dst first: merging the ranks'
 * accumulators in rank order gives every rank the same bits).  Columns with src n = 0 are left alone. */
int sfod_bn_pop_merge(double* dst, const double* src, int64_t columns, void* stream);
/* Layers whose statistics fit one slice (nblocks <= 64) are finalised by ONE launch instead of two (default 1; environment
 * SFOD_BN_FINALIZE_FUSED): the same sums in the same order, bit-identical outputs.  0 keeps the two launches (A/B runs, the
 * parity test). */
int sfod_set_bn_finalize_fused(int on);
/* size (in floats, 8-byte aligned) of the `ws` scratch of sfod_bn_finalize */
int sfod_bn_finalize_ws_floats(int C);
/* z = relu(gamma*(y-mean)*invstd+beta); `pool` is a flag word: bit 0 additionally 2x2/2 max-pools z
 * (floor: H / 2 by W / 2, the last row / column of an odd map is not covered), bit 1 drops the ReLU (d2 BottleneckBlock
 * conv3 / shortcut norms, no activation).
 * Definition the kernels are held to, per element (oracle/pointwise_definitions.py bn_affine,
 * tests/test_gpu_pointwise_definition.py): z_pre = (y - mean) * (invstd * gamma) + beta (+ residual) within 5 * 2^-24 of
 * (|y| + |mean|) |invstd gamma| + |beta| (+ |residual|), then the output rounding -- for every output type, the pair outputs
 * included.  The ReLU is fmaxf(z_pre, 0): a NaN gives +0 (it is NOT propagated, unlike torch.relu), -0 gives +0; the window
 * maximum drops a NaN the same way (identity 0 with the ReLU, -inf without).  sfod_bn_add_relu_fwd and sfod_add_act share
 * this, and the backward gates (z_pre > 0, y > 0) pass no gradient there. */
int sfod_bn_relu_pool_fwd(const void* y, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, void* z, int B, int H, int W,
                          int C, int pool, int dt, int out_dt, void* stream);
/* the same with a second output: out_dt SFOD_F16X3 (z: half pairs, the next convolution's forward operand) and z2 (may be
 * NULL) the same values as SFOD_BF16X3 pairs (that convolution's weight-gradient operand) -- "f16x3" mode, student pass */
int sfod_bn_relu_pool_fwd2(const void* y, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, void* z, void* z2, int B, int H, int W,
                           int C, int pool, int dt, int out_dt, void* stream);
/* Bottleneck tail of the ResNet path (d2 BottleneckBlock.forward, reached through build_resnet_backbone of the r101
 * yaml): z = relu(bn(y) + residual) in one pass over [rows, C]; same statistics / affine inputs as above.
 * z_pairs (may be NULL; dt SFOD_F32, C % 8 == 0): additionally the same values as operand pairs of type pairs_dt
 * (SFOD_BF16X3 / SFOD_F16X3) -- the block output is both the fp32 residual stream and the next convolution's MFMA
 * operand; z_pairs2 (may be NULL; pairs_dt SFOD_F16X3): once more as SFOD_BF16X3 pairs -- that convolution's
 * weight-gradient operand in "f16x3" mode. */
int sfod_bn_add_relu_fwd(const void* y, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, const void* residual, void* z, void* z_pairs, void* z_pairs2, int64_t rows,
                         int C, int dt, int pairs_dt, void* stream);
/* backward of the block above.  dz: grad w.r.t. block output; y: saved conv output; returns dy
 * (grad w.r.t. conv output), dgamma, dbeta.  ws: fp32 workspace [nblk*2*C] (see ws query).
 * Definition (oracle/pointwise_definitions.py bn_backward; held per channel / per element by
 * tests/test_gpu_pointwise_definition.py): g = dz routed to the FIRST maximum of z_pre in its 2x2 window in the order (0,0),
 * (0,1), (1,0), (1,1) -- an exact tie sends the whole gradient to the earlier member -- gated by z_pre > 0 unless bit 1 of
 * `pool`; dbeta = sum g, dgamma = sum g * xhat, dy = gamma * invstd * (g - dbeta / M - xhat * dgamma / M) with
 * xhat = (y - mean) * invstd and M = B * H * W: the leftover pixels of an odd H / W count in M, their g is 0 and their dy is
 * the mean terms alone.  A pooled map without any window (H or W = 1) has an empty dz (may be NULL): dgamma = dbeta = 0.
 * dgamma_acc / dbeta_acc (may be NULL): the parameters' gradient accumulators (+= this call's dgamma /
 * dbeta), so the caller needs no separate accumulate pass per BatchNorm layer.
 * dy == NULL: the sums only (reduction, or the pre-reduced rows, then the same finalize) -- no apply pass; for a layer
 * whose dy is formed by its consumer (sfod_conv_first_wgrad_bn). */
int sfod_bn_relu_pool_bwd(const void* dz, const void* y, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, void* dy, float* dgamma,
                          float* dbeta, float* dgamma_acc, float* dbeta_acc, float* ws, int B, int H,
                          int W, int C, int pool, int dt, int out_dt, int reduced_blocks, void* stream);
/* reduced_blocks > 0: `ws` already holds that many rows of partial (dbeta | dgamma) sums, written by the epilogue of the
 * data-gradient convolution that produced dz (sfod_conv_dgrad_bnred): the reduction pass over dz and y is skipped.
 * `ws` must then have SFOD_BN_BWD_SCRATCH_ROWS more rows of 2 * C floats behind them (scratch of the two-stage sum). */
#define SFOD_BN_BWD_SCRATCH_ROWS 32
int sfod_bn_bwd_ws_floats(int M, int C);
/* ---- GroupNorm + ReLU of the box head's convolutions (MODEL.ROI_BOX_HEAD.NORM "GN": d2 get_norm -> torch.nn.GroupNorm(32,
 * CONV_DIM), eps 1e-5, behind every conv of FastRCNNConvFCHead) on ROI tensors [R, PP, C], NHWC.  Statistics are per (ROI,
 * group) over the n = PP * C / groups elements of the group, in fp32: the mean first (sum / n), then the centred sum of
 * squares (var = sum (y - mean)^2 / n, biased); rstd = 1 / sqrt(var + eps).  E[y^2] - E[y]^2 is never formed.
 *   z = relu(((y - mean_g) * rstd_g) * gamma_c + beta_c)      (the last two as one fused multiply-add; relu = fmaxf(., 0))
 * y: the convolution's output, y_dt SFOD_F32 or SFOD_BF16.  z: z_dt = y_dt, or SFOD_BF16X3 / SFOD_F16X3 from an fp32 y (the
 * next layer's operand, written directly); z_grad_operand (may be NULL; z_dt SFOD_F16X3 only): the same values once more as
 * SFOD_BF16X3 pairs, that layer's weight-gradient operand (the producer-writes-both convention of sfod_bn_relu_pool_fwd2).
 * mean, rstd: fp32 [R, groups], saved for the backward.  An all-zero (padding) ROI gives exactly relu(beta), as does any
 * group of one element.  relu 0 / 1.  C <= 1024, C % groups == 0, C % 8 == 0 (fp32 z: C % 4 == 0); R == 0: no launch.
 * Held per element to DESIGN.md 4.7's bound (tests/helpers/box_head_definitions.py gn_forward_bound). */
int sfod_group_norm_relu_fwd(const void* y, const float* gamma, const float* beta, void* z, void* z_grad_operand,
                             float* mean, float* rstd, int R, int PP, int C, int groups, float eps, int relu, int y_dt,
                             int z_dt, void* stream);
/* backward: dz the gradient of z, y / mean / rstd as the forward saw and saved them.  The ReLU gate is RECOMPUTED from y
 * (the forward's own pre-activation expression, bit for bit: gate = pre-activation > 0), z is not needed.  With
 * gz = dz * gate, g = gz * gamma_c, xhat = (y - mean_g) * rstd_g and mean_grp the mean over the group's n elements:
 *   dy = rstd_g * (g - mean_grp(g) - xhat * mean_grp(g * xhat)),  dbeta_c = sum_{r,p} gz,  dgamma_c = sum_{r,p} gz * xhat.
 * dz, y: dt SFOD_F32 or SFOD_BF16; dy: dy_dt = dt, or SFOD_BF16X3 from fp32 (the operand of the backward products).
 * dgamma / dbeta: every workgroup writes the sums of its ROIs (taken in ROI order) to its row of ws
 * (sfod_group_norm_bwd_ws_floats(R, C) floats), a second launch adds the rows in row order: no atomics, the same bits on
 * every run; accumulate 1 adds the result into dgamma / dbeta (a parameter's gradient accumulator) instead of storing it.
 * A ROI whose dz is zero (a padding row) adds nothing and gets dy = 0.  R == 0: no kernel (dgamma = dbeta = 0 unless
 * accumulating). */
int sfod_group_norm_relu_bwd(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, void* dy, float* dgamma, float* dbeta, float* ws, int R, int PP, int C,
                             int groups, int relu, int accumulate, int dt, int dy_dt, void* stream);
int64_t sfod_group_norm_bwd_ws_floats(int R, int C);
/* ---- ResNet-101-C4 backbone helpers (d2 build_resnet_backbone selected by the r101 yaml's missing
 * BACKBONE.NAME, configs/r101_c4_cs_foggy_adaptive_teacher_source_free.yaml:1-28) ----
 * The pointwise kernels below (add_act, subsample2, maxpool3s2, act_bwd, add_inplace, add_act_bwd, mul_mask) are each ONE
 * fp32 operation per element, rounded once (nearest even) to bf16 for bf16 data: bit for bit equal to the same torch
 * operation in fp32 (tests/test_gpu_pointwise_definition.py), +-0, denormals and +-inf included.  NaN: sums and products
 * propagate it; the ReLU of sfod_add_act (act 1) is fmaxf(v, 0) = +0 for a NaN and for -0, like the BatchNorm + ReLU
 * kernels (pinned -- torch.relu would propagate the NaN); a gate (y > 0) is closed for y = NaN and y = -0.
 * out = act(a + b), act 0/1: residual join of BottleneckBlock (relu(conv3(x) + shortcut(x))); out_pairs (may be NULL,
 * fp32 data, n % 8 == 0 with 8-channel groups): the same values as operand pairs of type pairs_dt; out_pairs2 (may be NULL;
 * pairs_dt SFOD_F16X3): once more as SFOD_BF16X3 pairs */
int sfod_add_act(const void* a, const void* b, void* out, void* out_pairs, void* out_pairs2, int64_t n, int act, int dt,
                 int pairs_dt, void* stream);
/* backward=0: dst [B,ceil(H/2),ceil(W/2),C] = src [B,H,W,C] at even pixels (data movement of a 1x1
 * stride-2 conv, STRIDE_IN_1X1); backward=1: the adjoint (dst [B,H,W,C] zero except even pixels) */
int sfod_subsample2(const void* src, void* dst, int B, int H, int W, int C, int backward, int dt,
                    void* stream);
/* ResNet BasicStem as one kernel on operand pairs (d2 build_resnet_backbone: conv 7x7 stride 2 pad 3, 3 -> 64, FrozenBN
 * folded into w / bias, ReLU): replaces sfod_im2col_stem + sfod_conv_fwd for dt SFOD_BF16X3 / SFOD_F16X3 -- the [pixels][160]
 * operand matrix is gathered from an LDS patch of the input in registers and never written (bit-identical output: same k
 * order, same splits, same MFMA sequence).  x fp32 [B,H,W,Cp] (channels 0-2 used, Cp % 4 == 0); w_packed: sfod_pack_fc_weight
 * of the [64][160] matrix (k = (ky*7+kx)*3+c, zero columns from 147), w_absmax its SFOD_F16X3 scale word or NULL;
 * y fp32 [B,Ho,Wo,64], Ho = (H-1)/2+1.  act 0 / 1 (ReLU).  The max-pool that follows stays sfod_maxpool3s2. */
int sfod_stem7x7_supported(int B, int H, int W, int Cp, int dt);
int sfod_stem7x7(const float* x, const void* w_packed, const uint32_t* w_absmax, const float* bias, float* y, int B, int H,
                 int W, int Cp, int act, int dt, void* stream);
/* im2col of BasicStem's 7x7 stride-2 pad-3 conv: out [B,Ho,Wo,Kpad], column (ky*7+kx)*3+c; out_dt = dt, or
 * SFOD_BF16X3 from fp32 input (the stem GEMM's operand pairs, written directly) */
int sfod_im2col_stem(const void* x, void* out, int B, int H, int W, int Cp, int Kpad, int dt, int out_dt,
                     void* stream);
/* BasicStem max_pool2d(kernel 3, stride 2, padding 1), forward (the stem is frozen).  The maximum of the window's in-map
 * pixels by fmaxf from -inf: -inf is an ordinary value, a NaN is dropped (torch propagates it). */
int sfod_maxpool3s2(const void* x, void* y, int B, int H, int W, int C, int dt, void* stream);
/* elementwise: dx = y > 0 ? dy : +0 (act 1, ReLU) or y > 0 ? dy : 0.2f * dy (act 2, LeakyReLU, the fp32 slope) in place on dy */
int sfod_act_bwd(void* dy, const void* y, int64_t n, int act, int dt, void* stream);
/* a += b  (fp32 or bf16 elementwise) */
int sfod_add_inplace(void* a, const void* b, int64_t n, int dt, void* stream);
/* a = (a + b) * [y > 0]: sum of a residual join's two gradient branches taken through the ReLU of the block below
 * (its output y) in one pass -- sfod_add_inplace followed by sfod_act_bwd(act 1) */
int sfod_add_act_bwd(void* a, const void* b, const void* y, int64_t n, int dt, void* stream);
/* a = mask ? a * scale : 0 (mask: one 0/1 byte per element): F.dropout forward and backward of the
 * instance-level domain discriminator (daod/modeling/dann/dann.py:146-151), scale = 1 / (1 - p) */
int sfod_mul_mask(void* a, const uint8_t* mask, int64_t n, float scale, int dt, void* stream);

/* ---- K6/K7: anchors + proposal decode.  d2 DefaultAnchorGenerator / Box2BoxTransform /
 * find_top_rpn_proposals reached from daod/modeling/proposal_generator/rpn.py:25,54-56.
 * rpn_out: fp32 [B*Hf*Wf, ld]: cols [0,A) objectness, cols [A, 5A) deltas (a*4+j).
 * props: [B,NA,4] decoded+clipped boxes (order y,x,a); scores: [B,NA]; flags[0] |= 1 if any
 * non-finite prediction (d2 raises FloatingPointError). */
int sfod_rpn_decode(const float* rpn_out, int ld, const float* cell_anchors, int A, int B, int Hf,
                    int Wf, int stride, const int32_t* image_sizes, float* props, float* scores,
                    int32_t* flags, void* stream);
/* General form: Box2BoxTransform weights (wx, wy, ww, wh) = MODEL.RPN.BBOX_REG_WEIGHTS by value (finite, > 0, else
 * SFOD_EBADARG).  sfod_rpn_decode is this call with (1, 1, 1, 1): one kernel, bit-identical results. */
int sfod_rpn_decode_opt(const float* rpn_out, int ld, const float* cell_anchors, int A, int B, int Hf,
                        int Wf, int stride, const int32_t* image_sizes, float* props, float* scores,
                        int32_t* flags, float wx, float wy, float ww, float wh, void* stream);
/* ---- Proposal and matcher options (MODEL.ANCHOR_GENERATOR.OFFSET, MODEL.RPN.BOUNDARY_THRESH,
 * MODEL.PROPOSAL_GENERATOR.MIN_SIZE, MODEL.ROI_HEADS.IOU_THRESHOLDS / IOU_LABELS).  The entry points that rebuild the
 * anchors in registers (sfod_rpn_decode_shift, sfod_anchor_match_opt, sfod_rpn_loss_shift) take, by value:
 *   shift   float32(OFFSET * stride): the caller's product of two python doubles rounded ONCE (the convention of
 *           ema_one_minus_keep below; float32(OFFSET) * stride rounds twice and differs, e.g. for OFFSET 0.3, stride 16).
 *           Anchor (y, x, a) = cell_anchors[a] + (sx, sy, sx, sy) with sx = shift + (float)(x * stride),
 *           sy = shift + (float)(y * stride): one fp32 add each, no contraction -- the float32
 *           torch.arange(offset * stride, n * stride, step=stride) of d2's _create_grid_offsets.  shift must be 0 or finite
 *           and inside (0, stride), else SFOD_EBADARG.  shift 0 gives the bits of the forms without it (0.f + v == v).
 * Every pointer, extent and float of these entry points is checked before anything is launched.
 * sfod_rpn_decode_shift: sfod_rpn_decode_opt with `shift`; sfod_rpn_decode_opt is this call with shift 0. */
int sfod_rpn_decode_shift(const float* rpn_out, int ld, const float* cell_anchors, int A, int B, int Hf,
                          int Wf, int stride, const int32_t* image_sizes, float* props, float* scores,
                          int32_t* flags, float wx, float wy, float ww, float wh, float shift, void* stream);
/* stable descending segmented sort of B segments of n floats; out_idx int32 [B,n].
 * ws: workspace of sfod_sort_ws_bytes(B,n) bytes. */
int64_t sfod_sort_ws_bytes(int B, int n);
int sfod_segmented_sort_desc(const float* keys, int B, int n, float* out_keys, int32_t* out_idx,
                             void* ws, int64_t ws_bytes, void* stream);
/* gather the first k sorted candidates: boxes[b][j] = props[b][idx[b][j]], valid = nonempty and a finite score (d2's
 * find_top_rpn_proposals drops a candidate whose box or logit is not finite; a non-finite box is empty after the clip) */
int sfod_rpn_gather_topk(const float* props, const float* sorted_scores, const int32_t* sorted_idx,
                         int B, int NA, int k, float* cand_boxes, float* cand_scores,
                         uint8_t* cand_valid, void* stream);
/* General form: min_size = MODEL.PROPOSAL_GENERATOR.MIN_SIZE, finite and >= 0 (else SFOD_EBADARG):
 * valid = (x2 - x1) > min_size && (y2 - y1) > min_size on the clipped box, strict (d2 Boxes.nonempty(threshold)).
 * sfod_rpn_gather_topk is this call with 0. */
int sfod_rpn_gather_topk_opt(const float* props, const float* sorted_scores, const int32_t* sorted_idx,
                             int B, int NA, int k, float min_size, float* cand_boxes, float* cand_scores,
                             uint8_t* cand_valid, void* stream);

/* ---- K8/K16: greedy NMS.  tv nms / batched_nms via d2 batched_nms (Appendix A.6):
 * boxes already sorted by descending score; suppress j>i when IoU > thr (strict, fp32, no +1).
 * classes (optional int32): pairs of different class never suppress each other ("vanilla"
 * batched_nms); alt_boxes/mode (optional): per image mode[b]!=0 selects alt_boxes (the
 * coordinate-offset boxes) and disables the class test -- torchvision's strategy switch.
 * n_per_image (optional int32 [B]) bounds the live prefix, else n.  mask: u64 [B,n,ceil(n/64)].
 * keep_idx int32 [B,max_keep] (positions in the sorted order), keep_count int32 [B]. */
int64_t sfod_nms_mask_bytes(int B, int n);
int sfod_nms(const float* boxes, const float* alt_boxes, const int32_t* classes,
             const int32_t* mode, const uint8_t* valid, const int32_t* n_per_image, int B, int n,
             float thr, int max_keep, uint64_t* mask, int32_t* keep_idx, int32_t* keep_count,
             void* stream);
/* proposals[b][j] = cand_boxes[b][keep_idx[b][j]] for j < keep_count[b], zero-filled above */
int sfod_gather_kept(const float* cand_boxes, const float* cand_scores, const int32_t* keep_idx,
                     const int32_t* keep_count, int B, int n, int max_keep, float* out_boxes,
                     float* out_scores, void* stream);

/* ---- K9/K12: pairwise IoU + Matcher.  d2 pairwise_iou + Matcher (Appendix A.8) as reached
 * from rpn.py:45 (anchors, thresholds [0.3,0.7], labels [0,-1,1], low-quality on) and
 * source_free_adaptive_teacher_roi_heads.py:179-183 (proposals, [0.5], [0,1]).
 * anchors are generated in-kernel from (Hf,Wf,stride,cell_anchors).  gt: [B,Gcap,4] + count.
 * out: matched int32 [B,NA], labels int8 [B,NA]; gtmax fp32 [B,Gcap] scratch. */
int sfod_anchor_match(const float* cell_anchors, int A, int B, int Hf, int Wf, int stride,
                      const float* gt_boxes, const int32_t* gt_count, int Gcap, float lo, float hi,
                      int32_t* matched, int8_t* labels, float* gtmax, void* stream);
/* General form: `shift` (above) and MODEL.RPN.BOUNDARY_THRESH.  image_sizes: int32 [B,2] as (h, w), the layout
 * sfod_rpn_decode reads.  With t = boundary_thresh >= 0, AFTER the matcher's label (low-quality promotion included, and also
 * for an image without ground truth, whose anchors are all 0) an anchor is relabelled -1 unless
 *   x1 >= -t && y1 >= -t && x2 < w + t && y2 < h + t            (d2 Boxes.inside_box, fp32, on the anchor built above).
 * boundary_thresh < 0: the test is off and image_sizes may be NULL; >= 0 with NULL image_sizes, NaN or +inf: SFOD_EBADARG.
 * `matched` does not depend on it.  sfod_anchor_match is this call with shift 0, boundary_thresh -1, NULL. */
int sfod_anchor_match_opt(const float* cell_anchors, int A, int B, int Hf, int Wf, int stride,
                          const float* gt_boxes, const int32_t* gt_count, int Gcap, float lo, float hi,
                          float shift, float boundary_thresh, const int32_t* image_sizes, int32_t* matched,
                          int8_t* labels, float* gtmax, void* stream);
/* ROI version: boxes [B,P,4] with count; one threshold; writes the class target:
 * cls[b][p] = gt_classes[matched] if IoU>=thr else num_classes; -2 for p >= count. */
int sfod_roi_match(const float* boxes, const int32_t* box_count, int B, int P,
                   const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_count,
                   int Gcap, float thr, int num_classes, int32_t* matched, int32_t* cls,
                   void* stream);
/* General form: d2 Matcher with thresholds [lo, hi] / labels [0, -1, 1] followed by _sample_proposals' class targets:
 *   cls[b][p] = best >= hi ? gt_classes[matched] : (best >= lo ? -1 : num_classes),   best = max IoU over the image's GT;
 * -2 for p >= count; an image without ground truth stays all num_classes.  lo, hi finite, lo <= hi (else SFOD_EBADARG).
 * sfod_subsample mode 1 never samples a -1.  sfod_roi_match is this call with lo == hi == thr ([thr] / [0, 1]). */
int sfod_roi_match_opt(const float* boxes, const int32_t* box_count, int B, int P,
                       const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_count,
                       int Gcap, float lo, float hi, int num_classes, int32_t* matched, int32_t* cls,
                       void* stream);
/* ---- K10: subsample_labels (Appendix A.9).  The random choice is an INPUT: one uint32 key per
 * element; the sample is the n candidates with the smallest (key, index).
 * mode 0 (RPN, _subsample_labels): labels int8 in/out [B,n]: positives = 1, negatives = 0,
 *   everything not sampled becomes -1.
 * mode 1 (ROI, _sample_proposals): cls int32 [B,n] in; out_idx int32 [B,num] = sampled fg indices
 *   ascending then bg ascending, out_count [B]. */
int sfod_subsample(void* labels_or_cls, const uint32_t* keys, int B, int n, int num, float pos_frac,
                   int bg_label, int mode, int32_t* out_idx, int32_t* out_count, void* stream);
/* The same with the positive quota given as a count.  d2 evaluates int(num * positive_fraction) in double; the fp32 product of
 * the fraction rounded to fp32, which sfod_subsample takes, is one less for some pairs (300 * 0.21: 63 against 62), so a caller
 * that holds the configured fraction computes the count itself.  0 <= pos_quota <= num, else SFOD_EBADARG.  sfod_subsample is
 * this call with pos_quota = (int)((float)num * pos_frac); it refuses a pos_frac outside [0, 1] (NaN included). */
int sfod_subsample_quota(void* labels_or_cls, const uint32_t* keys, int B, int n, int num, int pos_quota,
                         int bg_label, int mode, int32_t* out_idx, int32_t* out_count, void* stream);

/* ---- K11: RPN losses (Appendix A.10; rpn.py:46-49).  loss[0]=loss_rpn_cls, loss[1]=
 * loss_rpn_loc, both / (batch_per_image*B).  With grad_scale != NULL (device fp32 [2], the
 * upstream d(total)/d(loss_k)) also writes d_rpn_out (same layout as rpn_out, dense). */
int sfod_rpn_loss(const float* rpn_out, int ld, const float* cell_anchors, int A, int B, int Hf,
                  int Wf, int stride, const int8_t* labels, const int32_t* matched,
                  const float* gt_boxes, const int32_t* gt_count, int Gcap, int batch_per_image,
                  float* loss, const float* grad_scale, float* d_rpn_out, float* ws, void* stream);
/* ---- Box-regression options (d2 _dense_box_regression_loss / FastRCNNOutputLayers.box_reg_loss, fvcore
 * smooth_l1_loss / giou_loss).  The `_opt` entry points below take, by value:
 *   wx, wy, ww, wh  Box2BoxTransform weights (BBOX_REG_WEIGHTS); finite and > 0.
 *   loss_type       0 smooth-L1, 1 GIoU (BBOX_REG_LOSS_TYPE); anything else: SFOD_EBADARG.
 *   beta            SMOOTH_L1_BETA, finite and >= 0; read by loss_type 0 only.
 *   cls_agnostic    (ROI head) CLS_AGNOSTIC_BBOX_REG: the prediction row is [0,K] scores, [K+1,K+5) ONE delta
 *                   quadruple shared by all classes (ld >= K + 5) instead of [K+1, K+1+4K) (ld >= 5K + 1).
 * Per positive anchor / foreground row, with src the anchor / proposal, g the matched ground truth, d the deltas:
 *   smooth-L1: t = get_deltas(src, g; weights), n = |d - t| per component.  beta < 1e-5: sum n, gradient sign(d - t)
 *              (the L1 the default entry points compute); otherwise sum (n < beta ? 0.5 n^2 / beta : n - 0.5 beta),
 *              gradient (d - t) / beta inside the quadratic zone, sign(d - t) outside.
 *   GIoU:      p = apply_deltas(d, src; weights) with SCALE_CLAMP on dw / dh, not clipped to the image; eps = 1e-7;
 *              I = overlap area (0 unless both extents > 0), U = area(p) + area(g) - I, C = enclosing area;
 *              term = 1 - I / (U + eps) + (C - U) / (C + eps).  The gradient goes through apply_deltas and is exactly 0
 *              for a dw / dh ABOVE the clamp (equal to it: passes, as torch.clamp).  At an exact tie of a max / min
 *              between a predicted and a ground-truth coordinate the kernel takes the ground-truth side: the tied term
 *              contributes no gradient (torch's autograd would give each side half).
 * Normalisers are the default forms' (RPN: 1 / (batch_per_image * B); ROI: 1 / max(n_valid, 1)); value and gradient stay
 * fused in one launch + the partial sum; no float atomics, bit-identical from run to run.  The default entry points are
 * these calls with weights (1,1,1,1) / (10,10,5,5), loss_type 0, beta 0, cls_agnostic 0: one kernel body each, and --
 * this file being built without fast-math and with -ffp-contract=off -- bit-identical to the literal-weight kernels. */
int sfod_rpn_loss_opt(const float* rpn_out, int ld, const float* cell_anchors, int A, int B, int Hf,
                      int Wf, int stride, const int8_t* labels, const int32_t* matched,
                      const float* gt_boxes, const int32_t* gt_count, int Gcap, int batch_per_image,
                      float* loss, const float* grad_scale, float* d_rpn_out, float* ws, float wx, float wy,
                      float ww, float wh, int loss_type, float beta, void* stream);
/* sfod_rpn_loss_opt with the anchor `shift` (Proposal and matcher options, above); sfod_rpn_loss_opt is this call with 0. */
int sfod_rpn_loss_shift(const float* rpn_out, int ld, const float* cell_anchors, int A, int B, int Hf,
                        int Wf, int stride, const int8_t* labels, const int32_t* matched,
                        const float* gt_boxes, const int32_t* gt_count, int Gcap, int batch_per_image,
                        float* loss, const float* grad_scale, float* d_rpn_out, float* ws, float wx, float wy,
                        float ww, float wh, int loss_type, float beta, float shift, void* stream);

/* concat proposals and GT boxes: d2 add_ground_truth_to_proposals (roi_heads.py:170) */
int sfod_append_gt(const float* props, const int32_t* prop_count, int B, int P,
                   const float* gt_boxes, const int32_t* gt_count, int Gcap, float* out_boxes,
                   int32_t* out_count, void* stream);
/* build the sampled ROI batch: rois [B*S,5], gt_cls int32 [B*S] (-1 on padding rows),
 * gt_box [B*S,4]; n_valid int32[1] = number of real rows in the whole batch. */
int sfod_roi_build_samples(const float* boxes, const int32_t* cls, const int32_t* matched,
                           const int32_t* samp_idx, const int32_t* samp_count, int B, int P, int S,
                           const float* gt_boxes, const int32_t* gt_count, int Gcap, float* rois,
                           int32_t* gt_cls, float* gt_box, int32_t* n_valid, void* stream);
/* rois [B*P,5] from per-image proposal arrays (padding rows get batch index -1) */
int sfod_make_rois(const float* props, const int32_t* prop_count, int B, int P, float* rois,
                   void* stream);

/* ---- K13: ROIAlign (tv roi_align; Appendix A.11) on NHWC features.  out: [R, PH*PW, C] (dt).  rois with batch index < 0 are
 * padding rows: the forward writes zeros for them, the backward ignores them.  pooled in [1, 16], both directions.
 * Definition (oracle/pointwise_definitions.py roi_align_matrices, with the options tests/helpers/roi_pooler_definitions.py;
 * held per element by tests/test_gpu_roi_definition.py and tests/test_gpu_roi_pooler_options.py, in fp32, bf16 and on the
 * exact values of operand pairs): out[r, ph, pw, c] = sum_{py, px} Ay[r, ph, py] Ax[r, pw, px] feat[b_r, py, px, c] / count_r,
 * Ay / Ax the bilinear weights of the bin's grid_h / grid_w sample rows / columns, sample i of bin p at
 * start + p * bin + (i + .5) * bin / grid with bin = roi_len / pooled, count = max(grid_h grid_w, 1), the coordinates in fp32
 * as torchvision writes them, a sample outside [-1, H] x [-1, W] dropped.
 *   aligned = 1 (d2 "ROIAlignV2"): start = coord * scale - 0.5, roi_len = end - start (a zero-sized ROI has grid 0 and gives zeros)
 *   aligned = 0 (d2 "ROIAlign"):   start = coord * scale,       roi_len = max(end - start, 1)
 *   sampling_ratio = 0: grid = ceil(roi_len / pooled) per ROI and axis;  sampling_ratio in [1, 16]: grid_h = grid_w = sampling_ratio
 *     (a fixed grid samples an inverted ROI, end < start under aligned = 1, with its negative bin, like torchvision; both directions do)
 * sfod_roi_align_fwd is sfod_roi_align_fwd_opt with (sampling_ratio, aligned) = (0, 1), likewise the backward. */
int sfod_roi_align_fwd(const void* feat, int B, int H, int W, int C, const float* rois, int R,
                       int pooled, float scale, void* out, int dt, void* stream);
int sfod_roi_align_fwd_opt(const void* feat, int B, int H, int W, int C, const float* rois, int R,
                           int pooled, float scale, int sampling_ratio, int aligned, void* out, int dt, void* stream);
/* dfeat fp32 [B,H,W,C] += adjoint of the forward above (zero-init by the caller, or an earlier gradient to add to).
 * Tiled gather for every pooled size: one owner per gradient element, ROIs summed in ROI order, no float atomics
 * (bit-reproducible).  SFOD_ROI_BWD_ATOMIC=1 (read at load; an A/B switch) selects, for pooled <= 8, one workgroup per ROI
 * with one float atomic per footprint pixel and channel. */
int sfod_roi_align_bwd(const void* dout, int B, int H, int W, int C, const float* rois, int R,
                       int pooled, float scale, float* dfeat, int dt, void* stream);
int sfod_roi_align_bwd_opt(const void* dout, int B, int H, int W, int C, const float* rois, int R,
                           int pooled, float scale, int sampling_ratio, int aligned, float* dfeat, int dt, void* stream);

/* ---- K15: Fast R-CNN losses (Appendix A.12; roi_heads.py:124).  pred: fp32 [R, ld]: cols
 * [0,K] class scores, cols [K+1, K+1+4K) deltas.  loss[0]=loss_cls, loss[1]=loss_box_reg. */
int sfod_frcnn_loss(const float* pred, int ld, int R, int K, const float* rois,
                    const int32_t* gt_cls, const float* gt_box, const int32_t* n_valid,
                    float* loss, const float* grad_scale, float* d_pred, float* ws, void* stream);
/* General form (options: see sfod_rpn_loss_opt).  cls_agnostic: the loss takes the row's single delta quadruple for every
 * foreground row, whatever its class; rows that are not foreground get no box gradient. */
int sfod_frcnn_loss_opt(const float* pred, int ld, int R, int K, const float* rois,
                        const int32_t* gt_cls, const float* gt_box, const int32_t* n_valid,
                        float* loss, const float* grad_scale, float* d_pred, float* ws, float wx, float wy,
                        float ww, float wh, int loss_type, float beta, int cls_agnostic, void* stream);
/* Most general form: the box options above plus the classification loss (MODEL.ROI_HEADS.LOSS,
 * MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE; definitions restated in tests/helpers/cls_loss_definitions.py).  Per live row r
 * (gt_cls[r] = c >= 0), N = n_valid[0], g = grad_scale[0]:
 *   cls_mode 0  cross-entropy: CE_r = logsumexp(z[0..K]) - z_c; loss[0] = sum CE / N.  What the two entry points above run.
 *   cls_mode 1  focal (Unbiased Teacher's FastRCNNFocalLoss): p = exp(-CE), q = 1 - p taken as -expm1(-CE);
 *               loss[0] = sum q^gamma CE / N; d/dz_j = A (softmax_j - [j == c]) g / N with
 *               A = q^gamma (1 + gamma p CE / q), CE / q := 1 at q == 0.  gamma 0 is the cross-entropy (0^0 = 1).
 *   cls_mode 2  sigmoid cross-entropy (d2 USE_SIGMOID_CE): target t = one-hot of c over K + 1 columns without the last, so a
 *               background row has the all-zero target; loss[0] = sum_r sum_{j < K} (max(z_j, 0) - z_j t_j + log1p(exp(-|z_j|))) / N;
 *               d/dz_j = (sigmoid(z_j) - t_j) g / N for j < K, the background column gets no gradient.
 * Modes 1 and 2 form the row's scalars in double and round every gradient element once to fp32; the loss terms stay in
 * double through the per-block partial and the final sum, so loss[0] is the fp32 rounding of its definition.  Both are
 * finite for every gamma >= 0 at both ends of p; a NaN or +inf score gives a NaN loss, as in mode 0.  ws: 2 * ceil(R / 256)
 * floats in mode 0 (as above), 3 * ceil(R / 256) in modes 1 and 2 (the class partial of a block is a pair of floats).
 * gamma (read by mode 1 only) must be finite and >= 0 in every mode.  The box half (loss[1], the delta columns of d_pred)
 * does not depend on cls_mode.  One owner per gradient element, no float atomics; padding rows and padding columns of
 * d_pred are zero. */
int sfod_frcnn_loss_cls(const float* pred, int ld, int R, int K, const float* rois,
                        const int32_t* gt_cls, const float* gt_box, const int32_t* n_valid,
                        float* loss, const float* grad_scale, float* d_pred, float* ws, float wx, float wy,
                        float ww, float wh, int loss_type, float beta, int cls_agnostic, int cls_mode, float gamma,
                        void* stream);

/* ---- Domain losses of DA Faster R-CNN (daod/modeling/meta_arch/da_faster_rcnn.py:228-272; csrc/da_losses.hip).  Logits
 * are fp32 columns of a padded matrix: element i at z[i * ld] (the one-channel GEMM output under ldy = 8).  Gradients come
 * back dense with the same ld, the padding columns zero.  grad_scale: device fp32 [1], the upstream d(total)/d(loss) (the
 * sfod_rpn_loss convention).  No float atomics: every sum has one owner and a fixed order.
 *
 * sfod_da_bce: loss[0] = mean over the live rows of max(z, 0) - z * label + log1p(exp(-|z|)), loss[1] = the live count.
 * rois ([n, 5], may be NULL): row i is padding (not live) when rois[5 i] < 0.  With grad_scale also
 * dz[i * ld] = (sigmoid(z) - label) * g / n_live for live rows, 0 for the rest.  No live row: loss 0, gradient 0.
 * ws: 2 * ceil(n / 256) floats. */
int sfod_da_bce(const float* z, int64_t n, int ld, const float* rois, float label, float* loss,
                const float* grad_scale, float* dz, float* ws, void* stream);
/* sfod_da_consistency_fwd: z_img [B, H, W] with pixel stride ld, z_ins [R] with row stride ld_ins, rois [R, 5] (batch index
 * < 0: padding).  Per live ROI p_img[r] = the mean over all pooled x pooled bins of ROIAlign (K13's definition, with its
 * scale / sampling_ratio / aligned) applied to sigmoid(z_img); p_ins = sigmoid(z_ins[r]); loss[0] = mean over the live
 * ROIs of |p_img - p_ins|, loss[1] = the live count.  Kept for the backward: sgn[r] = sign(p_img - p_ins) (0 at a tie and
 * for padding), wts [R, H + W] = the ROI's separable pixel weights (Ay / (count pooled^2) | Ax); term [R] is scratch.
 * No live ROI: loss 0 (torch's l1_loss of an empty tensor is NaN). */
int sfod_da_consistency_fwd(const float* z_img, int B, int H, int W, int ld, const float* z_ins, int ld_ins,
                            const float* rois, int R, int pooled, float scale, int sampling_ratio, int aligned,
                            float* loss, float* p_img, float* sgn, float* term, float* wts, void* stream);
/* dz_ins[r * ld_ins] = -sgn_r * g / n_live * p_ins (1 - p_ins); dz_img[b, y, x] = sigmoid'(z_img) * g / n_live *
 * sum over the image's ROIs of sgn_r * Ay_r[y] * Ax_r[x] (one owner per pixel; 16 contiguous parts of the ROI rows, each summed in
 * ROI order, added in part order).  loss / sgn / wts: the forward's. */
int sfod_da_consistency_bwd(const float* z_img, int B, int H, int W, int ld, const float* z_ins, int ld_ins,
                            const float* rois, int R, const float* loss, const float* sgn, const float* wts,
                            const float* grad_scale, float* dz_img, float* dz_ins, void* stream);

/* ---- Class conditioning of conditional DA Faster R-CNN (daod/modeling/meta_arch/cda_faster_rcnn.py:22-33, 263-283;
 * csrc/cda_condition.hip).  f [R, D]: the box features in storage type f_dt (any of the four), decoded to fp32.  scores: fp32,
 * row r at scores + r * ld, C live columns (ld >= C).  rois [R, 5]: row r is padding when rois[5 r] < 0.  Per live row:
 *   p = softmax(scores) (the maximum subtracted),
 *   w = 1 + exp(sum_c p_c * log(p_c + 1e-5)) when entropy is 1 (the reference's entropy(): its fp32 1e-5 inside the log), else 1,
 *   x[r, c * D + d] = p[r, c] * f[r, d]      (bmm(g.unsqueeze(2), f.unsqueeze(1)).view(R, -1)).
 * The row's C scalars are formed in double (they cost nothing beside the C * D stores) and the product is rounded once to
 * fp32 and from there to x's storage type, so x is that type's rounding of the exact product to double's precision; p and w
 * come back as the fp32 roundings.
 * x [R, C * D] is written in storage type x_dt, the operand of the product that follows; x_grad_operand (may be NULL; x_dt
 * SFOD_F16X3 only): the same values once more as SFOD_BF16X3 pairs, the weight gradient's operand (the convention of
 * sfod_group_norm_relu_fwd); a value beyond half's range is clamped and reported through sfod_f16x3_poll.  p [R, C] and
 * w [R]: fp32, kept for the backward and the weighted loss.  A padding row gives zeros in x, p and w whatever its scores
 * hold.  D a multiple of 8, 2 <= C <= 4096 (the row's probabilities sit in LDS); R == 0: no launch. */
int sfod_cda_condition_fwd(const void* f, int f_dt, const float* scores, int ld, const float* rois, int R, int D, int C,
                           int entropy, void* x, int x_dt, void* x_grad_operand, float* p, float* w, void* stream);
/* df[r, d] = sum over c (ascending) of p[r, c] * dx[r, c * D + d], fused multiply-adds in double, rounded once to fp32 and
 * from there to df's type; one owner per element; 0 for a
 * padding row.  dx and df: dt SFOD_F32 or SFOD_BF16 (what the data-gradient product writes).  The condition is detached in
 * the reference: there is no gradient to the scores. */
int sfod_cda_condition_bwd(const void* dx, int dt, const float* p, const float* rois, int R, int D, int C, void* df,
                           void* stream);
/* sfod_da_bce with a weight per row (weight [n] fp32; rois may be NULL): loss[0] = sum_live w_i * bce_i / sum_live w_i (the
 * reference's weight / weight.mean() followed by the mean), loss[1] = the live count, and with grad_scale
 * dz[i * ld] = g * (w_i / sum_live w) * (sigmoid(z_i) - label) for live rows, 0 for the rest.  No live row, or live weights
 * that sum to 0: loss 0, gradient 0.  ws: sfod_da_bce_weighted_ws_floats(n) floats.  n < 2^24. */
int64_t sfod_da_bce_weighted_ws_floats(int64_t n);
int sfod_da_bce_weighted(const float* z, int64_t n, int ld, const float* rois, const float* weight, float label, float* loss,
                         const float* grad_scale, float* dz, float* ws, void* stream);

/* ---- K16: teacher inference post-processing (Appendix A.13; roi_heads.py:161) ----
 * step 1: softmax + per-class decode + clip + score filter -> candidates [B, P*K]
 *         (cand_scores = -1 for filtered entries), cand_count[b] = number passing. */
int sfod_frcnn_candidates(const float* pred, int ld, int B, int P, int K, const float* props,
                          const int32_t* prop_count, const int32_t* image_sizes,
                          float score_thresh, float* cand_boxes, float* cand_scores,
                          int32_t* cand_count, void* stream);
/* General form: transform weights by value; cls_agnostic: every class of a row decodes the same four deltas (the
 * candidates stay [B, P*K]: K identical boxes with the K class scores). */
int sfod_frcnn_candidates_opt(const float* pred, int ld, int B, int P, int K, const float* props,
                              const int32_t* prop_count, const int32_t* image_sizes,
                              float score_thresh, float* cand_boxes, float* cand_scores,
                              int32_t* cand_count, float wx, float wy, float ww, float wh, int cls_agnostic,
                              void* stream);
/* Most general form: cls_mode as in sfod_frcnn_loss_cls, here naming the row's class probabilities: 0 / 1 the row softmax
 * (the operation order above), 2 the sigmoid 1 / (1 + exp(-z)) of each of the K + 1 scores (the finite test covers all K + 1;
 * the last column is dropped as before).  One device function serves this kernel, sfod_predict_probs_cls and
 * sfod_bpc_loss_cls.  The three take the class options as the loss does, cls_mode and gamma by value: gamma must be
 * finite and >= 0 and no probability depends on it. */
int sfod_frcnn_candidates_cls(const float* pred, int ld, int B, int P, int K, const float* props,
                              const int32_t* prop_count, const int32_t* image_sizes,
                              float score_thresh, float* cand_boxes, float* cand_scores,
                              int32_t* cand_count, float wx, float wy, float ww, float wh, int cls_agnostic,
                              int cls_mode, float gamma, void* stream);
/* d2 FastRCNNOutputLayers.predict_probs (reached from daod/modeling/roi_heads/source_free_fast_rcnn.py:16-17): row
 * softmax of scores [R, ld] (K+1 class scores per row) -> probs [R, K+1], in step 1's operation order. */
int sfod_predict_probs(const float* scores, int ld, int R, int K, float* probs, void* stream);
/* General form: cls_mode 0 / 1 the row softmax, 2 the per-score sigmoid (sfod_frcnn_candidates_cls). */
int sfod_predict_probs_cls(const float* scores, int ld, int R, int K, int cls_mode, float gamma, float* probs,
                           void* stream);
/* step 2 (after sorting scores): gather sorted candidates, classes, coordinate-offset boxes
 * and the torchvision strategy flag (mode[b]=1: coordinate trick, 0: per-class). */
int sfod_frcnn_prepare_nms(const float* cand_boxes, const float* sorted_scores,
                           const int32_t* sorted_idx, const int32_t* cand_count, int B, int n,
                           int K, int numel_limit, float* s_boxes, float* s_alt_boxes,
                           int32_t* s_classes, int32_t* mode, float* maxcoord_ws, void* stream);
/* step 3 (after NMS): top-`max_det` detections + the pseudo-label filter score > thr
 * (daod/engine/trainers/source_free_adaptive_teacher.py:167-181, strict '>'). */
int sfod_frcnn_finalize(const float* s_boxes, const float* sorted_scores, const int32_t* s_classes,
                        const int32_t* keep_idx, const int32_t* keep_count, int B, int n,
                        int max_det, float pseudo_thr, float* det_boxes, float* det_scores,
                        int32_t* det_classes, int32_t* det_count, float* gt_boxes,
                        int32_t* gt_classes, int32_t* gt_count, void* stream);

/* ---- TEST.AUG: the box merge of test-time augmentation (d2 GeneralizedRCNNWithTTA: _get_augmented_boxes and the entry of
 * _merge_detections -> fast_rcnn_inference_single_image), one launch per batch of images, nothing read back ----
 * Reads the det_* containers of sfod_frcnn_finalize for B images x A augmentations: det_boxes [B,A,cap,4] fp32 at the
 * augmented pass's size, det_scores [B,A,cap], det_classes [B,A,cap] i32, det_count [B,A] (clamped to 0..cap; a slot at or
 * beyond the count is never read).  aug_table [B,A,8] fp32 = (w_a, h_a, flip != 0, w / w_a, h / h_a, W0 / w, H0 / h, unused):
 * the augmented tensor's size, whether it was mirrored, and the two ratio pairs, each the double quotient rounded to fp32
 * once.  image_sizes [B,2] i32 = (H0, W0), the frame the detections go back to.  Per live slot, in fp32 without contraction:
 *   1. the inverse transforms in reverse order, each on the corners with min / max as d2's Transform.apply_box does:
 *      x -> w_a - x when mirrored; (x, y) * (w / w_a, h / h_a); (x, y) * (W0 / w, H0 / h) -- two separate multiplications;
 *   2. dropped when a coordinate (before or after 1.) or the score is not finite, or the class is outside [0, K);
 *   3. clipped to [0, W0] x [0, H0];  4. kept when score > score_thresh (strict).
 * Writes the COMPACT candidates in concatenation order (augmentation, then slot): cand_boxes [B,A*cap,4], cand_scores
 * [B,A*cap] (-1 for a slot that is dead or dropped, box and class 0), cand_classes [B,A*cap] i32, cand_count [B] = the number
 * kept (a workgroup sum in fixed order; no atomics).  After sfod_segmented_sort_desc on cand_scores the chain continues with
 * sfod_frcnn_prepare_nms_cls -> sfod_nms -> sfod_frcnn_finalize.  SFOD_EBADARG before any launch: a NULL pointer, B outside
 * 1..65535, A outside 1..64, cap < 1, A * cap > 4096, K < 1, a non-finite score_thresh. */
int sfod_tta_merge(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                   const int32_t* det_count, const float* aug_table, const int32_t* image_sizes, int B, int A, int cap,
                   int K, float score_thresh, float* cand_boxes, float* cand_scores, int32_t* cand_classes,
                   int32_t* cand_count, void* stream);
/* sfod_frcnn_prepare_nms for compact candidates: the class of a candidate is cand_classes [B,n] at its index, not
 * index % K.  One kernel pair serves both forms.  SFOD_EBADARG before any launch: a NULL pointer, B outside 1..65535, n < 1. */
int sfod_frcnn_prepare_nms_cls(const float* cand_boxes, const int32_t* cand_classes, const int32_t* sorted_idx,
                               const int32_t* cand_count, int B, int n, int numel_limit, float* s_boxes,
                               float* s_alt_boxes, int32_t* s_classes, int32_t* mode, float* maxcoord_ws, void* stream);

/* BPC calibration metric of the student's training pass (SURVEY 8a row a6 + 8f rank 4), logged as
 * calibration/bpc_loss and weighted by 0 (source_free_adaptive_teacher.py:549-550,566).  Fuses
 * SourceFreeFastRCNNOutputLayers.convert_bbox_scores (daod/modeling/roi_heads/source_free_fast_rcnn.py:15-36,
 * 82-147: softmax, per-class decode, non-finite rows dropped, clip, score > 0, no NMS) applied -- as the
 * reference does -- to the sampled proposals AFTER their boxes were overwritten by
 * predict_boxes_for_gt_classes (source_free_adaptive_teacher_roi_heads.py:136-143), with bpc_loss
 * (daod/loss/bpc_loss.py:10-262) against the images' (pseudo) ground truth.
 * pred [R,ld] fp32 = (K+1 logits | 4K deltas) per sampled row; rois [R,5] (image, x1,y1,x2,y2; image < 0:
 * padding row); roi_cls [R] the rows' gt classes (K = background); image_sizes [B,2] (h,w);
 * gt_boxes [B,G,4], gt_classes [B,G], gt_count [B].  ws: B*4 doubles.  loss: 1 float. */
int sfod_bpc_loss(const float* pred, int ld, int R, int K, const float* rois, const int32_t* roi_cls,
                  int B, const int32_t* image_sizes, const float* gt_boxes, const int32_t* gt_classes,
                  const int32_t* gt_count, int G, float iou_thresh, float* loss, void* ws, void* stream);
/* General form: transform weights by value; cls_agnostic: the gt-class decode and the K per-class decodes all read the
 * row's single delta quadruple. */
int sfod_bpc_loss_opt(const float* pred, int ld, int R, int K, const float* rois, const int32_t* roi_cls,
                      int B, const int32_t* image_sizes, const float* gt_boxes, const int32_t* gt_classes,
                      const int32_t* gt_count, int G, float iou_thresh, float* loss, void* ws, float wx, float wy,
                      float ww, float wh, int cls_agnostic, void* stream);
/* Most general form: cls_mode 0 / 1 scores by the row softmax, 2 by the per-score sigmoid (sfod_frcnn_candidates_cls). */
int sfod_bpc_loss_cls(const float* pred, int ld, int R, int K, const float* rois, const int32_t* roi_cls,
                      int B, const int32_t* image_sizes, const float* gt_boxes, const int32_t* gt_classes,
                      const int32_t* gt_count, int G, float iou_thresh, float* loss, void* ws, float wx, float wy,
                      float ww, float wh, int cls_agnostic, int cls_mode, float gamma, void* stream);

/* F1Evaluator (daod/evaluation/f1_evaluator.py:8-230, appended to every trainer's evaluator list, base.py:149): per image
 * and class the counts TP / FP / FN that its F1 score is made of, one wavefront per image, nothing read back.
 *   1. detector_postprocess to the loader's scale: box * (sx, sy, sx, sy) in fp32, clip to [0, w] x [0, h], keep width > 0
 *      and height > 0;  2. keep score >= `score` (fp32);  3. keep the `top_n` highest scores over all classes together
 *      (equal scores: the later index ranks first);  4. detection coordinates truncated toward zero to integers, ground
 *      truth stays fp32;  5. IoU with the "+1" pixel convention over (ground truth, kept detection) pairs of equal class:
 *      ground-truth area in fp32, detection area in int32, intersection extents max(0, min - max + 1) and the quotient
 *      inter / (ga + da - inter) in fp64, no contraction;  6. greedy matching: while the matrix maximum is > `iou` (strict,
 *      fp64) its FIRST position in row-major order (rows: ground truths by index; columns: kept detections by descending
 *      score) is matched and its row and column leave;  7. class k in [0, K): TP = matched ground truths, FP = kept
 *      detections not matched, FN = ground truths not matched; other classes are counted nowhere.
 * det_boxes [B,D,4] fp32 (x1,y1,x2,y2 at the model's output size), det_scores [B,D], det_classes [B,D] i32, det_count [B];
 * gt_boxes [B,G,4], gt_classes [B,G], gt_count [B] (at the loader's size); counts above D / G are clamped, entries beyond
 * the counts are never read.  scale [B,2] fp32 (sx, sy), clip_size [B,2] i32 (h, w).  D, G <= 100, 1 <= top_n <= D,
 * 1 <= K <= 32, iou finite and >= 0.  counts [B,K,3] i32 (TP, FP, FN): every element is written. */
int sfod_f1_count(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                  const int32_t* det_count, const float* gt_boxes, const int32_t* gt_classes,
                  const int32_t* gt_count, const float* scale, const int32_t* clip_size, int B, int D, int G, int K,
                  double iou, int top_n, float score, int32_t* counts, void* stream);

/* COCOeval's per-image matching (pycocotools computeIoU + evaluateImg for boxes, as evaluation.py::COCOevalBBox.evaluate /
 * _evaluate_img state it -- that code is the definition), one launch per batch, one wavefront per image, nothing read back.
 * Only detections and ground truths of equal category in [0, K) meet.
 *   det_boxes [B,D,4] fp32 XYXY as the model returned them, det_scores [B,D] fp32, det_classes [B,D] i32, det_count [B];
 *   gt_boxes [B,G,4] f64 XYWH, gt_area [B,G] f64 (the annotation's own field, need not be w * h), gt_classes [B,G] i32,
 *   gt_iscrowd [B,G] i32, gt_count [B].  Counts above D / G are clamped, entries beyond the counts are never read.
 *   iou_thrs [T] and area_rng [A][2] = (lo, hi) are HOST arrays of doubles (they must be readable by the calling thread: the
 *   entry point validates and copies them before it returns); they travel in the launch arguments by value and
 *   are never recomputed on the device.
 *   1. order: inside one (image, category) descending score, stable (equal scores keep index order, a NaN score ranks behind
 *      every number, as numpy's mergesort of -score leaves it).  rank [B,D] i32 = the position in that order; -1 for a slot
 *      beyond the count or a class outside [0, K) (its match / ignore words are 0).
 *   2. detection w = x2 - x1, h = y2 - y1 in fp32; everything after that in fp64 without contraction, IEEE division.
 *   3. IoU: extents min(dx + dw, gx + gw) - max(dx, gx) and the same in y; 0 when either is <= 0; otherwise
 *      inter / ((da + ga) - inter), for a crowd ground truth inter / da, with da = dw * dh and ga = gw * gh.
 *   4. per area range a a ground truth is ignored when it is crowd or gt_area < lo or gt_area > hi; ground truths are visited
 *      not-ignored first, each group in annotation order.
 *   5. per threshold t the greedy loop: start from iou = min(t, 1 - 1e-10); skip a ground truth already matched and not
 *      crowd; stop when a not-ignored match is held and the next ground truth is ignored; skip when its IoU < iou (equality
 *      passes: on equal IoU the later-visited one replaces the earlier); otherwise it becomes the match and iou its IoU.
 *   6. bit a * T + t of match [B,D] u64: the detection matched.  The same bit of ignore [B,D] u64: it matched an ignored
 *      ground truth, or it is unmatched and dw * dh < lo or > hi.
 *   7. npig [B,K,A] i32: the ground truths of class k that are not ignored in area range a.
 * Every output element is written; plain vector stores, no atomics.  SFOD_EBADARG before any launch, outputs untouched: a NULL
 * pointer, A < 1, T < 1, A * T > 64, D outside 1..100, G outside 1..256, K < 1, a non-finite threshold or range.
 * B == 0 is a valid call that launches nothing. */
int sfod_coco_match(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                    const int32_t* det_count, const double* gt_boxes, const double* gt_area, const int32_t* gt_classes,
                    const int32_t* gt_iscrowd, const int32_t* gt_count, int B, int D, int G, int K, const double* iou_thrs,
                    int T, const double* area_rng, int A, int32_t* rank, uint64_t* match, uint64_t* ignore, int32_t* npig,
                    void* stream);

/* Class-wise adaptive pseudo-label threshold: AdaptiveConfidenceBasedSelfTrainingLoss
 * (daod/modeling/adaptive_thresh/adaptive_confidence.py:6-34, "convex" curve) with the trainer's bookkeeping
 * (daod/engine/trainers/source_free_adaptive_teacher.py:282-295 count_label_prediction, :297-309
 * update_adaptive_threshold, :393-404 per-step update, :461-466 selection).  Over the det_* arrays of
 * sfod_frcnn_finalize [B,max_det]: writes the per-class counts of score > thr into reserve[row] ([R][K] fp32
 * ring, caller-owned state), class_acc[K] = counter / max(max(counter), 1) with classes 0 and 2 excluded from
 * the counter and pinned to 1, and, when `select` != 0, replaces the pseudo ground truth of every image by the
 * stable subset score >= thr * (acc[c] / (2 - acc[c])) (gt_boxes/gt_classes/gt_scores [B,max_det], gt_count [B]).
 * K <= 64. */
int sfod_adaptive_pseudo_labels(const float* det_boxes, const float* det_scores,
                                const int32_t* det_classes, const int32_t* det_count, int B,
                                int max_det, int K, float thr, float* reserve, int R, int row,
                                float* class_acc, int select, float* gt_boxes, int32_t* gt_classes,
                                float* gt_scores, int32_t* gt_count, void* stream);

/* ---- Strong augmentation on the device: build_strong_augmentation
 * (daod/data/detection_utils.py:7-36) as applied by DatasetMapperTwoCropSeparate
 * (daod/data/mappers/two_crop_augmentation_mapper.py:141-146), on planar uint8 [3][H][W] frames; bit-exact
 * with the torchvision-on-Pillow path (channels in stored order, as the reference hands its BGR array to
 * Pillow as "RGB").
 * sfod_aug_color: a sequence of <= 8 point operations: 0 brightness, 1 contrast (at most one per call), 2
 * saturation (Pillow ImageEnhance = Image.blend with black / the mean-luma level / the luma image; factor =
 * blend alpha), 3 hue (Pillow HSV round trip; the factor slot carries the wrapped uint8 shift
 * np.uint8(hue_factor * 255)), 4 grayscale (convert("L") replicated; factor ignored).  codes / factors are HOST
 * arrays.  ws: 8 bytes of device memory (the contrast op's luma sum).  in may equal out.
 * sfod_aug_gaussian_blur: ImageFilter.GaussianBlur(radius=sigma) (daod/data/transforms/augmentations.py:6-21):
 * Pillow's three extended-box passes along x then along y; in, out, tmp distinct, C*H*W bytes each.
 * sfod_aug_erase: RandomErasing(value="random") followed by ToPILImage: rectangle (i, j, h, w) of every channel
 * is overwritten by (uint8)(noise * 255) (truncation, low 8 bits); noise [C][h][w] fp32 on the device. */
int sfod_aug_color(const uint8_t* in, uint8_t* out, int H, int W, int n_ops, const int32_t* codes,
                   const float* factors, void* ws, void* stream);
int sfod_aug_gaussian_blur(const uint8_t* in, uint8_t* out, uint8_t* tmp, int C, int H, int W, float sigma,
                           void* stream);
int sfod_aug_erase(uint8_t* img, int C, int H, int W, int i, int j, int h, int w, const float* noise,
                   void* stream);

/* ---- K20/K21: fused SGD(momentum, weight decay) + EMA teacher update over flat fp32 arrays.
 * d2 build_optimizer + torch SGD (Appendix A.15) and _update_teacher_model
 * (source_free_adaptive_teacher.py:583-603).  lr is a device scalar (no host sync on schedule).
 * first_step: momentum buffer is initialised to the gradient (torch SGD semantics).
 * teacher may be NULL (no EMA).
 * ema_one_minus_keep: the caller's (1 - k) computed in double and rounded once (the reference multiplies by the python
 * float 1 - keep_rate); the kernels use two rounded products and a rounded sum like torch's op chain, so the teacher
 * is bit-identical to _update_teacher_model's (tests/golden/glue_ref.npz). */
int sfod_sgd_ema(float* param, const float* grad, float* mom, float* teacher, int64_t n,
                 const float* lr, float momentum, float weight_decay, float grad_scale,
                 float ema_keep, float ema_one_minus_keep, int first_step, void* stream);
/* ---- Solver options on the flat buffers (Detectron2 SOLVER.CLIP_GRADIENTS / NESTEROV / BIAS_LR_FACTOR /
 * WEIGHT_DECAY_BIAS): a SEGMENT TABLE describes the parameter tensors inside the flat arrays.  All tables are DEVICE
 * arrays of nseg entries:
 *   seg_off  int64  first element of the segment; ascending, a multiple of 4 (16-byte lanes never straddle two segments)
 *   seg_len  int64  number of elements, any value >= 0; seg_off[s] + seg_len[s] <= seg_off[s + 1] and <= n.  The lanes
 *                   between the end of a segment and the next offset are padding.
 *   seg_hp   fp32   [nseg][2] = {weight_decay, lr_factor}
 *   coef     fp32   [nseg] clip coefficient, written by sfod_grad_clip_coef, read by sfod_sgd_ema_seg
 * n (a multiple of 4) is the length of the flat arrays, which are 16-byte aligned.  The kernels bound every access by n,
 * so a table that breaks the rules above gives wrong numbers, never an access outside the arrays.
 *
 * sfod_grad_clip_coef: coef[s] = what torch.nn.utils.clip_grad_norm_(p, clip_value, norm_type) computes for tensor s alone,
 * of the gradient the optimiser applies (grad * grad_scale):  c = clip_value / (norm + 1e-6);  coef = c > 1 ? 1 : c.
 * norm_type 0: 2-norm (sum of squares, sqrt); 1: max-norm.  Padding lanes are not read into the norm.  Two launches
 * whatever nseg is: partials per 4096-element chunk of the flat array (one writer per slot, no atomics), then one
 * workgroup per segment adds its partials in a fixed order -- the result is bit-identical from run to run.  No host read.
 * Non-finite gradients: an infinity gives norm = inf and coef = 0; a NaN gives coef = NaN (the comparison keeps it,
 * like torch).  ws: sfod_grad_clip_ws_floats(n, nseg) floats of device memory, need not be initialised.
 *
 * sfod_sgd_ema_seg: sfod_sgd_ema over [0, n) in ONE launch with per-segment hyper-parameters.  Per element
 *   g' = grad * grad_scale
 *   clip_type 1 ("value"): g' = clamp(g', -clip_value, clip_value), NaN stays NaN
 *   clip_type 2 ("norm"):  g' = grad * (grad_scale * coef[s])   (the coefficient folded into the scale: with coef == 1
 *                          the update is bit-identical to clip_type 0; an infinite gradient under coef == 0 becomes NaN)
 *   gr = g' + weight_decay[s] * p;   m = first_step ? gr : momentum * m + gr;   d = nesterov ? gr + momentum * m : m
 *   p -= (lr * lr_factor[s]) * d;    teacher = p * (1 - k) + teacher * k  as in sfod_sgd_ema (teacher may be NULL).
 * An element belongs to the last segment whose offset is <= its index, so padding lanes are updated with their
 * segment's values like sfod_sgd_ema does (they hold zeros and keep them).  clip_coef may be NULL unless clip_type == 2.
 * With clip_type 0, nesterov 0 and every lr_factor 1 the result equals sfod_sgd_ema's bit for bit. */
int64_t sfod_grad_clip_ws_floats(int64_t n, int nseg);
int sfod_grad_clip_coef(const float* grad, int64_t n, const int64_t* seg_off, const int64_t* seg_len, int nseg,
                        float grad_scale, float clip_value, int norm_type, float* coef, float* ws,
                        int64_t ws_floats, void* stream);
int sfod_sgd_ema_seg(float* param, const float* grad, float* mom, float* teacher, int64_t n,
                     const int64_t* seg_off, int nseg, const float* seg_hp, const float* clip_coef,
                     const float* lr, float momentum, float grad_scale, int clip_type, float clip_value,
                     int nesterov, float ema_keep, float ema_one_minus_keep, int first_step, void* stream);
/* t = s*(1-k) + t*k  on fp32 buffers (BN running stats) */
int sfod_ema(float* teacher, const float* student, int64_t n, float keep, float one_minus_keep, void* stream);
/* the same update on the int64 buffers (num_batches_tracked): fp32 arithmetic, truncated on the way back like the
 * reference's load_state_dict copy (source_free_adaptive_teacher.py:583-603, SURVEY A.17 iv).  Both factors are passed
 * as the caller rounded them (torch rounds the Python doubles k and 1 - k to fp32 separately). */
int sfod_ema_i64(int64_t* teacher, const int64_t* student, int n, float keep, float one_minus_keep, void* stream);
/* the scalars the trainer logs after the teacher pass (source_free_adaptive_teacher.py:411-423,445-452): out[0] mean over
 * images of the mean detection score, out[1] RPN proposals with logit > thr per image, out[2] mean pseudo-label count.
 * det_scores [B,D] / det_count [B], rpn_logits [B,P] / rpn_count [B], gt_count [B]; out: 3 floats. */
int sfod_teacher_metrics(const float* det_scores, const int* det_count, int D, const float* rpn_logits,
                         const int* rpn_count, int P, const int* gt_count, int B, float thr, float* out,
                         void* stream);

/* fp32 [n] (n % 8 == 0) -> SFOD_F16X3 pairs and SFOD_BF16X3 pairs of the same values in one pass ("f16x3" mode: a tensor
 * that is the operand of a forward product and of a weight gradient; replaces the reference's single fp32 tensor at
 * every such site, e.g. the RPN head input daod/modeling/proposal_generator/rpn.py:25-56) */
int sfod_cast_pairs_both(const float* src, void* dst_f16x3, void* dst_bf16x3, int64_t n, void* stream);
/* SFOD_F16X3 range report: every producer of half pairs raises a device flag when a value beyond +-65504 (an infinity included; NaN stays NaN) had to be
 * clamped (activations or scaled weights outside the window the mode assumes).  This call ORs the flags into the caller's
 * device word (zeroed by the caller once) and clears them; no host synchronisation -- the trainer reads the word at its
 * metrics period, beside the RPN's non-finite flag (d2 raises FloatingPointError inside predict_proposals). */
int sfod_f16x3_poll(uint32_t* word, void* stream);
/* utilities */
int sfod_fill_f32(float* p, int64_t n, float v, void* stream);
/* src (src_dt) -> dst (dst_dt), n logical elements.  Served: SFOD_F32 <-> SFOD_BF16 and the two copies; SFOD_F32 <-> either
 * pair format, pair -> the same pair, pair -> the other pair (the re-split of fp32(hi + lo)); pairs need n % 8 == 0.
 * Anything else -- an unknown storage type, SFOD_BF16 <-> a pair format -- is refused with SFOD_EBADARG before any launch. */
int sfod_cast(const void* src, void* dst, int64_t n, int src_dt, int dst_dt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
