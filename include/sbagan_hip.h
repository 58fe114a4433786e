/*
 * sbagan_hip.h -- C ABI of libsbagan_hip.so: the MI355X (gfx950) kernels behind
 * the SBA-GAN adversarial training hot path.
 *
 * Conventions
 *  - every entry point is extern "C", takes raw DEVICE pointers, sizes and a
 *    hipStream_t (passed as void*), returns int: 0 = ok, <0 = SBA_E_* below.
 *    Nothing is allocated, freed or synchronised inside; no global state; the
 *    library is thread-safe per stream and graph-capturable.
 *  - activations are NHWC ("channels last").  `dtype` selects the storage and
 *    MFMA input type of activations / packed weights: SBA_F32 (exact f32 MFMA,
 *    v_mfma_f32_32x32x2_f32) or SBA_BF16 (v_mfma_f32_32x32x16_bf16, f32
 *    accumulate).  Statistics, losses, master weights, gradients of weights and
 *    optimizer state are always f32.
 *  - "reference" citations are relative to zhengfei0908/SBA-GAN AttnGAN2/code.
 *    The reference has no FFI of its own: each function below
 *    replaces the torch.nn call sequence cited next to it.
 */
#ifndef SBAGAN_HIP_H
#define SBAGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBA_F32 0
#define SBA_BF16 1
/* bf16 activations / packed weights as SBA_BF16, but the RAW conv output y -- the pre-BatchNorm tensor, which is
 * only ever read by the BatchNorm kernels, never an MFMA operand -- is stored as IEEE binary16 (values saturate
 * at +-65504): three more mantissa bits at the same bytes, which removes one of the two bf16 roundings per
 * conv + BatchNorm + activation layer.  Accepted by sba_conv_igemm (no addend / bias / ReLU / mask epilogue) and by
 * the sba_bn_* entry points (where it describes y; out, dout, residual and dy stay bf16). */
#define SBA_BF16_YH 2

#define SBA_OK 0
#define SBA_E_ARG (-1)      /* shape / alignment / enum argument the kernels do not support */
#define SBA_E_LAUNCH (-2)   /* hipGetLastError() != hipSuccess after the launch */
#define SBA_E_UNSUPPORTED (-3)   /* sba_replay_create: the captured graph holds a node kind that cannot be re-issued */

#define SBA_ACT_NONE 0
#define SBA_ACT_GLU 1       /* model.py:15-23 */
#define SBA_ACT_LRELU 2     /* LeakyReLU(0.2), model.py:544 */
#define SBA_ACT_RELU 3      /* sba_bn_act_fwd only: BasicConv2d of the Inception trunk in TRAINING mode (frozen weights,
                             * batch statistics: pretrain_DAMSM.py:51 cnn_model.train(), model.py:170-199); no backward */

#define SBA_MAX_TAPS 32

/* Geometry of one implicit-GEMM convolution launch.  Output pixel (oy, ox) of
 * the OHs x OWs sub-grid reads input pixel (oy*sy + ty[t], ox*sx + tx[t]) for
 * tap t (zero outside the logical input), and is stored at output pixel
 * (oy*osy + ooy, ox*osx + oox) of the OH x OW output.  ups != 0: the logical
 * input is the nearest-neighbour x2 upsampling of the physical IH x IW tensor
 * (reference nn.Upsample(scale_factor=2), model.py:41), read as (iy>>1, ix>>1).
 * Packed weights for the launch are [Cout][ntaps][Cin]. */
typedef struct sba_conv_geom {
    int32_t N, IH, IW, Cin;
    int32_t OH, OW, Cout;
    int32_t OHs, OWs;
    int32_t sy, sx;
    int32_t osy, osx, ooy, oox;
    int32_t ups;
    int32_t ntaps;
    int8_t ty[SBA_MAX_TAPS];
    int8_t tx[SBA_MAX_TAPS];
    /* channel strides / offsets (elements) of the input and output tensors, for reading from /
     * writing into a channel slice of a wider NHWC tensor (Inception concats); 0 = dense
     * (x_cstride = Cin, y_cstride = Cout).  Honoured by sba_conv_igemm only. */
    int32_t x_cstride, x_coff, y_cstride, y_coff;
    int32_t relu;               /* epilogue: y = max(acc + bias, 0) when set (with `bias`) */
    /* tile configuration of sba_conv_igemm: 0 = the library's rule table; 1..SBA_IGEMM_TILES = a row of the tile table
     * (kTiles in csrc/igemm.hip, the only list of the ids; measured per layer shape by tools/tune_igemm.py into
     * sbagan/igemm_table.json; bf16 only, an id the geometry cannot use falls back to the rules).
     * ksplit: 0 = the library decides, n >= 1 = split K n ways. */
    int32_t tile, ksplit;
    /* sba_conv_wgrad only: non-zero = the caller knows dw is all zeros (just cleared, nothing accumulated yet):
     * kernel paths whose workgroups own their outputs exclusively then STORE instead of read-modify-write (the
     * GEMM-like layers' weight gradients are bound by that traffic: 268 MB for D_NET256's widest layer).  Paths
     * that add with atomics ignore it.  0 = always accumulate. */
    int32_t first_write;
    /* sba_conv_igemm: layout of the packed weights `w`.  0 = row-major [Cout][ntaps][Cin].  1 = FRAGMENT-MAJOR
     * (sba_pack_frag_multi): accepted only where sba_conv_igemm_plan (asked with w_layout = 1) reports family 0 or 4 -- the
     * halo-tile 3x3 kernels, bf16, stride 1, the nine taps = the nine cells of a 3 x 3 window, Cin % 32 == 0,
     * Cout % 32 == 0, no statistics for family 4 -- which keep the weight fragments in registers instead of LDS. */
    int32_t w_layout;
} sba_conv_geom;
#define SBA_IGEMM_TILES 18

const char* sba_version(void);

/* ---- deterministic-reduction mode ----------------------------------------------------------------------------
 * The one piece of process-wide state in the library.  Off (default): partial sums of BatchNorm / InstanceNorm
 * statistics, split-K tiles, pixel-split weight gradients, the attention / DAMSM gradients etc. meet in f32 atomics
 * (LDS and global), so results depend on workgroup arrival order in the last bits (like cuDNN's default algorithms
 * under the reference, torch.backends.cudnn.deterministic = False).  On: every such kernel writes its partial sums
 * to a private slot of the caller's `scratch` ring (plain stores) and an ordered fold adds the slots in slot order,
 * in-workgroup accumulation is done wave by wave, split-K is disabled and the conv epilogue's BatchNorm statistics
 * are replaced by the ordered sba_bn_stats pass over the stored tensor: two runs of the same launches on the same
 * inputs are BIT-IDENTICAL, whatever the stream / graph / replayer issues them.  Slower (about 1.3x on the step);
 * meant for parity tests and debugging, not for the benchmark.
 *   scratch: device memory, 256-byte aligned, >= 1 MiB; size it for the partial sums of one whole step (the
 *   B = 20 step uses about 0.6 GiB; sba_det_high_water() reports the largest amount handed out between two resets).
 *   The ring never wraps: an allocation that does not fit in what is left since the last sba_det_reset() fails
 *   (SBA_E_ARG from the launching entry point, one line on stderr) -- slots handed out earlier may still be waiting for
 *   their fold.  sba_det_reset() rewinds the ring (call it at the start of a
 *   step, before capture: the addresses are baked into captured graphs).  Switch the mode only while the device is
 *   idle. */
int sba_set_deterministic(int on, void* scratch, int64_t scratch_bytes);
int sba_get_deterministic(void);
int sba_det_reset(void);
int64_t sba_det_high_water(void);
/* Scratch ring for two-stage reductions in the DEFAULT mode (optional; NULL / 0 removes it).  Launches whose workgroups
 * would all add into the same few hundred addresses at their end (sba_d_stem_bwd's and sba_img_head_bwd's weight
 * gradients) then store per-workgroup partial sums into the ring and a second small launch folds them into the
 * destination; without a ring they use f32 atomics (correct, ~30 us slower per launch at 256 px).  Device memory,
 * 256-byte aligned, >= 1 MiB; a launch takes at most a quarter of it (larger requests fall back to atomics); regions
 * are handed out round-robin at host-issue time, so size it for the launches of one whole step (64 MiB covers the B = 20
 * step, which uses ~33 MB).  REUSE-DISTANCE ASSUMPTION: a region is handed out again after `scratch_bytes` of later
 * requests; the caller guarantees that the fold of its previous user has completed by then -- true when every step
 * joins its streams before the next one starts (GANStep.step does; a captured step re-uses the SAME regions every replay,
 * ordered by that join).  ONE ring per process = one device per process (the launch model of this library: one process
 * per GPU); the host refuses a second device (sbagan.ops.reduce_scratch). */
int sba_set_reduce_scratch(void* scratch, int64_t scratch_bytes);
/* SBA_BN_STAT_SLOTS the library was compiled with (the host sizes its statistics buffers with it) */
int sba_bn_stat_slots(void);

/* ---- convolutions (replace nn.Conv2d fwd / autograd bwd; model.py:32-35,552,563-574) ---- */
/* y[pixel][co] = sum_t sum_ci x[gather(pixel,t)][ci] * w[co][t][ci]  (+ addend[pixel][co]).
 * stats != NULL: also accumulates per-channel sum(y), sum(y^2) of the f32 accumulators into
 * stats[0..Cout) and stats[Cout..2Cout) (caller zeroes it) -- the BatchNorm batch statistics. */
/* workspace (may be NULL): scratch for split-K of small-M / long-K layers, used when it holds
 * >= 4*M*Cout bytes.  It must be ZERO-FILLED when first handed in; every call leaves it zero-filled
 * again, so stream-ordered reuse of one buffer needs no further memsets. */
int sba_conv_igemm(int dtype, const void* x, const void* w, void* y, const void* addend,
                   float* stats, const sba_conv_geom* g, void* workspace, int64_t workspace_bytes,
                   void* stream);
/* same with a per-output-channel f32 bias (may be NULL) added before the optional ReLU of g->relu
 * (frozen conv + folded BatchNorm(eval) + ReLU of the image encoder, model.py:170-199), and an optional
 * relu_mask tensor laid out like y: after the addend, outputs are zeroed where relu_mask <= 0 -- used by
 * the data-gradient that completes d(loss)/d(t) to apply the backward of the ReLU that produced t. */
int sba_conv_igemm_bias(int dtype, const void* x, const void* w, void* y, const void* addend,
                        float* stats, const float* bias, const void* relu_mask, const sba_conv_geom* g,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* Which kernel sba_conv_igemm launches for a geometry (nothing is launched; measurement / reporting aid):
 * plan[0] = family (0 halo-tile 3x3 conv3x3_halo_kernel, 1 igemm_dma2_kernel, 2 igemm_dma_kernel, 3 igemm_kernel, 4 the general
 * register-weight halo kernel conv3x3_halo3g_kernel -- only with g->w_layout = 1),
 * plan[1] = tile id (families 1 / 2: the ids of sba_conv_geom.tile) or configuration, plan[2] = K splits. */
int sba_conv_igemm_plan(int dtype, const sba_conv_geom* g, int64_t workspace_bytes, int* plan);
/* *bm x *bn = the workgroup tile (output pixels x output channels) of tile id 1..SBA_IGEMM_TILES */
int sba_conv_igemm_tile_shape(int tile, int* bm, int* bn);

/* ---- inference: conv + BatchNorm(eval) + GLU as ONE launch (sbagan/infer.py) ----
 * sba_fold_bn_pack: fold an eval-mode BatchNorm into the layer in front of it and pack the result for the forward
 * kernels.  w: f32 [O][taps][Cin] (a conv parameter stored channels_last, or a dense weight with taps = 1);
 *   out[r][tap][ci] = w[src(r)][tap][ci] * s,   bias[r] = beta - running_mean * s,   s = gamma / sqrt(running_var + eps)
 * with the product formed in f32 and rounded once to `dtype`.  glu = 0: O rows, src(r) = r.  glu = 1 (O = 2C, channel c
 * gated by channel C + c): 64 * ceil(C / 32) rows, interleaved in granules of 32 -- rows 64 b .. 64 b + 31 are value
 * channels 32 b .. 32 b + 31, rows 64 b + 32 .. 64 b + 63 their gates, rows of channels >= C are zero -- so that the
 * 32 x 32 MFMA output layout leaves a value and its gate in the same lane.  The fragment-major copy the register-weight
 * halo kernel reads is sba_pack_frag_multi of `out`. */
int sba_fold_bn_pack(int dtype, const float* w, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, void* out, float* bias, int O, int taps, int Cin, int glu,
                     void* stream);
/* y[pixel][c] = (acc[c] + bias[row of c]) * sigmoid(acc[C + c] + bias[row of C + c]), c < C, dense NHWC, for the
 * stride-1 3 x 3 geometries ('3x3', and '3x3up' behind the nearest x2 upsample) with w / bias from
 * sba_fold_bn_pack(glu = 1); g->Cout = the PACKED row count 64 * ceil(C / 32), g->y_cstride = g->y_coff = 0,
 * g->w_layout = 1 for the fragment-major copy where the plan reports family 0.  bf16: C % 8 == 0.  No split-K, no
 * workspace.  The residual half of a ResBlock (bias + addend, no activation) is sba_conv_igemm_bias with
 * sba_fold_bn_pack(glu = 0) operands. */
int sba_conv_igemm_glu(int dtype, const void* x, const void* w, const float* bias, void* y, int C,
                       const sba_conv_geom* g, void* stream);
/* the kernel sba_conv_igemm_glu launches: plan[0] = 0 halo-tile kernels (plan[1]: bit 0 = behind the upsample, bit 1 =
 * conv3x3_halo3_kernel, fragment-major weights), 3 igemm_kernel (plan[1] = configuration: 0 128x128, 1 256x64, 2 128x64,
 * 5 64x64 two waves); plan[2] = 1. */
int sba_conv_igemm_glu_plan(int dtype, const sba_conv_geom* g, int C, int* plan);
/* GROUPED launch: n <= SBA_GROUP_MAX independent convolutions -- no output of one is an input of another, their outputs
 * do not overlap -- as ONE grid (bf16 only, no split-K, no statistics; bias / ReLU (g->relu) / addend /
 * relu_mask per item as in sba_conv_igemm_bias).  For the branches of an Inception block at one depth level (model.py:226-262:
 * the reference runs them one after the other): each alone is 120..273 workgroups of a 64 x 64 tile on 256 CUs.
 * tile: an id whose row of the tile table has a grouped form -- 1, 3, 5, 7 (0 = 1; 7 falls back to 5 when some
 * Cin % 64 != 0).  The item array is HOST memory, read during the call. */
#define SBA_GROUP_MAX 8
typedef struct sba_conv_group_item {
    const void* x; const void* w; void* y; const void* addend; const float* bias; const void* relu_mask;
    const sba_conv_geom* g;
} sba_conv_group_item;
int sba_conv_igemm_group(int dtype, int n, const sba_conv_group_item* items, int tile, void* stream);
/* The same with split-K: every item's K range (ntaps * Cin) is cut into `ksplit` slices (grid.z), partial sums meet in
 * f32 atomics in the item's own [M][Cout] slice of `workspace` (zero-filled when handed in, left zero-filled; needs
 * sum_i 4 * M_i * Cout_i bytes, 16-byte aligned) and ONE finishing launch for the whole group applies the epilogues.
 * Falls back to ksplit = 1 when the workspace is too small, some Cin % 64 != 0, or in the deterministic mode.
 * Used for the four parity classes of the data gradient of the 4x4 stride-2 conv (model.py:552 downBlock backward):
 * they read the same dy, write disjoint pixels of dx, and were four launches of 80..640 workgroups each. */
int sba_conv_igemm_group_splitk(int dtype, int n, const sba_conv_group_item* items, int tile, int ksplit,
                                void* workspace, int64_t workspace_bytes, void* stream);
/* dw[co][t][ci] += sum_pixel dy[pixel][co] * x[gather(pixel,t)][ci]   (f32 accumulate/output).
 * ksplit > 1 splits the pixel range over that many workgroups (atomic accumulation). */
int sba_conv_wgrad(int dtype, const void* x, const void* dy, float* dw, const sba_conv_geom* g,
                   int ksplit, void* stream);
/* The launch sba_conv_wgrad makes for a geometry (g->first_write included), with the deterministic mode on (det != 0)
 * or off; nothing is launched, no device is needed.  plan[0] = family: 0 wgrad_row_dma_kernel, 1 wgrad_small_dma_kernel,
 * 2 wgrad_small_kernel, 3 wgrad_rows_kernel, 4 wgrad_kernel; plan[1..4] = template arguments (family 0: KW, SX, XB, D;
 * family 1: CT, D; the others: the dtype); plan[5..7] = grid x / y / z (z = pixel splits); plan[8] = threads;
 * plan[9] = dynamic LDS bytes; plan[10] = pixel chunks (family 3: 64-pixel row segments) per split; plan[11] = epilogue
 * mode: 0 dw += sum, 1 f32 atomics, 2 store; plan[12] = partial tensors the deterministic mode folds in order (0 = none);
 * plan[13] = family 0: log2 of the output columns of a 32-pixel chunk. */
#define SBA_WGRAD_PLAN_INTS 14
int sba_conv_wgrad_plan(int dtype, const sba_conv_geom* g, int ksplit, int det, int* plan);
/* weight packing: master f32 [Cout][KH][KW][Cin] (= torch channels_last storage of an OIHW
 * parameter) -> packed `dtype` weights.  mode 0: same order (cast).  mode 1: data-gradient
 * weights of a stride-1 'same' conv: out[ci][KH-1-kh][KW-1-kw][co].  mode 2: data-gradient of
 * the 4x4 stride-2 pad-1 conv, four parity classes: out[(py*2+px)][ci][j*2+i][co] with
 * kh = (1-py) + 2j, kw = (1-px) + 2i.  mode 3 (3x3 only): data-gradient of (nearest x2 -> conv3x3)
 * collapsed into ONE 4x4 stride-2 pad-1 conv over dy (16/36 of the FLOPs of the conv at the upsampled
 * resolution + 2x2 sum pooling): out[ci][dd*4+ee][co] = sum_{kh in S(dd), kw in S(ee)} w[co][kh][kw][ci]
 * with S(0)={2}, S(1)={1,2}, S(2)={0,1}, S(3)={0}; 16*Cin*Cout elements. */
int sba_pack_weight(int dtype, const float* w, void* out, int Cout, int KH, int KW, int Cin,
                    int mode, void* stream);
/* All packed copies of ONE network's conv weights in one launch (after its optimizer step, cf.
 * trainer.py:275,296): per tensor the forward operand (mode-0 cast, skipped when fwd is NULL)
 * and the data-gradient operand (mode 1, 2 or 3 as above, skipped when tr is NULL) are written from a
 * single read of the f32 master.  `descs` is a DEVICE array; workgroup b serves the tensor d with
 * tile_begin[d] <= b < tile_begin[d+1] (tiles: tap-major, then 64-row Cout tiles, then 64-column
 * Cin tiles; co_tiles = ceil(Cout/64), ci_tiles = ceil(Cin/64)); total_tiles = sum over tensors
 * of slots*co_tiles*ci_tiles with slots = KH*KW (16 for mode 3).  Cin must be a multiple of 4. */
typedef struct sba_pack_desc {
    const float* w;
    void* fwd;
    void* tr;
    int32_t Cout, KH, KW, Cin;
    int32_t mode;
    int32_t tile_begin;
    int32_t co_tiles, ci_tiles;
} sba_pack_desc;
int sba_pack_weights_multi(int dtype, const sba_pack_desc* descs, int ndesc, int total_tiles, void* stream);
/* Row-major packed bf16 conv operands [R][taps][K] (R, K multiples of 64: the outputs of sba_pack_weight /
 * sba_pack_weights_multi; R a multiple of 32, K of 16) -> FRAGMENT-MAJOR copies [ceil(R/64)][taps][2][K/16][64][8] (the
 * destination holds ceil(R/64)*64 * taps * K elements): the 64 lanes' 16-byte MFMA B fragments of one (tap, 32-row tile,
 * 16-deep k-step) contiguous (1 KB), lane = ((k >> 3) & 1) * 32 + (r & 31).  `descs` is a DEVICE
 * array; one work unit = 16 bytes, tensor d owns units [unit_begin[d], unit_begin[d+1]); total_units = sum R*taps*K/8. */
typedef struct sba_frag_desc {
    const void* src;
    void* dst;
    int32_t R, taps, K, unit_begin;
} sba_frag_desc;
int sba_pack_frag_multi(const sba_frag_desc* descs, int ndesc, int total_units, void* stream);
/* sum each 2x2 block: dx[n][y][x][c] = sum dup[n][2y+a][2x+b][c] (bwd of nearest x2). */
int sba_pool2x2_sum(int dtype, const void* dup, void* dx, int N, int H, int W, int C, void* stream);

/* ---- BatchNorm(train) + activation (model.py:43-44,62-65,543-544,553-554) ---- */
/* BatchNorm batch statistics are accumulated in SBA_BN_STAT_SLOTS replicas ("slots") of the
 * (sum[C], sumsq[C]) pair: a conv epilogue adds into slot (workgroup index mod SLOTS), which divides the
 * same-address atomic contention of thousands of workgroups by SLOTS; readers add the slots up.  A
 * statistics buffer is therefore stats[groups][SBA_BN_STAT_SLOTS][2C] floats, zeroed by the caller. */
#ifndef SBA_BN_STAT_SLOTS
#define SBA_BN_STAT_SLOTS 8
#endif
/* All BatchNorm entry points take `groups` >= 1 independent BatchNorm batches laid back to back
 * (`rows` NHWC rows each; the discriminator's real | fake passes of losses.py:139-140 share one conv
 * launch); per-group arrays are stats[groups][SLOTS][2C], aux[groups][4C] (= scale, shift, mean, rstd),
 * red[groups][2C].  C a power of two <= 4096. */
/* stats[g][slot][0..C) += sum(y), stats[g][slot][C..2C) += sum(y^2) (caller zeroes): only needed when the conv
 * epilogue could not produce them (groups > 1). */
int sba_bn_stats(int dtype, const void* y, float* stats, int64_t rows, int groups, int C, void* stream);
/* finalize + normalise + activation in one launch: scale/shift/mean/rstd from stats (training) or
 * from the running statistics (training == 0) -> aux; running stats update per group in order
 * (momentum, unbiased var), num_batches_tracked += groups; out = act(y*scale+shift) (+ residual).
 * GLU halves the channel count.  out may have a larger channel stride (out_cstride) and offset
 * (out_coff) so that it can be written into a concat. */
int sba_bn_act_fwd(int dtype, const void* y, const float* stats, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float* aux,
                   const void* residual, void* out, int64_t rows, int groups, int C, int act,
                   int out_cstride, int out_coff, float eps, float momentum, int training, void* stream);
/* pass 1 of the backward: red[g][slot][0..C) += sum dz, red[g][slot][C..2C) += sum dz*xhat, where dz is the
 * gradient w.r.t. the BN output (activation backward applied to dout on the fly).  Like the forward statistics the
 * sums are spread over SBA_BN_STAT_SLOTS replicas: red is [groups][SBA_BN_STAT_SLOTS][2C] floats, zeroed by the
 * caller; pass 2 adds the replicas up. */
int sba_bn_act_bwd_reduce(int dtype, const void* y, const void* dout, const float* aux, float* red,
                          int64_t rows, int groups, int C, int act, int dout_cstride, int dout_coff,
                          void* stream);
/* pass 2: dy = gamma*rstd*(dz - mean(dz) - xhat*mean(dz*xhat)); also dgamma += sum_slots red[g][.][C+c],
 * dbeta += sum_slots red[g][.][c]. */
int sba_bn_act_bwd_apply(int dtype, const void* y, const void* dout, const float* aux, const float* red,
                         void* dy, float* dgamma, float* dbeta, int64_t rows, int groups, int C, int act,
                         int dout_cstride, int dout_coff, void* stream);
/* training-mode forward for small maps WITHOUT conv-epilogue statistics (grouped passes): batch statistics,
 * finalize (aux, running stats per group in order, num_batches_tracked += groups) and normalise + activation
 * in ONE launch; no residual. */
int sba_bn_act_fwd_fused(int dtype, const void* y, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, int64_t* num_batches_tracked, float* aux, void* out, int64_t rows,
                         int groups, int C, int act, int out_cstride, int out_coff, float eps, float momentum,
                         void* stream);
/* both passes in ONE launch for small maps (a workgroup owns a channel vector over all rows of a group):
 * same results as reduce + apply; the host picks it when rows per group is at most a few thousand. */
int sba_bn_act_bwd_fused(int dtype, const void* y, const void* dout, const float* aux, void* dy,
                         float* dgamma, float* dbeta, int64_t rows, int groups, int C, int act,
                         int dout_cstride, int dout_coff, void* stream);
/* Linear(no bias)+BatchNorm1d(train)+GLU on [B][F] f32, output permuted to NHWC [B][4*4][F/2/16]
 * (INIT_STAGE_G.fc + view, model.py:353-356,372-373). */
int sba_bn1d_glu_fwd(int dtype, const float* y, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* nbt, float* mean,
                     float* rstd, void* out, int B, int F, float eps, float momentum, void* stream);
int sba_bn1d_glu_bwd(int dtype, const float* y, const void* dout, const float* gamma,
                     const float* beta, const float* mean, const float* rstd, float* dy,
                     float* dgamma, float* dbeta, int B, int F, void* stream);

/* ---- small dense layers, f32 (CA_NET, MAPPING_NET, INIT fc, AdaIN style; model.py:278,306-313,330,354) ---- */
int sba_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int N,
                   void* stream);
/* inference INIT_STAGE_G.fc: Linear(no bias) + BatchNorm1d(eval) + GLU + view(B, F2 / 16, 4, 4) in one launch:
 * out[b][p][c] (NHWC, `dtype`) = GLU feature 16 c + p of x[b] with wp / bias = sba_fold_bn_pack(SBA_F32, ..., O = 2 F2,
 * taps = 1, Cin = K, glu = 1).  F2 % 16 == 0. */
int sba_linear_glu_fwd(int dtype, const float* x, const float* wp, const float* bias, void* out, int B, int K,
                       int F2, void* stream);
/* dx = dy*W (may be NULL); dw += dy^T x (may be NULL); dbias += sum dy (may be NULL).  dbias is summed by the dw
 * kernels: dbias without dw is refused (SBA_E_ARG), not ignored. */
int sba_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw,
                   float* dbias, int B, int K, int N, void* stream);
/* CA_NET tail (model.py:281-294): h[B][4c] -> GLU -> mu|logvar; c = eps*exp(.5*logvar)+mu. */
int sba_ca_fwd(const float* h, const float* eps, float* c, float* mu, float* logvar, int B, int C,
               void* stream);
int sba_ca_bwd(const float* h, const float* eps, const float* dc, const float* dmu,
               const float* dlogvar, float* dh, int B, int C, void* stream);

/* attention key projection conv_context (GlobalAttention.py:75,95-97): src[b][i][l] = sum_c W[i][c] words[b][c][l].
 * bwd: dW += ..., dwords = ... (may be NULL). */
int sba_ctx_proj_fwd(const float* words, const float* W, float* src, int B, int idf, int cdf, int L,
                     void* stream);
/* sba_ctx_proj_fwd with FP8 (OCP e4m3) operands on v_mfma_f32_32x32x16_fp8_fp8, block-scaled per 32-row tile,
 * f32 accumulate (BASELINE config 5).  cdf % 16 == 0.  Relative L2 error of src <= 8e-2 on N(0,1) data. */
int sba_ctx_proj_fwd_fp8(const float* words, const float* W, float* src, int B, int idf, int cdf, int L,
                         void* stream);
int sba_ctx_proj_bwd(const float* words, const float* W, const float* dsrc, float* dW, float* dwords,
                     int B, int idf, int cdf, int L, void* stream);

/* ---- AdaIN (model.py:324-339) ---- */
/* per (n,c) sum/sumsq of h over HW -> mean/rstd (biased var, eps). */
int sba_instnorm_stats(int dtype, const void* h, float* mean, float* rstd, int N, int HW, int C,
                       float eps, void* stream);
/* out[..., coff + c] = (style[n][c]+1)*xhat + style[n][C+c]. */
int sba_adain_fwd(int dtype, const void* h, const float* mean, const float* rstd, const float* style,
                  void* out, int N, int HW, int C, int out_cstride, int out_coff, void* stream);
/* red[n][c][0..2) += (sum dout*xhat, sum dout)  -> dstyle; */
int sba_adain_bwd_reduce(int dtype, const void* h, const void* dout, const float* mean,
                         const float* rstd, float* red, int N, int HW, int C, int dout_cstride,
                         int dout_coff, void* stream);
/* dh (+)= (style+1)*rstd*(dout - mean(dout) - xhat*mean(dout*xhat)); dstyle[n][c] = red sumxhat,
 * dstyle[n][C+c] = red sum.  accumulate != 0 adds into dh. */
int sba_adain_bwd_apply(int dtype, const void* h, const void* dout, const float* mean,
                        const float* rstd, const float* style, const float* red, void* dh,
                        float* dstyle, int N, int HW, int C, int dout_cstride, int dout_coff,
                        int accumulate, void* stream);

/* ---- word attention (GlobalAttention.py:82-121) ---- */
/* src[B][idf][L] f32 is conv_context applied to the words (use sba_linear_fwd).
 * mask[B][L] uint8 or NULL.  mask_mode 0 = the reference's row order
 * (row r = b*Q+q of the score matrix takes mask[r % B]), 1 = per-sample mask[b].
 * ctx written at channel offset out_coff of a tensor with out_cstride channels.
 * att (f32 [B][L][Q]) may be NULL. */
int sba_word_attn_fwd(int dtype, const void* h, const float* src, const uint8_t* mask, void* ctx,
                      float* att, int B, int Q, int idf, int L, int mask_mode, int out_cstride,
                      int out_coff, void* stream);
/* BASELINE config 5 ("fp8 MFMA for the attention / context GEMM"): the same forward (bf16 activations) with BOTH
 * contractions of GlobalAttention.py:103,117 on v_mfma_f32_32x32x16_fp8_fp8 -- OCP e4m3 operands, f32 accumulate, h scaled
 * per 32-query tile and the keys per image by powers of two (exact un-scaling), probabilities x 256.  Forward only: the
 * backward (sba_word_attn_bwd) keeps the bf16 / f32 operands (straight-through w.r.t. the quantisation).  Stated tolerance:
 * context rel L2 <= 8e-2, attention map abs <= 0.12 on N(0,1)-scaled inputs (tests/test_kernels_gpu.py). */
int sba_word_attn_fwd_fp8(const void* h, const float* src, const uint8_t* mask, void* ctx, float* att, int B, int Q,
                          int idf, int L, int mask_mode, int out_cstride, int out_coff, void* stream);
/* dh = d/dh, dsrc[B][idf][L] += d/dsrc (f32, caller zeroes).  accumulate != 0: dh += . */
int sba_word_attn_bwd(int dtype, const void* h, const float* src, const uint8_t* mask,
                      const void* dctx, void* dh, float* dsrc, int B, int Q, int idf, int L,
                      int mask_mode, int dctx_cstride, int dctx_coff, int accumulate, void* stream);

/* ---- image head: conv3x3(ngf->3)+tanh, NHWC in, NCHW f32 out (model.py:426-437) ---- */
int sba_img_head_fwd(int dtype, const void* h, const float* w, float* img, int N, int H, int W,
                     int C, void* stream);
/* dh (+)= ..., dw[3][3][3][C] += ...  (w and dw in channels_last [co][kh][kw][ci]). */
int sba_img_head_bwd(int dtype, const void* h, const float* w, const float* img, const float* dimg,
                     void* dh, float* dw, int N, int H, int W, int C, int accumulate, void* stream);

/* ---- discriminator stem: conv4x4 s2 p1 (3->ndf) + LeakyReLU(0.2), NCHW f32 in, NHWC out
 *      (model.py:563-564) ---- */
int sba_d_stem_fwd(int dtype, const float* img, const float* w, void* out, int N, int S, int C,
                   void* stream);
/* dw[C][4][4][3] += ; dimg (NCHW f32, may be NULL) = . `out` is the saved forward output. */
int sba_d_stem_bwd(int dtype, const float* img, const float* w, const void* out, const void* dout,
                   float* dimg, float* dw, int N, int S, int C, void* stream);

/* ---- logits head: conv4x4 s4 (8ndf->1, bias) + sigmoid on a 4x4 map (model.py:590-592,606-607) ---- */
int sba_logits_fwd(int dtype, const void* h, const float* w, const float* bias, float* prob, int B,
                   int K, void* stream);
int sba_logits_bwd(int dtype, const void* h, const float* w, const float* prob, const float* dprob,
                   void* dh, float* dw, float* dbias, int B, int K, int accumulate, void* stream);
/* cat(h[B][16][C], sent[B][E] tiled 4x4) -> out[B][16][C+E]  (model.py:597-600) */
int sba_cond_cat_fwd(int dtype, const void* h, const float* sent, void* out, int B, int C, int E,
                     void* stream);
int sba_cond_cat_bwd(int dtype, const void* dout, void* dh, float* dsent, int B, int C, int E,
                     int accumulate, void* stream);

/* ---- frozen image encoder pieces (CNN_ENCODER, model.py:162-267; forward + backward-data only) ---- */
/* bilinear resize, align_corners=True (model.py:210), NCHW f32 [NC][S][S] -> [NC][D][D];
 * backward != 0: `in` is d(out) [NC][D][D] and `out` receives d(in) [NC][S][S]. */
int sba_resize_bilinear(const float* in, float* out, int NC, int S, int D, int backward, void* stream);
/* Conv2d_1a_3x3: conv3x3 s2 p0 (3->C) + bias + ReLU, NCHW f32 image -> NHWC features. */
int sba_enc_stem_fwd(int dtype, const float* img, const float* w, const float* bias, void* out, int N, int S, int C,
                     void* stream);
int sba_enc_stem_bwd(int dtype, const float* w, const void* out, const void* dout, float* dimg, int N, int S, int C,
                     void* stream);
/* both of the above in one launch: the stem conv (C = 32) reading the S -> D bilinear resize of the image on the fly -- the
 * D x D tensor (model.py:210: 299 x 299) is never written; the interpolation is sba_resize_bilinear's expression. */
int sba_enc_stem_resize_fwd(int dtype, const float* img, const float* w, const float* bias, void* out, int N, int S, int D,
                            int C, void* stream);
/* F.max_pool2d(x, 3, 2) on NHWC channel slices (cs = channel stride, co = channel offset); the backward
 * routes each window's gradient to its first maximum in scan order (torch's tie rule). */
int sba_maxpool3x3s2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, int xcs, int xco, int ycs,
                         int yco, void* stream);
int sba_maxpool3x3s2_bwd(int dtype, const void* x, const void* dy, void* dx, int N, int H, int W, int C, int xcs,
                         int xco, int dycs, int dyco, int dxcs, int dxco, int accumulate, void* stream);
/* the same pair with the argmax kept: fwd also writes argmax[N][OH][OW][C] (uint8: kh*3+kw of the first maximum, 8-byte
 * aligned), bwd reads it instead of re-deriving it from x (4 instead of 36 input loads per vector) */
int sba_maxpool3x3s2_fwd_arg(int dtype, const void* x, void* y, uint8_t* argmax, int N, int H, int W, int C, int xcs,
                             int xco, int ycs, int yco, void* stream);
int sba_maxpool3x3s2_bwd_arg(int dtype, const uint8_t* argmax, const void* dy, void* dx, int N, int H, int W, int C,
                             int dycs, int dyco, int dxcs, int dxco, int accumulate, const void* relu_mask, void* stream);
/* (relu_mask, optional: a tensor laid out like dx -- the pooled tensor itself when a ReLU produced it; dx is zeroed where
 * it is <= 0, after the accumulation: the ReLU's backward without a pass of its own) */
/* F.avg_pool2d(x, 3, 1, 1) (count_include_pad); self-adjoint, so it is also its own backward. */
int sba_avgpool3x3(int dtype, const void* x, void* y, int N, int H, int W, int C, int xcs, int xco, int ycs, int yco,
                   int accumulate, void* stream);
/* dpre[rows][C] = (out > 0) ? dout : 0 on channel slices. */
int sba_relu_bwd(int dtype, const void* out, const void* dout, void* dpre, int64_t rows, int C, int ocs, int oco,
                 int dcs, int dco, void* stream);
/* F.avg_pool2d over the whole HW map: x NHWC -> y [N][C] f32; backward != 0: x receives dy / HW. */
int sba_global_avgpool(int dtype, void* x, float* y, int N, int HW, int C, int backward, void* stream);
/* NHWC features <-> NCHW f32 (to_nhwc != 0: nchw -> nhwc). */
int sba_layout_nhwc_nchw(int dtype, void* nhwc, float* nchw, int N, int HW, int C, int to_nhwc, void* stream);

/* ---- losses ---- */
/* loss[0] = sum_s weight[s] * mean BCE(prob_s, target[s]) over nseg segments given by
 * offsets[s]..offsets[s+1] into the concatenated prob array (nn.BCELoss, losses.py:144-158,175-178).
 * dprob = d loss / d prob (scaled later by the upstream gradient). */
int sba_bce_multi(const float* prob, const int32_t* offsets, const float* target, const float* weight,
                  int nseg, float* loss, float* dprob, void* stream);
/* KL_loss (losses.py:210-214): loss, dmu, dlogvar. */
int sba_kl_loss(const float* mu, const float* logvar, float* loss, float* dmu, float* dlogvar,
                int n, void* stream);
/* DAMSM word loss (losses.py:62-132 with func_attention GlobalAttention.py:31-69).
 * feat[B][nef][R] f32 (R = 17*17), words[B][nef][L] f32, cap_lens int64[B].
 * sim[j][i] (image j, caption i) = log sum_t exp(g2 * cos(word_t, attended context)).
 * Saves attn[B*B][Lmax][R] and attn1 (first softmax) for the backward.
 * nef % 32 == 0, R <= 320, L <= 32, B <= 1024; cap_lens is clamped to [1, L] on the device (T below).
 * Which outputs are STORED and which are ADDED TO (tests/test_damsm_kernels_gpu.py holds the kernels to this):
 *   forward (both families): sim[B][B], attn and attn1 [B*B][L][R], wctx [B*B][L][nef] are stored -- for the words
 *     t < T only; the elements of attn, attn1 and wctx at t >= T are left UNWRITTEN, and no backward reads them.
 *   sba_damsm_words_bwd: dfeat[B][nef][R] and dwords[B][nef][L] (may be NULL) are ADDED TO (f32 atomics): the caller
 *     clears them -- also in deterministic mode, where the ordered fold adds the pairs' sum onto what is there.
 *   sba_damsm_words_bwd_mfma: dfeat is stored with accumulate = 0 and added to with accumulate = 1 (one owner per
 *     element either way); dwords (may be NULL) is added to, as above.
 *   sba_damsm_sent_fwd: s[B][B] is stored.  sba_damsm_sent_bwd: dcnn and drnn (each may be NULL) are ADDED TO, in
 *     both modes.  sba_damsm_sent_direct: loss_out[0] and dcnn (may be NULL) are stored.
 *   sba_ce_pair, sba_ce_pair_direct, sba_combine2: every output is stored. */
int sba_damsm_words_fwd(const float* feat, const float* words, const int64_t* cap_lens, float* sim,
                        float* attn, float* attn1, float* wctx, int B, int nef, int R, int L,
                        float gamma1, float gamma2, void* stream);
int sba_damsm_words_bwd(const float* feat, const float* words, const int64_t* cap_lens,
                        const float* sim, const float* attn, const float* attn1, const float* wctx,
                        const float* dsim, float* dfeat, float* dwords, int B, int nef, int R, int L,
                        float gamma1, float gamma2, void* stream);
/* sentence similarity matrix (losses.py:41-47): s[j][i] = cos(cnn[j], rnn[i]) * g3. */
/* The same loss on the bf16 MATRIX CORES (csrc/damsm_mfma.hip; nef % 64 == 0, nef <= 1024, R <= 384, L <= 32, and
 * 128 (nef + R rounded up to 32) + 4096 bytes of LDS per pair within 160 KB -- sba_damsm_prep_bytes and
 * sba_damsm_bwd_bytes return -1 otherwise and the callers keep the f32 kernels above; a positive size means that
 * sba_damsm_prep and both kernels below accept the shape).  Every product is formed from bf16 hi + lo parts of its
 * f32 factors (xh yh + xl yh + xh yl, f32 sums): results agree with the f32 kernels to ~1e-5 relative.
 *   sba_damsm_prep: features / words -> hi + lo operands in `prep` (caller-owned scratch of sba_damsm_prep_bytes bytes,
 *     16-byte aligned; read by the forward AND the backward of the same inputs).
 *   forward: one workgroup per (caption, image) pair; same outputs as sba_damsm_words_fwd.
 *   backward: `scratch` (caller-owned, sba_damsm_bwd_bytes bytes, 16-byte aligned, any contents): pass 1 (per pair)
 *     fills it with d(context), the attention and d(scores) as bf16 hi + lo MFMA fragments, pass 2 forms
 *     dfeat[j] (= or +=, `accumulate`) sum over (caption, word) of A x dcontext + dS x q as ONE contraction per image --
 *     every element of dfeat has one owner: no atomics, the same bits in every run.  dwords (may be NULL) is accumulated
 *     with f32 atomics (deterministic mode: ordered fold). */
int64_t sba_damsm_prep_bytes(int B, int nef, int R, int L);
int64_t sba_damsm_bwd_bytes(int B, int nef, int R, int L);
int sba_damsm_prep(const float* feat, const float* words, const int64_t* cap_lens, void* prep, int64_t prep_bytes,
                   int B, int nef, int R, int L, void* stream);
int sba_damsm_words_fwd_mfma(const void* prep, const float* words, const int64_t* cap_lens, float* sim, float* attn,
                             float* attn1, float* wctx, int B, int nef, int R, int L, float gamma1, float gamma2,
                             void* stream);
int sba_damsm_words_bwd_mfma(const void* prep, const float* words, const int64_t* cap_lens, const float* sim,
                             const float* attn, const float* attn1, const float* wctx, const float* dsim,
                             void* scratch, int64_t scratch_bytes, float* dfeat, int accumulate, float* dwords,
                             int B, int nef, int R, int L, float gamma1, float gamma2, void* stream);
/* The loss heads of the generator step with a FROZEN text side (losses.py:187-204: the upstream gradient of the four
 * cross-entropy terms is the constant LAMBDA), each as ONE launch instead of ce_pair + combine2 + scalar arithmetic:
 *   sba_ce_pair_direct: loss_out[0] = lam (loss0 + loss1) of the two cross entropies over the B x B scores (x scale,
 *     masked), dscore = d(that) / d(score);
 *   sba_damsm_sent_direct: the whole sentence loss -- cosine scores x gamma3, both cross entropies,
 *     loss_out[0] = lam (loss0 + loss1), dcnn = d(that) / d(cnn) (STORED; may be NULL); one workgroup, B <= 96,
 *     deterministic (partners walked in order). */
int sba_ce_pair_direct(const float* score, const uint8_t* mask, float scale, float lam, float* loss_out,
                       float* dscore, int B, void* stream);
int sba_damsm_sent_direct(const float* cnn, const float* rnn, const uint8_t* mask, float gamma3, float eps, float lam,
                          float* loss_out, float* dcnn, int B, int nef, void* stream);
int sba_damsm_sent_fwd(const float* cnn, const float* rnn, float* s, int B, int nef, float gamma3,
                       float eps, void* stream);
int sba_damsm_sent_bwd(const float* cnn, const float* rnn, const float* ds, float* dcnn, float* drnn,
                       int B, int nef, float gamma3, float eps, void* stream);
/* two cross entropies over a B x B score matrix and its transpose with labels = arange(B) and the
 * same-class mask (uint8[B][B], may be NULL) filled with -inf (losses.py:51-56,123-129):
 * loss[0] = CE(rows), loss[1] = CE(cols); dscore0/dscore1 = their gradients. `scale` multiplies
 * the scores first (gamma3 for the word loss). */
int sba_ce_pair(const float* score, const uint8_t* mask, float scale, float* loss, float* dscore0,
                float* dscore1, int B, void* stream);

/* out[k] = ga[0]*a[k] + gb[0]*b[k]: combines the two CE gradients with their upstream (device) scalars. */
int sba_combine2(float* out, const float* a, const float* ga, const float* b, const float* gb, int n,
                 void* stream);

/* ---- optimizer (trainer.py:136-143,275,297-299) ---- */
/* state = {int32 step; float step_size; float inv_sqrt_bc2}: step += 1 and the Adam bias
 * corrections for (lr, beta1, beta2), computed on device so the step is graph-replayable. */
int sba_adam_prepare(void* state, float lr, float beta1, float beta2, void* stream);
/* Adam update of n contiguous f32 parameters; avg != NULL: EMA avg = .999*avg + .001*p;
 * shadow != NULL: bf16 copy of the updated parameters (the packed forward weights). */
int sba_adam_step(float* p, const float* g, float* m, float* v, float* avg, void* shadow,
                  const void* state, int64_t n, float beta1, float beta2, float eps, float grad_scale,
                  void* stream);
/* RNN_ENCODER.forward of the frozen text encoder (model.py:127-159; trainer.py:248-252 calls it under
 * eval/no_grad every step): Embedding -> one-layer bidirectional LSTM over packed sequences.
 *   captions [B][T] int64 token ids, cap_lens [B] int64 (device memory: replaces the reference's
 *   cap_lens.tolist() host sync, model.py:139), emb_weight [ntoken][ninput],
 *   w_ih [2][4H][ninput], w_hh [2][4H][H], b_ih / b_hh [2][4H]  (= weight_ih_l0 | weight_ih_l0_reverse ...,
 *   PyTorch gate order i|f|g|o), h0 / c0 [2][B][H] or both NULL (= init_hidden zeros),
 *   gx_scratch [2][B*T][4H] f32 workspace.
 * Outputs: words [B][2H][Lout] (zeros past each caption's length, like pad_packed_sequence; Lout <= T is
 * the reference's max(cap_lens) when the host knows it, else T), sent [B][2H] (last valid hidden state,
 * forward | backward).  H in {64, 128}, ninput % 4 == 0. */
int sba_lstm_bidir_fwd(const int64_t* captions, const int64_t* cap_lens, const float* emb_weight,
                       const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                       const float* h0, const float* c0, float* gx_scratch, float* words, float* sent,
                       int B, int T, int Lout, int ntoken, int ninput, int H, void* stream);
/* ---- multi-stream launch replayer (host side of the step loop; no counterpart in the reference, whose
 * trainer.py:245-299 issues every launch from Python) ----
 * sba_replay_create walks a CAPTURED hipGraph_t (stream capture of one training step, or of one phase of it:
 * kernel / 1-D memcpy / memset / empty nodes and their edges), assigns every node a stream -- a chain keeps its
 * stream, a fork takes the next of at most max_streams -- and stores the launch list; sba_replay_launch
 * re-issues the nodes in topological order as plain asynchronous launches on those streams, with events only
 * where a dependency crosses streams; it begins after everything already queued on `stream` and `stream` waits
 * for its end.  flags: bit 0 = print a summary to stderr; bit 1 = issue the first chain of the graph on `stream`
 * ITSELF (for the per-phase graphs: a single-chain graph then uses no stream of its own -- a process has 4 hardware
 * queues by default and every extra stream shares one; max_streams = 4 is the measured optimum for the whole step).
 * Do not set bit 1 for callers on the NULL stream.  Unlike hipGraphLaunch on ROCm 7.2, independent branches then really run concurrently, at ~3 us
 * of host time per launch.  The graph must outlive the handle (kernel arguments live in its nodes); the handle
 * owns its streams and events.  Returns SBA_E_UNSUPPORTED for node kinds it cannot re-issue (callers fall
 * back to hipGraphLaunch).  info8 = {nodes, kernels, copies, memsets, streams, cross-stream waits, events, 0}.
 * This is the one entry point family that creates HIP objects (streams / events), at create time only. */
int sba_replay_create(void* hip_graph, int max_streams, int flags, void** out_handle);
int sba_replay_launch(void* handle, void* stream);
int sba_replay_info(void* handle, int* info8);
/* PRIORITIES for the longest dependency path.  Kernels of independent chains that run side by side share the CUs, and the
 * chain the step's duration hangs on (generator forward -> image encoder -> DAMSM -> their backward passes) is slowed by the
 * three discriminator updates beside it as much as they are by it.  sba_replay_prioritize
 *   1. issues every recorded node ONCE, alone, in order on `stream` with an event between neighbours -- this IS one
 *      execution of the recording (host-call nodes included: the callback runs), the caller counts it as a replay -- and keeps
 *      the durations;
 *   2. computes every node's earliest start and longest path to the end from them; nodes whose slack against the longest
 *      path of the whole recording is <= slack_frac of it are CRITICAL;
 *   3. assigns streams again, in two pools: n_high streams for the critical nodes, max_streams - n_high for the rest, created
 *      with hipStreamCreateWithPriority: mode 1 = (high, normal), 2 = (high, low), 3 = (normal, low); 0 = one pool, no
 *      priorities (only max_streams changes).
 * The dependencies enforced are the recorded ones in every mode: results do not depend on it.  verbose: 1 = a summary on
 * stderr, 2 = also the longest path node by node (start, duration alone, kernel, grid), 3 = also every node (duration alone, slack). */
int sba_replay_prioritize(void* handle, void* stream, int mode, int max_streams, int n_high, float slack_frac, int verbose);
/* HOST-CALL nodes.  sba_replay_marker launches a no-op kernel carrying `tag` (>= 0) on `stream`; captured into the graph it
 * becomes a node with the dependencies of its stream position.  A replay does not launch that node: it calls the callback
 * registered with sba_replay_set_callback -- void fn(int tag, void* stream, void* user) -- with the stream the node was
 * assigned to, after everything the node depends on has been issued.  The host issues there what cannot be recorded: an
 * RCCL collective (on its own stream, ordered behind `stream`), the wait for one (make `stream` wait for it), launches
 * that depend on host state.  This is how the DATA-PARALLEL step is one recording: the gradient exchanges sit between
 * its launches exactly where the eager step has them.  Without a callback the node is skipped.  info8[7] of
 * sba_replay_info = the number of such nodes. */
int sba_replay_marker(int tag, void* stream);
int sba_replay_set_callback(void* handle, void* fn, void* user);
int sba_replay_destroy(void* handle);
/* Training path of the same encoder (DAMSM pre-training, pretrain_DAMSM.py:49-130).
 *   sba_lstm_recur_train: the packed bidirectional recurrence on pre-computed input projections
 *     gx [2][B*T][4H] (= x W_ih^T + b_ih + b_hh, a plain GEMM the caller runs), also storing what BPTT needs:
 *     gates [2][B*T][4H] (i | f | g | o after their nonlinearities), cs / hs [2][B*T][H];
 *   sba_lstm_recur_bwd: back-propagation through time given d words [B][2H][Lout] and d sent [B][2H]:
 *     dG [2][B*T][4H] = gradient w.r.t. the gate pre-activations and hprev [2][B*T][H] = the hidden state every
 *     step started from (both must be ZERO-FILLED by the caller: rows past a caption's length are not written).
 *     The caller finishes with plain GEMMs: dW_ih = dG^T x, dW_hh = dG^T hprev, db = sum dG, dx = dG W_ih. */
int sba_lstm_recur_train(const float* gx, const int64_t* cap_lens, const float* w_hh, const float* h0,
                         const float* c0, float* words, float* sent, float* gates, float* cs, float* hs,
                         int B, int T, int Lout, int H, void* stream);
int sba_lstm_recur_bwd(const int64_t* cap_lens, const float* w_hh, const float* h0, const float* c0,
                       const float* gates, const float* cs, const float* hs, const float* dwords,
                       const float* dsent, float* dG, float* hprev, int B, int T, int Lout, int H, void* stream);
/* ---- BertEncoder forward (model_bert.py:161-189: frozen BERT-base trunk of the bert / mix variants) ----
 * The dense layers are 1x1 convolutions on sba_conv_igemm_bias (rows = B*L tokens); these are the pieces between
 * them.  Activations [B*L][C] of `dtype`; LayerNorm statistics and the softmax in f32.
 *   embed_ln:  LayerNorm(word_emb[token] + pos_emb[position] + type_emb[0]), eps as given (BERT: 1e-12)
 *   add_ln:    LayerNorm(x + residual)
 *   attention: per (caption, head) softmax(q k^T / 8) v over L <= 32 tokens with NO mask (the reference passes
 *              none, model_bert.py:181); qkv [B*L][3C] = q | k | v, heads of 64 channels
 *   gelu:      exact (erf) GELU in place;  tanh_transpose: y[b][c][l] = tanh(x[b*L + l][c]) (f32 out). */
int sba_bert_embed_ln(int dtype, const int64_t* tokens, const float* word_emb, const float* pos_emb,
                      const float* type_emb, const float* gamma, const float* beta, void* out, int B, int L,
                      int C, int ntoken, float eps, void* stream);
int sba_bert_add_ln(int dtype, const void* x, const void* residual, const float* gamma, const float* beta,
                    void* out, int rows, int C, float eps, void* stream);
int sba_bert_attention(int dtype, const void* qkv, void* ctx, int B, int L, int C, int heads, void* stream);
int sba_bert_gelu(int dtype, void* x, int64_t n, void* stream);
int sba_bert_tanh_transpose(int dtype, const void* x, float* y, int B, int L, int C, void* stream);
/* ---- BertEncoder training path (pretrain_DAMSM_bert.py: frozen trunk in train mode, trained heads) ----
 * Train-mode trunk: the three kernels above with dropout fused, same arguments after (p, seed, offset, site).  Kept
 * values are scaled by 1 / (1 - p) in f32 before the store; 0 <= p < 1 (p = 0: bit-identical to the entry points above).
 *   embed_ln_train:  dropout(LayerNorm(emb)),            element index = row * C + c
 *   attention_train: dropout(softmax) before the product with v, element index = ((b * heads + head) * L + query) * L + key
 *   add_ln_train:    LayerNorm(dropout(x) + residual),   element index = row * C + c  (x = dense output with its bias)
 * Sites (HF BertModel call order): 0 = embeddings; 1 + 3l + {0, 1, 2} = layer l's attention probabilities, attention
 * output, FFN output.  The mask is a pure function, no state and nothing stored:
 *   Philox4x32-10 with key (k0, k1) = (seed & 0xffffffff, seed >> 32) and counter (c0, c1, c2, c3) =
 *   (element index, site, offset & 0xffffffff, offset >> 32); each of the ten rounds is
 *     (hi0, lo0) = mulhilo32(0xD2511F53, c0); (hi1, lo1) = mulhilo32(0xCD9E8D57, c2);
 *     (c0, c1, c2, c3) = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); k0 += 0x9E3779B9; k1 += 0xBB67AE85 (mod 2^32);
 *   u = (float)(c0 >> 8) * 2^-24 of the final c0; the element is DROPPED when u < p. */
int sba_bert_embed_ln_train(float p, uint64_t seed, uint64_t offset, int site, int dtype, const int64_t* tokens,
                            const float* word_emb, const float* pos_emb, const float* type_emb, const float* gamma,
                            const float* beta, void* out, int B, int L, int C, int ntoken, float eps, void* stream);
int sba_bert_add_ln_train(float p, uint64_t seed, uint64_t offset, int site, int dtype, const void* x,
                          const void* residual, const float* gamma, const float* beta, void* out, int rows, int C,
                          float eps, void* stream);
int sba_bert_attention_train(float p, uint64_t seed, uint64_t offset, int site, int dtype, const void* qkv, void* ctx,
                             int B, int L, int C, int heads, void* stream);
/* Words head backward (words = tanh(conv_text(tokens)) transposed to [B][nef][L] f32): dwords, words [B][nef][L] f32 ->
 * dpre [B*L][nef] = (dwords * (1 - words^2)) transposed, in `dtype`; dbias[nef] += sum over (b, l) of the f32 values, in
 * a fixed order (no atomics).  dW_conv_text = dpre^T x is sba_conv_wgrad on the 1x1 geometry.  L <= 32, nef % 64 == 0. */
int sba_bert_words_head_bwd(int dtype, const float* dwords, const float* words, void* dpre, float* dbias, int B, int L,
                            int nef, void* stream);
/* Sentence head chain backward, sent = tanh(fc(pooled)), pooled = tanh(pooler(cls)), all f32, two launches, no atomics:
 *   g = dsent * (1 - sent^2);  dw_fc[nef][C] += g^T pooled;  db_fc += sum_b g;  dpooled[B][C] = g w_fc (stored);
 *   h = dpooled * (1 - pooled^2);  dw_pool[C][C] += h^T cls;  db_pool += sum_b h.   B <= 64, C and nef % 64 == 0. */
int sba_bert_sent_head_bwd(const float* dsent, const float* sent, const float* pooled, const float* cls,
                           const float* w_fc, float* dpooled, float* dw_fc, float* db_fc, float* dw_pool,
                           float* db_pool, int B, int C, int nef, void* stream);
/* y = cast(x) between f32 and dtype, n elements. */
int sba_cast(int dtype_dst, void* dst, int dtype_src, const void* src, int64_t n, void* stream);

/* R-precision ranking (evaluation; sbagan/rprecision.py).  For every image b < B: the cosine score
 * dot / max(|a| |c|, eps) of its global code cnn[b] against true_emb[b] (candidate 0) and against the M rows
 * pool[idx[b][m]] of the split's sentence-embedding pool, all f32, and
 *     rank[b] = #{ m : NOT (score_m < score_0) }
 * -- a tie counts against the image, and so does a NaN on either side.  cnn [B][nef], true_emb [B][nef], pool [P][nef]:
 * row-major, contiguous, 16-byte aligned; idx [B][M] int32 rows of pool, NOT range-checked on the device (may be NULL
 * when M == 0); rank [B]; scores [B][M + 1] (column 0 = the true caption) or NULL.  One workgroup per image, candidate
 * rows gathered by index, no intermediate, no atomics, no workspace; the lane partition and reduction order are fixed
 * and the true score takes the code path of a candidate's, so byte-identical rows give bit-identical scores (a pool row
 * equal to true_emb[b] is an exact tie).  SBA_E_ARG unless B >= 1, M >= 0, P >= 1, nef % 4 == 0, 4 <= nef <= 1024. */
int sba_rprec_rank(const float* cnn, const float* true_emb, const float* pool, const int32_t* idx, float eps,
                   int32_t* rank, float* scores, int B, int M, int nef, int P, void* stream);

/* Attention-map overlays (sbagan/visualize.py).
 * sba_vis_expand: out[i] = M x'[i] M^T for the n maps x [n][a][a] (f32) of one dump in ONE launch.  M [V][a] (f32, 16-byte
 * aligned) is the resize-then-blur operator built on the host; M == NULL (only with V == a) copies the maps.
 * x' = x where thresh == NULL, else x * (x > thresh[i]).  Also per map: mn[i] / mx[i] = min / max of out[i], and
 * conf[i] = sum of the x[i] above 2 thresh[i] (of all of x[i] where thresh == NULL).  One workgroup per map, sequential
 * f32 FMA chains of length a per product, no workspace, no atomics, fixed reduction order: two launches are bit-identical.
 * SBA_E_ARG unless 1 <= n <= 65535, 1 <= a <= 128, a <= V <= 1024.
 * sba_vis_compose: the uint8 HWC canvas [H][W][3] of an overlay image, everything but the caption text, one thread per
 * pixel.  The canvas is nS blocks stacked vertically, each a colour band of `band` rows above nr rows of V x V tiles;
 * horizontally nc cells of V + 2 columns (the tile and 2 black columns; the band's colour band_rgb[s][c] = r | g << 8 |
 * b << 16 fills the whole cell).  W == nc (V + 2), H == nS (band + nr V).  Cell (s, r, c) is desc[s][r][c] = {kind,
 * image, map, m} (int32) and par[s][r][c] = {lo, den} (f32):
 *   kind 0 black;  1 image tile: image `image & 65535` of batch `image >> 16` (img0 [n0][3][S0][S0] or img1
 *   [n1][3][S1][S1], f32 in [-1, 1]) resized to V x V (bilinear, align_corners), byte = trunc(clamp((v + 1) 127.5, 0, 255));
 *   2 map tile: gray byte = trunc(clamp(255 (E[map] - lo) / den, 0, 255)), 0 when den <= 0, E [nE][V][V] f32;
 *   3 the map byte pasted over the image byte with the constant 8-bit mask m: t = map m + img (255 - m) + 128,
 *   ((t >> 8) + t) >> 8.
 * A cell whose indices are out of range is left black (callers check them on the host). */
int sba_vis_expand(const float* x, const float* thresh, const float* M, float* out, float* mn, float* mx, float* conf,
                   int n, int a, int V, void* stream);
int sba_vis_compose(uint8_t* canvas, int W, int H, int V, int band, int nS, int nr, int nc, const int32_t* desc,
                    const float* par, const uint32_t* band_rgb, const float* E, int nE, const float* img0, int n0, int S0,
                    const float* img1, int n1, int S1, void* stream);

/* FID statistics (evaluation; sbagan/fid.py), all accumulation in float64.
 * sba_fid_accumulate: sum[D] += sum_k x[k][:] and gram[D][D] += X^T X over the n f32 feature rows x[k] (row stride ldx
 * floats), on the f64 matrix instruction; the f32 values are widened in registers (their products are exact in f64, the
 * only rounding is the f64 accumulation).  ONLY the upper-triangular 64 x 64 tiles of gram (tile row <= tile column) are
 * updated; the tiles below the diagonal are not touched.  One workgroup per tile pair does one read-modify-write of its
 * tile; no atomics, no workspace, a fixed summation order: two runs on the same input are bit-identical.  Rows >= n
 * feed 0.0, so n may be any value >= 1.  SBA_E_ARG before any launch unless n >= 1, D >= 64, D % 64 == 0, ldx >= D,
 * ldx % 4 == 0, x 16-byte aligned, sum and gram 8-byte aligned.
 * sba_fid_finalize: mu = sum / n; sigma = (gram - sum sum^T / n) / (n - 1) (the ddof = 1 covariance) as the FULL
 * symmetric [D][D] matrix, its lower triangle a bitwise copy of the upper; trace[0] = sum_i sigma_ii in a fixed order.
 * Reads only the upper triangle of gram.  SBA_E_ARG unless n >= 2, D >= 64, D % 64 == 0. */
int sba_fid_accumulate(const float* x, int n, int D, int ldx, double* sum, double* gram, void* stream);
int sba_fid_finalize(const double* sum, const double* gram, int64_t n, int D, double* mu, double* sigma, double* trace,
                     void* stream);

/* k-nearest-neighbour manifold metrics (evaluation; sbagan/prdc.py): all-pairs squared distances between
 * two sets of f32 feature rows (unit column stride, row stride ld >= D floats, ld % 4 == 0, 16-byte aligned, D a positive
 * multiple of 64) with a row-wise selection fused behind them; the na x nb matrix is never written.  All distance
 * arithmetic is float64:
 *     d2(i, j) = max((na[i] + nb[j]) - 2 g(i, j), 0)
 * g the dot product on the f64 matrix instruction over the feature axis in ascending order (the f32 values are widened in
 * registers, every product is exact), na / nb the squared norms in f64 in one fixed order.  d2(i, j) has the same bits
 * whichever tile or column split computed it, and d2(i, j) == d2(j, i) bitwise when both sets are the same rows.
 * sba_prdc_knn_radius: radius2[i] = the k-th smallest d2(i, j) over the OTHER rows j != i of x [n][D]; self is excluded
 *   by index, not by value, so a duplicate row counts at distance 0.  1 <= k <= 8, n >= k + 1.
 * sba_prdc_ball_counts: in_b[i] = #{j : d2(i, j) <= radius_b[j]} and in_own[i] = #{j : d2(i, j) <= radius_a[i]} over the
 *   rows j of b [nb][D], for every row i of a [na][D], as int32.  Either radius vector may be null: its count is then not
 *   written (and its output pointer is ignored); one of them must be given, and a given vector needs its output.
 * splits: the B range is cut into that many parts of whole 64-row tiles (one workgroup per 64 A rows and part), capped at
 *   32 and at the number of tiles; 0 = the library's choice (enough parts for 512 workgroups).  With more than one part
 *   the partial lists / counts go to `ws` (8-byte aligned, at least sba_prdc_workspace_bytes(na, nb, splits) bytes; -1
 *   for bad arguments, 0 when one part is used and ws may be null) and a second small launch merges them in part order.
 *   Results are bit-identical for every split count.  No atomics, no memset, no allocation.
 * SBA_E_ARG before any launch on a null pointer, bad D, k, n, strides, alignment, splits or a workspace too small. */
int64_t sba_prdc_workspace_bytes(int na, int nb, int splits);
int sba_prdc_knn_radius(const float* x, int n, int D, int ld, int k, int splits, double* radius2, void* ws,
                        int64_t ws_bytes, void* stream);
int sba_prdc_ball_counts(const float* a, int na, int lda, const float* b, int nb, int ldb, int D, const double* radius_a,
                         const double* radius_b, int splits, int32_t* in_b, int32_t* in_own, void* ws, int64_t ws_bytes,
                         void* stream);

/* Nearest rows of another set (evaluation; sbagan/nearest.py): for every row i of a [na][D] the k rows j of
 * b [nb][D] with the smallest (d2(i, j), j) in lexicographic order, ascending: d2 [na][k] float64 and idx [na][k] int32.
 * Rows and d2(i, j) are those of sba_prdc_* above, bit for bit (one shared tile function computes both).  A tie in d2
 * goes to the smaller j.  A NaN d2 is never listed, nor is a d2 of +inf; where b has fewer than k listable rows the tail
 * is d2 = +inf, idx = -1, so a query row that holds a NaN comes back all +inf / -1.  The key is a total order, so the
 * result has the same bits and the same indices for every tile, split count and launch.  1 <= k <= 8, na >= 1, nb >= 1.
 * splits, ws as above: with more than one part the per-part lists go to `ws` (8-byte aligned, at least
 * sba_knn_workspace_bytes(na, nb, k, splits) bytes; -1 for bad arguments, 0 when one part is used and ws may be null)
 * and a second small launch merges them under the same key.  No atomics, no memset, no allocation.
 * SBA_E_ARG before any launch, and nothing written, on a null pointer, bad D, k, n, strides, alignment (d2 8 bytes, idx
 * 4), splits or a workspace too small. */
int64_t sba_knn_workspace_bytes(int na, int nb, int k, int splits);
int sba_knn_topk(const float* a, int na, int lda, const float* b, int nb, int ldb, int D, int k, int splits, double* d2,
                 int32_t* idx, void* ws, int64_t ws_bytes, void* stream);

/* Cross-modal retrieval ranks (evaluation of the DAMSM encoders; sbagan/retrieval.py): all-pairs cosine
 * scores between two sets of f32 code rows (rows as for the k-NN metrics above) with a row-wise selection fused behind
 * them; the na x nb matrix is never written.  All score arithmetic is float64:
 *     s(i, j) = g(i, j) / max(sqrt(na[i] * nb[j]), eps)
 * g the dot product on the f64 matrix instruction over the feature axis in ascending order (the f32 values are widened in
 * registers, every product is exact), na / nb the squared norms in f64 in one fixed order, square root and division the
 * IEEE operations.  s(i, j) has the same bits whichever tile, column split or launch computed it and whichever of the
 * two sets is `a`: a threshold taken by one launch compares exactly in the next.
 * key_a [na] / key_b [nb], cls_a / cls_b: int32 vectors that are only ever compared, never used as addresses.
 * sba_retrieval_own_best: best[i] (f64) = the largest s(i, j) over the rows j of b with key_b[j] == key_a[i]; -inf when
 *   there is none, NaN when any such score is NaN.
 * sba_retrieval_counts: above[i] = #{j : key_b[j] != key_a[i] and NOT (s(i, j) < best[i])} as int32 -- a tie counts, and
 *   so does a NaN on either side; above_masked[i] = the same count over the rows j whose class also differs
 *   (cls_b[j] != cls_a[i]).  cls_a, cls_b and above_masked may be null together; then only `above` is written.
 * splits, ws: as for the k-NN metrics (whole 64-row tiles of b, 0 = the library's choice, at most 32; the partials go to
 *   `ws`, 8-byte aligned, at least sba_retrieval_workspace_bytes(na, nb, splits) bytes, and a second small launch merges
 *   them in part order: a maximum for best, a sum for the counts).  Results are bit-identical for every split count.  No
 *   atomics, no memset, no allocation.
 * SBA_E_ARG before any launch on a null pointer, bad D, strides, alignment, eps <= 0, splits, class arguments given in
 *   part, or a workspace too small. */
int64_t sba_retrieval_workspace_bytes(int na, int nb, int splits);
int sba_retrieval_own_best(const float* a, int na, int lda, const float* b, int nb, int ldb, int D, const int32_t* key_a,
                           const int32_t* key_b, double eps, int splits, double* best, void* ws, int64_t ws_bytes,
                           void* stream);
int sba_retrieval_counts(const float* a, int na, int lda, const float* b, int nb, int ldb, int D, const int32_t* key_a,
                         const int32_t* key_b, const int32_t* cls_a, const int32_t* cls_b, const double* best, double eps,
                         int splits, int32_t* above, int32_t* above_masked, void* ws, int64_t ws_bytes, void* stream);

/* Kernel Inception Distance (evaluation; sbagan/kid.py): sums of the polynomial kernel
 *     k(x, y) = (x . y / D + 1)^3
 * over pairs of gathered f32 feature rows (rows as for the k-NN metrics above), one sum per subset, in float64:
 *     sums[s] = sum over positions i < ma, j < mb (and i != j when exclude_diag) of k(a[idx_a[s][i]], b[idx_b[s][j]])
 * The dot product runs on the f64 matrix instruction over the feature axis in ascending order (the f32 values are widened
 * in registers, every product is exact); t = g / (double)D + 1.0, k = (t * t) * t.  The kernel matrix is never written.
 * idx_a [subsets][ma] / idx_b [subsets][mb]: int32 row numbers into a [na][lda] / b [nb][ldb]; a null vector means the
 *   rows 0 .. m - 1 for every subset.  An index outside [0, n) is never turned into an address: its row reads as zeros
 *   and every pair it belongs to is left out of the sum, like a position past m in the last tile.
 * exclude_diag: the pairs of EQUAL POSITION are left out (by position, never by value or by subtraction); ma == mb.
 * One launch covers all subsets: grid (blocks of 64 A positions, column splits, subsets); every workgroup adds its
 *   elements in a fixed order and writes one partial to `ws`, and a second small launch adds the partials of a subset in
 *   (block, split) order.  splits: 0 = the library's choice (enough for 512 workgroups), capped at 32 and at the number
 *   of 64-position B tiles.  ws: 8-byte aligned, at least sba_kid_workspace_bytes(ma, mb, subsets, splits) bytes (-1 for
 *   bad arguments; 0 when a subset has a single partial, which then goes to sums directly and ws may be null).
 *   The same arguments give the same bits; no atomics, no memset, no allocation.
 * SBA_E_ARG before any launch unless D >= 64, D % 64 == 0, rows 16-byte aligned, ld >= D, ld % 4 == 0, na, nb, ma, mb
 *   >= 1, 1 <= subsets <= 1024, 0 <= splits <= 32, exclude_diag only with ma == mb, sums non-null and 8-byte aligned,
 *   index vectors 4-byte aligned, and the workspace large enough. */
int64_t sba_kid_workspace_bytes(int ma, int mb, int subsets, int splits);
int sba_kid_kernel_sums(const float* a, int na, int lda, const int32_t* idx_a, int ma, const float* b, int nb, int ldb,
                        const int32_t* idx_b, int mb, int D, int subsets, int exclude_diag, int splits, double* sums,
                        void* ws, int64_t ws_bytes, void* stream);

/* Multi-scale structural similarity of image pairs (evaluation; sbagan/msssim.py): per pair, channel and
 * scale the MEAN SSIM and the MEAN contrast-structure term (cs) over the valid window positions, in float64.
 * imgs  [n][3][H][W] uint8, planar, dense, on the device;  pairs [P][2] int32 image numbers, on the device;
 * out   [P][3][scales][2] f64: {mean ssim, mean cs}.
 * Pixel values are the bytes 0 .. 255: L = 255, C1 = (0.01 L)^2, C2 = (0.03 L)^2.  The window is
 *   g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0 .. 10, normalised to sum 1 in double on the host, applied separably
 *   (along the rows, then down the columns, taps in ascending order) with NO padding.
 * Scale s (0-based) works on the image pooled s times by a 2 x 2 mean, a trailing odd row or column dropped: Hs = H >> s,
 *   Ws = W >> s.  The kernel pools from the bytes while it stages a tile (the mean of a 2^s x 2^s block of bytes is
 *   exact); no pyramid is stored.
 * Per position: mx, my, sxx = E[xx] - mx^2, syy = E[yy] - my^2, sxy = E[xy] - mx my,
 *   cs = (2 sxy + C2) / (sxx + syy + C2),  ssim = cs * (2 mx my + C1) / (mx^2 + my^2 + C1);
 *   the mean is the sum over the (Hs - 10) x (Ws - 10) positions divided by their count.
 * A pair with an image number outside [0, n) reads nothing; its 6 * scales outputs are NaN.
 * One launch per scale, grid (P * tiles of 16 x 32 positions, 3); every workgroup adds its positions in a fixed order
 *   and writes one {ssim, cs} partial to `ws`; a last small launch adds the partials of a (pair, channel, scale) in tile
 *   order and divides.  ws: 8-byte aligned, at least sba_msssim_workspace_bytes(H, W, P, scales) bytes (it does not
 *   depend on n; -1 for a refused shape).  All arithmetic is f64; the same arguments give the same bits; no atomics,
 *   no memset, no allocation.
 * SBA_E_ARG before any launch unless 1 <= scales <= 5, min(H, W) >> (scales - 1) >= 11, H, W <= 1024, n >= 1,
 *   1 <= P <= 2^20 (and P * tiles of scale 0 < 2^31), imgs non-null, pairs 4-byte aligned, out and ws 8-byte aligned and
 *   non-null, and the workspace large enough. */
int64_t sba_msssim_workspace_bytes(int H, int W, int P, int scales);
int sba_msssim_pairs(const uint8_t* imgs, int n, int H, int W, const int32_t* pairs, int P, int scales, double* out,
                     void* ws, int64_t ws_bytes, void* stream);

/* Sliced Wasserstein distance of Laplacian-pyramid patch descriptors (evaluation; sbagan/swd.py), one
 * pyramid level at a time, all arithmetic in float64.  None of the four uses atomics, a memset or an allocation; the same
 * arguments give the same bits.  SBA_E_ARG is returned before anything is launched or copied.
 *
 * sba_swd_descriptors: the 7 x 7 x 3 patch descriptors of level `level` (0 = the image itself, finest) of n square S px
 *   images, P patches an image.
 *   imgs    [n][3][S][S] uint8, planar, dense, on the device (image offsets are 64-bit);  S in {32, 64, 128, 256};
 *           levels = log2(S / 16) + 1, 0 <= level < levels; the side of the level is Sl = S >> level.
 *   centres [n * P][2] int32 {x, y} ON THE HOST: descriptor j belongs to image j / P.  Every value must lie in
 *           [3, Sl - 4]; they are checked here and then copied to `ws` on the stream.
 *   desc    [n * P][147] f64 on the device, NOT normalised: entry (c * 7 + dy) * 7 + dx = Lap[c][y - 3 + dy][x - 3 + dx].
 *   stats   [6] f64 on the device: the sums of the n * P * 49 values of channel 0, 1, 2, then the sums of their squared
 *           deviations from the channel mean stats[c] / (n * P * 49) (taken in a second pass over desc: no cancellation).
 *   Pyramid: k = (1, 4, 6, 4, 1), K = k k^T / 256; G_{l+1} = conv(G_l, K)[::2, ::2]; up(G) = conv(Z, 4 K) with Z zero
 *   except Z[::2, ::2] = G; mirror boundary WITHOUT repeating the edge sample (-1 -> 1, n -> n - 2);
 *   Lap_l = G_l - up(G_{l+1}) for l < levels - 1, Lap_{levels-1} = G_{levels-1}.  The pyramid of one (image, channel) is
 *   built in LDS as exact integers over a power of two and never written to memory, so desc is EXACT (it equals any
 *   float64 evaluation of the definition bit for bit).  One workgroup per (image, channel) adds its values in a fixed
 *   order; a small launch adds the workgroups' partial sums in image order (sums first, then the deviations alike).  All
 *   these sums carry their rounding errors along (two-sum), so each statistic is within a rounding or two of exact.
 *   ws: 8-byte aligned, on the device, at least 48 n + 8 n P bytes.
 *   SBA_E_ARG unless the pointers are non-null, centres 4-byte and desc, stats, ws 8-byte aligned, S in the set,
 *   0 <= level < levels, 1 <= n < 2^31, 1 <= P <= 4096, every centre in range and the workspace large enough.
 *
 * sba_swd_project: out[d][i] = sum_k (desc[i][k] - mu_c) / sigma_c * dirs[k][d], channel c = k / 49, with
 *   mu_c = stats[c] / (49 m), sigma_c = sqrt(stats[3 + c] / (49 m)) (the population deviation), evaluated as
 *   sum_k (desc[i][k] - mu_c) dir'[k][d] with dir'[k][d] = dirs[k][d] * (1 / sigma_c), made on the device from `stats`; the
 *   mean is taken off as a descriptor tile is staged (an offset subtracted after the contraction would cancel a digit or
 *   two where |mu| > sigma).  The contraction runs on the f64 matrix instruction, k ascending four at a time, K padded
 *   from 147 to 148 by zeros.  sigma_c = 0 gives non-finite values, never a fault.
 *   desc [m][147], stats [6], dirs [147][D], out [D][m] (direction-major), all f64 on the device, 8-byte aligned.
 *   ws: 8-byte aligned, at least 8 * 148 * D bytes.  SBA_E_ARG unless 1 <= D <= 65535, 1 <= m, D * m <= 2^40.
 *
 * sba_swd_sort_columns: sorts each of the D columns of length m of data [D][m] (f64) ascending; the result is in `data`.
 *   tmp: a second [D][m] buffer, needed (non-null, not `data`) when m > 2048, the tile that one workgroup sorts in LDS;
 *   longer columns are merged pairwise from sorted tiles.  Any m >= 1.  Values compare with <: -0 and +0 are equal and
 *   the order of NaNs is undefined (nothing is rejected).  Same limits on D and m.
 *
 * sba_swd_abs_mean: out[d] = (sum_i |a[d][i] - b[d][i]|) / m for a, b [D][m] f64: one partial sum per workgroup and chunk of
 *   4096 values, the partials of a column added in chunk order.  ws: 8-byte aligned, at least 8 * D * ceil(m / 4096)
 *   bytes.  Same limits on D and m. */
int sba_swd_descriptors(const uint8_t* imgs, int64_t n, int S, int level, const int32_t* centres, int P, double* desc,
                        double* stats, void* ws, int64_t ws_bytes, void* stream);
int sba_swd_project(const double* desc, int64_t m, const double* stats, const double* dirs, int D, double* out, void* ws,
                    int64_t ws_bytes, void* stream);
int sba_swd_sort_columns(double* data, double* tmp, int D, int64_t m, void* stream);
int sba_swd_abs_mean(const double* a, const double* b, int D, int64_t m, double* out, void* ws, int64_t ws_bytes,
                     void* stream);

/* Training batches from the device-resident image cache (sbagan/device_data.py): gather, crop, mirror,
 * every scale of the image pyramid and the normalisation in ONE launch, bit-identical to the PIL data path.
 * cache: all images back to back, each HWC uint8 [H_i][W_i][3]; offset[i] (int64): byte offset of image i; hw[i] = {H_i,
 * W_i} (int32), i < N.  params[b] = {index, x1, y1, flip} (int32), b < B: the window [y1, y1 + T) x [x1, x1 + T) of image
 * `index`, mirrored left-right when flip != 0.  out_l [B][3][T >> l][T >> l]: f32, planar, contiguous, l < levels.
 *   level 0: out0 = lut[byte], lut a 256-entry f32 table (the host builds it with the torch operations of ToTensor and
 *   Normalize, which is what makes the floats bit-equal);
 *   levels 1, 2 (factors 2, 4): each resized FROM THE LEVEL-0 CROP by PIL's 8-bit BILINEAR resampling -- the horizontal
 *   pass, the intermediate rounded to a byte, then the vertical pass; each pass byte = clip((2^21 + sum pixel k) >> 22,
 *   0, 255) in int32 -- then lut[byte].  The coefficients come from the host: tab_l [T >> l][10] = {xmin, n, k0..k7}
 *   (int32), windows clipped to the crop, n <= 8; a tap outside the crop window is never read.
 * out1 / tab1 (out2 / tab2) are ignored when levels < 2 (< 3).  A params row whose index is outside [0, N) or whose
 * window is not inside its image writes nothing for that image and reads nothing out of range.  One workgroup per 32 x 32
 * level-0 tile, no atomics, no workspace.  SBA_E_ARG before any launch on a null pointer of a level in use, or unless
 * 1 <= levels <= 3, 4 <= T <= 1024, T % (1 << (levels - 1)) == 0, 1 <= B <= 65535, N >= 1. */
int sba_batch_pyramid(const uint8_t* cache, const int64_t* offset, const int32_t* hw, int N, const int32_t* params, int B,
                      int T, int levels, const int32_t* tab1, const int32_t* tab2, const float* lut, float* out0,
                      float* out1, float* out2, void* stream);

/* The two masks of one training batch from integers already on the device, in ONE launch (sbagan/static_batch.py,
 * DESIGN.md 7g): deterministic and free of host state, so it can be recorded in front of the training step.
 * captions [B][L] int64 word ids, 0 = padding; class_ids [B] int64, compared as full 64-bit values.
 *   word_mask  [B][L] uint8: 1 where captions == 0, else 0          (sbagan.trainer.build_mask)
 *   class_mask [B][B] uint8: class_mask[i][j] = 1 where class_ids[j] == class_ids[i] and j != i, else 0
 *                                                                    (miscc.losses.class_mask)
 * Every byte written is exactly 0 or 1 and nothing outside the two outputs is written.  Grid-stride over B * L + B * B
 * elements, plain byte stores, no atomics, no LDS, no workspace.  SBA_E_ARG before any launch on a null pointer or
 * unless 1 <= B <= 65535 and 1 <= L <= 65535. */
int sba_batch_masks(const int64_t* captions, const int64_t* class_ids, uint8_t* word_mask, uint8_t* class_mask, int B,
                    int L, void* stream);

/* ---- the recorded DAMSM pre-training update (sbagan/damsm.py: DAMSMSlotStep) ----
 * What the eager update does on the host, or with host floats, done on the device so that the update can be recorded
 * once and re-issued: plain vector loads and stores, no atomics, no host synchronisation, the same bits on every run.
 *
 * Embedding -> Dropout of RNN_ENCODER's training path with the keep mask as a TENSOR (the caller draws it per batch):
 *   ids [N] int64, W [ntoken][ninput] f32, keep [N][ninput] uint8 (non-zero = kept), out / dout [N][ninput] f32,
 *   scale = float(1 / (1 - p)).  out[i][c] = keep[i][c] ? W[ids[i]][c] * scale : 0.  An id outside [0, ntoken) is
 *   compared before it indexes: its output row is zero and it adds nothing to dW.
 *   dW[id][c] += sum_{j: ids[j] == id} keep[j][c] * dout[j][c] * scale, added in increasing j by the ONE workgroup of
 *   the first position that holds the id (ids of the batch in LDS).
 * 1 <= N <= 8192, ninput % 4 == 0, W / out / dout / dW 16-byte aligned, keep 4-byte aligned; else SBA_E_ARG. */
int sba_embed_dropout_fwd(const int64_t* ids, const float* W, const uint8_t* keep, float scale, float* out, int N,
                          int ntoken, int ninput, void* stream);
int sba_embed_dropout_bwd(const int64_t* ids, const uint8_t* keep, float scale, const float* dout, float* dW, int N,
                          int ntoken, int ninput, void* stream);
/* clip_grad_norm_ over n contiguous f32 gradients, in two launches.  sba_sqnorm_partials: nparts workgroups (1..1024),
 * each writes ONE f64 = the sum of g^2 over the elements it visits (the square in f32, the sum in f64, folded in LDS in
 * a fixed order).  sba_clip_adam_prepare: one workgroup adds the partials in index order in f64 and writes
 * out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6)) (both f32); then sba_adam_prepare's work on `state` with the
 * learning rate READ from lr_dev (one f32 in device memory). */
int sba_sqnorm_partials(const float* g, int64_t n, double* partials, int nparts, void* stream);
int sba_clip_adam_prepare(void* state, const double* partials, int nparts, const float* lr_dev, float max_norm,
                          float beta1, float beta2, float* out, void* stream);
/* sba_adam_step with the gradient scale read from device memory when the kernel runs (grad_scale_dev: one f32, e.g.
 * out + 1 of sba_clip_adam_prepare; NULL = 1): the same kernel body, bit-identical to sba_adam_step for the same scale. */
int sba_adam_step_dscale(float* p, const float* g, float* m, float* v, float* avg, void* shadow, const void* state,
                         int64_t n, float beta1, float beta2, float eps, const float* grad_scale_dev, void* stream);

/* Differentiable Augmentation of the images a discriminator sees (Zhao et al., NeurIPS 2020, policy
 * color,translation,cutout; csrc/diffaug.hip, sbagan/ops.py: DiffAugFn).  Images are f32 NCHW [n][3][S][S],
 * contiguous, 16-byte aligned.  params [n][8] f32: row n holds seven uniforms u0..u6 in [0, 1) (column 7 is unused).
 * flags: 1 color | 2 translation | 4 cutout; a part that is off is skipped.
 *   color        x + (u0 - 0.5);  (x - mean_c x) * (2 u1) + mean_c x;  (x - mean_chw x) * (u2 + 0.5) + mean_chw x
 *   translation  shift = int(S / 8 + 0.5), ty = min(int(u3 * (2 shift + 1)), 2 shift) - shift (product in f32), tx from u4;
 *                out[i][j] = in[i + ty][j + tx] inside the image, +0.0 elsewhere
 *   cutout       cut = int(S / 2 + 0.5), oy = min(int(u5 * (S + 1 - cut % 2)), S - cut % 2), ox from u6; output rows
 *                [oy - cut / 2, oy - cut / 2 + cut) and the same columns, intersected with the image, are +0.0
 * With color off every output element is a bit-exact copy of an input element or +0.0.
 * sba_diffaug_fwd: out [(nr + nf)] = the transform of [real (nr images) | fake (nf images)] -- the concatenation and the
 *   augmentation in one pass; real may be NULL with nr = 0.
 * sba_diffaug_bwd: dx [n] = the gradient of the n inputs for the output gradient dout [n] (the map is affine in x: no saved
 *   input).  With color off dx is the exact scatter of dout.
 * workspace: sba_diffaug_workspace_bytes(n, S) bytes (n = nr + nf), 8-byte aligned, needed with color on only: the f64
 *   partial sums of the per-image reductions, added in a fixed order that depends on S alone.  No atomics; two calls
 *   give the same bits.  Per-element math is f32.
 * SBA_E_ARG before any launch unless 8 <= S <= 4096, S even, 1 <= flags <= 7, nr, nf >= 0, 1 <= nr + nf <= 65535, and
 * on a needed pointer that is NULL or misaligned. */
int64_t sba_diffaug_workspace_bytes(int n, int S);
int sba_diffaug_fwd(const float* real, int nr, const float* fake, int nf, const float* params, float* out, int S,
                    int flags, void* workspace, void* stream);
int sba_diffaug_bwd(const float* dout, int n, const float* params, float* dx, int S, int flags, void* workspace,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SBAGAN_HIP_H */
