/*
 * ammc_hip.h - C ABI of libammc_hip.so: the MI355X (gfx950) kernels behind the
 * appearance-motion memory-consistency network's forward()/backward().
 *
 * The reference (NjuHaoZhang/AMMCNet_AAAI2021) has no native code: its hot
 * path is `twostream.forward` (Code/models/unet.py:981-1007) executed by
 * torch.nn modules on cuDNN/ATen.  Every entry below replaces the ATen/cuDNN
 * call(s) named in its comment; the Python host
 * (ammcnet_aaai2021_amd/unet.py) keeps the reference's nn.Module interface and
 * state_dict layout and binds these symbols with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers unless stated;
 *   - every entry takes the hipStream_t to launch on (as void*), launches
 *     asynchronously, allocates nothing and never synchronises;
 *   - return 0 on success, a negative AMMC_E* code on bad arguments, or the
 *     positive hipError_t of a failed launch; never abort();
 *   - activations inside the path are fp32 NHWC ("pixel-major"); tensors that
 *     feed a 3x3 convolution carry a one-pixel zero halo:
 *     [B][H+2][W+2][C].  Strides below are in ELEMENTS.
 */
#ifndef AMMC_HIP_H
#define AMMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMMC_OK 0
#define AMMC_EINVAL (-1)   /* bad shape / alignment / null pointer   */
#define AMMC_EUNSUP (-2)   /* shape not supported by any kernel tile */

#define AMMC_ACT_NONE 0
#define AMMC_ACT_RELU 1
#define AMMC_ACT_TANH 2
#define AMMC_ACT_LRELU 3   /* nn.LeakyReLU(0.1), pix2pix_networks.py:606 */

/* library / device identification ---------------------------------------- */
int ammc_abi_version(void);                    /* bumps on any signature change */
/* "file=digest,file=digest,..." (sha256[:12]) of the source files the library was compiled from; profiles/ files carry
 * the same map and bench.py quotes a profiled figure of a kernel only while the kernel's file, ammc_common.h and this
 * header are unchanged ("" for a library built outside ammcnet_aaai2021_amd/build.py) */
const char* ammc_source_digests(void);
const char* ammc_build_info(void);             /* "gfx950 ..." */
const char* ammc_error_string(int code);
/* Dispatch options, for A/B measurements and for tests that must reach every kernel instance:
 *   "s16_mf"  MFMA shape of the halo-patch kernel (conv_tap_s16<..., MF>): -1 = the measured faster one per
 *             variant (default), 1 = v_mfma_f32_16x16x32_f16, 0 = v_mfma_f32_32x32x16_f16.  Initial value: AMMC_S16_MF.
 *   "outc_stream"  1 = the output layer (32-filter tile, fp32 NCHW output) on the streaming kernel conv_outc_s16
 *             (default), 0 = on the halo-patch kernel.  Initial value: AMMC_OUTC_STREAM.
 *   "memory_rt"  feature rows per workgroup of ammc_memory_topk_fwd_s16: 0 = by size (64 from 16384 rows up, k <= 2,
 *             m <= 2048; default), 1 = 32, 2 = 64.  Results are bit-identical.  Initial value: AMMC_MEMORY_RT.
 *   "memory_split"  ammc_memory_topk_fwd_f16: -1 / 0 = one fused launch (default), 1 = the contraction runs in chunks of
 *             whole rounds of workgroups on the caller's stream and the HBM-bound gather / commit of each chunk on a
 *             second, library-owned stream beside the next chunk's contraction (the caller's stream waits for it before
 *             the call's successors run; measured 1 % faster at 262144 rows).  Initial value: AMMC_MEMORY_SPLIT.
 * Returns AMMC_EUNSUP for an unknown key, AMMC_EINVAL for a value out of range.  These are PROCESS defaults
 * (not thread safe against concurrent launches); a caller that needs a per-call choice sets the descriptor fields
 * `s16_mf` / `outc_stream` instead, which take precedence and touch no global state. */
int ammc_set_option(const char* key, int32_t value);

/*
 * Implicit-GEMM convolution on the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32):
 *   y[m, n] = act( scale[n] * sum_k A[m, k] * Wp[n, k] + shift[n] ) + res[m, n]
 * m runs over the B*H*W pixels, k = tap*Cin + c over `ntaps` (1 or 9) window
 * taps and Cin channels; A is gathered on the fly from the NHWC input.
 *
 * Replaces, by mode:
 *   ntaps=9            nn.Conv2d(3x3, pad 1, bias=False) + BatchNorm2d(eval) + ReLU
 *                      (unet.py:11-16, `double_conv`), the AMFT residual add
 *                      (unet.py:962-965) through `res`
 *   ntaps=1            nn.Conv2d 1x1 + bias, `enc`/`dec` (unet.py:321-330) and
 *                      `out += x` (unet.py:386) through `res`
 *   ntaps=9, n=32, n_store=cout, act=TANH, NCHW strides
 *                      `outc` + torch.tanh (unet.py:920, 998-1007): the 2-3 output channels
 *                      ride in a 32-wide MFMA column tile
 *   ntaps=4, x_step=2  gradient of that ConvTranspose2d w.r.t. its input (autograd of unet.py:51)
 *   ntaps=9 on dY with the flipped/transposed filter: gradient of the 3x3 conv w.r.t. its input
 *   ntaps=1, up=2      nn.ConvTranspose2d(C, C/2, 2, stride 2) + bias (unet.py:47,51):
 *                      N = 4*cgroup columns, column n = (dy*2+dx)*cgroup + co is
 *                      scattered to pixel (2y+dy, 2x+dx); writing into a channel
 *                      slice of the concat buffer replaces torch.cat (unet.py:57)
 */
typedef struct AmmcConvDesc {
  const float* x;        /* input, offset to tap (0,0) of pixel (0,0,0), channel 0        */
  const float* w;        /* packed weights [N][Kpad], Kpad = roundup(ntaps*Cin, 32)       */
  float* y;              /* output, offset to pixel (0,0,0) (+halo) and channel offset     */
  const float* scale;    /* [N] or NULL (=1)                                              */
  const float* shift;    /* [N] or NULL (=0)                                              */
  const float* res;      /* residual added after the activation, or NULL (S16 kernels: S16, or fp32 NHWC when y_f32) */
  int32_t batch, height, width;        /* pixel space of m                               */
  int32_t cin;           /* channels per tap: power of two >= 4                           */
  int32_t ntaps;         /* 9 (3x3, pad 1 via the halo), 4 (2x2, see x_step), 16 (4x4) or 1 */
  int32_t n;             /* GEMM N: 32, or a multiple of 64                               */
  int32_t up;            /* 1, or 2 for the ConvTranspose scatter                         */
  int32_t cgroup;        /* channels per (dy,dx) group when up=2 (multiple of 32); else n */
  int32_t act;           /* AMMC_ACT_*                                                    */
  int32_t n_store;       /* columns actually stored (0 = all n); lets a small-N layer pad N to 32 */
  int64_t x_bs, x_rs, x_ps;            /* input batch / row / pixel strides              */
  int64_t y_bs, y_rs, y_ps;            /* output strides (of the OUTPUT resolution)      */
  int64_t r_bs, r_rs, r_ps;            /* residual strides                               */
  int64_t y_cs;          /* output channel stride: 0/1 = NHWC; H*W (with y_ps=1, y_rs=W) = NCHW    */
  int32_t x_step;        /* 0/1; 2 = the input is at twice the resolution of m (with ntaps=4: the  */
  int32_t y_f32;         /* (2x2 stride-2 gather of the ConvTranspose dgrad).  y_f32: ammc_conv_gemm_s16 only, 1 = fp32 output */
  int32_t s16_mf;        /* ammc_conv_gemm_s16 only, per CALL (re-entrant): 0 = the process default (ammc_set_option "s16_mf"), 1 = v_mfma_f32_32x32x16_f16, */
  int32_t outc_stream;   /* 2 = v_mfma_f32_16x16x32_f16 forced.  outc_stream: 0 = process default, 1 = halo-patch kernel, 2 = streaming kernel */
  int32_t* overflow_flag; /* ammc_conv_gemm_s16 only, may be NULL: set to 1 when an S16 output exceeds the half range */
  float* splitk_ws;      /* ammc_conv_gemm_s16 only, may be NULL: fp32 workspace that lets small-M layers split K    */
  int64_t splitk_ws_floats; /* over workgroups ([ksplit][M][N] partial tiles + a finishing kernel)                   */
  const float* sq_target; /* fp32-output epilogues only (outc), may be NULL: a tensor laid out like y; the kernel adds   */
  float* sq_acc;          /* sum(((t+1)/2 - (y+1)/2)^2) of every stored element to sq_acc[sample] (fp32 atomics): the  */
                          /* per-sample squared error of `psnr_error` (utils/utils.py:141-148) without re-reading y     */
  float* pool_y;          /* ammc_conv_gemm_s16, S16 3x3 layers that its halo-patch kernel serves (Cin % 32 == 0, W % 32  */
  int64_t pool_bs, pool_rs, pool_ps; /* == 0, H % 8 == 0, >= 192 patches; no residual), may be NULL: also store the 2x2   */
                          /* max-pooled output (nn.MaxPool2d(2) of the `down` block that follows, unet.py:36) at half     */
                          /* resolution; AMMC_EUNSUP when the layer is not that kernel's                                  */
  float* stats;           /* ammc_conv_gemm_s16, fp32 outputs, may be NULL: per-channel sum and sum of squares of the STORED    */
                          /* values of every output patch, stats[patch][2][n] - the partial rows ammc_bn_finalize_f32 combines */
                          /* (training-mode BatchNorm2d statistics, models/unet.py:12,15, without re-reading the tensor);      */
                          /* rows = ammc_conv_gemm_s16_stats_rows(desc), AMMC_EUNSUP when that is 0                            */
  const float* bn_c;      /* with `stats`, may be NULL: the output is the gradient of a BatchNorm(+ReLU) unit's output and the  */
  int64_t bn_bs, bn_rs, bn_ps; /* statistics are those of that unit's BACKWARD (autograd through models/unet.py:12-16):         */
  const float *bn_mean, *bn_invstd, *bn_scale, *bn_shift; /* stats[patch][4][n] = sum g, sum g xhat, max |g|, max |xhat| with   */
  int32_t bn_relu;        /* g = y [bn_relu == 0 or bn_c scale + shift > 0], xhat = (bn_c - mean) invstd; bn_c = the unit's     */
  int32_t reserved0;      /* saved convolution output at the same pixels (own strides), scale / shift its folded BatchNorm:    */
                          /* the rows ammc_bn_bwd_finalize_f32 combines, without ammc_bn_bwd_reduce_bound_f32's pass            */
} AmmcConvDesc;

int ammc_conv_gemm_f32(const AmmcConvDesc* desc, void* stream);

/* nn.MaxPool2d(2) (unet.py:36) on NHWC; input strides explicit (the skip tensor lives in
 * the concat buffer), output strides explicit (halo-padded). h,w are OUTPUT sizes. */
int ammc_maxpool2x2_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps,
                        float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps,
                        int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);

/* module-boundary layout change: NCHW fp32 [B,C,H,W] -> NHWC with explicit strides
 * (y points at pixel (0,0), i.e. inside the halo; channels c..cp-1 are written as zero,
 * cp % 4 == 0).  Writing into a channel slice of a wider buffer is allowed. */
int ammc_nchw_to_nhwc_f32(const float* x, int32_t batch, int32_t c, int32_t h, int32_t w,
                          float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t cp, void* stream);
/* NHWC (strided) -> NCHW, for tensors handed back across the module boundary */
int ammc_nhwc_to_nchw_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps,
                          int32_t batch, int32_t c, int32_t h, int32_t w, float* y, void* stream);
/* zero the one-pixel border of a [B][H+2][W+2][C] buffer */
int ammc_zero_halo_f32(float* y, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);

/* weight pre-packing (run once per load_state_dict / optimizer step) ------ */
/* OIHW [cout][cin][kh][kw] (kh=kw=3 or 1) -> [cout][Kpad], k = (r*kw+s)*cin_p + c */
int ammc_pack_conv_weight_f32(const float* w_oihw, int32_t cout, int32_t cin, int32_t ksize,
                              int32_t cin_p, float* out, void* stream);
/* ConvTranspose2d IOHW [cin][co][2][2] -> [4*co][cin], row (dy*2+dx)*co + c_out */
int ammc_pack_convt_weight_f32(const float* w_iohw, int32_t cin, int32_t co, float* out, void* stream);
/* eval-mode BatchNorm2d folded to y = scale*x + shift (unet.py:12,15) */
int ammc_bn_fold_f32(const float* gamma, const float* beta, const float* mean, const float* var,
                     float eps, int32_t c, float* scale, float* shift, void* stream);
/* codebook [D][M] -> slot-major [M][D] plus |E_m|^2 (unet.py:287, 315-316) */
int ammc_pack_codebook_f32(const float* embed_dm, int32_t d, int32_t m, float* embed_md,
                           float* enorm, void* stream);

/*
 * Memory addressing, forward (`Quantize_topk.forward`, unet.py:282-297, 310-313):
 * squared-L2 distance of each of n feature vectors x[n][d] to the m slots,
 * the k nearest slots (nearest first), their rows gathered and concatenated
 * into q_topk[n][k*d], q_one[n][d] = x + (E[i1]-x), and per-block partial
 * sums of (E[i1]-x)^2 written to diff_partial[ammc_memory_topk_blocks(n)].
 * embed_dm is the module's own buffer [d][m]; embed_md / enorm come from
 * ammc_pack_codebook_f32.  d in {64,128,192,256}, k <= 4, q_one may be NULL.
 * The n x m distance matrix never reaches HBM.
 */
int ammc_memory_topk_blocks(int32_t n);
int ammc_memory_topk_fwd_f32(const float* x, const float* embed_dm, const float* embed_md,
                             const float* enorm, int32_t n, int32_t d, int32_t m, int32_t k,
                             int32_t* idx_topk, float* q_topk, float* q_one,
                             float* diff_partial, void* stream);
/* The same memory addressing with the distance GEMM on the fp16 MFMA pipe in fp32-EQUIVALENT arithmetic (features and
 * slots as (hi, lo) half pairs, three MFMAs per product, fp32 accumulation; norms, gather, commit distance from the fp32
 * data as in ammc_memory_topk_fwd_f32): the inference default for the model's embed_dim = 64 (d != 64: AMMC_EUNSUP, use
 * the fp32 entry).  e_s16 = ammc_pack_codebook_s16(embed [d][m]): [d/8][hi | lo][mpad][8] halfs (opaque to callers), mpad = m rounded up
 * to 32; enorm / embed_md from ammc_pack_codebook_f32; diff_partial has ammc_memory_topk_blocks(n) entries. */
int ammc_pack_codebook_s16(const float* embed_dm, int32_t d, int32_t m, void* e_s16, void* stream);
/* ... and with a range verdict: *range_flag (device int32, zeroed by the caller, sticky) is raised when an entry of the
 * codebook does not fit the hi half (|v| > 65504 or not finite).  The reference's own EMA update (models/unet.py:298-309)
 * produces such entries from its initial state (:277-280: cluster_size = 0): a slot no row has hit yet sits at
 * embed = 0.99^t e0 / ~1e-5 ~ 1e5 x N(0, 1) for the first ~150 training steps.  A flagged codebook must be looked up with
 * ammc_memory_topk_fwd_f32 (an inf / NaN slot of the S16 image corrupts the ranking). */
int ammc_pack_codebook_s16_guarded(const float* embed_dm, int32_t d, int32_t m, void* e_s16, int32_t* range_flag, void* stream);
int ammc_memory_topk_fwd_s16(const float* x, const void* e_s16, const float* embed_md, const float* enorm, int32_t n,
                             int32_t d, int32_t m, int32_t k, int32_t* idx_topk, float* q_topk, float* q_one,
                             float* diff_partial, void* stream);

/* The whole memory block of the inference path as ONE launch (`enc_quan_dec_res_topk.forward`, models/unet.py:318-331,
 * 379-387): enc 1x1 (c -> d, + enc_b) -> distances + top-k (ammc_memory_topk_fwd_s16's arithmetic) -> gather -> dec 1x1
 * (k d -> c, + dec_b) -> += x, for 64-pixel tiles; z, the n x m distances and the gathered rows never leave the CU.
 * x / y: S16 activations [batch][h][w][c] (pointer to interior pixel 0, strides in floats); enc_w [d][c], dec_w [c][k d]:
 * ammc_pack_conv_weight_f32 (ksize 1) + ammc_split_rows_f32; e_s16 / embed_md / enorm as for ammc_memory_topk_fwd_s16.
 * Outputs: y, idx_topk [n][k], q_one [n][d] (may be NULL), q_topk [n][k d] fp32 (may be NULL), diff[0] = commit
 * distance (the LAST workgroup sums diff_partial[ammc_memory_topk_blocks(n)] in ammc_sum_partials_f32's order; *counter
 * is a device int32 the caller zeroes ONCE - the kernel leaves it at zero), *overflow_flag raised like the S16 epilogues
 * and ammc_split_rows_guarded_f32 do.  Bit-identical to the five-launch chain it replaces (same k order and expressions).
 * dec_wf is dec_w in FRAGMENT-major order (ammc_pack_frag_rows_s16 below).
 * Shapes: d = 64, k = 2, c = 512, m <= 2048 (the shipped block; otherwise AMMC_EUNSUP: use the chain). */
int ammc_memory_block_s16(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, float* y, int64_t y_bs, int64_t y_rs,
                          int64_t y_ps, int32_t batch, int32_t h, int32_t w, int32_t c, const float* enc_w, const float* enc_b,
                          const void* e_s16, const float* embed_md, const float* enorm, int32_t d, int32_t m, int32_t k,
                          const float* dec_wf, const float* dec_b, int32_t* idx_topk, float* q_topk, float* q_one,
                          float* diff_partial, float* diff, int32_t* counter, int32_t* overflow_flag, void* stream);
/* S16 filter rows [n][k] (ammc_pack_conv_weight_f32 + ammc_split_rows_f32; n % 32 == 0, k % 8 == 0) -> fragment-major
 * [k/8][hi | lo][n][8 halfs], the rows of every 32-row tile in MFMA order: what a lane of ammc_memory_block_s16's dec
 * phase reads is then 16 bytes of a 512-byte run shared with its 31 neighbours.  Same size in bytes. */
int ammc_pack_frag_rows_s16(const float* w_s16, int32_t n, int32_t k, float* out, void* stream);

/* diff = sum(partials) / count, fixed order (deterministic) */
int ammc_sum_partials_f32(const float* partial, int32_t nparts, float inv_count, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * "S16": fp32-equivalent arithmetic on the fp16 MFMA pipe.  A value v is the pair of halfs
 * hi = half(v), lo = half((v-hi)*2^11); tensors are NHWC with channels in groups of 8, each group
 * 32 bytes [8 hi | 8 lo] (4 B/element: strides in ELEMENTS are those of the fp32 layout).
 * ammc_conv_gemm_s16 takes the same descriptor as ammc_conv_gemm_f32 with x, w and res in S16
 * and computes a*b as hi*hi + (hi*lo + lo*hi)*2^-11 with three v_mfma_f32_32x32x16_f16 and fp32
 * accumulation; y is S16 unless y_f32 = 1 (then n_store / y_cs / TANH and an fp32 residual are available; up = 2
 * only without them).  Replaces the same reference calls as ammc_conv_gemm_f32.
 * ---------------------------------------------------------------------------------------- */
int ammc_conv_gemm_s16(const AmmcConvDesc* desc, void* stream);
/* `up.forward` of the decoder in inference (models/unet.py:50-59) as one launch: y = act(scale * conv3x3(cat([skip,
 * ConvTranspose2d(x2, k 2, s 2) + b])) + shift).  desc describes the 3x3 conv over the SKIP half only: x = the skip
 * tensor (S16, halo corner), cin = c skip channels, w = the S16 filter of the whole conv ([n][9 * 2c], k = tap * 2c +
 * ch: ammc_pack_conv_weight_f32 + ammc_split_rows_f32), scale, act, y (S16); desc->shift is ignored.  The other half
 * comes from x2 (S16, half resolution, halo 1, up_cin = 2c channels: what the transposed conv reads) through the
 * COMPOSED filters of ammc_pack_up_conv_f32 (the transposed conv folded into the 3x3 taps per output-pixel parity,
 * summed in double: no intermediate tensor; then ammc_split_rows_f32) and its border-class shifts shift9[3][3][n].
 * Needs W % 32 == 0, H % 8 == 0, c % 32 == 0, n = 64 or a multiple of 128; AMMC_EUNSUP otherwise (callers then run
 * the transposed conv and the 3x3 conv separately). */
int ammc_pack_up_conv_f32(const float* w3_oihw, const float* wt_iohw, const float* bt, const float* scale,
                          const float* shift, int32_t n, int32_t c, float* w2_out, float* shift9_out, void* stream);
int ammc_conv_up_s16(const AmmcConvDesc* desc, const float* up_x, int64_t up_bs, int64_t up_rs, int64_t up_ps,
                     int32_t up_cin, const float* up_w, const float* shift9, void* stream);
/* The first layer of a stream in inference (`inconv`'s first conv + BatchNorm(eval) + ReLU, models/unet.py:11-13, 23-30)
 * straight from the module-boundary tensor: x is NCHW fp32 [batch][c <= 16][h][w] (zero padding applied by the kernel),
 * y the S16 NHWC activation (64 channels, pixel (0,0), strides in elements).  Replaces ammc_nchw_to_s16_f32 +
 * ammc_conv_gemm_s16 for that layer.  w_image = ammc_pack_first_conv_f32(OIHW [64][c][3][3]) (ammc_first_conv_image_floats()
 * floats).  Needs w % 32 == 0, h % 8 == 0; AMMC_EUNSUP otherwise. */
int ammc_first_conv_image_floats(void);
int ammc_pack_first_conv_f32(const float* w_oihw, int32_t cout, int32_t cin, float* out, void* stream);
int ammc_conv_first_s16(const float* x_nchw, int32_t batch, int32_t c, int32_t h, int32_t w, const float* w_image,
                        const float* scale, const float* shift, int32_t act, float* y, int64_t y_bs, int64_t y_rs,
                        int64_t y_ps, int32_t* overflow_flag, void* stream);
/* The same with an explicit batch stride of x (elements; c * h * w = contiguous).  The evaluation loop's clips are
 * OVERLAPPING windows of one resident sub-video - clip b = frames [s + b, s + b + 4) of a [T][3][h][w] tensor
 * (test_helper.py:433-438: `view(B, t * c, H, W)` of consecutive frames) - so x = &frames[s], x_bs = 3 * h * w runs a batch
 * of 16 clips without first gathering 16 x 12 planes into a contiguous tensor (harness.score_batch_device). */
int ammc_conv_first_s16_bs(const float* x_nchw, int64_t x_bs, int32_t batch, int32_t c, int32_t h, int32_t w,
                           const float* w_image, const float* scale, const float* shift, int32_t act, float* y,
                           int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t* overflow_flag, void* stream);
/* Which kernel ammc_conv_gemm_s16 launches for this descriptor, as the NUL-terminated name rocprofv3 reports for it
 * (e.g. "conv_tap_s16<4, 1, 2, 4, 1>", "conv_gemm_s16<128x128>", "...+splitk4"), without launching anything: the same
 * argument checks and the same dispatch code run with the launch replaced by the label.  Tests pin kernel coverage on
 * it and bench.py labels its per-kernel timings with it. */
int ammc_conv_gemm_s16_variant(const AmmcConvDesc* desc, char* out, int32_t out_len);
/* Rows of `desc->stats` the kernel ammc_conv_gemm_s16 would launch for this descriptor writes (one per 8 x 32 output
 * patch), or 0 when that kernel has no statistics epilogue (the caller then runs ammc_bn_stats_f32 on the output as
 * before).  `desc->stats` itself is ignored here.  Same argument checks and dispatch code as the launch. */
int ammc_conv_gemm_s16_stats_rows(const AmmcConvDesc* desc);
/* fp32 -> S16, count elements (multiple of 8): packed filters, gathered codebook rows */
int ammc_split_rows_f32(const float* src, int64_t count, float* dst, void* stream);
/* ... and with a range verdict: *range_flag (device int32, sticky; the same flag the S16 epilogues raise through
 * AmmcConvDesc.overflow_flag) is raised when a value does not fit the hi half (|v| > 65504 or not finite): the S16 image
 * would hold inf there.  range_flag may be NULL (= ammc_split_rows_f32). */
int ammc_split_rows_guarded_f32(const float* src, int64_t count, float* dst, int32_t* range_flag, void* stream);
/* Gradient tensors as S16 operands (what autograd derives for the 3x3 convs, train_helper.py:337-339): the largest
 * |v| of the tensor as its fp32 bit pattern (atomicMax into one of the 256 slots out_bits[0..256), zeroed by the
 * caller; the consumer takes the maximum of the slots), then the split of
 * v * 2^k with k chosen so that the maximum lands at 2^10; inv_scale[0..n) = 2^-k is the epilogue scale of the
 * convolution that consumes the tensor. */
int ammc_absmax_bits_f32(const float* src, int64_t count, int32_t* out_bits, void* stream);
int ammc_split_rows_scaled_f32(const float* src, int64_t count, float* dst, const int32_t* amax_bits, float* inv_scale,
                               int32_t n, void* stream);
/* module-boundary layout: NCHW fp32 -> S16 NHWC (cp % 8 == 0) and back */
int ammc_nchw_to_s16_f32(const float* x, int32_t batch, int32_t c, int32_t h, int32_t w, float* y,
                         int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t cp, void* stream);
int ammc_s16_to_nchw_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t c,
                         int32_t h, int32_t w, float* y, void* stream);
/* nn.MaxPool2d(2) on S16 tensors */
int ammc_maxpool2x2_s16(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, float* y, int64_t y_bs,
                        int64_t y_rs, int64_t y_ps, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);

/* ... that also records, for every pooled element, which of the four window positions (row-major, the first maximum)
 * it came from: idx[batch][h][w][c], a byte each (8-byte aligned) - what ammc_maxpool2x2_bwd_idx_f32 routes gradients by */
int ammc_maxpool2x2_s16_idx(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, float* y, int64_t y_bs,
                            int64_t y_rs, int64_t y_ps, uint8_t* idx, int32_t batch, int32_t h, int32_t w, int32_t c,
                            void* stream);

/* fp16-operand form of the memory addressing for large memories (BASELINE.json config 5: 8192
 * slots x 512-d): distance GEMM on v_mfma_f32_32x32x16_f16 with fp32 accumulation, everything
 * else as ammc_memory_topk_fwd_f32 (gather / q_one / commit distance from the fp32 codebook).
 * Not the parity path: the ranking sees fp16-rounded operands.  d in {128,256,384,512}, k <= 4.
 * e_kblk_f16: [d/8][roundup(m,32)][8] halfs from ammc_pack_codebook_f16 (which also returns
 * |half(E_s)|^2); diff_partial has ammc_memory_topk_f16_blocks(n) entries. */
int ammc_pack_codebook_f16(const float* embed_dm, int32_t d, int32_t m, void* e_kblk_f16, float* enorm16,
                           void* stream);
int ammc_memory_topk_f16_blocks(int32_t n);
int ammc_memory_topk_fwd_f16(const float* x, const void* e_kblk_f16, const float* embed_md, const float* enorm16,
                             int32_t n, int32_t d, int32_t m, int32_t k, int32_t* idx_topk, float* q_topk,
                             float* q_one, float* diff_partial, void* stream);

/* The same operator with the feature ROWS resident in registers and the codebook streamed through LDS (round 5; what
 * config 5 runs): a wave keeps 3 x 32 rows x d features as fp16 MFMA operands in its VGPRs for a whole sweep of the
 * codebook, the codebook goes L2 -> LDS once per workgroup (tile images of ammc_pack_codebook_f16_tiles:
 * ammc_codebook_f16_tiles_bytes(d, m) bytes, 16-byte aligned) instead of L2 -> registers once per 128 rows.  Same
 * outputs and arithmetic contract as ammc_memory_topk_fwd_f16 (ranking from fp16-rounded operands with fp32
 * accumulation - key x.E_s - |E_s|^2 / 2; gather / q_one / commit from the fp32 codebook and features).  Exact ties
 * (k = 2, d >= 288: the packed-key form): two returned slots whose keys tie come in slot order; WHICH of several exactly
 * tied candidates takes the last place of the top-k is unspecified (other shapes: ties to the lower slot throughout);
 * q_one may be NULL; diff_partial has ammc_memory_topk_f16r_blocks(n) = ceil(n / 32) entries, each written
 * once (no atomics: deterministic).  d in {128,256,384,512}, k <= 4; pointers 16-byte aligned. */
int64_t ammc_codebook_f16_tiles_bytes(int32_t d, int32_t m);
int ammc_pack_codebook_f16_tiles(const float* embed_dm, int32_t d, int32_t m, void* tiles, void* stream);
int ammc_memory_topk_f16r_blocks(int32_t n);
int ammc_memory_topk_fwd_f16r(const float* x, const void* tiles, const float* embed_md, int32_t n, int32_t d, int32_t m,
                              int32_t k, int32_t* idx_topk, float* q_topk, float* q_one, float* diff_partial,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * Training mode (autograd of the same path; the reference derives these with torch.autograd)
 * ---------------------------------------------------------------------------------------- */

/* Weight gradient dWp[n][k] += sum_m G[m][n] * A[m, k], packed layout of ammc_conv_gemm_f32's
 * weights (the caller zeroes dw; partial tiles are combined with fp32 atomics).
 *   3x3 conv:      g = gradient of the raw conv output (pixel (0,0)), a = conv input (tap (0,0))
 *   1x1 conv:      ntaps 1
 *   ConvTranspose: g = layer input, a = output gradient at 2x resolution (a_step 2, ntaps 4),
 *                  rows = input channels, k = (dy*2+dx)*co + c_out
 * zeros: >= 128 floats of zeros (source of out-of-range pixels).  n % 32 == 0. */
typedef struct AmmcWgradDesc {
  const float* g;
  const float* a;
  float* dw;
  const float* zeros;
  int32_t batch, height, width;     /* pixel space of m (resolution of g)                     */
  int32_t n;                        /* rows of dWp                                            */
  int32_t cin;                      /* channels per tap of the a side                         */
  int32_t ntaps;                    /* 9, 4 or 1                                              */
  int32_t a_step;                   /* 0/1, or 2                                              */
  int32_t reserved;
  int64_t g_bs, g_rs, g_ps;
  int64_t a_bs, a_rs, a_ps;
} AmmcWgradDesc;
int ammc_conv_wgrad_f32(const AmmcWgradDesc* desc, void* stream);
/* the same with S16 operands (g, a: the S16 twins of the fp32 tensors, same strides): fp16 MFMA with transposed LDS
 * fragment reads; g_inv_scale (device, may be NULL): the power-of-two that ammc_split_rows_scaled_f32 left in g (or in
 * a: it is one scalar on the result), divided out.  ntaps 9 (the stride-1 3x3 layers: halo-patch kernels), 16 (4x4,
 * a_step 1 | 2: PixelDiscriminator) or 4 (2x2, a_step 2: ConvTranspose); cin a power of two >= 8, n % 32 == 0. */
int ammc_conv_wgrad_s16(const AmmcWgradDesc* desc, const float* g_inv_scale, void* stream);
/* The 3x3 form with the split partials SUMMED INTO THE PARAMETER GRADIENT by a second kernel (round 5): every workgroup of
 * the halo-patch weight-gradient kernel stores its tile of the packed gradient into the slab of its patch split
 * (slabs: [splits][n][kpad] floats of caller workspace, plain stores) and a reduce kernel writes dw_oihw [cout][cin][3][3]
 * (cout <= n, cin <= desc->cin: the unpadded channel counts) - replaces ammc_conv_wgrad_s16's fp32 atomics into a zeroed
 * packed buffer + ammc_unpack_conv_wgrad_f32; fixed summation order, so deterministic.  desc->dw is not used.
 * ammc_conv_wgrad_s16_slab_floats: the workspace this descriptor needs, or 0 when its kernel has no slab form (callers
 * then use ammc_conv_wgrad_s16). */
int64_t ammc_conv_wgrad_s16_slab_floats(const AmmcWgradDesc* desc);
int ammc_conv_wgrad_s16_slabs(const AmmcWgradDesc* desc, const float* g_inv_scale, float* slabs, int64_t slab_floats,
                              float* dw_oihw, int32_t cout, int32_t cin, void* stream);
/* Which kernel ammc_conv_wgrad_s16 launches for this descriptor, as the NUL-terminated name of the instance
 * ("wgrad_tap3_s16<2, 2, 2, 2, 1, 1>", "wgrad_tap3_s16<1, 2, 4, 4>", "wgrad_s16": the instance's parameters <NG, NA, NP,
 * PH, 1, ROLL, G11>, trailing zeros and the 1 in front of them left out), without launching anything and without a HIP call: the same argument checks (all
 * four pointers of the descriptor included) and the same dispatch code, its environment switch included, with the launch
 * replaced by the label; the same status codes as ammc_conv_wgrad_s16 for the same descriptor.  out_len >= 48.
 * ammc_conv_wgrad_s16_slabs_variant: the same for ammc_conv_wgrad_s16_slabs (desc->dw is not looked at): the instance's
 * name + "+slabs<k>", k = the slabs the launch writes = ammc_conv_wgrad_s16_slab_floats / (n * kpad); AMMC_EUNSUP where
 * the slab entry has no kernel for the descriptor (slab_floats == 0), AMMC_EINVAL as that entry.  out_len >= 64. */
int ammc_conv_wgrad_s16_variant(const AmmcWgradDesc* desc, char* out, int32_t out_len);
int ammc_conv_wgrad_s16_slabs_variant(const AmmcWgradDesc* desc, char* out, int32_t out_len);
/* Deterministic forms of the two implicit-GEMM weight-gradient kernels (wgrad_s16_kernel / wgrad_f32_kernel): the same
 * operands, the same pixel splits and the same packed result desc->dw [n][kpad] as ammc_conv_wgrad_s16 /
 * ammc_conv_wgrad_f32 (ammc_unpack_conv_wgrad_f32 / ammc_unpack_convt_wgrad_f32 follow as before), but no atomic: every
 * workgroup stores its tile into the slab of its pixel split (slabs: [k][n][kpad] floats of caller workspace, plain
 * stores; nothing of it needs initialising) and a second kernel writes dw[r][c] = slab 0 [r][c] + slab 1 [r][c] + ... +
 * slab k-1 [r][c], added in that order.  dw needs NO zeroing: every element [n][kpad] is written (the S16 form writes the
 * columns ntaps * cin .. kpad as zeros).  Equal operands give equal bits, whatever else the device runs.
 *   ammc_conv_wgrad_*_det_floats: the workspace, k * n * kpad floats, k = the pixel splits - a function of the descriptor
 *     alone (shape, n, cin, ntaps; no device query, no environment switch, no launch history).  0 where the descriptor
 *     is refused and where k == 1: the one workgroup per tile then stores straight into dw and `slabs` may be NULL.
 *   ammc_conv_wgrad_s16_det runs wgrad_s16_kernel for EVERY descriptor ammc_conv_wgrad_s16's checks accept - the
 *     halo-patch dispatcher and its switch (AMMC_WGRAD_G11) are not asked; the stride-1 3x3 layers that have a
 *     slab form are better served by ammc_conv_wgrad_s16_slabs, which is deterministic too.
 *   Status codes: those of the atomics entry for the same descriptor; AMMC_EINVAL when k > 1 and slabs is NULL or
 *     slab_floats is short.
 *   ammc_conv_wgrad_*_det_variant: nothing is launched, no HIP call, the same checks (all four pointers included); the
 *     kernel's name + "+det<k>" ("wgrad_s16+det3", "wgrad_f32<1, 4, 2, 1>+det12").  out_len >= 48. */
int64_t ammc_conv_wgrad_s16_det_floats(const AmmcWgradDesc* desc);
int ammc_conv_wgrad_s16_det(const AmmcWgradDesc* desc, const float* g_inv_scale, float* slabs, int64_t slab_floats,
                            void* stream);
int ammc_conv_wgrad_s16_det_variant(const AmmcWgradDesc* desc, char* out, int32_t out_len);
int64_t ammc_conv_wgrad_f32_det_floats(const AmmcWgradDesc* desc);
int ammc_conv_wgrad_f32_det(const AmmcWgradDesc* desc, float* slabs, int64_t slab_floats, void* stream);
int ammc_conv_wgrad_f32_det_variant(const AmmcWgradDesc* desc, char* out, int32_t out_len);
/* packed gradient -> the module's parameter layout */
int ammc_unpack_conv_wgrad_f32(const float* packed, int32_t cout, int32_t cin, int32_t ksize, int32_t cin_p,
                               float* out_oihw, void* stream);
int ammc_unpack_convt_wgrad_f32(const float* packed, int32_t cin, int32_t co, float* out_iohw, void* stream);
/* filters of the input-gradient convolutions (run through ammc_conv_gemm_f32):
 * 3x3: [rows>=cin][Kpad], k = tap*cout_p + n, value W[n][c][2-r][2-s];  1x1: transpose, zero padded */
int ammc_pack_conv_dgrad_weight_f32(const float* w_oihw, int32_t cout, int32_t cin, int32_t cout_p, int32_t rows,
                                    float* out, void* stream);
int ammc_transpose_pad_f32(const float* w, int32_t rows, int32_t cols, int32_t rows_p, float* out, void* stream);

/* All 3x3 filters of a training step packed in ONE launch, straight to the S16 images the split-fp16 kernels read
 * (= ammc_pack_conv_weight_f32 / ammc_pack_conv_dgrad_weight_f32 followed by ammc_split_rows_f32, per layer).  items_dev: a
 * device array of n_items records of ammc_pack_filters_item_bytes() bytes each:
 *   { const float* w_oihw; float* out16; int32 cout, cin, inner_p, kpad, kind, rows; int64 group_end; }
 * kind 0 = forward filter [rows = cout][kpad], k = tap * inner_p + c (inner_p = cin_p); kind 1 = input-gradient filter
 * [rows >= cin][kpad], k = tap * inner_p + n (inner_p = cout_p); group_end = running total of rows * kpad / 8. */
int ammc_pack_filters_item_bytes(void);
int ammc_pack_filters_s16(const void* items_dev, int32_t n_items, int64_t total_groups, void* stream);

/* PixelDiscriminator (Code/models/pix2pix_networks.py:580-631): Conv2d(k 4, padding 2, stride 2|1, bias) + LeakyReLU(0.1).
 * Forward and weight gradient run through ammc_conv_gemm_f32 / ammc_conv_wgrad_f32 with ntaps 16 (x_step / a_step =
 * the stride, x / a = the corner of a 2-pixel halo).  Input gradient: stride 1 = one 16-tap conv with the flipped
 * filter; stride 2 = four 2x2-tap convs over the output gradient, one per input-pixel parity (py, px), written
 * through doubled y strides.  This packs those filters: stride 1 -> [rows][16*cout_p], stride 2 ->
 * [4][rows][4*cout_p] (phase = py*2+px). */
int ammc_pack_conv4_dgrad_weight_f32(const float* w_oihw, int32_t cout, int32_t cin, int32_t cout_p, int32_t rows,
                                     int32_t stride, int32_t pad /* of the convolution: 2 (D) or 1 */, float* out,
                                     void* stream);

/* FlowNet2-SD forward (Code/models/flownet2/models.py:15-59): the pieces that are not convolutions.  Its Conv2d(k 3,
 * stride 1|2) + LeakyReLU(0.1) layers are ammc_conv_gemm_f32 (ntaps 9, x_step = stride, AMMC_ACT_LRELU); its
 * ConvTranspose2d(k 4, s 2, p 1) layers are the four 2x2-tap parity convolutions of ammc_pack_conv4_dgrad_weight_f32
 * (pad 1); layers whose input is a concatenation run once per part and accumulate through `res`. */
/* scratch: ammc_flownet_prep_scratch_doubles(batch) doubles of device memory (per (sample, colour) slice sums of the mean:
 * summed by 32 workgroups each, combined in a fixed order) */
int ammc_flownet_prep_scratch_doubles(int32_t batch);
int ammc_flownet_prep_f32(const float* in /* [B][3][2][H][W], 0..rgb_max */, int32_t batch, int32_t h, int32_t w,
                          float* y /* NHWC, 8 channels */, int64_t y_bs, int64_t y_rs, int64_t y_ps, float rgb_max,
                          double* scratch, void* stream);
int ammc_lrelu_f32(float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t batch, int32_t h, int32_t w, int32_t c,
                   float slope, void* stream);
/* the same LeakyReLU in place on an S16 activation (c % 8 == 0): the split-fp16 form of the FlowNet2-SD forward */
int ammc_lrelu_s16(float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t batch, int32_t h, int32_t w, int32_t c,
                   float slope, void* stream);
int ammc_upsample4_bilinear_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t h,
                                int32_t w, int32_t c, float premul, float* out /* NCHW [B][c][4h][4w] */, void* stream);
/* g *= (y > 0 ? 1 : slope) in place: autograd of nn.LeakyReLU evaluated on the layer output */
int ammc_lrelu_bwd_f32(const float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps, float* g, int64_t g_bs, int64_t g_rs,
                       int64_t g_ps, int32_t batch, int32_t h, int32_t w, int32_t c, float slope, void* stream);

/* Device half of the input pipeline (Code/dataset/two_stream_dataset.py:72-99, 503-506): per frame, once.
 * frames: uint8 [n][h][w][3] (RGB; bgr != 0: as decoded by cv2 / TurboJPEG, the cvtColor of :76 is folded in) ->
 *   cv2.resize INTER_LINEAR (8-bit fixed point) -> /255 -> (x - 0.5) / 0.5 -> float32 [n][3][oh][ow].
 * flows: float32 [n][h][w][2] (.flo payload, flowlib.py:589-611) -> cv2.resize INTER_LINEAR (float) ->
 *   c0 = u / oh, c1 = c0 / ow (the loader derives channel 1 from the scaled channel 0, :94-95) -> [n][2][oh][ow]. */
int ammc_frames_u8_to_f32(const uint8_t* src, int32_t n, int32_t h, int32_t w, float* dst, int32_t oh, int32_t ow,
                          int32_t bgr, void* stream);
int ammc_flows_to_f32(const float* src, int32_t n, int32_t h, int32_t w, float* dst, int32_t oh, int32_t ow,
                      void* stream);

/* Clip bank of the training loop (pipeline.ClipBank): each frame resized once into a device-resident bank, each
 * iteration's clips gathered from it by one launch, bit-identical to the two entries above.
 * frames: as ammc_frames_u8_to_f32, stopping before the normalisation: the 8-bit resize result, uint8 [n][3][oh][ow]
 *   (RGB order).
 * flows: as ammc_flows_to_f32, channel 0 only: c0 = u / oh, float32 [n][oh][ow].
 * gather: clip b = bank frames [rgb_first[b], + rgb_len) and [op_first[b], + op_len) (device int32 [batch] each) ->
 *   rgb_out float32 [batch][rgb_len][3][h][w] = (v / 255 - 0.5) / 0.5, op_out float32 [batch][op_len][2][h][w] =
 *   (c0, c0 / w).  n_rgb / n_op: frames in the banks.  Needs h * w % 4 == 0, rgb_bank 4-byte and op_bank / outputs
 *   16-byte aligned, batch * (3 rgb_len + op_len) <= 65535; AMMC_EINVAL otherwise.  The caller validates the indices
 *   (a clip never crosses a sub-video); a clip whose index is outside [0, n - len] is written as NaN, nothing is read. */
int ammc_frames_u8_resize_u8(const uint8_t* src, int32_t n, int32_t h, int32_t w, uint8_t* dst, int32_t oh, int32_t ow,
                             int32_t bgr, void* stream);
int ammc_flows_resize_c0(const float* src, int32_t n, int32_t h, int32_t w, float* dst, int32_t oh, int32_t ow,
                         void* stream);
int ammc_gather_clips(const uint8_t* rgb_bank, int64_t n_rgb, const float* op_bank, int64_t n_op, const int32_t* rgb_first,
                      const int32_t* op_first, int32_t batch, int32_t rgb_len, int32_t op_len, int32_t h, int32_t w,
                      float* rgb_out, float* op_out, void* stream);
/* The clips of ONE bank, for a single-stream training stage (pipeline.ClipBank with one root): kind 0 = the rgb bank
 * (uint8 [n][3][h][w]) -> out float32 [batch][len][3][h][w], kind 1 = the op bank (float32 [n][h][w]) -> out float32
 * [batch][len][2][h][w]; bit-identical to the rgb / op half of ammc_gather_clips for the same indices.  Same
 * requirements (the bank 4-byte (rgb) or 16-byte (op) aligned, batch * planes <= 65535 with 3 planes per rgb frame and
 * one per op frame) and the same NaN output for an index outside [0, n - len]. */
int ammc_gather_clips_one(const void* bank, int64_t n, int32_t kind, const int32_t* first, int32_t batch, int32_t len,
                          int32_t h, int32_t w, float* out, void* stream);

/* The same gather from a bank split between two tiers (pipeline.ClipBank with a host budget), one launch: frames
 * [0, n_*_dev) of a kind are device memory at *_dev + f * stride, frames [n_*_dev, n_*) are pinned or registered,
 * device-mapped HOST memory at *_host + (f - n_*_dev) * stride (stride: 3 h w bytes of the rgb bank, h w floats of the
 * op bank).  Output layout, normalisation, derived flow channel and the NaN rule are those of ammc_gather_clips, so the
 * result is bit-identical to it (and to ammc_gather_clips_one) on an all-device copy of the bank wherever the split
 * lies, a clip that straddles it included.  A kind whose `first` is NULL is skipped (its other arguments are not read):
 * one entry for the joint stage and both single stages; both NULL is AMMC_EINVAL.
 * Needs h * w % 4 == 0; 0 <= n_dev <= n and n >= len per kind; a tier's base may be NULL only if the tier is empty;
 * rgb_dev 4-byte, op_dev, both host bases and the outputs 16-byte aligned; batch * planes <= 65535 (3 planes per rgb
 * frame, one per op frame, of the kinds gathered).  The host tier is read 16 bytes per lane, several loads in flight
 * (16 rgb pixels per load when h * w % 16 == 0, 4 otherwise).  A non-empty host tier whose base
 * hipPointerGetAttributes does not report as host memory mapped to the device - a pageable pointer - is AMMC_EINVAL and
 * nothing is launched; that check runs after all the others, which need no device. */
int ammc_gather_clips_tiered(const uint8_t* rgb_dev, const uint8_t* rgb_host, int64_t n_rgb_dev, int64_t n_rgb,
                             const float* op_dev, const float* op_host, int64_t n_op_dev, int64_t n_op,
                             const int32_t* rgb_first, const int32_t* op_first, int32_t batch, int32_t rgb_len,
                             int32_t op_len, int32_t h, int32_t w, float* rgb_out, float* op_out, void* stream);

/* Gradient buckets of data-parallel training (parallel.BucketedGradReducer; the reference is single-GPU): the gather of
 * up to AMMC_BUCKET_MAX contiguous fp32 member tensors into one flat all-reduce buffer, and the way back with the
 * average folded in, one launch each (torch._foreach_copy_ / _foreach_mul_ / _foreach_copy_ otherwise).
 * table: HOST memory, read during the call only (it travels to the device in the kernel arguments: nothing is
 *   uploaded and nothing on the device outlives the launch).  ptr[i]: device base of member i, 4-byte aligned;
 *   end[i]: the flat offset, in floats, one past member i.  Member i starts at end[i - 1] (0 for i = 0), rounded up
 *   to a multiple of `pad` floats: pad = 1 packs like torch.cat, pad = 4 starts every member on 16 bytes (the padding
 *   floats are neither read nor written: allocate the flat buffer zeroed).  Members are non-empty (end[i] > start).
 * flat: device, 4-byte (pad = 1) / 16-byte (pad = 4) aligned, end[n - 1] floats.
 * pack:   flat[start_i + j] = member_i[j]
 * unpack: member_i[j] = flat[start_i + j] * scale   (one fp32 multiply: bit-identical to mul_ followed by copy_)
 * Runs whose two sides are congruent modulo 16 bytes move 16 bytes per lane, others float by float.  A bucket of more
 * than AMMC_BUCKET_MAX members is several calls, each with `flat` advanced to its first member's start.
 * AMMC_EINVAL: null / misaligned pointers, n outside [1, AMMC_BUCKET_MAX], pad not 1 or 4, an empty member. */
#define AMMC_BUCKET_MAX 128
typedef struct AmmcBucketTable {
  void* ptr[AMMC_BUCKET_MAX];
  int64_t end[AMMC_BUCKET_MAX];
} AmmcBucketTable;
int ammc_bucket_pack_f32(const AmmcBucketTable* table, int32_t n, int32_t pad, float* flat, void* stream);
int ammc_bucket_unpack_scale_f32(const AmmcBucketTable* table, int32_t n, int32_t pad, const float* flat, float scale,
                                 void* stream);

/* nn.BatchNorm2d in training mode (unet.py:12,15).  Per-channel reductions write
 * partial[ammc_chan_reduce_blocks(B*H*W)][Q][C]; the finalizers combine them in fp64, fixed order. */
int ammc_chan_reduce_blocks(int32_t pixels);
int ammc_bn_stats_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t h, int32_t w,
                      int32_t c, float* partial /* Q=2: sum, sum of squares */, void* stream);
int ammc_bn_finalize_f32(const float* partial, int32_t nblocks, int32_t c, float count, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                         float* mean, float* invstd, float* scale, float* shift, void* stream);
/* y = act(x*scale + shift) + res on interior pixels (BN apply + ReLU + AMFT residual) */
int ammc_scale_shift_act_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, const float* scale,
                             const float* shift, const float* res, int64_t r_bs, int64_t r_rs, int64_t r_ps,
                             float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t relu, int32_t batch,
                             int32_t h, int32_t w, int32_t c, void* stream);
/* The same apply pass with the S16 image of y as its output (same strides; the fp32 y32 is optional): tensors that only
 * the split-fp16 convolutions read - the middle activation of a double_conv in training - never exist in fp32. */
int ammc_scale_shift_act_s16_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, const float* scale,
                                 const float* shift, const float* res, int64_t r_bs, int64_t r_rs, int64_t r_ps,
                                 float* y32 /* may be NULL */, float* y16, int64_t y_bs, int64_t y_rs, int64_t y_ps,
                                 int32_t relu, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* ... of a tensor that nn.MaxPool2d(2) follows (the second unit of `inconv` / `down`, models/unet.py:23-37): y as above, plus
 * its pooled S16 image pool16 (h/2 x w/2, own strides) and the window positions idx[batch][h/2][w/2][c] exactly as
 * ammc_maxpool2x2_s16_idx would produce them from y16 - in the same pass.  h, w even, c/8 a power of two <= 256; else
 * AMMC_EUNSUP (run the two passes). */
int ammc_scale_shift_act_s16_pool_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, const float* scale,
                                      const float* shift, float* y32 /* may be NULL */, float* y16, int64_t y_bs, int64_t y_rs,
                                      int64_t y_ps, float* pool16, int64_t p_bs, int64_t p_rs, int64_t p_ps, uint8_t* idx,
                                      int32_t relu, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* BN (+ReLU) backward: partial Q=2: sum g, sum g*xhat with g = dy*[c*scale+shift > 0]; then
 * dc = scale*(g - sums[0]/M - xhat*sums[1]/M); sums[0] = dbeta, sums[1] = dgamma.
 * NOTE: the `gamma`/`beta` arguments take the FOLDED scale (gamma*invstd) and shift produced by
 * ammc_bn_finalize_f32, so that the ReLU mask is evaluated exactly as in the forward. */
int ammc_bn_bwd_reduce_f32(const float* c_raw, int64_t c_bs, int64_t c_rs, int64_t c_ps, const float* dy,
                           int64_t d_bs, int64_t d_rs, int64_t d_ps, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, int32_t relu, int32_t batch, int32_t h, int32_t w,
                           int32_t c, float* partial, void* stream);
int ammc_bn_bwd_apply_f32(const float* c_raw, int64_t c_bs, int64_t c_rs, int64_t c_ps, const float* dy,
                          int64_t d_bs, int64_t d_rs, int64_t d_ps, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, const float* sums, int32_t relu, float* dc,
                          int64_t o_bs, int64_t o_rs, int64_t o_ps, int32_t batch, int32_t h, int32_t w, int32_t c,
                          int32_t* amax_bits /* may be NULL: [256] slots, max |dc| as in ammc_absmax_bits_f32 */,
                          void* stream);
/* The same backward with the S16 twin of dc as its output (training on the split-fp16 kernels, one rank):
 * reduce_bound: partial Q=4 = the two sums + per-channel max|g|, max|xhat|; finalize: sums[2][C] and an upper bound of
 * max|dc| (|scale| (max|g| + |sum_g|/M + max|xhat| |sum_gx|/M)) into the [256] amax slots (zeroed by the caller) - the
 * power-of-two rescaling of the gradient is known before dc exists; apply_s16: dc * 2^k as an S16 image (dc16; same
 * strides for the optional fp32 dc32), 2^-k into inv_scale[0..n_inv) for the consumers' epilogues. */
int ammc_bn_bwd_reduce_bound_f32(const float* c_raw, int64_t c_bs, int64_t c_rs, int64_t c_ps, const float* dy,
                                 int64_t d_bs, int64_t d_rs, int64_t d_ps, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, int32_t relu, int32_t batch, int32_t h,
                                 int32_t w, int32_t c, float* partial, void* stream);
int ammc_bn_bwd_finalize_f32(const float* partial, int32_t nblocks, int32_t c, int32_t pixels, const float* gamma,
                             float* sums, int32_t* amax_bits, void* stream);
int ammc_bn_bwd_apply_s16_f32(const float* c_raw, int64_t c_bs, int64_t c_rs, int64_t c_ps, const float* dy,
                              int64_t d_bs, int64_t d_rs, int64_t d_ps, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, const float* sums, int32_t relu, float* dc16,
                              float* dc32 /* may be NULL */, int64_t o_bs, int64_t o_rs, int64_t o_ps, int32_t batch,
                              int32_t h, int32_t w, int32_t c, const int32_t* amax_bits, float* inv_scale,
                              int32_t n_inv, void* stream);
/* per-channel sum over pixels (bias gradients): partial Q=1 */
int ammc_chan_sum_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t h, int32_t w,
                      int32_t c, float* partial, void* stream);
/* the same pass with max |x| of the whole tensor left in the [256] amax slots (zeroed by the caller; as
 * ammc_absmax_bits_f32): the bias-gradient pass of a ConvTranspose also finds the power of two of its gradient's S16
 * re-encoding; then that re-encoding for a channel SLICE (strided form of ammc_split_rows_scaled_f32; c % 8 == 0) */
int ammc_chan_sum_absmax_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t h, int32_t w,
                             int32_t c, float* partial, int32_t* amax_bits, void* stream);
int ammc_split_scaled_strided_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, float* y16, int64_t y_bs,
                                  int64_t y_rs, int64_t y_ps, int32_t batch, int32_t h, int32_t w, int32_t c,
                                  const int32_t* amax_bits, float* inv_scale, int32_t n, void* stream);
int ammc_reduce_partials_f32(const float* partial, int32_t nblocks, int32_t qc, float scale, float* out, void* stream);
/* the same per run of seg_rows rows: out[ceil(nblocks / seg_rows)][qc] - a first stage in front of ammc_bn_finalize_f32 /
 * ammc_bn_bwd_finalize_f32 when a convolution's statistics output (AmmcConvDesc.stats) has thousands of rows.  Columns
 * max_from .. qc - 1 (max_from % 8 == 0; = qc for none) are combined by max: the max |g|, max |xhat| rows of a
 * BatchNorm-backward partial (max_from = 2 c of its [4][c] rows). */
int ammc_reduce_partials_seg_f32(const float* partial, int32_t nblocks, int32_t qc, int32_t seg_rows, int32_t max_from,
                                 float* out, void* stream);
/* nn.MaxPool2d(2) backward (+ `add`, the gradient reaching the same tensor through the skip).  h, w: the pooled size;
 * in_h, in_w: the size of x / add / dx (2h or 2h+1: the last row / column of an odd size is in no window and gets `add`
 * alone, as MaxPool2d's floor does) */
int ammc_maxpool2x2_bwd_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, const float* dp, int64_t p_bs,
                            int64_t p_rs, int64_t p_ps, const float* add, int64_t a_bs, int64_t a_rs, int64_t a_ps,
                            float* dx, int64_t o_bs, int64_t o_rs, int64_t o_ps, int32_t batch, int32_t h, int32_t w,
                            int32_t in_h, int32_t in_w, int32_t c, void* stream);
/* the same from the window positions recorded by ammc_maxpool2x2_s16_idx in the forward (c % 8 == 0): the pooled tensor is
 * not read at all */
int ammc_maxpool2x2_bwd_idx_f32(const uint8_t* idx, const float* dp, int64_t p_bs, int64_t p_rs, int64_t p_ps, const float* add,
                                int64_t a_bs, int64_t a_rs, int64_t a_ps, float* dx, int64_t o_bs, int64_t o_rs, int64_t o_ps,
                                int32_t batch, int32_t h, int32_t w, int32_t in_h, int32_t in_w, int32_t c, void* stream);
/* BatchNorm (+ReLU) backward of a unit whose output was max-pooled in the forward, WITHOUT materialising its output
 * gradient: dy = add + MaxPool2d(2)-backward(dpo), formed on the fly from `add` (the gradient through the skip path, laid out
 * like dy), the pooled gradient dpo[batch][ph][pw][c] (own strides) and the window positions idx[batch][ph][pw][c] recorded
 * by the forward (ammc_maxpool2x2_s16_idx / ammc_scale_shift_act_s16_pool_f32); ph = h / 2, pw = w / 2 (floor).  Otherwise
 * ammc_bn_bwd_reduce_bound_f32 / ammc_bn_bwd_apply_s16_f32.  The apply form needs ammc_bn_bwd_unpool_supported(c, pixel
 * strides of c_raw / add / dc, w) != 0, else AMMC_EUNSUP (materialise dy with ammc_maxpool2x2_bwd_idx_f32). */
int ammc_bn_bwd_unpool_supported(int32_t c, int64_t c_ps, int64_t d_ps, int64_t o_ps, int32_t w);
/* 1 when ammc_scale_shift_act_s16_pool_f32 takes this geometry (even h, w; c / 8 a power of two <= 256; the row form's
 * stride limits; AMMC_ROW_KERNELS not 0), else 0: callers then run ammc_scale_shift_act_s16_f32 + ammc_maxpool2x2_s16_idx
 * (the same query shape as ammc_bn_bwd_unpool_supported for the backward side). */
int ammc_scale_shift_act_s16_pool_supported(int32_t c, int32_t h, int32_t w, int64_t x_rs, int64_t x_ps, int64_t y_rs,
                                            int64_t y_ps, int64_t p_ps);
int ammc_bn_bwd_reduce_bound_unpool_f32(const float* c_raw, int64_t c_bs, int64_t c_rs, int64_t c_ps, const float* add,
                                        int64_t d_bs, int64_t d_rs, int64_t d_ps, const float* dpo, int64_t p_bs, int64_t p_rs,
                                        int64_t p_ps, const uint8_t* idx, int32_t ph, int32_t pw, const float* mean,
                                        const float* invstd, const float* gamma, const float* beta, int32_t relu, int32_t batch,
                                        int32_t h, int32_t w, int32_t c, float* partial, void* stream);
int ammc_bn_bwd_apply_s16_unpool_f32(const float* c_raw, int64_t c_bs, int64_t c_rs, int64_t c_ps, const float* add,
                                     int64_t d_bs, int64_t d_rs, int64_t d_ps, const float* dpo, int64_t p_bs, int64_t p_rs,
                                     int64_t p_ps, const uint8_t* idx, int32_t ph, int32_t pw, const float* mean,
                                     const float* invstd, const float* gamma, const float* beta, const float* sums,
                                     int32_t relu, float* dc16, float* dc32, int64_t o_bs, int64_t o_rs, int64_t o_ps,
                                     int32_t batch, int32_t h, int32_t w, int32_t c, const int32_t* amax_bits,
                                     float* inv_scale, int32_t n_inv, void* stream);
/* torch.tanh backward at the module boundary: NCHW (dout, out) -> NHWC d(pre-tanh), cp channels */
int ammc_tanh_bwd_nhwc_f32(const float* dout_nchw, const float* out_nchw, int32_t batch, int32_t c, int32_t h,
                           int32_t w, float* y, int64_t y_bs, int64_t y_rs, int64_t y_ps, int32_t cp, void* stream);
/* gradient of the commit term and of q_one w.r.t. the encoder output (unet.py:310-311) */
int ammc_commit_bwd_f32(const float* z, const float* embed_md, const int32_t* idx_topk, int32_t k,
                        const float* ddiff, const float* dq, float* dz, int32_t n, int32_t d, void* stream);
/* the same update in two halves, for data-parallel training with synchronised statistics: per-slot counts [m]
 * and feature sums [d][m] of this rank (all-reduce them), then the EMA + renormalisation */
int ammc_codebook_count_f32(const float* x, const int32_t* idx_topk, int32_t k, int32_t n, int32_t d, int32_t m,
                            float* counts, float* sums, void* stream);
int ammc_codebook_ema_apply_f32(const float* counts, const float* sums, int32_t d, int32_t m, float decay,
                                float one_minus_decay, float eps, float* cluster_size, float* embed_avg, float* embed,
                                void* stream);
/* EMA codebook update (unet.py:298-309), deterministic (no atomics) */
int ammc_codebook_ema_f32(const float* x, const int32_t* idx_topk, int32_t k, int32_t n, int32_t d, int32_t m,
                          float decay, float one_minus_decay, float eps, float* cluster_size, float* embed_avg,
                          float* embed, void* stream);

/* ------------------------------------------------------------------------------------------
 * The per-pixel terms of the generator's objective and their gradient (csrc/loss.hip), on the NCHW fp32 tensors of the
 * module boundary: pred / target [batch][c][h][w], c = 2 or 3 (otherwise AMMC_EUNSUP), dense, any h, w >= 1 (16-byte
 * loads when w % 4 == 0 and the tensors start on 16-byte boundaries, 4-byte loads otherwise); the target's samples may lie target_bs >= c h w floats apart (the last frame of every clip of a batch, in place).  Replaces models/losses/losses_utils.py: `L2` (:124-129, the intensity term), `Gradient_Loss` (:30-61,
 * alpha = 1 only) and `Flow_Loss` (:10-15).  No allocation, no synchronisation, no atomics; the same bits on every
 * launch.  (The LSGAN terms, :100-110, act on patch maps of a few thousand elements and are not here.)
 * ---------------------------------------------------------------------------------------- */
#define AMMC_PRED_LOSS_ROWS 4  /* image rows one workgroup (= one partial row) of the two kernels below covers */
#define AMMC_L1_CHUNK 4096     /* elements one workgroup (= one partial) of ammc_l1_partials_f32 covers         */
/* partial rows of ammc_pred_loss_fwd_f32: ceil(batch * h / AMMC_PRED_LOSS_ROWS); 0 for a non-positive / oversized shape */
int ammc_pred_loss_partial_rows(int32_t batch, int32_t h, int32_t w);
/* partial[rows][2] = fp32 sums over the pixels of a workgroup's image rows (at most AMMC_PRED_LOSS_ROWS * w of them) of
 *   [0] sqrt(sum_c (pred - target)^2)                      `torch.norm(pred - target, p=2, dim=1)` before the mean
 *   [1] |tx - gx| + |ty - gy|  (want_gdl != 0, else 0)      s = sum_c, gx[x] = s[x] - s[x-1], gx[0] = s[0]; gy down the rows
 * Combine with ammc_reduce_partials_f32(partial, rows, 2, 1 / (batch h w), out): out[0] = the intensity term, out[1] = the
 * gradient-difference term (fp64, fixed order). */
int ammc_pred_loss_fwd_f32(const float* pred, const float* target, int64_t target_bs, int32_t batch, int32_t c, int32_t h,
                           int32_t w, int32_t want_gdl, float* partial, void* stream);
/* d_pred (fully overwritten) = g_int[0] * d(intensity term) / d(pred) + g_gdl[0] * d(gradient-difference term) / d(pred);
 * g_int / g_gdl: DEVICE scalars, either may be NULL (= 0; with g_gdl NULL no neighbour row is read).  torch's backward:
 * 0 where the channel norm is 0, sign(0) = 0.  Reads rows y - 1, y, y + 1 of both tensors; nothing is materialised. */
int ammc_pred_loss_bwd_f32(const float* pred, const float* target, int64_t target_bs, const float* g_int, const float* g_gdl,
                           int32_t batch, int32_t c, int32_t h, int32_t w, float* d_pred, void* stream);
/* partial[ceil(count / AMMC_L1_CHUNK)] = sums of |a - b| (value only: `Flow_Loss` on flows that carry no gradient);
 * combine with ammc_sum_partials_f32(partial, n, 1 / count, out). */
int ammc_l1_partials_f32(const float* a, const float* b, int64_t count, float* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * Anomaly localisation (csrc/error_maps.hip): per-patch and per-pixel squared-error maps of a predicted frame against
 * its target, the frame's squared error summed in a fixed order, and the worst patch.  pred / target: fp32
 * [batch][c][h][w] views, pixel stride 1, batch / channel / row strides in floats (the targets of a batch are a slice of
 * a resident sub-video).  With e = 0.5f * (target - pred), the reference's `psnr_error` on [0, 1] (utils/utils.py:143-147):
 *   pixel[b][y][x]      mean over the channels of e^2   (optional: pixel may be NULL; rows w floats apart, samples px_bs)
 *   patch_sum[b][i][j]  sum of e^2 over the channels and pixels of patch (i, j): patch x patch pixels anchored at (0, 0),
 *                       the last patch row / column ragged (only the pixels that exist); ph = ceil(h / patch),
 *                       pw = ceil(w / patch), rows pw floats apart, samples ps_bs floats apart
 *   patch_mean[b][i][j] patch_sum / (c * rows * cols) with the patch's true pixel count (same shape and strides)
 *   frame_sq[b]         for each patch row i a double adds (double)patch_sum[b][i][0], [1], ... in that order; a second
 *                       double adds those row values for i = 0, 1, ...; rounded once to fp32.
 *                       PSNR = 10 log10(c h w / frame_sq)
 *   worst[b]            the largest patch_mean[b] (one of the stored values, bit for bit)
 *   worst_idx[b]        i * pw + j of that patch, the lowest index among equal values
 * Two launches, no atomics, no allocation, no synchronisation: the same bits on every launch, and the order in which a
 * patch's terms are added depends on (c, rows, cols, patch) of that patch only - not on the sample's place in the
 * batch, the batch size, the strides or the alignment (16-byte loads where all bases and strides allow, 4-byte loads
 * otherwise; both add in one order).  Non-finite inputs propagate into patch_sum, patch_mean, pixel and frame_sq;
 * worst and worst_idx are UNSPECIFIED for a sample whose patch means hold a NaN.
 * AMMC_EINVAL: a null pointer other than pixel; batch, c, h or w <= 0; pointers not 4-byte aligned; a row stride < w;
 * a channel / batch stride smaller than the extent below it; ps_bs < ph * pw; px_bs < h * w with pixel given.
 * AMMC_EUNSUP: c > 4; patch not 8, 16 or 32; batch * ph or ph * pw >= 2^31; a frame so wide that its quads (4 pixels)
 * need more than 65535 column chunks of 64 (patch 8) or 32 (patch 16, 32) quads on the grid's y dimension, i.e.
 * w > 16776960 resp. 8388480 (element offsets are 64-bit).
 * All of them are decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
/* ceil(h / patch) * ceil(w / patch); 0 for bad arguments */
int ammc_error_maps_patch_count(int32_t h, int32_t w, int32_t patch);
int ammc_error_maps_f32(const float* pred, int64_t p_bs, int64_t p_cs, int64_t p_rs, const float* target, int64_t t_bs,
                        int64_t t_cs, int64_t t_rs, int32_t batch, int32_t c, int32_t h, int32_t w, int32_t patch,
                        float* patch_sum, int64_t ps_bs, float* patch_mean, float* pixel, int64_t px_bs, float* frame_sq,
                        float* worst, int32_t* worst_idx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-clip memory-commit scores (csrc/memory_scores.hip): the memory module's commitment distance per position and per
 * clip, from a pass of its own over the bottleneck in front of the memory block.  x: fp32 NHWC [batch][h][w][c],
 * channel stride 1, batch / row / pixel strides in floats.  enc_w [d][c] and enc_b [d]: the module's `enc` 1x1 as it
 * lies in memory (no packing).  embed_dm [d][m]: the module buffer E; embed_md [m][d], enorm [m] from
 * ammc_pack_codebook_f32.  With p a position of clip b:
 *   z[p][j]       = (sum_i x[p][i] * enc_w[j][i]) + enc_b[j] in fp32.  The channels are added in chains of at most 64
 *                   consecutive ones (fmaf chains from 0, in channel order), the chains are added in order, the bias
 *                   last: the order is a function of c alone
 *   r[p][s]       = enorm[s] - 2 * sum_j z[p][j] * E[j][s] in fp32 (one fmaf chain over j = 0, 1, ... from 0): the
 *                   reference's `dist` (models/unet.py:284-288) without its row-constant |z|^2
 *   idx[p][0..k)  = the k smallest keys, nearest first; exactly equal keys in ascending slot order
 *   s[p]          = sum_j (E[j][idx0] - z[p][j])^2, j = 0, 1, ... in order, each square a rounded product: taken
 *                   directly from the fp32 data, never from the expanded form
 *   map[b][y][x]  = s[p] / d                    (rows w floats apart, clips map_bs floats apart)
 *   idx_topk      int32 [batch][h][w][k], dense; may be NULL
 *   commit[b]     = (float)(S / (h * w)): for each row y a double adds (double)map[b][y][0], [y][1], ... in that order,
 *                   a second double adds the rows in order, that total is S (the construction of frame_sq above)
 *   worst[b]      the largest stored map[b] value, bit for bit;  worst_idx[b] the lowest y * w + x that attains it
 * Two launches, no atomics, no arrival counter, no allocation: every output has one writer.  The outputs of clip b are
 * a function of (x[b], enc_w, enc_b, E, h, w, c, m, k) and of nothing else - not the batch size, the clip's place in
 * the batch, a stride or an alignment (16-byte loads where the bases and strides allow, 4-byte loads otherwise), nor
 * whether idx_topk was asked for.  A NaN or +inf key never ranks; where fewer than k keys of a position rank the empty
 * places report slot m - 1.  worst / worst_idx are UNSPECIFIED for a clip whose map holds a NaN.
 * AMMC_EINVAL: a null pointer other than idx_topk; pointers not 4-byte aligned; batch, h, w, c, d, m or k <= 0;
 * x_ps < c; a row / batch stride smaller than the extent below it; map_bs < h * w.
 * AMMC_EUNSUP: d != 64; k > 2; c % 32 != 0 or c > 1024; m < k; h * w > 2^31 - 64 or batch * ceil(h w / 64) >= 2^31.
 * All of them are decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ammc_memory_scores_f32(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_ps, int32_t batch, int32_t h, int32_t w,
                           int32_t c, const float* enc_w, const float* enc_b, const float* embed_dm, const float* embed_md,
                           const float* enorm, int32_t d, int32_t m, int32_t k, float* map, int64_t map_bs, int32_t* idx_topk,
                           float* commit, float* worst, int32_t* worst_idx, void* stream);

/* ------------------------------------------------------------------------------------------
 * SSIM and squared-error frame scores (csrc/ssim.hip): the reference's `ssim_error` (utils/pytorch_ssim.py) and the sum
 * its `mse_error` / `psnr_error` are functions of, from a pass of its own over a predicted frame and its target.
 * pred / target: fp32 [batch][c][h][w] views, pixel stride 1, batch / channel / row strides in floats (the targets of a
 * batch are a slice of a resident sub-video).  The values are used AS THEY ARE: the reference applies C1 = 0.01^2 and
 * C2 = 0.03^2 (rounded to fp32) to its frames on [-1, 1] without rescaling them to [0, 1], and so does this pass.
 * win: a HOST array of 11 floats, read during the call: the reference's 1-D window, exp(-(x - 5)^2 / (2 * 1.5^2)) taken
 * in double, rounded to fp32 and divided by the fp32 sum.  With f = 0 outside the frame (a tap there adds an exact + 0):
 *   G(f)(y, x)      = sum_i win[i] * (sum_j win[j] * f(y + i - 5, x + j - 5)): the row pass over j = 0..10, then the
 *                     column pass over i = 0..10, each ONE fmaf chain from 0 in tap order.  (The reference convolves
 *                     with the fp32-rounded outer product of win; on the map the two differ by 1e-7 .. 3e-7 in exact
 *                     arithmetic, below the fp32 noise of either.  The separable form is the definition here.)
 *   mu1 = G(pred), mu2 = G(target), s1 = G(pred * pred) - mu1 * mu1, s2 = G(target * target) - mu2 * mu2,
 *   s12 = G(pred * target) - mu1 * mu2        (every product rounded; nothing but the chains of G is fused)
 *   ssim_px         = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / (((mu1 * mu1 + mu2 * mu2) + C1) * ((s1 + s2) + C2))
 *                     where pred == target over the whole window this is x / x == 1.0f exactly
 *   map[b][y][x]    = (ssim_px of channel 0 + channel 1 + ...) / c       (optional: map may be NULL; rows w floats apart,
 *                     samples map_bs floats apart)
 *   ssim_c[b][ch]   = (float)(S / ((double)h * w)), S the sum of ssim_px over the channel's pixels (order below)
 *   ssim[b]         = (float)(((double)ssim_c[b][0] + (double)ssim_c[b][1] + ...) / (double)c) from the STORED ssim_c:
 *                     the reference's `ssim_error` on a batch of one
 *   sq[b]           = the sum over the channels and pixels of (target - pred)^2 (order below).
 *                     mse_error = 256 * sq / (c h w) (utils/utils.py:110-111); PSNR = 10 log10(4 c h w / sq) (the 4 is
 *                     `psnr_error`'s halving of the difference)
 * Order.  The frame is cut into tiles of ammc_ssim_tile() x ammc_ssim_tile() pixels anchored at (0, 0), the last tile row
 * / column ragged; pixels of a tile past the frame's edge enter its sums as 0.  Within a tile a thread owns one column
 * and 4 consecutive rows: (v0 + v1) + (v2 + v3), for d^2 then the channels in order; the 64 threads of a wave (32 columns
 * x 2 groups of 4 rows) meet in a fixed xor tree (offsets 1, 2, .. 32); the 4 waves are added in order.  Each tile leaves
 * c + 1 partials in workspace[(b * tiles + tile) * (c + 1) + k]; the second launch adds a sample's partials k in double
 * in tile order (row-major) and rounds once.  Two launches, no atomics, no arrival counter, no allocation, no
 * synchronisation: the same bits on every launch, and the order in which a tile's terms are added depends on
 * (c, rows, cols) of that tile only - not on the sample's place in the batch, the batch size, the strides or the
 * alignment (16-byte loads where all bases and strides allow, 4-byte loads otherwise; both fill the same LDS words in
 * front of the same arithmetic), nor on whether map was asked for.  Non-finite inputs propagate into the outputs of
 * their sample and into no other's.
 * workspace: at least ammc_ssim_workspace_floats(batch, c, h, w) = batch * tiles * (c + 1) floats, owned by the call
 * until its launches have run (one per stream).
 * AMMC_EINVAL: a null pointer other than map; batch, c, h or w <= 0; pointers not 4-byte aligned; a row stride < w;
 * a channel / batch stride smaller than the extent below it; map_bs < h * w with map given; workspace_floats smaller
 * than the query's value.
 * AMMC_EUNSUP: c > 4; batch * tiles >= 2^31 (the grid's x dimension; element offsets are 64-bit).
 * All of them are decided before any HIP call and before win is read.
 * ---------------------------------------------------------------------------------------- */
int ammc_ssim_tile(void);
/* batch * ceil(h / tile) * ceil(w / tile) * (c + 1); 0 for non-positive arguments */
int64_t ammc_ssim_workspace_floats(int32_t batch, int32_t c, int32_t h, int32_t w);
int ammc_ssim_f32(const float* pred, int64_t p_bs, int64_t p_cs, int64_t p_rs, const float* target, int64_t t_bs,
                  int64_t t_cs, int64_t t_rs, int32_t batch, int32_t c, int32_t h, int32_t w, const float* win, float* ssim,
                  float* ssim_c, float* sq, float* map, int64_t map_bs, float* workspace, int64_t workspace_floats,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Score-fusion sweep (csrc/fusion_sweep.hip): the exact numerator of the frame-level AUC of a weighted, one-tap-smoothed
 * fusion of k score channels, at every point of a grid of g weight vectors x s smoothing pairs, from a pass of its own.
 * (The reference fuses two channels at one published pair per dataset, main/eval_metric.py:382-439; the grids it
 * defines at :422-423 are never iterated.)
 *   chan     fp32 [k][n], rows chan_rs floats apart: k normalised score channels over the n scored frames in sequence
 *            order; higher = more normal; all finite (the caller checks: a NaN has no place in an order)
 *   w        fp32 [g][k]: the weight vectors
 *   sm       fp32 [s][2]: the smoothing pairs (a, b); for the reference's lam_smooth l2 the caller passes
 *            a = (float)(1 - l2), b = (float)l2
 *   pos_idx  int32 [n_pos]: the frames of the positive class (the NORMAL class, label 0); neg_idx int32 [n_neg]: the
 *            others.  Together a partition of 0 .. n - 1: n_pos + n_neg == n, n_pos, n_neg >= 1.  (An index outside
 *            [0, n) is clamped into it: a meaningless count, never an access outside chan.)
 * All five are DEVICE arrays.  For grid point (gi, si), with (a, b) = sm[si], every product and every sum a rounded fp32
 * operation, nothing contracted into an FMA:
 *   f[i]   = ((w[gi][0] * chan[0][i] + w[gi][1] * chan[1][i]) + w[gi][2] * chan[2][i]) + ...          left to right
 *   t[0]   = f[0];   t[i] = a * f[i - 1] + b * f[i]  for i >= 1
 *            from the UNSMOOTHED neighbour, across the whole concatenated sequence: the reference's smoothing does not
 *            restart at a video boundary (eval_metric.py:427)
 *   key[i] = t[i] + 0.0f             (-0.0 and +0.0 tie, as they do in an IEEE comparison)
 *   two_u[gi][si] = sum over the positive p and the negative q of (2 * [key_p > key_q] + [key_p == key_q])
 *            int64 [g][s], exact: twice the Mann-Whitney U statistic of the positives, ties counted half.
 *   AUC    = two_u / (2.0 * n_pos * n_neg) in double, the caller's division: the area under the ROC curve with the
 *            normal class positive, ties sharing one threshold (the trapezoid over distinct thresholds).
 * With k = 2, w = ((float)(1 - l1), (float)l1) and chan = (img_n, 1.0f - fea_n) the keys are the scores of the
 * reference's fusion bit for bit.
 * One launch, one workgroup per grid point: the keys of the SMALLER class are sorted in LDS (a bitonic network over the
 * next power of two, padded with a word above every finite key), every frame of the other class is located in the
 * sorted array by two binary searches, and the workgroup adds the counts in int64.  An integer sum: no atomics, no
 * arrival counter, nothing passes between workgroups, the same integers on every launch, in every grid, on every stream.
 * Capacity: min(n_pos, n_neg) <= ammc_fusion_sweep_max_sorted() = 32768 (128 KiB of the CU's 160 KiB of LDS); n itself
 * is bounded by int32 only.
 * AMMC_EINVAL: a null pointer; k < 1 or k > 8; n < 2; g < 1 or s < 1; n_pos < 1 or n_neg < 1; n_pos + n_neg != n;
 * chan_rs < n; chan, w, sm or an index list not 4-byte aligned, two_u not 8-byte aligned; min(n_pos, n_neg) over the
 * capacity.  AMMC_EUNSUP: g * s >= 2^31 (the grid's x dimension).  All of them are decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ammc_fusion_sweep_max_sorted(void);
int ammc_fusion_sweep_f32(const float* chan, int64_t chan_rs, int32_t k, int32_t n, const float* w, int32_t g, const float* sm,
                          int32_t s, const int32_t* pos_idx, int32_t n_pos, const int32_t* neg_idx, int32_t n_neg,
                          int64_t* two_u, void* stream);

/* ------------------------------------------------------------------------------------------
 * Curve sweep (csrc/curve_sweep.hip): at every point of the same grid, what the equal error rate, the average precision
 * and the precision-recall area of the fused score are made of (the reference's other two evaluation types, `compute_eer`
 * and `precision_recall_auc`, main/eval_metric.py:442-446), from a pass of its own.
 * chan, chan_rs, k, n, w, g, sm, s, pos_idx, n_pos, neg_idx, n_neg and key[i] are exactly those of ammc_fusion_sweep_f32:
 * rounded fp32, left to right, nothing contracted, key = t + 0.0f.  The positive class is the NORMAL one (the reference's
 * pos_label = 0).  Per grid point, with P = n_pos, Q = n_neg, and for a value v
 *   TP(v)   = the number of positives with key >= v,  FP(v)   = the number of negatives with key >= v
 *   TPgt(v) = the number of positives with key >  v,  FPgt(v) = the number of negatives with key >  v
 * let v_1 > ... > v_D be the distinct values of all n keys.  Vertex d of the ROC curve is (TP(v_d), FP(v_d)), vertex 0 is
 * (0, 0) with the threshold +inf, and G_d = P * FP_d + Q * TP_d - P * Q in int64 (P Q (fpr + tpr - 1)) rises strictly
 * from -P Q to +P Q.  With a the largest d with G_d <= 0 and b = a + 1:
 *   two_u   int64 [g][s]     ammc_fusion_sweep_f32's, bit for bit
 *   pts     int32 [g][s][4]  (TP_a, FP_a, TP_b, FP_b)
 *   thr     fp32  [g][s][2]  (v_a, v_b), the key values themselves; v_a = +inf when a = 0
 *   sums    fp64  [g][s][2]  over the distinct key values u of the positives, with m(u) = TP(u) - TPgt(u):
 *             sums[0] = sum of m(u) * TP(u) / (TP(u) + FP(u))
 *             sums[1] = sum of 0.5 * m(u) * (L(u) + TP(u) / (TP(u) + FP(u))),  L(u) = TPgt(u) / (TPgt(u) + FPgt(u)) if
 *                       TPgt(u) > 0, else 0 if FPgt(u) > 0, else 1 (the curve's appended point: recall 0, precision 1)
 * From these the caller derives, in double:
 *   eer_vertex = FP_a / Q if |G_a| <= |G_b| else FP_b / Q      the reference's `cal_eer` (fpr at argmin |fnr - fpr|, the
 *                first index on a tie) on the FULL curve, sklearn's roc_curve(drop_intermediate=False)
 *   eer        = (FP_a + lam * (FP_b - FP_a)) / Q, lam = -G_a / (G_b - G_a): where segment a-b crosses fpr + tpr = 1
 *   ap         = sums[0] / P     sklearn's average_precision_score
 *   pr_auc     = sums[1] / P     the reference's auc(recall, precision) over precision_recall_curve
 * The integers and thr are exact.  Each sum has at most P terms, a term at most its m(u), so any order of evaluation is
 * within (P + 4) * 2^-53 of the real value after the division by P; the order here is fixed by n_pos and n_neg alone, so
 * all outputs are the same on every launch: a point alone or inside a grid, from any chan_rs, on any stream.
 * One launch, one workgroup per grid point: the larger class's keys are sorted in LDS and written to the point's row of
 * `workspace`, the smaller class's are sorted in the same LDS, and each sorted array is walked once, its tie runs counted
 * by position and the other class's counts found by binary search.  No float atomics, no arrival counter, nothing passes
 * between workgroups.  `workspace`: DEVICE memory of at least ammc_curve_sweep_workspace_bytes(g * s, n_pos, n_neg) bytes
 * (g * s rows of max(n_pos, n_neg) words, a row rounded up to 64 words; 0 for a non-positive argument or a class over the
 * capacity), scratch of this launch alone.
 * Capacity: max(n_pos, n_neg) <= ammc_curve_sweep_max_class() = 32768 (128 KiB of the CU's 160 KiB of LDS).
 * AMMC_EINVAL: everything ammc_fusion_sweep_f32 refuses but its capacity; a class over this capacity; a null output or
 * workspace; pts, thr or workspace not 4-byte aligned, two_u or sums not 8-byte aligned; workspace_bytes below the
 * query's answer for g * s points.  AMMC_EUNSUP: g * s >= 2^31.  All of them are decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ammc_curve_sweep_max_class(void);
int64_t ammc_curve_sweep_workspace_bytes(int32_t points, int32_t n_pos, int32_t n_neg);
int ammc_curve_sweep_f32(const float* chan, int64_t chan_rs, int32_t k, int32_t n, const float* w, int32_t g, const float* sm,
                         int32_t s, const int32_t* pos_idx, int32_t n_pos, const int32_t* neg_idx, int32_t n_neg,
                         int64_t* two_u, int32_t* pts, float* thr, double* sums, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-video pair counts (csrc/video_pairs.hip): ammc_fusion_sweep_f32's count split by the video of either frame - what
 * the macro AUC and a bootstrap over videos are made of.
 * chan, chan_rs, k, n, w, g, sm, s, pos_idx, n_pos, neg_idx, n_neg and key[i] are exactly those of ammc_fusion_sweep_f32:
 * rounded fp32, left to right, nothing contracted, key = t + 0.0f, the smoothing's neighbour taken across the WHOLE
 * sequence - a video's first scored frame keeps the previous video's last frame as its neighbour.
 *   pos_off  int32 [v + 1]: video x's positive frames are pos_idx[pos_off[x] .. pos_off[x + 1]); neg_off int32 [v + 1]
 *            likewise into neg_idx.  Non-decreasing, the first entry 0, the last n_pos (n_neg); a video may have no frame
 *            of either class, or of both.  DEVICE arrays, like the others.  (An offset outside its list is clamped into
 *            it and a segment to max_segment: meaningless counts, never an access outside an array.)
 *   max_segment  the caller's bound on the longest segment of the class that is sorted - the smaller one, the negatives
 *            when n_neg <= n_pos: it sizes the workgroup's LDS.  The size of that class is always a valid bound.
 *   pairs    int64 [g][s][v][v]:
 *              pairs[gi][si][a][b] = sum over the positive frames p of video a and the negative frames q of video b of
 *                                    (2 * [key_p > key_q] + [key_p == key_q])
 *            exact.  Every element is written exactly once by a plain store, a pair with an empty side as 0: nothing
 *            needs clearing beforehand.
 * The sum of a block is two_u[gi][si]; pairs[a][a] / (2.0 * P_a * Q_a) is video a's own AUC; a replica that draws video
 * x mult[x] times has two_u = sum_ab mult[a] * mult[b] * pairs[a][b] over 2 * (sum mult[a] P_a) * (sum mult[b] Q_b).
 * One launch, one workgroup per (grid point, video of the sorted class): that video's keys are sorted in LDS, the other
 * class is walked once, each frame located by two binary searches and its count added to its video's int64 total in LDS
 * (a wave's sum, one integer LDS add).  No float arithmetic beyond the key, no global atomics, nothing passes between
 * workgroups: the same integers on every launch, for a point alone or inside a grid, on every stream.
 * Capacity: max_segment <= ammc_video_pairs_max_segment() = 32768, v <= ammc_video_pairs_max_videos() = 1024 (together
 * 140 KiB of the CU's 160 KiB of LDS).
 * AMMC_EINVAL: everything ammc_fusion_sweep_f32 refuses but its capacity; a null offset vector or one not 4-byte aligned;
 * v < 1 or over its capacity; max_segment < 1 or over its capacity.  AMMC_EUNSUP: g * s * v >= 2^31 (the grid's x
 * dimension).  All of them are decided before any HIP call.
 *
 * ammc_bootstrap_pairs_i64: the bilinear form above for b multiplicity rows and m blocks at once.
 *   pairs    int64 [m][v][v], every entry >= 0 (ammc_video_pairs_f32's output, [g * s] flattened, or any part of it)
 *   mult     int32 [b][v], every entry >= 0: how often replica r draws video x
 *   out      int64 [b][m]:  out[r][j] = sum over a, b of mult[r][a] * mult[r][b] * pairs[j][a][b]
 * exact in int64 under the PRECONDITION the caller checks per replica: 2 * P_r * Q_r < 2^63 with P_r = sum mult[r][a] P_a
 * and Q_r = sum mult[r][b] Q_b, the replica's own denominator - it bounds the sum, whose terms are all non-negative.
 * One launch, a workgroup per (128 replicas, block), a thread per replica; one writer per element, plain stores.
 * AMMC_EINVAL: a null pointer; m < 1, b < 1, v < 1 or v over ammc_video_pairs_max_videos(); pairs or out not 8-byte
 * aligned, mult not 4-byte aligned.  AMMC_EUNSUP: more than 65535 * 128 replicas (the grid's y dimension).
 * ---------------------------------------------------------------------------------------- */
int ammc_video_pairs_max_segment(void);
int ammc_video_pairs_max_videos(void);
int ammc_video_pairs_f32(const float* chan, int64_t chan_rs, int32_t k, int32_t n, const float* w, int32_t g, const float* sm,
                         int32_t s, const int32_t* pos_idx, int32_t n_pos, const int32_t* neg_idx, int32_t n_neg,
                         const int32_t* pos_off, const int32_t* neg_off, int32_t v, int32_t max_segment, int64_t* pairs,
                         void* stream);
int ammc_bootstrap_pairs_i64(const int64_t* pairs, int32_t m, int32_t v, const int32_t* mult, int32_t b, int64_t* out,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Pixel-level evaluation (csrc/pixel_scores.hip): what the pixel-level criterion of Mahadevan et al. needs of a score
 * map and a ground-truth mask, per sample, from a pass of its own.
 *   map      fp32 [batch][h][w], higher = more anomalous; a sample contiguous (h * w floats), samples map_bs floats apart
 *   mask     uint8 [batch][h][w], nonzero = anomalous; a sample contiguous, samples mask_bs bytes apart
 * Both are DEVICE arrays.  With M(b) the mask pixels of sample b:
 *   m[b]        = |M(b)|
 *   kth[b]      = the k-th largest map value over M(b), counted with multiplicity, k = (m * frac_num + frac_den - 1) /
 *                 frac_den in int64 = ceil(frac_num * m / frac_den): at least the fraction frac_num / frac_den of M(b) is
 *                 >= a threshold t exactly when kth[b] >= t.  (frac 1/1: the minimum over M(b); m * num <= den: max_in)
 *   max_in[b]   = the largest value over M(b);  max_out[b] = the largest value over the pixels outside M(b)
 *   an empty set gives -inf: kth and max_in where m == 0, max_out where m == h * w
 * Every float output is one of the stored map values, bit for bit.  No floating-point operation touches a map value:
 * every comparison is an unsigned comparison of key(bits) = bits has its sign bit ? ~bits : bits | 0x80000000, which
 * orders all non-NaN values as their values do (-0.0 one step below +0.0), denormals and negative values included.  NaN
 * is the CALLER's duty to keep out of the map: a NaN ranks by its key (above +inf or below -inf, by its sign) and
 * nothing reports it; check the returned values for finiteness.
 * One launch, one workgroup per sample: a radix select over the keys in three passes (11, 11 and 10 bits) that re-read
 * the sample, integer histograms in LDS.  Plain stores, every output written once by one thread, nothing passes between
 * workgroups, no global atomics: the outputs of sample b are a function of (map[b], mask[b], h * w, frac_num, frac_den)
 * and of nothing else - not the batch size, the sample's place in the batch, a stride or an alignment (16-byte map
 * loads and 4-byte mask loads where the bases and batch strides allow, 4-byte and 1-byte loads otherwise).
 * AMMC_EINVAL: a null pointer; batch, h or w < 1; h * w > 2^24; frac_num < 1, frac_den < frac_num or frac_den > 4096;
 * with batch > 1 a batch stride < h * w; map or an output not 4-byte aligned.  All decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ammc_pixel_scores_f32(const float* map, int64_t map_bs, const uint8_t* mask, int64_t mask_bs, int32_t batch, int32_t h,
                          int32_t w, int32_t frac_num, int32_t frac_den, int32_t* m, float* kth, float* max_in,
                          float* max_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Qualitative evaluation (csrc/render.hip): finished uint8 panels of the predicted and target frames, the Middlebury
 * colour code of the predicted and target flows and heat maps of their per-pixel errors, from a pass of its own.
 *   rgb_pred, rgb_target   fp32 [batch][3][h][w] on the model's [-1, 1] range
 *   op_pred, op_target     fp32 [batch][2][h][w] flows
 * DEVICE arrays, a sample contiguous, each with a batch stride of its own in floats (>= the sample's size).
 * All arithmetic is fp32; no product is contracted into a sum except where an fma is named.
 * Frame tile.  Per channel u8 = floor(clamp((x + 1) * 127.5, 0, 255) + 0.5), taken of the real value: x is clamped to
 *   [-1, 1] (a NaN to -1), y = fma(x, 127.5, 128), n = floor(y), and n steps back by one where fma(x, 127.5, 128 - n) < 0.
 * Flow tile.  The Middlebury colour code.  wheel[1..55][3]: the colour wheel of the segment lengths 15, 6, 4, 11, 13, 6
 *   (red-yellow, yellow-green, green-cyan, cyan-blue, blue-magenta, magenta-red; along a segment of length n one channel
 *   holds 255 and one ramps floor(255 i / n), up in the 1st, 3rd and 5th segment and down from 255 in the others), each
 *   value divided by 255.  u = su * flow[0], v = sv * flow[1].  A pixel with |u| > 1e7, |v| > 1e7 or a NaN is UNKNOWN: it
 *   is drawn black and enters no maximum (as u = v = 0).  raw = sqrt(u * u + v * v); maxrad: the sample's largest raw,
 *   or a supplied value; inv = 1 / (maxrad + 2^-52); a = atan2(-v, -u) / pi; fk = (a + 1) / 2 * 54 + 1; k0 = floor(fk)
 *   (kept in 1..55); k1 = k0 + 1, 56 wrapping to 1; f = fk - k0; per channel col = (1 - f) * wheel[k0] + f * wheel[k1];
 *   a pixel is INSIDE when raw <= maxrad, then col = 1 - rad * (1 - col) with rad = min(raw * inv, 1); otherwise
 *   col = col * 0.75; u8 = floor(255 * col).  A zero flow is white.
 * Heat tile.  e = ((d_0^2 + d_1^2) + ...) / c with d_ch = 0.5 * (target_ch - pred_ch): ammc_error_maps_f32's `pixel`.
 *   A NaN e counts as 0, and so does the flow pair's e where either flow is unknown.  t = min(e / heat_max, 1), 0 where
 *   heat_max <= 0, with heat_max the sample's largest e or a supplied value; colour (r, g, b) = clamp(1.5 - |4 t - 3|,
 *   0, 1), clamp(1.5 - |4 t - 2|, 0, 1), clamp(1.5 - |4 t - 1|, 0, 1); u8 = floor(((1 - alpha) * grey + (alpha * 255) *
 *   colour) + 0.5) with grey = (r + g + b) / 3 of the target's frame tile bytes, 128 for the flow pair.
 *
 * ammc_render_stats_f32: stats[b] = (largest raw of op_target, largest raw of op_pred, largest e of the frame pair,
 *   largest e of the flow pair), fp32 [batch][4].  An input may be NULL (the frame pair: both or neither; not all
 *   four): the values that would read it are 0.  A memset node that zeroes stats and one kernel launch on `stream`; the
 *   workgroups publish their maxima by integer atomic maxima of the floats' bits (non-negative, never NaN: the order of
 *   the bits is the order of the values), so stats holds THE maxima: the same bits on every launch and for every launch
 *   geometry, whatever stats held before, equal to an IEEE fp32 restatement (square root correctly rounded).
 * ammc_render_panels_u8: out[b] = uint8 [rows * h][cols * w][3], samples out_bs BYTES apart: tile tiles[r * cols + c]
 *   at rows [r h, (r + 1) h) and columns [c w, (c + 1) w).  tiles: a HOST array of rows * cols <= 6 tile ids, read
 *   during the call, each id at most once: 0 rgb_target, 1 rgb_pred, 2 rgb_heat, 3 op_target, 4 op_pred, 5 op_heat.
 *   An input no chosen tile reads may be NULL.  Normalisation: max_rad [batch] (both flow tiles), heat_rgb [batch],
 *   heat_op [batch] where given, otherwise stats [batch][4] as ammc_render_stats_f32 left them on the same stream:
 *   op_target by stats[b][0]; op_pred by stats[b][0] too (flow_each = 0: the two tiles are comparable) or by its own
 *   stats[b][1] (flow_each = 1).  stats may be NULL where nothing reads it.  One launch; plain stores, every byte
 *   written once; a sample's panel is a function of the sample and the arguments alone.  16-byte loads and dword stores
 *   where w % 4 == 0 and the bases and batch strides allow, scalar loads and byte stores otherwise: the same bytes.
 * ammc_flow_colour_u8: the colour code of a flow batch alone, out[b] = uint8 [h][w][3]; max_rad [batch] or NULL: by the
 *   sample's own maximum, taken into workspace (4 * batch floats, zeroed inside the call) by the stats launch.
 * AMMC_EINVAL: a missing pointer; batch, h or w < 1; su or sv not finite; alpha outside [0, 1]; flow_each not 0 / 1;
 *   rows or cols < 1, rows * cols > 6, a tile id outside 0..5 or given twice; a float pointer not 4-byte aligned; with
 *   batch > 1 a batch stride smaller than a sample.  AMMC_EUNSUP: batch > 65535; h * w > 2^28.
 * All of them are decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ammc_render_stats_f32(const float* rgb_pred, int64_t rp_bs, const float* rgb_target, int64_t rt_bs, const float* op_pred,
                          int64_t fp_bs, const float* op_target, int64_t ft_bs, int32_t batch, int32_t h, int32_t w, float su,
                          float sv, float* stats, void* stream);
int ammc_render_panels_u8(const float* rgb_pred, int64_t rp_bs, const float* rgb_target, int64_t rt_bs, const float* op_pred,
                          int64_t fp_bs, const float* op_target, int64_t ft_bs, int32_t batch, int32_t h, int32_t w, float su,
                          float sv, const int32_t* tiles, int32_t rows, int32_t cols, const float* stats, int32_t flow_each,
                          const float* max_rad, const float* heat_rgb, const float* heat_op, float alpha, uint8_t* out,
                          int64_t out_bs, void* stream);
int ammc_flow_colour_u8(const float* flow, int64_t flow_bs, int32_t batch, int32_t h, int32_t w, float su, float sv,
                        const float* max_rad, float* workspace, uint8_t* out, int64_t out_bs, void* stream);

/* ------------------------------------------------------------------------------------------
 * Region-based evaluation (csrc/region_scores.hip): what the region-based detection criterion (RBDC, Ramachandra and
 * Jones) needs of a score map and a frame's ground-truth regions, per sample and threshold, from a pass of its own.
 *   map         fp32 [batch][h][w], higher = more anomalous; a sample contiguous, samples map_bs floats apart
 *   mask        uint8 [batch][h][w], nonzero = anomalous; a sample contiguous, samples mask_bs bytes apart
 *   labels      uint8 [batch][h][w], 0 = background, r = ground-truth region r; samples labels_bs bytes apart
 *   thresholds  fp32 [t], any values in any order
 * DEVICE arrays.  connectivity is 8 (a pixel touches its 8 neighbours) or 4 (W, E, N, S only).
 * Detected regions.  At threshold thr the detected regions of a sample are the connected components of
 *   {map >= thr}.  The comparison is the only floating-point operation on a map value; NaN compares false, -0.0 >= +0.0.
 *   Components with fewer than min_area pixels are dropped: they are neither false positives nor able to detect.
 * Ground-truth regions.  The connected components of {mask != 0} with the same connectivity and a min_area of their own,
 *   numbered 1, 2, ... in raster order of each kept component's first pixel (its smallest flat index y * w + x).
 *   ammc_label_regions_u8 writes that label image; count[b] is the TRUE number of kept components, also beyond 32;
 *   components ranked beyond 32 are written as 0.
 * Match.  Detected region C matches ground-truth region G iff |C n G| * den >= num * (|C| + |G| - |C n G|), evaluated in
 *   64-bit integers (num / den = 1 / 10: IoU >= 0.1), 1 <= num <= den <= 4096.  |G| counts the label's pixels.
 * ammc_region_scores_f32, per sample b and threshold index j, at [b * out_rs + j] of four int32 arrays:
 *   n_px    the detected pixels (before min_area)
 *   n_comp  the kept components
 *   n_fp    the kept components that match no ground-truth region
 *   hit     bit r - 1 is set iff some kept component matches region r, r = 1..32
 *   Label values above 32 are treated as BACKGROUND.  All four are functions of the sample's map values, its label image
 *   and the threshold alone - not of thread order, the batch size, the sample's place in the batch, a stride or an
 *   alignment: every atomic is an integer count inside the workgroup's own workspace slice or LDS.
 * One launch each, one workgroup per (sample, threshold) / per sample, labelling by a lock-free union-find that hangs
 * the larger root below the smaller (the root of a component is its first pixel in raster order).  Every loop is
 * bounded before it starts; should the bound on a union's retries ever be hit, n_comp = -1 (n_px = n_fp = hit = 0) or
 * count = -1 reports it.  workspace: ammc_region_workspace_bytes(batch, t, h, w) bytes (3 int32 per pixel, sample and
 * threshold; t = 1 for ammc_label_regions_u8), 4-byte aligned, contents irrelevant before and after;
 * the function returns -1 for sizes the entries refuse.
 * AMMC_EINVAL: a null pointer; batch, h, w, t or min_area < 1; h * w > 2^22; connectivity not 4 or 8; num < 1, den < num or
 * den > 4096; with batch > 1 a batch stride < h * w or out_rs < t; map, thresholds, an int32 output or the workspace not
 * 4-byte aligned; workspace_bytes too small.  AMMC_EUNSUP: batch * t >= 2^31.  All decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int64_t ammc_region_workspace_bytes(int32_t batch, int32_t t, int32_t h, int32_t w);
int ammc_label_regions_u8(const uint8_t* mask, int64_t mask_bs, int32_t batch, int32_t h, int32_t w, int32_t min_area,
                          int32_t connectivity, uint8_t* labels, int64_t labels_bs, int32_t* count, void* workspace,
                          int64_t workspace_bytes, void* stream);
int ammc_region_scores_f32(const float* map, int64_t map_bs, const uint8_t* labels, int64_t labels_bs, int32_t batch, int32_t h,
                           int32_t w, const float* thresholds, int32_t t, int32_t num, int32_t den, int32_t min_area,
                           int32_t connectivity, int32_t* n_px, int32_t* n_comp, int32_t* n_fp, int32_t* hit, int64_t out_rs,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused localisation maps (csrc/fuse_maps.hip): several score maps of different resolution become one smoothed map of
 * the frame's size, its patch means and its largest value, from a pass of its own.
 *   src[c]   fp32 [batch][gh[c]][gw[c]], c < n_ch (1..4); a sample's rows and columns contiguous, samples src_bs[c]
 *            floats apart.  cell[c] >= 1 is the edge of the square of frame pixels one source value covers:
 *            gh[c] is h / cell[c] or ceil(h / cell[c]) and >= 1, gw[c] the same of w.  src, src_bs, gh, gw and cell are
 *            HOST arrays of n_ch entries, read during the call; the maps themselves are DEVICE arrays.
 *   coef     fp32 [n_ch], a DEVICE array (the caller computes it on the device without a host wait)
 *   radius   0..8: the box window is (2 radius + 1)^2;  patch: 8, 16 or 32
 * All arithmetic is fp32 and no product is contracted into a sum.
 *   m_c(b, y, x)   = src[c][b][min(y / cell[c], gh[c] - 1)][min(x / cell[c], gw[c] - 1)]      (blocky, no interpolation)
 *   raw(b, y, x)   = ((coef[0] * m_0 + coef[1] * m_1) + coef[2] * m_2) + coef[3] * m_3, truncated to n_ch terms
 *   pixel[b][y][x] = the sum of raw over the pixels (y', x') of the frame with |y' - y| <= radius and |x' - x| <= radius,
 *                    divided by their number: a count-normalised mean, no zero padding.  Per row of the window the
 *                    columns are added left to right, the row sums top to bottom, each starting from its first term,
 *                    then one division: sums only add (no sliding-window subtraction), so with non-negative inputs a
 *                    value is within (2 n_ch + 4 radius) * 2^-24 relative of the real one.  With n_ch = 1, coef = 1,
 *                    cell = 1 and radius = 0, pixel equals the source bit for bit.
 *   patch_mean[b][i][j] = the sum of pixel over patch (i, j) of ammc_error_maps_f32's grid (patch x patch pixels
 *                    anchored at (0, 0), the last row / column ragged) divided by its true pixel count; per image row
 *                    quads (p0 + p1) + (p2 + p3) left to right, then the rows top to bottom.  [batch][ph][pw], samples
 *                    pm_bs floats apart.
 *   frame_max[b]   = the largest pixel value of the sample, one of them bit for bit.
 * pixel is [batch][h][w], a sample contiguous, samples px_bs floats apart (16-byte stores where the base, px_bs and w
 * are multiples of 4 floats, 4-byte stores otherwise: the same bits).
 * The kernel checks no values: NaN and infinities propagate through the sums, and a NaN pixel makes frame_max NaN.
 * Callers pass non-negative finite maps and coefficients.
 * Two launches: one 256-thread workgroup per 32 x 64 tile of a sample (whole patches live in one workgroup; the tile
 * and its halo are staged in LDS once), then one workgroup per sample over the tiles' maxima.  workspace: batch *
 * ceil(h / 32) * ceil(w / 64) floats, contents irrelevant before and after.  No atomics; every output is written once
 * by one thread and is a function of the sample's own values, coef, the sizes, radius and patch - not of the batch
 * size, the sample's place in the batch, a stride or an alignment.  Equal inputs give equal bits.
 * AMMC_EINVAL: a null pointer; n_ch outside 1..4; batch, h or w < 1; radius outside 0..8; patch not 8, 16 or 32; a
 *   cell < 1 or a grid size that is neither h / cell nor ceil(h / cell) (w alike) or < 1; a float pointer not 4-byte
 *   aligned; with batch > 1 a batch stride smaller than a sample.  AMMC_EUNSUP: h * w > 2^28; batch * tiles >= 2^31.
 * All decided before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ammc_fuse_maps_f32(const float* const* src, const int64_t* src_bs, const int32_t* gh, const int32_t* gw, const int32_t* cell,
                       int32_t n_ch, const float* coef, int32_t batch, int32_t h, int32_t w, int32_t radius, int32_t patch,
                       float* pixel, int64_t px_bs, float* patch_mean, int64_t pm_bs, float* frame_max, float* workspace,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMMC_HIP_H */
