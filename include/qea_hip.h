/*
 * qea_hip.h — C ABI of libqea_hip.so, the MI355X (gfx950) kernel library under the
 * preprocessor-training inner loop of tataganesh/Query-Efficient-Approx-to-improve-OCR.
 *
 * The reference has no FFI of its own: every op on the path is a stock torch.nn call
 * (SURVEY.md §2.3).  Each entry point below therefore cites the reference line that
 * ISSUES the op it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *    synchronises, nothing is allocated (caller owns outputs and workspaces);
 *  - return 0 on success, <0 on error (qea_last_error() gives the message); never throws;
 *  - activations are NHWC fp32: element (b,h,w,c) of a tensor with pixel stride `ld`
 *    lives at ((b*H+h)*W+w)*ld + c, so channel slices of wider buffers (UNet skip
 *    concatenations) are addressed with a base pointer + ld and no copy;
 *  - conv weights are [Cout][KH][KW][Cin] (= the checkpoint's OIHW tensor in
 *    torch.channels_last memory format), ConvTranspose2d weights are
 *    [Cin][KH][KW][Cout] (= IOHW in channels_last); LSTM/Linear weights are torch's
 *    row-major [out][in].
 */
#ifndef QEA_HIP_H
#define QEA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QEA_OK 0
#define QEA_ERR_INVALID (-1)
#define QEA_ERR_LAUNCH (-2)
#define QEA_ERR_WORKSPACE (-3)

/* ABI version; bumped whenever a struct below changes or entry points are added. */
int qea_version(void);
const char* qea_last_error(void);

/* Event-bracketed timing of one kernel class, for bench.py's roofline leg: while enabled,
 * every launch of that class is bracketed by hipEvents on its own stream; read() syncs
 * the events and returns summed milliseconds, algorithmic flops / bytes and launch count. */
#define QEA_PROF_CONV_IGEMM 0
#define QEA_PROF_CONV_WGRAD 1
#define QEA_PROF_LSTM_STEP 2
#define QEA_PROF_NCLASS 3
int qea_prof_enable(int klass, int on);
int qea_prof_reset(void);
int qea_prof_read(int klass, double* ms, double* flops, double* bytes, int64_t* launches);
/* per-launch view of the same records (in launch order): up to `capacity` entries, *count = recorded launches */
int qea_prof_read_launches(int klass, double* ms, double* flops, int64_t capacity, int64_t* count);
/* The same sums restricted to the launches one kernel took.  Tags of QEA_PROF_CONV_IGEMM: the tile id, except for the
 * split-bf16 LDS-halo kernel, whose template instantiation conv3x3_halo_bf3_kernel<CIN, COUT, .., STATS> is
 * QEA_PROF_TAG_HALO_BF3(CIN, COUT, STATS) — the name rocprofv3 lists it under, so that bench.py's roofline figures of the
 * dominant kernel can be checked against the kernel trace. */
#define QEA_PROF_TAG_HALO_BF3(cin_chunk, cout_group, stats) (24000 + ((cin_chunk) == 64 ? 1000 : 0) + (cout_group) + ((stats) ? 500 : 0))
/* (+ 20 * image width for the small-image instantiations, + 5 for the two-way fp16 instantiation: each is its own kernel in a trace); + 2000 * pool_kw for the instantiations with the fused max-pool, ABI v7) */
int qea_prof_read_tagged(int klass, int32_t tag, double* ms, double* flops, double* bytes, int64_t* launches);
/* The part of a class's algorithmic flops that ran through the split-bf16 kernels (six bf16 MFMAs per fp32
 * multiply-add): bench.py blends the fp32 and the bf16/6 matrix peaks with it. */
int qea_prof_read_split_bf16(int klass, double* flops);
/* ABI v6: the part that ran through the two-way fp16 split (three fp16 MFMAs per fp32 multiply-add) */
int qea_prof_read_split_f16(int klass, double* flops);

/* Which matrix instruction the GEMM-class launches use: 0 = split-bf16 tiles where the dispatcher prefers them
 * (default), 1 = every product on v_mfma_f32_32x32x2_f32.  The initial value comes from QEA_MFMA=f32 in the
 * environment; tests and bench.py's native-fp32 leg switch it at run time.  Returns the previous mode, or
 * QEA_ERR_INVALID for a mode other than 0/1 (mode -1 only queries).
 *
 * PROCESS-GLOBAL STATE, one of two exceptions to "no global mutable state" (the other: the profiling registry above, which
 * only records).  The mode is read by every GEMM-class entry point at LAUNCH time and selects the kernel, i.e. the summation
 * order of the results: a caller that flips it while another host thread of the same process is launching changes that
 * thread's results (both forms are fp32-class — see DESIGN.md §4 — but not bit-identical).  The library is used with one host
 * thread per GPU process; a process that needs both forms concurrently must serialise the switch with its
 * launches itself.  A single launch can be pinned regardless of the mode through its descriptor's `tile` field (tiles 1-9: fp32
 * instruction, 20-25: split-bf16). */
#define QEA_MFMA_SPLIT_BF16 0
#define QEA_MFMA_F32 1
int qea_set_mfma_mode(int mode);

/* ------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the matrix cores with fp32-class accuracy: v_mfma_f32_32x32x2_f32, or — by default
 * for N >= 64-128 output channels and K >= 256 (tiles 20-23) — the split-bf16 form: fp32 operands split on the fly into
 * three bf16 values x = h + m + l, six v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation (at least as close to
 * the fp64 result as the fp32 instruction on long reductions).  QEA_MFMA=f32 in the environment keeps every launch on
 * the fp32 instruction.
 *   y[b,oh,ow,n] = epilogue( sum_{kh,kw,c} x[b, oh*sh+kh-ph, ow*sw+kw-pw, c] * w[n,kh,kw,c] )
 * Replaces nn.Conv2d forward at models/model_unet.py:78-109 (3x3 p1, bias=False),
 * models/model_crnn.py:38-45,49-55 (3x3 p1 and the 2x2 p0 conv7); run on
 * flipped/transposed weights it is also their input-gradient; with KH=KW=2, stride 2 it
 * is the input-gradient of nn.ConvTranspose2d (model_unet.py:25-41); with out_mode
 * QEA_OUT_CONVT it is ConvTranspose2d forward; with KH=KW=1 it is the plain GEMM
 * y = x * w^T of nn.LSTM's input projection and nn.Linear (model_crnn.py:9-10,19-20).
 * Cin must be a multiple of 32 (the C_in = 1 layers use qea_conv_c1_*).
 * Epilogue order: v = acc * scale[n] + bias[n]; relu; mask (v = mask[row,n] > 0 ? v : 0);
 * accumulate (y += v).
 * ---------------------------------------------------------------------------------- */
#define QEA_OUT_NHWC 0  /* row m=(b,oh,ow) -> y + m*ldy                                  */
#define QEA_OUT_TBC 1   /* OH==1: row (b,ow) -> y + (ow*B+b)*ldy  (CRNN map_to_sequence,  */
                        /* models/model_crnn.py:23-28)                                    */
#define QEA_OUT_CONVT 2 /* N = 4*Cout', n=(a,bb,co): y[b,2oh+a,2ow+bb,co]; bias[co]        */

typedef struct qea_conv_desc {
  const float* x;     /* input, NHWC, pixel stride ldx                                   */
  const float* w;     /* [N][KH*KW*Cin]                                                   */
  float* y;           /* output                                                           */
  const float* scale; /* [N] or NULL                                                      */
  const float* bias;  /* [N] or NULL  (QEA_OUT_CONVT: [N/4])                              */
  const float* mask;  /* same row/channel indexing as y with stride ldmask, or NULL       */
  int32_t B, H, W, Cin;
  int32_t OH, OW, N;
  int32_t KH, KW, pad_h, pad_w, stride_h, stride_w;
  int32_t ldx, ldy, ldmask;
  int32_t relu;       /* 0/1                                                              */
  int32_t accumulate; /* 0/1                                                              */
  int32_t out_mode;   /* QEA_OUT_*                                                        */
  int32_t tile;       /* 0 = auto; else forced tile config id (tests / tuning)            */
  /* ABI v2: optional PRE-SPLIT operands of the split-bf16 tiles (NULL: split on the fly).  Both in the P3 format written
   * by qea_split_planes: x_planes from x (M = B*H*W rows, Cin channels), w_planes from w (N rows, K = KH*KW*Cin).   */
  const void* x_planes;
  const void* w_planes;
  /* ABI v3: fused BatchNorm batch statistics.  When non-NULL the launch also writes, per partial block k and output column
   * n, stats[(k*N + n)*2 + {0,1}] = fp64 sum / sum of squares of the stored outputs of that block's rows;
   * qea_conv_igemm_stats_blocks(d) gives the block count (0: this launch has no such epilogue — run qea_bn_train_stats).
   * qea_bn_train_stats_from_partials turns the partials into the BatchNorm coefficients. */
  double* stats;
  /* ABI v4: filter of a 3x3 pad-1 stride-1 layer as bf16 planes in MFMA-fragment order (qea_pack_frag_planes): operand of the
   * split-bf16 LDS-halo kernel (tile 24: Cin = 32 or 64k <= 512, N in {32, 64, 128k}; W % 32 == 0 and H % 4 == 0 (8 for Cin = 32),
   * or — round 3, no ABI change — whole small images per tile: 4x16 / 2x8 pixel images with Cin = 64k, N = 128k);
   * qea_conv_igemm_wants_frag_planes(d) tells.  Without it such a launch runs on the fp32 halo / generic tiles. */
  const void* w_frag_planes;
  /* ABI v6: TWO-WAY fp16 split of the LDS-halo kernel (tile 24).  When non-NULL: device pointer to ONE float = the largest finite
   * |x| of the input tensor (qea_absmax), and w_frag_planes must then hold the FP16 planes of qea_pack_frag_planes_f16.  Both
   * operands are scaled by powers of two into fp16's range and split into h + l (11 + 11 bits); a product is three
   * v_mfma_f32_32x32x16_f16 (lh, hl, hh) instead of six bf16 ones, the accumulators are un-scaled in the epilogue (exact).
   * Same accuracy class as the three-way bf16 split, half the matrix instructions, two thirds of the LDS.
   * The hybrid tiles (20-23, 25 with w_planes and no x_planes) take the same switch: w_planes must then come from
   * qea_split_planes_f16.  NULL: the bf16 form. */
  const float* x_absmax;
  /* ABI v6: zero-filled float slot receiving max |v| of the finite values this launch STORES (see qea_bn_apply's absmax_out);
   * honoured by the LDS-halo kernel (tile 24) and by the generic split tiles 20-23 / 25 (incl. QEA_OUT_CONVT); NULL = off. */
  float* y_absmax;
  /* ABI v7: the max-pool that FOLLOWS the layer, fused into the epilogue of the LDS-halo kernel (nothing in the reference: fn.max_pool2d
   * after relu(conv), models/model_crnn.py:49,51; self.poolN(encN), models/model_unet.py:52-59 in the inference pass).  pool_y non-NULL:
   * besides y the launch writes pool_y [B, H/2, W/pool_kw, N] (pixel stride ldpool) = max over 2 x pool_kw windows of the stored
   * values, first maximum in scan order / NaN propagating as qea_maxpool_fwd — bit-identical to that call on y — and folds its
   * abs-max into pool_absmax (zero-filled slot, may be NULL).  Only where qea_conv_igemm_can_pool(d, pool_kw) returns 1 and the fp16
   * operands (x_absmax, w_frag_planes of qea_pack_frag_planes_f16) are given; anything else is QEA_ERR_INVALID. */
  float* pool_y;
  int32_t ldpool;
  int32_t pool_kw;
  float* pool_absmax;
  /* ABI v7: the launch is an INPUT GRADIENT (3x3 dgrad on the LDS-halo kernel, fp16 operands) whose output da feeds the backward of a
   * train-mode BatchNorm(+ReLU) (models/model_unet.py:78-109 under autograd).  bst_y non-NULL (with `stats`): instead of the forward
   * statistics, `stats` receives per partial block the fp64 sums of dz = da * [bst_scale * bst_y + bst_shift > 0] and of
   * dz * (bst_y - mean) * invstd, mean / invstd = bst_stat64[0..N) / [N..2N) — the reductions qea_bn_bwd otherwise makes in a pass of
   * its own over da and bst_y; qea_bn_bwd_from_partials consumes them.  Block count: qea_conv_igemm_stats_blocks. */
  const float* bst_y;
  int32_t ldbst;
  const double* bst_stat64;
  const float* bst_scale;
  const float* bst_shift;
} qea_conv_desc;

int qea_conv_igemm(const qea_conv_desc* d, void* stream);
/* 1 when qea_conv_igemm would run this launch on a split-bf16 tile (so that pre-split operands pay), else 0 */
int qea_conv_igemm_uses_split_bf16(const qea_conv_desc* d);
int qea_conv_igemm_stats_blocks(const qea_conv_desc* d);
/* ABI v7: 1 when this launch (pool_y aside) has an LDS-halo instance with the fused 2 x kw max-pool (kw = 1 or 2) */
int qea_conv_igemm_can_pool(const qea_conv_desc* d, int32_t kw);
/* 1: the launch would run on the LDS-halo 3x3 kernel (tile 24) given w_frag_planes = qea_pack_frag_planes / _f16 of the filter;
 * 2 (ABI v7): it would run on the 1x1 LDS tile (tile 26) given x_absmax and w_frag_planes = qea_pack_frag_planes_f16_1x1; 0: neither */
int qea_conv_igemm_wants_frag_planes(const qea_conv_desc* d);
/* ABI v7 (additive).  Filter [N][K] of a 1x1 stride-1 GEMM (N % 128 == 0, K % 64 == 0) as two fp16 planes in the fragment order of
 * tile 26, scaled from wmax[0] like qea_pack_frag_planes_f16, followed by one float = the inverse scale.  Tile 26 replaces the
 * generic split tiles for the launches behind nn.ConvTranspose2d forward (/root/reference/models/model_unet.py:25-44, 61-73), the BiLSTM
 * input projections and their input gradients (/root/reference/models/model_crnn.py:9) when the two-way fp16 split is on. */
size_t qea_pack_frag_planes_f16_1x1_bytes(int32_t N, int32_t K);
int qea_pack_frag_planes_f16_1x1(const float* w, int32_t N, int32_t K, const float* wmax, void* planes, void* stream);
/* ABI v6.  out[0] = max |x[r*ld + c]| over r < M, c < C with NaN / inf elements ignored (a non-finite element must not decide the
 * scale of the finite ones: it stays non-finite in the products it enters).  One pass over the tensor; `out` is overwritten. */
int qea_absmax(const float* x, int32_t ld, int64_t M, int32_t C, float* out, void* stream);
/* ABI v6.  The filter [N][9][Cin] as two fp16 planes in the fragment order of qea_pack_frag_planes, scaled by the power of two that
 * qea_f16_scale derives from wmax[0] (= qea_absmax of the filter), followed by one float holding the inverse scale.
 * qea_pack_frag_planes_f16_bytes gives the buffer size. */
size_t qea_pack_frag_planes_f16_bytes(int32_t N, int32_t Cin);
/* ABI v6.  The row format of qea_split_planes with TWO fp16 planes per value, scaled by the power of two of xmax[0] (= qea_absmax of
 * x), the 128-byte zero tail, then one float = the inverse scale: the filter operand (w_planes) of the hybrid tiles 20-23 / 25
 * when qea_conv_desc.x_absmax is given. */
size_t qea_split_planes_f16_bytes(int64_t M, int32_t C);
int qea_split_planes_f16(const float* x, int32_t ld, int64_t M, int32_t C, const float* xmax, void* planes, void* stream);
int qea_pack_frag_planes_f16(const float* w, int32_t N, int32_t Cin, const float* wmax, void* planes, void* stream);
size_t qea_pack_frag_planes_bytes(int32_t N, int32_t Cin);
int qea_pack_frag_planes(const float* w, int32_t N, int32_t Cin, void* planes, void* stream);

/* P3 format of a fp32 matrix [M][ld] with C used columns (C % 16 == 0): planes[row][C/16][3][16] bf16 — per 16-column
 * slice the three bf16 planes h, m, l of x = h + m + l (|x - (h+m+l)| <= 2^-24 |x|), 96 contiguous bytes — followed by
 * a 128-byte zero tail (the source of out-of-image taps).  One HBM pass: 4 B read + 6 B written per element, against
 * ~5.5 VALU operations per element for EVERY tap and N-tile when the conv kernel splits on the fly.  Used for the
 * activations / gradients entering nn.Conv2d forward, input-gradient (models/model_unet.py:78-109,
 * models/model_crnn.py:38-45) and for their filters. */
size_t qea_split_planes_bytes(int64_t M, int32_t C);
int qea_split_planes(const float* x, int32_t ld, int64_t M, int32_t C, void* planes, void* stream);

/* ------------------------------------------------------------------------------------
 * Weight gradient on the matrix cores (fp32 MFMA, or the split-bf16 form of qea_conv_igemm for R, C >= 64 with one
 * of them >= 128: tiles 20-22); reduction over pixels, split over blocks, order-fixed second pass: bit-reproducible.
 *   dw[r][kh][kw][c] (+)= sum_{b,ph,pw} p[b,ph,pw][r] * q[b, ph*sh+kh-pad_h, pw*sw+kw-pad_w][c]
 * nn.Conv2d weight gradient (autograd of models/model_unet.py:78-109, model_crnn.py:38-45):
 *   p = dY, q = X.  nn.ConvTranspose2d (model_unet.py:25-41): p = X, q = dY, KH=KW=2,
 *   stride 2, pad 0 -> dw in [Cin][2][2][Cout].  nn.Linear / nn.LSTM weights: KH=KW=1.
 * R, C, ldp, ldq multiples of 4.  Workspace: qea_conv_wgrad_workspace_bytes(d).
 * ---------------------------------------------------------------------------------- */
typedef struct qea_wgrad_desc {
  const float* p;   /* [B*PH*PW][ldp], R channels used                                    */
  const float* q;   /* NHWC image [B,QH,QW] with pixel stride ldq, C channels used        */
  float* dw;        /* [R][KH*KW][C]                                                      */
  void* workspace;
  size_t workspace_bytes;
  int32_t B, PH, PW, QH, QW, R, C;
  int32_t KH, KW, pad_h, pad_w, stride_h, stride_w;
  int32_t ldp, ldq;
  int32_t accumulate; /* dw += result                                                     */
  int32_t splits;     /* 0 = auto                                                         */
  int32_t tile;       /* 0 = auto; 23 = the nine-tap LDS-halo kernel (with both abs-max pointers and R, C multiples of 64: its
                       * producer / consumer form, round 4), 29 = the nine-tap kernel in the round-3 form (every wave stages),
                       * 6 = the fp32 LDS-halo kernel; every other id is a row of TILES in csrc/conv_wgrad.hip (route() there
                       * holds the order of preference for tile 0) */
  /* ABI v6: when BOTH are non-NULL (device pointers to one float each: qea_absmax of p and of q) a launch that runs on a split tile —
   * the nine-tap LDS-halo kernel (3x3 pad 1 stride 1, PW in {16, 32k}, R and C multiples of 32) or tiles 20-22 — takes the TWO-way
   * fp16 split: three MFMAs per product instead of six (see qea_conv_desc.x_absmax).  Other launches ignore them. */
  const float* p_absmax;
  const float* q_absmax;
  /* ABI v8 (the descriptor grew at its end: v7 callers must re-compile).  dbias [R] (NULL = off): the bias gradient = column sums of p
   * (`nn.Conv2d(bias=True)` under autograd, models/model_crnn.py:38-45), accumulated with the same `accumulate` flag as dw.  Taken only by the
   * producer / consumer nine-tap form, where every p element passes through the staging waves' registers anyway (no pass of its own,
   * no qea_colsum launch): ask qea_conv_wgrad_fuses_bias(d) first — with dbias set, any other form refuses the call. */
  float* dbias;
} qea_wgrad_desc;

int qea_conv_wgrad_fuses_bias(const qea_wgrad_desc* d);
/* Additive (no ABI bump).  1 when the launch this descriptor routes to reads p_absmax / q_absmax once both are set (the nine-tap kernel in
 * any form, tiles 20-22), 0 when it would ignore them (the fp32 tiles): lets a caller skip the two qea_absmax passes nothing would read.
 * Depends on the shape, the tile and the MFMA mode only, not on whether the pointers are set; needs no device pointers. */
int qea_conv_wgrad_wants_absmax(const qea_wgrad_desc* d);
size_t qea_conv_wgrad_workspace_bytes(const qea_wgrad_desc* d);
int qea_conv_wgrad(const qea_wgrad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * BatchNorm2d over NHWC rows [M = B*H*W][C] (nn.BatchNorm2d at models/model_unet.py:92,105 and
 * models/model_crnn.py:42,44; mode policy train_nn_patch.py:226-227,312-314, utils.py:113-115).
 * Statistics are accumulated in fp64.  a = y*scale + shift (+ReLU) with
 * scale = gamma*invstd, shift = beta - mean*scale.
 * qea_bn_train_stats : batch mean / biased var -> mean, invstd, scale, shift; running stats
 *                      updated in place with momentum and the UNBIASED variance.
 * qea_bn_eval_coeff  : the same four vectors from the running statistics (conv_bias, if given,
 *                      is folded into shift).
 * qea_bn_bwd         : dz = da * relu'; dgamma = sum dz*xhat, dbeta = sum dz;
 *                      training: dy = scale*(dz - mean(dz) - xhat*mean(dz*xhat)), eval: dy = scale*dz.
 *                      dy may alias da.  relu' comes from a > 0 when a is given, or — without reading
 *                      a — from y*relu_scale + relu_shift > 0 (the very fused multiply-add qea_bn_apply
 *                      evaluates, hence the identical mask); both NULL: no ReLU.
 * stat64 (optional, [2][C] doubles): the batch mean and invstd unrounded; handing it back to
 * qea_bn_bwd keeps the per-channel constants of the backward in fp64 — they are common to every
 * pixel, so fp32 rounding of them is a CORRELATED error that later per-channel sums amplify by M.
 * Workspace for stats / bwd / colsum: qea_colreduce_workspace_bytes(M, C).
 * ---------------------------------------------------------------------------------- */
size_t qea_colreduce_workspace_bytes(int64_t M, int32_t C);
int qea_bn_train_stats(const float* y, int32_t ldy, int64_t M, int32_t C, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var, float* mean_out,
                       float* invstd_out, float* scale_out, float* shift_out, double* stat64, void* workspace,
                       size_t workspace_bytes, void* stream);
/* the same, from the per-block partial sums a convolution's fused-statistics epilogue wrote (qea_conv_desc.stats).  The
 * buffer must hold QEA_BN_PARTIAL_SCRATCH_ROWS more rows ([C][2] doubles each) behind the `blocks` partial rows: with many
 * blocks the reduction runs in two order-fixed stages through them. */
#define QEA_BN_PARTIAL_SCRATCH_ROWS 256
int qea_bn_train_stats_from_partials(const double* partials, int32_t blocks, int64_t M, int32_t C, const float* gamma,
                                     const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                     float* mean_out, float* invstd_out, float* scale_out, float* shift_out, double* stat64,
                                     void* stream);
int qea_bn_eval_coeff(int32_t C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, const float* conv_bias, float* mean_out,
                      float* invstd_out, float* scale_out, float* shift_out, void* stream);
/* absmax_out (ABI v6; here and in qea_bn_bwd / qea_maxpool_fwd / qea_maxpool_bwd; NULL = off): a zero-filled float slot into which the
 * kernel folds max |v| of the finite values it stores (atomicMax on the bits) — the scale source of the two-way fp16 split for the
 * conv / wgrad launch that consumes the tensor (qea_conv_desc.x_absmax, qea_wgrad_desc.p_absmax / q_absmax), carried by the
 * producer instead of a qea_absmax pass.  Several launches may share one slot (per-group BatchNorm, the halves of a concat). */
int qea_bn_apply(const float* y, int32_t ldy, float* a, int32_t lda, int64_t M, int32_t C, const float* scale,
                 const float* shift, int32_t relu, float* absmax_out, void* stream);
int qea_bn_bwd(const float* da, int32_t ldda, const float* a, int32_t lda, const float* relu_scale,
               const float* relu_shift, const float* y, int32_t ldy, int64_t M, int32_t C, const float* gamma, const float* mean, const float* invstd, const double* stat64,
               int32_t training, float* dgamma, float* dbeta, int32_t accumulate_param_grads, float* dy,
               int32_t lddy, void* workspace, size_t workspace_bytes, float* absmax_out, void* stream);
/* ABI v8 (additive).  qea_maxpool_bwd(accumulate) + qea_bn_bwd in one: the BatchNorm(+ReLU) backward of a block whose output went to a
 * 2 x kw max-pool (kw in {1, 2}; model_unet.py:52-59 pool1-4, model_crnn.py:53-54 the (2,1) pools) and possibly to a skip connection.
 * da [B*H*W][ldda] = the gradient from the skip path (NULL: none), dpool [B*(H/2)*(W/kw)][lddp] = the gradient of the pooled tensor;
 * the pool's winners and the ReLU mask are recomputed from y with relu_scale / relu_shift (required), so neither the activation nor
 * the summed gradient is read or written.  Same values as the two calls (the fp64 reductions visit the pixels in another order).
 * Workspace: qea_colreduce_workspace_bytes(B*H*W, C). */
int qea_bn_bwd_pool(const float* da, int32_t ldda, const float* dpool, int32_t lddp, int32_t kw, const float* relu_scale,
                    const float* relu_shift, const float* y, int32_t ldy, int32_t B, int32_t H, int32_t W, int32_t C, const float* gamma,
                    const float* mean, const float* invstd, const double* stat64, int32_t training, float* dgamma, float* dbeta,
                    int32_t accumulate_param_grads, float* dy, int32_t lddy, void* workspace, size_t workspace_bytes, float* absmax_out,
                    void* stream);
/* ABI v7 (additive).  qea_bn_bwd with the two per-channel reductions taken from `partials` [blocks (+ 256 scratch rows)][C][2] fp64, as
 * written by the producing input-gradient launch (qea_conv_desc.bst_y), instead of a pass over da and y: finalize + the elementwise
 * pass only.  stat64 and relu_scale / relu_shift are required (what the producer used); workspace: 3 * C doubles.  As its two siblings it
 * needs C % 4 == 0 and C / 4 <= 256 (one float4 column per thread) and answers QEA_ERR_INVALID otherwise, before any launch. */
int qea_bn_bwd_from_partials(const double* partials, int32_t blocks, const float* da, int32_t ldda, const float* relu_scale,
                             const float* relu_shift, const float* y, int32_t ldy, int64_t M, int32_t C, const float* gamma,
                             const float* mean, const float* invstd, const double* stat64, int32_t training, float* dgamma, float* dbeta,
                             int32_t accumulate_param_grads, float* dy, int32_t lddy, void* workspace, size_t workspace_bytes,
                             float* absmax_out, void* stream);
/* out[c] (+)= sum_m x[m][c]  — conv / linear / LSTM bias gradients */
int qea_colsum(const float* x, int32_t ldx, int64_t M, int32_t C, float* out, int32_t accumulate, void* workspace,
               size_t workspace_bytes, void* stream);

/* Max-pool, window == stride (nn.MaxPool2d(2,2) model_unet.py:14-20; fn.max_pool2d (2,2)/(2,1)
 * model_crnn.py:48-54).  First maximum in (kh,kw) scan order wins, as ATen.  bwd recomputes the
 * arg-max from x; relu_mask additionally zeroes the gradient where the maximum is <= 0 (pool of
 * a ReLU output); accumulate: dx += (UNet skip connections). */
int qea_maxpool_fwd(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t B, int32_t H, int32_t W, int32_t C,
                    int32_t kh, int32_t kw, float* absmax_out, void* stream);
/* ABI v7 (additive).  qea_bn_apply followed by qea_maxpool_fwd in ONE pass over y [B,H,W,C]: a = relu?(y*scale + shift) at full
 * resolution (pixel stride lda) and pooled = max-pool(a) (pixel stride ldp), both bit-identical to the two separate calls, which
 * read the activation a second time (model_unet.py:51-59: encoder block -> MaxPool2d(2,2)); absmax_a / absmax_pooled as absmax_out. */
int qea_bn_apply_pool(const float* y, int32_t ldy, float* a, int32_t lda, float* pooled, int32_t ldp, int32_t B, int32_t H, int32_t W,
                      int32_t C, const float* scale, const float* shift, int32_t relu, int32_t kh, int32_t kw, float* absmax_a,
                      float* absmax_pooled, void* stream);
int qea_maxpool_bwd(const float* x, int32_t ldx, const float* dy, int32_t lddy, float* dx, int32_t lddx, int32_t B,
                    int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t relu_mask, int32_t accumulate,
                    float* absmax_out, void* stream);

/* Filter re-layouts for the gradient GEMMs (run once per optimiser step):
 * out[c][r] = in[r][c];  wt[ci][KH-1-kh][KW-1-kw][co] = w[co][kh][kw][ci]. */
int qea_transpose2d(const float* in, float* out, int32_t R, int32_t Cc, void* stream);
int qea_filter_flip_transpose(const float* w, float* wt, int32_t Co, int32_t Ci, int32_t KH, int32_t KW, void* stream);

/* 3x3 pad-1 convolution with ONE input channel (UNet enc1conv1 model_unet.py:13; CRNN conv1
 * model_crnn.py:37,48): x [B,H,W], w [Co][9], y NHWC.  wgrad also yields the bias gradient
 * (db may be NULL); dgrad: dx[B,H,W] (+)= sum_{tap,co} dy * w. */
int qea_conv_c1_fwd(const float* x, const float* w, const float* bias, float* y, int32_t ldy, int32_t B, int32_t H,
                    int32_t W, int32_t Co, int32_t relu, void* stream);
/* ABI v7 (additive).  qea_conv_c1_fwd followed by the 2x2 max-pool in one pass (CRNN conv1 -> ReLU -> max_pool2d(2,2),
 * model_crnn.py:48): y (full resolution: the pool's backward reads it) and pooled [B,H/2,W/2,Co], bit-identical to the two calls.
 * Needs H % 2 == 0, W % 4 == 0, Co in {32, 64, 128}; absmax_pooled as qea_maxpool_fwd's absmax_out. */
int qea_conv_c1_fwd_pool(const float* x, const float* w, const float* bias, float* y, int32_t ldy, float* pooled, int32_t ldp, int32_t B,
                         int32_t H, int32_t W, int32_t Co, int32_t relu, float* absmax_pooled, void* stream);
/* ABI v8 (additive).  The whole backward of conv1 -> ReLU -> max_pool2d(2, 2) (models/model_crnn.py:37-38,47-48) from the POOLED tensor's
 * gradient and the 1-channel input: the full-resolution activation is rebuilt from x (nine multiply-adds per element, the forward's own
 * chain, so the pool's winners and the ReLU mask are the forward's bit for bit), neither it nor its gradient is read or written —
 * qea_conv_c1_fwd_pool may therefore be given y = NULL.  dpool [B*(H/2)*(W/2)][lddp] is OVERWRITTEN with its ReLU-masked values;
 * dw [Co][3][3], db [Co] (accumulate as in qea_conv_c1_wgrad; dw NULL: no parameter gradients), dx [B][H][W] (NULL: not wanted).
 * Co = 64.  Same values as qea_maxpool_bwd(relu_mask) + qea_conv_c1_wgrad + qea_conv_c1_dgrad up to the order of the fp32 partial sums. */
size_t qea_conv_c1_pool_bwd_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Co, int32_t need_dx);
int qea_conv_c1_pool_bwd(const float* x, const float* w, const float* bias, float* dpool, int32_t lddp, float* dw, float* db, float* dx,
                         int32_t B, int32_t H, int32_t W, int32_t Co, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
size_t qea_conv_c1_wgrad_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Co);
int qea_conv_c1_wgrad(const float* x, const float* dy, int32_t lddy, float* dw, float* db, int32_t B, int32_t H,
                      int32_t W, int32_t Co, int32_t accumulate, void* workspace, size_t workspace_bytes,
                      void* stream);
int qea_conv_c1_dgrad(const float* dy, int32_t lddy, const float* w, float* dx, int32_t B, int32_t H, int32_t W,
                      int32_t Co, int32_t accumulate, void* stream);

/* UNet head: y[m] = sigmoid(<x[m,:], w> + b)  (nn.Conv2d 1x1 + torch.sigmoid, model_unet.py:45,76)
 * bwd: dz = dyy*y*(1-y); dx = dz*w; dw (+)= sum dz*x; db (+)= sum dz. */
int qea_head_fwd(const float* x, int32_t ldx, const float* w, const float* b, float* y, int64_t M, int32_t C,
                 void* stream);
size_t qea_head_bwd_workspace_bytes(int64_t M, int32_t C);
int qea_head_bwd(const float* x, int32_t ldx, const float* y, const float* dyy, const float* w, float* dx,
                 int32_t lddx, float* dw, float* db, int32_t accumulate, int64_t M, int32_t C, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * One bidirectional LSTM layer, hidden 256 (nn.LSTM(512,256,2,bidirectional=True),
 * models/model_crnn.py:9,19; gate order i,f,g,o; zero initial state).
 * Buffers (seq-first, both directions side by side):
 *   gates [T][B][2][4][256]  in: x*W_ih^T + b_ih + b_hh (from qea_conv_igemm), out: activations
 *   c     [T][B][2][256], y [T][B][2][256] (= the layer output)
 * qea_lstm_pack_whh re-orders one direction's W_hh [1024][256] into per-lane MFMA fragment
 * order for the forward (h*W_hh^T) and backward (dgates*W_hh) step GEMMs; the two directions'
 * packed copies must be contiguous ([2][1024*256]).
 * qea_lstm_layer_bwd turns `gates` in place into pre-activation gate gradients given dy;
 * dX, dW_ih, dW_hh, db then follow from qea_conv_igemm / qea_conv_wgrad / qea_colsum.
 * ---------------------------------------------------------------------------------- */
int qea_lstm_pack_whh(const float* w_hh, float* packed_fwd, float* packed_bwd, void* stream);
int qea_lstm_layer_fwd(float* gates, float* c, float* y, const float* packed_fwd, int32_t T, int32_t B, void* stream);
int qea_lstm_layer_bwd(float* gates, const float* c, const float* dy, const float* packed_bwd, float* dc_scratch,
                       int32_t T, int32_t B, void* stream);
/* ABI v5: the same layer with the recurrent GEMMs in split-bf16 form (three bf16 planes per fp32 value, six
 * v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate: the arithmetic of the split convolution kernels).
 * qea_lstm_pack_whh_split writes one direction's W_hh as pre-split planes in MFMA-fragment order
 * (qea_lstm_pack_whh_split_bytes() bytes for each of the forward and backward forms; the two directions' copies
 * contiguous, as above); h_prev / dgates rows are split on the fly.  The forward step of batches of >= 1 536 rows runs
 * 128-row workgroups whose weight fragments pass through LDS once per workgroup (LDS-DMA); everything else the 32-row
 * shape of the fp32 step. */
size_t qea_lstm_pack_whh_split_bytes(void);
int qea_lstm_pack_whh_split(const float* w_hh, void* planes_fwd, void* planes_bwd, void* stream);
int qea_lstm_layer_fwd_split(float* gates, float* c, float* y, const void* planes_fwd, int32_t T, int32_t B, void* stream);
int qea_lstm_layer_bwd_split(float* gates, const float* c, const float* dy, const void* planes_bwd, float* dc_scratch,
                             int32_t T, int32_t B, void* stream);

/* ABI v9: the same layer in ONE launch per pass (csrc/lstm_seq.hip): the time loop runs inside the kernel, a workgroup keeps its
 * W_hh slice in LDS for all T steps as two fp16 planes (qea_lstm_seq_pack: qea_lstm_seq_pack_bytes() bytes per direction and form,
 * the two directions' copies contiguous; w_absmax: a device float >= the direction's largest |W_hh|, e.g. qea_absmax's — the scale
 * source of the planes; the layer calls take the two directions' values as [2] floats), c / dc stay in registers, and the eight workgroups of a (row block, direction) exchange h[t] (forward) or the gate
 * gradients (backward) through global memory with write-through stores, one arrival counter per group and sc1 loads — no
 * grid-wide barrier, no residency requirement beyond the group's own eight workgroups, every spin bounded (on a timeout the outputs
 * are NaN).  Three v_mfma_f32_32x32x16_f16 per product (|h| < 1 and W_hh by its abs-max; the gate gradients by a per-row,
 * per-64-column-chunk scale taken in the kernel).  workspace: qea_lstm_seq_workspace_bytes(B) bytes, zeroed by the call itself.
 * Buffers and results as qea_lstm_layer_fwd / _bwd (no dc_scratch).  y_absmax / dgates_absmax: NULL, or a ZEROED device float that
 * receives the largest finite |y| / |gate gradient| of the pass (the scale source of the GEMMs that read the tensor next: no separate
 * abs-max pass over it). */
size_t qea_lstm_seq_pack_bytes(void);
size_t qea_lstm_seq_workspace_bytes(int32_t B);
int qea_lstm_seq_pack(const float* w_hh, void* planes_fwd, void* planes_bwd, const float* w_absmax, void* stream);
int qea_lstm_seq_fwd(float* gates, float* c, float* y, const void* planes_fwd, const float* w_absmax, int32_t T, int32_t B,
                     void* workspace, float* y_absmax, void* stream);
int qea_lstm_seq_bwd(float* gates, const float* c, const float* dy, const void* planes_bwd, const float* w_absmax, int32_t T,
                     int32_t B, void* workspace, float* dgates_absmax, void* stream);
/* ABI v9 (additive).  The index of the uint32 word of `workspace` that a pass at B rows sets to 1 when one of its bounded spins ran
 * out (backward != 0: qea_lstm_seq_bwd, else qea_lstm_seq_fwd; -1 for B <= 0).  The word lies in front of the exchange area, is
 * zeroed by the pass itself and is valid once the pass has finished on its stream; the query dereferences nothing. */
int qea_lstm_seq_timeout_index(int32_t B, int32_t backward);

/* ABI v9 (additive).  Several derived weight forms in ONE launch (a model has ~110 of them per optimiser step, a few microseconds each):
 * kind 0 = qea_filter_flip_transpose (a, b, c, d = Co, Ci, KH, KW; amax unused), kind 1 = qea_pack_frag_planes_f16 (a, b = N, Cin),
 * kind 2 = qea_pack_frag_planes_f16_1x1 (a, b = N, K); same bytes as the single calls.  `jobs` is a HOST array of 1..64 jobs; a job
 * must not read what another job of the same call writes (flip first, then pack the flipped filters in a second call). */
typedef struct qea_wform_job {
  const float* src;
  void* dst;
  const float* amax;
  int32_t kind, a, b, c, d;
} qea_wform_job;
int qea_weight_forms_multi(const qea_wform_job* jobs, int32_t n, void* stream);

/* log_softmax over the last dim (fn.log_softmax(.., 2), model_crnn.py:20) and its backward
 * dx = g - exp(lp)*sum(g), with the reference's NaN scrub (CRNN.backward_hook,
 * model_crnn.py:30-32, registered at train_nn_patch.py:94) when nan_scrub != 0; columns
 * [C, Cpad) of dx are zeroed. */
int qea_log_softmax_fwd(const float* x, int32_t ldx, float* y, int32_t ldy, int64_t M, int32_t C, void* stream);
int qea_log_softmax_bwd(const float* g, int32_t ldg, const float* lp, int32_t ldlp, float* dx, int32_t lddx, int64_t M,
                        int32_t C, int32_t Cpad, int32_t nan_scrub, void* stream);

/* CTC loss (torch.nn.CTCLoss, blank 0, zero_infinity=False; train_nn_patch.py:143,178,294,
 * train_nn_area.py:146-147,265).  lp element (t,n,c) at t*ld_t + n*ld_n + c.  targets:
 * concatenated int32 (device), target_offsets[n] = start of sample n.  reduction 1 = 'mean'
 * (mean_n nll_n/max(len_n,1)), 0 = 'none' (loss = sum, nll[] per sample).  grad (may be NULL)
 * = d(reduced loss * grad_scale)/d lp exactly as ATen forms it (NaN for infeasible samples).
 * S_max >= 2*max(target_len)+1, <= 256. */
size_t qea_ctc_workspace_bytes(int32_t T, int32_t N, int32_t S_max);
int qea_ctc_loss(const float* lp, int32_t ld_t, int32_t ld_n, const int32_t* targets, const int64_t* target_offsets,
                 const int32_t* input_lengths, const int32_t* target_lengths, int32_t T, int32_t N, int32_t C,
                 int32_t blank, int32_t S_max, int32_t reduction, float grad_scale, float* nll, float* loss,
                 float* grad, int32_t gld_t, int32_t gld_n, void* workspace, size_t workspace_bytes, void* stream);

/* torch.optim.Adam step over one flat fp32 buffer (train_nn_patch.py:146-152,308-309,343-345):
 * g' = g*grad_scale + wd*p; m,v update; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps). */
int qea_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, float grad_scale, void* stream);
/* The same update with the step count held on the device (torch.optim.Adam(capturable=True)): step[0] (a float,
 * as torch keeps it) is incremented by a one-thread kernel which also writes the two bias-correction
 * coefficients to coef[0..1]; no launch argument depends on the step count, so the pair of launches can be
 * recorded into a hipGraph and replayed. */
int qea_adam_step_capturable(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, float* step, float* coef, float grad_scale,
                             void* stream);

/* AddGaussianNoice (transform_helper.py:33-45) for R replicas of K images fused into the batch
 * dim: out[r*K+k] = clamp(img[k] - coef*sigma[r*K+k]*N(0,1), 0, 1); Philox4x32-10 keyed by
 * (seed, offset); noise_out (optional) receives sigma*N(0,1).  qea_jitter_apply takes the
 * noise as an input instead (parity tests; train_nn_area.py:184-191 returns the noise). */
int qea_jitter(const float* img, const float* sigma, float* out, float* noise_out, int32_t K, int32_t R, int32_t HW,
               float coef, uint64_t seed, uint64_t offset, void* stream);
int qea_jitter_apply(const float* img, const float* noise, float* out, int32_t K, int32_t R, int32_t HW, float coef,
                     void* stream);

/* TopKCERSampler.query ranking (selection_utils.py:144-151): indices of the k largest keys,
 * descending, equal keys in ascending index order (stable); n <= 16384. */
int qea_topk_desc_stable(const float* keys, int32_t n, int32_t k, int64_t* idx_out, void* stream);

/* utils.get_text_stack / padder (utils.py:118-141): crop boxes (x0,y0,x1,y1, already clipped to
 * the image) out of a [H][W] image, centre on a white OH x OW canvas; scatter is its backward
 * (adds into dimg). */
int qea_crop_pad_gather(const float* img, int32_t H, int32_t W, const int32_t* boxes, int32_t N, int32_t OH, int32_t OW,
                        float* out, void* stream);
int qea_crop_pad_scatter(const float* dout, const int32_t* boxes, int32_t N, int32_t OH, int32_t OW, float* dimg,
                         int32_t H, int32_t W, void* stream);

/* utils.pred_to_string (utils.py:74-92): per-step argmax (torch.argmax's rule: the first NaN if the row
 * has one, else the first maximum), collapse repeats, drop blank -> tokens [N][T] int32 + lengths [N];
 * scores element (t,n,c) at t*ld_t + n*ld_n + c. */
int qea_greedy_decode(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank,
                      int32_t* tokens, int32_t* lengths, void* stream);

/* CTC prefix beam search: stands beside utils.pred_to_string (utils.py:74-92), which decodes greedily; the reference has no beam.
 * Per sample the K most probable LABELLINGS (the alignments that spell the same text added up), best first, with their
 * log-probabilities.  Specified in fp64 with a fixed candidate order (DESIGN.md "CTC prefix beam search"): scores element (t,n,c) at
 * t*ld_t + n*ld_n + c is converted to fp64 exactly, a NaN counts as -inf, lse(a,b) = max(a,b) + log1p(exp(-|a-b|)); the candidates
 * of a step are walked by (beam rank, slot) with slot 0 = the prefix itself and slot s >= 1 = the prefix plus the s-th non-blank class;
 * an extension that is itself a beam entry is folded into that entry's slot 0; candidates of score -inf are dropped; the next beam is
 * the K best, equal scores in candidate order (a stable sort).
 *   tokens [N][K][T] int32: the prefix of rank k, then -1 up to T;  lengths [N][K]: its length, -1 for the ranks beyond the live
 *   count;  beam_scores [N][K] fp64: its log-probability, -inf for those ranks.
 * One workgroup per sample, one launch, no workspace, no atomics; every output element is written once.
 * Refused before any launch: K outside 1..32, C outside 2..256, T outside 1..512, blank outside 0..C-1, N < 1, NULL pointers.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects it by symbol.) */
int qea_ctc_beam_decode(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                        int32_t* tokens, int32_t* lengths, double* beam_scores, void* stream);

/* The same search with a character n-gram prior fused in (DESIGN.md "Character n-gram fusion"); everything above stands, plus:
 *   lm_context m = 0, 1, 2 (unigram, bigram, trigram).  The context of a prefix is its last m tokens, padded on the left with BOS, which
 *   is represented by the blank index; ctx(p) = sum_q tok_q * C^(m-1-q), ctx(p + c) = (ctx(p) * C + c) mod C^m, ctx = 0 for m = 0.
 *   lm_table [C^m][C] fp64, already alpha * log P(c | ctx) + beta; a NaN entry counts as -inf; column `blank` is never read.  The device
 *   only ever ADDS table entries.  A beam entry also carries lm (0 at the start) and ctx.  Slot 0 of entry i keeps lm_i and ctx_i and
 *   ranks by lse(pb', pnb') + lm_i; slot c has lm' = lm_i + lm_table[ctx_i][c] and ranks by pnb' + lm' (first lm', then the sum), pnb'
 *   the plain search's term.  A ranking score that is not greater than -inf is dropped; the next beam is the K best by RANKING score,
 *   equal scores in candidate order.  pb / pnb stay pure CTC quantities; folding is unchanged (the same prefix has the same lm, ctx).
 *   ctc_scores [N][K]: lse(pb, pnb) of rank k;  total_scores [N][K]: ctc + lm, what the order was decided by;  both -inf (and length
 *   -1) beyond the live count.  With an all-zero table tokens, lengths and ctc_scores are qea_ctc_beam_decode's, and total == ctc.
 * Refused before any launch: what qea_ctc_beam_decode refuses, lm_context outside 0..2, C^(lm_context + 1) > 2^21 table entries
 * (16 MB: a trigram up to C = 128, a bigram up to C = 256), NULL lm_table / total_scores.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects it by symbol.) */
int qea_ctc_beam_decode_lm(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                           const double* lm_table, int32_t lm_context, int32_t* tokens, int32_t* lengths, double* ctc_scores,
                           double* total_scores, void* stream);

/* The plain search restricted to the paths of a deterministic automaton over the non-blank classes (DESIGN.md "Automaton-constrained
 * search"; a word-list trie is the usual one: qea/lexicon.py); everything said for qea_ctc_beam_decode stands, plus:
 *   S >= 1 states, state 0 the start, E edges in CSR form: first [S+1] int32 (first[0] = 0, non-decreasing, first[S] = E), the edges of
 *   state s are first[s] .. first[s+1]-1; label [E] int32, the class of each edge, strictly ascending within a state, never the blank;
 *   child [E] int32, the target state.  Which states accept is the host's business: the device never sees it.
 *   A beam entry also carries a state, 0 for the empty prefix.  Slot c of entry i exists only when state(i) has an edge labelled c (a
 *   slot that does not exist scores -inf, exactly like a folded one); the new entry carries that edge's child; slot 0 keeps its state.
 *   Folding, pb / pnb / tot, the candidate order and the stable selection are unchanged, and the scores stay pure CTC quantities: a
 *   returned score is the CTC log-likelihood of that labelling.
 *   states [N][K] int32: the state of rank k, -1 beyond the live count.  The whole last beam is returned, accepted or not.
 *   Tables that break the statements above cannot make the kernel read outside the four arrays: an edge whose label is the blank or
 *   outside 0..C-1, or whose child is outside 0..S-1, is absent, and the values of `first` are clamped to 0..E.
 *   With the one-state automaton that loops on every class, tokens, lengths and beam_scores are qea_ctc_beam_decode's bit for bit.
 * Refused before any launch: what qea_ctc_beam_decode refuses, S < 1, E outside 0..2^26-1 (the edges of up to 32 live states are
 * counted in an int32), NULL first / label / child / states.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects it by symbol.) */
int qea_ctc_beam_decode_dfa(const float* scores, int32_t ld_t, int32_t ld_n, int32_t T, int32_t N, int32_t C, int32_t blank, int32_t K,
                            const int32_t* first, const int32_t* label, const int32_t* child, int32_t S, int32_t E, int32_t* tokens,
                            int32_t* lengths, double* beam_scores, int32_t* states, void* stream);

/* Unit-cost edit distance between the greedy decode of each sample (pred_tokens [N][ldp], pred_len)
 * and its ground-truth token string (concatenated gt_tokens, gt_offsets, gt_len): the numerator of
 * utils.compare_labels' CER (utils.py:95-110, python-Levenshtein `distance`); the host divides by
 * max(1, len(gt)) in float64 as the reference does.  ldp <= 128. */
int qea_edit_distance(const int32_t* pred_tokens, int32_t ldp, const int32_t* pred_len, const int32_t* gt_tokens,
                      const int64_t* gt_offsets, const int32_t* gt_len, int32_t N, int32_t* out, void* stream);

/* Dataset pruning: greedy facility-location selection (pruning/methods.py:12-23, apricot's FacilityLocationSelection with
 * optimizer='naive' on squared-euclidean similarities) over n feature rows x[n][d] of fp64, 1 <= d <= 32, 1 <= k <= n:
 *   S[i][j] = M - sum_dd (x[i][dd] - x[j][dd])^2 (terms added in ascending dd), M = the largest squared distance of any pair;
 *   cur[j] = 0; pick t takes the unpicked i with the largest gain[i] = sum_j max(S[i][j], cur[j]) (the LOWEST index on an exact
 *   tie), then cur[j] = max(cur[j], S[i][j]).
 * ranking_out[t] receives the index and gain_out[t] (may be NULL) the gain of pick t.  S is recomputed from x for every pick (no
 * n x n buffer); the sum over j has one fixed order for every i, so rows with identical features tie exactly; the k picks (two
 * launches each) and the computation of M are enqueued on `stream` without a host synchronisation.  `workspace`: 16-byte aligned,
 * qea_facility_workspace_bytes(n, d) bytes (0 for sizes the call refuses), zeroed by the call itself.  Refused before any launch:
 * NULL x / ranking_out / workspace, d outside 1..32, k outside 1..n.  Non-finite features (or squared distances that overflow) are
 * found on the device: the picks then do nothing and ranking_out / gain_out stay unwritten; qea_facility_status — the ONE entry
 * point here that synchronises `stream`, meant to follow the caller's own read-back of the ranking — reads the workspace's flag
 * word and returns QEA_ERR_INVALID with the message.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these three by symbol.) */
size_t qea_facility_workspace_bytes(int32_t n, int32_t d);
int qea_facility_select(const double* x, int32_t n, int32_t d, int32_t k, int32_t* ranking_out, double* gain_out, void* workspace,
                        void* stream);
int qea_facility_status(const void* workspace, void* stream);

/* Label-history loss weights (--inner_limit_skip with --window_size > 1), the whole [n][W+1] table of one minibatch in ONE launch.
 * Both calls write every element of `out` (fp32 [n][W+1]): column 0 is 1, columns 1..count[r] are the weights of strip r's
 * remembered labels, most recent first, the rest are 0.  count[r] (clamped to 0..W) = remembered labels inside the window, 0 for
 * a strip without history.  W <= QEA_HISTORY_MAX_WINDOW.  Nothing synchronises.
 *
 * qea_history_lev_weights — LevenshteinWeightGenerator.gen_weights (label_tracking/tracking_methods.py:63-101):
 *   tokens [n][W][QEA_HISTORY_MAX_LEN] int32 Unicode code points (raw characters, no char_to_index), lens [n][W] (a length
 *   outside 0..QEA_HISTORY_MAX_LEN is clamped, so nothing is read out of bounds: the caller routes longer words elsewhere);
 *   out[r][i+1] = 0.5 * (1 - min(mean_i, c_i) / c_i), mean_i = (integer sum of the unit-cost edit distances of word i to the
 *   other count-1 words) / max(count-1, 1), c_i = max(1, len_i), evaluated in fp64 and rounded once to fp32: bit-identical to the
 *   reference's Python floats stored into a float32 tensor.  Each of the W(W-1)/2 distances is computed once.
 *
 * qea_history_attn_weights — AttentionWeightGenerator.gen_weights (label_tracking/tracking_methods.py:26-59) through
 *   HistoryAttention.forward (models/model_attention.py:7-38), fp32:
 *   char_idx [n][W][n_chars] int32 indices into `embedding` [V1][E] as tracking_utils.str_to_tensor builds them (pad index V1-1 for
 *   missing characters and missing words; an index outside 0..V1-1 is read as V1-1); words = mean over the n_chars rows (always
 *   / n_chars) + positional_encodings [W][E]; q = words Wq^T + wq_bias (wq_weight [Dq][E]); a = softmax_rows(q q^T / sqrt(Dq));
 *   z = a coef_weight^T + coef_bias (coef_weight [W], coef_bias [1]); activation 0: sigmoid(z), 1: softmax of z over the W window
 *   rows, 2: relu(z) / (sum relu(z) + 1e-6).  Strips with count 0 get [1, 0, ...] without evaluating the scorer.
 *   (V1 + W) * Dq <= QEA_HISTORY_ATTN_MAX_TABLE, E a multiple of 4, all float pointers 16-byte aligned.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these two by symbol.) */
#define QEA_HISTORY_MAX_WINDOW 8
#define QEA_HISTORY_MAX_LEN 128
#define QEA_HISTORY_ATTN_MAX_TABLE 12288
#define QEA_HISTORY_ACT_SIGMOID 0
#define QEA_HISTORY_ACT_SOFTMAX 1
#define QEA_HISTORY_ACT_RELU 2
int qea_history_lev_weights(const int32_t* tokens, const int32_t* lens, const int32_t* count, int32_t n, int32_t W, float* out,
                            void* stream);
int qea_history_attn_weights(const int32_t* char_idx, const int32_t* count, int32_t n, int32_t W, int32_t n_chars,
                             const float* embedding, int32_t V1, int32_t E, const float* wq_weight, const float* wq_bias, int32_t Dq,
                             const float* coef_weight, const float* coef_bias, const float* positional_encodings, int32_t activation,
                             float* out, void* stream);

/* Label-history weighted CTC loss (tracking_utils.py:59-75: weighted_ctc_loss) of one minibatch in one device pass: every strip n
 * carries up to W problems, one per history depth i, that share the log-prob rows lp[:, n, :] (element (t,n,c) at
 * t*ld_t + n*ld_n + c, as qea_ctc_loss).  input_lengths [N]; lens [N][W] int32, -1 = strip n has no label at depth i, 0 = a real,
 * empty label; offs [N][W] int32 = start of that label in the concatenated int32 `chars`; depth_n [W] = strips present at depth i.
 * weights element (n,i) at n*w_stride_n + i*w_stride_i (fp32): the sample-wise [N][W+1] table has strides (W+1, 1), the decaying
 * [W] vector (0, 1).  With
 *   coef[n,i] = w[n,i] / depth_n[i]                       mean_by_length = 0   (:69-73, mean(w * CTCLoss(reduction="none")) per depth)
 *   coef[n,i] = w[n,i] / (depth_n[i] * max(len,1))        mean_by_length = 1   (:66-67, w[i] * CTCLoss() per depth)
 * loss[0] = sum_{n,i present} coef * nll[n,i];  grad (may be NULL; element (t,n,c) at t*gld_t + n*gld_n + c)
 *   = sum_i coef[n,i] * (exp(lp) - exp(lse_{s: l'_s = c}(alpha+beta) + nll - lp)), rows t >= input_length and strips without any
 * label are zero; nll [N][W] fp32, 0 where absent.  Recursion, nll, coef and the sums over depths (ascending i) run in fp64, each
 * output element is written once by one thread and rounded once: bit-reproducible, no atomics.  An infeasible target gives
 * nll = +inf, a non-finite loss and NaN rows t < input_length of THAT strip only (as qea_ctc_loss does).
 * At most three launches whatever W and the histories (two when grad is NULL); nothing synchronises and nothing is copied, so the
 * call can be captured in a hipGraph.  W <= QEA_HISTORY_MAX_WINDOW, S_max >= 2*max(len)+1, <= 256, T <= 65535.  workspace:
 * qea_ctc_history_workspace_bytes(T, N, W, S_max) = (2*T*S_max + 2) * N*W * 8 bytes (alpha, beta, nll, coef in fp64), 8-byte aligned.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these two by symbol.) */
size_t qea_ctc_history_workspace_bytes(int32_t T, int32_t N, int32_t W, int32_t S_max);
int qea_ctc_history_loss(const float* lp, int32_t ld_t, int32_t ld_n, const int32_t* input_lengths, const int32_t* lens,
                         const int32_t* offs, const int32_t* chars, const int32_t* depth_n, const float* weights,
                         int32_t w_stride_n, int32_t w_stride_i, int32_t mean_by_length, int32_t T, int32_t N, int32_t C, int32_t W,
                         int32_t blank, int32_t S_max, float* loss, float* grad, int32_t gld_t, int32_t gld_n, float* nll,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Minibatch assembly from a device-resident strip store (datasets/resident.py: ResidentStrips; --resident of area_cli.py and
 * train_crnn.py).  The store holds the n strips of a dataset as 8-bit grey after the loader's own PIL decode (and thumbnail of
 * oversize strips): strip s is h[s] rows of w[s] bytes, row-major without padding, at pixels + offset[s].  ONE launch writes the
 * whole batch out[B][OH][OW] (fp32, 16-byte aligned): strip idx[b] on a white (1.0) ground,
 *   QEA_STRIP_ANCHOR_CENTRE  left = (OW - w) / 2, top = (OH - h) / 2 (rounded down): transform_helper.PadWhite followed by the
 *                            loader's float32(p) / 255
 *   QEA_STRIP_ANCHOR_LEFT    left = 0, top as above: datasets/bucketing.pad_to_bucket
 * and every strip byte p replaced by table[p].  `table` is 256 fp32 values on the device, built by the HOST as float32(p) / 255, so
 * the batch equals the loader's bit for bit whatever the device compiler makes of a division.  Every element of `out` is written
 * exactly once (no prior fill); one 16-byte store per lane, hence OW % 4 == 0.  A strip taller than OH or wider than OW is clipped
 * to its first OH rows / OW columns; an idx[b] outside 0..n-1 gives an all-white image (the Python caller validates idx on the host
 * first).  No workspace, no LDS, nothing synchronises.  Refused before the launch: a NULL pointer, n < 1, B outside 1..2^24, OH
 * outside 1..4096, OW outside 4..16384 or not a multiple of 4, an unknown anchor, a misaligned `out`.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects the entry point by symbol.) */
#define QEA_STRIP_ANCHOR_CENTRE 0
#define QEA_STRIP_ANCHOR_LEFT 1
int qea_strip_batch(const uint8_t* pixels, const int64_t* offset, const int32_t* h, const int32_t* w, int32_t n, const int64_t* idx,
                    int32_t B, int32_t OH, int32_t OW, int32_t anchor, const float* table, float* out, void* stream);

/* All text strips of a step cut out of its documents in ONE launch, and their gradient put back in ONE launch (csrc/doc_crops.hip;
 * datasets/resident.py: ResidentDocuments.crops; --resident of patch_cli.py).  The reference cuts them one document at a time
 * (utils.py:118-141 over the samples of datasets/patch_dataset.py:14-129).
 *   box [n_boxes][4] int32 = (x0, y0, x1, y1) of every word box of the store, clipped to the canvas; the boxes of document d are rows
 *   box_first[d] .. box_first[d+1]-1 (box_first int32 [n_docs+1]).  A step holds N images [N][H][W] fp32, image n being document
 *   doc[n] (int64 [N]); its S strips are all boxes of its documents, in document order and then box order:
 *   strip_first int32 [N+1] = prefix sums of the chosen documents' box counts, strip_first[N] = S.
 * qea_doc_crops_gather — out[S][OH][OW]: for every strip bit for bit what qea_crop_pad_gather gives for that image and box (the crop
 *   centred on white 1.0; a crop larger than the target loses its extra pixel on the left / top).  Every element is written, one
 *   16-byte store per lane: OW % 4 == 0, `out` 16-byte aligned.  A strip whose document or box does not exist is all white.
 * qea_doc_crops_scatter — the backward, in gather form and WITHOUT atomics: dimg[n][y][x] = the sum over the boxes of document doc[n]
 *   that cover (x, y), in ASCENDING box order starting from 0, of the dout element that read it; 0 where no box does.  accumulate = 1
 *   adds that sum to what dimg holds.  Every element of dimg is written exactly once (no prior fill), one 16-byte store per lane:
 *   W % 4 == 0, `dimg` 16-byte aligned.  The result is fixed by the inputs; for boxes that do not overlap it equals a zero fill
 *   followed by qea_crop_pad_scatter per document, bit for bit.  6 KB of LDS (the boxes culled against a workgroup's 16 x 64 tile).
 * Nothing synchronises, no workspace.  Refused before the launch: a NULL pointer, n_docs or n_boxes < 1, N outside 1..2^16, H outside
 * 1..8192, W or OW outside 4..8192 or not a multiple of 4, S outside 1..2^24, OH outside 1..4096, a misaligned out / dimg.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these two by symbol.) */
int qea_doc_crops_gather(const float* imgs, int32_t N, int32_t H, int32_t W, const int32_t* box, const int32_t* box_first, int32_t n_docs,
                         int32_t n_boxes, const int64_t* doc, const int32_t* strip_first, int32_t S, int32_t OH, int32_t OW, float* out,
                         void* stream);
int qea_doc_crops_scatter(const float* dout, int32_t S, int32_t OH, int32_t OW, const int32_t* box, const int32_t* box_first,
                          int32_t n_docs, int32_t n_boxes, const int64_t* doc, const int32_t* strip_first, float* dimg, int32_t N, int32_t H,
                          int32_t W, int32_t accumulate, void* stream);

/* The two minibatch samplers that pick on per-strip estimates (--minibatch_subset rangeCER / uniformEntropy).
 *
 * qea_spread_pick — the range sampling of CerRangeSampler.query (selection_utils.py:129-134) and sampleUsingEstimates
 *   (selection_utils.py:52-57), the k serial picks in ONE launch of one workgroup, bit-identical to the host loop for finite inputs:
 *   left = a private fp32 copy of est[0..n) (est is not written); for i = 0..k-1: j = the LOWEST index that minimises
 *   fabsf(pts[i] - left[j]) (one fp32 subtraction, then the absolute value: no fma, no wider type; torch.argmin's first-index
 *   rule), idx[i] = j (int64), left[j] = 100.0f.  The reference's sentinel is kept as it is: with k > n every estimate is 100
 *   after n picks and index 0 repeats; an estimate >= 100 competes with the sentinel on equal terms.  `pts` is built by the host
 *   exactly as before ((max - min) * torch.rand(k) + min in fp32), so the CPU generator is consumed as before.  est and pts must
 *   be finite (the Python caller sends anything else to the host loop); n, k in 1..QEA_SPREAD_MAX_N.  `left` lives in LDS up to
 *   QEA_SPREAD_LDS_MAX_N estimates; above, in `workspace` (16-byte aligned, qea_spread_pick_workspace_bytes(n) bytes — 0 for an
 *   n that needs none, where `workspace` may be NULL).  The form is chosen by n alone: one wave up to QEA_SPREAD_WAVE_MAX_N, four
 *   waves up to QEA_SPREAD_LDS4_MAX_N, sixteen above (thresholds measured: profiles/samplers.json, csrc/sampling.hip).  Nothing synchronises.
 *
 * qea_seq_entropy — update_entropies + calc_entropy (selection_utils.py:10-27) for a whole batch in one launch, one wave per
 *   strip: lp holds log-probs, element (t,b,c) at t*ld_t + b*ld_n + c (any non-negative strides: the CRNN's 96-column rows, a
 *   [:, a:b, :] slice);  out[b] = fp32( mean_t( -sum_c p log(p + 1e-6) ) / log(num_classes) ),  p = exp(lp[t,b,c]), evaluated in
 *   fp64 and rounded once.  lp = -inf contributes 0.  num_classes is the reference's constant 95 whatever C is.  T * C <= 2^30.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these three by symbol.) */
#define QEA_SPREAD_WAVE_MAX_N 1536
#define QEA_SPREAD_LDS4_MAX_N 24576
#define QEA_SPREAD_LDS_MAX_N 32768
#define QEA_SPREAD_MAX_N (1 << 24)
size_t qea_spread_pick_workspace_bytes(int32_t n);
int qea_spread_pick(const float* est, int32_t n, const float* pts, int32_t k, int64_t* idx, void* workspace, void* stream);
int qea_seq_entropy(const float* lp, int64_t ld_t, int64_t ld_n, int32_t T, int32_t B, int32_t C, int32_t num_classes, float* out,
                    void* stream);

/* Whole pages of any size through the eval-mode UNet, tile by tile (csrc/page_tiles.hip; qea/pages.py: clean_pages, whose
 * tiles_gather_spec / tiles_scatter_spec are the specification of these two).  A page store holds n_pages pages back to back, row-major
 * without padding: page p is h[p] rows of w[p] elements at ELEMENT offset[p] of a store of store_elems elements (8-bit grey, so pages start
 * at any byte, or fp32); the outputs of the scatter are packed the same way with the same offsets.  All tiles of one call are TH x TW; they
 * may belong to several pages.
 * qea_page_tiles_gather — out[N][TH][TW] (fp32, 16-byte aligned) in ONE launch.  tile int32 [N][3] = (page, oy, ox): out[t][y][x] is page
 *   pixel (oy + y, ox + x), and white (1.0) where that lies outside the page's h x w (the padding of a page to a multiple of 16 is never
 *   stored).  store_is_f32 = 0: 8-bit pixels, each replaced by table[p] (256 fp32 values on the device, built by the HOST as float32(p) /
 *   255 as for qea_strip_batch); store_is_f32 = 1: fp32 pixels copied as they are, `table` may be NULL.  Every element of `out` is written
 *   exactly once, one 16-byte store per lane: TW % 4 == 0.
 * qea_page_tiles_scatter — tiles[N][TH][TW] (fp32, 16-byte aligned) pasted into the packed outputs in ONE launch.  tile int32 [N][7] =
 *   (page, oy, ox, cy0, cy1, cx0, cx1): the tile owns the page pixels of its core [cy0, cy1) x [cx0, cx1) (page coordinates) that lie inside
 *   the tile and inside the page's h x w; each is stored to out_f32 (as it is) and / or to out_u8 as
 *   (uint8)(min(max(x, 0), 1) * 255.0f) — ONE fp32 multiply and no fused add, then truncation: (x.clamp(0, 1) * 255).to(torch.uint8) bit for
 *   bit, what ToPILImage makes of a float tensor.  NaN gives 0.  Either output may be NULL, not both.  With cores that partition every
 *   page (qea/pages.py: plan_tiles) each output element is written exactly once: no atomics, no prior fill; what no core covers is left
 *   as it was.
 * A row of either table whose page does not exist or does not lie inside the store (offset[p] < 0 or offset[p] + h[p] * w[p] > store_elems)
 * gives a white tile / writes nothing.  Nothing synchronises, no workspace, no LDS.  Refused before the launch: a NULL pointer, n_pages or N
 * outside 1..2^24, store_elems < 1, TH outside 1..8192, TW outside 4..8192 or not a multiple of 4, a flag that is neither 0 nor 1, an 8-bit
 * store without a table, a misaligned out / tiles / fp32 pointer.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these two by symbol.) */
int qea_page_tiles_gather(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                          const int32_t* w, int32_t n_pages, const int32_t* tile, int32_t N, int32_t TH, int32_t TW, const float* table,
                          float* out, void* stream);
int qea_page_tiles_scatter(const float* tiles, int32_t N, int32_t TH, int32_t TW, const int32_t* tile, const int64_t* offset,
                           const int32_t* h, const int32_t* w, int32_t n_pages, int64_t store_elems, float* out_f32, uint8_t* out_u8,
                           void* stream);

/* Classic binarisation baselines over the same page store (csrc/binarize.hip; qea/binarize.py: binarize_pages; the statement, which all
 * three reproduce bit for bit, is tests/binarize_spec.py and DESIGN.md "Binarisation baselines").  store / store_elems / offset / h / w /
 * n_pages are those of qea_page_tiles_*; an fp32 pixel is read as its 8-bit value (uint8)(min(max(x, 0), 1) * 255.0f), NaN as 0.  Ink is
 * foreground: a foreground pixel is written as 0 / 0.0f, a background pixel as 255 / 1.0f, to out_u8 and / or out_f32 (either may be NULL,
 * not both), which are packed like the store with the same offsets; what lies between the pages is never written.  host_h / host_w are
 * the caller's HOST copies of h / w: the entry point validates the page sizes and sizes its grid from them, the kernels read the device
 * tables.  The block-to-page map is a prefix table on the device, int32 [n_pages + 1] with first[0] = 0, uploaded with the page table:
 *   tile_first[p + 1] - tile_first[p]   = ceil(h[p] / QEA_BINARIZE_TILE_H) * ceil(w[p] / QEA_BINARIZE_TILE_W)   (Sauvola)
 *   chunk_first[p + 1] - chunk_first[p] = ceil(h[p] * w[p] / QEA_BINARIZE_CHUNK)                                 (Otsu)
 * Device tables that disagree with the host copies leave pixels unwritten; they never cause an access outside the buffers.
 * qea_binarize_sauvola — ONE launch for all pages.  Per pixel v, over the win x win window centred on it and clipped to the page (n pixels,
 *   S1 = sum v, S2 = sum v^2, Q = n S2 - S1^2, all exact integers): A = double(n v) - double(S1) * (1.0 - k); foreground iff A <= 0 or
 *   L * L <= (G * G) * double(Q) with L = A * (R * double(n)), G = k * double(S1): the textbook v <= m (1 + k (s / R - 1)) without sqrt or
 *   division, every fp64 operation rounded as written.  win is odd in 3..QEA_BINARIZE_MAX_WINDOW, 0 < k < 1, R > 0 and finite.  LDS:
 *   33.5 KiB at win = 25, 110.5 KiB at win = 127 (the largest is reserved once per process).
 * qea_otsu_histogram — launch 1 of Otsu: zeroes hist (uint32 [n_pages][256], hipMemsetAsync on the stream) and counts every page's pixels
 *   into its row with integer atomics (deterministic).
 * qea_binarize_otsu — launch 2: every workgroup derives its page's t* from the 256 bins (N = sum hist, S = sum v hist[v]; for t = 0..254
 *   ascending with w0 = sum hist[..t] > 0 and w1 = N - w0 > 0: d = s0 N - S w0 in int64, num = double(d)^2, den = double(w0) double(w1); t
 *   replaces the best iff num * den_best > num_best * den, so ties keep the smaller t) and writes foreground iff v <= t*.  thresholds
 *   (int32 [n_pages]) receives t*, or -1 for a page of a single grey level, which is all background.
 * Nothing synchronises, no workspace.  Refused before any launch: a NULL pointer, a flag that is neither 0 nor 1, n_pages outside 1..2^24,
 * store_elems < 1, an empty page, a page of more than QEA_BINARIZE_MAX_PAGE_PIXELS pixels (the bound that keeps 255 N^2 < 2^63), more
 * than 2^31 - 1 workgroups, win even or outside its range, k or R outside their ranges or not finite, both outputs NULL, a misaligned
 * fp32 store / out_f32 / hist / thresholds.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these three by symbol.) */
#define QEA_BINARIZE_TILE_H 32
#define QEA_BINARIZE_TILE_W 64
#define QEA_BINARIZE_CHUNK 32768
#define QEA_BINARIZE_MAX_WINDOW 127
#define QEA_BINARIZE_MAX_PAGE_PIXELS (1 << 27)
int qea_binarize_sauvola(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                         const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                         int32_t win, double k, double R, float* out_f32, uint8_t* out_u8, void* stream);
int qea_otsu_histogram(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                       const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* chunk_first,
                       uint32_t* hist, void* stream);
int qea_binarize_otsu(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                      const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* chunk_first,
                      const uint32_t* hist, float* out_f32, uint8_t* out_u8, int32_t* thresholds, void* stream);

/* Connected components over the same page store (csrc/components.hip; qea/components.py: label_pages, page_components, despeckle_pages,
 * word_boxes; the statement, which the device, the host path and tests/components_spec.py reproduce bit for bit, is DESIGN.md "Connected
 * components").  The leading arguments, host_h / host_w and tile_first are those of qea_binarize_sauvola (tiles of QEA_BINARIZE_TILE_H x
 * QEA_BINARIZE_TILE_W).  A pixel is ink iff its 8-bit value is <= ink_max (0..254), or, where a uint8 mask packed like the store is given
 * (ink_mask / in_mask, may be NULL), iff its mask byte is not 0.  labels and area are int32 arrays packed like the store (page p's element
 * i at offset[p] + i); what lies between the pages is never written, by any of the five.
 * qea_cc_label — three launches (tile, border, flatten): labels[i] = the smallest row-major index y * w + x within the page over the pixels
 *   of pixel i's component at connectivity 4 or 8, -1 for background.  The border launch is a lock-free min-index union-find with agent-scope
 *   atomics; no kernel waits for another workgroup, every walk moves to a strictly smaller index.  If area is not NULL its in-page elements
 *   are cleared to 0 by the first launch, which is what qea_cc_stats expects.
 * qea_cc_stats — one launch: ADDS every component's pixel count to area[its root] (one integer atomic per tile and distinct root: exact),
 *   so that after qea_cc_label(..., area) + qea_cc_stats area holds the component's area at its root and 0 at every other in-page element.
 * qea_cc_despeckle — one launch: ink pixels of components with area >= min_area (>= 1) are written as 0 / 0.0f, everything else in the
 *   pages as 255 / 1.0f, to out_u8 and / or out_f32 (either may be NULL, not both), as qea_binarize_sauvola writes.
 * qea_cc_smear — one launch, one direction of run-length smoothing (vertical = 0: along rows, 1: along columns): out_mask (uint8, 1 = ink,
 *   0 = background) = the ink, plus every background pixel with ink at distance a >= 1 before and b >= 1 after it in its row / column and
 *   a + b - 1 <= gap (0..QEA_CC_MAX_GAP).  Outside the page is background.  out_mask must not be in_mask.
 * qea_cc_boxes — one launch: roots is the caller's ascending list of page-relative roots of all pages, int32 [n_roots], page p's being
 *   roots[root_first[p] .. root_first[p + 1]) (root_first: int32 [n_pages + 1] on the device); boxes is int32 [n_roots][4] =
 *   (x_min, y_min, x_max, y_max), which the caller fills with (INT32_MAX, INT32_MAX, -1, -1); every pixel whose label is listed lowers /
 *   raises its row with integer atomicMin / atomicMax (one per tile, distinct root and bound).  Labels that are not listed are skipped.
 * Nothing synchronises, no workspace; the launches of a call do not depend on the page count or content.  Refused before any launch: what
 * the binarisers refuse of the leading arguments (a NULL pointer, n_pages < 1, an empty page, a page over 2^27 pixels, ...), a NULL or
 * misaligned labels / area / roots / root_first / boxes / out_f32, both outputs NULL, connectivity other than 4 or 8, ink_max outside
 * 0..254, min_area < 1, a gap outside 0..QEA_CC_MAX_GAP, n_roots < 0.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these five by symbol.) */
#define QEA_CC_MAX_GAP 127
int qea_cc_label(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h, const int32_t* w,
                 int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first, const uint8_t* ink_mask,
                 int32_t ink_max, int32_t connectivity, int32_t* labels, int32_t* area, void* stream);
int qea_cc_stats(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h, const int32_t* w,
                 int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first, const int32_t* labels,
                 int32_t* area, void* stream);
int qea_cc_despeckle(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                     const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                     const int32_t* labels, const int32_t* area, int32_t min_area, float* out_f32, uint8_t* out_u8, void* stream);
int qea_cc_smear(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h, const int32_t* w,
                 int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first, const uint8_t* in_mask,
                 int32_t ink_max, int32_t gap, int32_t vertical, uint8_t* out_mask, void* stream);
int qea_cc_boxes(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h, const int32_t* w,
                 int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first, const int32_t* labels,
                 const int32_t* roots, const int32_t* root_first, int32_t n_roots, int32_t* boxes, void* stream);

/* Page skew estimation and deskew over the same page store (csrc/deskew.hip; qea/deskew.py: estimate_skew, deskew_pages; the statement,
 * which the device, the host path and tests/deskew_spec.py reproduce bit for bit, is DESIGN.md "Deskew").  Everything is an integer.  The
 * leading arguments and host_h / host_w are those of qea_binarize_sauvola; a page is at most QEA_DESKEW_MAX_SIDE rows and columns and
 * QEA_BINARIZE_MAX_PAGE_PIXELS pixels.  A candidate slope is a / 1024 for a = -A..A, A in 0..QEA_DESKEW_MAX_SLOPE.
 * qea_skew_strip_sums — one launch, one pass over the pixels: C[j][y] = the number of ink pixels of row y in columns [32 j, 32 j + 32) cut
 *   to w, for j < ns = ceil(w / 32).  A pixel is ink iff its 8-bit value is <= ink_max; ink_max is ink_max_dev[p] (int32 [n_pages] on the
 *   device, e.g. the thresholds of qea_binarize_otsu, -1..254, -1 = no ink) where that pointer is given, else the scalar (0..254).  C is a
 *   byte array PACKED LIKE THE STORE: page p's C[j][y] is byte offset[p] + j * h[p] + y (ns h <= h w); nothing else is written.
 * qea_skew_scores — zeroes scores (int64 [n_pages][2 A + 1], hipMemsetAsync on the stream), then one launch: with the shift
 *   d(j, a) = floor((a (32 j + 16 - w div 2) + 512) / 1024) and P_a[r] = sum_j C[j][r + d(j, a)] (rows outside [0, h) count 0),
 *   scores[p][a + A] = sum_{r = 0}^{h - 2} (P_a[r + 1] - P_a[r])^2.  Partial sums over chunks of rows meet in integer atomics: exact.
 * qea_skew_pick — one launch: slopes[p] = the a of the largest score, ties to the smallest |a|, then to the negative one; kept only if
 *   100 (S_a - S_0) >= g S_0 in int64 (g in 0..10000), else 0.  It reads any scores array of that shape.
 * qea_deskew_rotate — ONE launch for all pages (tiles and tile_first of qea_binarize_sauvola): page p is rotated about its centre by the
 *   slope a = slopes[p] (device int32 [n_pages]) into outputs packed like the store.  table is int32 [2 A + 1][2] on the device, row
 *   a + A = (C16, S16) = (round(65536 / n), round(65536 t / n)), t = a / 1024, n = sqrt(1 + t t), built by the HOST.  For output pixel
 *   (x, y), in int64: dx2 = 2 x - (w - 1), dy2 = 2 y - (h - 1), X = C16 dx2 - S16 dy2 + 65536 (w - 1), Y = S16 dx2 + C16 dy2 + 65536 (h - 1),
 *   x0 = X >> 17, y0 = Y >> 17, fx = (X >> 9) & 255, fy = (Y >> 9) & 255 (arithmetic shifts) and
 *   out = ((256 - fx)(256 - fy) p(y0, x0) + fx (256 - fy) p(y0, x0 + 1) + (256 - fx) fy p(y0 + 1, x0) + fx fy p(y0 + 1, x0 + 1) + 32768) >> 16;
 *   nearest = 1 takes p((Y + 65536) >> 17, (X + 65536) >> 17) instead.  A tap outside the page reads fill (0..255).  out_u8 receives the
 *   value, out_f32 norm[value] (norm: 256 fp32 values on the device, float32(v) / 255 built by the host); either may be NULL, not both,
 *   and neither may overlap the store.  A page whose slope lies outside -A..A is left unwritten.
 * Nothing synchronises, no workspace, no LDS beyond a transpose buffer; the launches do not depend on the content.  Refused before any
 * launch: what the binarisers refuse of the leading arguments, a side over QEA_DESKEW_MAX_SIDE, A, g, ink_max, fill or nearest outside
 * their ranges, a NULL or misaligned C / scores / slopes / table / norm / out_f32, both outputs NULL, an output that overlaps the store.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects these four by symbol.) */
#define QEA_DESKEW_MAX_SIDE 32767
#define QEA_DESKEW_MAX_SLOPE 256
#define QEA_DESKEW_MAX_GAIN 10000
int qea_skew_strip_sums(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                        const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* ink_max_dev,
                        int32_t ink_max, uint8_t* C, void* stream);
int qea_skew_scores(const uint8_t* C, int64_t store_elems, const int64_t* offset, const int32_t* h, const int32_t* w, int32_t n_pages,
                    const int32_t* host_h, const int32_t* host_w, int32_t A, int64_t* scores, void* stream);
int qea_skew_pick(const int64_t* scores, int32_t n_pages, int32_t A, int32_t g, int32_t* slopes, void* stream);
int qea_deskew_rotate(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                      const int32_t* w, int32_t n_pages, const int32_t* host_h, const int32_t* host_w, const int32_t* tile_first,
                      const int32_t* slopes, const int32_t* table, int32_t A, int32_t nearest, int32_t fill, const float* norm,
                      float* out_f32, uint8_t* out_u8, void* stream);

/* Word boxes of the same page store cut into CRNN strips (csrc/word_strips.hip; qea/reading.py: word_strips, read_pages; the statement,
 * which the device, the host path and tests/word_strips_spec.py reproduce bit for bit, is DESIGN.md "Word strips").
 * qea_word_strips — ONE launch writes every element of out, fp32 [n][QEA_WORD_STRIP_H][OW].  store / store_is_f32 / store_elems / offset /
 *   h / w / n_pages are the leading arguments of qea_binarize_sauvola (an fp32 element is read as the 8-bit value
 *   (uint8)(min(max(x, 0), 1) * 255.0f)); boxes is int32 [n][5] = (page, x0, y0, x1, y1) on the device, x1 / y1 EXCLUSIVE, any int32 values;
 *   norm is the 256 fp32 values a grey level is written as (float32(v) / 255 built by the host).  Per box: clipped to its page,
 *   cw = x1 - x0, ch = y1 - y0; an empty box, a page index outside 0..n_pages-1, a page that does not lie inside the store or has a side
 *   over QEA_WORD_STRIP_MAX_SIDE give an all-white (1.0f) strip.  ch <= 32: the crop centred in 32 x OW with Python floor division (left =
 *   floor((OW - cw) / 2): an oversize width loses its extra pixel on the left), white elsewhere — the strip of qea_crop_pad_gather.
 *   ch > 32: shrunk by ch / 32 in both axes by the exact area average, lengths in units of 1 / 32 source pixel: sw = ceil(32 cw / ch)
 *   columns; row oy covers [oy ch, (oy + 1) ch), column j covers [j ch, (j + 1) ch) cut to [0, 32 cw); with the integer overlap lengths
 *   wy(oy, r) with source row [32 r, 32 r + 32) and wx(j, c) likewise, S = sum wy wx p(y0 + r, x0 + c), Area = ch min(ch, 32 cw - j ch),
 *   level = floor((2 S + Area) / (2 Area)) in 0..255, value norm[level]; the sw columns are centred in OW by the same rule.  Integers
 *   throughout (64-bit where ch > 2048 needs them), so the result does not depend on any order of summation.
 * No workspace, no atomics, nothing synchronises.  Refused before any launch: a NULL or misaligned pointer (out: 16 bytes), store_is_f32
 * other than 0 / 1, n_pages < 1, store_elems < 1, n < 0 or n > QEA_WORD_STRIP_MAX_BOXES, OW not a multiple of 16 in
 * QEA_WORD_STRIP_MIN_W..QEA_WORD_STRIP_MAX_W.  n = 0 is accepted and launches nothing.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects it by symbol.) */
#define QEA_WORD_STRIP_H 32
#define QEA_WORD_STRIP_MIN_W 64
#define QEA_WORD_STRIP_MAX_W 512
#define QEA_WORD_STRIP_MAX_BOXES (1 << 20)
#define QEA_WORD_STRIP_MAX_SIDE 32767
int qea_word_strips(const void* store, int32_t store_is_f32, int64_t store_elems, const int64_t* offset, const int32_t* h,
                    const int32_t* w, int32_t n_pages, const int32_t* boxes, int32_t n, int32_t OW, const float* norm, float* out,
                    void* stream);

/* CTC forced alignment (csrc/ctc_align.hip; qea/align.py, qea.ops.ctc_align, utils.char_spans; the statement, which the device, the host
 * path and tests/align_spec.py reproduce bit for bit, scores included, is DESIGN.md "Forced alignment"): the best single alignment of a
 * GIVEN label to a sample's log-probs, where the beam searches return labellings, which carry no positions.
 *   scores element (t,n,c) at t*ld_t + n*ld_n + c, converted to fp64 exactly; NaN and +inf count as -inf.  targets: the labels end to
 *   end, int32; target_offsets [N+1] int64, label n = targets[target_offsets[n] .. target_offsets[n+1]), L characters, S = 2L+1 extended
 *   states: ext(s) = blank for even s and l[s>>1] for odd s; skip(s) for odd s >= 3 with l[s>>1] != l[(s>>1)-1].
 *   v_0(0) = lp[0][blank], v_0(1) = lp[0][l_0], the rest -inf; for t >= 1 the candidates are, IN THIS ORDER, stay v_{t-1}(s), step
 *   v_{t-1}(s-1) (s >= 1), skip v_{t-1}(s-2) (skip(s)); the largest wins, of equal ones the earliest; v_t(s) = winner + lp[t][ext(s)], one
 *   fp64 add; the winner's kind 0 / 1 / 2 is the back-pointer.  The path ends in S-1 or S-2 (L >= 1), the larger v_{T-1}, S-1 on equality.
 *   score [N] fp64: that value; -inf = infeasible (T too short for L plus its adjacent repeats; impossible classes on every path), and so
 *   is a label longer than L_max or with an entry outside 0..C-1 or equal to blank: such an entry is never used as an address.
 *   path [N][T] int32: the character index at step t, -1 for blank; -2 throughout an infeasible sample.
 *   first / last [target_offsets[N]] int32, laid out as targets: the steps character k's state 2k+1 occupies (contiguous); -1 / -1 when
 *   infeasible.  char_score, likewise, fp64: lp[t][l_k] added up over t = first .. last in ASCENDING t; -inf when infeasible.
 *   L = 0 is feasible: the all-blank path.  Every sample uses all T steps.
 * L_max bounds the label lengths as S_max does for qea_ctc_loss.  One workgroup per sample, one thread per extended state, the prev rows
 * in LDS and a barrier per step, as the loss scans; the back-pointers, 2 bits each, stay in LDS (32 KB at T = 512, L_max = 127).  One
 * launch, no workspace, no atomics, nothing synchronises; every output element is stored exactly once.
 * Refused before any launch: T outside 1..512, C outside 2..256, blank outside 0..C-1, L_max outside 0..127, N < 0, negative ld_t / ld_n,
 * and with N > 0 a NULL pointer.  N = 0 is accepted and launches nothing.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects it by symbol.) */
int qea_ctc_align(const float* scores, int32_t ld_t, int32_t ld_n, const int32_t* targets, const int64_t* target_offsets, int32_t T,
                  int32_t N, int32_t C, int32_t blank, int32_t L_max, double* score, int32_t* path, int32_t* first, int32_t* last,
                  double* char_score, void* stream);

/* Word boxes grouped into text lines and put into reading order (csrc/lines.hip; qea/lines.py: group_lines, page_text; clean_cli.py
 * --lines --text; the statement, which the device, the host path and tests/lines_spec.py reproduce bit for bit, is DESIGN.md "Text lines").
 * qea_line_group — ONE launch, one workgroup per page, whatever the pages hold.  boxes is int32 [n_boxes][4] = (x_min, y_min, x_max, y_max),
 *   inclusive, any int32 values, on the device, page after page as qea_cc_boxes writes them; box_first is int32 [n_pages + 1] on the
 *   device, page p's boxes being rows box_first[p] .. box_first[p + 1] - 1.  overlap (1..100, per cent), tall (1..QEA_LINE_MAX_TALL) and gap
 *   (0..QEA_LINE_MAX_GAP, 0 = no limit) are the statement's parameters.  All arithmetic is 64-bit.  Per page, with i counting within it:
 *   a box with h_i = y_max - y_min + 1 <= 0 or w_i <= 0 is empty and a line of its own; med = the element of rank (m - 1) div 2 among the
 *   ascending heights of the m non-empty boxes (0 if m = 0); a non-empty box is linkable iff h_i <= tall med; two linkable boxes are in
 *   one height band iff 100 ov >= overlap min(h_i, h_j), ov = min(y_max_i, y_max_j) - max(y_min_i, y_min_j) + 1; under the key
 *   (x_min_i, i), succ(i) / pred(i) is the box of i's band with the smallest key above / the largest key below i's; the link i - succ(i)
 *   exists iff gap = 0 or x_min_succ - x_max_i - 1 <= gap med, the link i - pred(i) iff gap = 0 or x_min_i - x_max_pred - 1 <= gap med; a
 *   line is a connected component of the links, its box the union of its members'; lines are numbered ascending by
 *   (y_min + y_max, x_min, smallest member) of their boxes; a box's position is its rank under (line, x_min, y_min, i).
 *   line / pos / order [n_boxes] int32, laid out as boxes: the box's line, its position, and the inverse of pos (order[first + pos_i] = i).
 *   line_box [n_boxes][4] int32: rows box_first[p] .. box_first[p] + L_p - 1 hold the page's line boxes in line order, the rest of the
 *   page's rows -1.  n_lines [n_pages] int32 = L_p, med [n_pages] int64.
 * max_boxes (0..QEA_LINE_MAX_BOXES) is a HOST value the caller vouches for, the largest page; it sizes the workgroup's LDS tables (36 B per
 * box).  A page of more than max_boxes boxes gets -1 in all of its outputs, n_lines and med included; a page whose range runs backwards or
 * leaves [0, n_boxes] gets n_lines = med = -1 and nothing else.  Neither is read or written out of bounds.
 * The lines are found by a min-index union-find in LDS: no loop runs "until converged", every walk moves to a strictly smaller index.
 * No workspace, no global atomics, nothing synchronises.  Refused before any launch: n_pages < 0, n_boxes < 0, boxes without a page,
 * max_boxes, overlap, tall or gap outside its range, a NULL or misaligned pointer (boxes and line_box: 16 bytes, med: 8).  n_pages = 0
 * is accepted and does nothing; n_boxes = 0 clears n_lines and med (hipMemsetAsync on the stream) and launches nothing.
 * (Additive: no struct changed and qea_version() is unchanged; a caller detects it by symbol.) */
#define QEA_LINE_MAX_BOXES 4096
#define QEA_LINE_MAX_TALL 64
#define QEA_LINE_MAX_GAP 1024
int qea_line_group(const int32_t* boxes, const int32_t* box_first, int32_t n_pages, int32_t n_boxes, int32_t max_boxes, int32_t overlap,
                   int32_t tall, int32_t gap, int32_t* line, int32_t* pos, int32_t* order, int32_t* line_box, int32_t* n_lines,
                   int64_t* med, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QEA_HIP_H */
