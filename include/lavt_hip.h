/*
 * lavt_hip.h -- C ABI of the MI355X (gfx950) LAVT hot-path library (liblavt_hip.so).
 *
 * Every entry point is `extern "C"`, takes raw DEVICE pointers + sizes + a hipStream_t (as void*),
 * allocates nothing, launches asynchronously on the given stream and returns 0 or a negative LAVT_ERR_*
 * code.  No torch types anywhere.  Global state: the (thread-local) last-error string and one table of
 * dispatch switches -- the LAVT_* environment variables listed in lavt-rs_amd/csrc/tuning.hip (and in
 * INTEGRATION.md), which force one of several equivalent kernel configurations (tile sizes, ring depths)
 * for the test-suite.  They are read once, at the first launch; lavt_tuning_reload() re-reads them.  No
 * launch path calls getenv, and no switch makes a kernel skip work.
 *
 * The reference (Yxxxb/LAVT-RS) is pure PyTorch and has no native layer; each group of functions
 * below names the reference code (file:line under the reference root) whose arithmetic it replaces.
 * The Python host side that binds these with ctypes is lavt-rs_amd/lavt_hip/_capi.py;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Layout conventions: activations are token-major / NHWC ([rows][channels], channels contiguous);
 * "dtype" selects the storage type of activations and of the compute copies of the weights
 * (LAVT_F32 = exact-fp32 MFMA path used for parity, LAVT_BF16 = bf16 MFMA with fp32 accumulation).
 * Biases, LayerNorm/BatchNorm affine parameters, statistics and every parameter GRADIENT are fp32.
 */
#ifndef LAVT_HIP_H
#define LAVT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAVT_F32 0
#define LAVT_BF16 1
#define LAVT_FP8 2 /* lavt_gemm_nt only: A and B are OCP e4m3 (1 byte / element, k-contiguous), C / bias / residual bf16, fp32 accumulate */

#define LAVT_OK 0
#define LAVT_ERR_INVALID (-22) /* bad argument (EINVAL) */
#define LAVT_ERR_LAUNCH (-5)   /* kernel launch failed (EIO) */

#define LAVT_ACT_NONE 0
#define LAVT_ACT_GELU 1 /* exact erf form */
#define LAVT_ACT_RELU 2
#define LAVT_ACT_TANH 3
#define LAVT_ACT_GELU_D 4 /* lavt_gemm_nt.act: GELU whose Cpre output holds GELU'(pre) instead of pre (bf16 operands; the derivative shares the
                           * exponential of the activation: +2 fma per element), for a consumer that only needs the derivative (ABI v4).
                           * LayerNorm-folded launches only (ln_wsum): the branch is compiled into that kernel alone */
#define LAVT_ACT_STORED 5 /* lavt_gemm_nt.dact: dact_pre already holds act'(pre) (written by a LAVT_ACT_GELU_D launch): C * dact_pre (ABI v4) */

int lavt_abi_version(void);
const char* lavt_last_error(void);
int lavt_tuning_reload(void); /* ABI v5: re-read the LAVT_* tuning switches from the environment (tests that force a tile configuration) */

/* ---------------------------------------------------------------------------------------------
 * Gather-GEMM, "NT" family:   C[M,N] = epilogue( alpha * A_op[M,K] x B_op[K,N] )
 *
 * Replaces every nn.Linear / 1x1 Conv1d / 3x3 Conv2d forward and data-gradient on the path:
 *   qkv, proj (lib/backbone.py:121,141), Mlp fc1/fc2 (:24-30), PatchMerging.reduction (:286),
 *   PWAM vis_project/f_query/f_key/f_value/W/project_mm (:1244-1327), res_gate (:604-611),
 *   PatchEmbed.proj (:309, after lavt_im2col4), SimpleDecoding conv3x3 (lib/mask_predictor.py:18-38),
 *   and the window partition / roll / pad / reverse copies (lib/backbone.py:33-62, 204-237), which become
 *   row gather (a_rowmap) and row scatter (c_rowmap) of the GEMMs on either side of the attention core.
 *
 * A_op: rows along M with K contiguous.  Row m is read from source row a_rowmap[m] (or m); -1 reads zeros.
 *   conv_cin > 0 makes this an implicit-GEMM 3x3 convolution (pad 1) over a (batch, conv_h, conv_w) pixel grid:
 *   K = 9*conv_kc, k = tap*conv_kc + c, tap = (dy+1)*3+(dx+1); row m = pixel, source row = neighbour pixel
 *   (mirrored neighbour when conv_flip = 1, i.e. the data gradient).  Channels c >= a_split come from A2
 *   (fused torch.cat of [top-down, skip], lib/mask_predictor.py:60,70,81).
 * B_op: b_kmajor = 0: B[N][K] (nn.Linear weight layout);  1: B[K][N] (used for x @ W, i.e. data gradients).
 *   With conv and b_kmajor = 1, k = tap*conv_kc + c addresses B + c*ldb + tap*b_tap_stride + n.
 * Epilogue, in order: *alpha, +bias[n], *row_scale[m / row_scale_div], (Cpre[out_row][n] = value), act, *mul[out_row][n],
 *   +R[out_row][n], store.  Output row = c_rowmap[m] (or m); -1 drops the row: nothing of it is stored, in C, C2 or Cpre.
 *   row_scale is indexed by the GEMM row m; every side buffer that has the output's shape -- Cpre, mul, R, dact_pre -- by the
 *   output row.  Columns >= c_split go to C2 (fused split of the gradient of a concatenation).  c_f32 stores C and C2 as
 *   fp32 whatever dtype is.  With batch > 1, bias / row_scale / C (and C2) advance by their strides per entry; Cpre, mul, R
 *   and dact_pre have no stride.  The kernel writes nothing else: columns between N (or c_split) and ldc keep their bytes.
 * Requirements: K % (16/sizeof(dtype)) == 0; if b_kmajor, N % (16/sizeof(dtype)) == 0; lda/ldb/ldc multiples of
 *   the same; all pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct lavt_gemm_nt {
    int32_t dtype, M, N, K, batch;
    /* A */
    const void* A;
    int64_t lda, strideA;
    const void* A2;
    int64_t lda2;
    int32_t a_split;
    const int32_t* a_rowmap;
    int32_t conv_h, conv_w, conv_kc, conv_flip;
    /* B */
    const void* B;
    int64_t ldb, strideB;
    int32_t b_kmajor;
    int64_t b_tap_stride;
    /* epilogue */
    float alpha;
    const float* bias;
    int64_t strideBias;
    const float* row_scale;
    int64_t strideRowScale;
    int32_t row_scale_div; /* row m uses row_scale[m / row_scale_div] (<=1 means m): per-sample DropPath factors */
    int32_t act;
    void* Cpre;
    int64_t ldcpre;
    const void* R;
    int64_t ldr;
    void* C;
    int64_t ldc, strideC;
    void* C2;
    int64_t ldc2;
    int32_t c_split;
    const int32_t* c_rowmap;
    int32_t c_f32;
    const void* zeros; /* optional: >= 16 bytes of zeros in device memory; enables the LDS-DMA pipeline kernel (bf16) */
    int32_t epi_lds;   /* reserved: always 0 */
    /* 3-D generalisation of the implicit-GEMM convolution (Conv3d of SepTPWAM, lib/video_swin_transformer.py:1327-1460): rows are voxels of a
     * (batch, conv_d, conv_h, conv_w) grid and the taps run over conv_kd x conv_kh x conv_kw (each 1 or 3, 'same' zero padding), kw fastest.
     * All zero = the 2-D default (conv_d = 1, taps 1 x 3 x 3). */
    int32_t conv_d, conv_kd, conv_kh, conv_kw;
    /* Fused activation gradient (ABI v2): when dact_pre != NULL the stored value is C * act'(dact_pre[out_row][n]) (+ R[out_row][n], if given)
     * with act = dact (LAVT_ACT_*), C = (alpha acc + bias) row_scale and out_row the OUTPUT row (c_rowmap[m], as for R and mul):
     * the data gradient of the layer AFTER an activation leaves as the gradient w.r.t. the pre-activation (fc2's dgrad of a Swin Mlp applies
     * GELU' of fc1's saved pre-activation, reference lib/backbone.py:24-30 under autograd), so no separate element-wise pass exists.
     * bf16, b_kmajor, no conv taps, K % 64 == 0, lddact % 8 == 0, no act / mul / Cpre / C2 / c_f32 only (LAVT_ERR_INVALID otherwise: the caller
     * keeps the two-kernel form). */
    const void* dact_pre;
    int64_t lddact;
    int32_t dact;
    /* dtype == LAVT_FP8 (BASELINE.json configs[4]): per-tensor scaling.  deq_a / deq_b point at the device floats holding the |max| the A / B
     * tensors were quantised against (lavt_fp8_quantize*: q = e4m3(x * 448 / amax); a value <= 0 means "scale 1"); the epilogue multiplies the
     * accumulator by (amax_a / 448) * (amax_b / 448) * alpha.  The contraction runs on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block
     * scales (twice the bf16 MFMA rate at half the operand bytes).  Requirements: !b_kmajor, no dact_pre, K % 16 == 0, lda / ldb % 16 == 0,
     * conv_kc (and a_split) % 128 == 0 for the tap-walking fast path. */
    const float* deq_a;
    const float* deq_b;
    int32_t epi_wide; /* set by the library: 16-byte stores from paired accumulator fragments (all row strides / splits 8-element aligned) */
    /* ABI v4, fused PWAM path (reference lib/backbone.py:604-611, 669 and its autograd mirror):
     * mul: element-wise multiplier [out_row][n] applied after the activation and before the residual -- with act = LAVT_ACT_TANH, Cpre, R = x
     *   and mul = r the second gate GEMM writes x + tanh(g) * r directly (the language gate is no separate kernel).
     * res_first (with dact_pre and R): the stored value is (C + R) * act'(dact_pre) instead of C * act'(dact_pre) + R -- a gradient that arrives
     *   beside the GEMM's own contribution joins before the activation gradient. */
    const void* mul;
    int64_t ldmul;
    int32_t res_first;
    /* conv_tap_split > 0 (ABI v4): the reduction of a convolution is cut at tap boundaries over the batch index -- entry bz contracts taps
     * [bz * conv_tap_split, (bz + 1) * conv_tap_split) only (K = conv_tap_split * conv_kc, batch * conv_tap_split = taps; with !b_kmajor strideB
     * advances the packed weight by conv_tap_split * conv_kc elements, with b_kmajor strideB = 0).  Used with c_f32 + strideC as split-K through
     * fp32 partial outputs for the decoder's small-pixel-count convolutions (1 800 rows x K = 13 824: 60-232 tiles with serial chains of 72-216
     * K tiles otherwise); lavt_splitk_reduce adds the partials.  Tap-walking fast path only (conv_kc % 64 == 0). */
    int32_t conv_tap_split;
    /* LayerNorm-folded A operand (ABI v4): ln_wsum != NULL makes this GEMM compute LN(A) B^T + b without a LayerNorm launch: A = the RAW rows of the
     * norm's input, B = the gamma-folded weight and bias = the folded bias of lavt_ln_fold, ln_wsum [N] its row sums; the kernel accumulates the
     * row statistics from the A tiles it streams (K = the normalised width: every tile walks all of it) and applies rstd (acc - mu wsum_n) before the
     * epilogue.  ln_mean / ln_rstd (optional, [M]) receive the statistics for the LayerNorm backward.  bf16, plain k-contiguous problems only
     * (norm2 -> fc1 of a Swin block, lib/backbone.py:243 + :24-30). */
    const float* ln_wsum;
    float* ln_mean;
    float* ln_rstd;
    float ln_eps;
    /* Column statistics of the output from the epilogue (ABI v6): BatchNorm statistics of a bias-free convolution without a pass over its output
     * (reference lib/mask_predictor.py:60-97: conv -> BatchNorm2d -> ReLU).  colstats != NULL: every block of `rows_per_block` output rows (both as
     * reported by lavt_gemm_nt_colstats_plan for this problem) stores, per column n, the sum of its rows and their second moment about the block's
     * own mean -- colstats[(block * 2 + 0) * N + n], colstats[(block * 2 + 1) * N + n] -- taken from the fp32 accumulators (alpha applied, before
     * the rounding to bf16).  lavt_colstats_finish_blocks combines the blocks (parallel-variance form, no E[x^2] - E[x]^2).  Only for launches
     * lavt_gemm_nt_colstats_plan accepts (LAVT_ERR_INVALID otherwise): bf16, batch 1, no bias / activation / residual / row map / fp32 output. */
    float* colstats;
    /* conv_kc_split > 0 (ABI v6): the reduction of a convolution is cut over CHANNEL blocks instead of taps -- entry bz of the batch contracts channels
     * [bz * conv_kc_split, (bz + 1) * conv_kc_split) of every tap (K = taps * conv_kc_split, batch * conv_kc_split = conv_kc, conv_kc_split % 64 == 0,
     * strideB = 0: both weight layouts are offset inside the kernel).  Any divisor of conv_kc / 64 is a split count, where conv_tap_split offers 3 or 9:
     * the decoder's 1 800-row convolutions run as 480 workgroups instead of 180.  With c_f32 + strideC as split-K through fp32 partial outputs
     * (lavt_splitk_reduce).  Pipelined tap-walking kernel only (csrc/gemm_nt_pipe.hip: conv_kc % 64 == 0, a_split % 64 == 0, bf16). */
    int32_t conv_kc_split;
} lavt_gemm_nt_t;

int lavt_gemm_nt(const lavt_gemm_nt_t* p, void* stream);
/* The kernel lavt_gemm_nt(p) launches: one instantiation of one of the three NT kernel families and the arguments the library derives for it
 * (csrc/gemm_nt_plan.hip decides, the families launch from this answer).  A host-side query: nothing is launched and no pointer of p is read
 * through.  New symbol only: no existing prototype or struct changed, lavt_abi_version() stays 7. */
#define LAVT_NT_CLASSIC 0 /* csrc/gemm.hip: register-staged double buffer (fp32, and bf16 without a zero page / 16-byte aligned rows) */
#define LAVT_NT_V2 1      /* csrc/gemm_v2.hip: LDS-DMA ring */
#define LAVT_NT_PIPE 2    /* csrc/gemm_nt_pipe.hip: LDS-DMA ring with the software-pipelined K loop */
#define LAVT_NT_WALK_GENERAL 0 /* every K tile decoded from scratch (K tails, conv taps that fit no faster walk); the classic family's only walk */
#define LAVT_NT_WALK_PLAIN 1   /* no taps, no concat source, K a multiple of the K tile: running pointers */
#define LAVT_NT_WALK_TAPS 2    /* convolution taps walked with the K loop (conv_kc and a_split multiples of the K tile, <= 32 taps) */
#define LAVT_NT_WALK_PARTIAL 3 /* the tap walk with a partial last channel block (conv_kc % 64 != 0; pipelined family, k-contiguous bf16 weights) */
#define LAVT_NT_DACT 1 /* kind bits: fused activation gradient (dact_pre) */
#define LAVT_NT_LNA 2  /* LayerNorm-folded A operand (ln_wsum) */
#define LAVT_NT_GD 4   /* the stored-derivative form: with LNA, act = LAVT_ACT_GELU_D; with DACT, dact = LAVT_ACT_STORED and no residual / bias / row map */
#define LAVT_NT_F8 8   /* e4m3 operands */
typedef struct lavt_gemm_nt_route {
    int32_t family;   /* LAVT_NT_CLASSIC / _V2 / _PIPE */
    int32_t tile;     /* square output tile of a workgroup: 64, 128 or 256 */
    int32_t stages;   /* K tiles in the LDS ring: 2 or 4 (classic: its 2 buffers) */
    int32_t waves;    /* waves per workgroup: 4 or 8 */
    int32_t kwalk;    /* LAVT_NT_WALK_* */
    int32_t b_kmajor; /* B layout the kernel is built for: 0 = B[N][K], 1 = B[K][N] */
    int32_t kind;     /* LAVT_NT_DACT / _LNA / _GD / _F8 bits */
    int32_t lean;     /* epilogue instantiation: 0 full, 1 bias / residual / row scale / row map only, 2 bare store, 3 bare store with C2 kept */
    int32_t epi_wide; /* the value the launch stores into lavt_gemm_nt_t.epi_wide: bit 0 the 16-byte store form, bit 1 side inputs requested before the K loop */
    int32_t dtype;    /* element type of the operands (LAVT_F32 / LAVT_BF16 / LAVT_FP8); the classic family's template type */
} lavt_gemm_nt_route_t;
/* -> LAVT_OK and *out, or LAVT_ERR_INVALID (lavt_last_error set) exactly where lavt_gemm_nt(p) refuses the problem */
int lavt_gemm_nt_route(const lavt_gemm_nt_t* p, lavt_gemm_nt_route_t* out);
/* -> number of row blocks whose partial statistics lavt_gemm_nt(p) would store into p->colstats (0: this problem's kernel has no statistics
 * epilogue -- leave colstats NULL and take the statistics from the output with lavt_colstats_meanrstd); *rows_per_block = rows per block */
int lavt_gemm_nt_colstats_plan(const lavt_gemm_nt_t* p, int* rows_per_block);
/* second stage: blocks' (sum, centred second moment) pairs -> mean / rstd (+ running estimates, momentum form of nn.BatchNorm2d) and / or the
 * (sum, M2) pair of all `rows` rows (sum_out / m2_out: what the SyncBatchNorm exchange carries).  Any of the output groups may be NULL. */
int lavt_colstats_finish_blocks(const float* partials, int nblk, int rows_per_block, int rows, int C, float eps, float* mean, float* rstd,
                                float* sum_out, float* m2_out, float* running_mean, float* running_var, float momentum, void* stream);
/* out[m][n] (dtype) = sum_s parts[s][m][n] (fp32): second stage of a split reduction of lavt_gemm_nt (c_f32 partial outputs, one per batch entry) */
int lavt_splitk_reduce(int dtype, const float* parts, int splits, int64_t M, int N, void* out, int64_t ldc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gather-GEMM, "TN" family (weight gradients):   C[I,J] += alpha * sum_k A[k][i] * B[k][j]      (fp32 C)
 *
 * Replaces the weight-gradient half of autograd for every layer listed above (the reference gets it from
 * torch.autograd; there is no reference source line).  Rows k of A / B are gathered through a_rowmap / b_rowmap
 * (-1 = zero row); conv_cin > 0: J = 9*conv_kc and column j = tap*conv_kc + c reads B row = neighbour pixel of k
 * for that tap (channels >= b_split from B2).  c_conv_permute stores column (tap,c) at c*9+tap so that C is
 * directly the PyTorch [Cout][Cin][3][3] gradient.  The reduction over k is split across workgroups
 * (split_k, 0 = auto) and accumulated with fp32 atomics: C must hold zeros or a running sum.
 * colsum (optional, fp32 [I]) additionally receives the bias gradient under the same factors as C:
 *     colsum[i] += alpha * sum_k s_k * A[a_rowmap[k]][i],      s_k = a_rowscale[k / a_rowscale_div]
 * (s_k = 1 without a row scale; with a_rowscale_binary: 1 where the entry is non-zero -- the caller folded the
 * one non-zero value into alpha, so alpha carries it into C and colsum alike: the fc2 bias gradient of a block
 * under DropPath needs its 1 / keep).  Every kernel of the family computes this.
 * batch > 1: entry b reads A + b * strideA and B + b * strideB and writes C + b * strideC and
 * colsum + b * strideColsum (one vector of I sums per entry); a_rowmap, b_rowmap and a_rowscale are indexed by
 * k alone and shared by the entries, as is B2.
 * accumulate covers colsum as it covers C: 0 promises that both hold zeros (an unsplit launch may store them
 * plainly, a split one adds), 1 adds to their contents; colsum_atomic adds to colsum in either case.
 * Requirements: I, J (and conv_kc) % (16/sizeof(dtype)) == 0; lda/ldb likewise.
 * ------------------------------------------------------------------------------------------- */
typedef struct lavt_gemm_tn {
    int32_t dtype, I, J, K, batch;
    const void* A;
    int64_t lda, strideA;
    const int32_t* a_rowmap;
    const float* a_rowscale; /* optional fp32 factor of A row k: a_rowscale[k / a_rowscale_div] (mask / DropPath of the forward) */
    int32_t a_rowscale_div;
    const void* B;
    int64_t ldb, strideB;
    const void* B2;
    int64_t ldb2;
    int32_t b_split;
    const int32_t* b_rowmap;
    int32_t conv_h, conv_w, conv_kc;
    float alpha;
    float* C;
    int64_t ldc, strideC;
    int32_t c_conv_permute;
    int32_t split_k;
    float* colsum;
    int64_t strideColsum;
    const void* zeros; /* optional zero page, as in lavt_gemm_nt_t */
    int32_t a_rowscale_binary; /* 1: a_rowscale holds only 0 and ONE non-zero value which the caller folded into alpha (row masks) */
    int32_t accumulate;        /* 1: C += (atomics) even without split-K; 0: C may be overwritten when the reduction is not split */
    int32_t conv_d, conv_kd, conv_kh, conv_kw; /* 3-D taps, as in lavt_gemm_nt_t; c_conv_permute then stores column (tap,c) at c*taps+tap */
    float* partials;           /* optional scratch (ABI v3): with it a split reduction (many K pieces on few output tiles: the long-K weight gradients */
    int64_t partials_floats;   /* of PWAM's 1x1 convolutions, K = 28 800 rows) stores one plain partial tile per piece ([piece][I][J], then [piece][I] */
                               /* for colsum) and a second small kernel adds the pieces into C -- instead of up to ~60 workgroups adding into the same */
                               /* 64x64 tile through fp32 atomics.  Needs pieces*(I*J + I) floats (lavt_gemm_tn_pieces gives an upper bound); too small */
                               /* or NULL selects the atomic form.  The scratch may be shared by consecutive calls on one stream. */
    int32_t colsum_atomic;     /* ABI v4: colsum is ADDED with fp32 atomics even where C is stored plainly -- two problems then share one bias gradient:
                                * a windowed qkv weight gradient taken over the REAL tokens only (token order: the zero rows of padded window
                                * positions are skipped, K = tokens instead of window rows) + a side problem over the padded rows alone, whose
                                * dq / dk / dv still belong to the bias gradient (the reference pads after norm1: lib/backbone.py:205-209) */
    int64_t a_src_rows, b_src_rows; /* ABI v7: rows of the tensors that a_rowmap / b_rowmap index (0 = unknown: at most K).  The pipelined grouped kernel addresses a
                                * mapped operand through ONE 2 GB buffer descriptor with 32-bit byte offsets row * ld * 2: a problem whose mapped source
                                * reaches beyond that falls back to the 64x64 launch instead of reading zeros from beyond the descriptor's range */
} lavt_gemm_tn_t;

int lavt_gemm_tn(const lavt_gemm_tn_t* p, void* stream);
/* upper bound of the K pieces lavt_gemm_tn may cut this problem into (for sizing `partials`) */
int lavt_gemm_tn_pieces(const lavt_gemm_tn_t* p);
/* n (<= 6) independent problems of the family in one call, e.g. the four weight gradients of a Swin block: when they qualify (bf16, no
 * conv taps / concat, batch 1, together >= 256 64x64 output tiles) they run as ONE launch without split-K -- every output element then has
 * a single writer, and with accumulate == 0 it is stored plainly instead of added through fp32 atomics; otherwise they are issued one by
 * one exactly as lavt_gemm_tn would.  A member with split_k < 0 declares that its C (and colsum) hold ZEROS, so that storing and adding
 * give the same result: the grouped launch may then cut its reduction into up to 4 pieces that meet through atomics (the launch lasts as
 * long as its longest serial chain of K tiles). */
int lavt_gemm_tn_grouped(const lavt_gemm_tn_t* probs, int n, void* stream);
/* lavt_gemm_tn_grouped + ONE LayerNorm backward as rider workgroups (ABI v5): the partial-sum form of lavt_layernorm_bwd_partial (bf16, no gather; dy, x,
 * gamma, mean, rstd, dx, dres, rows, C, ws as there) needs nothing from the grouped launch and the launch nothing from it, so when the group runs on the
 * 64x64 launch with column sums (the four weight gradients of a Swin block) the LayerNorm's workgroups are appended to its grid instead of being a launch
 * of their own on the critical chain (norm1's backward of a Swin block: 7.7 us x 24 per Swin-B step).  In every other case the two are issued one after
 * the other: same result. */
int lavt_gemm_tn_grouped_ln(const lavt_gemm_tn_t* probs, int n, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                            void* dx, float* ws, int64_t ws_floats, const void* dres, int rows, int C, void* stream);
/* The same launch in stream-K form (ABI v5): 128x128 tiles, the K-tile iterations of all members cut into equal runs for ~512 persistent
 * workgroups (every workgroup ingests the same number of bytes); tiles whose reduction is split between runs meet through `scratch` (plain partial
 * tiles + a fixed-order sum: no atomics).  lavt_gemm_tn_grouped_sk_ws returns the floats of scratch the group wants, or 0 when it does not qualify
 * (conv taps, batch > 1, too little work): call lavt_gemm_tn_grouped then.  Members' `partials` fields are ignored. */
int64_t lavt_gemm_tn_grouped_sk_ws(const lavt_gemm_tn_t* probs, int n);
int lavt_gemm_tn_grouped_sk(const lavt_gemm_tn_t* probs, int n, float* scratch, int64_t scratch_floats, void* stream);
/* What lavt_gemm_tn(p) launches: the kernel family, its instantiation, the K pieces and how they meet in C (csrc/gemm_tn_plan.hip decides, the
 * families launch from this answer).  A host-side query: nothing is launched and no pointer of p is read through.  New symbols only: no existing
 * prototype or struct changed, lavt_abi_version() stays 7. */
#define LAVT_TN_CLASSIC 0 /* csrc/gemm.hip: register-staged double buffer (fp32, and bf16 problems the LDS-DMA kernels decline); always adds atomically */
#define LAVT_TN_V2 1      /* csrc/gemm_tn_v2.hip: LDS-DMA ring, bf16 */
#define LAVT_TN_STORE 0   /* one writer per output element, stored plainly */
#define LAVT_TN_ATOMIC 1  /* fp32 atomics (K pieces meeting in C, or accumulate) */
#define LAVT_TN_PARTS 2   /* K pieces stored as plain tiles into `partials`, added into C by tn_reduce_pieces */
typedef struct lavt_gemm_tn_route {
    int32_t family;       /* LAVT_TN_CLASSIC / _V2 */
    int32_t dtype;        /* element type of the operands; the classic family's template type */
    int32_t tile, waves;  /* square output tile of a workgroup (64 / 128) and its waves (4 / 8) */
    int32_t maps;         /* the K loop that carries row maps / the row mask (V2) */
    int32_t colsum_form;  /* V2: 0 none, 1 scalar walk of the LDS tile, 2 on the matrix cores */
    int32_t convp;        /* V2: the kernel with the tap state of a convolution weight gradient */
    int32_t kt_per_piece; /* K tiles (64 rows; classic fp32: 16) per piece */
    int32_t pieces;       /* K pieces = grid z, none of them empty */
    int32_t write;        /* LAVT_TN_STORE / _ATOMIC / _PARTS */
} lavt_gemm_tn_route_t;
/* -> LAVT_OK and *out, or LAVT_ERR_INVALID (lavt_last_error set) exactly where lavt_gemm_tn(p) refuses the problem */
int lavt_gemm_tn_route(const lavt_gemm_tn_t* p, lavt_gemm_tn_route_t* out);
/* What a grouped entry launches for n problems.  entry: LAVT_TN_ENTRY_GROUPED (lavt_gemm_tn_grouped; with ln_rows > 0 lavt_gemm_tn_grouped_ln
 * offering a LayerNorm backward over [ln_rows][ln_C]) or LAVT_TN_ENTRY_SK (lavt_gemm_tn_grouped_sk).  A host-side query, as above. */
#define LAVT_TN_GROUP_MAX 6
#define LAVT_TN_ENTRY_GROUPED 0
#define LAVT_TN_ENTRY_SK 1
#define LAVT_TN_EACH 0    /* the group does not form: one lavt_gemm_tn per problem */
#define LAVT_TN_GROUP64 1 /* csrc/gemm_tn_v2.hip: 64x64 tiles, gemm_tn_v2_grouped_kernel / _grouped_ln_kernel */
#define LAVT_TN_PIPE 2    /* csrc/gemm_tn_pipe.hip: 128x128 software-pipelined tiles */
#define LAVT_TN_SK 3      /* csrc/gemm_tn_v2.hip: stream-K on 128x128 tiles + tn_streamk_fixup */
#define LAVT_TN_REDUCE_NONE 0
#define LAVT_TN_REDUCE_GROUP 1     /* tn_reduce_pieces_group */
#define LAVT_TN_REDUCE_PIPE 2      /* tnp_reduce_pieces */
#define LAVT_TN_REDUCE_PIPE_DEEP 3 /* tnp_reduce_pieces_deep */
#define LAVT_TN_RIDER_NONE 0  /* no LayerNorm was offered */
#define LAVT_TN_RIDER_RIDES 1 /* it runs as extra workgroups of the launch */
#define LAVT_TN_RIDER_AFTER 2 /* the entry launches it on its own after the weight gradients */
typedef struct lavt_gemm_tn_group_route {
    int32_t launch;      /* LAVT_TN_EACH / _GROUP64 / _PIPE / _SK */
    int32_t stages;      /* ring depth: 2, the pipelined launch 3 / 4 (EACH: 0) */
    int32_t maps;        /* some member carries row maps / a row mask (GROUP64, SK: the kernel's MAPS) */
    int32_t colsum_form; /* 0 none, 1 scalar (SK), 2 matrix cores (GROUP64, PIPE) */
    int32_t workgroups;  /* workgroups of the weight gradients (riders not counted; SK: the persistent workgroups; EACH: 0) */
    int32_t pieces[LAVT_TN_GROUP_MAX], kt_per_piece[LAVT_TN_GROUP_MAX]; /* per member (EACH: of its own lavt_gemm_tn_route) */
    int32_t parts[LAVT_TN_GROUP_MAX]; /* per member: its pieces go through its partials scratch */
    int32_t any_parts, reducer, reducer_grid_x; /* LAVT_TN_REDUCE_* and the x size of its grid (y = n) */
    int32_t rider, rider_lpr, rider_blocks, rider_wgs; /* LAVT_TN_RIDER_*; RIDES: lanes per row, LayerNorm units and the workgroups they occupy */
    int64_t scratch_floats; /* SK: floats of scratch (what lavt_gemm_tn_grouped_sk_ws answers) */
} lavt_gemm_tn_group_route_t;
/* -> LAVT_OK and *out, or LAVT_ERR_INVALID: a member lavt_gemm_tn refuses (EACH), a group the stream-K entry does not take */
int lavt_gemm_tn_group_route(const lavt_gemm_tn_t* probs, int n, int entry, int ln_rows, int ln_C, lavt_gemm_tn_group_route_t* out);

/* 3x3 / pad 1 / no-bias convolution weight gradient with the nine taps fused (ABI v5; bf16; csrc/conv_wgrad.hip) -- the gradient autograd computes for
 * SimpleDecoding's conv1_4 .. conv2_2 (lib/mask_predictor.py:60-97):  dW[co][ci][tap] += sum_p dY[p][co] * X[p + (dy, dx)][ci],
 * tap = (dy + 1) * 3 + (dx + 1), pixels p over B images of H x W (NHWC rows), X = the channel concat of x1 (c1 channels) and x2 (Cin - c1; NULL
 * for a single source).  dW is the [Cout][Cin][3][3] parameter gradient itself: accumulate != 0 adds to it, 0 overwrites it (a zeroed buffer with
 * this one writer: saves reading it).  `parts`: caller-lent fp32 scratch of
 * lavt_conv3x3_wgrad_ws(...) floats (partial tiles of the split pixel reduction; no atomics, run-to-run identical); _ws returns 0 for shapes the
 * kernel does not cover (Cout % 128, Cin % 8, c1 % 64, W <= 128) -- use lavt_gemm_tn's tap-shifted form + lavt_unpack_conv_grad then. */
int64_t lavt_conv3x3_wgrad_ws(int B, int H, int W, int Cout, int Cin, int c1);
int lavt_conv3x3_wgrad(const void* dy, int64_t ldy, const void* x1, int64_t ldx1, const void* x2, int64_t ldx2, int c1, int B, int H, int W, int Cout,
                       int Cin, float* parts, int64_t parts_floats, float* dW, int accumulate, const void* zeros, void* stream);
/* The same gradient from OCP e4m3 operands on the fp8 MFMA (round 5; BASELINE.json configs[4]): dy, x1, x2 hold bytes q = value * 448 / |max|
 * ([pixels][channels]; leading dimensions in bytes, multiples of 16) -- the copies lavt_fp8_quantize / lavt_fp8_quantize_current wrote for the forward
 * convolution and the data gradient --, amax_dy / amax_x point at the |max| each was quantised against (x1 and x2 share one scale: they feed one
 * contraction); dW receives the de-quantised fp32 gradient.  Scratch as lavt_conv3x3_wgrad_ws.  lavt_conv3x3_wgrad_f8_ok returns 0 for shapes the
 * kernel does not cover (32 < W <= 128, Cout % 128, Cin % 16, c1 % 64, H even when W <= 64): use the bf16 entry then. */
int lavt_conv3x3_wgrad_f8_ok(int B, int H, int W, int Cout, int Cin, int c1);
int lavt_conv3x3_wgrad_f8(const void* dy, int64_t ldy, const float* amax_dy, const void* x1, int64_t ldx1, const void* x2, int64_t ldx2, const float* amax_x, int c1,
                          int B, int H, int W, int Cout, int Cin, float* parts, int64_t parts_floats, float* dW, int accumulate, const void* zeros, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Shifted-window attention core (WindowAttention.forward, lib/backbone.py:123-140; mask :634-652).
 * qkv: [nwin*N][3C] in windowed row order (columns s*C + h*32 + d, s in {q,k,v}), head_dim = C/heads.
 * out: [nwin*N][C].  bias: dense fp32 [heads][N][bias_ld] (from lavt_relpos_expand; bias_ld = N rounded up to a multiple
 * of 16 -- 64 for 7x7, 160 for 12x12, 416 for the 392-token 8x7x7 video windows -- lets the bf16 MFMA kernels run; padding columns hold -1e30).  region: optional int8
 * [nw_img][N] region ids of the shift mask (window w uses row w % nw_img); unequal ids add -100.
 * lse: fp32 [nwin][heads][N] log-sum-exp of each score row (saved for backward).
 * table = relative_position_bias_table fp32 [(2wd-1)(2wh-1)(2ww-1)][heads] with the FULL window shape (wd, wh, ww) (wd = 1 for the 2-D Swin;
 *   a clipped video window has N < wd*wh*ww tokens and uses the top-left block of the index matrix).  The bf16 MFMA kernels (N <= 400: Q, K, V(, dO) of a whole window in LDS;
 *   WindowAttention3D.forward, lib/video_swin_transformer.py:137-168, with its default 8x7x7 window included) keep the head's table column in LDS and never read the dense bias: `bias` may then be NULL; lavt_attn_uses_table(dtype, N) tells.
 * Backward: dqkv [nwin*N][3C] (every element written); dtable accumulates the table gradient.  bf16 MFMA kernel: every (window, head)
 *   writes its fp32 dS slab into ws (lavt_window_attn_bwd_ws floats; bias_ld = 64 / 160 / 416) with plain stores;
 *   two small kernels sum the slabs over windows, bin them by relative-position index and add the result to dtable (LDS float atomics inside the attention
 *   kernel measured 37 of 57 us per window-head).  Exact-fp32 kernel: global atomics into dtable; needs the dense `bias`.
 * ------------------------------------------------------------------------------------------- */
int lavt_window_attn_fwd(int dtype, const void* qkv, const float* bias, int bias_ld, const int8_t* region, int nw_img, void* out,
                         float* lse, const float* table, int wd, int wh, int ww, int nwin, int N, int heads, int head_dim, float scale,
                         void* stream);
int lavt_window_attn_bwd(int dtype, const void* qkv, const float* bias, int bias_ld, const int8_t* region, int nw_img,
                         const void* out, const void* dout, const float* lse, void* dqkv, const float* table, float* dtable,
                         float* ws, int64_t ws_floats, float* parts, int wd, int wh, int ww, int nwin, int N, int heads, int head_dim, float scale,
                         void* stream);
/* Chained table-gradient binning (ABI v5, bf16 MFMA path, deferred form).  The binning of a launch's dS slabs is needed by nothing before the end of
 * backward, yet as its own launch it sat on the critical chain (7.5 us x 24 per Swin-B step).  lavt_window_attn_bwd_chained does not launch it: it
 * describes it in *mine, and runs the job `prev` describes -- the binning of an EARLIER launch, whose slabs must still be alive -- as extra
 * workgroups of this launch (they fill CU slots the (window, head) workgroups leave free).  lavt_attn_dtable_run launches a job on its own (the last
 * one of a backward pass).  parts as in lavt_window_attn_bwd. */
typedef struct {
    const void* slab;
    float* part;
    int32_t slab_ld, wd, wh, ww, nwin, N, heads, rows_per_block, win_per_group, gx, gz;
} lavt_dtable_job_t;
int lavt_window_attn_bwd_chained(int dtype, const void* qkv, int bias_ld, const int8_t* region, int nw_img, const void* out, const void* dout,
                                 const float* lse, void* dqkv, const float* table, float* ws, int64_t ws_floats, float* parts, int wd, int wh, int ww,
                                 int nwin, int N, int heads, int head_dim, float scale, const lavt_dtable_job_t* prev, lavt_dtable_job_t* mine, void* stream);
int lavt_attn_dtable_run(const lavt_dtable_job_t* job, void* stream);
/* 1 when lavt_window_attn_fwd/bwd take the bias from the table for this (dtype, N) -- no dense bias / lavt_relpos_expand needed */
int lavt_attn_uses_table(int dtype, int N);
/* Deferred table gradient (bf16 MFMA path): with `parts` != NULL (a caller-owned buffer of lavt_window_attn_bwd_pieces(...) * heads * (2wd-1)(2wh-1)(2ww-1)
 * floats that outlives the call) lavt_window_attn_bwd leaves its per-workgroup table histograms there and does not touch dtable; one
 * lavt_attn_dtable_finish_multi launch later adds the histograms of any number of layers into their table gradients:
 * desc = device int64 [n][5] rows {parts, pieces, heads, R, dtable}; max_R / max_heads size the grid. */
int lavt_window_attn_bwd_pieces(int dtype, int nwin, int N, int heads, int bias_ld);
int lavt_attn_dtable_finish_multi(const int64_t* desc, int n, int max_R, int max_heads, void* stream);
/* the same launch sized for the (layer, head) pairs that exist: total_heads = sum over the n <= 64 layers of their head counts */
int lavt_attn_dtable_finish_multi_compact(const int64_t* desc, int n, int max_R, int total_heads, void* stream);
/* floats of scratch (`ws`) lavt_window_attn_bwd wants for these shapes: dS slabs + per-workgroup table histograms (0 for the exact-fp32 kernel) */
int64_t lavt_window_attn_bwd_ws(int dtype, int nwin, int N, int heads, int bias_ld, int wd, int wh, int ww);

/* Streaming (online-softmax) bf16 kernels for windows too large for the fused ones (N > 400: Video-Swin --window12, 8x12x12 = 1152 tokens;
 * WindowAttention3D.forward, lib/video_swin_transformer.py:137-168 with window_size (8, 12, 12), lib/segmentation.py:63).  Same arithmetic
 * contract as lavt_window_attn_fwd / _bwd above (qkv, out, region, lse, table of the FULL window, top-left index block of a clipped window), without
 * the dense bias: K and V stream through LDS, nothing of size nwin * heads * N^2 is formed.
 * lavt_window_attn_stream_ok: 1 when the kernels cover the problem (bf16, head_dim 32, 16 <= N <= 2048, N <= wd*wh*ww, the table column fits the LDS budget).
 * Backward: dqkv [nwin*N][3C] (every element written); dtable ACCUMULATES the table gradient.  No float atomics: bitwise reproducible.  ws: caller-lent
 * scratch of lavt_window_attn_stream_bwd_ws floats = nwin*heads*N (delta = rowsum(dO o O)) + heads*N*ld (dense bias gradient summed over windows,
 * ld = N rounded up to a multiple of 32; binned by lavt_relpos_reduce). */
int lavt_window_attn_stream_ok(int dtype, int N, int wd, int wh, int ww, int heads, int head_dim);
int lavt_window_attn_stream_fwd(int dtype, const void* qkv, const int8_t* region, int nw_img, void* out, float* lse, const float* table,
                                int wd, int wh, int ww, int nwin, int N, int heads, int head_dim, float scale, void* stream);
int64_t lavt_window_attn_stream_bwd_ws(int dtype, int nwin, int N, int heads, int wd, int wh, int ww);
int lavt_window_attn_stream_bwd(int dtype, const void* qkv, const int8_t* region, int nw_img, const void* out, const void* dout, const float* lse,
                                void* dqkv, const float* table, float* dtable, float* ws, int64_t ws_floats, int wd, int wh, int ww, int nwin, int N,
                                int heads, int head_dim, float scale, void* stream);

/* relative_position_bias_table[(2wd-1)(2wh-1)(2ww-1)][heads] -> dense bias[heads][N][ld]   (wd = 1 for the 2-D Swin; N <= wd*wh*ww tokens) (lib/backbone.py:89-103,125-127)
 * and its transpose (dense gradient -> table gradient, deterministic, accumulates into dtable). */
int lavt_relpos_expand(const float* table, float* dense, int wd, int wh, int ww, int N, int heads, int ld, void* stream);
int lavt_relpos_reduce(const float* ddense, float* dtable, int wd, int wh, int ww, int N, int heads, int ld, void* stream);
/* Row softmax of attention scores for windows too large for the fused kernels (Video-Swin N = 392 / 1152; WindowAttention3D.forward,
 * lib/video_swin_transformer.py:147-161): p[row][j] = softmax_j(s[row][j] + bias[i][j] + mask), i = row % rpw, window = row / rpw (rpw >= N rows
 * per window, rows i >= N are padding and give p = 0); s already holds scale * q k^T (lavt_gemm_nt); padding columns of p (j >= N, up to ld)
 * are written as 0.  heads >= 1: rows come in blocks of rpw ordered (window, head): block b is window b / heads with bias[b % heads] (bias is
 * [heads][N][bias_ld]); heads = 1 for one head at a time.  Backward overwrites dp with ds. */
int lavt_attn_softmax_fwd(int dtype, const void* s, const float* bias, int bias_ld, const int8_t* region, int nw_img, void* p,
                          int64_t rows, int rpw, int N, int ld, int heads, void* stream);
int lavt_attn_softmax_bwd(int dtype, const void* p, void* dp, int64_t rows, int N, int ld, void* stream);
/* dense bias gradient of that path: out[h][i][j] (fp32 [heads][N][ld]) = sum_w ds[w][h][i][j], ds [nwin][heads][rpw][ld] in `dtype` (the `.sum(0)` over
 * windows that autograd performs for the broadcast `attn + relative_position_bias.unsqueeze(0)`, lib/video_swin_transformer.py:151-153);
 * feed the result to lavt_relpos_reduce. */
int lavt_attn_dbias_sum(int dtype, const void* ds, float* out, int nwin, int heads, int N, int rpw, int ld, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm over the channel dimension (nn.LayerNorm, eps 1e-5; lib/backbone.py:201,243,285,328,510).
 * x,y: [rows][C].  mean/rstd: fp32 [rows] saved for backward.  gamma/beta fp32 [C].
 * gather != NULL: row r of the INPUT is assembled from 4 source rows gather[4r..4r+3] of C/4 channels each
 * (-1 = zeros): the 2x2 neighbour concat of PatchMerging (lib/backbone.py:278-283) fused into its LayerNorm.
 * Backward accumulates dgamma/dbeta (fp32 atomics); with gather, dx rows are scattered back (every source
 * row appears exactly once).
 * ------------------------------------------------------------------------------------------- */
int lavt_layernorm_fwd(int dtype, const void* x, const int32_t* gather, const float* gamma, const float* beta, void* y,
                       float* mean, float* rstd, int rows, int C, float eps, void* stream);
int lavt_layernorm_bwd(int dtype, const void* dy, const void* x, const int32_t* gather, const float* gamma,
                       const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta, float* ws, int64_t ws_floats,
                       const void* dres, int rows, int C, void* stream);
/* Deferred form: the weight / bias gradients of a LayerNorm feed nothing but the gradient buffer, so their partial sums need not be reduced
 * inside backward.  lavt_layernorm_bwd_partial writes ONLY the per-workgroup partials (ws: >= lavt_layernorm_bwd_blocks(...) * 2 * C floats,
 * [block][dgamma | dbeta][C]) besides dx; lavt_reduce_partials_multi later adds any number of such partial sets into their gradients in ONE
 * launch: desc = device int64 [n][5] rows {partials, blocks, C, dgamma, dbeta}.  (60 two-kernel reductions per Swin-B step -> 1 launch.) */
int lavt_layernorm_bwd_blocks(int dtype, int rows, int C);
int lavt_layernorm_bwd_partial(int dtype, const void* dy, const void* x, const int32_t* gather, const float* gamma, const float* mean,
                               const float* rstd, void* dx, float* ws, int64_t ws_floats, const void* dres, int rows, int C, void* stream);
/* LayerNorm backward that also writes the LayerNorm OUTPUT xn = xhat * gamma + beta (ABI v4): for a forward that folded the norm into the consumer's GEMM
 * (lavt_gemm_nt.ln_wsum) and never materialised it; the consumer's weight gradient reads xn.  _partial_xn = the deferred-reduction form. */
int lavt_layernorm_bwd_partial_xn(int dtype, const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                  void* dx, void* xn, float* ws, int64_t ws_floats, const void* dres, int rows, int C, void* stream);
/* ABI v7: the same launch + the table-gradient binning job of an earlier lavt_window_attn_bwd_chained launch as rider workgroups (`job` as that call
 * returned it in *mine).  xn == beta == NULL: the plain form (lavt_layernorm_bwd_partial without gather).  Returns 1 and launches NOTHING when this
 * LayerNorm geometry has no rider form: issue the two launches separately. */
int lavt_layernorm_bwd_partial_xn_dtable(int dtype, const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                         void* dx, void* xn, float* ws, int64_t ws_floats, const void* dres, int rows, int C, const lavt_dtable_job_t* job, void* stream);
int lavt_layernorm_bwd_xn(int dtype, const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                          void* dx, void* xn, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, const void* dres, int rows, int C, void* stream);
int lavt_reduce_partials_multi(const int64_t* desc, int n, int total_column_blocks, void* stream); /* total_column_blocks = sum over the sets of lavt_reduce_partials_column_blocks(C) (<= 0: unknown; a larger number -- e.g. the ceil(2 C / 32) of the first ABI v6 builds -- only starts idle workgroups) */
int lavt_reduce_partials_column_blocks(int C);
/* dres (optional, [rows][C], not with gather): gradient of the residual stream that bypassed the LayerNorm (x -> LN(x) and x -> + ...):
 * dx = LN'(dy) + dres in the same pass, instead of a separate element-wise add of the two gradients of x */

/* ---------------------------------------------------------------------------------------------
 * Per-channel statistics over rows, and the normalisations built on them:
 *   InstanceNorm1d over all H*W positions (PWAM f_query / W, lib/backbone.py:1311-1327): groups = batch;
 *   BatchNorm2d (+ReLU) of the decoder (lib/mask_predictor.py:19-37; SyncBN = all-reduce of sums between the calls).
 * lavt_colstats: x [groups][rows][C] -> sum = sum_r x and m2 = sum_r (x - mean_group)^2, fp32 [groups][C] (with scratch the call clears them itself; without it pass zeroed buffers).
 *   The second moment is centred (accumulated about the group's first row, then re-centred), never E[x^2]-E[x]^2.
 *   Combining ranks (SyncBN): all-reduce sum -> global mean; m2_r += rows_r*(mean_r - mean)^2; all-reduce m2.
 * lavt_stats_finalize: mean = sum/count, var = m2/count (biased), rstd = 1/sqrt(var+eps); optional running-stat update (unbiased var).
 * ws / ws_floats (here and in lavt_norm_bwd_stats): optional fp32 scratch of >= 1025*groups*2*C floats; with it the per-workgroup partial
 *   sums are written out and reduced by a second tiny kernel instead of contending atomics on the same C addresses.  lavt_layernorm_bwd's
 *   scratch is lavt_layernorm_bwd_blocks(dtype, rows, C) * 2 * C floats (up to 2048 blocks); a smaller one selects the atomic form (slow:
 *   hundreds of workgroups adding to the same C addresses).
 * lavt_norm_apply: y = ((x-mean)*rstd*gamma + beta) (*mul) with optional ReLU; mean/rstd [groups][C]; gamma/beta/mul optional.
 * lavt_norm_bwd_stats: s1 = sum(g), s2 = sum(g*xhat) (cleared by the call when scratch is given, else added to the zeroed buffers passed in) with g = dy (*mul) masked by relu (y>0);  [groups][C].
 *   With relu, gamma / beta given and no mul (BatchNorm + ReLU of the decoder) the mask is recomputed from x with lavt_norm_apply's own expression and y is not read
 *   (lavt_norm_bwd_apply likewise): two of the seven map passes of the BatchNorm backward less.
 * lavt_norm_bwd_apply: dx = gamma*rstd*(g - s1/n - xhat*s2/n); dmul = dy*xhat_affine (optional).
 * ------------------------------------------------------------------------------------------- */
int lavt_colstats(int dtype, const void* x, float* sum, float* m2, float* ws, int64_t ws_floats, int groups, int rows, int C, void* stream);
/* SyncBatchNorm forward after the all-gather of every rank's (sum, m2) pair (allst: [world][2][C], `rows_per_rank` rows each): parallel-variance
 * combination + lavt_stats_finalize in one launch (mean / rstd of the global batch, running estimates with the unbiased variance) */
int lavt_syncbn_combine(const float* allst, int world, float rows_per_rank, float eps, float* mean, float* rstd, float* running_mean,
                        float* running_var, float momentum, int C, void* stream);
/* lavt_colstats + lavt_stats_finalize in two launches instead of four, for the cases where nothing sits between the sums and their use
 * (InstanceNorm; BatchNorm without a cross-rank exchange): mean / rstd [groups][C] directly, optional running-statistics update (groups == 1). */
int lavt_colstats_meanrstd(int dtype, const void* x, float* mean, float* rstd, float* ws, int64_t ws_floats, int groups, int rows, int C, float eps,
                           float* running_mean, float* running_var, float momentum, void* stream);
int lavt_stats_finalize(const float* sum, const float* m2, float count, float eps, float* mean, float* rstd,
                        float* running_mean, float* running_var, float momentum, int n, void* stream);
int lavt_norm_apply(int dtype, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                    const void* mul, int relu, void* y, int groups, int rows, int C, void* stream);
int lavt_norm_bwd_stats(int dtype, const void* dy, const void* x, const void* y, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const void* mul, int relu, float* s1, float* s2,
                        float* ws, int64_t ws_floats, int groups, int rows, int C, void* stream);
int lavt_norm_bwd_apply(int dtype, const void* dy, const void* x, const void* y, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const void* mul, int relu, const float* s1, const float* s2,
                        float count, void* dx, void* dmul, int groups, int rows, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Element-wise pieces.
 * ------------------------------------------------------------------------------------------- */
/* dx = dy * act'(pre)   (GELU of Mlp / PWAM projections, ReLU of res_gate) */
int lavt_act_bwd(int dtype, int act, const void* dy, const void* pre, void* dx, int64_t n, void* stream);
/* language gate, lib/backbone.py:669:  xo = x + tanh(gpre) * r ;  backward gives dgpre, dr (+= into dr_acc semantics: written) */
/* O(batch) glue of a forward, one launch each (ABI v5).  lavt_lang_mask: l_mask [B][n_l] (float32, or int64 with is_int64 = 1) -> mask_rows [B * n_l]
 * (float) and maskbias [B][ld] = 1e4 * m - 1e4, -1e4 beyond n_l (lib/backbone.py:1360).  lavt_droppath_factors: f[n][B] = floor(keep[n] + u[n][B]) / keep[n]
 * (timm drop_path, the reference's DropPath: lib/backbone.py:6, 240-245) from one uniform draw u. */
int lavt_lang_mask(const void* l_mask, int is_int64, float* mask_rows, float* maskbias, int B, int n_l, int ld, void* stream);
int lavt_droppath_factors(const float* u, const float* keep, float* f, int n, int B, void* stream);
/* the same factors with the uniform draw made on the device: u[e] = (Philox4x32-10(key = state[0], counter = (state[1], e, 0))[0] >> 8) * 2^-24; the
 *   kernel advances state[1] (two uint64 in device memory: seed, draw counter), so a captured step draws fresh factors on every replay */
int lavt_droppath_draw(void* state, const float* keep, float* f, int n, int B, void* stream);
int lavt_gate_fwd(int dtype, const void* x, const void* gpre, const void* r, void* xo, int64_t n, void* stream);
int lavt_gate_bwd(int dtype, const void* dxo, const void* gpre, const void* r, const void* dr_add, void* dgpre, void* dr, int64_t n, void* stream); /* dr = dxo * tanh(gpre) (+ dr_add) */

/* ---------------------------------------------------------------------------------------------
 * One-kernel W-MSA / SW-MSA forward (ABI v4, bf16): norm1 + pad / roll / window_partition + qkv + relative-position-bias attention
 * (SwinTransformerBlock.forward lib/backbone.py:201-217, WindowAttention.forward :113-140).  One workgroup per (window, head): the window's
 * token rows (row map, -1 = padded token) and the head's 96 weight rows stream through an LDS-DMA ring, LayerNorm is applied algebraically
 * (raw rows x gamma-folded weights, row statistics from the resident tiles, epilogue rstd (acc - mu wsum) + biasp; padded tokens get the plain
 * bias: the reference pads after norm1), q / k / v stay in LDS for the attention core.  Side outputs for backward: qkv [nwin*N][3C], the
 * LayerNorm output xn [tokens][C] and its row statistics.  Needs C = 32 * heads, C % 64 == 0, ws * ws <= 160.
 *   lavt_ln_fold: Wg[n][k] = bf16(gamma_k W[n][k]), wsum[n] = sum_k Wg[n][k], biasp[n] = bias_n + sum_k beta_k W[n][k]   (per weight update)
 * ------------------------------------------------------------------------------------------- */
int lavt_ln_fold(const float* W, const float* gamma, const float* beta, const float* bias, void* Wg, float* wsum, float* biasp, int N, int K, void* stream);
/* every fold of a model in one launch: desc int64 [count][9] = {W, gamma, beta, bias, Wg, wsum, biasp, N, K} in device memory */
int lavt_ln_fold_multi(const int64_t* desc, int count, void* stream);
int lavt_wmsa_fwd(const void* x, const int32_t* wmap, const void* Wg, const float* wsum, const float* biasp, const float* bias, const float* gamma,
                  const float* beta, const float* table, const int8_t* region, int nw_img, void* out, float* lse, void* qkv, void* xn, float* mean,
                  float* rstd, const void* zeros, int ws, int nwin, int N, int heads, int C, float eps, float scale, void* stream);
/* The same launch with a zero-fill RIDER (ABI v5): fill_bytes bytes at fill (16-byte aligned, multiples of 16) are set to zero by extra workgroups appended
 * to the launch's grid.  The step harness zeroes its flat gradient buffer this way, a slice per stage-2 block: the fill is needed by nothing before
 * backward, and as its own launch (58 us at the HBM rate for Swin-B's 475 MB) it headed the captured chain. */
int lavt_wmsa_fwd_rider(const void* x, const int32_t* wmap, const void* Wg, const float* wsum, const float* biasp, const float* bias, const float* gamma,
                        const float* beta, const float* table, const int8_t* region, int nw_img, void* out, float* lse, void* qkv, void* xn, float* mean,
                        float* rstd, const void* zeros, int ws, int nwin, int N, int heads, int C, float eps, float scale, void* fill, int64_t fill_bytes,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused PWAM (ABI v4, bf16).  Replaces, with the GEMMs above, PWAM.forward (lib/backbone.py:1265-1278),
 * SpatialImageLanguageAttention.forward (:1329-1372) and the language gate (:604-611, :669) and their autograd backward.
 * The instance norm of the query folds into the keys and the W projection collapses onto the <= 32 word probabilities
 * (w = P (V Wo^T) + bo, so IN(w) = (P - Pbar) VW' from the word statistics alone): see csrc/pwam.hip; tests/pwam_stages.py states every kernel in fp64.
 * Word axes are padded to 32 slots; B samples of T pixels each, rows [B*T]; C % 32 == 0.
 *   lavt_pwam_words_fwd: P[row][32] = softmax_{j < n_l}(alpha * IN_T(q) K^T + maskbias)   (q raw, mean / rstd [B][C] of q over the T pixels)
 *   lavt_pwam_lang_fwd:  from V [B][32][ldv], Wo [C][C] (bf16 compute copy), PP = P^T P [B][32][32], sumP [B][32]:
 *                        VW' channel-major VWc [B][C][32] and word-major VWw [B][32][C] (bf16), beta = -Pbar VW' [B][C], rw = rstd of w [B][C],
 *                        Pbar [B][32], Cov [B][32][32]
 *   lavt_pwam_mix mode 0: out0 = GELU(X + xbias) * (Wd Wc^T + v0)      (mm = vis * IN(w);  Wd = P, Wc = VWc, v0 = beta, X = x Wv^T, xbias = bv)
 *                 mode 1: out0 = D * what * GELU'(X), out1 = D * GELU(X)  (d vpre, d what;  D = d mm)
 *                 mode 2: out0 = Wd Wc^T + v0 - X * v1                  (dq;  Wd = dS, Wc = K''^T, X = q)
 *   lavt_pwam_lang_bwd1: HT = dwhat^T P [B][C][32], s = colsum(dwhat) [B][C] -> dVW [B*32][C] (bf16), partial records of Q [32][32] and u [32] in Qp
 *   lavt_pwam_words_bwd: dS[row][32] = P * (dP - sum_j P_j dP_j),  dP = dwhat VW'^T - P Q + (Pbar Q - u)
 *   lavt_pwam_lang_bwd2: G = dS^T q [B][32][C], sdS = colsum(dS) [B][32] -> dK [B*32][lddk] (bf16), K''^T [B][C][32] (bf16), c0, c1 [B][C]
 * ------------------------------------------------------------------------------------------- */
int lavt_pwam_words_fwd(const void* q, int64_t ldq, const void* K, int64_t ldk, const float* mean, const float* rstd, const float* maskbias,
                        void* P, int B, int T, int C, int n_l, float alpha, void* stream);
/* ABI v7: the same launch also leaves the second moments of the word probabilities as per-workgroup records -- rec [B][lavt_pwam_words_records(B, T, C)][1056]
 * floats: [32][32] P^T P | [32] colsum(P) over the workgroup's rows (of the bf16 P it stored) -- which lavt_pwam_lang_fwd_records adds in index order:
 * replaces the P^T P launch and its reduction launch.  rec == NULL: as lavt_pwam_words_fwd. */
int lavt_pwam_words_fwd_moments(const void* q, int64_t ldq, const void* K, int64_t ldk, const float* mean, const float* rstd, const float* maskbias,
                                void* P, float* rec, int B, int T, int C, int n_l, float alpha, void* stream);
int lavt_pwam_words_records(int B, int T, int C);
int lavt_pwam_words_bwd(const void* dwhat, int64_t ldx, const void* VWw, const float* Qp, const float* pbar, const void* P,
                        void* dS, int B, int T, int C, void* stream);
int lavt_pwam_q_parts(int C); /* records per sample in Qp: [B][records][1024 Q | 32 u] floats, written by lavt_pwam_lang_bwd1, summed in fixed order by lavt_pwam_words_bwd */
int lavt_pwam_mix(int mode, const void* Wd, const void* Wc, const float* v0, const float* v1, const float* xbias, const void* X, int64_t ldx, const void* D, int64_t ldd,
                  void* out0, int64_t ld0, void* out1, int64_t ld1, int B, int T, int C, void* stream);
int lavt_pwam_lang_fwd(const void* V, int64_t ldv, const void* Wo, const float* PP, const float* sumP, void* VWc, void* VWw, float* beta, float* rw,
                       float* pbar, float* cov, int B, int T, int C, float eps, void* stream);
/* ABI v7: lavt_pwam_lang_fwd with the moments given as records (PP == NULL): rec [B][nrec][1056] of lavt_pwam_words_fwd_moments */
int lavt_pwam_lang_fwd_records(const void* V, int64_t ldv, const void* Wo, const float* PP, const float* sumP, const float* rec, int nrec, void* VWc, void* VWw,
                               float* beta, float* rw, float* pbar, float* cov, int B, int T, int C, float eps, void* stream);
int lavt_pwam_lang_bwd1(const float* HT, const float* s, const void* VWc, const float* rw, const float* pbar, const float* cov, void* dVW, float* Qp,
                        int B, int T, int C, void* stream);
/* ABI v7: lavt_pwam_mix(1) on workgroups that own one 64-channel group, with H^T = dwhat^T P and colsum(dwhat) as a by-product when rec != NULL:
 * rec [B][lavt_pwam_mix1_records(B, T, C)][C * 33] floats (per record C x 32 H^T, then C sums), added in record order by lavt_pwam_lang_bwd1_records
 * (HT == NULL): replaces the H launch and its reduction launch. */
int lavt_pwam_mix1(const void* P, const void* VWc, const float* beta, const float* xbias, const void* X, int64_t ldx, const void* D, int64_t ldd, void* dvpre,
                   int64_t ld0, void* dwhat, int64_t ld1, float* rec, int B, int T, int C, void* stream);
int lavt_pwam_mix1_records(int B, int T, int C);
int lavt_pwam_lang_bwd1_records(const float* HT, const float* s, const float* rec, int nrec, const void* VWc, const float* rw, const float* pbar, const float* cov,
                                void* dVW, float* Qp, int B, int T, int C, void* stream);
int lavt_pwam_lang_bwd2(const float* G, const float* sdS, const void* K, int64_t ldk, const float* mean, const float* rstd, void* dK, int64_t lddk, void* K2c,
                        float* c0, float* c1, int B, int T, int C, float alpha, void* stream);
/* masked softmax over the (padded) word axis of PWAM scores, lib/backbone.py:1358-1361.
 * s,p: [rows][ld] (only the first n_l columns are real; p's padding columns are written as 0). */
int lavt_rowsoftmax_fwd(int dtype, const void* s, void* p, int64_t rows, int n_l, int ld, void* stream);
int lavt_rowsoftmax_bwd(int dtype, const void* p, const void* dp, void* ds, int64_t rows, int n_l, int ld, void* stream);
/* bilinear resize, align_corners=True, NHWC (F.interpolate in lib/mask_predictor.py:59,69,80) */
int lavt_bilinear_fwd(int dtype, const void* x, void* y, int B, int Hi, int Wi, int Ho, int Wo, int C, void* stream);
/* Producers that write the e4m3 twin of their bf16 output (round 5; BASELINE.json configs[4]): q = e4m3(bf16(y) * 448 / *amax_prev) (scale 1 while
 * *amax_prev <= 0) -- exactly the bytes lavt_fp8_quantize(y) would write -- and |max| of y recorded into *amax_cur by atomic max (delayed scaling):
 * the quantiser launch in front of the consuming fp8 convolution disappears.  lavt_norm_bwd_apply_amax records |max| of the stored dx into *amax
 * (zeroed by the caller once per step, lavt_fp8_advance does): the |max| pass of lavt_fp8_quantize_current disappears. */
int lavt_bilinear_fwd_q8(const void* x, void* y, void* q, const float* amax_prev, float* amax_cur, int B, int Hi, int Wi, int Ho, int Wo, int C, void* stream);
int lavt_norm_apply_q8(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* mul, int relu, void* y,
                       void* q, const float* amax_prev, float* amax_cur, int groups, int rows, int C, void* stream);
int lavt_norm_bwd_apply_amax(const void* dy, const void* x, const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const void* mul, int relu, const float* s1, const float* s2, float count, void* dx, void* dmul, float* amax, int groups, int rows,
                             int C, void* stream);
int lavt_bilinear_bwd(int dtype, const void* dy, void* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, void* stream);
/* final logits: NHWC [B,Hi,Wi,2] (dtype) -> NCHW fp32 [B,2,Ho,Wo] (lib/_utils.py:21) and its gradient */
int lavt_logits_up_fwd(int dtype, const void* x, float* y, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_logits_up_bwd(int dtype, const float* dy, void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
/* The caller's step right after the path, fused: bilinear upsample (align_corners) of the 2-class low-resolution logits
 * x NHWC [B,Hi,Wi,2] to (Ho, Wo) + class-weighted cross-entropy against target int64 [B,Ho,Wo] (losses.py:7-11, weights (w0, w1);
 * targets other than 0 / 1 are ignored) + the I / U pixel counts of train.py:64-76 (prediction = argmax, class 0 on ties).
 * The [B,2,Ho,Wo] logits are never materialised.  out4 = {loss, sum of weights, I, U} (device, fp32); ws: >= 4*2048 floats of scratch.
 * Backward: dx NHWC [B,Hi,Wi,2] = dloss[0] (device scalar, NULL = 1) * d loss / d x, recomputed from x (gather form, no atomics). */
int lavt_upsample_ce_fwd(int dtype, const void* x, const int64_t* target, float w0, float w1, float* ws, int64_t ws_floats, float* out4,
                         int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_ce_bwd(int dtype, const void* x, const int64_t* target, float w0, float w1, const float* out4, const float* dloss,
                         void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
/* Fused bilinear upsample (align_corners) + MultiClassDiceLoss (reference losses.py:38-77, `--loss mc_dice`, train.py:703-704) on the 2-class
 * low-resolution logits x NHWC [B,Hi,Wi,2]; target int64 [B,Ho,Wo] in {0,1}.  stats (device fp32, 2 + 6*B floats) = {loss, 0, then per sample
 * {I0, I1, sum p0^2, sum p1^2, #[t==0], #[t==1]}}; ws: >= 6*256*B floats of scratch.  Backward: dx = dloss[0] (NULL = 1) * d loss / d x, gather form.
 * With Hi == Ho and Wi == Wo the upsample is the identity: the same entry points serve the un-fused criterion on full-resolution logits. */
int lavt_upsample_dice_fwd(int dtype, const void* x, const int64_t* target, float* ws, int64_t ws_floats, float* stats,
                           int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_dice_bwd(int dtype, const void* x, const int64_t* target, const float* stats, const float* dloss, void* dx,
                           int B, int Hi, int Wi, int Ho, int Wo, void* stream);
/* Annotated-frame selection.  A2D-Sentences / JHMDB annotate one frame per clip, and the reference selects before it scores (train.py:282-285,
 * 366-369; test.py:182-205): valid = [i * t + ind ...]; output_valid = index_select(output, 0, valid); criterion(output_valid, masks).
 * The _sel_ pairs are the two fused criteria above with that indirection: x NHWC [B,Hi,Wi,2] holds all B frames, sel is a DEVICE int32 [nsel],
 * target int64 [nsel,Ho,Wo]; sample j of the loss reads logits frame sel[j] and target j.  out4 / stats (2 + 6*nsel floats, per SELECTED sample; the
 * Dice mean is over nsel samples and 2 classes) cover the nsel selected frames only; scratch as above with nsel in the place of B.
 * Backward writes EVERY element of dx [B,Hi,Wi,2]: frames named by sel get the gradient, all others exactly +0.0 (both forms of the cross-entropy
 * backward, the 8x8 LDS tile form and the wave-per-pixel form; every frame scans sel for its own index -- nsel is a handful -- no inverse table).
 * Contract for sel: 0 < nsel <= B; the entries are distinct and lie in [0, B).  The kernels read sel on the device, so a replayed graph follows a
 * changed buffer, and therefore they cannot raise: an entry outside [0, B) is never dereferenced and contributes nothing (no loss term, no counts,
 * zero Dice sums; lavt_gather_samples zero-fills that sample); of two equal entries the first receives the gradient.  Distinctness and range are
 * checked on the host wherever the indices arrive from the host (lavt_hip.engine: set_valid_indices). */
int lavt_upsample_ce_sel_fwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float w0, float w1, float* ws,
                             int64_t ws_floats, float* out4, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_ce_sel_bwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float w0, float w1, const float* out4,
                             const float* dloss, void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_dice_sel_fwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float* ws, int64_t ws_floats,
                               float* stats, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_dice_sel_bwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, const float* stats, const float* dloss,
                               void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
/* Fused bilinear upsample (align_corners) + DiceBoundaryLoss (reference losses.py:142-244, `--loss dice_boundary`, train.py:709-711; the rates are
 * args.py:83-84: dice_rate 1, boundary_rate 0.05) on the 2-class low-resolution logits x NHWC [B,Hi,Wi,2]; target int64 [B,Ho,Wo] in {0,1}.
 *   loss = dice_rate * dice + boundary_rate * boundary; dice is the criterion of lavt_upsample_dice_*; boundary = mean over (sample, class c) of 1 - BF1:
 *   a = 1 - p_c, h = 1 - [t == c]; pred_b = maxpool3(a) - a, gt_b = maxpool3(h) - h, pred_b_ext = maxpool5(pred_b), gt_b_ext = maxpool5(gt_b) (stride 1, windows
 *   clipped at the border); S1 = sum pred_b gt_b_ext, S2 = sum pred_b, S3 = sum pred_b_ext gt_b, S4 = sum gt_b; P = S1 / (S2 + 1e-7), R = S3 / (S4 + 1e-7),
 *   BF1 = 2 P R / (P + R + 1e-7)                                                                                                 (losses.py:191-244).
 * stats (device fp32, 3 + 14*n floats, n = samples) = {loss, dice, boundary, then per sample {I0, I1, sum p0^2, sum p1^2, #[t==0], #[t==1],
 * S1..S4 of class 0, S1..S4 of class 1}}.  One workgroup per 32x32 output tile recomputes the probabilities of the tile and its halo in LDS: the
 * [B,2,Ho,Wo] probabilities are never written.  No floating-point atomics anywhere: results are identical from run to run.
 * ws: lavt_upsample_dice_boundary_ws(n, Ho, Wo) floats of scratch -- the forward's partial rows (14 per tile and sample), then the backward's
 * fp32 map dz [n,Ho,Wo] = d loss / d (z1 - z0); forward and backward may be lent the same buffer or different ones of that size.
 * Backward: dx NHWC [B,Hi,Wi,2] = dloss[0] (device scalar, NULL = 1) * d loss / d x in two launches: the dz map per tile (the gradient passes both
 * max-pools by arg-max, torch's choice: window scanned row-major, the first maximum wins), then its transposed bilinear in gather form.
 * With Hi == Ho and Wi == Wo the upsample is the identity (lavt-rs_amd/losses.py: DiceBoundaryLoss on full-resolution logits).
 * _sel_: annotated-frame selection exactly as for the pairs above (sel DEVICE int32 [nsel], target [nsel,Ho,Wo], stats / ws with n = nsel). */
int64_t lavt_upsample_dice_boundary_ws(int n, int Ho, int Wo);
int lavt_upsample_dice_boundary_fwd(int dtype, const void* x, const int64_t* target, float dice_rate, float boundary_rate, float* ws, int64_t ws_floats,
                                    float* stats, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_dice_boundary_bwd(int dtype, const void* x, const int64_t* target, float dice_rate, float boundary_rate, const float* stats,
                                    const float* dloss, float* ws, int64_t ws_floats, void* dx, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_dice_boundary_sel_fwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float dice_rate, float boundary_rate,
                                        float* ws, int64_t ws_floats, float* stats, int B, int Hi, int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_dice_boundary_sel_bwd(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, float dice_rate, float boundary_rate,
                                        const float* stats, const float* dloss, float* ws, int64_t ws_floats, void* dx, int B, int Hi, int Wi, int Ho,
                                        int Wo, void* stream);
/* dst[j] = src[sel[j]] for whole samples of sample_elems elements (dtype LAVT_F32 / LAVT_BF16; src holds B samples, dst nsel <= 65535): the gather of
 * the backbone outputs in front of the BatchNorm-folded decoder when only the annotated frames are scored (test.py:182-205 selects behind the
 * decoder; in eval mode the decoder is per-sample independent).  16-byte copies when the sample size and both bases are multiples of 16 bytes,
 * element copies otherwise.  sel as above. */
int lavt_gather_samples(int dtype, const void* src, const int32_t* sel, int nsel, int B, int64_t sample_elems, void* dst, void* stream);
/* The backward of that gather for a pair-list TRAIN batch (the reference trains one image per sentence, train.py:197-243, on datasets that carry
 * several sentences per image, data/dataset_refer_bert.py; here stage 0 runs once per image and its rows are gathered per slot):
 *   dx[b] = sum over {j : sel[j] == b} of dy[j]        dy holds nsel samples, dx B, sel is the DEVICE int32 [nsel] of the forward.
 * Gather form, no atomics: a workgroup owns a slice of one image's sample, walks j = 0 .. nsel-1, adds the slots that name its image and stores
 * once.  THE SUMMATION ORDER IS FIXED: ascending j, fp32 adds starting from +0.0, and for bf16 one round-to-nearest-even at the end -- the same bits
 * on every launch, so the default and the deterministic mode share the kernel.  Every element of dx is written: an image no slot names gets zeros
 * (dx may arrive uninitialised).  An entry of sel outside [0, B) is never read through and contributes nothing: memory-safe for any buffer
 * contents.  A slot that names another image costs a workgroup one scalar load and no vector traffic, so the launch reads nsel samples and writes
 * B.  16-byte accesses when the sample size and both bases are multiples of 16 bytes, element accesses otherwise, as in the forward.
 * 1 <= nsel <= 65535, 1 <= B <= 65535 (a grid dimension), sample_elems > 0, dtype LAVT_F32 / LAVT_BF16; else LAVT_ERR_INVALID, nothing launched.
 * Correct for any nsel in range, but every workgroup scans all of sel: linear in nsel per workgroup.  Training uses tens of slots. */
int lavt_gather_samples_bwd(int dtype, const void* dy, const int32_t* sel, int nsel, int B, int64_t sample_elems, void* dx, void* stream);
/* ---- fp8 (OCP e4m3) operand preparation for lavt_gemm_nt(dtype = LAVT_FP8) ----
 * lavt_fp8_quantize: activations, delayed scaling: dst[i] = e4m3(clamp(src[i] * s, +-448)), s = *amax_prev > 0 ? 448 / *amax_prev : 1 (the |max| seen
 *   in the PREVIOUS step; the GEMM reads the same float through deq_a); max |src| of THIS call is folded into *amax_cur (atomic max).
 * lavt_fp8_advance: start of a step, for n slots: prev[i] = cur[i] > 0 ? cur[i] : prev[i]; cur[i] = 0.
 * lavt_fp8_quantize_weight: fp32 parameter -> e4m3 with CURRENT scaling (*amax is computed here, over the whole tensor); taps > 1 re-packs a
 *   [Cout][Cin][taps] convolution weight as [Cout][taps][Cin] (the implicit-GEMM layout) on the way. */
int lavt_fp8_quantize(int src_dtype, const void* src, void* dst, int64_t n, const float* amax_prev, float* amax_cur, void* stream);
int lavt_fp8_advance(float* amax_prev, float* amax_cur, int n, void* stream);
/* lavt_fp8_quantize_current: CURRENT scaling for tensors whose range moves from step to step (the dY operand of the e4m3 data gradients): *amax = max |src|
 *   of THIS tensor (computed here, one extra read pass), dst[i] = e4m3(src[i] * 448 / *amax); the GEMM reads *amax through deq_a.  No calibration step. */
int lavt_fp8_quantize_current(int src_dtype, const void* src, void* dst, int64_t n, float* amax, void* stream);
int lavt_fp8_quantize_weight(const float* src, void* dst, float* amax, int cout, int cin, int taps, void* stream);
/* lavt_fp8_quantize_weight_t: the same scaling, packed TRANSPOSED as [Cin][taps][Cout] -- the k-contiguous weight operand of the e4m3 data gradient
 *   (reference lib/mask_predictor.py:60-97, backward of the 3x3 convolutions: dX[m][ci] = sum over (tap, co) of dY[m - tap][co] * W[co][ci][tap]). */
int lavt_fp8_quantize_weight_t(const float* src, void* dst, float* amax, int cout, int cin, int taps, void* stream);
/* classifier head conv1_1: 1x1 conv hidden->2 with bias (lib/mask_predictor.py:50,99) */
int lavt_cls_head_fwd(int dtype, const void* x, const float* w, const float* b, void* y, int64_t rows, int C, void* stream);
int lavt_cls_head_bwd(int dtype, const void* x, const void* dy, const float* w, void* dx, float* dw, float* db,
                      int64_t rows, int C, void* stream);
/* the same backward with the weight / bias gradient sums left as one record per workgroup (pw [blocks][2 C], pb [blocks][2], blocks =
 *   lavt_cls_head_bwd_blocks) for lavt_reduce_partials_multi: no global atomics, run-to-run identical sums */
int lavt_cls_head_bwd_blocks(int dtype, int64_t rows, int C);
int lavt_cls_head_bwd_partial(int dtype, const void* x, const void* dy, const float* w, void* dx, float* pw, float* pb,
                              int64_t rows, int C, void* stream);
/* PatchEmbed im2col: NCHW fp32 image -> [B*H4*W4][48] patches (zero padded to x4), lib/backbone.py:318-324;
 * col2im scatters the patch gradient back to an NCHW fp32 image gradient. */
int lavt_im2col4(int dtype, const float* img, void* cols, int B, int H, int W, void* stream);
int lavt_col2im4(int dtype, const void* dcols, float* dimg, int B, int H, int W, void* stream);
/* layout / dtype plumbing */
int lavt_cast(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n, void* stream);
int lavt_nchw_to_nhwc(int src_dtype, const void* src, int dst_dtype, void* dst, int B, int C, int HW, void* stream);
int lavt_nhwc_to_nchw(int src_dtype, const void* src, int dst_dtype, void* dst, int B, int C, int HW, void* stream);
/* conv weight fp32 [Cout][Cin][taps] (taps = 9 for 3x3, 27 for 3x3x3, ...) -> dtype [Cout][taps][Cin] (compute copy used by lavt_gemm_nt) */
int lavt_pack_conv3x3(const float* w, int dtype, void* packed, int Cout, int Cin, int taps, void* stream);
/* gradient counterpart: dw fp32 [Cout][Cin][taps] += packed fp32 [Cout][taps][Cin] (what lavt_gemm_tn writes without c_conv_permute) */
int lavt_unpack_conv_grad(const float* packed, float* dw, int Cout, int Cin, int taps, void* stream);
/* many small fp32 -> dtype casts in one launch: desc = int64 triples (src_ptr, dst_ptr, n) on the DEVICE */
int lavt_cast_multi(const int64_t* desc, int count, int dst_dtype, void* stream);
/* The caller's optimizer step (train.py:688-700: torch.optim.AdamW + LambdaLR((1 - it/T)^0.9)) as one
 * multi-tensor launch.  desc: int64 [count][5] = {param, grad, exp_avg, exp_avg_sq (fp32 device pointers), numel}; hyper: fp32 [count][5] =
 * {base lr, weight decay, beta1, beta2, eps} (both tables in device memory); step: device fp32 scalar = optimizer steps taken so far,
 * incremented by the call (so a captured hipGraph keeps advancing its schedule); lr = base lr * (1 - step/total_steps)^power, or the
 * base lr when total_steps <= 0.  Update rule identical to torch.optim.AdamW (decoupled decay, bias-corrected moments) with amsgrad off;
 * amsgrad on: lavt_adamw_step_chunks_amsgrad below. */
int lavt_adamw_step(const int64_t* desc, const float* hyper, int count, float* step, float total_steps, float power, void* stream);
/* The same update driven by a chunk table (ABI v4): desc int64 [count][6] = {param, grad, exp_avg, exp_avg_sq, numel, copy} -- a non-zero `copy` is the
 * parameter's bf16 compute copy in the same layout, written by the same kernel (the mixed-precision trainer's re-cast of the weights the next
 * forward reads, without a second pass over the parameters); chunks int32 [nchunks][2] = {tensor index, chunk index}: workgroup c updates elements
 * [chunk * lavt_adamw_chunk_elems(), ...) of its tensor, so every workgroup has work.  hyper, step, schedule as above. */
#define LAVT_ADAMW_DESC_COLS 6 /* int64 columns of a desc row, in this order: */
#define LAVT_ADAMW_DESC_PARAM 0
#define LAVT_ADAMW_DESC_GRAD 1
#define LAVT_ADAMW_DESC_EXP_AVG 2
#define LAVT_ADAMW_DESC_EXP_AVG_SQ 3
#define LAVT_ADAMW_DESC_NUMEL 4
#define LAVT_ADAMW_DESC_COPY 5
#define LAVT_ADAMW_HYPER_COLS 5 /* fp32 columns of a hyper row, in this order: */
#define LAVT_ADAMW_HYPER_LR 0
#define LAVT_ADAMW_HYPER_WEIGHT_DECAY 1
#define LAVT_ADAMW_HYPER_BETA1 2
#define LAVT_ADAMW_HYPER_BETA2 3
#define LAVT_ADAMW_HYPER_EPS 4
int lavt_adamw_chunk_elems(void);
int lavt_adamw_step_chunks(const int64_t* desc, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps, float power, void* stream);
/* The guard around the optimizer step (csrc/optim.hip): every decision is taken on the device, so the sequence can be captured into a
 * hipGraph.  All three entry points were added under ABI v7 (new symbols only: no existing prototype or struct changed).
 *
 * Control block `ctl`: device fp32[8], zero-initialised by the caller except ctl[1] = 1.
 *   [0] global L2 norm of the gradients        [1] clip coefficient the update multiplies every gradient by
 *   [2] skip: 1 = this update must not happen  [3] running count of skipped updates (incremented by the guarded update's tick)
 *   [4] hold: written by the HOST only; non-zero = the update does nothing and nothing is counted
 *   [5] accumulating: written by lavt_grad_accumulate; 1 = this micro-step does not end its accumulation cycle -- lavt_grad_norm and the guarded
 *       updates then behave as under hold (no store, ctl[0..3] and the step counter untouched)
 *   [6] micro index m of the accumulation cycle, 0 <= m < k: read by lavt_grad_accumulate, advanced by the guarded update's tick
 *   [7] reserved, zero.   Without lavt_grad_accumulate [5] and [6] stay 0 and every entry point below computes what it computed before they existed.
 *
 * lavt_grad_norm: global L2 norm over the gradients listed by the desc / chunks tables of the chunked update above (so it covers exactly the
 * tensors the update touches), in two launches without atomics: one workgroup per chunk writes an fp32 sum of squares to ws[chunk], one
 * workgroup adds the partials in fp64 in a fixed order -- the result is bitwise reproducible from run to run.  It then writes
 *   ctl[0] = norm;  ctl[1] = min(1, max_norm / (norm + 1e-6)) if max_norm > 0 and the norm is finite, else 1 (torch.nn.utils.clip_grad_norm_);
 *   ctl[2] = 1 if skip_nonfinite != 0 and the norm is NaN or Inf, else 0 (rewritten by every call).
 * A chunk's fp32 sum of squares that overflows for finite gradients (|g| ~ 1e19 and beyond) makes the norm Inf: that counts as non-finite.
 * ws: device scratch of lavt_grad_norm_ws floats; the formula is part of the interface:  ws floats = nchunks  (one partial per chunk).
 *
 * lavt_adamw_step_chunks_guarded: the chunked update with every gradient multiplied by ctl[1]; if ctl[2] != 0 or ctl[4] != 0 (or ctl[5] != 0) every workgroup
 * returns before its first store (parameters, both moments and the bf16 `copy` column stay untouched) and the step counter does not advance;
 * ctl[3] += ctl[2] unless on hold (hence the non-const pointer).  With ctl[1] = 1, ctl[2] = ctl[4] = 0 the result equals the unguarded
 * update's bit for bit (one shared update body). */
#define LAVT_CTL_NORM 0 /* the slots of the control block, as numbered above */
#define LAVT_CTL_CLIP 1
#define LAVT_CTL_SKIP 2
#define LAVT_CTL_SKIPPED 3
#define LAVT_CTL_HOLD 4
#define LAVT_CTL_ACCUMULATING 5
#define LAVT_CTL_MICRO 6
#define LAVT_CTL_FLOATS 8
int64_t lavt_grad_norm_ws(int nchunks);
int lavt_grad_norm(const int64_t* desc, const int32_t* chunks, int nchunks, float* ws, float* ctl, float max_norm, int skip_nonfinite, void* stream);
int lavt_adamw_step_chunks_guarded(const int64_t* desc, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps, float power,
                                   float* ctl, void* stream);
/* AMSGrad (train.py:689-693, --amsgrad; a new symbol under ABI v7): the chunked update with a fifth fp32 stream x = max_exp_avg_sq.
 * torch.optim.AdamW(amsgrad=True), single-tensor form:
 *   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  x = max(x, v)   (the UNcorrected second moment, after its update; a NaN stays)
 *   p = p*(1 - lr*wd) - (lr/bc1) * m / (sqrt(x)/sqrt(bc2) + eps)
 * desc, hyper, chunks, step and the schedule are those of lavt_adamw_step_chunks (desc keeps its six columns, so lavt_grad_norm reads the same
 * table); vmax: device int64 [count] = the fp32 device pointer of x for every desc row.  ctl == NULL: the unguarded update and tick of
 * lavt_adamw_step_chunks.  ctl != NULL: the control block above, obeyed as by lavt_adamw_step_chunks_guarded -- g is multiplied by ctl[1] first;
 * on skip or hold nothing is stored (x included), the step counter does not advance, and ctl[3] += ctl[2] unless on hold (hence non-const). */
int lavt_adamw_step_chunks_amsgrad(const int64_t* desc, const int64_t* vmax, const float* hyper, const int32_t* chunks, int nchunks, float* step, float total_steps,
                                   float power, float* ctl /* NULL: unguarded */, void* stream);
/* Gradient accumulation over k micro-batches (a new symbol under ABI v7): fold the flat fp32 gradient g [n] of one micro-batch into the accumulation
 * buffer acc [n] (no overlap with g) and keep the phase of the cycle in the control block above, all on the device.  With s = 1/k (fp32) and
 * m = ctl[6]:
 *   ctl[4] != 0 (hold): nothing is read or written -- acc, ctl[5] and ctl[6] keep their bits;
 *   otherwise  acc[i] = (m == 0) ? s * g[i] : fmaf(s, g[i], acc[i])  -- the first micro-step of a cycle SELECTS: acc is not read, so it needs no
 *   zero fill and a NaN / Inf left by an earlier cycle cannot survive -- and then ctl[5] = (m != k - 1).
 * One streaming launch, no atomics, bitwise reproducible; float4 accesses when both bases are 16-byte aligned, element by element otherwise and for
 * the n % 4 tail.  m itself is advanced -- m = (m + 1) % k, not under hold -- by the tick of the guarded update that follows in the same step
 * (lavt_adamw_step_chunks_guarded, lavt_adamw_step_chunks_amsgrad with ctl), after every kernel of that step has read the phase: the sequence of
 * one micro-step is  lavt_grad_accumulate -> [lavt_grad_norm over acc] -> guarded update over acc.  On the k-th micro-step of a cycle ctl[5] = 0 and
 * norm, clip, non-finite skip and update act on acc = the mean of the k gradients; on the others they do nothing.  1 <= k <= 2^20. */
int lavt_grad_accumulate(const float* g, float* acc, int64_t n, int k, float* ctl, void* stream);
/* Weight EMA (two new symbols under ABI v7): the chunked update with one more fp32 stream e = the exponential moving average of the parameter.
 * torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)), applied after the parameter update from the registers that hold
 * the new p:   step[0] == 0 (the first applied update): e = p;   otherwise  e += (1 - decay) * (p - e).
 * desc, hyper, chunks, step, the schedule and ctl are those of lavt_adamw_step_chunks_amsgrad; ema: device int64 [count] = the fp32 device pointer of e
 * for every desc row; vmax: the AMSGrad table, or NULL for the plain rule; 0 < decay < 1.  ctl == NULL: the unguarded update and tick.  ctl != NULL: on
 * skip, hold or an accumulating micro-step nothing is stored, e included -- the average moves exactly when the parameters move.
 * lavt_ema_swap: p <-> e in place for every tensor of the same tables (one launch; every element is read and written by one thread); where
 * desc[.][5] names a bf16 compute copy it is written from the new p.  Two calls restore every bit. */
int lavt_adamw_step_chunks_ema(const int64_t* desc, const int64_t* vmax /* NULL: no AMSGrad */, const int64_t* ema, const float* hyper, const int32_t* chunks, int nchunks,
                               float* step, float total_steps, float power, float decay, float* ctl /* NULL: unguarded */, void* stream);
int lavt_ema_swap(const int64_t* desc, const int64_t* ema, const int32_t* chunks, int nchunks, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training meters (csrc/meters.hip; the reference's per-iteration log, train.py:231-235 and 463-500: loss.item(), IoU(output, masks),
 * precision@X, cumulative I / U, metric_logger.update(loss=, lr=, iou=)) kept on the device: they follow graph replays and are copied out when the
 * host wants to look.  Three new symbols under ABI v7: no existing prototype or struct changed.
 *
 * The meter block: lavt_meter_bytes(capacity) = 8 * LAVT_METER_HEADER_DOUBLES + capacity * LAVT_METER_RECORD_BYTES bytes of device memory, 8-byte
 * aligned, zero-filled by the caller except header[0].  Header: fp64[LAVT_METER_HEADER_DOUBLES] (counts are whole numbers held in fp64):
 *   [0] capacity (host; informational)      [1] hold: written by the HOST only, non-zero = an append does nothing
 *   [2] n: records appended since the block was made = the `it` of the next record          [3] n at the last epoch reset (host)
 *   the epoch accumulators, zeroed by the host's epoch reset:
 *   [4] iterations          [5] sum of the finite losses    [6] their count          [7] non-finite losses (left out of [5])
 *   [8] sum of iou          [9] cumulative I                [10] cumulative U        [11..15] seg_correct: iterations with iou >= .5, .6, .7, .8, .9
 *   [16] applied updates    [17] skipped updates            [18] accumulating micro-steps
 *   [19] sum of lr          [20] sum of the finite gradient norms of the records that ended a cycle    [21] their count    [22..31] reserved, zero
 * Ring: capacity records of LAVT_METER_RECORD_BYTES bytes behind the header, record `it` in slot it % capacity:
 *   offset 0 fp32 loss | 4 fp32 I | 8 fp32 U | 12 fp32 lr | 16 fp32 grad_norm | 20 uint32 flags | 24 fp64 iou | 32 int64 it
 *
 * lavt_meter_append: ONE single-writer launch at the end of an iteration, after the optimizer's tick.  stats: the fp32[4] {loss, sum of weights, I, U} of
 * the fused cross-entropy, or the row of lavt_upsample_iu below for the criteria that do not count I / U ([1] is not read).  ctl: the control block of lavt_grad_norm, or NULL.  step: the optimizer's counter, or NULL.  hyper: the hyper row whose base lr is
 * logged (fp32[5], [0] = base lr), or NULL.  Nothing at all is stored when header[1] != 0 or ctl[4] != 0.  Otherwise the record is
 *   iou  = (I == 0 || U == 0) ? 0 : (double)I / (double)U  (train.py:64-76), seg_correct compares it in fp64 against the double literals;
 *   lr   = hyper[0] * (total_steps > 0 ? powf(fmaxf(1 - step[0] / total_steps, 0), power) : 1) with the counter as the update's tick left it -- the lr
 *          of the NEXT update, what optimizer.param_groups[0]["lr"] holds after lr_scheduler.step(); 0 without step or hyper;
 *   grad_norm = ctl[0], 0 without ctl;     flags: the bits below;     it = header[2];
 * and the accumulators move as listed.  A non-finite loss is counted in [7] and left OUT of [5] (the reference's running sum would stay NaN for the
 * rest of the epoch); the ring keeps the raw value.  Plain stores from one lane, no atomics: launches are ordered on the stream.
 * Flags: ACCUMULATING = ctl[5] != 0 (the micro-step did not end its cycle); SKIPPED = not accumulating and ctl[2] != 0; APPLIED = a step counter was
 * given and neither of the two; LOSS_NONFINITE = the loss is NaN / Inf.  `capacity` must be the block's.
 *
 * lavt_grad_norm_tensors (csrc/optim.hip, with the norm it reads): per-tensor sums of squares from the per-chunk partials lavt_grad_norm's first pass left in ws [nchunks] -- the chunk table
 * lists every tensor's chunks contiguously in ascending order, so tensor t owns ws[first[t] .. first[t + 1]) (first: device int32 [count + 1]).  One
 * launch, one wave per tensor in turn: lane l adds partials l, l + 64, ... in sequence in fp64, a fixed xor tree joins the lanes -- bit-reproducible.
 *   out[t] = the sum (fp64; sqrt gives the norm);   bad: device int32[4] = {first non-finite tensor of this call or -1, how many were non-finite,
 *   first non-finite tensor of the most recent call that had one (sticky: initialise to -1), reserved}.
 * ctl[4] != 0 (hold) or ctl[5] != 0 (accumulating): returns before any store, exactly like lavt_grad_norm (out and bad keep the last cycle's). */
#define LAVT_METER_HEADER_DOUBLES 32
#define LAVT_METER_RECORD_BYTES 40
#define LAVT_METER_APPLIED 1u
#define LAVT_METER_SKIPPED 2u
#define LAVT_METER_ACCUMULATING 4u
#define LAVT_METER_LOSS_NONFINITE 8u
int64_t lavt_meter_bytes(int capacity);
int lavt_meter_append(const float* stats, const float* ctl /* NULL */, const float* step /* NULL */, const float* hyper /* NULL */, float total_steps, float power,
                      void* block, int capacity, void* stream);
int lavt_grad_norm_tensors(const float* ws, int nchunks, const int32_t* first, int count, const float* ctl, double* out, int32_t* bad, void* stream);
/* The hard-mask I / U of a training batch for the criteria whose own statistics do not hold them (csrc/meters.hip; three new symbols under ABI v7).
 * The reference logs IoU(output, masks) in its training loops whatever --loss is (train.py:64-76: pred = output.argmax(1); I = sum(pred * gt);
 * U = sum(pred + gt) - I, pooled over the batch).  lavt_upsample_ce_fwd leaves these counts in out4[2:4]; the `stats` of the two Dice criteria
 * hold soft sums at pinned offsets and no argmax counts, so a metered step of those criteria runs this pass behind the criterion's forward:
 * a fused bilinear upsample (align_corners) + argmax + pooled I / U over the low-resolution 2-class logits x NHWC [B,Hi,Wi,2] (LAVT_F32 / LAVT_BF16),
 * target int64 [n,Ho,Wo] in {0,1}, n = B (or nsel).  Every pixel is computed exactly as the cross-entropy kernel computes it; pred = up1 > up0 (a tie
 * is class 0, as argmax), tgt = (t == 1), I = #(pred && tgt), U = #(pred || tgt) over all samples.
 *   row (device fp32[4]) = {loss_src ? loss_src[0] : 0, 0, I, U} -- exactly the row lavt_meter_append reads as `stats`; loss_src[0] is copied bit for bit.
 * Counted in integers: per wave with ballot + popcount, one int32 pair per workgroup in ws, then a one-workgroup finish that adds the pairs in a fixed
 * order in 64-bit integers and converts each total to fp32 once.  Two launches, no floating-point atomics: identical bits from run to run, the same
 * kernels in deterministic mode.  ws: lavt_upsample_iu_ws(n, Ho, Wo) 32-bit words of scratch (host arithmetic; 0 for n <= 0).
 * _sel: annotated-frame selection as for the criteria (sel DEVICE int32 [nsel], 0 < nsel <= B, read on the device so a replayed graph follows the
 * buffer; sample j reads logits frame sel[j] and target j; an entry outside [0, B) is never dereferenced and adds nothing to I or U).
 * Bad arguments (a null pointer other than loss_src, a non-positive size, nsel outside 1..B, another dtype, ws_words below the query) return
 * LAVT_ERR_INVALID with row untouched. */
int64_t lavt_upsample_iu_ws(int n, int Ho, int Wo);
int lavt_upsample_iu(int dtype, const void* x, const int64_t* target, const float* loss_src /* NULL */, int32_t* ws, int64_t ws_words, float* row, int B, int Hi,
                     int Wi, int Ho, int Wo, void* stream);
int lavt_upsample_iu_sel(int dtype, const void* x, const int32_t* sel, int nsel, const int64_t* target, const float* loss_src /* NULL */, int32_t* ws,
                         int64_t ws_words, float* row, int B, int Hi, int Wi, int Ho, int Wo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation meter (csrc/meters.hip; the reference's evaluation log, test.py:84-108: per-sample IoU, cumulative I / U, precision@X) kept on the
 * device like the training meters: it follows graph replays and is copied out when the host wants to look.  Two new symbols under ABI v7.
 *
 * The block: lavt_eval_meter_bytes(capacity) = 8 * LAVT_EVAL_METER_HEADER_DOUBLES + capacity * LAVT_EVAL_METER_RECORD_BYTES bytes of device memory,
 * 8-byte aligned, zero-filled by the caller except header[0].  Header: fp64[LAVT_EVAL_METER_HEADER_DOUBLES]; counts are whole numbers held in fp64,
 * exact up to 2^53:
 *   [0] capacity (host; informational)      [1] hold: written by the HOST only, non-zero = an append does nothing
 *   [2] n: samples appended since the block was made = the running sample number of the next record
 *   the accumulators, zeroed by the host's reset:
 *   [3] count      [4] sum of iou      [5] cumulative I      [6] cumulative U      [7..11] correct: samples with iou >= .5, .6, .7, .8, .9
 *   [12..15] reserved, zero
 * Ring: capacity records of LAVT_EVAL_METER_RECORD_BYTES bytes behind the header, sample `s` in slot s % capacity:
 *   offset 0 int32 I | 4 int32 U | 8 int64 running sample number
 *
 * lavt_eval_meter_append: ONE single-writer launch behind the mask kernel.  iu: int32 [n][2], the (I, U) rows of lavt_upsample_mask(_pairs).
 * image_of: the pair list's DEVICE int32 [n] with n_images (the image_of contract below), or NULL = every slot is live.  For every live slot in
 * slot order, what EvalMeter.update does for one (I, U) (test.py:84-95):
 *   iou = U == 0 ? 0 : (double)I / (double)U (an fp64 division); count += 1; sum of iou += iou (fp64, in order); cumulative I += I, U += U;
 *   correct[k] += iou >= th_k, compared in fp64 against the double literals .5 .. .9; the record {I, U, header[2]} is stored and header[2] += 1.
 * An empty slot's row of iu is not read.  Nothing at all is stored when header[1] != 0.  `capacity` must be the block's. */
#define LAVT_EVAL_METER_HEADER_DOUBLES 16
#define LAVT_EVAL_METER_RECORD_BYTES 16
int64_t lavt_eval_meter_bytes(int capacity);
int lavt_eval_meter_append(const int32_t* iu, const int32_t* image_of /* NULL: every slot live */, int n_images, int n, void* block, int capacity, void* stream);

/* ---------------------------------------------------------------------------------------------
 * J&F measure (csrc/jf_measure.hip, csrc/meters.hip): the video measure of Refer-YouTube-VOS / Ref-DAVIS -- J, region similarity; F, the boundary
 * F-measure of the DAVIS 2017 evaluation; J&F, their mean -- as the toolkit's db_eval_iou, db_eval_boundary and _seg2bmap compute them WITHOUT void
 * pixels.  The recall and decay statistics of the toolkit are not computed.  Five new symbols under ABI v7.
 *
 * A frame is a predicted mask P and a ground truth G, both H x W, nonzero = foreground.
 *   Region       I = |P and G|, U = |P or G|;  J = 1 if U == 0 (two empty masks agree -- unlike the evaluation meter above), else I / U.
 *   Boundary map b = bmap(S):  e[y,x] = S[y,x+1], s[y,x] = S[y+1,x], se[y,x] = S[y+1,x+1], zero where the source lies outside the frame;
 *                b = (S^e) | (S^s) | (S^se); then the last row is S^e, the last column S^s and the bottom-right pixel 0.
 *   Radius       bound_pix = ceil(0.008 * sqrt(H*H + W*W)) in fp64 is the toolkit's (8 at 480x854, 12 at 720x1280); the caller passes it.
 *   Disk         {(dy,dx) : dy*dy + dx*dx <= r*r};  dil(b)[y,x] = OR of b[y+dy,x+dx] over the disk, positions outside the frame ignored.
 *   Counts       n_fg = |bmap(P)|, n_gt = |bmap(G)|, m_fg = |bmap(P) and dil(bmap(G))|, m_gt = |bmap(G) and dil(bmap(P))|.
 *   F            n_fg == 0 and n_gt > 0: precision 1, recall 0;  n_fg > 0 and n_gt == 0: precision 0, recall 1;  both zero: 1 and 1;
 *                otherwise precision = m_fg / n_fg, recall = m_gt / n_gt.  F = 0 if precision + recall == 0, else ((2.0 * p) * r) / (p + r),
 *                every step one fp64 rounding.
 *   A sequence   one object or expression over its frames: J_seq, F_seq = the sum over its frames in frame order, divided by their number.
 *   Dataset      J, F = the means of J_seq, F_seq over the sequences;  J&F = (J + F) / 2.
 *
 * lavt_boundary_counts: pred uint8 [n][H][W] (the mask of lavt_upsample_mask), and exactly one of target_u8 (uint8) / target_i64 (int64) [n][H][W];
 * nonzero = foreground for all three, whatever the value (255, 7 and 1 << 32 are foreground).  counts int32 [n][8]: row j =
 * {I, U, n_fg, n_gt, m_fg, m_gt, 0, 0} of frame j.  Every call overwrites every row (a zero-fill kernel, then integer atomic adds -- order-independent,
 * no floating point anywhere), so a replayed graph needs nothing from what the buffer held.  Frames adjacent in memory never see each other's pixels.
 * Three kernels (fill, pack, boundary), capturable, no host synchronisation.  ws: lavt_boundary_counts_ws(n, H, W) 64-bit words of scratch (host
 * arithmetic: 2 * n * H * ceil(W / 64), the two masks as bit rows; 0 for a non-positive size), 8-byte aligned.
 * LAVT_ERR_INVALID with counts untouched and nothing launched: a null pred, ws or counts, both or neither target, a non-positive size, bound_pix outside
 * 1 .. LAVT_BOUNDARY_MAX_RADIUS, ws_words below the query.
 *
 * The J&F meter block: lavt_jf_meter_bytes(capacity) = 8 * LAVT_JF_METER_HEADER_DOUBLES + capacity * LAVT_JF_METER_RECORD_BYTES bytes of device
 * memory, 8-byte aligned, zero-filled by the caller except header[0].  Header: fp64[LAVT_JF_METER_HEADER_DOUBLES], counts exact up to 2^53:
 *   [0] capacity (host; informational)      [1] hold: written by the HOST only, non-zero = an append stores nothing
 *   [2] the running sequence number of the next record
 *   the accumulators, zeroed by the host's reset:
 *   [3] sequences      [4] sum of J_seq      [5] sum of F_seq      [6] frames      [7] sum of J over frames      [8] sum of F over frames
 *   [9..15] reserved, zero
 * Ring: capacity records of LAVT_JF_METER_RECORD_BYTES bytes behind the header, sequence `q` in slot q % capacity:
 *   offset 0 int32 frames | 4 int32 0 | 8 fp64 J_seq | 16 fp64 F_seq | 24 int64 running sequence number
 *
 * lavt_jf_meter_append: ONE single-writer launch behind the counts.  n must be a multiple of frames_per_seq; sequence k is the frames
 * k*T .. k*T + T - 1, taken in ascending order.  live: device int32 [n], live[j] == 0 = frame j is not read; NULL = every frame is live.  Inside a
 * sequence the live frames are taken in ascending order with the arithmetic above in fp64; [6], [7], [8] move with every live frame; a sequence
 * with no live frame stores nothing.  `capacity` must be the block's. */
#define LAVT_BOUNDARY_MAX_RADIUS 40
#define LAVT_JF_METER_HEADER_DOUBLES 16
#define LAVT_JF_METER_RECORD_BYTES 32
int64_t lavt_boundary_counts_ws(int n, int H, int W);
int lavt_boundary_counts(const uint8_t* pred, const uint8_t* target_u8, const int64_t* target_i64, int n, int H, int W, int bound_pix, uint64_t* ws,
                         int64_t ws_words, int32_t* counts /* [n][8] */, void* stream);
int64_t lavt_jf_meter_bytes(int capacity);
int lavt_jf_meter_append(const int32_t* counts, const int32_t* live /* NULL: every frame */, int n, int frames_per_seq, void* block, int capacity, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Inference path (csrc/infer.hip; reference test.py:60-110 and test_ytvos.py:230-260: batch-1 forward under model.eval() / torch.no_grad(), argmax,
 * I / U).  New symbols only, added under ABI v7: no existing prototype or struct changed.
 *
 * lavt_conv_bn_fold: an eval-mode BatchNorm folded into the convolution in front of it (lib/mask_predictor.py:61-66 and the five sibling
 *   conv -> bn -> relu triples under eval()).  In fp32: s[co] = gamma[co] / sqrt(running_var[co] + eps);
 *   w_packed[co][tap][ci] = dtype(w[co][ci][tap] * s[co]) -- the [Cout][taps][Cin] layout of lavt_pack_conv3x3 --
 *   and bias[co] (fp32) = beta[co] - running_mean[co] * s[co].  gamma / beta NULL = 1 / 0.  dtype (of w_packed): LAVT_F32 or LAVT_BF16.
 * lavt_splitk_reduce_epi: lavt_splitk_reduce (same partial layout, same summation order) with out = act(sum + bias[n]) before the store;
 *   bias fp32 [N] or NULL, act = LAVT_ACT_NONE / GELU / RELU / TANH.  With it a split-K convolution carries the folded BatchNorm + ReLU;
 *   bias NULL and LAVT_ACT_NONE store the bytes lavt_splitk_reduce stores.
 * lavt_upsample_mask: the final upsample fused with the caller's argmax(1) and pixel counts (lib/_utils.py:21 + test.py:81-83, 242-246):
 *   x = decoder logit rows [B*Hi*Wi][2] (dtype); mask uint8 [B][Ho][Wo] = (v1 > v0), a tie gives 0 as argmax does, where v is the bilinear
 *   align_corners=True interpolation in fp32 with the coordinate arithmetic of lavt_logits_up_fwd.  Hm = Wm = 0: one interpolation
 *   (Hi, Wi) -> (Ho, Wo); otherwise the composition (Hi, Wi) -> (Hm, Wm) -> (Ho, Wo) of test_ytvos.py:249-253 (the model's own upsample to the
 *   network input size, then the caller's to the original frame size): the four corners on the intermediate grid are interpolated themselves,
 *   no intermediate map is written.  target (optional) int64 [B][Ho][Wo], nonzero = foreground; with it iu int32 [B][2] receives
 *   += sum(pred & gt), += sum(pred | gt) per sample through integer atomics: the CALLER zeroes iu in front of every launch. */
int lavt_conv_bn_fold(const float* w, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int dtype,
                      void* w_packed, float* bias, int Cout, int Cin, int taps, void* stream);
int lavt_splitk_reduce_epi(int dtype, const float* parts, int splits, int64_t M, int N, const float* bias, int act, void* out, int64_t ldc, void* stream);
int lavt_upsample_mask(int dtype, const void* x, int B, int Hi, int Wi, int Hm, int Wm, int Ho, int Wo, uint8_t* mask, const int64_t* target, int32_t* iu,
                       void* stream);
/* Pair-list prediction batches.  A batch is a list of n pairs (image, expression): the network holds n_images images and n expressions, and a DEVICE
 * int32 [n] buffer image_of names the image of every slot (lavt_gather_samples repeats stage 0's rows by it; everything behind runs on n samples).
 * Contract for image_of, next to the contract for sel above: n may be smaller than, equal to or larger than n_images; entries may repeat; an entry
 * outside [0, n_images) -- canonically -1 -- marks an EMPTY slot, so the last batch of a dataset replays the graph of a full one.  The kernels read
 * image_of on the device, so a replayed graph follows a changed buffer, and therefore they cannot raise: an empty slot is gathered as zeros, the
 * network runs on those and on whatever language the slot holds, and its logits (possibly NaN) are never read for a decision.  Range is checked on
 * the host where the entries arrive from the host (lavt_hip.engine: Predictor.set_image_of).
 * lavt_upsample_mask_pairs: lavt_upsample_mask with B = n slots and that buffer.  A live slot's mask bytes and iu row are those lavt_upsample_mask
 * stores for the same logit rows; an empty slot's mask is all zero and it adds nothing to iu, so its row stays what the caller's fill left: (0, 0). */
int lavt_upsample_mask_pairs(int dtype, const void* x, int B, int Hi, int Wi, int Hm, int Wm, int Ho, int Wo, uint8_t* mask, const int64_t* target, int32_t* iu,
                             const int32_t* image_of, int n_images, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame preprocessing (csrc/preprocess.hip; replaces the host-side transforms.py:20-31 (Resize), 83-87 (ToTensor), 106-113 (Normalize) and the
 * per-frame loop of test_ytvos.py:236-243 for frames that are on the device as uint8).  New symbols only, added under ABI v7.
 *
 * lavt_resize_norm_u8: N uint8 HWC RGB frames of Hs x Ws, frame f at src + f * frame_stride (elements = bytes; >= Hs * Ws * 3, so the frames may be
 *   a slice of a larger upload), -> out fp32 [N][3][Ho][Wo].  The resize is PIL's bilinear (antialiased) resample of 8-bit data, applied by ITS
 *   fixed-point tables, which the caller builds (lavt_hip/preprocess.py: resample_tables) and passes per axis: coef int32 [out][ksize] and bounds
 *   int32 [out][2] = (first source index, tap count), in device memory.  Width first, rounded to uint8, then height, each as
 *   clip((2^21 + sum_k coef[k] * pix[first + k]) >> 22, 0, 255); then ((v / 255.f) - mean[c]) / std[c] in these three fp32 operations.
 *   bounds_y_host is the bounds_y table in HOST memory: from it the entry picks the tile height TH (the largest of 16, 8, 4, 2, 1 whose source-row
 *   span keeps the tile's LDS request, 192 bytes per source row, within 64 KB) without reading device memory; LAVT_ERR_INVALID when a single output
 *   row does not fit (beyond ~170x downscale) or the table is not a non-decreasing sequence of row ranges inside the source.  One launch; N <= 65535.
 * lavt_resize_nearest_u8: N uint8 single-channel masks (mask f at src + f * frame_stride, >= Hs * Ws) -> out int64 [N][Ho][Wo] =
 *   src[idx_y[y]][idx_x[x]]: PIL's NEAREST with the caller's index tables (int32 [Ho], [Wo], device memory; lavt_hip/preprocess.py: nearest_table). */
int lavt_resize_norm_u8(const uint8_t* src, int64_t frame_stride, int N, int Hs, int Ws, const int32_t* coef_x, const int32_t* bounds_x, int ksize_x,
                        const int32_t* coef_y, const int32_t* bounds_y, int ksize_y, const int32_t* bounds_y_host, float* out, int Ho, int Wo,
                        float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream);
int lavt_resize_nearest_u8(const uint8_t* src, int64_t frame_stride, int N, int Hs, int Ws, const int32_t* idx_y, const int32_t* idx_x, int64_t* out, int Ho,
                           int Wo, void* stream);

/* Batched form for sources of MIXED sizes (a training batch of RefCOCO / COCO images; lavt_hip/preprocess.py: pack_batch, BatchPreprocessor): one
 * launch for all output frames.  New symbols only, added under ABI v7.
 *
 * lavt_pp_item_t: one descriptor per OUTPUT frame, 64 bytes.  An image descriptor names its source (src_off: byte offset of an Hs x Ws x 3 HWC
 *   image in the pixel buffer; any alignment) and its four tables as ELEMENT offsets into one int32 table buffer: coef_x [Wo][ksize_x],
 *   bounds_x [Wo][2], coef_y [Ho][ksize_y], bounds_y [Ho][2] (the tables of lavt_resize_norm_u8).  A target descriptor names its mask (mask_off:
 *   byte offset of an Hs x Ws mask in the mask buffer) and its nearest-index tables idx_y [Ho], idx_x [Wo].  Fields a launch does not use are
 *   ignored by it.  Several descriptors may name the same source and the same tables; their order is free (output frame i = descriptor i).
 * lavt_resize_norm_u8_batch: n image descriptors -> out fp32 [n][3][Ho][Wo], the arithmetic of lavt_resize_norm_u8.  items / tables / pixels are
 *   device memory; items_host / tables_host are the same descriptors and tables in HOST memory (they are packed there).  From the host copy the
 *   entry checks, before launching: 1 <= n <= 65535; every source lies inside pixel_bytes; every table lies inside table_elems; ksize > 0; every
 *   bounds row is a tap range inside its source (0 <= first, 0 <= taps <= ksize, first + taps <= size); bounds_y is non-decreasing in first and in
 *   first + taps.  It picks ONE tile height for the launch, the largest of 16, 8, 4, 2, 1 whose worst source-row span over all items keeps the LDS
 *   request (192 bytes per source row) within 64 KB.  LAVT_ERR_INVALID with a message, and no launch, when any check fails or a single output row of
 *   some item does not fit.  The kernel repeats the range checks on what it reads from device memory: a descriptor or table that does not belong
 *   causes no read outside the buffers and no write.
 * lavt_resize_nearest_u8_batch: n target descriptors -> out int64 [n][Ho][Wo] = mask[idx_y[y]][idx_x[x]].  Checked from the host copy: n >= 1,
 *   every mask inside mask_bytes, every table inside table_elems, every index inside its mask. */
typedef struct lavt_pp_item {
    int64_t src_off, mask_off;
    int32_t Hs, Ws;
    int32_t coef_x, bounds_x, ksize_x;
    int32_t coef_y, bounds_y, ksize_y;
    int32_t idx_y, idx_x;
    int32_t reserved0, reserved1;
} lavt_pp_item_t;
int lavt_resize_norm_u8_batch(const lavt_pp_item_t* items, const lavt_pp_item_t* items_host, int n, const int32_t* tables, const int32_t* tables_host,
                              int64_t table_elems, const uint8_t* pixels, int64_t pixel_bytes, float* out, int Ho, int Wo, float mean0, float mean1,
                              float mean2, float std0, float std1, float std2, void* stream);
int lavt_resize_nearest_u8_batch(const lavt_pp_item_t* items, const lavt_pp_item_t* items_host, int n, const int32_t* tables, const int32_t* tables_host,
                                 int64_t table_elems, const uint8_t* masks, int64_t mask_bytes, int64_t* out, int Ho, int Wo, void* stream);

/* Pseudo-video augmentation (`--pseudo_video_aug weak-rotate-translate-shear-crop`, args.py:132-137): affine warps of uint8 sources into uint8 frames
 * of the same size, which the batched resize entries above then read.  New symbols only, added under ABI v7.  The contract is Pillow's, pixel for
 * pixel: `Image.transform((Ws, Hs), Image.AFFINE, a, resample=BILINEAR)` for RGB, `resample=NEAREST` for masks, both with fill 0.
 *
 * lavt_pp_warp_t: one descriptor per WARPED frame, 128 bytes.  src_off / dst_off: byte offsets of the Hs x Ws (x 3) source in `src` and of the
 *   warped frame of the same size in `dst`; any alignment; several descriptors may name one source, destinations must not overlap (not checked).
 *   a[6]: Pillow's coefficients, output pixel (x, y) reads the source at (a0 (x + .5) + a1 (y + .5) + a2, a3 (x + .5) + a4 (y + .5) + a5).
 *   The image entry reads a only; the mask entry reads, by `mode`,
 *     LAVT_WARP_FIXED: A[6], Pillow's 16.16 fixed-point form of a (A0, A1, A3, A4 = floor(a * 65536 + .5); A2, A5 = the same of a2 + a0 / 2 + a1 / 2,
 *       a5 + a3 / 2 + a4 / 2): out[y][x] = src[(A5 + A4 y + A3 x) >> 16][(A2 + A1 y + A0 x) >> 16] where that lies inside, else 0;
 *     LAVT_WARP_TABLES (what Pillow does when a1 == 0 and a3 == 0): idx_x [Ws], idx_y [Hs], element offsets into the int32 table buffer:
 *       out[y][x] = src[idx_y[y]][idx_x[x]], an index of -1 = outside = 0 (lavt_hip/preprocess.py: warp_axis_table builds them as Pillow does,
 *       by repeated fp64 addition).
 * lavt_affine_u8_batch: n descriptors, RGB bilinear in fp64 without contraction, the operations of Pillow's bilinear filter in its order; the result is
 *   truncated to uint8.  warps is device memory, warps_host the same descriptors in HOST memory.  Checked from the host copy before launching:
 *   1 <= n <= 65535, 1 <= Hs, Ws <= 8192, every source inside src_bytes and every destination inside dst_bytes, every coefficient finite.
 * lavt_affine_nearest_u8_batch: n descriptors, single-channel nearest.  Checked as above (a is not read), and: mode is one of the two; FIXED: the
 *   fixed-point coordinates at the four corners (0, 0), (Ws, 0), (0, Hs), (Ws, Hs) fit int32 (where Pillow's own `int` would overflow); TABLES: both
 *   tables inside table_elems, every entry in [-1, size).  tables / tables_host may be null when table_elems is 0 and no descriptor is TABLES.
 * LAVT_ERR_INVALID with a message, and no launch, when a check fails.  The kernels repeat the range checks on what they read from device memory: a
 * descriptor or table that does not belong causes no read outside the buffers and no write. */
#define LAVT_WARP_FIXED 0
#define LAVT_WARP_TABLES 1
typedef struct lavt_pp_warp {
    int64_t src_off, dst_off;
    int32_t Hs, Ws;
    int32_t mode, idx_x, idx_y, reserved0;
    double a[6];
    int32_t A[6];
    int32_t reserved1[4];
} lavt_pp_warp_t;
int lavt_affine_u8_batch(const lavt_pp_warp_t* warps, const lavt_pp_warp_t* warps_host, int n, const uint8_t* src, int64_t src_bytes, uint8_t* dst,
                         int64_t dst_bytes, void* stream);
int lavt_affine_nearest_u8_batch(const lavt_pp_warp_t* warps, const lavt_pp_warp_t* warps_host, int n, const int32_t* tables, const int32_t* tables_host,
                                 int64_t table_elems, const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Text side (lavt_one / lavt_video carry BERT inside the model: lib/_utils.py:38-52; train.py:595-602; the encoder is HF transformers
 * 3.0.2 `BertModel`, absent from the reference tree).  Its Linear / LayerNorm / GELU / attention GEMMs use the entry points above.
 * lavt_bert_embed_fwd: out[r] = word[ids[r]] + type[token_type ? token_type[r] : 0] + pos[r % N]  (BertEmbeddings.forward before LayerNorm;
 *   ids / token_type int64 [rows], tables fp32, out [rows][H] in `dtype`).  lavt_bert_embed_bwd scatter-adds dy into the three fp32 table
 *   gradients (atomics; the buffers must hold the running sums, e.g. zeros).
 * lavt_dropout: y = (keep ? x * scale : 0) + residual (nn.Dropout in training with a caller-drawn uint8 keep mask, scale = 1/(1-p); residual
 *   optional: the `dropout(dense(h)) + input` of BertSelfOutput / BertOutput); without residual it is its own backward. */
int lavt_bert_embed_fwd(int dtype, const int64_t* ids, const int64_t* token_type, const float* word, const float* pos, const float* type,
                        void* out, int rows, int N, int H, void* stream);
int lavt_bert_embed_bwd(int dtype, const void* dy, const int64_t* ids, const int64_t* token_type, float* dword, float* dpos, float* dtype_,
                        int rows, int N, int H, void* stream);
int lavt_dropout(int dtype, const void* x, const uint8_t* keep, float scale, const void* residual, void* y, int64_t n, void* stream);

/* Sentence attention: the BertSelfAttention core, softmax(q k^T / sqrt(hd) + keybias) -> dropout -> . v, fused for sentence-length sequences (new
 * symbols only: no existing prototype or struct changed, lavt_abi_version() stays 7).
 *   qkv      token-major [B*N][3H] in `dtype` (LAVT_BF16 / LAVT_F32), columns q | k | v, each heads x hd: the output of one GEMM over the stacked
 *            query / key / value weights, read as it is (no head-major copy)
 *   keybias  fp32 [B][N] = (1 - attention_mask) * -10000: a masked key is biased by -10000, not -inf, so a fully masked row is uniform over its keys
 *            (HF's behaviour); rows of padded QUERY tokens are computed like any other
 *   keep     uint8 [B][heads][N][N], the dropout keep mask of the probabilities (drawn by the caller), or NULL for no dropout; drop_scale = 1 / (1 - p)
 *            multiplies the kept ones (ignored when keep is NULL; keep of all ones with drop_scale 1 gives the bits of NULL)
 * lavt_sentence_attn_fwd writes out [B*N][H] token-major in `dtype` and nothing else (no probabilities, no scratch).
 * lavt_sentence_attn_bwd takes the same qkv / keybias / keep and dout [B*N][H], recomputes the probabilities with the forward's own arithmetic and
 *   writes EVERY element of dqkv [B*N][3H] in `dtype`.
 * One workgroup per (sample, head) with all its operands in LDS as fp32; fp32 accumulation in index order, one rounding to `dtype` at the store; no
 * atomics, no reduction across workgroups: the same bits on every run, so the kernels are their own deterministic form.
 * Geometry: hd == 64 and 1 <= N <= 64; anything else is LAVT_ERR_INVALID with a message and no launch (the caller keeps its composed route:
 * lavt_gemm_nt / lavt_attn_softmax_* / lavt_gemm_tn).  The backward asks for up to 99,072 bytes of LDS (N = 64). */
int lavt_sentence_attn_fwd(int dtype, const void* qkv, const float* keybias, const uint8_t* keep, float drop_scale, void* out, int B, int N, int heads,
                           int hd, void* stream);
int lavt_sentence_attn_bwd(int dtype, const void* qkv, const float* keybias, const uint8_t* keep, float drop_scale, const void* dout, void* dqkv, int B,
                           int N, int heads, int hd, void* stream);

/* The opening of the encoder in inference as one launch (DESIGN.md "Text encoder in the prediction"; a new symbol only: no existing prototype or
 * struct changed, lavt_abi_version() stays 7).  What lavt_bert_embed_fwd + lavt_layernorm_fwd + the three element-wise steps of
 * `(1.0 - attention_mask.float()) * -10000.0` compute, without the rounding to `dtype` between the embedding sum and the LayerNorm:
 *   out[r]     = dtype(LayerNorm((word[ids[r]] + type[token_type ? token_type[r] : 0]) + pos[r % N]) * gamma + beta)      [rows][H], LAVT_F32 / LAVT_BF16
 *   keybias[r] = (1.f - (float)attn_mask[r]) * -10000.f                                                                    fp32 [rows]
 * ids / token_type / attn_mask int64 [rows]; tables, gamma, beta fp32.  The sum is formed in BertEmbeddings.forward's order and stays fp32; the
 * statistics are two-pass in fp32 (the mean, then the mean of squared deviations ABOUT it -- never E[x^2] - mean^2: BERT's eps is 1e-12 and its rows
 * are not centred); one rounding to `dtype`, at the store.  keybias is evaluated literally, so it holds the bits of the torch expression for any
 * integer mask; token_type NULL = type 0 everywhere; attn_mask and keybias are both given or both NULL.
 * The kernel cannot raise and reads nothing outside its tables: an id outside [0, vocab) reads word row 0 (the pad row), a type outside
 * [0, n_types) reads type row 0, and r % N lies inside [0, n_pos) because the entry refuses N > n_pos.  Range checks with a message belong to the
 * host, where the values come from the host (lavt_hip.engine.check_sentences).
 * A wave per row holding its H / 64 elements in registers between the passes; no LDS, no atomics, no scratch: the same bits on every run.
 * LAVT_ERR_INVALID with a message and no launch: a null pointer (token_type and the attn_mask / keybias pair excepted), rows / N / H or a table's
 * row count <= 0, H % 4 != 0, H > 2048, N > n_pos, keybias without attn_mask or the reverse, a dtype other than LAVT_F32 / LAVT_BF16. */
int lavt_bert_embed_ln_fwd(int dtype, const int64_t* ids, const int64_t* token_type, const int64_t* attn_mask, const float* word, const float* pos,
                           const float* type, const float* gamma, const float* beta, float eps, void* out, float* keybias, int rows, int N, int H,
                           int vocab, int n_pos, int n_types, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Deterministic forms (DESIGN.md "Deterministic mode"; new symbols only: no existing prototype or struct changed, lavt_abi_version() stays 7).
 * Every entry point below computes what its sibling above computes WITHOUT float atomics: the same bits on every run from the same inputs.  The
 * library keeps no mode: the host calls these instead of the siblings (lavt_hip.ops.deterministic()).  The weight-gradient GEMMs need no new entry
 * point: a caller that lends `partials` to every launch that may split, or asks for split_k = 1, never reaches their atomic branches (one addend
 * per output element; a colsum_atomic vector shared by exactly two members of a launch receives 0 + a + b, which does not depend on the order).
 * lavt_reduce_partials_det: partials [nblk][W] (W = groups * 2 * C: per group C "sum-1" values, then C "sum-2" values) are ADDED into o1 / o2 [groups][C].
 *   Two-level: the row slices of the atomic form store their sums to `stage` (lavt_reduce_partials_det_stage(W) floats), a second launch adds them in
 *   slice order.  stage NULL / too small: one slice walks all rows.  lavt_layernorm_bwd_partial(_xn) / lavt_cls_head_bwd_partial + this call replace
 *   lavt_layernorm_bwd(_xn) / lavt_cls_head_bwd.
 * lavt_reduce_partials_multi_det: lavt_reduce_partials_multi's compact launch (n <= 64 sets, total_column_blocks as there) with the eight row slices of
 *   every column block stored to stage (>= total_column_blocks * 8 * 128 floats) and added in slice order by a second launch.
 * lavt_norm_bwd_stats_det: lavt_norm_bwd_stats with scratch REQUIRED (the block sums) and reduced as lavt_reduce_partials_det does; with
 *   lavt_reduce_partials_det_stage(groups * 2 * C) floats more in ws the reduction is two-level.
 * lavt_window_attn_bwd_det: lavt_window_attn_bwd's arguments; ws of lavt_window_attn_bwd_det_ws floats is REQUIRED.  bf16 MFMA path: the table gradient
 *   is GATHERED -- one thread per (table entry, head) walks the query rows in ascending order, takes the one key whose offset is its entry and sums the
 *   slab values over the windows in window order; the per-workgroup records (same count and layout as the histogram form: lavt_window_attn_bwd_pieces)
 *   are added in record order by one thread per entry (dtable), or left in parts for lavt_attn_dtable_finish_multi.  Exact-fp32 kernel: dS goes to
 *   per-(window, head) fp32 slabs, summed over the windows (lavt_attn_dbias_sum's kernel) and binned (lavt_relpos_reduce's); the waves of a workgroup add
 *   their dK / dV tiles in wave order; no deferred (parts) form.
 * lavt_bert_embed_bwd_det: lavt_bert_embed_bwd with one writer per target row: the first token row that names a word / position / type row adds the dy
 *   rows of all token rows naming it, in ascending row order, to that row's running sum.
 * lavt_gemm_tn_v2_eligible: 1 when lavt_gemm_tn runs the problem on the bf16 LDS-DMA kernels, the ones that honour `partials`; a query, nothing is launched. */
int lavt_gemm_tn_v2_eligible(const lavt_gemm_tn_t* p);
int64_t lavt_reduce_partials_det_stage(int W);
int lavt_reduce_partials_det(const float* partials, int nblk, int W, int C, float* o1, float* o2, float* stage, int64_t stage_floats, void* stream);
int lavt_reduce_partials_multi_det(const int64_t* desc, int n, int total_column_blocks, float* stage, int64_t stage_floats, void* stream);
int lavt_norm_bwd_stats_det(int dtype, const void* dy, const void* x, const void* y, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, const void* mul, int relu, float* s1, float* s2,
                            float* ws, int64_t ws_floats, int groups, int rows, int C, void* stream);
int64_t lavt_window_attn_bwd_det_ws(int dtype, int nwin, int N, int heads, int bias_ld, int wd, int wh, int ww);
int lavt_window_attn_bwd_det(int dtype, const void* qkv, const float* bias, int bias_ld, const int8_t* region, int nw_img,
                             const void* out, const void* dout, const float* lse, void* dqkv, const float* table, float* dtable,
                             float* ws, int64_t ws_floats, float* parts, int wd, int wh, int ww, int nwin, int N, int heads, int head_dim, float scale,
                             void* stream);
int lavt_bert_embed_bwd_det(int dtype, const void* dy, const int64_t* ids, const int64_t* token_type, float* dword, float* dpos, float* dtype_,
                            int rows, int N, int H, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LAVT_HIP_H */
