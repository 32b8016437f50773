/*
 * reid_hip.h -- C-ABI of libreid_hip.so, the MI355X (gfx950) kernels of the
 * PRCV2025REID hot path.
 *
 * The reference (LingmaFuture/PRCV2025REID) is pure Python on PyTorch and has no
 * FFI of its own; every entry point below therefore cites the
 * reference *Python* code whose arithmetic it replaces.  The boundary a user of
 * the reference sees is the Python surface in prcv2025reid_amd/model.py, which
 * calls these functions through ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative reid_status otherwise;
 *     reid_last_error() returns a thread-local message for the last failure;
 *   - all pointers are DEVICE pointers unless named host_*; nothing is allocated
 *     or synchronised inside a call; `stream` is a hipStream_t passed as void*;
 *   - matrices are row-major with explicit leading dimensions in ELEMENTS;
 *   - bf16 = upper 16 bits of IEEE fp32 (round-to-nearest-even on conversion).
 */
#ifndef REID_HIP_H
#define REID_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    REID_OK = 0,
    REID_ERR_ARG = -1,      /* bad shape / null pointer / unsupported size */
    REID_ERR_LAUNCH = -2,   /* hipLaunch / hipGetLastError failed          */
    REID_ERR_DEVICE = -3    /* not a gfx950 device                         */
} reid_status;

/* REID_BF16 = the 16-bit format of the library flavor (see reid_flavor); REID_F16 = IEEE half WHATEVER the flavor, with saturating
 * conversion (a finite value beyond +-65504 is stored as +-65504): accepted only where an entry point says so -- for tensors that are
 * not MFMA operands, where half's 11 significant bits cost nothing (the residual-branch output between a GEMM and the add + LayerNorm). */
typedef enum { REID_BF16 = 0, REID_F32 = 1, REID_F16 = 2 } reid_dtype;

typedef enum {
    REID_ACT_NONE = 0,
    REID_ACT_GELU_ERF = 1,    /* nn.GELU() exact, models/mer_lora.py:257             */
    REID_ACT_QUICK_GELU = 2,  /* HF CLIP text MLP x*sigmoid(1.702x)                   */
    REID_ACT_RELU = 3,        /* models/model.py:42                                   */
    REID_ACT_DGELU_ERF = 4,   /* out = acc * gelu'(aux)        (backward of 1)        */
    REID_ACT_DQUICK_GELU = 5, /* out = acc * quick_gelu'(aux)  (backward of 2)        */
    REID_ACT_DRELU = 6,       /* out = acc * (aux > 0)                                */
    REID_ACT_MUL_AUX = 7,     /* out = acc * aux               (backward of 8: aux = the saved derivative)          */
    REID_ACT_GELU_ERF_DSAVE = 8 /* out = gelu(acc), C2 = gelu'(acc) instead of the pre-activation: the backward
                                 * product is then one multiply per element (7) instead of erfc + exp            */
} reid_act;

const char* reid_last_error(void);
/* ABI version of this header: REID_ABI_VERSION.  201: reid_layernorm_bwd gained `overflow`; r04's positional y_dtype of
 * reid_add_layernorm_fwd, dx_dtype of reid_layernorm_bwd and REID_F16 came without a bump of 200.  Bindings refuse any other value. */
#define REID_ABI_VERSION 201
int reid_version(void);
/* 16-bit operand format of this build: 0 = bf16 (libreid_hip.so), 1 = IEEE f16 (libreid_hip_f16.so, same sources
 * compiled with -DREID_FLAVOR_F16).  Every `bf16` / REID_BF16 in this header means "the 16-bit format of the flavor". */
int reid_flavor(void);
/* Checks that device `dev` is gfx950 (MI355X).  */
int reid_check_device(int dev);
/* Knobs that force a kernel form (tests, tools/ and the A/B harnesses only; the product path never calls this): sets the
 * cached value of knob `name` = the REID_<name> environment variable, which is read ONCE per process; value -1 restores
 * "not set" (the built-in default).  The knobs: "GEMM_TILE" (3 = the 128 x 128 tile, 12 / 14 = the 256 / 224-row ping-pong
 * tile), "ATTN_BWD" (1 = the two-kernel backward), "LORA_IMPL" (1 = the slab kernel), "LN_IMPL" (1 = the four-column
 * LayerNorm backward), "TOPK_TILE" (9 = select_kernel for phase C), "TOPK_SCAN" (0 = the tiled filter instead of the
 * query-resident scan), "LORA_SPAN" (1, 2, 4, 8 = images per workgroup of the adapter-gradient image kernels).  Any other name:
 * REID_ERR_ARG. */
int reid_set_knob(const char* name, int value);

/* ------------------------------------------------------------------------------------------
 * MER GEMM:  C = epilogue( A . B^T  +  A2 . B2^T + bias )      bf16 MFMA, fp32 accumulate
 *
 * Replaces MERLinear.forward (models/mer_lora.py:80-99: shared_linear(x) + lora_B(lora_A(x))*s)
 * and, with A2 = NULL, every plain nn.Linear on the path (models/clip_backbone.py:284,311;
 * HF CLIP text q/k/v/out/fc1/fc2) and their dX backward products.
 *   A  [M, K]  bf16 activations          B  [N, K]  bf16 weight (nn.Linear layout)
 *   A2 [M, *]  bf16 low-rank activations B2 [N, K2] bf16 (scaled LoRA up-projection)
 *   The low-rank pair extends the K loop by K2 (multiple of 32) columns.  With
 *   k2_group_n > 0 output columns [g*k2_group_n, (g+1)*k2_group_n) read A2 columns
 *   [g*K2, (g+1)*K2)  (fused q|k|v projection: one adapter set per projection).
 * Epilogue, in order: + bias[n]; + R (residual, r_dtype; row index m, or m % r_period when
 *   r_period > 0, e.g. the position embedding of models/clip_backbone.py:273); C2 = value
 *   (pre-activation, optional); activation `act` (for the D* forms `aux` [M, ldaux] bf16 holds
 *   the saved pre-activation); row-modality mask (mask_r > 0: column c is kept only if
 *   (c % K_mask_period)/mask_r == img_mod[m / rows_per_img], the LoRA routing of
 *   mer_lora.py:96 for a batch that mixes modalities); * alpha; store as c_dtype at row
 *   (m / c_group) * c_group_stride + m % c_group + c_row_off when c_group > 0 (patch rows ->
 *   token rows behind the CLS slot, models/clip_backbone.py:269-270), else row m.  alpha == 0 is taken as 1 (a zero-filled
 *   argument struct multiplies by nothing).
 * Requirements: K % 64 == 0 (other K are refused), K2 % 32 == 0, N % 4 == 0, 16-byte aligned rows.
 * ------------------------------------------------------------------------------------------ */
#define REID_GEMM_MAX_GROUPS 8
typedef struct {
    const void* A; const void* B; const void* A2; const void* B2;
    const float* bias;
    const void* R; const void* aux;
    void* C; void* C2;
    const int32_t* img_mod;
    int32_t M, N, K, K2;
    int32_t lda, ldb, lda2, ldb2, ldr, ldaux, ldc, ldc2;
    int32_t k2_group_n;
    int32_t act, c_dtype, c2_dtype, r_dtype;
    int32_t r_period;
    int32_t mask_r, mask_period, rows_per_img;
    int32_t c_group, c_group_stride, c_row_off;
    float alpha;
    const float* row_scale;   /* optional f32 [rows / rows_per_img]: out = R + row_scale[row / rows_per_img] * (A.B^T + bias)  (DropPath,
                                 clip_backbone.py:137-141: per-sample branch scale 0 or 1/keep); NULL = 1 */
    /* Row groups (MERLinear routing of mer_lora.py:80-99 for a batch packed modality by modality): with n_row_groups > 0 the rows
     * [row_group_end[g-1], row_group_end[g]) (row_group_end[-1] = 0; the last end must equal M) use weight matrix number
     * row_group_b[g] of a stack: B + row_group_b[g] * b_group_stride (16-bit elements).  The stack holds the MERGED weights
     * W + (alpha/r) B_mu A_mu of each modality (reid_merge_lora), so shared_linear(x) + lora_B(lora_A(x)) * s is ONE GEMM without
     * a K extension.  Row tiles never straddle two groups. */
    int32_t n_row_groups;
    int32_t row_group_end[REID_GEMM_MAX_GROUPS];
    int32_t row_group_b[REID_GEMM_MAX_GROUPS];
    int64_t b_group_stride;
} reid_gemm_args;
int reid_mer_gemm(const reid_gemm_args* host_args, void* stream);

/* The launch reid_mer_gemm chooses, as data: the one host-side statement of the dispatch (csrc/gemm.hip make_plan), which the
 * launcher executes and the tests query. */
typedef enum { REID_GEMM_TILED = 0, REID_GEMM_PP = 1, REID_GEMM_PPS = 2 } reid_gemm_kernel;
typedef enum {
    REID_EPI_GENERIC = 0,   /* every option evaluated at run time */
    REID_EPI_PLAIN16 = 1, REID_EPI_RES32 = 2, REID_EPI_GELU2 = 3, REID_EPI_DGELU = 4, REID_EPI_GELU2D = 5, REID_EPI_MULAUX = 6,
    REID_EPI_PLAIN16H = 7   /* the plain 16-bit store in IEEE half (bf16 flavor only) */
} reid_gemm_epilogue;
typedef struct reid_gemm_plan {
    int32_t kernel;            /* REID_GEMM_TILED: one tile per workgroup (mer_gemm_kernel); REID_GEMM_PP: ping-pong tile; REID_GEMM_PPS: persistent ping-pong */
    int32_t bm, bn;            /* tile */
    int32_t epilogue;          /* REID_EPI_* */
    int32_t tiles_m, tiles_n;  /* row tiles (summed over row groups) and column tiles */
    int32_t grid;              /* workgroups launched */
} reid_gemm_plan;
/* What reid_mer_gemm would launch for *a on a device of `cus` compute units with GEMM_TILE = tile_knob (<= 0: not set).
 * Checks the arguments exactly as reid_mer_gemm does (same return codes and messages), launches nothing, touches no device.
 * cus <= 0: the current device's count. */
int reid_mer_gemm_plan(const reid_gemm_args* a, int32_t cus, int32_t tile_knob, reid_gemm_plan* out);

/* ------------------------------------------------------------------------------------------
 * Reduce-over-rows GEMM:  C[P, Q] = beta*C + alpha * X[M, P]^T . Y[M, Q]   (fp32 out)
 * Weight-gradient products of the backward pass: dB = dY^T T and dA = U^T X for LoRA
 * (autograd of models/mer_lora.py:48), dW = dY^T X for unfrozen linears.
 * X, Y bf16; partial sums over row slabs are combined with fp32 atomics (C must hold
 * beta*C on entry; this call zero-fills C itself when beta == 0).
 * ------------------------------------------------------------------------------------------ */
int reid_gemm_tn(const void* X, const void* Y, float* C, int32_t M, int32_t P, int32_t Q,
                 int32_t ldx, int32_t ldy, int32_t ldc, float alpha, float beta, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (eps 1e-5; models/clip_backbone.py:35-36,73-75,82,210,280).
 *   fwd: y = (x-mean)*rstd*gamma+beta; x f32 [rows, ld]; y bf16 and/or f32; saves mean/rstd.
 *        row_index != NULL gathers x rows (CLS rows, clip_backbone.py:281: LN is per-row, so
 *        only the rows that are used get normalised).
 *   bwd: dx = dres + rstd*(g - mean(g) - xhat*mean(g*xhat)), g = dy*gamma;  dy bf16 or f32.
 *        writes dx f32 and optional bf16 copy; dgamma/dbeta (f32 [cols], atomically
 *        accumulated) only when non-NULL.  row_index != NULL scatters into rows of dx.
 *        bf16_row_scale != NULL: the 16-bit copy is dx * bf16_row_scale[row / rows_per_img] (the gradient entering a
 *        DropPath-scaled residual branch); the f32 dx is unscaled.
 *        dx_dtype: REID_F32, or REID_F16 = the residual-stream gradient (dres read AND dx written) in IEEE half, saturating:
 *        12 instead of 16 bytes per element; the caller keeps the stream inside half's range by scaling the loss.
 *        overflow (nullable, int32 on the device): with dx_dtype = REID_F16 the call ORs 1 into *overflow when it stored any
 *        element clamped to +-65504, i.e. a finite value with |v| >= 65520 (in the f16 flavor: dx or its 16-bit copy); inf and
 *        NaN are stored as they are and do not set it.  The caller zeroes the flag; REID_F32 forms leave it untouched.
 * ------------------------------------------------------------------------------------------ */
int reid_layernorm_fwd(const float* x, int32_t ldx, const int32_t* row_index, const float* gamma,
                       const float* beta, void* y_bf16, float* y_f32, int32_t ldy, float* mean, float* rstd,
                       int32_t rows, int32_t cols, float eps, void* stream);
/* Residual add fused into the LayerNorm that follows it (models/clip_backbone.py:76 -> :82, :83 -> next block's :73):
 *   x_out = x + row_scale[row / rows_per_img] * y        (x f32, y = the 16-bit branch output of reid_mer_gemm; row_scale NULL = 1:
 *                                                         DropPath, clip_backbone.py:137-141);  h = LayerNorm(x_out) in 16 bits,
 *   mean / rstd of x_out saved for the backward pass.  x_out may alias x.  y_dtype: REID_BF16 (the flavor's format) or REID_F16
 *   (IEEE half whatever the flavor: what reid_mer_gemm stores with c_dtype = REID_F16). */
int reid_add_layernorm_fwd(const float* x, int32_t ldx, const void* y_bf16, int32_t y_dtype, int32_t ldy, const float* row_scale, int32_t rows_per_img,
                           float* x_out, int32_t ldxo, const float* gamma, const float* beta, void* h_bf16, int32_t ldh,
                           float* mean, float* rstd, int32_t rows, int32_t cols, float eps, void* stream);
int reid_layernorm_bwd(const void* dy, int32_t dy_dtype, int32_t lddy, const float* x, int32_t ldx,
                       const int32_t* row_index, const float* gamma, const float* mean, const float* rstd,
                       const void* dres, void* dx, int32_t dx_dtype, void* dx_bf16, int32_t lddx,
                       float* dgamma, float* dbeta, int32_t rows, int32_t cols,
                       const float* bf16_row_scale, int32_t rows_per_img, int32_t* overflow, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch extraction (im2col of the k=s=16 conv, models/patch_embeds.py:45-76):
 *   images f32 [n_img, 3, H, W] -> patches bf16 [n_img*(H/16)*(W/16), cin*256]; cin == 1 first
 *   averages the three channels (patch_embeds.py:63-65).  The conv itself is reid_mer_gemm.
 * cls rows: x[img*tokens + 0] = cls + pos[0]   (models/clip_backbone.py:269-273); cols % 4 == 0, ldx % 4 == 0, ldx >= cols (16-byte
 *   stores); no other row and no padding column of x is written.
 * ------------------------------------------------------------------------------------------ */
int reid_patch_im2col(const float* images, void* patches, int32_t n_img, int32_t H, int32_t W,
                      int32_t patch, int32_t cin, void* stream);
int reid_cls_rows(const float* cls, const float* pos0, float* x, int32_t ldx, int32_t n_img,
                  int32_t tokens, int32_t cols, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-head attention, head_dim 64, sequences of S <= 224 tokens held on chip
 * (MERMultiheadAttention SDPA call, models/mer_lora.py:166-190, scale 1/8; HF CLIP text
 *  attention with causal + key-padding mask; nn.MultiheadAttention of FeatureFusion,
 *  models/model.py:152-155).
 *   qkv bf16 [n_seq*S, ld] with q at column 0, k at column d, v at column 2d (d = heads*64).
 *   key_mask uint8 [n_seq, S] (1 = attend) or NULL; causal != 0 adds key <= query.
 *   out bf16 [n_seq*S, ldo]; lse f32 [n_seq, heads, S] (natural-log-sum-exp of scaled scores).
 *   bwd writes dqkv bf16 in the qkv layout.
 *   q_tiles > 0: only the first q_tiles 32-row query tiles of every sequence are evaluated (all keys take part): rows
 *   of out / lse beyond them are left untouched, dout is assumed zero there and dQ is written as zero -- the last ViT block,
 *   whose output is used at the class token only (clip_backbone.py:281).
 * ------------------------------------------------------------------------------------------ */
int reid_attn_fwd(const void* qkv, int32_t ld, const uint8_t* key_mask, void* out, int32_t ldo, float* lse,
                  int32_t n_seq, int32_t S, int32_t heads, int32_t causal, int32_t q_tiles, void* stream);
int reid_attn_bwd(const void* qkv, int32_t ld, const uint8_t* key_mask, const void* out, const void* dout,
                  int32_t ldo, const float* lse, void* dqkv, int32_t lddqkv, float* delta_ws,
                  int32_t n_seq, int32_t S, int32_t heads, int32_t causal, int32_t q_tiles, void* stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise helpers.
 * ------------------------------------------------------------------------------------------ */
/* fp32 -> the flavor's 16-bit format, round-to-nearest-even (IEEE half saturates finite overflow to +-65504; inf and NaN pass), 16-byte
 * aligned pointers; and back, exactly.  Exactly n elements are written. */
int reid_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
int reid_cast_bf16_f32(const void* src, float* dst, int64_t n, void* stream);
/* Batched fp32 -> bf16 repack of many small matrices that live in one fp32 arena (the LoRA parameters):
 * table[e] = {src_off, rows, cols, dst_off, dstT_off} (int64, element offsets; a negative dst offset skips that copy).
 * dst gets the same-layout bf16 copy at dst_off and the TRANSPOSED bf16 copy at dstT_off.  One launch per step. */
int reid_pack_bf16_table(const float* src, void* dst_bf16, const int64_t* table, int32_t n_entries, void* stream);
/* Adapter gradients of one MERLinear whose output width is N = 768 (autograd of LoRAAdapter, mer_lora.py:40-49), both products that
 * read the output cotangent dY in ONE pass:
 *   U[m, :]  = mask_modality(dY[m, :] . B) * scale      (16-bit [M, Rp]; column c kept iff c / mask_r == img_mod[m / rows_per_img];
 *                                                        BT = B^T [Rp, N] 16-bit; the operand of dA = U^T x, reid_gemm_tn)
 *   dB      += dY^T . T                                  (fp32 [N, Rp], atomics; T = the forward's masked x . A^T, 16-bit [M, Rp])
 * Rp must be 32, or 64 with rows_per_img >= 32 and mask_r a divisor of 16 (the one-image-per-workgroup kernel below; the class-row form
 * rows_per_img < 32 and REID_LORA_IMPL = 1 have no kernel for 64 adapter columns: REID_ERR_ARG).  A wider cotangent (fc1: 3072
 * columns) is handled as column blocks of 768, one launch each on the same stream:
 * u_mode bit 0 = add the fp32 partial sums u_partial [M, Rp] of the earlier blocks to this block's, bit 1 = store the sum to
 * u_partial instead of finishing U (mask, scale, 16-bit); the last block has bit 1 clear.  u_mode = 0: a 768-column linear, u_partial unused.
 * Other shapes: reid_mer_gemm (U) + reid_gemm_tn (dB).
 * T must be modality-masked (T[m, c] = 0 unless c / mask_r == img_mod[m / rows_per_img]) -- it is how reid_mer_gemm's mask epilogue
 * produces it: with rows_per_img >= 32 and mask_r a divisor of 16 one workgroup streams one image (one modality) and touches only the
 * aligned 16-column group of adapter columns that holds the modality's; elsewhere dB stays as it was.  A workgroup owns a span of G
 * consecutive images and streams each maximal run of one modality inside it as one row range (one flush of dB atomics per run: a batch
 * packed modality by modality pays G times fewer of them); any img_mod is correct.  G: knob "LORA_SPAN" = 1, 2, 4 or 8 (1 = one image
 * per workgroup, the reference form of the tests); unset or -1, a rule of the image count and the device's compute units. */
int reid_lora_bwd_fused(const void* dY, int32_t lddy, const void* T, int32_t ldt, const void* BT, int32_t ldbt, void* U, int32_t ldu,
                        float* dB, int32_t lddb, const int32_t* img_mod, int32_t rows_per_img, int32_t mask_r, int32_t M, int32_t N,
                        int32_t Rp, float scale, float* u_partial, int32_t u_mode, void* stream);
/* The other adapter gradient of a MERLinear, dA += U^T . X (autograd of lora_A, mer_lora.py:40-49), as one pass over the linear's INPUT
 * X [M, K] (16-bit; K a multiple of 768): dA[g Rp + c, k] += sum_m U[m, g Rp + c] X[m, k] for the n_groups (1, or 3 for the fused q|k|v
 * projection) adapter groups of Rp = 32 or 64 columns of U [M, n_groups Rp] (16-bit, modality-masked as reid_lora_bwd_fused writes it).
 * dA: fp32 [n_groups Rp, K] (row stride ldda), accumulated with atomics.  One workgroup per (span of G images, 768-column block), the
 * span worked through as runs of one modality like reid_lora_bwd_fused's (knob "LORA_SPAN", or the entry's own rule): rows_per_img >= 32,
 * mask_r a divisor of 16; other shapes: reid_gemm_tn(U, X). */
int reid_lora_da_fused(const void* X, int32_t ldx, const void* U, int32_t ldu, float* dA, int32_t ldda, const int32_t* img_mod,
                       int32_t rows_per_img, int32_t mask_r, int32_t M, int32_t K, int32_t Rp, int32_t n_groups, void* stream);

/* Merged MER-LoRA weights (mer_lora.py:80-99): for every table entry e and modality mu < nmod
 *     W_eff[e][mu] = W_e + scaling * Bcat_e[:, mu r : (mu+1) r] . Acat_e[g Rp + mu r : g Rp + (mu+1) r, :]      (16-bit, rounded once)
 * and its transpose -- the operands of reid_mer_gemm's row-group form.  table[e] = {W pointer (f32 [N, K] contiguous), arena
 * offset of Acat [G*Rp, K], arena offset of Bcat [N, Rp], destination offset of W_eff [nmod][N][K], destination offset of
 * W_eff^T [nmod][K][N] (negative: skip), N, K, G} (int64; offsets in elements; N, K, N/G multiples of 64; G = projections fused
 * along N, each with its own adapter rows g Rp ...).  max_tiles >= (N/64)(K/64) of every entry.  One launch per optimizer step.
 * Ranks: r <= 64 per modality and nmod * r <= Rp (up to 64 adapter rows are staged at once, more one modality at a time: same results). */
int reid_merge_lora_table(const int64_t* table, int32_t n_entries, int32_t max_tiles, const float* arena, void* weff,
                          int32_t Rp, int32_t r, int32_t nmod, float scaling, void* stream);
/* dst[r, :] = src[index[r], :] (f32; cols, lds, ldd multiples of 4; every index inside src);  scatter_add is the adjoint. */
int reid_gather_rows_f32(const float* src, int32_t lds, const int32_t* index, float* dst, int32_t ldd,
                         int32_t rows, int32_t cols, void* stream);
/* Text-tower input (HF CLIPTextEmbeddings, models/clip_backbone.py:307): out[b*T + t, :] = tok[ids[b, t], :] + pos[t, :]
 * (f32 tables [vocab, D] / [>= T, D], ids int64 [B, T], D % 4 == 0; ids outside the vocabulary are clamped as 64-bit numbers: below 0
 * to row 0, at or above vocab to row vocab - 1). */
int reid_embed_tokens(const float* tok, const float* pos, const int64_t* ids, float* out, int32_t B, int32_t T, int32_t D,
                      int32_t vocab, void* stream);
/* out[index[r], :] += src[r, :] (f32; rows with an index outside [0, out_rows) are skipped): gradient of an embedding
 * lookup (HF CLIPTextEmbeddings.token_embedding) when the text tower trains. */
int reid_scatter_add_rows_f32(const float* src, int32_t lds, const int32_t* index, float* out, int32_t ldo,
                              int32_t rows, int32_t cols, int32_t out_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * BN-neck (BNNeck.forward, models/model.py:208-224): BatchNorm1d(D) -> 8*L2-normalise.
 *   training != 0: batch statistics over `rows` (biased variance), running stats updated with
 *   momentum 0.1 / unbiased variance; else running statistics.  The classifier GEMM that
 *   follows is reid_mer_gemm on the bf16 copy.
 *   Statistics, training != 0: reid_bnneck_stats writes the column sums of x and x^2 (fp32, zeroed by the call) into sum / sqsum.
 *     count == rows (the sums are this call's own rows; the only form the model uses): the mean is taken from `sum` and the
 *       variance from a second pass over x, centred on that mean and accumulated in fp64 -- mean and invstd are the correctly
 *       rounded batch statistics to a few fp32 ulps whatever |mean|/std of a column is (sqsum is not read).
 *     count != rows (data-parallel SyncBN: the caller adds the sums of all ranks between the two phases and passes the global
 *       count): the call cannot see the other ranks' rows, so var = sqsum/count - mean^2 in fp32, clamped at 0.  With d fp32
 *       roundings on the way of a term through the sums, |d var| <= (3 d + 6) 2^-24 E[x^2]: the RELATIVE error of the variance
 *       (half of it in invstd) grows as 1 + (mean/std)^2 -- about 1e-6 at |mean|/std = 1, 1e-4..1e-3 at 30, useless beyond
 *       a few hundred.  A caller with such columns must reduce centred sums itself.
 *   fwd outputs: y f32 [rows, D] (norm 8 per row), y_bf16 optional, saved xhat-free state:
 *   mean[D], invstd[D], rnorm[rows].
 * ------------------------------------------------------------------------------------------ */
int reid_bnneck_stats(const float* x, int32_t ldx, int32_t rows, int32_t D, float* sum, float* sqsum, void* stream);
int reid_bnneck_fwd(const float* x, int32_t ldx, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, const float* sum, const float* sqsum, float count, int32_t training,
                    float* y, void* y_bf16, int32_t ldy, float* mean, float* invstd, float* rnorm,
                    int32_t rows, int32_t D, float eps, float momentum, float scale, void* stream);
/* bwd phase 1: per-row L2-normalise backward -> dz (grad wrt BN output), and column sums
 *   sum_dz[D], sum_dz_xhat[D] (all-reduced by the caller under data parallelism); dy and x are read 16 bytes at a time: lddy and ldx
 *   multiples of 4 and >= D; dz is [rows, D] contiguous;
 * bwd phase 2: dx = gamma*invstd*(dz - sum_dz/count - xhat*sum_dz_xhat/count); dgamma = sum_dz_xhat; dbeta = sum_dz */
int reid_bnneck_bwd_p1(const float* dy, int32_t lddy, const float* x, int32_t ldx, const float* gamma,
                       const float* beta, const float* mean, const float* invstd, const float* rnorm,
                       float* dz, float* sum_dz, float* sum_dz_xhat, int32_t rows, int32_t D, float scale,
                       void* stream);
int reid_bnneck_bwd_p2(const float* dz, const float* x, int32_t ldx, const float* gamma, const float* mean,
                       const float* invstd, const float* sum_dz, const float* sum_dz_xhat, float count,
                       int32_t training, float* dx, int32_t lddx, int32_t rows, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cross entropy with label smoothing (nn.CrossEntropyLoss(label_smoothing=0.1), models/model.py:290,
 * 529-549): mean over rows with valid[r] != 0 and 0 <= label < C.
 *   loss_sum[0] += sum of row losses, loss_sum[1] += number of rows used (both f32, zeroed by caller);
 *   dlogits = (softmax - smoothed one-hot) * grad_scale for used rows, 0 otherwise (grad_scale =
 *   ce_weight / global_count, read from device memory so no host sync is needed).
 * ------------------------------------------------------------------------------------------ */
int reid_ce_ls_fwd(const float* logits, int32_t ld, const int64_t* labels, const uint8_t* valid, int32_t rows,
                   int32_t C, float smoothing, float* row_loss, float* loss_sum, void* stream);
int reid_ce_ls_bwd(const float* logits, int32_t ld, const int64_t* labels, const uint8_t* valid, int32_t rows,
                   int32_t C, float smoothing, const float* grad_scale, float* dlogits, int32_t lddl, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused SDM loss (sdm_loss_stable, models/sdm_loss.py:13-149) for ALL modality pairs of a step (models/model.py:586-622
 * calls it once per non-vis modality against vis):
 *   q [P*N, D] f32 = the P query sides stacked (rows [p*N, (p+1)*N) = pair p), g [Mg, D] f32 = the shared vis side;
 *   q_label [N] (the batch labels, shared by the pairs), g_label [Mg]; q_valid [P*N] / g_valid [Mg] uint8 or NULL (rows that
 *   take part, models/model.py:570,595); positives y[i,j] = (q_label[i] == g_label[j]) (models/model.py:605);
 *   tau clamped to [0.15, 0.5] (:28); unit vectors with eps 1e-8 (:31-32); S = q^ g^T / tau clamped to +-20 (:86,94).
 *   result[2p]   = 0.5 * (mean over rows with a positive of CE(q->g) + mean over such columns of CE(g->q))  (:34-70,121-123)
 *   result[2p+1] = 1 if pair p has any positive (it contributes to the modality mean), else 0 and result[2p] = 0 (:105-106).
 * S is never materialised: each tile of it exists only in MFMA accumulators (v_mfma_f32_32x32x2_f32 on the fp32 unit
 * vectors, exact fp32) and is reduced to per-tile row / column partial sums that a second small launch adds in a fixed order;
 * the backward pass recomputes the tiles.  No N x Mg array exists in fwd or bwd.
 *   ws (reid_sdm_ws_floats(P, N, Mg, D) floats, kept from fwd to bwd):
 *     unit vectors (P N + Mg) D | {lse, #pos} per row and column 2 P (N + Mg) | 4 P sums | P (N + Mg) loss terms |
 *     max( per-tile partials 4 (tiles_n P N + tiles_m P Mg),  gradient accumulators (P N + Mg) D )      [tiles of 64 or 128]
 *   bwd: dq [P*N, D] and dg [Mg, D] (+= into f32) for the upstream gradients gscale[p] (device array [P]).
 * Requirements: D % 32 == 0, 32 <= D <= 1024.
 * ------------------------------------------------------------------------------------------ */
int reid_sdm_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label,
                 const int64_t* g_label, const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg,
                 int32_t D, float tau, float* ws, float* result, void* stream);
int reid_sdm_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label,
                 const int64_t* g_label, const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg,
                 int32_t D, float tau, float* ws, const float* gscale, float* dq, int32_t lddq, float* dg,
                 int32_t lddg, void* stream);
int64_t reid_sdm_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D);

/* ------------------------------------------------------------------------------------------
 * Batch-hard triplet loss (Hermans et al. 2017; the reference has no such loss) on x [rows, D] f32 (leading dimension ldx), the
 * fused feature in front of the BN-neck:
 *   labels [rows] int64; valid [rows] uint8 or NULL (rows with valid == 0 are neither anchors nor candidates);
 *   d2(i,j) = sum_c (x_ic - x_jc)^2 in the DIFFERENCE form (never |x|^2 + |y|^2 - 2 x.y: the feature is mostly batch mean),
 *   d(i,j) = sqrt(max(d2, 1e-12)); where d2 <= 1e-12 that term's gradient is zero (clamp(min=1e-12).sqrt()).
 *   Hardest positive of anchor i: the valid j != i with labels[j] == labels[i] and the largest d2; hardest negative: the valid j with
 *   another label and the smallest d2; ties on the fp32 d2 go to the lowest index, for both.  An anchor is active if it is valid and
 *   has both; otherwise idx_p = idx_n = -1 and d_ap = d_an = row_loss = 0.
 *   row_loss[i] = max(0, d_ap - d_an + margin) for margin >= 0, softplus(d_ap - d_an) for margin < 0 (the soft-margin form);
 *   result[0] = sum of the active rows' losses / max(1, n_active), result[1] = n_active (a float: no host read-back; no active anchor
 *   gives loss 0 and a zero gradient).  The sum is taken in a fixed order in fp64 by a one-workgroup second launch.
 *   bwd: dx [rows, D] (leading dimension lddx) is OVERWRITTEN with dloss[0] * d result[0] / dx, gathered per output row from the saved
 *   d_ap, d_an, idx_p, idx_n in ascending anchor order (one launch); a saved distance equal to the clamp value contributes nothing
 *   (that also covers a d2 a few ulp above 1e-12 whose square root rounds to the same float).  Non-finite features: a d2 that
 *   overflowed to +inf is an ordinary candidate (it can be the hardest positive, and the hardest negative when it is the only one);
 *   a NaN d2 never ranks before anything.
 *   No atomics in either direction: two runs give the same bits.  The features are not L2-normalised inside the loss.
 * Requirements: D % 4 == 0, 4 <= D <= 1024, 1 <= rows <= 8192, ldx / lddx multiples of 4 and >= D, rows * ld < 2^31, x and dx 16-byte
 * aligned.
 * ------------------------------------------------------------------------------------------ */
int reid_triplet_hard_fwd(const float* x, int32_t ldx, const int64_t* labels, const uint8_t* valid, int32_t rows, int32_t D,
                          float margin, float* d_ap, float* d_an, int32_t* idx_p, int32_t* idx_n, float* row_loss,
                          float* result, void* stream);
int reid_triplet_hard_bwd(const float* x, int32_t ldx, int32_t rows, int32_t D, float margin, const float* d_ap,
                          const float* d_an, const int32_t* idx_p, const int32_t* idx_n, const float* result,
                          const float* dloss, float* dx, int32_t lddx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cross-modal batch-hard triplet loss (bi-directional cross-modality triplet of Ye et al., AGW 2021, with the mining of Hermans et
 * al. 2017; the reference has no such loss): every non-vis modality against vis, on the raw modality features.  All fp32.
 *   q [P*N, D] (leading dimension ldq) = the P query sides stacked, rows [p*N, (p+1)*N) = pair p; g [Mg, D] (ldg) = the shared vis
 *   side; q_label [N] int64 (shared by the pairs), g_label [Mg]; q_valid [P*N] / g_valid [Mg] uint8 or NULL (rows with 0 are neither
 *   anchors nor candidates) -- the conventions of reid_sdm_fwd.
 *   Unit rows (normalize == 1): x^ = x * (1 / max(sqrt(sum_c x_c^2), eps)), evaluated as reid_l2norm_rows evaluates it (bit-equal rows
 *   give bit-equal unit rows); normalize == 0: the rows are used as they are.
 *   d2(a,b) = sum_c (a^_c - b^_c)^2 in the DIFFERENCE form (never 2 - 2 cos: the modality features share a large common mean),
 *   d = sqrt(max(d2, 1e-12)); a term whose saved d equals the clamp value has no gradient (the rule of reid_triplet_hard_*).
 *   Mining compares the fp32 d2 (a D-term sum).  The two distances an anchor KEEPS are then re-evaluated from the same fp32 rows with
 *   an fp64 sum, rounded once to fp32 and rooted there: l'(d_ap - d_an) of the backward inherits the absolute error of the saved
 *   distances, and the few ulp of the fp32 sum at d = 40 are already 1e-5 of the soft margin's gradient.
 *   Mining, per pair p, in two directions.  q->g: every valid q row i of pair p is an anchor; hardest positive = the valid g row j
 *   with g_label[j] == q_label[i] and the largest d2, hardest negative = the valid g row with another label and the smallest d2.
 *   g->q: every valid g row j is an anchor against the valid q rows of pair p by the same rules, indices pair-local (0..N-1).  Ties on
 *   the fp32 d2 go to the lowest index in both directions.  There is NO self-exclusion: row i of q and row i of g are one person in
 *   two modalities, a legitimate positive.  An anchor is active when it is valid and has both a positive and a negative; otherwise
 *   its indices are -1 and its distances and row loss 0.  A +inf d2 is an ordinary candidate, a NaN d2 never ranks before anything.
 *   Row loss l = max(0, d_ap - d_an + margin) for margin >= 0, softplus(d_ap - d_an) for margin < 0 (the soft-margin form).
 *   L_p = 0.5 * (sum over the active q anchors of l / max(1, n_qg[p]) + sum over the active g anchors of l / max(1, n_gq[p])), the
 *   sums taken in a fixed order in fp64 by a small last launch; result [P, 4] = {L_p, flag_p, n_qg[p], n_gq[p]} with flag_p = 1 iff
 *   n_qg + n_gq > 0 (L_p = 0 otherwise).  Nothing is read back to the host.
 *   Saved: q_d [2, P*N] = d_ap | d_an, q_idx [2, P*N] = idx_p | idx_n (rows of g); g_d [2, P*Mg], g_idx [2, P*Mg] (rows 0..N-1 of
 *   pair p's q side); ws (reid_cross_triplet_ws_floats(P, N, Mg, D) floats, kept from fwd to bwd):
 *     unit rows (P N + Mg) D | 1 / max(|x|, eps) (P N + Mg) | |x| (P N + Mg) | row losses P N + P Mg   (a negative count = bad shape).
 *   bwd: dq [P*N, D] (lddq) and dg [Mg, D] (lddg) are OVERWRITTEN (every row is written, invalid rows with zeros) in a gather form
 *   without atomics.  The unit-space gradient G of q row (p, i): its own two terms as an anchor, then every g anchor j of pair p in
 *   ascending j whose idx_p or idx_n is i.  Of g row j, for p ascending: its own two terms as an anchor of pair p, then the q anchors
 *   of pair p in ascending i that chose j.  A term is c (x^_i - x^_a) / d with c = gscale[p] * 0.5 * l' / max(1, n), n the count of
 *   the ANCHOR's direction; gscale f32 [P] on the device = dLoss / dL_p.  normalize == 1: dx = (G - x^ (x^ . G)) / max(|x|, eps)
 *   where |x| >= eps and dx = G / eps where |x| < eps (what autograd gives for x / norm.clamp_min(eps)); normalize == 0: dx = G.
 *   Two runs give the same bits in every output.  Nothing is allocated or synchronised inside a call.
 * Requirements: 1 <= P <= 8; 1 <= N, Mg <= 8192; D % 4 == 0, 4 <= D <= 1024; ldq / ldg / lddq / lddg multiples of 4 and >= D;
 * rows * ld < 2^31; q, g, ws, dq, dg 16-byte aligned; margin not NaN; normalize 0 or 1; eps >= 0.  Anything else: REID_ERR_ARG
 * before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t reid_cross_triplet_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D);
int reid_cross_triplet_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label,
                           const int64_t* g_label, const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N,
                           int32_t Mg, int32_t D, float margin, int32_t normalize, float eps, float* q_d, int32_t* q_idx,
                           float* g_d, int32_t* g_idx, float* ws, float* result, void* stream);
int reid_cross_triplet_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const uint8_t* q_valid,
                           const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg, int32_t D, float margin,
                           int32_t normalize, float eps, const float* q_d, const int32_t* q_idx, const float* g_d,
                           const int32_t* g_idx, const float* ws, const float* result, const float* gscale, float* dq,
                           int32_t lddq, float* dg, int32_t lddg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hetero-center triplet loss (Zhu et al., "Hetero-Center Loss", Neurocomputing 2020; Liu et al., "Parameter Sharing Exploration and
 * Hetero-Center Triplet Loss", IEEE TMM 2020; the reference has no such loss): the triplet runs on the per-identity CENTRES of
 * every modality inside the batch, each non-vis modality against vis.  All fp32.  Inputs as reid_cross_triplet_*: q [P*N, D] (ldq),
 * g [Mg, D] (ldg), q_label [N] / g_label [Mg] int64, q_valid [P*N] / g_valid [Mg] uint8 or NULL.
 *   1. Unit rows (normalize == 1): x^ exactly as reid_cross_triplet_fwd and reid_l2norm_rows evaluate it; normalize == 0: the rows as
 *      they are.
 *   2. Centres.  On one side (pair p's q rows, or the g rows) the leader of a valid row i is the lowest-index valid row of that side
 *      with the same label.  The centres of a side are listed in ascending leader order, compacted: centre s belongs to the s-th
 *      leader; every side has its own centre count S, which exists only on the device.  centre = (fp32 sum of the members' x^ in
 *      ascending row order) / float(count), one division per element.  The g centres are computed once and shared by all pairs.
 *      Saved: lead int32 [P*N + Mg] per ROW (q rows, then g rows) = the centre slot of the row within its side, -1 for an invalid row;
 *      count int32 [P*N + Mg] per SLOT (pair p's q slots at p*N, the g slots at P*N) = members, 0 behind S; clabel int64 [P*N + Mg] =
 *      the centre's label per slot (0 behind S).
 *   3. Mining, per pair p, over the union U_p = [q centres of pair p | g centres] in the index space 0 .. N+Mg-1: q centre s -> s,
 *      g centre t -> N + t.  Every centre is an anchor.  Its positive is the centre of the OTHER side with the same label (at most one:
 *      labels are distinct within a side); its negative is the centre of U_p with another label and the smallest fp32 d2, from either
 *      side, ties to the lowest index.  d2 in the difference form, d = sqrt(max(d2, 1e-12)); clamped, +inf and NaN distances follow the
 *      rules of reid_triplet_hard_*.  An anchor is active when it has a positive and a negative; otherwise its indices are -1 and its
 *      distances and loss 0 (so are the slots behind a side's S).  The two distances an active anchor keeps are re-evaluated from the
 *      fp32 centres with an fp64 sum, rounded once and rooted in fp32, as reid_cross_triplet_fwd does.
 *      Saved: d [2, P, N+Mg] = d_ap | d_an, idx [2, P, N+Mg] = idx_p | idx_n, both in the index space.
 *   4. Loss.  l = max(0, d_ap - d_an + margin) for margin >= 0, softplus(d_ap - d_an) for margin < 0 (soft margin).
 *      L_p = sum over the active anchors of l / max(1, n_q[p] + n_g[p]) (n_q / n_g: active anchors among the q / g centres), summed in
 *      a fixed order in fp64; result [P, 4] = {L_p, flag_p, n_q, n_g} with flag_p = 1 iff n_q + n_g > 0.
 *   5. bwd: dq [P*N, D] (lddq) and dg [Mg, D] (lddg) are OVERWRITTEN (invalid rows with zeros), gather form, no atomics.  The
 *      centre-space gradient of a centre: its own two terms as an anchor, then the anchors of U_p that chose it in ascending index;
 *      for a g centre this runs over p ascending.  A term is gscale[p] * l' / max(1, n_q + n_g) * (c_i - c_a) / d (nothing where the
 *      saved d is the clamp value).  A valid row receives G_centre(lead) / float(count), then the projection through the normalisation
 *      exactly as reid_cross_triplet_bwd, the |x| < eps branch included.  Two runs give the same bits in every output.
 *   ws: reid_hc_triplet_ws_floats(P, N, Mg, D) floats, kept from fwd to bwd (bwd writes the centre gradients into it):
 *     unit rows R D | centres P U D (compact per pair: S_q[p] q centres, then S_g g centres) | centre gradients R D | centre labels
 *     P U int64 | compact distances 2 P U | compact indices 2 P U | anchor losses P U | 1 / max(|x|, eps) R | |x| R | leader rows R |
 *     centre counts P + 1, with R = P N + Mg and U = N + Mg (a negative count = bad shape).
 *   Nothing is allocated, synchronised or read back inside a call.
 * Requirements and argument checks: those of reid_cross_triplet_* (REID_ERR_ARG before any launch).
 * ------------------------------------------------------------------------------------------ */
int64_t reid_hc_triplet_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D);
int reid_hc_triplet_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label,
                        const int64_t* g_label, const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N,
                        int32_t Mg, int32_t D, float margin, int32_t normalize, float eps, int32_t* lead, int32_t* count,
                        int64_t* clabel, float* d, int32_t* idx, float* ws, float* result, void* stream);
int reid_hc_triplet_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, int32_t P, int32_t N, int32_t Mg, int32_t D,
                        float margin, int32_t normalize, float eps, const int32_t* lead, const int32_t* count, float* ws,
                        const float* result, const float* gscale, float* dq, int32_t lddq, float* dg, int32_t lddg,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Cross-batch memory for the cross-modal triplet loss (Wang et al., "Cross-Batch Memory for Embedding Learning", CVPR 2020; the
 * reference has no such loss): the rows of the last batches stay in a ring on the device, and the anchors of the current batch mine
 * their hardest positive / negative among ALL of the ring's rows, which are constants.  All fp32.
 *   Sides: 0 = vis, 1 .. P = the P non-vis modalities (P <= 8).  The memory of capacity M (N <= M <= 8192) is
 *     rows [P+1, M, D] f32 (contiguous) | mem_labels [M] int64 | mem_valid [P+1, M] uint8 | cursor int32 [2] = (next slot, rows ever
 *     written; the count stops at 2^31 - 1), all on the device.  A fresh or reset memory: mem_valid = 0 everywhere, cursor = (0, 0).
 *   A batch: q [P*N, D] (ldq) = the P non-vis sides stacked, g [N, D] (ldg) = the vis side, labels [N] int64, q_valid [P*N] / g_valid
 *   [N] uint8 or NULL (all valid); row i of every side is the same instance.
 *   reid_xbm_enqueue: row i of side s goes to slot (cursor[0] + i) mod M of side s (a batch may wrap; the oldest rows are overwritten),
 *   as its unit row x * (1 / max(|x|, eps)) when normalize == 1 -- evaluated as reid_l2norm_rows evaluates it, bit for bit -- or as it
 *   is; labels[i] and the sides' validity bytes go to the same slot (an invalid row is stored with mem_valid = 0).  Then the cursor
 *   advances by N.  The cursor is read and written ON THE DEVICE (one launch for the rows, a one-thread launch behind it for the
 *   cursor), so a captured graph that holds the call keeps filing rows where the last replay stopped.
 *   reid_xbm_triplet_fwd mines the memory AS IT STANDS (call reid_xbm_enqueue first and the current batch is part of it, as in the
 *   paper).  Per pair p, direction q->mem: every valid row of q's pair p is an anchor against the valid slots of side 0; direction
 *   g->mem: every valid row of g is an anchor against the valid slots of side p + 1.  The rules are those of reid_cross_triplet_fwd:
 *   hardest positive = same label at the largest d2, hardest negative = another label at the smallest d2; d2 in the difference form
 *   in fp32; ties go to the lowest SLOT; no self-exclusion (an anchor never meets its own side); an anchor is active when it is valid
 *   and has both, otherwise its indices are -1 and its distances and row loss 0; the two kept distances are re-evaluated with an fp64
 *   sum, d = sqrt(max(d2, 1e-12)).  normalize == 1: the anchors are the unit rows of the batch (the ring is expected to hold unit rows
 *   too).  Row loss l = max(0, d_ap - d_an + margin) for margin >= 0, softplus(d_ap - d_an) for margin < 0.
 *   L_p = 0.5 * (sum over the active q anchors of l / max(1, n_q[p]) + sum over the active g anchors of l / max(1, n_g[p])), summed in a
 *   fixed order in fp64; result [P, 4] = {L_p, flag_p, n_q[p], n_g[p]} with flag_p = 1 iff n_q + n_g > 0.
 *   Saved: q_d [2, P*N] = d_ap | d_an, q_idx [2, P*N] = idx_p | idx_n (slots of side 0); g_d, g_idx [2, P*N] (slots of side p + 1);
 *   ws (reid_xbm_ws_floats(P, N, M, D) floats, kept from fwd to bwd; a negative count = bad shape):
 *     unit rows (P + 1) N D | COPIES of the two kept rows of every active anchor 2 P N x 2 D | 1 / max(|x|, eps) (P + 1) N | |x| (P + 1) N
 *     | row losses 2 P N.
 *   reid_xbm_triplet_bwd: dq [P*N, D] (lddq) and dg [N, D] (lddg) are OVERWRITTEN (invalid rows with zeros).  The memory's rows are
 *   constants: an anchor gets only its own two terms, c ((x^ - m_p) / d_ap - (x^ - m_n) / d_an) with c = gscale[p] * 0.5 * l' /
 *   max(1, n) (n of the anchor's direction; a term whose saved d is the clamp value is dropped); a g row adds its terms for p = 0 ..
 *   P-1 in ascending order; then the projection through the normalisation exactly as reid_cross_triplet_bwd.  m_p and m_n are the
 *   COPIES in ws: the backward never reads the ring, which later enqueues may have overwritten.
 *   No atomics: two runs give the same bits in every output and in the ring.  Nothing is allocated, synchronised or read back.
 * Requirements: those of reid_cross_triplet_* with Mg = N, and N <= M <= 8192; rows 16-byte aligned.  Anything else: REID_ERR_ARG
 * before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t reid_xbm_ws_floats(int32_t P, int32_t N, int32_t M, int32_t D);
int reid_xbm_enqueue(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* labels, const uint8_t* q_valid,
                     const uint8_t* g_valid, int32_t P, int32_t N, int32_t M, int32_t D, int32_t normalize, float eps,
                     float* rows, int64_t* mem_labels, uint8_t* mem_valid, int32_t* cursor, void* stream);
int reid_xbm_triplet_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* labels, const uint8_t* q_valid,
                         const uint8_t* g_valid, int32_t P, int32_t N, int32_t M, int32_t D, float margin, int32_t normalize,
                         float eps, const float* rows, const int64_t* mem_labels, const uint8_t* mem_valid, float* q_d,
                         int32_t* q_idx, float* g_d, int32_t* g_idx, float* ws, float* result, void* stream);
int reid_xbm_triplet_bwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const uint8_t* q_valid, const uint8_t* g_valid,
                         int32_t P, int32_t N, int32_t D, float margin, int32_t normalize, float eps, const float* q_d,
                         const int32_t* q_idx, const float* g_d, const int32_t* g_idx, const float* ws, const float* result,
                         const float* gscale, float* dq, int32_t lddq, float* dg, int32_t lddg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Center loss (Wen et al., "A Discriminative Feature Learning Approach for Deep Face Recognition", ECCV 2016; the reference has no
 * such loss; csrc/center.hip): one centre per identity in a table on the device, every used row pulled towards the centre of its
 * label, and Wen's update (eq. 4) of the centres the forward has just used.  All fp32, every operation rounded on its own (no fused
 * multiply-add), so a float32 loop on the host reproduces diff, the updated centres and dx bit for bit.
 *   x [S*N, D] (ldx): S sides stacked, row s*N + i = instance i of side s; labels [N] int64, shared by the sides; valid [S*N] uint8 or
 *   NULL (all valid); centers [C, D] f32, contiguous.  A row is USED when it is valid and 0 <= labels[i] < C.
 *   ws: reid_center_ws_floats(S, N, D) floats kept from fwd to bwd (a negative count = bad shape): diff S N D | used flags S N.
 *   reid_center_fwd: diff[r, c] = x[r, c] - centers[y_r, c] (unused rows: zeros; they read no centre); d2[r] = sum_c diff^2 in fp32
 *   (per-lane partial sums, then a butterfly over the wave; unused rows 0); a one-workgroup launch behind it writes
 *   result[0] = 0.5 * sum over the used rows of d2 / max(1, n_used), added in ascending row order in fp64 and rounded once, and
 *   result[1] = n_used as a float.  Neither is read back.
 *   reid_center_update (with the labels / valid the forward had): a row CONTRIBUTES when it is used and its d2 is finite (a NaN or inf
 *   feature makes the loss non-finite, which the step driver skips; it must not reach a centre).  For every class j with n_j >= 1
 *   contributing rows: acc = 0; for those rows r ascending: acc = acc + (-diff[r, c]); delta = acc / float(1 + n_j);
 *   centers[j, c] = centers[j, c] - alpha * delta.  Gather form: the wave of the lowest contributing row of a label does its centre
 *   row, every other wave leaves; rows of classes not in the batch keep their bits.
 *   reid_center_bwd: coef = dloss[0] / max(1.0f, result[1]) (one fp32 division); dx[r, c] = coef * diff[r, c]; dx [S*N, D] (lddx) is
 *   OVERWRITTEN (unused rows with zeros, padding columns untouched).  It reads ws and result only, never centers: an update between
 *   the forward and the backward does not change the gradient (the rule of reid_xbm_triplet_bwd).
 *   No atomics: two runs give the same bits in every output and in the table.  Nothing is allocated, synchronised or read back.
 * Requirements: 1 <= S <= 9, 1 <= N <= 8192, C >= 1, D % 4 == 0, 4 <= D <= 1024, ldx / lddx multiples of 4 and >= D, S*N*ld < 2^31,
 * C*D < 2^31, x, centers, ws and dx 16-byte aligned, alpha finite.  Anything else: REID_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t reid_center_ws_floats(int32_t S, int32_t N, int32_t D);
int reid_center_fwd(const float* x, int32_t ldx, const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D,
                    const float* centers, int32_t C, float* ws, float* d2, float* result, void* stream);
int reid_center_update(const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* d2,
                       const float* ws, float* centers, int32_t C, float alpha, void* stream);
int reid_center_bwd(int32_t S, int32_t N, int32_t D, const float* ws, const float* result, const float* dloss, float* dx,
                    int32_t lddx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cluster-contrast memory loss, "ClusterNCE" (the cluster-level memory of SpCL, Ge et al., NeurIPS 2020; Cluster-Contrast, Dai et
 * al., 2021; the reference has no such loss; csrc/cluster_nce.hip): a non-parametric classifier over one unit centroid per cluster
 * of a pseudo-labelled set, kept in a table on the device and moved by momentum.  All fp32.
 *   x [S*N, D] (ldx): S sides stacked, row r = s*N + i = instance i of side s; labels [N] int64, shared by the sides; valid [S*N] uint8
 *   or NULL (all valid); table [K, D] f32, contiguous, unit rows.  A row is USED when it is valid and 0 <= labels[i] < K (a DBSCAN
 *   noise label of -1 is simply unused).  With x^ = x / max(|x|, 1e-12):
 *     l_rc = (x^_r . C_c) / tau,   loss = mean over the used rows of (lse_c(l_rc) - l_r,y),  0 when no row is used.
 *   reid_cluster_nce_plan(R, K, D, plan): plan[0] = row tile, plan[1] = class tile, plan[2] = the number of splits of the class range
 *   over workgroups, plan[3] = class tiles per split (split s takes class tiles [s * plan[3], (s + 1) * plan[3])).  It depends on the
 *   shape only: splits = min(class tiles, 64, max(1, 512 / row tiles)), then made free of empty splits.
 *   ws: reid_cluster_nce_ws_floats(S, N, D, K) floats kept from fwd to update and bwd (a negative count = bad shape).
 *   reid_cluster_nce_fwd: the [S*N, K] logits are never stored -- a tile of x^ C^T lives in v_mfma_f32_32x32x2_f32 accumulators (exact
 *   fp32 products); every row carries a running maximum and sum of exp over the class tiles, the splits' partials are merged in
 *   split order by a second kernel, which also writes row_loss[r] = lse_r - l_r,y and target_cos[r] = x^_r . C_y (unused rows: 0) and
 *   result[0] = sum over the used rows of row_loss / max(1, n_used), added in ascending row order in fp64 and rounded once,
 *   result[1] = n_used as a float.  Neither is read back.  with_grad = 0 stops there: the table is streamed ONCE.  with_grad = 1
 *   streams it a second time for sum_c p_rc C_c (p = exp(l - lse), per-split partials added in split order) and leaves
 *     G_r = (sum_c p_rc C_c - C_y) / tau,   H_r = (G_r - x^_r (x^_r . G_r)) / max(|x_r|, 1e-12)      (unused rows: zeros)
 *   in ws.  The table is a constant of the loss.
 *   reid_cluster_nce_update (with the labels / valid the forward had, after the forward): a row CONTRIBUTES when it is used and its
 *   row_loss is finite.  For every label with a contributing row, mode REID_CLUSTER_NCE_MEAN applies, for its contributing rows in
 *   ascending row order,  c = momentum * c + (1 - momentum) * x^_r;  c = c / max(|c|, 1e-12)  (Cluster-Contrast's sequential loop);
 *   REID_CLUSTER_NCE_HARD applies the same blend once, with the contributing row of the smallest target_cos (ties: the lowest row).
 *   Gather form: the wave of the lowest contributing row of a label does its centroid, every other wave leaves; centroids of labels
 *   not in the batch keep their bits.
 *   reid_cluster_nce_bwd: dx[r, c] = (dloss[0] / max(1.0f, result[1])) * H[r, c]; dx [S*N, D] (lddx) is OVERWRITTEN (unused rows with
 *   zeros, padding columns untouched).  It reads ws and result only, never the table: an update or a second forward into another ws
 *   between the forward and the backward does not change the gradient.
 *   reid_cluster_centroids: table[k] = the normalised fp32 mean of the rows order[offsets[k]] .. order[offsets[k + 1] - 1] of feats
 *   [rows, D] (ldf), summed in that order (the caller groups the row indices by label, ascending inside a label: offsets [K + 1]);
 *   one wave per cluster; an empty cluster gets zeros.
 *   No atomics: two runs give the same bits in every output and in the table.  Nothing is allocated, synchronised or read back.
 * Requirements: 1 <= S <= 9, 1 <= N <= 8192, K >= 1, D % 32 == 0, 32 <= D <= 1024, K*D < 2^31, ldx / lddx / ldf multiples of 4 and
 * >= D, rows * ld < 2^31, x, feats, table, ws and dx 16-byte aligned, tau > 0 and finite, 0 <= momentum <= 1, with_grad 0 or 1.
 * Anything else: REID_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------------ */
#define REID_CLUSTER_NCE_MEAN 0
#define REID_CLUSTER_NCE_HARD 1
int64_t reid_cluster_nce_ws_floats(int32_t S, int32_t N, int32_t D, int32_t K);
int reid_cluster_nce_plan(int32_t R, int32_t K, int32_t D, int32_t* plan);
int reid_cluster_nce_fwd(const float* x, int32_t ldx, const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D,
                         const float* table, int32_t K, float tau, int32_t with_grad, float* ws, float* row_loss, float* target_cos,
                         float* result, void* stream);
int reid_cluster_nce_update(const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* row_loss,
                            const float* target_cos, const float* ws, float* table, int32_t K, float momentum, int32_t mode,
                            void* stream);
int reid_cluster_nce_bwd(int32_t S, int32_t N, int32_t D, const float* ws, const float* result, const float* dloss, float* dx,
                         int32_t lddx, void* stream);
int reid_cluster_centroids(const float* feats, int32_t ldf, int64_t rows, const int64_t* order, const int64_t* offsets, int32_t K,
                           int32_t D, float* table, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cross-modal Smooth-AP ranking loss (Brown et al., "Smooth-AP: Smoothing the Path Towards Large-Scale Image Retrieval", ECCV 2020;
 * the reference has no such loss; csrc/smooth_ap.hip): the differentiable form of the AP the evaluator
 * reports, in the batch or against the slots of a cross-batch memory.  All fp32 in and out.
 *   q [P*N, D] (ldq), g [Mg, D] (ldg), q_label [N], g_label [Mg] int64, q_valid [P*N] / g_valid [Mg] uint8 or NULL (all valid): as
 *   for reid_cross_triplet_fwd.  Every direction of every pair p is one set of ranking problems against a GALLERY given as (rows, ld,
 *   labels, validity bytes or NULL, count):
 *     q->g: the valid rows of q[p] are the anchors, gallery A = (ga, ldga, ga_label [Ga], ga_valid [Ga], Ga), shared by the pairs;
 *     g->q: the valid rows of g are the anchors, gallery B of pair p = rows [p*Gb, (p+1)*Gb) of gb (ldgb), gb_label [Gb] shared,
 *           gb_valid [P*Gb].
 *   gallery_grad = 1, the batch form: the galleries ARE the batch (ga = g, gb = q, with their labels, validity and counts: anything
 *   else is refused) and receive a gradient.  gallery_grad = 0, the ring form: gallery A = side 0 of a memory filed by
 *   reid_xbm_enqueue, gallery B = its sides 1 .. P; their rows are constants, taken as they are.
 *   Score of anchor a and gallery row j: s_j = x^_a . g^_j with x^ = x / max(|x|, eps) (normalize = 0: the rows as they are; ring rows
 *   are always taken as they are) -- the dot product and the norms in fp64 from the fp32 inputs, rounded to fp32 ONCE.  No
 *   self-exclusion.  P_a = the valid gallery rows with the anchor's label; a is ACTIVE when it is valid, P_a is not empty and a
 *   valid gallery row lies outside it.  With sigma_ij = sigma((s_j - s_i) / tau) over the valid gallery rows:
 *     R_i = 1 + sum_{j != i} sigma_ij,  R+_i = 1 + sum_{j in P_a, j != i} sigma_ij,  AP_a = (1 / |P_a|) sum_{i in P_a} R+_i / R_i,
 *     L_dir = mean over the active anchors of (1 - AP_a) (0 when there is none),  L_p = 0.5 * (L_qg + L_gq).
 *   sigma is evaluated in fp32 as e = exp(-|d|): d >= 0 ? 1 / (1 + e) : e / (1 + e).  Every sum has a fixed order (over j: per-lane
 *   ascending, then a butterfly across the lanes; over i, anchors and pairs: ascending); no atomics; two runs give the same bits.
 *   Outputs: q_ap [P*N], g_ap [P*Mg] = AP_a (-1: not active), q_npos / g_npos int32 = |P_a| (0 for an invalid anchor), result
 *   [P, 4] = (L_p, flag_p, n_qg, n_gq) with flag_p = 1 when either direction has an active anchor; the means are fp64 sums in
 *   ascending row order, rounded once.  None is read back.
 *   ws: reid_smooth_ap_ws_floats(P, N, Mg, D, Ga, Gb, with_grad) floats (a negative count = bad shape).  with_grad = 0 stops after
 *   result.  with_grad = 1 also forms d(1 - AP_a)/ds in closed form, gathers it into the unit-space gradients of the anchors (and, in
 *   the batch form, of the gallery rows), projects them through the normalisation as reid_cross_triplet_bwd does (G / eps where
 *   |x| < eps) and leaves Hq [P*N, D], Hg [P, Mg, D] at the head of ws: everything the backward needs, so an enqueue or a second
 *   forward into another ws between the forward and the backward does not change the gradient.
 *   reid_smooth_ap_bwd: dq[p*N + i] = gscale[p] * Hq[p*N + i], dg[j] = sum over p ascending of gscale[p] * Hg[p, j]; dq [P*N, D]
 *   (lddq) and dg [Mg, D] (lddg) are OVERWRITTEN (invalid rows with zeros, padding columns untouched); ws must come from a forward
 *   with with_grad = 1.
 * Requirements: those of reid_cross_triplet_fwd / _bwd for P, N, Mg, D, the leading dimensions and eps; 1 <= Ga, Gb <= 8192, ldga /
 * ldgb multiples of 4 and >= D, tau finite and > 0, normalize / gallery_grad / with_grad 0 or 1, q, g, ga, gb, ws, dq, dg 16-byte
 * aligned.  Anything else: REID_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t reid_smooth_ap_ws_floats(int32_t P, int32_t N, int32_t Mg, int32_t D, int32_t Ga, int32_t Gb, int32_t with_grad);
int reid_smooth_ap_fwd(const float* q, int32_t ldq, const float* g, int32_t ldg, const int64_t* q_label, const int64_t* g_label,
                       const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg, int32_t D, float tau,
                       int32_t normalize, float eps, const float* ga, int32_t ldga, const int64_t* ga_label, const uint8_t* ga_valid,
                       int32_t Ga, const float* gb, int32_t ldgb, const int64_t* gb_label, const uint8_t* gb_valid, int32_t Gb,
                       int32_t gallery_grad, int32_t with_grad, float* q_ap, int32_t* q_npos, float* g_ap, int32_t* g_npos, float* ws,
                       float* result, void* stream);
int reid_smooth_ap_bwd(const uint8_t* q_valid, const uint8_t* g_valid, int32_t P, int32_t N, int32_t Mg, int32_t D, const float* ws,
                       const float* gscale, float* dq, int32_t lddq, float* dg, int32_t lddg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hybrid memory loss (SpCL: Ge et al., "Self-paced Contrastive Learning with Hybrid Memory", NeurIPS 2020, sections 3.1-3.2; the
 * reference has no such loss; csrc/hybrid_nce.hip): the memory behind the cluster-NCE block's forward and
 * backward when EVERY instance trains -- a cluster is a class, an un-clustered instance is a class of its own.  All fp32.
 *   State: V [M, D] (ldv) holds one unit entry per training instance and persists across re-clusterings; cls [M] (host side) the
 *   class of every instance in 0..C-1, every class with at least one member; the members of class c are order[offsets[c]] ..
 *   order[offsets[c + 1] - 1] in ASCENDING instance index (order [M], offsets [C + 1] int64); n_c = their number.
 *   Table T [C, D], contiguous: per column d
 *     T_c[d] = fl( fl(sum of V_i[d] over the members i of c, added one by one in ascending i, fp32, not fused) / float(n_c) ),
 *   the sum starting from the first member; the rows are NOT renormalised (SpCL's mean; |T_c| <= 1 up to rounding); a singleton
 *   class is its entry, bit for bit.
 *   Loss: x [S*N, D] with S sides stacked (row r = s*N + n), index [N] int64 shared by the sides (the dataset row of each
 *   instance), valid [S*N] or NULL.  A row is USED when it is valid and 0 <= index < M; its label is y_r = cls[index_n];
 *   loss = mean over the used rows of lse_c(x^_r . T_c / tau) - x^_r . T_y / tau, 0 when no row is used.  The mean of dot products
 *   is the dot product with the mean, so forward and backward ARE reid_cluster_nce_fwd / reid_cluster_nce_bwd with table = T,
 *   K = C and labels[n] = cls[index[n]] (-1 for an index outside 0..M-1).
 *   reid_class_means: T from (V, order, offsets) by the formula above, one workgroup per class; an empty class gets zeros.
 *   Update, after the forward, with what the forward had (row_loss, its ws): a row CONTRIBUTES when it is used and its row_loss is
 *   finite.
 *   reid_hybrid_update_instances: for every instance with a contributing row, over its contributing rows in ascending r (the
 *   sides of an instance in side order, an index that appears twice in a side in row order), with x^_r from ws:
 *     v = momentum * v + (1 - momentum) * x^_r;  v = v / max(|v|, 1e-12).
 *   The wave of the instance's lowest contributing row is the only reader and writer of that entry; other entries keep their bits.
 *   reid_hybrid_refresh_classes (labels = the gathered labels the forward had; after reid_hybrid_update_instances in stream order):
 *   every class with a contributing row has its row of T re-formed from the UPDATED V by the table formula, by the workgroup of the
 *   class's lowest contributing row, the only writer of that row; untouched classes keep their bits.  After any number of steps T
 *   equals reid_class_means of V bit for bit.
 *   No atomics: two runs give the same bits in V and T.  Nothing is allocated, synchronised or read back.
 * Requirements: 1 <= S <= 9, 1 <= N <= 8192, D % 32 == 0, 32 <= D <= 1024, C >= 1, C*D < 2^31, M >= 1 (rows of V are addressed in
 * 64 bits), ldv a multiple of 4 and >= D, V, T and ws 16-byte aligned, 0 <= momentum <= 1; every order[t] in 0..M-1 and offsets
 * ascending from 0 (the caller's: they are not read on the host).  Anything else: REID_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------------ */
int reid_class_means(const float* V, int32_t ldv, int64_t M, const int64_t* order, const int64_t* offsets, int32_t C, int32_t D,
                     float* T, void* stream);
int reid_hybrid_update_instances(const int64_t* index, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* row_loss,
                                 const float* ws, float* V, int32_t ldv, int64_t M, float momentum, void* stream);
int reid_hybrid_refresh_classes(const int64_t* labels, const uint8_t* valid, int32_t S, int32_t N, int32_t D, const float* row_loss,
                                const float* V, int32_t ldv, int64_t M, const int64_t* order, const int64_t* offsets, float* T,
                                int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval (train.py:499 + :463; tools/eval_mm_protocol.py:50-53,401-423,622-625):
 *   sim = Q . G^T on L2-normalised rows, per-query top-k in (score desc, index asc) order.
 *   Q [Nq, D], G [Ng, D] bf16 copies drive a tiled MFMA GEMM with an on-chip candidate filter;
 *   survivors are re-scored in fp32 from Qf/Gf so the order equals the fp32 oracle's.
 *   exclude_q/exclude_g (int32 ids, or NULL): entries with equal non-negative id get -1e9
 *   (same-image mask, eval_mm_protocol.py:421-422) and STAY in the ranking, as in the reference's masked_fill + argsort: a query
 *   with fewer than k other rows gets them behind those, in index order, with score -1e9; an id of -1 on either side excludes nothing.
 *   k <= Ng, so a complete list holds k gallery indices >= 0 (never -1).
 *   out_idx int32 [Nq, k], out_score f32 [Nq, k], contiguous (row q at element q k).  ws: reid_topk_ws_bytes(); scratch, may hold anything.
 *   Nq <= 128 with k <= 16, D = 256 or 512, at least 4 k 64-row chunks of gallery (Ng > 256 k - 64; and 4 k <= compute units) and
 *   Nq min(Ng, 8192) >= 6144 (the scan's counters live in the workspace's sample area): the candidate filter is ONE pass of a query-resident
 *   scan kernel (the 16-bit gallery streamed once, the queries as MFMA operands in registers, the bar of each query taken from the
 *   scan's own running maxima) instead of the sample / threshold / tiled filter launches -- same candidate lists contract, same
 *   results, same workspace.  A query whose candidate list overflows (more than 6 k ceil(Ng / 8192) + 64 candidates, clamped to
 *   256 .. 8192; for k <= 32 also more than 512 rows within the filter margin of the k-th score, e.g. a tie group) is marked
 *   out_idx[q, 0] = -2 (the rest of its row is not written) for reid_cosine_topk_exact(_slots).
 * ------------------------------------------------------------------------------------------ */
int64_t reid_topk_ws_bytes(int32_t Nq, int32_t Ng, int32_t k);
/* 1 when reid_cosine_topk takes the query-resident scan for this shape (then also the faster form for 2-4 queries). */
int32_t reid_topk_scan_ok(int32_t Nq, int32_t Ng, int32_t D, int32_t k);
int reid_cosine_topk(const void* Q_bf16, const void* G_bf16, const float* Qf, const float* Gf,
                     int32_t Nq, int32_t Ng, int32_t D, int32_t k, const int32_t* exclude_q,
                     const int32_t* exclude_g, void* ws, int32_t* out_idx, float* out_score, void* stream);
/* Exact fp32 pass for the queries reid_cosine_topk flagged with out_idx[q][0] == -2 (candidate list
 * overflow, e.g. thousands of near-duplicates); scratch holds Nq*Ng floats; other queries are untouched. */
int reid_cosine_topk_exact(const float* Qf, const float* Gf, int32_t Nq, int32_t Ng, int32_t D, int32_t k,
                           const int32_t* exclude_q, const int32_t* exclude_g, float* scratch, int32_t* out_idx,
                           float* out_score, void* stream);
/* The same exact pass without reading the flags back: the flagged queries are compacted on the device into `slots` (int32 [1 + n_slots]:
 * count, then query ids) and EVERY listed query is resolved by the one call -- list entry e uses scratch row e (scratch: n_slots * Ng
 * floats; touched only for flagged queries).  n_slots >= Nq guarantees that no -2 marker survives the call; with a smaller list the
 * queries beyond it keep their marker and slots[0] (> n_slots) says so. */
int reid_cosine_topk_exact_slots(const float* Qf, const float* Gf, int32_t Nq, int32_t Ng, int32_t D, int32_t k,
                                 const int32_t* exclude_q, const int32_t* exclude_g, int32_t n_slots, int32_t* slots,
                                 float* scratch, int32_t* out_idx, float* out_score, void* stream);
/* The reference's one-query-at-a-time form (tools/eval_mm_protocol.py:401-455: sim = q @ G.T; argsort) for a handful of
 * queries: ONE pass over the fp32 gallery (Ng*D*4 bytes, HBM-bound) instead of the batched pipeline's launch chain.  Same
 * fp32 scores and the same (score desc, index asc) lists as reid_cosine_topk.  Allowed when reid_topk_stream_ok() returns 1
 * (Nq <= 4, k <= 32, D a multiple of 256 up to 1024).  ws: reid_topk_stream_ws_bytes(k) bytes of scratch for the call: the scan kernel
 * writes every per-workgroup list entry the merge kernel then reads, so the buffer may hold anything on entry (its last 256 bytes are
 * not used: they held the arrival counter of an earlier one-launch form and stay part of the size).  No query is ever flagged. */
int32_t reid_topk_stream_ok(int32_t Nq, int32_t Ng, int32_t D, int32_t k);
int64_t reid_topk_stream_ws_bytes(int32_t k);
int reid_cosine_topk_stream(const float* Qf, const float* Gf, int32_t Nq, int32_t Ng, int32_t D, int32_t k,
                            const int32_t* exclude_q, const int32_t* exclude_g, void* ws, int32_t* out_idx,
                            float* out_score, void* stream);
/* fp32 C[M,N] = act(alpha * op(A).op(B) + bias[n]) + beta*C on the vector ALU with arbitrary element strides
 * (A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]); the small exact GEMMs of the head
 * (models/model.py:57-77,152-162) and of the SDM loss.  act: REID_ACT_NONE, _GELU_ERF, _QUICK_GELU or _RELU; the RELU epilogue is
 * torch.relu (a NaN stays NaN).  beta == 0: C is not read.  K > 0, ldc >= N.  The K range is split over the 8 (at most 256 tiles of
 * 32 x 32) or 4 waves of a workgroup and reduced in a fixed order: bit-reproducible. */
int reid_sgemm(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int64_t sam, int64_t sak,
               int64_t sbk, int64_t sbn, int32_t ldc, float alpha, float beta, const float* bias, int32_t act,
               void* stream);
/* ------------------------------------------------------------------------------------------
 * Small fp32 pieces of the head: SemanticDisentanglementModule.forward (models/model.py:57-77) and
 * FeatureFusion.forward (:113-183) on [B,512] / [B,M<=8,512] tensors.
 *   reid_eltwise_f32: op 0 out=x+alpha*y, 1 relu(x), 2 relu' (x pre-activation, y = dy), 3 erf-GELU(x),
 *                     4 y*GELU'(x), 5 x*y, 6 nan_to_num(x, 0, 1e4, -1e4) (model.py:165), 7 dropout multiplier from a uniform draw x:
 *                     1/(1-alpha) where x >= alpha, else 0 (out may be x).  relu and relu' are torch's on non-finite input: relu(NaN)
 *                     = NaN, relu' is 0 where x <= 0 and dy elsewhere (NaN and +inf included) -- the SDM module's ReLU (model.py:42)
 *                     is not followed by nan_to_num, so a diverged activation must stay visible to the loss's isfinite checks
 *   reid_small_attn_fwd/bwd: softmax(q k^T / 8 + key-padding mask) v over S <= 8 tokens, head_dim 64, fp32
 *                     (nn.MultiheadAttention, model.py:152-155); qkv [n_seq*S, ld] = q|k|v; probs [n_seq, heads, 8, 8] saved;
 *                     drop (optional, same layout as probs): attention-dropout multipliers 0 or 1/keep applied to the
 *                     probabilities after the softmax (nn.MultiheadAttention(dropout=0.1), model.py:35,95).
 *                     ld >= 3*heads*64 (also lddqkv), ldo >= heads*64.  probs[item, i, j]: rows i < S are written, with +0 for masked
 *                     keys and for j >= S; rows i >= S are not.  A sequence whose keys are ALL masked gives NaN in its rows of out and
 *                     probs (what torch's softmax over nothing gives), and only there
 *   reid_masked_mean: out[b,:] = sum_m mask[b,m] x[b,m,:] / max(sum_m mask[b,m], 1) (model.py:168-178); backward != 0:
 *                     x = dout [B,D], out = dx [B,M,D] (all M rows written, +0 where mask == 0); B <= 65535
 * ------------------------------------------------------------------------------------------ */
int reid_eltwise_f32(int32_t op, const float* x, const float* y, float* out, int64_t n, float alpha, void* stream);
int reid_small_attn_fwd(const float* qkv, int32_t ld, const uint8_t* key_mask, const float* drop, float* out, int32_t ldo,
                        float* probs, int32_t n_seq, int32_t S, int32_t heads, void* stream);
int reid_small_attn_bwd(const float* qkv, int32_t ld, const float* probs, const float* drop, const float* dout, int32_t ldo,
                        float* dqkv, int32_t lddqkv, int32_t n_seq, int32_t S, int32_t heads, void* stream);
int reid_masked_mean(const float* x, const float* mask, float* out, int32_t B, int32_t M, int32_t D, int32_t backward,
                     void* stream);
/* L2-normalise rows (F.normalize, train.py:442): x f32 [rows, D] -> y = x * scale / max(||x||, eps) as f32 and/or bf16 (one ldy for both).
 * D % 4 == 0, D <= 1024; ldx and ldy multiples of 4 and >= D (16-byte accesses). */
int reid_l2norm_rows(const float* x, int32_t ldx, float* y, void* y_bf16, int32_t ldy, int32_t rows, int32_t D,
                     float eps, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step of the training driver: train.py:85-96 (_sanitize_grads),
 * :975-1047 (gradient norm, adaptive / fixed clip, optimizer.step()) with torch.optim.AdamW semantics
 * (decoupled weight decay, bias correction, no amsgrad), as three sync-free launches over a DEVICE table of
 * reid_opt_entry records (one per trainable flat fp32 buffer, 16-byte aligned; g == NULL skips the entry):
 *   reid_opt_sumsq  non-finite gradient entries := 0 in place; per-workgroup partial sums of g^2 and counts -> ws
 *   reid_opt_clip   state[1] = ||g||_2 (fixed summation order), state[3] = max_norm, state[2] = clip coefficient
 *                   min(1, max_norm / (||g|| + 1e-6)) (torch.nn.utils.clip_grad_norm_), state[4] = #non-finite;
 *                   adaptive != 0: train.py:981-1001 -- when record != 0 the norm is appended to the history
 *                   (state[5] = count, state[6..15] = last ten), max_norm = min(3, max(0.5, 1.15 * percentile70(last ten)))
 *                   once more than ten norms were recorded, else 1.0; adaptive == 0: max_norm = fixed_max_norm
 *   reid_opt_adamw  p, exp_avg, exp_avg_sq updated with gradient g * (*coef) (coef may be NULL = 1); step counts from 1;
 *                   step == 0: the step counter and bias corrections live in state[16..18] and advance on the device, and
 *                   reid_opt_clip's record < 0 means "record when (device batch counter state[19]) % (-record) == 0" -- the
 *                   forms a captured HIP graph replays;
 *                   zero_grad != 0 clears g in the same pass (optimizer.zero_grad at the next accumulation window)
 * An entry with g == NULL is skipped by every kernel: its p, exp_avg and exp_avg_sq are not touched, and reid_opt_sumsq writes
 * zeros for its partials (ws never keeps stale values).  The squares are summed in fp32 within a workgroup (as clip_grad_norm_
 * does on fp32 tensors): a g * g that overflows fp32 gives ||g|| = inf and a clip coefficient of 0.
 * Refused before any launch: a null table (sumsq, adamw), ws (sumsq, clip) or state (clip), n_entries < 1 (or > 65535, the grid's y
 * extent), fixed_max_norm that is not > 0 (NaN included), beta1 or beta2 outside [0, 1), eps that is not > 0, step < 0, step == 0
 * without state.  No atomics, nothing is allocated, nothing is synchronised; grid = 128 x n_entries workgroups.
 * ------------------------------------------------------------------------------------------ */
typedef struct reid_opt_entry {
    float* p; float* g; float* exp_avg; float* exp_avg_sq;
    int64_t n;
    float lr, weight_decay;
} reid_opt_entry;
int32_t reid_opt_entry_bytes(void);
int32_t reid_opt_ws_floats(int32_t n_entries);
int32_t reid_opt_state_floats(void);
int reid_opt_sumsq(const void* table, int32_t n_entries, float* ws, void* stream);
int reid_opt_clip(const float* ws, int32_t n_entries, float* state, int32_t adaptive, float fixed_max_norm,
                  int32_t record, void* stream);
int reid_opt_adamw(const void* table, int32_t n_entries, const float* coef, float beta1, float beta2, float eps,
                   int32_t step, int32_t zero_grad, float* state, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exponential moving average of the trainable weights (csrc/ema.hip): the model the evaluator scores and the best checkpoint is
 * chosen on.  A DEVICE table of reid_ema_entry records of its own (parameter p, shadow s, both flat fp32 and 16-byte aligned, n
 * elements), so buffers reid_opt_adamw never sees (BatchNorm running statistics) can be averaged by the same launch.
 *   reid_ema_update  per element s := s + w * (p - s), the difference, the product and the sum each rounded once to fp32 (never
 *                    contracted into a fused multiply-add: a float32 loop on the host reproduces the bits);
 *                    w = (float)(1.0 - d_t), d_t = min((double)decay, (1 + t) / (10 + t)) when warmup != 0, else (double)decay,
 *                    evaluated in double; t = 1-based number of the optimizer step just taken: step >= 1 gives it from the host,
 *                    step == 0 reads it from state[16], the counter reid_opt_adamw(step == 0) has advanced on the same stream --
 *                    the form a captured HIP graph replays.  state is only read, and only when step == 0.
 *   reid_ema_swap    exchanges p[i] and s[i] IN PLACE as raw 32-bit words (NaN payloads, -0 and denormals survive): every pointer
 *                    held elsewhere -- the optimizer table, a captured graph's kernel arguments, views of the parameters -- stays
 *                    valid, and a second swap restores both sides exactly.
 * Refused before any launch: decay outside (0, 1), a null table, n_entries < 1 (or > 65535, the grid's y extent), step < 0, step == 0
 * without state.  No atomics, nothing is allocated, nothing is synchronised; grid = 128 x n_entries workgroups.
 * ------------------------------------------------------------------------------------------ */
typedef struct reid_ema_entry {
    float* p; float* s;
    int64_t n;
} reid_ema_entry;
int32_t reid_ema_entry_bytes(void);
int reid_ema_update(const void* table, int32_t n_entries, float decay, int32_t warmup, int32_t step, const float* state,
                    void* stream);
int reid_ema_swap(const void* table, int32_t n_entries, void* stream);

/* ------------------------------------------------------------------------------------------
 * AP / CMC from fp32 similarity rows: the metric half of rank_and_metrics,
 * tools/eval_mm_protocol.py:401-469 (and _reid_map, train.py:450-479) without sorting the gallery.
 *   scores  f32 [nq, ld] (ld % 4 == 0, 16-byte aligned): cosine similarities of nq queries against Ng gallery rows
 *   g_pid   i32 [Ng]; g_img i32 [Ng] image ids (NULL or -1 = none)
 *   q_pid   i32 [nq]; q_slot i32 [nq] = row of the query's pid in the CSR below, -1 if the pid has no gallery row
 *   q_excl  i32 [nq, 4] image ids whose gallery rows are ignored for that query (-1 = unused; NULL = no masking)
 *   csr_off i32 [n_pid + 1], csr_idx i32 [Ng]: gallery rows grouped by pid
 * outputs per query: ap f64 (0 when there is no positive), rank1 i32 = rank of the best positive (CMC@k = rank1 <= k),
 *   npos i32 = number of unmasked positives (0: the reference skips the query; -1: more than 8192, not evaluated).
 *   max_pos = length of the longest CSR row (sizes the LDS list of positives).
 * Ranking rule: score descending, gallery index ascending on ties (a stable descending argsort); masked rows rank last.
 * ------------------------------------------------------------------------------------------ */
int reid_rank_metrics(const float* scores, int64_t ld, const int32_t* g_pid, const int32_t* g_img,
                      const int32_t* q_pid, const int32_t* q_slot, const int32_t* q_excl, const int32_t* csr_off,
                      const int32_t* csr_idx, int32_t nq, int32_t Ng, int32_t max_pos, double* ap, int32_t* rank1,
                      int32_t* npos, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cutoff metrics: what mAP@K, CMC@K and mINP are made of (reference: compute_map / compute_cmc, train.py:101-138, the metric the
 * competition ranks by at K = 100; mINP: Ye et al., TPAMI 2021).  Definitions, for one query: let
 *   rank_0 < rank_1 < ... < rank_{np-1}
 * be the ranks (1-based) of its np unmasked positives in the ranking of reid_rank_metrics -- score descending, gallery index
 * ascending on ties, same-image rows removed.  For a cutoff K >= 1:
 *   hits_K    = #{r : rank_r <= K}
 *   sum_K     = sum over {r : rank_r <= K} of (r + 1) / rank_r, formed in fp64
 *   rank_last = rank_{np-1}
 *   AP@K, norm 'hits' = sum_K / hits_K, a query with hits_K == 0 left out of the mean (compute_map of the reference)
 *   AP@K, norm 'min'  = sum_K / min(K, np) over every query with np > 0 (the usual truncated AP)
 *   CMC@K = (rank_0 <= K);  INP = np / rank_last, mINP its mean over the queries with np > 0.
 * The divisions and means are the caller's (evaluate.cutoff_summary); the kernels return hits, sum and the ranks.
 *
 * reid_rank_metrics_at: reid_rank_metrics with cutoffs -- the same one-pass kernel, the same arguments, plus
 *   cutoffs   i32 [n_cut] ON THE HOST, 1 <= n_cut <= REID_METRICS_MAX_CUTOFFS, each >= 1, strictly ascending; a cutoff above Ng is
 *             allowed.  They travel by value in the kernel's parameters: the array may be reused as soon as the call returns.
 *   rank_last i32 [nq], hits i32 [nq, n_cut], sum_at f64 [nq, n_cut], contiguous
 * ap, rank1 and npos are bit for bit those of reid_rank_metrics on the same rows.  A query without a positive (npos = 0) or with more
 * than 8192 (npos = -1) writes zeros to the three new outputs.  The new sums are reduced in the fixed order of ap (lane shuffles,
 * then the four wave partials): deterministic; no atomics beyond the integer LDS counters of reid_rank_metrics.
 * ------------------------------------------------------------------------------------------ */
#define REID_METRICS_MAX_CUTOFFS 8
int reid_rank_metrics_at(const float* scores, int64_t ld, const int32_t* g_pid, const int32_t* g_img,
                         const int32_t* q_pid, const int32_t* q_slot, const int32_t* q_excl, const int32_t* csr_off,
                         const int32_t* csr_idx, int32_t nq, int32_t Ng, int32_t max_pos, const int32_t* cutoffs,
                         int32_t n_cut, double* ap, int32_t* rank1, int32_t* npos, int32_t* rank_last, int32_t* hits,
                         double* sum_at, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact top-k lists of fp32 score rows (csrc/select.hip): the ranked lists of the rows reid_rank_metrics scores, without a sort
 * of the row.
 *   scores  f32 [nq, ld], ld >= n, ld % 4 == 0, base 16-byte aligned (what reid_rank_metrics accepts and the re-ranking kernels
 *           write); columns >= n are never candidates and may hold any bits, NaN and +inf included
 *   g_img   i32 [n], q_excl i32 [nq, 4]: when BOTH are given, column j is dropped for row q iff g_img[j] >= 0 and g_img[j] is one of
 *           q_excl[q, 0..3] (reid_rank_metrics' exclusion); either NULL = no masking
 *   out_idx i32 [nq, k], out_score f32 [nq, k], contiguous: position r of row q is the r-th entry of a stable descending sort of
 *           scores[q, :n] restricted to the eligible columns; the score is the unchanged bits of scores[q, idx]; positions at or
 *           beyond the number of eligible columns hold index -1 and score -inf
 * Order: by key descending, then column ascending; key(x) is the order-preserving u32 image of x + 0.0f (-0 and +0 are equal):
 *   bits | 0x80000000 for non-negative values, ~bits for negative ones, 0xFFFFFFFF for every NaN (NaNs come first and are equal
 *   to each other) -- the order of torch.sort(descending=True, stable=True).
 * Limits: 1 <= k <= REID_ROWS_TOPK_MAX_K (k > n is allowed), nq >= 1, 1 <= n < 2^31; anything else is refused before a launch.
 * One workgroup per row; deterministic (integer LDS counters only); nothing is allocated, nothing is synchronised.
 * ------------------------------------------------------------------------------------------ */
#define REID_ROWS_TOPK_MAX_K 1024
int reid_rows_topk(const float* scores, int64_t ld, int32_t nq, int32_t n, int32_t k, const int32_t* g_img,
                   const int32_t* q_excl, int32_t* out_idx, float* out_score, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cutoff metrics of ranked lists (csrc/list_metrics.hip): hits and sum of the definitions above from the first k gallery rows of a
 * ranking -- the lists of reid_rows_topk / reid_cosine_topk*, or of a submission file -- instead of from score rows.
 *   idx     i32 [nq, k], contiguous, 1 <= k <= REID_ROWS_TOPK_MAX_K: position t of row q is the gallery row ranked (t + 1)-th;
 *           -1 = no entry, allowed only behind the last entry
 *   g_pid, g_img, q_pid, q_slot, q_excl, csr_off, csr_idx: as in reid_rank_metrics; Ng = number of gallery rows
 *   cutoffs i32 [n_cut] ON THE HOST (by value in the kernel's parameters): 1 <= n_cut <= REID_METRICS_MAX_CUTOFFS, each >= 1,
 *           strictly ascending and <= k -- a list of k entries says nothing about a rank beyond k; refused before the launch
 * outputs per query:
 *   npos    i32 [nq]: the unmasked positives IN THE GALLERY, counted from the CSR under the exclusion (what norm 'min' divides by)
 *   rank1   i32 [nq]: the position of the first hit, 0 when the list holds none
 *   hits    i32 [nq, n_cut], sum_at f64 [nq, n_cut]
 *   status  i32 [nq]: 0, or a sum of REID_LIST_BAD_* -- the query's other outputs are then all zero
 * Positions: an entry whose gallery row the query excludes (g_img / q_excl) is SKIPPED and the positions behind it move up by one,
 * so a list is scored as the ranking with the same-image rows removed.  Lists of reid_rows_topk under the same exclusion hold no
 * such entry; a foreign list may.
 * Malformed lists: an index below -1 (REID_LIST_BAD_NEGATIVE), an index >= Ng (REID_LIST_BAD_RANGE), an entry behind a -1
 * (REID_LIST_BAD_ORDER).  Every index is checked before g_pid / g_img are read: nothing is read out of bounds.  A gallery row
 * listed twice is NOT detected here (ProtocolEvaluator.score_lists checks it with a sort).
 * One wave per query; 64 positions at a time: ballots of the counted entries and of the hits, positions by popcount, running
 * carries across the chunks; fp64 sums in a fixed shuffle order per chunk, chunks added in order: deterministic.  No atomics, no LDS,
 * nothing is allocated, nothing is synchronised or read back.
 * ------------------------------------------------------------------------------------------ */
#define REID_LIST_BAD_NEGATIVE 1
#define REID_LIST_BAD_RANGE 2
#define REID_LIST_BAD_ORDER 4
int reid_list_metrics(const int32_t* idx, int32_t nq, int32_t k, const int32_t* g_pid, const int32_t* g_img,
                      const int32_t* q_pid, const int32_t* q_slot, const int32_t* q_excl, const int32_t* csr_off,
                      const int32_t* csr_idx, int32_t Ng, const int32_t* cutoffs, int32_t n_cut, int32_t* npos,
                      int32_t* rank1, int32_t* hits, double* sum_at, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image transforms of the training input (datasets/dataset.py:284-307, train.py:1634-1641; eval: dataset.py:300-307,
 * tools/eval_mm_protocol.py:171-173), bit-exact against PIL + torch for given parameters, per image in this order:
 *   Image.crop(box).resize((S, S), BILINEAR) -> horizontal flip -> ImageEnhance.Brightness / .Contrast (Image.blend) in the
 *   drawn order -> ToTensor + Normalize (lut f32 [3, 256] = (v / 255 - mean[c]) / std[c] computed by torch on fp32) ->
 *   RandomErasing(value=0) over the erase box of the output; an empty slot (absent modality) is all zeros.
 *   src   uint8 RGB HWC images packed into one buffer of src_bytes bytes
 *   table / host_table  int32 [n, REID_AUG_FIELDS], the same entries on the device (read by the kernels) and on the host
 *         (validated before any launch): off_lo, off_hi (byte offset of the image in src), H, W, crop x, crop y, crop w,
 *         crop h, flags (reid_aug_flag), brightness factor, contrast factor (fp32 bit patterns; 1.0 = identity), erase x,
 *         erase y, erase w, erase h (w = 0: no erase), 0
 *   ws    scratch of reid_augment_ws_bytes(n, S) bytes, 16-byte aligned; out f32 [n, 3, S, S], 16-byte aligned
 * Limits: 4 <= S <= 1024, S % 4 == 0; 1 <= H, W <= 8192; crop inside the image; erase box inside S x S.
 * ------------------------------------------------------------------------------------------ */
#define REID_AUG_FIELDS 16
typedef enum { REID_AUG_FLIP = 1, REID_AUG_CONTRAST_FIRST = 2, REID_AUG_EMPTY = 4 } reid_aug_flag;
int64_t reid_augment_ws_bytes(int32_t n, int32_t S);
int reid_augment_images(const void* src, int64_t src_bytes, const int32_t* table, const int32_t* host_table, int32_t n,
                        int32_t S, const float* lut, void* ws, int64_t ws_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Query expansion (AQE, Chum et al. ICCV 2007; alpha-QE, Radenovic et al. TPAMI 2018) and database-side augmentation (DBA) in
 * one call (csrc/expand.hip): every row becomes itself plus a weighted sum of the table rows its ranked list names.  The reference
 * has neither; this comment is the definition (DESIGN.md "Query expansion and database-side augmentation").
 *   x      f32 [rows, ldx >= D]  the rows being expanded, L2-normalised by the caller
 *   table  f32 [M, ldt >= D]     the rows the lists index (the gallery)
 *   nbr i32, score f32 [rows, ldn >= kl]  row i's list, score descending, as reid_cosine_topk* / reid_rows_topk write it
 *   out    f32 [rows, ldo >= D]; columns >= D and rows >= rows are not written
 * Eligibility: the kl entries of row i are walked in list order.  An entry is eligible when 0 <= nbr < M, its score is not NaN,
 *   and nbr != self_base + i when self_base >= 0 (DBA: row i of a gallery chunk that starts at row self_base is its own leading
 *   term; it is recognised by index, not by position, so an exact duplicate that outranks it on the index tie rule is still used);
 *   self_base = -1: no such row.  The first k eligible entries are used.  The table row of an entry that is not used is never read.
 * Weight: alpha == 0: w = 1 (AQE).  alpha in 1..REID_EXPAND_MAX_ALPHA: with s = max(score, 0), w = s; repeat alpha - 1 times:
 *   w = w * s (fp32 products).  A used entry with w == 0 is not added at all.
 * Raw sum, per column d: raw = x[i][d]; then for each added entry in list order raw = raw + w * table[nbr][d], the product rounded to
 *   fp32 before the sum (no fused multiply-add): a float32 loop on the host reproduces the bits.
 * Output: normalize == 0: out = raw.  normalize == 1: out = raw * (1 / max(sqrt(sum_d raw^2), eps)), evaluated as reid_l2norm_rows
 *   does (per-lane partial sums, a wave reduction, sqrtf, one division, one product per element).
 * Limits: 1 <= k <= kl <= REID_EXPAND_MAX_LIST, D % 4 == 0, D <= 1024 (reid_l2norm_rows' limits), rows >= 1, M >= 1, eps >= 0;
 *   ldx, ldt, ldo multiples of 4 and >= D; x, table, out 16-byte aligned.  out must not overlap table or x: out == table and
 *   out == x are refused, any other overlap is the caller's to avoid (rows are read while other rows are written).  Anything else is
 *   refused before a launch.  One wavefront per row; 64-bit row offsets; deterministic (no atomics); nothing is allocated or
 *   synchronised.
 * ------------------------------------------------------------------------------------------ */
#define REID_EXPAND_MAX_LIST 64
#define REID_EXPAND_MAX_ALPHA 16
int reid_expand_rows(const float* x, int64_t ldx, const float* table, int64_t ldt, int32_t M, const int32_t* nbr,
                     const float* score, int32_t ldn, int32_t kl, int32_t k, int32_t alpha, int64_t self_base,
                     int32_t normalize, float eps, float* out, int64_t ldo, int32_t rows, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cosine-margin identity heads with a fused label-smoothed CE (csrc/margin_ce.hip; the reference has none: its identity branch is
 * a plain Linear followed by label-smoothed CE).  All fp32, no atomics (two runs give the same bits), nothing allocated, nothing
 * read back.  No alignment or leading-dimension multiple is asked for; padding columns are neither read nor written.
 *   x f32 [B, ldx >= D] (not assumed unit), W f32 [C, ldw >= D], scale s > 0, margin m, eps >= 0 (1e-12 = F.normalize's default).
 *   rx_b = 1 / max(|x_b|, eps), rw_c = 1 / max(|W_c|, eps), cos_bc = (x_b . W_c) rx_b rw_c, logits l_bc = s cos_bc.
 *   A row whose norm is below eps is divided by eps, and its gradient has no projection term (F.normalize).
 * The dot products of this head cancel (a class centre against an unrelated row; a gradient that is orthogonal to its own row), so
 * products and sums are formed in fp64 and every output is rounded to fp32 once.
 * reid_cos_logits_fwd       rx f64 [B], rw f64 [C] (kept for the backward) and logits f32 [B, ldl >= C]; two launches (inverse
 *       norms; 32 x 32 tiles of the products with the scaling as their epilogue).
 * reid_cos_logits_bwd_prep  from g = dL/dl f32 [B, ldg >= C]: G f64 [B, D] = g (rw . W), G_b = sum_c g_bc rw_c W_c (NULL: dx is not
 *       wanted; W and rw are then not read) and H f64 [C, D] = g^T (rx . x), H_c = sum_b g_bc rx_b x_b (NULL: dW is not wanted), each
 *       summed in a fixed order; one launch.
 * reid_cos_logits_bwd_fix   dx_b = s rx_b (G_b - xh_b (xh_b . G_b)), xh_b = x_b rx_b, and dW_c = s rw_c (H_c - wh_c (wh_c . H_c)),
 *       wh_c = W_c rw_c: with dz = s g rx_b rw_c and tb_b = sum_c g_bc l_bc = s xh_b . G_b these are dz W - x_b rx_b^2 tb_b and
 *       dz^T x - W_c rw_c^2 tc_c.  dx f32 [B, lddx >= D] or dW f32 [C, lddw >= D] may be NULL (with its inputs); one launch.
 * Margin logits z' of a row with label y (kind: REID_MARGIN_*; cos = l / s):
 *   COSINE   z' = l (margin ignored)
 *   COSFACE  z'_y = l_y - s m (0 <= m < 1)
 *   ARCFACE  t = clamp(cos_y, -1 + 2^-23, 1 - 2^-23); phi = t cos(m) - sqrt(1 - t^2) sin(m) where t > cos(pi - m), else
 *            t - m sin(pi - m); z'_y = s phi (0 <= m < pi/2).  dphi/dt = cos(m) + t sin(m) / sqrt(1 - t^2), 1 in the fallback, and
 *            0 where the clamp acted (torch.clamp).
 *   CIRCLE   alpha_p = max(1 + m - cos_y, 0), alpha_n = max(cos_c + m, 0), constants of the gradient; z'_y = s alpha_p (cos_y - (1 - m)),
 *            z'_c = s alpha_n (cos_c - m) for c != y (0 <= m < 1)
 *   every other class: z'_c = l_c.
 * Row loss = (1 - e)(lse(z') - z'_y) + e (lse(z') - mean_c z'_c), e = smoothing in [0, 1]; rows with valid == 0 (valid u8 [rows],
 * NULL: all) or a label outside [0, C) are unused: loss 0, gradient 0.
 * reid_margin_ce_fwd   row_loss f32 [rows]; result f32 [3] = (sum of the used rows' losses, their count, the mean = sum /
 *       max(count, 1)), added in fp64 in a fixed order; two launches; z' is never written to memory.
 * reid_margin_ce_bwd   dlogits f32 [rows, lddl >= C] = gs (p - e / C - (1 - e)[c == y]) dz'_c/dl_c, p = softmax(z'),
 *       gs = dloss[0] / max(result[1], 1) (dloss: a device scalar, the cotangent of the mean); unused rows are written as zeros.
 * ------------------------------------------------------------------------------------------ */
#define REID_MARGIN_COSINE 0
#define REID_MARGIN_COSFACE 1
#define REID_MARGIN_ARCFACE 2
#define REID_MARGIN_CIRCLE 3
int reid_cos_logits_fwd(const float* x, int32_t ldx, const float* W, int32_t ldw, int32_t B, int32_t C, int32_t D, float scale,
                        float eps, double* rx, double* rw, float* logits, int32_t ldl, void* stream);
int reid_cos_logits_bwd_prep(const float* g, int32_t ldg, const float* x, int32_t ldx, const float* W, int32_t ldw, const double* rx,
                             const double* rw, int32_t B, int32_t C, int32_t D, double* G, double* H, void* stream);
int reid_cos_logits_bwd_fix(const float* x, int32_t ldx, const double* rx, const double* G, float* dx, int32_t lddx, const float* W,
                            int32_t ldw, const double* rw, const double* H, float* dW, int32_t lddw, int32_t B, int32_t C, int32_t D,
                            float scale, float eps, void* stream);
int reid_margin_ce_fwd(const float* logits, int32_t ld, const int64_t* labels, const uint8_t* valid, int32_t rows, int32_t C,
                       int32_t kind, float scale, float margin, float smoothing, float* row_loss, float* result, void* stream);
int reid_margin_ce_bwd(const float* logits, int32_t ld, const int64_t* labels, const uint8_t* valid, int32_t rows, int32_t C,
                       int32_t kind, float scale, float margin, float smoothing, const float* result, const float* dloss,
                       float* dlogits, int32_t lddl, void* stream);

/* ------------------------------------------------------------------------------------------
 * DBSCAN over fp32 similarity rows (csrc/cluster.hip); the definition is DESIGN.md §22 (the reference has no clustering).
 * Given n rows, a similarity s(i, j) (larger = closer), a threshold thr and min_samples >= 1:
 *   N(i) = {i} + {j < n : s(i, j) >= thr}, compared in fp32 on the bits of row i alone: NaN is never a neighbour, +inf is, and the
 *   row's own column always counts, once.  core(i) <=> |N(i)| >= min_samples.  Cores i, j are joined iff j in N(i) or i in N(j);
 *   clusters are the connected components, named by their smallest core row (the root).  A non-core j takes the smallest root
 *   among the cores i with j in N(i); a row no core reaches is noise.
 * The rows arrive in chunks and are not kept; each chunk becomes its slice of the neighbour CSR:
 *   scores  f32 [nr, ld], ld >= n, ld % 4 == 0, base 16-byte aligned (what reid_rows_topk accepts and the re-ranking kernels write);
 *           columns >= n are never candidates and may hold any bits.  Row r of the chunk is row row0 + r of the matrix:
 *           0 <= row0, row0 + nr <= n.  thr must not be NaN.
 *   reid_dbscan_count   count i32 [nr] = |N(row0 + r)|, core u8 [nr] = (count >= min_samples).
 *   reid_dbscan_fill    rowptr i64 [nr + 1]: offsets into cols i32 [cap] (the caller's exclusive prefix sum of count); writes the
 *           columns of N(row0 + r) strictly ascending from rowptr[r]; never writes at or past rowptr[r + 1] or cap.
 * Components and labels on the CSR of all N rows (rowptr i64 [N + 1], cols i32 [nnz], core u8 [N]); a column outside 0 .. N - 1 is
 * skipped, offsets are clipped to 0 .. nnz:
 *   parent i32 [N], set to parent[i] = i by the caller.  Invariant: parent[x] <= x, and a parent only decreases.
 *   reid_dbscan_hook      for each directed edge (i, j) between two cores with parent[i] != parent[j]:
 *           atomicMin(parent[max(pi, pj)], min(pi, pj)); *changed (i32) grows by one per wave that saw such an edge, and stays
 *           as it is when there was none.
 *   reid_dbscan_compress  parent[x] = the fixed point of x -> parent[x] (at most x steps).
 *           The caller alternates the two until a hook pass leaves *changed untouched: parent[i] is then the root of core i.
 *   reid_dbscan_border    label i32 [N]: atomicMin(label[j], parent[i]) for each core i and each non-core j in N(i); the caller
 *           fills label beforehand (INT32_MAX = noise).
 * Integer atomicMin / atomicAdd only: every output is the same bits in every run.  No kernel waits for another workgroup.  Nothing is
 * allocated, nothing is synchronised or read back.  Anything outside the limits above is refused before a launch.
 * ------------------------------------------------------------------------------------------ */
int reid_dbscan_count(const float* scores, int64_t ld, int32_t nr, int32_t n, int64_t row0, float thr, int32_t min_samples,
                      int32_t* count, uint8_t* core, void* stream);
int reid_dbscan_fill(const float* scores, int64_t ld, int32_t nr, int32_t n, int64_t row0, float thr, const int64_t* rowptr,
                     int32_t* cols, int64_t cap, void* stream);
int reid_dbscan_hook(const int64_t* rowptr, const int32_t* cols, int64_t nnz, const uint8_t* core, int32_t* parent, int32_t N,
                     int32_t* changed, void* stream);
int reid_dbscan_compress(int32_t* parent, int32_t N, void* stream);
int reid_dbscan_border(const int64_t* rowptr, const int32_t* cols, int64_t nnz, const uint8_t* core, const int32_t* parent,
                       int32_t* label, int32_t N, void* stream);

/* ------------------------------------------------------------------------------------------
 * k-reciprocal re-ranking (Zhong et al., CVPR 2017) of pooled unit rows X = [Q; G], N = Nq + Ng <= 65 536, dense; the
 * definition is DESIGN.md "k-reciprocal re-ranking" (the reference has none).  kh = round-half-to-even(k1 / 2).
 *   nbr   i32 [N, ldn >= k1 + 1]: row i of the pooled ranking (score descending, index ascending; i itself is an entry)
 *   reid_rerank_weights   R(i, k) = { j in nbr[i, :k+1] : i in nbr[j, :k+1] };  R*(i) = R(i, k1) plus every R(j, kh),
 *         j in R(i, k1), with 3 |R(j, kh) & R(i, k1)| > 2 |R(j, kh)|;  V[i, c] = exp(x_i.x_c - 1) / sum over R*(i), else 0.
 *         X f32 [N, ldx >= D]; V f32 [N, ldv >= N], columns < N of every row zero-filled by the call.  1 <= k1 <= 64, k1 + 1 <= N.
 *   reid_rerank_expand    V2[i, :N] = (1 / k2) sum_{t < k2} V[nbr[i, t], :N]; 1 <= k2 <= k1 + 1 (k2 = 1 copies V bit for bit);
 *         ldv, ldo multiples of 4, 16-byte aligned.
 *   reid_rerank_jaccard   out[q, g] = (1 - lambda) m / (2 - m) + lambda cosr[q, g], m = sum_{j < N} min(A[q, j], B[g, j]), for
 *         nq rows of A (a query chunk of V2) and Ng rows of B (V2[Nq:]), both non-negative, lda and ldb multiples of 4,
 *         16-byte aligned; cosr f32 [nq, ldc >= Ng]; out f32 [nq, ldo >= Ng], ldo % 4 == 0 (what reid_rank_metrics accepts),
 *         columns >= Ng are not written.
 * All fp32, deterministic (no atomics), nothing allocated or synchronised.
 *
 * The sparse form computes the same V, V2 and out from the same nbr and X, stores the non-zeros only and has no limit on N
 * other than int32 row indices (offsets into the arrays of non-zeros are int64).  W = (k1 + 1)(kh + 2) >= |R*(i)|.
 *   V, padded rows    vcols i32 [N, ldw], vvals f32 [N, ldw], vcnt i32 [N], ldw >= W: row i holds the members of R*(i) once each
 *         (in the order the set is built) with exactly the value the dense call writes; positions >= vcnt[i] are not written.
 *   V2, CSR           rowptr i64 [N + 1], cols i32 [nnz], vals f32 [nnz]: columns strictly ascending inside a row, every value > 0
 *         and the dense call's value bit for bit (the terms present, added in ascending t, then divided by (float)k2).
 *   gallery rows of V2, transposed (CSC of rows Nq .. N - 1)   colptr i64 [N + 1], rows i32 [nnzc] (g = row - Nq, ascending inside
 *         a column), cvals f32 [nnzc].  The caller builds it from the CSR (a stable sort of the column indices).
 *   reid_rerank_weights_sparse   writes the padded rows and vcnt; nothing is zero-filled.
 *   reid_rerank_expand_count     cnt[i] = number of distinct columns in the padded rows nbr[i, t], t < k2: the row lengths of V2.
 *         The caller turns them into rowptr (an exclusive prefix sum) and sizes cols / vals by rowptr[N].
 *   reid_rerank_expand_sparse    fills cols / vals of every row at rowptr[i]; never writes at or past rowptr[i + 1].
 *         Both hold one row's merge in LDS: k2 W <= 8192 entries (REID_RERANK_MERGE_MAX), else REID_ERR_ARG.
 *   reid_rerank_jaccard_sparse   out[q, g] for q < nq and EVERY g < Ng, m summed over the columns both rows hold, in ascending
 *         column order; rowptr points at the first of the nq + 1 offsets of the query chunk (absolute offsets into cols / vals,
 *         which hold nnz entries in all); columns >= Ng of out are not written.  One workgroup owns one out row.  The two
 *         matrices need not come from a pooled problem; an index outside its range is skipped.
 * ------------------------------------------------------------------------------------------ */
#define REID_RERANK_MERGE_MAX 8192
int reid_rerank_weights_sparse(const int32_t* nbr, int32_t ldn, const float* X, int32_t ldx, int32_t* vcols, float* vvals,
                               int32_t* vcnt, int64_t ldw, int32_t N, int32_t D, int32_t k1, void* stream);
int reid_rerank_expand_count(const int32_t* vcols, const float* vvals, const int32_t* vcnt, int64_t ldw, const int32_t* nbr,
                             int32_t ldn, int32_t* cnt, int32_t N, int32_t k1, int32_t k2, void* stream);
int reid_rerank_expand_sparse(const int32_t* vcols, const float* vvals, const int32_t* vcnt, int64_t ldw, const int32_t* nbr,
                              int32_t ldn, const int64_t* rowptr, int32_t* cols, float* vals, int32_t N, int32_t k1, int32_t k2,
                              void* stream);
int reid_rerank_jaccard_sparse(const int64_t* rowptr, const int32_t* cols, const float* vals, int64_t nnz, const int64_t* colptr,
                               const int32_t* rows, const float* cvals, int64_t nnzc, const float* cosr, int64_t ldc, float* out,
                               int64_t ldo, int32_t nq, int32_t Ng, int32_t N, float lambda, void* stream);
int reid_rerank_weights(const int32_t* nbr, int32_t ldn, const float* X, int32_t ldx, float* V, int64_t ldv, int32_t N,
                        int32_t D, int32_t k1, void* stream);
int reid_rerank_expand(const float* V, int64_t ldv, const int32_t* nbr, int32_t ldn, float* V2, int64_t ldo, int32_t N,
                       int32_t k1, int32_t k2, void* stream);
int reid_rerank_jaccard(const float* A, int64_t lda, const float* B, int64_t ldb, const float* cosr, int64_t ldc, float* out,
                        int64_t ldo, int32_t nq, int32_t Ng, int32_t N, float lambda, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REID_HIP_H */
