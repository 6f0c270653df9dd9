/*
 * d2r_hip.h — C ABI of libd2r_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the D2R
 * dual-branch dynamic-routing forward/backward hot path.
 *
 * The reference (SorF520/D2R) has NO plugin / operator / FFI layer: its boundary is two Python classes
 * (`UnimoModelF.forward`, models/unimo_model.py:149-162; `MSDTrainer`, modules/train.py:53-328) and every
 * op is an ATen call.  This header is therefore the seam a maintainer of the reference would bind with
 * `ctypes`: each entry point replaces one ATen op *sequence* of the reference, cited
 * per function as reference file:line.
 *
 * Conventions:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless named `h_*`;
 *   - kernels are enqueued on the caller's `stream` (a hipStream_t passed as void*); the library never
 *     allocates, frees, synchronises or takes ownership — workspaces are caller-provided;
 *   - return 0 on success, a negative d2r_status on error; d2r_last_error() gives a thread-local message;
 *   - dtype of activations/weights `T` is D2R_F32, D2R_BF16 or D2R_F16 (IEEE half: BASELINE.json configs[4]); every
 *     entry point that says "16-bit" takes either of the two and runs the same kernel with the other MFMA operand type;
 *     accumulation, softmax statistics, router logits, biases, LayerNorm parameters and all reductions are fp32;
 *   - deterministic: fixed reduction order, no float atomics anywhere (the embedding-table gradient is a fixed-order gather-sum).
 */
#ifndef D2R_HIP_H
#define D2R_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { D2R_F32 = 0, D2R_BF16 = 1, D2R_F16 = 2 } d2r_dtype;

typedef enum {
  D2R_OK = 0,
  D2R_ERR_INVALID = -1,     /* bad argument (shape, alignment, null pointer, unsupported combination) */
  D2R_ERR_LAUNCH = -2,      /* hipGetLastError() after launch */
  D2R_ERR_WORKSPACE = -3    /* caller-provided workspace too small */
} d2r_status;

typedef enum {
  D2R_ACT_NONE = 0,
  D2R_ACT_RELU = 1,
  D2R_ACT_TANH = 2,
  D2R_ACT_GELU = 3,        /* erf GELU  (BertIntermediate, models/modeling_unimo.py:443-456) */
  D2R_ACT_QUICK_GELU = 4,  /* x*sigmoid(1.702x) (CLIPMLP, models/modeling_unimo.py:121-133) */
  D2R_ACT_TANH_RELU = 5,   /* relu(tanh(x)) = Router activateFunc (models/Router.py:6-8) */
  D2R_ACT_SIGMOID = 6
} d2r_act;

/* A-operand / B-operand storage of d2r_gemm: C[M,N] = sum_k A(m,k) * B(k,n) */
typedef enum {
  D2R_GEMM_NT = 0,  /* A stored [M,K] (k contiguous), B stored [N,K] (k contiguous): y = x W^T (nn.Linear fwd) */
  D2R_GEMM_NN = 1,  /* A stored [M,K], B stored [K,N] (n contiguous): dX = dY W ; O = P V             */
  D2R_GEMM_TN = 2   /* A stored [K,M] (m contiguous), B stored [K,N]: dW = dY^T X ; dV = P^T dO        */
} d2r_gemm_layout;

const char* d2r_version(void);
const char* d2r_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * K11  gemm_bias_act — every nn.Linear of the path, and the attention matmuls, as one MFMA kernel family.
 * Replaces: F.linear (+ReLU/tanh/GELU/quick_gelu, + residual add) e.g. models/SelfAttention.py:29-31,52-53,
 * models/Refinement.py:105-107,133-137, models/XModules.py:300-302, models/Cells.py:145-160,236-246,
 * models/modeling_unimo.py:173-176,217,353-355,411,451,466; torch.bmm/matmul at models/XModules.py:305,310,
 * models/SelfAttention.py:33,39, models/Cells.py:244-246; and their autograd backward (NN / TN layouts).
 *
 *   C[b,h] = epilogue( alpha * A[b,h] x B[b,h] )      batch index z = b*nh + h, pointer offset b*s?b + h*s?h
 *   epilogue(v) = act(v + bias[n]) + residual[m,n]     (then  C = v + beta*C_old  when beta != 0)
 * `preact` (optional) receives v + bias before the activation (needed by GELU backward).
 * All leading dimensions / strides are in ELEMENTS.  A and B have dtype `dtype`; C/residual/preact have
 * `c_dtype`.  bias is fp32 [N] (row b*s_bias_b for batch b) or NULL.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int dtype;      /* d2r_dtype of A and B */
  int c_dtype;    /* d2r_dtype of C, residual, preact */
  int layout;     /* d2r_gemm_layout */
  int act;        /* d2r_act */
  int M, N, K;
  int nb, nh;     /* batch = nb*nh (use 1,1 for a plain GEMM) */
  float alpha, beta;
  const void* A; int64_t lda, sAb, sAh;
  const void* B; int64_t ldb, sBb, sBh;
  void* C;       int64_t ldc, sCb, sCh;
  const float* bias;
  const void* residual; int64_t ldr, sRb, sRh;
  void* preact;  /* same ld/strides as C */
  /* optional scratch for deterministic split-K (GEMMs with few output tiles and a long reduction: weight
   * gradients, M<=32 router/pooler products; 16-bit NT / NN products with K >= 2048 over at most 448 tiles of 128 x 128, whose
   * partial sums meet inside the launch); used only when batch == 1.  NULL disables split-K.  The LAST 4 KiB of the workspace
   * hold the tile counters of the in-launch variant: they must be zero before the first use and are zero again when a launch has
   * finished; launches that share a workspace must be ordered (one stream). */
  void* workspace; size_t workspace_bytes;
  int64_t s_bias_b;  /* bias stride per outer batch index b (grouped linears: one bias row per group); 0 = shared */
  /* TN layout, batch == 1 only: dbias[m] += sum_k A[k,m] (fp32 [M], ACCUMULATED) — the bias gradient of a linear
   * layer computed inside its weight-gradient GEMM (dW = dY^T X reads dY anyway), replacing a separate column-sum
   * launch.  NULL disables. */
  float* dbias;
  /* optional, batch == 1: the result (after bias / act) is multiplied elementwise by d act(grad_act) evaluated at
   * grad_ref[m,n] (dtype and leading dimension of C; the pre-activation for gelu / quick_gelu, the activation
   * output for relu / tanh / sigmoid) — the activation backward of the PREVIOUS linear fused into this dX GEMM. */
  const void* grad_ref;
  int grad_act;
} d2r_gemm_desc;

int d2r_gemm(const d2r_gemm_desc* d, void* stream);
/* `n` INDEPENDENT products enqueued together (no output of one is an operand or an output of another; the caller guarantees it).
 * The 16-bit NT / NN products with at least 128 rows and columns leave as grouped launches of up to 16 problems on the 128 x 128
 * LDS-DMA tiles - the chains of 768 x 768 linears of the routing cells (models/Cells.py:30-255, models/Refinement.py:133-154) are
 * 192-300 tiles each, one partial round of workgroups; four to six of them together fill the chip - and every tile is computed
 * exactly as by d2r_gemm: bit-identical results.  Everything else is launched by d2r_gemm, one by one, in the order given. */
int d2r_gemm_group(const d2r_gemm_desc* descs, int n, void* stream);
/* `count` weight-gradient GEMMs of ONE shape in launches of up to 16 problems:
 *   C_i[M,N] (fp32, ldc) = beta * C_i + A_i^T B_i,   A_i [K,M] (lda), B_i [K,N] (ldb) of dtype;   dbias_i[m] += sum_k A_i[k,m]
 * h_A / h_B / h_C / h_dbias are HOST arrays of device pointers (h_dbias may be NULL).  Replaces `count` d2r_gemm TN
 * calls (dW = dY^T X of the 768x768 linears in models/Cells.py, Refinement.py, SelfAttention.py, XModules.py) that
 * each needed split-K slabs and a reduce launch to fill the chip; the caller defers them, nothing in the backward
 * pass reads a weight gradient.  Deterministic. */
int d2r_gemm_tn_grouped(int dtype, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, const void* const* h_A,
                        const void* const* h_B, float* const* h_C, float* const* h_dbias, int count, float beta,
                        void* stream);
/* Weight gradients of DIFFERENT shapes in one call: problem i is C_i[M_i,N_i] (fp32, ldc_i) = beta * C_i + A_i^T B_i with A_i [K_i,M_i]
 * (lda_i), B_i [K_i,N_i] (ldb_i) of dtype, dbias_i[m] += sum_k A_i[k,m] (h_dbias may be NULL).  All arrays are HOST arrays of `count`
 * entries.  The 16-bit problems with at least 128 rows, columns and reduction rows leave together on 256 x 256 tiles (launches of up
 * to 40 problems: the deferred weight gradients of a whole branch - models/modeling_unimo.py:334-470 and the cells' linears - fill
 * the chip whatever the single shapes are); the rest go through d2r_gemm_tn_grouped shape class by shape class.  No two problems may
 * share an output.  Deterministic. */
int d2r_gemm_tn_grouped_v(int dtype, int count, const int* M, const int* N, const int* K, const int64_t* lda, const int64_t* ldb,
                          const int64_t* ldc, const void* const* h_A, const void* const* h_B, float* const* h_C, float* const* h_dbias,
                          float beta, void* stream);
/* (measurement aids - per-launch timers, kernel-choice overrides, cycle stamps - are declared in d2r_hip_probes.h: not part of the
 * drop-in surface, process-global, not thread-safe; the library itself reads no environment variable) */
/* Data parallelism: there is deliberately NO d2r_comm_* entry point.  The gradient reduction of the path is a sum of the flat
 * fp32 gradient buffer over ranks; the host side (d2r_amd/dp.py) issues it as bucketed torch.distributed collectives - RCCL
 * all-reduce, or reduce-scatter + all-gather per bucket - on a communication stream ordered behind the compute streams.  The
 * data movement is RCCL's over xGMI; nothing of it is arithmetic of this library, so nothing of it sits behind this ABI.  A
 * binding from another host language calls its own RCCL on the same buffers (the 1 / world factor is d2r_adamw_step's grad_scale). */

/* ------------------------------------------------------------------------------------------------
 * Row kernels (fp32 statistics, wave-shuffle reductions)
 * ------------------------------------------------------------------------------------------------ */
/* softmax over the last dim of X[rows, cols] (row stride ld): Y = softmax(scale*X + mask[row / rows_per_mask]).
 * Replaces torch.softmax at models/XModules.py:309 (scale 100/sqrt(768)), models/SelfAttention.py:36,
 * models/Cells.py:245,204 and models/modeling_unimo.py:194,376-385 (additive -10000 key mask, fp32 [*,cols]). */
int d2r_softmax_fwd(int x_dtype, int y_dtype, const void* X, void* Y, int64_t ld, int64_t rows, int cols,
                    float scale, const float* mask, int64_t rows_per_mask, void* stream);
/* dS = scale * P o (dP - rowsum(dP o P)); dS has P's dtype, dP may be fp32 */
int d2r_softmax_bwd(int p_dtype, int dp_dtype, const void* P, const void* dP, void* dS, int64_t ld, int64_t rows,
                    int cols, float scale, void* stream);

/* LayerNorm over D (models/modeling_unimo.py:231,250,283,408,463,742). mean/rstd: fp32 [rows]. */
int d2r_layernorm_fwd(int dtype, const void* X, const float* gamma, const float* beta, float eps, int64_t rows,
                      int D, void* Y, float* mean, float* rstd, void* stream);
size_t d2r_layernorm_bwd_workspace(int64_t rows, int D);
/* dX always; dgamma/dbeta (fp32 [D]) are OVERWRITTEN. workspace: d2r_layernorm_bwd_workspace bytes. */
int d2r_layernorm_bwd(int dtype, const void* dY, const void* X, const float* gamma, const float* mean,
                      const float* rstd, int64_t rows, int D, void* dX, float* dgamma, float* dbeta,
                      void* workspace, size_t workspace_bytes, void* stream);

/* l2norm rows: y = x / (sqrt(sum x^2) + 1e-8)  (eps OUTSIDE the root; models/Cells.py:23-27).  norm: fp32 [rows] */
int d2r_l2norm_fwd(int dtype, const void* X, void* Y, float* norm, int64_t rows, int D, void* stream);
int d2r_l2norm_bwd(int dtype, const void* dY, const void* X, const float* norm, void* dX, int64_t rows, int D,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise kernels (16-byte vectorised)
 * ------------------------------------------------------------------------------------------------ */
/* dX = dY * act'(.)  — `ref` is the activation OUTPUT for relu/tanh/tanh_relu/sigmoid and the PRE-activation
 * for gelu/quick_gelu. */
int d2r_act_bwd(int dtype, int act, const void* dY, const void* ref, void* dX, int64_t n, void* stream);
int d2r_act_fwd(int dtype, int act, const void* X, void* Y, int64_t n, void* stream);
/* out = (a - b)^2 ; da = 2(a-b)dout, db = -da   (models/Cells.py:147,156) */
int d2r_sqdiff_fwd(int dtype, const void* a, const void* b, void* out, int64_t n, void* stream);
int d2r_sqdiff_bwd(int dtype, const void* a, const void* b, const void* dout, void* da, void* db, int64_t n,
                   void* stream);
/* out = a*s + h  (FiLM modulation, models/Refinement.py:136) ; backward gives da, ds (dh = dout) */
int d2r_muladd_fwd(int dtype, const void* a, const void* s, const void* h, void* out, int64_t n, void* stream);
int d2r_muladd_bwd(int dtype, const void* a, const void* s, const void* dout, void* da, void* ds, int64_t n,
                   void* stream);
/* out = g*a + (1-g)*b (GESC gate, models/Cells.py:205) ; backward gives dg, da, db */
int d2r_lerp_fwd(int dtype, const void* g, const void* a, const void* b, void* out, int64_t n, void* stream);
int d2r_lerp_bwd(int dtype, const void* g, const void* a, const void* b, const void* dout, void* dg, void* da,
                 void* db, int64_t n, void* stream);
/* nn.Dropout (models/modeling_unimo.py:330,388,413,468): y[i] = keep(i) ? x[i] / (1-p) : 0, plus add[i] when add != NULL
 * (the skip connection that follows the dropout in BertSelfOutput / BertOutput).  keep(i) is a pure function of
 * (seed, i): the backward pass calls the same entry point on dy with the same seed — no mask is stored. */
int d2r_dropout(int dtype, const void* x, const void* add, void* y, int64_t n, float p, uint64_t seed, void* stream);
/* Stochastic depth (DropPath; an extension, the reference has none) fused with the dropout above and the skip connection, over
 * x [B, per_sample] (bf16, fp16 or fp32; y == x allowed):
 *   y = add + keep_path(b) / (1 - p_path) * dropout_elem(x),  b = i / per_sample,  i in [0, B * per_sample)
 * dropout_elem is d2r_dropout's element mask with (p_elem, seed_elem) at element index i (p_elem = 0: identity).
 * keep_path(b) = rand24(seed_path, b) >= p_path * 2^24, the same counter-based generator applied to the SAMPLE index: a pure function
 * of (seed_path, b).  The backward pass calls the same entry point on dy with add = NULL and the same seeds.
 * A dropped sample is a select, not a multiply: its rows of y are a bit copy of add (+0 without add) and its x is never read, so an
 * inf / NaN in a dropped branch does not reach y.  A kept element is ((keep_elem ? x / (1 - p_elem) : 0) / (1 - p_path)) + add in
 * fp32, rounded once to the dtype; p_path = 0 is bit for bit d2r_dropout.  p_path, p_elem outside [0, 1): D2R_ERR_INVALID, no
 * launch.  B == 0 or per_sample == 0: no-op.  16-byte packs when x, add, y are 16-byte aligned and per_sample is a multiple of the
 * pack width (8 / 4 elements), else element by element; both keep exactly the same elements. */
int d2r_drop_path(int dtype, const void* x, const void* add, void* y, int64_t B, int64_t per_sample, float p_path,
                  uint64_t seed_path, float p_elem, uint64_t seed_elem, void* stream);
int d2r_add(int dtype, const void* a, const void* b, void* out, int64_t n, void* stream);
/* two independent problems of one size in one launch (element for element the arithmetic of two d2r_add / d2r_act_bwd calls): the
 * text / image and a / b pairs of per-sample vectors in the routing cells' backward (models/Cells.py:179-218, :222-255) */
int d2r_add2(int dtype, const void* a1, const void* b1, void* out1, const void* a2, const void* b2, void* out2, int64_t n, void* stream);
int d2r_act_bwd2(int dtype, int act, const void* dY1, const void* ref1, void* dX1, const void* dY2, const void* ref2, void* dX2, int64_t n,
                 void* stream);
/* out[0] = sum_k h_coef[k] * x_k[0]  (n <= 8 fp32 device scalars): loss = CE - w1*JS1 - w2*JS2 */
int d2r_lincomb(const float* const* h_x, const float* h_coef, int n, float* out, void* stream);
/* y = alpha*x + beta*y (dtype T), used for gradient accumulation ; cast between dtypes */
int d2r_axpby(int dtype, float alpha, const void* x, float beta, void* y, int64_t n, void* stream);
int d2r_cast(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n, void* stream);
/* column sums: out[n] (fp32, OVERWRITTEN) = sum_m X[m, n]   (bias gradients). workspace via query. */
size_t d2r_colsum_workspace(int64_t M, int N);
int d2r_colsum(int dtype, const void* X, int64_t ld, int64_t M, int N, float* out, void* workspace,
               size_t workspace_bytes, void* stream);
/* out[n] += sum_m X[m, n] for M <= 32 rows (one row slice): the bias gradient of a per-sample linear added straight into its fp32 sink */
int d2r_colsum_add(int dtype, const void* X, int64_t ld, int64_t M, int N, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * K1  router pooling  (models/Router.py:23: x.mean(-2));  pooled: fp32 [B, D]
 * nsrc sources pooled in ONE launch (layer >= 1 pools the six aggregated tensors at once).
 * ------------------------------------------------------------------------------------------------ */
int d2r_meanpool_fwd(int dtype, const void* const* h_srcs, int nsrc, int B, int L, int D, float* pooled /*[nsrc,B,D]*/,
                     void* stream);
/* dX[b,l,:] (+)= dpooled[b,:]/L ; accumulate!=0 adds into dX */
int d2r_meanpool_bwd(int dtype, const float* dpooled, int B, int L, int D, void* dX, int accumulate, void* stream);
/* n <= 8 pooled gradients dpooled[n,B,D] broadcast into n distinct [B,L,D] tensors in one launch (16-bit dtypes); bit j of acc_mask:
 * accumulate into dX[j] instead of overwriting it. */
int d2r_meanpool_bwd_multi(int dtype, const float* dpooled, int n, int B, int L, int D, void* const* dX, unsigned acc_mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K8  route_aggregate — path normalisation, threshold gate and aggregation of the cell outputs of one routing layer.
 * Replaces models/DynamicInteraction.py:50-67 (=:119-132, :170-187, :239-252) and the final-layer rule
 * :104-117 (=:224-237).  Cell order [RIC, GLAC, IMRC, CMRC, CRCMC, GESC] (:41-48).
 *   ncell    : number of cells of the layer = the first ncell of that list.  The reference hard-indexes six
 *              (ncell = 6); 2..5 is the declared-subset extension of SURVEY.md section 8c (BASELINE configs[4]: 4 cells):
 *              path normalisation over the ncell cells, final-layer threshold 1e-4/ncell (self.threshold/self.num_cell).
 *   embs[j]  : ncell cell outputs; j=1 (GLAC) and j=5 (GESC) are per-sample [B,D] broadcasts, the rest [B,L,D];
 *              embs[0] is the RIC *input* x0 — relu (models/Cells.py:38) is applied in-kernel.
 *   gates    : fp32 [B, ncell, P] raw router outputs g_j (P = ncell, or 1 for the final layer)
 *   refs     : (final layer only) the ncell layer inputs ref_j [B,L,D] used by the skip term
 *   outs[i]  : P output tensors [B,L,D];  probs: fp32 [B, P, ncell] (normalised for P=ncell, raw for P=1), sample b at
 *              probs + b*ld_probs (ld_probs >= P*ncell: the layers of a module write slices of one [B, total_paths] row)
 * ------------------------------------------------------------------------------------------------ */
int d2r_route_aggregate_fwd(int dtype, const void* const* h_embs /*ncell*/, const void* const* h_refs /*ncell or NULL*/,
                            const float* gates, int B, int L, int D, int ncell, int P, void* const* h_outs /*P*/,
                            float* probs, int64_t ld_probs, void* stream);
size_t d2r_route_aggregate_bwd_workspace(int B, int L, int D, int P);
/* d_embs[j] are OVERWRITTEN (d_embs[0] is w.r.t. the RIC input x0, relu' applied; broadcast ones are [B,D]);
 * d_refs[j] (final layer: gradient of the skip term) OVERWRITTEN, d_gates fp32 [B,ncell,P] OVERWRITTEN.
 * d_probs: fp32 [B,P,ncell] (sample stride ld_dprobs) gradient flowing into the returned `probs` (sim_paths -> JS loss) or NULL;
 * h_outs: forward outputs (only outs[0] of the final layer is read; may be NULL for P=ncell). */
int d2r_route_aggregate_bwd(int dtype, const void* const* h_embs, const void* const* h_refs, const float* gates,
                            const void* const* h_douts /*P*/, const void* const* h_outs, const float* d_probs,
                            int64_t ld_dprobs, int B, int L, int D, int ncell, int P, void* const* h_dembs /*ncell*/,
                            void* const* h_drefs /*ncell or NULL*/, float* d_gates, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K6  SAF gate — BatchNorm1d(1) + sigmoid + l1norm over the Lq+1 alignment scores of every sample
 * (models/XModules.py:380-381).  a: fp32 [B, n] pre-BN scores.  train!=0: batch statistics over all B*n
 * scalars and running-stat update (momentum 0.1, unbiased running var); else running stats.
 * stats (fp32[4]) receives {mean, biased var, rstd, sum-of-sigmoid...}; w: fp32 [B, n] attention weights.
 * ------------------------------------------------------------------------------------------------ */
int d2r_saf_gate_fwd(const float* a, int B, int n, const float* bn_weight, const float* bn_bias,
                     float* running_mean, float* running_var, int train, float* w, float* saved /*[2]: mean,rstd*/,
                     void* stream);
int d2r_saf_gate_bwd(const float* a, const float* dw, int B, int n, const float* bn_weight, const float* bn_bias,
                     const float* saved, int train, float* da, float* d_bn_weight, float* d_bn_bias, void* stream);
/* Global-batch-exact BatchNorm under data parallelism ("optional"): the reference's BatchNorm1d(1) normalises over all
 * B*(Lq+1) scores of the WHOLE batch (models/XModules.py:376,381).  d2r_saf_gate_stats leaves this rank's fp64 sums {sum a, sum a^2}
 * in `sums`; the caller all-reduces them over the ranks and passes the totals (and the global element count) to d2r_saf_gate_fwd_ex.
 * Backward: phase 1 of d2r_saf_gate_bwd_ex stops behind the sigmoid / l1norm part (d y in `da`, this rank's share of the BatchNorm
 * parameter gradients in d_bn_weight / d_bn_bias, fp64 {sum dy, sum dy*xhat} in gsums); after the all-reduce phase 2 finishes `da`
 * with the global sums.  gstats = NULL / phase 0: local-batch statistics (= d2r_saf_gate_fwd / _bwd). */
int d2r_saf_gate_stats(const float* a, int B, int n, double* sums, void* stream);
/* w16 / da16 (optional): a bf16 / fp16 copy of w (forward) and of the finished da (backward: phase 0 or 2), rounded as d2r_cast would -
 * their consumers read them as GEMM operands.  accumulate != 0: the BatchNorm parameter gradients are ADDED to d_bn_weight / d_bn_bias
 * (the caller's fp32 gradient sinks) instead of overwriting them. */
int d2r_saf_gate_fwd_ex(const float* a, int B, int n, const float* bn_weight, const float* bn_bias, float* running_mean,
                        float* running_var, int train, float* w, float* saved, const double* gstats, double ntotal, void* w16,
                        int w16_dtype, void* stream);
int d2r_saf_gate_bwd_ex(const float* a, const float* dw, int B, int n, const float* bn_weight, const float* bn_bias,
                        const float* saved, int train, float* da, float* d_bn_weight, float* d_bn_bias, int phase, double* gsums,
                        double ntotal, void* da16, int da16_dtype, int accumulate, void* stream);

/* The two rank-one products around the gate in the BACKWARD pass of the SAF-weighted sum wsum[b] = w[b] @ S[b]
 * (models/XModules.py:382-384; S [B,n,E], 16-bit): dw[b,i] = <dwsum[b,:], S[b,i,:]> (fp32 [B,n]) and
 * dS[b,i,:] = w[b,i] * dwsum[b,:] + da[b,i] * w_saf[:] (w 16-bit [B,n], da fp32 [B,n], w_saf = attn_sim_w.weight [E], 16-bit). */
int d2r_saf_dweights(int dtype, const void* dwsum, const void* S, int B, int n, int E, float* dw, void* stream);
int d2r_saf_dscores(int dtype, const void* w, const void* dwsum, const float* da, const void* w_saf, int B, int n, int E, void* dS,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * K9  js_div on two [B,B] logit matrices (models/XModules.py:32-41) and K13 cross-entropy
 * (models/unimo_model.py:147,160).  All fp32; single-workgroup latency kernels.
 * ------------------------------------------------------------------------------------------------ */
int d2r_jsdiv_fwd(const float* p_logits, const float* q_logits, int B, float* out /*[1]*/, void* stream);
int d2r_jsdiv_bwd(const float* p_logits, const float* q_logits, int B, const float* dout /*[1]*/, float* dp,
                  float* dq, void* stream);
int d2r_ce_fwd(const float* logits, const int64_t* labels, int B, int C, float* loss /*[1]*/, void* stream);
int d2r_ce_bwd(const float* logits, const int64_t* labels, int B, int C, const float* dloss /*[1]*/,
               float* dlogits, void* stream);
/* d2r_ce_fwd_ex / d2r_ce_bwd_ex: cross entropy with per-class weights and label smoothing, exactly torch.nn.functional.cross_entropy(logits, labels, weight=w,
 * label_smoothing=e, reduction="mean") - CrossEntropyLoss(weight=, label_smoothing=) at models/unimo_model.py:147.  With
 * lp = log_softmax(logits) and w == 1 when class_weight is NULL (class_weight: fp32 [C] on the device):
 *   loss         = sum_b [ (1-e) w[y_b] (-lp[b,y_b]) + (e/C) sum_c w[c] (-lp[b,c]) ] / sum_b w[y_b]
 *   dlogits[b,c] = dloss / sum_b w[y_b] * ( p[b,c] ((1-e) w[y_b] + (e/C) sum_k w[k]) - (1-e) w[y_b] [c == y_b] - (e/C) w[c] )
 * class_weight == NULL and label_smoothing == 0 launch the kernels of d2r_ce_fwd / d2r_ce_bwd: the result is bit-identical to theirs.
 * label_smoothing outside [0, 1) (a NaN included) is refused before anything is launched.  Labels outside [0, C) are the caller's
 * error, as for d2r_ce_fwd / d2r_ce_bwd (they are not checked on the device).  A batch whose labels all carry weight 0 divides by
 * zero and gives NaN, as torch does.  The backward kernel sums w[y_b] over the batch again in every workgroup (no workspace). */
int d2r_ce_fwd_ex(const float* logits, const int64_t* labels, const float* class_weight /* [C] or NULL */,
                  float label_smoothing, int B, int C, float* loss /*[1]*/, void* stream);
int d2r_ce_bwd_ex(const float* logits, const int64_t* labels, const float* class_weight, float label_smoothing,
                  int B, int C, const float* dloss /*[1]*/, float* dlogits /*[B,C]*/, void* stream);
/* d2r_ce_mix_fwd / d2r_ce_mix_bwd: cross entropy against TWO labels per row (MixUp / CutMix, d2r_amd/mix.py): the formula of
 * d2r_ce_fwd_ex / d2r_ce_bwd_ex with the one-hot target replaced by lam_b onehot(y_b) + (1 - lam_b) onehot(y2_b).  With
 * lp = log_softmax(logits), w == 1 when class_weight is NULL, y = labels[b], y2 = labels_b[b], lam = lam[b] (fp32 [B] on the device):
 *   hard_b(c)    = (1-e) ( lam w[y] [c == y] + (1-lam) w[y2] [c == y2] )
 *   loss         = sum_b [ sum_c hard_b(c) (-lp[b,c]) + (e/C) sum_c w[c] (-lp[b,c]) ] / W,   W = sum_b ( lam w[y] + (1-lam) w[y2] )
 *   dlogits[b,c] = dloss / W * ( p[b,c] (sum_k hard_b(k) + (e/C) sum_k w[k]) - hard_b(c) - (e/C) w[c] )
 * With every lam == 1 it is the formula of d2r_ce_*_ex exactly, and the result has their bits.  Without class weights it is
 * torch.nn.functional.cross_entropy(logits, lam onehot(y) + (1-lam) onehot(y2), label_smoothing=e) - probability targets.
 * labels_b and lam are both given or both NULL; only one of them is refused.  Both NULL forwards to d2r_ce_fwd_ex / d2r_ce_bwd_ex
 * (which forward to d2r_ce_fwd / d2r_ce_bwd without options): bit-identical to a call without them.  label_smoothing outside
 * [0, 1) is refused.  A lam outside [0, 1], like a label outside [0, C), is the caller's error (it lives on the device).  The same
 * launch shapes as the _ex kernels; the backward kernel sums W again in every workgroup (no workspace, no atomics). */
int d2r_ce_mix_fwd(const float* logits, const int64_t* labels, const int64_t* labels_b /* [B] or NULL */,
                   const float* lam /* fp32 [B] on the device, or NULL */, const float* class_weight /* [C] or NULL */,
                   float label_smoothing, int B, int C, float* loss /*[1]*/, void* stream);
int d2r_ce_mix_bwd(const float* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, const float* class_weight,
                   float label_smoothing, int B, int C, const float* dloss /*[1]*/, float* dlogits /*[B,C]*/, void* stream);
/* d2r_ce_focal_fwd / d2r_ce_focal_bwd: focal loss (Lin et al. 2017; --focal_gamma) on top of d2r_ce_mix_fwd / d2r_ce_mix_bwd: every
 * row's term is scaled by the g-th power of the probability mass that is NOT on its target, g = focal_gamma >= 0.  In the notation
 * above, with p = exp(lp) and t_b(c) = lam_b [c == y_b] + (1 - lam_b) [c == y2_b] row b's target (the one-hot of y_b without a pair):
 *   a_b(c) = (1-e) w[c] t_b(c) + (e/C) w[c]          (the coefficients of d2r_ce_mix_*)
 *   row_b  = sum_c a_b(c) (-lp[b,c])                 (their per-row term)
 *   q_b    = sum_c t_b(c) p[b,c]                     (probability mass on the target)
 *   u_b    = 1 - q_b = sum_c (1 - t_b(c)) p[b,c]     (a sum of non-negative terms)
 *   loss   = sum_b u_b^g row_b / W,    W = sum_b sum_c t_b(c) w[c]     (W unchanged: the normaliser of d2r_ce_mix_*)
 *   dlogits[b,c] = dloss / W * ( u_b^g (p[b,c] sum_k a_b(k) - a_b(c))  -  g u_b^g row_b (p[b,c] t_b(c) - r_b(c) q_b) )
 *   r_b(c) = p[b,c] (1 - t_b(c)) / u_b   in [0, 1];   u_b == 0 (C == 1, or underflow): u_b^g = 0 and r_b(c) = 0 for g > 0
 * Without weights, smoothing or a second label it is -(1 - p_t)^g log p_t, mean over the batch; with class weights, they play the
 * role of alpha.  The gradient is computed as written: the forms p - p (1 - t) / u and t - q cancel in fp32.  u_b is summed from
 * its non-negative terms (never 1 - q_b), u_b^g = exp(g (log su_b - log s_b)) with s_b / su_b the row's sums of exponentials with /
 * without the target's share, and u_b^(g-1), which overflows for a small g, is never formed.  Every output is finite for finite
 * logits, the rows whose target leads by more than fp32's exponent range included (they contribute 0).
 * focal_gamma == 0 forwards to d2r_ce_mix_fwd / d2r_ce_mix_bwd (which forward on to the _ex and the plain kernels): today's loss with
 * today's bits.  labels_b and lam are both given or both NULL; only one of them is refused.  A focal_gamma that is negative, NaN or
 * infinite and a label_smoothing outside [0, 1) are refused before anything is launched or written.  The same launch shapes as the
 * kernels above: one workgroup of 256 threads forward, cdiv(B, 256) workgroups backward, each of which sums W again in a fixed
 * order (no workspace, no atomics). */
int d2r_ce_focal_fwd(const float* logits, const int64_t* labels, const int64_t* labels_b /* [B] or NULL */,
                     const float* lam /* fp32 [B] on the device, or NULL */, const float* class_weight /* [C] or NULL */,
                     float label_smoothing, float focal_gamma, int B, int C, float* loss /*[1]*/, void* stream);
int d2r_ce_focal_bwd(const float* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, const float* class_weight,
                     float label_smoothing, float focal_gamma, int B, int C, const float* dloss /*[1]*/, float* dlogits /*[B,C]*/,
                     void* stream);
/* Predicted class per row of fp32 X[rows, cols] (row stride ld >= cols): idx[r] = argmax_c X[r, c], with torch.argmax's rules -
 * a tie goes to the lowest index, a NaN counts as the maximum and the first NaN of a row wins, +-inf compare as usual.
 * Replaces logits.argmax(-1) at modules/train.py:181,243 (prediction from a checkpoint).  rows == 0 launches nothing. */
int d2r_argmax_rows(const float* X, int64_t ld, int64_t rows, int cols, int64_t* idx /*[rows]*/, void* stream);
/* d2r_confusion_add: the confusion matrix of a batch, ADDED to counts (int64 [C, C], row = label, column = prediction): counts[labels[r], argmax_c
 * logits[r, c]] += 1 for every row r whose label lies in [0, C); a row with any other label (the loaders' -1 = unlabelled) is
 * counted nowhere.  The prediction follows d2r_argmax_rows' rules (first maximal index, torch's NaN rule).  Integer atomics: the
 * result does not depend on the order of the adds, and the call may be repeated on the same counts across the batches of a pass
 * (the caller zeroes counts once).  logits fp32 [rows, C] with row stride ld; rows < 1, C < 1 and ld < C are refused. */
int d2r_confusion_add(const float* logits, int64_t ld, const int64_t* labels, int64_t rows, int C,
                      int64_t* counts /* [C,C], row = label, column = prediction, ADDED to */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K10 Block fusion core (models/XModules.py:541-549): z[b,c,s] = sum_r m0[b,c,r,s]*m1[b,c,r,s];
 * signed sqrt; L2-normalise over s.  m0,m1: [B, C, R*S] (dtype T), out: [B, C*S] (dtype T), zraw fp32 [B,C*S].
 * ------------------------------------------------------------------------------------------------ */
int d2r_block_merge_fwd(int dtype, const void* m0, const void* m1, int B, int C, int R, int S, void* out,
                        float* zraw, void* stream);
int d2r_block_merge_bwd(int dtype, const void* m0, const void* m1, const float* zraw, const void* dout, int B,
                        int C, int R, int S, void* dm0, void* dm1, void* stream);

/* As d2r_layernorm_bwd, plus: dX += dres when dres != NULL (the gradient arriving through the skip connection
 * around the block this LayerNorm belongs to), and dgamma/dbeta ACCUMULATED when accumulate != 0. */
int d2r_layernorm_bwd_ex(int dtype, const void* dY, const void* X, const float* gamma, const float* mean,
                         const float* rstd, int64_t rows, int D, void* dX, const void* dres, float* dgamma,
                         float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* dgamma == dbeta == NULL in d2r_layernorm_bwd_ex DEFERS the second stage: the per-block partial sums stay in `workspace` (which
 * then has to outlive the call) and this entry point sums them for n LayerNorms of one shape (rows, D) in one launch per 32
 * problems; dgamma[i] / dbeta[i] overwritten, or accumulated when accumulate != 0.  Bit-identical to the undeferred sum. */
int d2r_layernorm_bwd_sum_grouped(const void* const* partials, float* const* dgamma, float* const* dbeta, int n, int64_t rows,
                                  int D, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3 fused multi-head attention core (16-bit dtypes, head_dim 64 or 48, Lq, Lk <= 1024: up to 256 tokens with the whole
 * head resident in LDS, above that a loop over 128-row blocks with the online softmax — BASELINE configs[3] / [4])
 *   O[b,:,h] = softmax(scale * Q_h K_h^T + mask[b]) V_h (+ residual)
 * Replaces BertSelfAttention scores/softmax/context (models/modeling_unimo.py:385-424), CLIPAttention (:150-215)
 * and the 16-head attention of models/SelfAttention.py:20-60 — scores and probabilities never reach HBM.
 * q/k/v/o/residual/dO/dq/dk/dv: bf16 [B, L, *] views given as (pointer to column 0 of head 0, row stride,
 * batch stride) in elements; head h occupies columns [h*head_dim, (h+1)*head_dim).  mask: fp32 additive [B,Lk] or
 * NULL.  lse: fp32 [B,H,Lq] row log-sum-exp written by fwd and read by bwd.  dsum (bwd): fp32 [B,H,Lq] scratch the
 * long-sequence backward hands from its dQ kernel to its dK/dV kernel; may be NULL when Lq, Lk <= 256.  Pointers 16-byte
 * aligned, strides multiples of 8 elements.  Deterministic.
 * p_drop / seed: dropout on the probabilities (attention_probs_dropout_prob, models/modeling_unimo.py:388) inside the kernel:
 * probability (b, h, q, key) is kept iff the counter-based generator of d2r_dropout, at element index
 * ((b*H + h)*Lq + q)*lkp + key with lkp = Lk rounded up to 8, says so, and is then scaled by 1/(1-p); the backward
 * regenerates the mask from the same (p_drop, seed).  p_drop = 0: no dropout.
 * ------------------------------------------------------------------------------------------------ */
int d2r_mha_supported(int dtype, int Lq, int Lk, int head_dim);
int d2r_mha_fwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                const void* v, int64_t ldv, int64_t svb, void* o, int64_t ldo, int64_t sob, const void* residual,
                int64_t ldr, int64_t srb, const float* mask, float* lse, int B, int H, int Lq, int Lk, int head_dim,
                float scale, float p_drop, uint64_t seed, void* stream);
int d2r_mha_bwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                const void* v, int64_t ldv, int64_t svb, const void* dO, int64_t ldg, int64_t sgb, const float* mask,
                const float* lse, float* dsum, void* dq, int64_t lddq, int64_t sdqb, void* dk, int64_t lddk, int64_t sdkb,
                void* dv, int64_t lddv, int64_t sdvb, int B, int H, int Lq, int Lk, int head_dim, float scale, float p_drop,
                uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K2 / K4 fused single-head attention over the full 768-wide feature (16-bit dtypes, D = 768, Lk <= 640)
 *   O[b] = softmax(scale * Q K^T + mask[b]) V (+ residual)
 * Replaces the CrossModalAlignment core (models/XModules.py:300-310 = models/Refinement.py:105-115, scale
 * 100/sqrt(768)) and the ContextRichCrossModalCell core (models/Cells.py:244-246, scale 1, residual Qs): three
 * launches (QK^T GEMM, softmax, PV GEMM) and an fp32 [B,Lq,Lk] round trip become one launch.
 * q/k/v/o/residual/dO/dq: bf16 [B, L, 768] views as (pointer, row stride, batch stride) in elements.
 * lse: fp32 [B, Lq].  d2r_xattn_bwd writes dq plus P and dS (16-bit [B, Lq, lkp]; lkp >= Lk, a multiple of 8, at most 640:
 * columns >= Lk are scratch) for the key-side products dV = P^T dO and dK = dS^T Q, which the caller runs as batched d2r_gemm
 * (TN) launches.  Pointers 16-byte aligned, strides multiples of 8 elements.  Deterministic.
 * ------------------------------------------------------------------------------------------------ */
int d2r_xattn_supported(int dtype, int Lq, int Lk, int D);
int d2r_xattn_fwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                  const void* v, int64_t ldv, int64_t svb, void* o, int64_t ldo, int64_t sob, const void* residual,
                  int64_t ldr, int64_t srb, const float* mask, float* lse, int B, int Lq, int Lk, int D, float scale,
                  void* stream);
int d2r_xattn_bwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                  const void* v, int64_t ldv, int64_t svb, const void* dO, int64_t ldg, int64_t sgb, const float* mask,
                  const float* lse, void* dq, int64_t lddq, int64_t sdqb, void* P, void* dS, int lkp, int B, int Lq,
                  int Lk, int D, float scale, void* stream);

/* Several attention problems ("cores") of IDENTICAL shape and strides in one launch: the three cross-modal alignment cores of a
 * routing layer (GlobalLocalAlignmentCell, CrossModalRefinementCell, ContextRichCrossModalCell: models/Cells.py:147,85,238 all
 * call the same softmax(100 q k^T / sqrt(768)) v on their own projections of the same two token tensors) give three times
 * the workgroups of one - a single core leaves half of the 256 CUs idle at B = 32.  h_* are HOST arrays of `ncore` (1..4)
 * device pointers; h_residual may be NULL (or hold NULLs).  d2r_xattn_bwd_multi also runs the key-side products
 * dV = P^T dO and dK = dS^T Q of every sample and core (ONE grouped, batched launch of the LDS-DMA GEMM kernel when dk / dv
 * share their strides, e.g. the two halves of a packed k|v gradient), so it returns dq, dk and dv; h_P / h_dS are scratch
 * (16-bit [B, Lq, lkp] each; lkp >= Lk, a multiple of 8, at most 640; need not be initialised).  With h_o given, Lk <= 256,
 * Lq <= 256 and lkp <= 256 the third-generation kernels run
 * (xattn3.hip: queries split over the waves, K / V streamed once through a six-slot LDS-DMA ring, D = rowsum(dO o (O - residual))
 * from the saved output; dk / dv may then be 8-byte aligned with strides multiples of 4); otherwise the second-generation
 * query-side kernel, which recomputes D from P and dP, and the TN launches. */
int d2r_xattn_fwd_multi(int dtype, int ncore, const void* const* h_q, int64_t ldq, int64_t sqb, const void* const* h_k, int64_t ldk,
                        int64_t skb, const void* const* h_v, int64_t ldv, int64_t svb, void* const* h_o, int64_t ldo, int64_t sob,
                        const void* const* h_residual, int64_t ldr, int64_t srb, const float* mask, float* const* h_lse, int B, int Lq,
                        int Lk, int D, float scale, void* stream);
int d2r_xattn_bwd_multi(int dtype, int ncore, const void* const* h_q, int64_t ldq, int64_t sqb, const void* const* h_k, int64_t ldk,
                        int64_t skb, const void* const* h_v, int64_t ldv, int64_t svb, const void* const* h_dO, int64_t ldg, int64_t sgb,
                        const void* const* h_o /* the forward outputs (residual included), or NULL */, int64_t ldo, int64_t sob,
                        const void* const* h_residual /* what the forward added, or NULL */, int64_t ldr, int64_t srb,
                        const float* mask, const float* const* h_lse, void* const* h_dq, int64_t lddq, int64_t sdqb, void* const* h_dk,
                        int64_t lddk, int64_t sdkb, void* const* h_dv, int64_t lddv, int64_t sdvb, void* const* h_P, void* const* h_dS,
                        int lkp, int B, int Lq, int Lk, int D, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K15 one transformer encoder layer per call (16-bit dtypes): BertLayer.forward (models/modeling_unimo.py:473-512,
 * post-LayerNorm, GELU) and CLIPEncoderLayer.forward (:222-268, pre-LayerNorm, quick_gelu), forward or backward.
 * Same kernels, same order as the single-op entry points; the 7 forward / ~16 backward launches are issued from
 * C++ in one call, skip-connection gradients ride in GEMM / LayerNorm epilogues, parameter gradients accumulate
 * into the caller's fp32 sinks.  All activation buffers are [B*L, *] row-major in `dtype`.
 *   post-LN: h1 = x + attn(x) ; n1 = LN1(h1) ; h2 = n1 + ffn(n1) ; y = LN2(h2)
 *   pre-LN : n1 = LN1(x) ; h1 = x + attn(n1) ; h2 = LN2(h1) ; y = h1 + ffn(h2)
 *   attn(a) = mha(a Wqkv^T + bqkv) Wo^T + bo ;  ffn(a) = act(a W1^T + b1) W2^T + b2
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int dtype;                  /* D2R_BF16 or D2R_F16 */
  int pre_ln;                 /* 0 post-LN (BERT), 1 pre-LN (CLIP ViT) */
  int act;                    /* D2R_ACT_GELU | D2R_ACT_QUICK_GELU */
  int B, L, E, H, F;          /* batch, tokens, hidden, heads, intermediate */
  float eps, scale;           /* LayerNorm eps; attention logit scale (head_dim^-0.5) */
  const float* mask;          /* additive key mask fp32 [B,L] or NULL */
  const void *w_qkv, *w_o, *w_1, *w_2;           /* [3E,E] (q|k|v rows), [E,E], [F,E], [E,F] in dtype */
  const float *b_qkv, *b_o, *b_1, *b_2, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  float *gw_qkv, *gw_o, *gw_1, *gw_2, *gb_qkv, *gb_o, *gb_1, *gb_2, *gln1_g, *gln1_b, *gln2_g, *gln2_b; /* bwd: += */
  const void* x;              /* in  [B*L,E] */
  void* y;                    /* out [B*L,E] */
  void *qkv, *ctx, *h1, *n1, *f_pre, *f, *h2;    /* saved by fwd, read by bwd: [T,3E] [T,E] [T,E] [T,E] [T,F] [T,F] [T,E] */
  float *lse, *mean1, *rstd1, *mean2, *rstd2;    /* [B,H,L], [T] x4 */
  const void* dy;             /* bwd in  [B*L,E] */
  void* dx;                   /* bwd out [B*L,E] */
  void* scratch; size_t scratch_bytes;           /* bwd: >= d2r_encoder_layer_bwd_scratch() */
  /* bwd: split-K scratch of the in-call weight-gradient GEMMs (d2r_gemm_desc.workspace and its rules: the last 4 KiB zero before the
   * first use, zero again afterwards; launches that share it are ordered).  NULL: those GEMMs run without split-K - same dx, o_dy[] and
   * LayerNorm gradients bit for bit, dW / db summed in another order.  Not used with defer_wgrad. */
  void* splitk_ws; size_t splitk_bytes;
  /* bwd: optional second stream (hipStream_t) for the four weight-gradient GEMMs, forked from `stream` inside the
   * call; the caller joins it before anything reads the gradient sinks, and keeps x, the saved activations, dy,
   * scratch, splitk_ws (then used on that stream only) and the sinks alive until it has drained.  NULL: everything on `stream`. */
  void* wgrad_stream;
  /* bwd: != 0 skips the four weight-gradient GEMMs (and bias gradients); the caller launches them later, grouped with
   * the same products of other layers (d2r_gemm_tn_grouped), from o_dy[] and the saved activations. */
  int defer_wgrad;
  /* bwd, written by the call: the output gradients of the qkv / out / fc1 / fc2 linears ([T,3E] [T,E] [T,F] [T,E], inside
   * `scratch` or dy itself) — dW = o_dy^T x with x = x|n1, ctx, n1|h2, f.  With p_hidden or p_path, o_dy[1] and o_dy[3] name the
   * MASKED gradients (mask o g / ((1 - p_hidden)(1 - p_path)): what the dense outputs receive), which are copies inside `scratch`;
   * without them o_dy[3] of a pre-LN layer is dy itself.  They stay valid until `scratch` is reused. */
  const void* o_dy[4];
  /* bwd, with defer_wgrad: != 0 also defers the second stage of the two LayerNorm backward passes (their gamma / beta gradients):
   * the call writes the per-block partial sums into `scratch` and reports them in o_lnws[0] (LayerNorm 1) / o_lnws[1] (LayerNorm 2);
   * the caller sums them later with d2r_layernorm_bwd_sum_grouped(rows = B*L, D = E, accumulate = 1) into gln{1,2}_{g,b}. */
  int defer_ln;
  const void* o_lnws[2];
  /* training-time dropout of the BERT layer (models/modeling_unimo.py:388 on the attention probabilities, :413 / :468 on
   * the two dense outputs in front of their residual adds); 0 disables.  The masks are functions of (seed, element index)
   * as in d2r_dropout: the probabilities use seed_attn inside the fused attention core, the dense outputs seed_hidden[0]
   * (attention output) and seed_hidden[1] (FFN output) with the element index in the [B*L, E] tensor.  The backward
   * call regenerates them from the same values. */
  float p_attn, p_hidden;
  uint64_t seed_attn, seed_hidden[2];
  /* training-time stochastic depth (an extension; 0 = off, what a zero-initialised tail means): each of the two residual branches
   * is dropped per sample with probability p_path and scaled by 1 / (1 - p_path) otherwise, by the pass that applies p_hidden
   * (d2r_drop_path over [B, L*E]; p_path = 0 leaves the call sequence as it was).  seed_path[0]: attention branch, [1]: FFN
   * branch; the mask is a function of (seed, sample index) and the backward call regenerates it. */
  float p_path;
  uint64_t seed_path[2];
} d2r_encoder_layer_desc;
size_t d2r_encoder_layer_bwd_scratch(int B, int L, int E, int F);
int d2r_encoder_layer_fwd(const d2r_encoder_layer_desc* d, void* stream);
int d2r_encoder_layer_bwd(d2r_encoder_layer_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K16 one whole (Reversed_)InteractionModule per call (16-bit compute dtype): the DR_step routing layers of
 * models/InteractionModule.py:22-55 (=:75-108) — every router (models/Router.py:22-26), the up to six cells of each layer
 * (models/Cells.py:30-255 with SelfAttention.py / Refinement.py / XModules.py:277-394), the path normalisation, threshold
 * gates and aggregation (models/DynamicInteraction.py:37-69, 90-134) and the concatenated path probabilities
 * (InteractionModule.py:33-53) — forward, or backward, issued from C++ in ONE call: the same kernels as the single-op
 * entry points above, without one Python autograd node and one foreign call per launch.  In the backward pass every
 * multi-consumer gradient (the module's two inputs, a layer's aggregated outputs) is accumulated in GEMM epilogues
 * (beta = 1 / residual operand) instead of separate add launches, and the 768x768-class weight gradients are queued and
 * launched grouped (d2r_gemm_tn_grouped) at the end of the call.  Parameter gradients ACCUMULATE into the caller's fp32
 * sinks.  `own` is the branch's own modality (text for InteractionModule, image tokens for the reversed module).
 * Requires the fused attention cores for the shapes: d2r_xattn_supported(Lq,Lk), (Lq,Lq) and d2r_mha_supported(Lq,Lq,48).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  const void* w;   /* [N,K] weight in the compute dtype (router linears: fp32 masters) */
  const float* b;  /* fp32 [N] */
  float* gw;       /* fp32 [N,K] gradient sink, accumulated */
  float* gb;       /* fp32 [N] gradient sink, accumulated */
} d2r_linear_params;
/* linears of one routing layer, in this order (same-input projections are ONE fused linear: rows back to back) */
enum {
  D2R_RL_R0 = 0,      /* the ncell routers' mlp.0, fused [ncell*hid, 768] fp32 */
  D2R_RL_R2,          /* the ncell routers' mlp.2, fused [ncell*P, hid] fp32 (one group per cell) */
  D2R_RL_IMRC_QKV,    /* sa.att_layer.linears.0|1|2  [2304,768] */
  D2R_RL_IMRC_FC1, D2R_RL_IMRC_FC2,
  D2R_RL_GLAC_Q, D2R_RL_GLAC_KV /* key|value [1536,768] */, D2R_RL_GLAC_LOC /* fc_sim_tranloc */, D2R_RL_GLAC_FC1,
  D2R_RL_GLAC_TPOOL /* text_cls_pool.dense (applied to OWN tokens) */, D2R_RL_GLAC_IPOOL /* image_cls_pool.dense (OTHER) */,
  D2R_RL_GLAC_GLO /* fc_sim_tranglo */, D2R_RL_GLAC_FC2, D2R_RL_GLAC_SAFW /* SAF_module.attn_sim_w [1,768] */,
  D2R_RL_CMRC_Q, D2R_RL_CMRC_KV, D2R_RL_CMRC_SCALE, D2R_RL_CMRC_SHIFT, D2R_RL_CMRC_FC1, D2R_RL_CMRC_FC2,
  D2R_RL_CRCMC_Q, D2R_RL_CRCMC_KV, D2R_RL_CRCMC_MLP1, D2R_RL_CRCMC_MLP2, D2R_RL_CRCMC_FC1, D2R_RL_CRCMC_FC2,
  D2R_RL_GESC_TPOOL, D2R_RL_GESC_IPOOL, D2R_RL_GESC_MLP0, D2R_RL_GESC_MLP2,
  D2R_RL_NLIN
};
typedef struct {
  d2r_linear_params lin[D2R_RL_NLIN];   /* entries of absent cells (declared subset) are ignored */
  const float *bn_weight, *bn_bias;     /* GLAC SAF BatchNorm1d(1) */
  float *bn_running_mean, *bn_running_var;
  float *g_bn_weight, *g_bn_bias;       /* fp32 [1] sinks, accumulated */
} d2r_routing_layer_params;
typedef struct {
  int dtype;                 /* D2R_BF16 */
  int B, Lq, Lk;             /* batch, own tokens, other tokens (hidden size is 768: models/Cells.py:140-143) */
  int ncell, nlayer;         /* cells per layer (2..6), routing layers = DR_step (>= 2): layer 0, middle layers, final layer */
  int hid_router, heads_imrc, hid_imrc;
  int train;                 /* BatchNorm: batch statistics + running-stat update (1) or running statistics (0) */
  const d2r_routing_layer_params* layers;  /* HOST array [nlayer] */
  const void* own;           /* [B,Lq,768] */
  const void* other;         /* [B,Lk,768] */
  void* out;                 /* [B,Lq,768]  fwd: written; bwd: read (final-layer aggregation backward) */
  float* paths;              /* fp32 [B, ncell*ncell*(nlayer-1) + ncell]  fwd: written */
  void* arena; size_t arena_bytes;        /* saved activations: fwd writes, bwd reads; >= d2r_interaction_arena_bytes() */
  void* splitk_ws; size_t splitk_bytes;   /* split-K scratch of small-M / weight-gradient GEMMs (may be NULL) */
  /* backward only */
  const void* d_out;         /* [B,Lq,768] or NULL (= zero) */
  const float* d_paths;      /* fp32 [B, total_paths] or NULL */
  void* d_own; void* d_other;             /* [B,Lq,768], [B,Lk,768]  OVERWRITTEN */
  void* scratch; size_t scratch_bytes;    /* >= d2r_interaction_bwd_scratch() */
  /* The key | value projections of `other` of EVERY alignment cell (GLAC, CMRC, CRCMC) of EVERY layer as one fused linear: rows
   * [k | v] of (layer 0: GLAC, CMRC, CRCMC), (layer 1: ...), ... i.e. [nkv * 1536, 768] with nkv = cells-with-alignment * nlayer
   * (`other` is the same tensor in every layer, models/DynamicInteraction.py:95-102): one GEMM with N = 13,824 at DR_step 3 in
   * the forward pass, one dX and one dW product in the backward pass.  The D2R_RL_*_KV entries of `layers` are then unused. */
  d2r_linear_params kv_all;
  /* Optional, data parallelism in the global-batch-exact mode: the BatchNorm1d(1) of every GLAC cell takes its statistics over the
   * samples of ALL ranks.  bn_sync(user, pair, stream) must SUM the two fp64 values at the device address `pair` over the ranks,
   * ordered on `stream` (e.g. an RCCL all-reduce), and return 0; it is called twice per routing layer and direction from inside the
   * call (the library itself has no communication).  bn_sync_buf: device scratch of 4 doubles per routing layer; bn_world: number
   * of ranks (the global score count is bn_world * B * (Lq + 1)).  bn_sync = NULL: local-batch statistics. */
  int (*bn_sync)(void* user, double* pair, void* stream);
  void* bn_sync_user;
  double* bn_sync_buf;
  int bn_world;
} d2r_interaction_desc;
int d2r_interaction_supported(int dtype, int Lq, int Lk, int ncell, int heads_imrc);
size_t d2r_interaction_arena_bytes(int B, int Lq, int Lk, int ncell, int nlayer, int hid_router, int hid_imrc);
size_t d2r_interaction_bwd_scratch(int B, int Lq, int Lk, int ncell, int nlayer, int hid_router, int hid_imrc);
int d2r_interaction_fwd(const d2r_interaction_desc* d, void* stream);
int d2r_interaction_bwd(const d2r_interaction_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K17 the classification head as ONE call each way, fp32: Block fusion of the two pooled vectors (models/XModules.py:478-555:
 * linear0 / linear1 [mm, E], `chunks` rank-`rank` merge projections per side, product, sum over the rank, signed square root,
 * per-chunk l2 normalisation, linear_out [E, mm]), fc [classes, E] (models/unimo_model.py:156-158), cross entropy and
 * loss = ce + js (models/unimo_model.py:160).  The same launches in the same order as the single-op entry points
 * (d2r_gemm, d2r_block_merge_*, d2r_ce_*, d2r_lincomb); parameter gradients ACCUMULATE into the caller's fp32 sinks.
 * merge0 / merge1: the `chunks` projections of a side back to back, [chunks * rank * (mm / chunks), mm / chunks].
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int B, E, mm, chunks, rank, classes;
  d2r_linear_params lin0, lin1, merge0, merge1, lin_out, fc;   /* fp32 weights */
  const float* x0; const float* x1;     /* fp32 [B, E]: pooled text / image vectors (Block's two inputs) */
  const int64_t* labels;                /* [B]; NULL in the forward call: logits / pooled only (below) */
  const float* js;                      /* fp32 [1]: the JS term of the loss (may be NULL when labels is) */
  float* loss; float* logits; float* pooled;   /* [1], [B, classes], [B, E] (Block's output)  OVERWRITTEN */
  void* arena; size_t arena_bytes;      /* forward activations kept for the backward call: >= d2r_head_arena_bytes() */
  void* splitk_ws; size_t splitk_bytes; /* split-K scratch of the weight-gradient GEMMs (may be NULL) */
  /* backward only */
  const float* d_loss;                  /* fp32 [1] */
  float* d_x0; float* d_x1; float* d_js;       /* [B, E], [B, E], [1]  OVERWRITTEN */
  void* scratch; size_t scratch_bytes;  /* >= d2r_head_bwd_scratch() */
  /* backward, optional: gradients arriving at the OTHER outputs of the head (a second loss on the logits, e.g. distillation, or
   * on Block's output), added to the cross-entropy path: fp32 [B, classes] / [B, E] or NULL.  (Label smoothing and class weights
   * are class_weight / label_smoothing below: they change the reported loss too.) */
  const float* d_logits; const float* d_pooled;
  /* optional, both ways: per-class weights (fp32 [classes] on the device, or NULL) and label smoothing in [0, 1) of the cross
   * entropy (d2r_ce_fwd_ex / d2r_ce_bwd_ex).  NULL and 0: d2r_ce_fwd / d2r_ce_bwd, exactly the launches without these fields. */
  const float* class_weight; float label_smoothing;
} d2r_head_desc;
size_t d2r_head_arena_bytes(int B, int E, int mm, int chunks, int rank, int classes);
size_t d2r_head_bwd_scratch(int B, int E, int mm, int chunks, int rank, int classes);
/* Prediction without labels: d2r_head_fwd with labels == NULL runs Block fusion, linear_out and fc as with labels and writes pooled
 * and logits only (no cross entropy, no sum; loss and js may then be NULL).  d2r_head_bwd always needs labels (there is no loss to
 * differentiate without them). */
int d2r_head_fwd(const d2r_head_desc* d, void* stream);
int d2r_head_bwd(const d2r_head_desc* d, void* stream);
/* The head on a MixUp / CutMix batch: d2r_head_desc with two fields after its end - the second label per row ([B]) and the first
 * label's share (fp32 [B] on the device).  d2r_head_desc itself keeps its layout, so callers of d2r_head_fwd / d2r_head_bwd are
 * not disturbed.  d2r_head_mix_fwd / d2r_head_mix_bwd are d2r_head_fwd / d2r_head_bwd with d2r_ce_mix_fwd / d2r_ce_mix_bwd as the cross
 * entropy; with labels_b and mix_lam both NULL they take exactly the branches of d2r_head_fwd / d2r_head_bwd (only one of the two
 * is refused). */
typedef struct {
  d2r_head_desc head;
  const int64_t* labels_b; const float* mix_lam;
} d2r_head_mix_desc;
int d2r_head_mix_fwd(const d2r_head_mix_desc* d, void* stream);
int d2r_head_mix_bwd(const d2r_head_mix_desc* d, void* stream);
/* The head with the focal cross entropy: d2r_head_mix_desc followed by focal_gamma; the two descriptors above keep their layouts.
 * d2r_head_focal_fwd / d2r_head_focal_bwd are d2r_head_mix_fwd / d2r_head_mix_bwd with d2r_ce_focal_fwd / d2r_ce_focal_bwd as the cross
 * entropy (labels_b and mix_lam may both be NULL); with focal_gamma == 0 they take exactly the branches of d2r_head_mix_fwd /
 * d2r_head_mix_bwd.  A focal_gamma that is negative, NaN or infinite is refused before anything is launched. */
typedef struct {
  d2r_head_mix_desc mix;
  float focal_gamma;
} d2r_head_focal_desc;
int d2r_head_focal_fwd(const d2r_head_focal_desc* d, void* stream);
int d2r_head_focal_bwd(const d2r_head_focal_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K12 embeddings (models/modeling_unimo.py:87-118, 272-331)
 * ------------------------------------------------------------------------------------------------ */
/* out[b,l,:] = word[ids[b,l]] + pos[l] + type[tt[b,l]]   (tables fp32, out dtype T; LayerNorm separately) */
int d2r_bert_embed_fwd(int dtype, const int64_t* ids, const int64_t* tt, const float* word, const float* pos,
                       const float* type, int B, int L, int D, int vocab, int ntype, void* out, void* stream);
/* Gradients of the three tables, ACCUMULATED (+=) into dword [vocab,D], dpos [>=L,D], dtype_tab [ntype,D] (fp32, so
 * they may be the flat gradient buffer itself): dword[id] += sum of dY rows of the tokens carrying id, dtype_tab
 * likewise per token type, dpos[l] += sum_b dY[b,l].  Deterministic (fixed summation order, no float atomics).
 * Rows with ids == pad_id get no gradient (padding_idx, models/modeling_unimo.py:277).  D % 4 == 0, D <= 1024. */
int d2r_bert_embed_bwd(int dtype, const void* dY, const int64_t* ids, const int64_t* tt, int B, int L, int D,
                       int ntype, int64_t pad_id, float* dword, float* dpos, float* dtype_tab, void* stream);
/* im2col for the stride=kernel patch conv: pixels fp32 [B,3,H,W] -> patches T [B*(H/p)*(W/p), 3*p*p] */
int d2r_patchify(int dtype, const float* pixels, int B, int H, int W, int p, void* patches, void* stream);
/* CLIP image preprocessing of a batch of decoded images (processor/dataset.py:87-95: CLIPProcessor(images=...) per sample,
 * with resample=BICUBIC, size={"shortest_edge": R}, crop_size=S x S): Pillow's antialiased fixed-point bicubic resize, the center
 * crop, the rescale and the normalisation, bit-identical to the CPU processor.  Only the cropped pixels are computed.
 *   src   : packed uint8 HWC RGB images, image i at byte src_offset (H x W x 3, rows contiguous); src_bytes bounds them all;
 *   tab   : int32 table of the resampler, built on the host in float64 (Pillow's operation order): per crop column j of image i,
 *           the pair (xmin, n) at tab[bx + 2j] and n <= kx fixed-point (22-bit) weights at tab[cx + j*kx]; likewise per crop row
 *           (ymin, n) at tab[by + 2i] and weights at tab[cy + i*ky];
 *   lut   : fp32 [3, 256]: the normalised value of every (channel, uint8) pair;
 *   out   : fp32 [B, 3, S, S] (what d2r_patchify consumes), OVERWRITTEN;
 *   ws    : the uint8 rows of the horizontal pass, >= d2r_clip_preprocess_ws_bytes(); image i owns [ws_offset, ws_offset +
 *           nrows * S * 3), regions in image order and disjoint.
 * h_desc / h_tab are host copies of desc / tab: every bound is checked on them before anything is enqueued, and a refused call
 * (D2R_ERR_INVALID / D2R_ERR_WORKSPACE) writes nothing.  A crop larger than the resized image is refused (no padding). */
typedef struct {
  int64_t src_offset;  /* byte offset of the image in src */
  int H, W;            /* source rows, columns */
  int rh, rw;          /* size after the resize */
  int top, left;       /* crop origin in the resized image */
  int kx, ky;          /* weights per crop column / row (row stride in tab) */
  int bx, cx, by, cy;  /* int32 offsets into tab (see above) */
  int row0, nrows;     /* source rows [row0, row0 + nrows) the horizontal pass covers (every crop row's support) */
  int64_t ws_offset;   /* byte offset of the image's intermediate rows in ws */
} d2r_clip_image_desc;
size_t d2r_clip_preprocess_ws_bytes(const d2r_clip_image_desc* h_desc, int B, int S);
int d2r_clip_preprocess(const uint8_t* src, int64_t src_bytes, const d2r_clip_image_desc* h_desc, const d2r_clip_image_desc* desc,
                        int B, int S, const int32_t* h_tab, const int32_t* tab, int64_t tab_len, const float* lut, float* out,
                        void* ws, size_t ws_bytes, void* stream);
/* K20  Device-resident dataset cache (d2r_amd/cache.py, --cache_dataset device): the uint8 crop the vertical pass of
 * d2r_clip_preprocess feeds to lut is a lossless cache entry (the pixel values are a function of it and the channel alone).
 * A cache is uint8 [cache_rows, d2r_clip_cache_row_bytes(S)], 16-byte aligned; a row holds one image's crop, planar [3, S, S], and
 * padding up to a multiple of 16 bytes (3 * S * S rounded up) that nothing reads as pixels.
 *
 * d2r_clip_preprocess_u8: d2r_clip_preprocess without the table - same src / desc / tab / ws and the same two passes, image b's crop
 * written to cache row slots[b] (the row's padding is left alone).  h_slots is the host copy of slots (int64 [B]): every slot must
 * lie in [0, cache_rows) and be named once per call; together with the descriptor checks of d2r_clip_preprocess this is verified
 * before anything is enqueued, and a refused call writes nothing.
 *
 * d2r_clip_cache_gather: out[b, c, i, j] = lut[c][cache[idx[b]][c, i, j]], fp32 [B, 3, S, S], OVERWRITTEN - bit for bit what
 * d2r_clip_preprocess writes for the same images (what d2r_patchify consumes).  Indices may repeat; h_idx is the host copy of idx
 * (int64 [B]) and an index outside [0, cache_rows) is refused before the launch.
 *
 * d2r_gather_rows: dst[b][0..row_bytes) = src[h_idx[b]][0..row_bytes) for b < B, rows of src and dst back to back (the token ids,
 * masks, segment ids and labels of a cached batch).  16-byte accesses when dst, src and row_bytes are multiples of 16, otherwise
 * 8-, 4- or 1-byte ones.  An index outside [0, src_rows) is refused before the launch; dst must not overlap src. */
size_t d2r_clip_cache_row_bytes(int S);
int d2r_clip_preprocess_u8(const uint8_t* src, int64_t src_bytes, const d2r_clip_image_desc* h_desc, const d2r_clip_image_desc* desc,
                           int B, int S, const int32_t* h_tab, const int32_t* tab, int64_t tab_len, uint8_t* cache,
                           int64_t cache_rows, const int64_t* h_slots, const int64_t* slots, void* ws, size_t ws_bytes, void* stream);
int d2r_clip_cache_gather(const uint8_t* cache, int64_t cache_rows, const int64_t* h_idx, const int64_t* idx, int B, int S,
                          const float* lut, float* out, void* stream);
int d2r_gather_rows(void* dst, const void* src, int64_t src_rows, int64_t row_bytes, const int64_t* h_idx, const int64_t* idx, int B,
                    void* stream);
/* K21  Image augmentation on the cache rows (d2r_amd/augment.py, --aug_crop_scale / --aug_flip).  d2r_clip_cache_augment is
 * d2r_clip_cache_gather with a box per output sample that is cut out of the normalised crop, resized bilinearly to S x S and mirrored when flip is set - torch's
 * interpolate(mode="bilinear", align_corners=False) on lut[c][crop][:, y0:y0+h, x0:x0+w], then .flip(-1).
 * Per sample b (row P = cache[idx[b]], T[c][v] = lut[c*256 + v]), channel c and output pixel (i, j):
 *   jj = flip ? S-1-j : j;  nx = max((2*jj+1)*w - S, 0) in integers;  ix0 = nx / (2*S), ix1 = min(ix0+1, w-1),
 *   fx = float(nx % (2*S)) / float(2*S);  ny, iy0, iy1, fy likewise from i and h;
 *   out[b,c,i,j] = (1-fy)*((1-fx)*a + fx*b_) + fy*((1-fx)*c_ + fx*d_) in fp32, every operation rounded on its own, with
 *   a, b_, c_, d_ = T[c][P[c, y0+iy{0,1}, x0+ix{0,1}]].
 * The upper taps are clamped to the box, not to the crop.  The box (0, 0, S, S) with flip 0 has fx = fy = 0 and ix0 = j: the call
 * then writes the very bits d2r_clip_cache_gather writes.  out is fp32 [B, 3, S, S], OVERWRITTEN.
 * One descriptor per output sample, 32 bytes, the reserved fields zero.  h_idx / h_aug are the host copies of idx / aug: an index
 * outside [0, cache_rows), a box with x0 < 0, y0 < 0, w < 1, h < 1, x0 + w > S or y0 + h > S, or a flip other than 0 / 1 is refused
 * before anything is enqueued, and a refused call writes nothing. */
typedef struct {
  int32_t x0, y0;      /* box origin in the crop (column, row) */
  int32_t w, h;        /* box size: 1 <= w <= S - x0, 1 <= h <= S - y0 */
  int32_t flip;        /* 1: mirrored horizontally after the resize */
  int32_t reserved[3]; /* zero */
} d2r_clip_augment_desc;
int d2r_clip_cache_augment(const uint8_t* cache, int64_t cache_rows, const int64_t* h_idx, const int64_t* idx,
                           const d2r_clip_augment_desc* h_aug, const d2r_clip_augment_desc* aug, int B, int S, const float* lut,
                           float* out, void* stream);
/* K22  Photometric augmentation on the cache rows (d2r_amd/augment.py, --aug_brightness / --aug_contrast / --aug_saturation /
 * --aug_hue / --aug_grayscale / --aug_erase).  d2r_clip_cache_augment_photo is d2r_clip_cache_augment on the RAW values: for sample b,
 * x[c,i,j] is K21's resample (the same box, taps, fx / fy, blend and mirror) of float(P[c,.,.]) * rescale in place of the table's
 * entries, a value in [0, 1]; then, in this fixed order, with g(x) = 0.299*x_R + 0.587*x_G + 0.114*x_B and clamp to [0, 1]:
 *   1. brightness: x <- clamp(brightness * x);
 *   2. contrast:   m = mean of g(x) over the S*S pixels of the sample after step 1;  x <- clamp(contrast * x + (1 - contrast) * m);
 *   3. saturation: x <- clamp(saturation * x + (1 - saturation) * g(x)) per pixel;
 *   4. hue:        RGB -> HSV by the hexcone formulas (v = max, s = (max - min) / max, s = 0 when max = 0; h = 0 when max = min,
 *                  else ((G-B)/(max-min) | 2 + (B-R)/(max-min) | 4 + (R-G)/(max-min)) / 6 by which channel is the maximum, R first),
 *                  h <- frac(h + hue), HSV -> RGB;
 *   5. gray = 1:   all three channels <- g(x);
 *   6. normalise:  (x - mean[c]) / std[c];
 *   7. erase box:  output pixels ex0 <= j < ex0 + ew, ey0 <= i < ey0 + eh become 0.0f in all channels (ew = 0: none).
 * Steps 1 - 3 are torchvision's float-tensor adjust_brightness / adjust_contrast / adjust_saturation, step 4 its adjust_hue, step 7
 * its RandomErasing(value=0) after Normalize; the order is fixed (the random permutation torchvision's ColorJitter draws is not
 * built).  A step whose factor is the identity (brightness, contrast, saturation = 1, hue = 0) is skipped, so a sample with everything
 * off is fl(fl(x - mean[c]) / std[c]) of the resample, and with the identity box x = fl(float(P) * rescale).  fp32 throughout.
 *   h_norm : HOST array of six floats, mean[0..3) then std[0..3) (std > 0); they and rescale reach the kernel by value;
 *   ws     : float workspace, >= d2r_clip_cache_augment_photo_ws_bytes(B, S) bytes: ceil(S * ceil(S/4) / 256) partial sums of g per
 *            sample.  It is written and read only when some sample of the batch has contrast != 1 (a pass of its own recomputes the
 *            resample and step 1 and adds g in a fixed order: no floating-point atomics, a second run gives the same bits);
 *   out    : fp32 [B, 3, S, S], OVERWRITTEN.
 * One d2r_clip_photo_desc per output sample, 48 bytes, next to its d2r_clip_augment_desc.  h_idx / h_aug / h_photo are the host
 * copies of idx / aug / photo: everything d2r_clip_cache_augment refuses, a factor that is negative or not finite, |hue| > 0.5, a gray
 * other than 0 / 1, an erase box that is neither empty nor inside S x S, a non-zero reserved field, a mean / std / rescale that is not
 * finite (std, rescale > 0) or a short workspace (D2R_ERR_WORKSPACE) is refused before anything is enqueued; a refused call writes
 * nothing. */
typedef struct {
  float brightness, contrast, saturation; /* factors >= 0; 1 = off */
  float hue;                              /* shift in turns, |hue| <= 0.5; 0 = off */
  int32_t gray;                           /* 1: grayscale */
  int32_t ex0, ey0, ew, eh;               /* erase box in output coordinates (column, row, width, height); ew = 0: none */
  int32_t reserved[3];                    /* zero */
} d2r_clip_photo_desc;
size_t d2r_clip_cache_augment_photo_ws_bytes(int B, int S);
int d2r_clip_cache_augment_photo(const uint8_t* cache, int64_t cache_rows, const int64_t* h_idx, const int64_t* idx,
                                 const d2r_clip_augment_desc* h_aug, const d2r_clip_augment_desc* aug,
                                 const d2r_clip_photo_desc* h_photo, const d2r_clip_photo_desc* photo, int B, int S, const float* h_norm,
                                 float rescale, float* out, void* ws, size_t ws_bytes, void* stream);
/* K24  MixUp / CutMix of a finished pixel batch (d2r_amd/mix.py, --aug_mixup / --aug_cutmix).  in and out are fp32 [B, 3, S, S], the
 * pixel values every batch-building path produces; out is OVERWRITTEN and must not overlap in (sample b reads sample partner_b).
 * One descriptor of eight int32 per sample: {partner, the fp32 bits of a, x0, y0, w, h, 0, 0}.  For sample b, channel c, pixel (y, x):
 *   out[b,c,y,x] = in[partner,c,y,x]                               if x0 <= x < x0+w and y0 <= y < y0+h   (the box; bit for bit)
 *                = in[b,c,y,x]                                     else if a == 1                         (a copy, bit for bit)
 *                = fl(fl(a * in[b,c,y,x]) + fl(fl(1-a) * in[partner,c,y,x]))   otherwise, in fp32, every operation rounded on its own.
 * w == 0 or h == 0 is an empty box.  a == 1 with an empty box still writes the copy.  One float4 per lane when S is a multiple of 4
 * and in and out are 16-byte aligned, single loads and stores otherwise; the partner is not read where it is not needed.
 * h_desc is the host copy of desc.  Refused before anything is enqueued (a refused call writes nothing): a null pointer, B outside
 * [1, 65535], S outside [1, 4096], in / out / desc not 4-byte aligned, out overlapping in, a partner outside [0, B), an a that is
 * not finite or outside [0, 1], a negative w or h, a box that does not lie inside [0, S] x [0, S]. */
int d2r_image_mix(const float* in, float* out, int B, int S, const int32_t* h_desc, const int32_t* desc, void* stream);
/* K25  PatchDropout (d2r_amd/patch_dropout.py, --patch_dropout): the vision embedding on a kept subset of the patches.  Every sample keeps
 * its class token and K of its np patches; d2r_patchify, d2r_clip_embed_finish and d2r_clip_embed_bwd each get a form that takes the
 * kept positions, so that the dropped patches are never read, never multiplied and never enter the tower.
 *   keep / h_keep : int32 [B, K] on the device and its host copy: per sample the kept patch positions (raster order, 0 .. np-1),
 *                   strictly increasing.
 * Checked on h_keep before anything is enqueued (a refused call writes nothing, d2r_last_error names the entry point): a null pointer,
 * B < 1, K outside [1, np], an index outside [0, np), a row that is not strictly increasing (a repeated index included), a bad dtype,
 * a pointer that is not aligned to its element size, and what the entry point's counterpart refuses.
 *
 * d2r_patchify_keep: patches[b*K + j, (c*p + i)*p + jj] = pixels[b, c, py*p + i, px*p + jj] with (py, px) = (keep[b,j] / (W/p),
 * keep[b,j] % (W/p)); patches is T [B*K, 3*p*p], OVERWRITTEN; only kept patches are read.  float4 loads along a patch row and one
 * 16-byte store per 8 (16-bit) or 4 (fp32) elements when p is a multiple of that count and pixels and patches are 16-byte aligned
 * (p = 16, 32), element by element otherwise (p = 14); both give the same bits.
 *
 * d2r_clip_embed_finish_keep: in place on x [B, 1+K, D], rows 1.. holding the patch GEMM output: x[b,0] = cls + pos[0];
 * x[b,1+j] = x[b,1+j] + pos[1 + keep[b,j]].  pos is fp32 [1+np, D]; the add is in fp32 and rounded once, as d2r_clip_embed_finish's.
 *
 * d2r_clip_embed_bwd_keep: dX is [B, 1+K, D]; dpos fp32 [1+np, D] and dcls fp32 [D] are OVERWRITTEN: dpos[0] = sum_b dX[b,0];
 * dpos[1+q] = the sum of dX[b, 1+j] over the samples b with keep[b,j] == q, in ascending b, in fp32 from 0.f; a position no sample
 * kept gets +0; dcls = dpos[0].  No atomics: a second run gives the same bits.
 *
 * With K == np and keep[b,j] == j each of the three writes bit for bit what its counterpart writes. */
int d2r_patchify_keep(int dtype, const float* pixels, int B, int H, int W, int p, const int32_t* h_keep, const int32_t* keep, int K,
                      void* patches, void* stream);
int d2r_clip_embed_finish_keep(int dtype, void* x, const float* cls, const float* pos, const int32_t* h_keep, const int32_t* keep,
                               int B, int K, int np, int D, void* stream);
int d2r_clip_embed_bwd_keep(int dtype, const void* dX, const int32_t* h_keep, const int32_t* keep, int B, int K, int np, int D,
                            float* dcls, float* dpos, void* stream);
/* K23  Text augmentation on the token rows (d2r_amd/text_augment.py, --aug_token_delete / --aug_token_mask / --aug_token_replace /
 * --aug_whole_word).  d2r_token_augment builds the three token tensors of a batch from their source rows - what three d2r_gather_rows
 * calls do - and deletes, masks or replaces tokens per sample on the way.
 *   ids, mask, seg : int64 [rows, L] on the device (the cache's tensors, or the batch's own);
 *   idx / h_idx    : the B source rows (int64 [B] on the device) and their host copy;
 *   plan / h_plan  : uint32 [B, L] on the device and its host copy, one word per output sample and SOURCE position: bits 0-1 the op
 *                    (0 keep, 1 delete, 2 mask, 3 replace), bits 2-31 the replacement id;
 *   cont           : uint8 [vocab] on the device, 1 where an id is a continuation piece of a word ("##..."), or NULL;
 *   out_ids, out_mask, out_seg : int64 [B, L], OVERWRITTEN.
 * For output sample b with source row r = idx[b]:
 *   - real tokens: n = the number of non-zero entries of mask[r]; the real tokens are the positions 0..n-1 (a mask that is not a
 *     prefix of ones is outside the contract; whatever it is, nothing outside the rows is read or written);
 *   - content positions: 0 ([CLS]) and n-1 ([SEP]) are never touched; the content positions are 1 <= l <= n-2, none when n <= 2 (the
 *     row then comes out unchanged);
 *   - word heads: l is a head if l == 1, or cont == NULL, or ids[r][l] lies outside [0, vocab) (the table is never read out of
 *     range); otherwise exactly when cont[ids[r][l]] == 0;
 *   - effective op: w(l) = the largest head <= l; the effective op of l is the op of plan[b][w(l)], so a word's pieces share their
 *     head's fate.  With cont == NULL every position is its own word;
 *   - keep-one rule: if the effective op of EVERY content position is delete, none is deleted: they are all kept, a post never
 *     becomes [CLS] [SEP].  Applied after the word propagation (mask and replace cannot occur in such a row);
 *   - value at a surviving content position: keep ids[r][l], mask mask_id, replace plan[b][l] >> 2 - the position's OWN replacement
 *     id, even when the op came from its head;
 *   - output layout: [CLS], the surviving content tokens in their order, [SEP] at positions 0..n'-1 of out_ids[b]; out_seg[b][j] is
 *     the seg value of the source position that landed at j, out_mask[b][j] = 1; positions n'..L-1 get pad_id, 0 and 0.
 * With an all-zero plan the three outputs are bit for bit what d2r_gather_rows gives for the three tensors, for rows whose padding is
 * pad_id / 0 / 0 and whose mask is a prefix of ones (what the data layer writes).  Integer work only: a second run gives the same bits.
 * Checked on the host copies before anything is enqueued (a refused call writes nothing): a null pointer other than cont, B outside
 * [1, 65535], L outside [2, 1024], rows < 1, an h_idx outside [0, rows), vocab < 1, mask_id or pad_id outside [0, vocab), a plan word
 * whose replacement id is >= vocab (with op 3, or with any other op: a continuation piece takes its head's op and its own id), int64
 * pointers that are not 8-byte or plan pointers that are not 4-byte aligned, an output range that overlaps an input tensor or
 * another output. */
int d2r_token_augment(const int64_t* ids, const int64_t* mask, const int64_t* seg, int64_t rows, int L, const int64_t* h_idx,
                      const int64_t* idx, const uint32_t* h_plan, const uint32_t* plan, int B, const uint8_t* cont /* or NULL */,
                      int64_t vocab, int64_t mask_id, int64_t pad_id, int64_t* out_ids, int64_t* out_mask, int64_t* out_seg,
                      void* stream);
/* K19  Baseline JPEG decoding of a batch of images on the device (processor/dataset.py:89: Image.open(p).convert("RGB") in the
 * reference's loader workers), bit-identical to libjpeg-turbo's default path as Pillow uses it: Huffman decoding, ISLOW IDCT with
 * its range-limit table, fancy h2v1 / h2v2 chroma upsampling, fixed-point YCbCr -> RGB.  The host (d2r_amd/jpeg.py) parses the
 * markers, removes byte stuffing and splits the scan at RSTn markers; what it accepts (SOF0 / SOF1, 8-bit, one scan, grayscale or
 * YCbCr at 4:4:4 / 4:2:2 / 4:2:0, optional restart interval) is decoded here.
 *   data  : the unstuffed restart segments, segment s at byte seg[s].offset (4-byte aligned), seg[s].bits bits, followed by at least
 *           D2R_JPEG_SEG_PAD zero bytes inside data_bytes;
 *   seg   : image i owns segments [seg0, seg0 + nseg), one per restart interval (nseg == 1 without one); chunk0 numbers the
 *           D2R_JPEG_CHUNK_BITS-bit chunks of the image's segments consecutively (at least one per segment), nchunk in all;
 *   tab   : int32 tables: per component c a 64-entry quantisation table (natural order) at tab[qt[c]], the DC and AC Huffman decode
 *           tables (D2R_JPEG_HUFF_INTS each: look[512] = (length << 8) | symbol for codes of at most 9 bits, maxcode[17],
 *           valoff[17], vals[256]) at tab[dc[c]] and tab[ac[c]];
 *   dst   : image i's uint8 HWC RGB pixels are written to [dst_offset, dst_offset + H * W * 3) (what d2r_clip_preprocess reads);
 *           regions in image order and disjoint;
 *   status: int32 [B], OVERWRITTEN: 0, or an OR of D2R_JPEG_BAD_CODE (no Huffman code matches), D2R_JPEG_SHORT (a segment's data
 *           ends before its last block; the blocks it does not reach stay zero), D2R_JPEG_BAD_RUN (a run of coefficients past the
 *           64th; decoded as libjpeg does).  A bad code reads as symbol 0 after 17 bits and decoding goes on; such an image's pixels
 *           need not match libjpeg's warn-and-continue output.  The other images of the batch are unaffected;
 *   stats : optional int32 [B, 2], OVERWRITTEN: the most synchronisation rounds any workgroup of the image took, and the chunks the
 *           cross-workgroup pass decoded again;
 *   ws    : >= d2r_jpeg_decode_ws_bytes(); image i owns 48 * nchunk bytes at ws_rec (chunk states), 128 bytes per block at ws_coef
 *           (coefficients) and 64 bytes per block at ws_plane (component samples); all ws_rec regions come first, then all ws_coef,
 *           then all ws_plane, each kind in image order, 256-byte aligned and disjoint.
 * h_desc / h_seg / h_tab are host copies of desc / seg / tab: every offset, size, table index and segment bound is checked on them
 * before anything is enqueued, and a refused call (D2R_ERR_INVALID / D2R_ERR_WORKSPACE) writes nothing.  No host read-back: the
 * entropy decode synchronises its chunks on the device (see csrc/jpeg.hip). */
#define D2R_JPEG_CHUNK_BITS 1024
#define D2R_JPEG_SEG_PAD 8
#define D2R_JPEG_HUFF_INTS 802
#define D2R_JPEG_BAD_CODE 1
#define D2R_JPEG_SHORT 2
#define D2R_JPEG_BAD_RUN 4
typedef struct {
  int64_t dst_offset;                /* byte offset of the image's HWC pixels in dst */
  int64_t ws_rec, ws_coef, ws_plane; /* byte offsets of the image's workspace regions */
  int H, W;
  int ncomp;                         /* 1 (grayscale, written as R = G = B) or 3 (YCbCr) */
  int hs, vs;                        /* chroma upsampling ratio: (1, 1), (2, 1) or (2, 2) */
  int fancy;                         /* libjpeg's fancy upsampling (chroma planes wider than 2 samples) */
  int mcux, mcuy;                    /* MCUs per row / column */
  int mcu_blocks;                    /* blocks per MCU (1 for grayscale) */
  int restart;                       /* restart interval in MCUs, 0 = none */
  int seg0, nseg, nchunk;            /* segments [seg0, seg0 + nseg) of seg, chunks in all */
  int h[3], v[3];                    /* blocks of component c per MCU, across and down */
  int bw[3], bh[3];                  /* blocks of component c per row / column (mcux * h[c], mcuy * v[c]) */
  int qt[3], dc[3], ac[3];           /* int32 offsets of component c's tables in tab */
  int mcu_map[10];                   /* block j of an MCU: component | (column in the MCU << 4) | (row in the MCU << 8) */
} d2r_jpeg_image_desc;
typedef struct {
  int64_t offset;  /* byte offset in data */
  int bits;        /* entropy-coded bits of the segment */
  int chunk0;      /* the image's chunk index of the segment's first chunk */
} d2r_jpeg_segment;
size_t d2r_jpeg_decode_ws_bytes(const d2r_jpeg_image_desc* h_desc, int B);
int d2r_jpeg_decode(const uint8_t* data, int64_t data_bytes, const d2r_jpeg_image_desc* h_desc, const d2r_jpeg_image_desc* desc, int B,
                    const d2r_jpeg_segment* h_seg, const d2r_jpeg_segment* seg, int nseg, const int32_t* h_tab, const int32_t* tab,
                    int64_t tab_len, uint8_t* dst, int64_t dst_bytes, int32_t* status, int32_t* stats, void* ws, size_t ws_bytes,
                    void* stream);
/* x[b,0,:] = cls + pos[0]; x[b,1+i,:] = patch_emb[b,i,:] + pos[1+i]  (in place on x [B,1+np,D], rows 1.. already
 * hold the patch GEMM output) */
int d2r_clip_embed_finish(int dtype, void* x, const float* cls, const float* pos, int B, int ntok, int D,
                          void* stream);
/* dcls[d] = sum_b dX[b,0,d]; dpos[t,d] = sum_b dX[b,t,d]  (fp32, OVERWRITTEN) */
int d2r_clip_embed_bwd(int dtype, const void* dX, int B, int ntok, int D, float* dcls, float* dpos, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K14 fused AdamW over a flat fp32 parameter range (modules/train.py:287-322: torch.optim.AdamW defaults
 * betas=(0.9,0.999), eps=1e-8, weight_decay=1e-2, decoupled) + optional 16-bit shadow copy of the weights.
 * lr already includes the schedule factor; step is the 1-based step count (bias correction).
 * ------------------------------------------------------------------------------------------------ */
int d2r_adamw_step(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                   const int* d_skip /*or NULL*/, void* stream);
/* hipGraph-capturable form: the per-step scalars {lr, 1-beta1^t, sqrt(1-beta2^t), grad_scale} are read from the
 * device array d_hyper[4], which the host refreshes before every graph replay.
 * w16 / w16_dtype: optional 16-bit shadow copy of the weights (D2R_BF16 or D2R_F16) rewritten by the same pass.
 * d_skip: optional device flag; when *d_skip != 0 the launch changes nothing (loss-scaled fp16 training: the step whose
 * gradients overflowed is dropped, as torch.cuda.amp.GradScaler.step does, without a host round trip). */
int d2r_adamw_step_dev(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t n,
                       const float* d_hyper, float beta1, float beta2, float eps, float weight_decay,
                       const int* d_skip /*or NULL*/, void* stream);
/* Gradient clipping by global norm: torch.nn.utils.clip_grad_norm_(params, max_norm) (norm type 2, error_if_nonfinite=False)
 * ahead of the AdamW step - an extension beyond the reference, which does not clip.
 * The _clip forms of the two AdamW entry points above update with (g * grad_scale) * (*d_coef), d_coef = the coefficient
 * d2r_grad_norm_finish wrote (device float); everything else as d2r_adamw_step / d2r_adamw_step_dev. */
int d2r_adamw_step_clip(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                        const int* d_skip /*or NULL*/, const float* d_coef, void* stream);
int d2r_adamw_step_dev_clip(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t n,
                            const float* d_hyper, float beta1, float beta2, float eps, float weight_decay,
                            const int* d_skip /*or NULL*/, const float* d_coef, void* stream);
/* Weight EMA (torch_ema.ExponentialMovingAverage, use_num_updates=True) in the same pass - an extension beyond the reference.
 * The _ema forms of the two AdamW entry points above also update ema[i] += omd * (w_new[i] - ema[i]), omd = 1 - decay_t
 * (ema_one_minus_decay in [0, 1] by value; the hipGraph form reads the device float d_ema_one_minus_decay, d_hyper keeps its
 * layout), w_new = the fp32 weight just computed.  ema: fp32 [n], 16-byte aligned, not w; a step dropped by d_skip leaves it
 * untouched.  d_coef is optional here (NULL: no clipping); everything else as d2r_adamw_step / d2r_adamw_step_dev. */
int d2r_adamw_step_ema(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                       const int* d_skip /*or NULL*/, const float* d_coef /*or NULL*/, float* ema, float ema_one_minus_decay,
                       void* stream);
int d2r_adamw_step_dev_ema(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t n,
                           const float* d_hyper, float beta1, float beta2, float eps, float weight_decay,
                           const int* d_skip /*or NULL*/, const float* d_coef /*or NULL*/, float* ema,
                           const float* d_ema_one_minus_decay, void* stream);
/* Per-parameter hyper-parameters (layer-wise learning-rate decay, no weight decay on biases and normalisation parameters) - an
 * extension beyond the reference, whose four groups each have one lr and one weight decay.  ONE launch over the flat buffers
 * replaces the launch per group of the entry points above: a small device table gives {lr scale, weight decay, group} per element
 * range, the per-step scalars still arrive per group.
 * Segment s covers the elements [end[s-1], end[s]) of the flat buffers, end[-1] = 0; the ends are strictly increasing and the last
 * one is the buffers' length.  `reserved` must be 0. */
#define D2R_ADAMW_MAX_SEGMENTS 4096 /* segments of one table (the full model needs at most one per parameter) */
#define D2R_ADAMW_MAX_GROUPS 8      /* groups a table may name */
typedef struct {
  int64_t end;        /* one past the segment's last element */
  float lr_scale;     /* finite, >= 0: the element's lr is lr[group] * lr_scale (one fp32 multiply, so 1 gives lr[group] itself) */
  float weight_decay; /* finite, >= 0 */
  int32_t group;      /* in [0, ngroups) */
  int32_t reserved;   /* 0 */
} d2r_adamw_seg;
/* Host only: enqueues nothing and needs no GPU.  Refuses (D2R_ERR_INVALID, d2r_last_error names the offending segment) an nseg
 * outside 1..D2R_ADAMW_MAX_SEGMENTS, an ngroups outside 1..D2R_ADAMW_MAX_GROUPS, ends that are not strictly increasing, a last end
 * != n, a non-finite or negative lr_scale or weight_decay, a group outside [0, ngroups) and a non-zero reserved - the host copy of a
 * descriptor is checked before anything reads its device copy, as d2r_jpeg_decode checks h_desc.  The step entry points below
 * cannot read d_table; they trust a table that passed here. */
int d2r_adamw_table_check(const d2r_adamw_seg* host_table, int nseg, int64_t n, int ngroups);
/* Extends d2r_adamw_step_ema (and with it d2r_adamw_step / d2r_adamw_step_clip: d_coef and ema are both optional here).
 * w, g, m, v, w16 and ema are the BASE pointers of the whole flat buffers (element 0), [begin, end) is the absolute element range
 * this launch updates: begin % 4 == 0 (the sharded optimiser's stripes are 16-byte aligned), end arbitrary,
 * 0 <= begin <= end <= n, n = the table's last end as given to d2r_adamw_table_check.  d_table: device copy of the checked table.
 * lr: HOST float[ngroups], the scheduled learning rate of each group.  Element i in segment s of group q is updated as
 * d2r_adamw_step updates an element, with lr = lr[q] * lr_scale[s] and weight_decay[s].  The arithmetic of an element is one piece
 * of code compiled without floating-point contraction, whichever lookup found its hyper-parameters and wherever it lies in
 * [begin, end) (the last (end - begin) % 4 elements go through it as a masked pack): the result does not depend on how [0, n) is
 * cut into launches, bit for bit.  lr_scale == 0 leaves w as it is and still updates m, v (and ema, the shadow).
 * A refused call writes nothing; begin == end launches nothing. */
int d2r_adamw_step_table(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t begin,
                         int64_t end, const d2r_adamw_seg* d_table, int nseg, int64_t n, const float* lr, int ngroups, float beta1,
                         float beta2, float eps, int64_t step, float grad_scale, const int* d_skip /*or NULL*/,
                         const float* d_coef /*or NULL*/, float* ema /*or NULL*/, float ema_one_minus_decay, void* stream);
/* hipGraph-capturable form, extends d2r_adamw_step_dev_ema: d_hyper = device float[ngroups][4], row q = {lr, 1-beta1^t,
 * sqrt(1-beta2^t), grad_scale} of group q (the layout d2r_adamw_step_dev reads one row of).  lr is read from the row of the
 * element's group; the bias corrections and grad_scale belong to the step, not to a group, and are read from row 0.
 * d_ema_one_minus_decay: device float, read when ema is given. */
int d2r_adamw_step_table_dev(float* w, const float* g, float* m, float* v, void* w16 /*or NULL*/, int w16_dtype, int64_t begin,
                             int64_t end, const d2r_adamw_seg* d_table, int nseg, int64_t n, const float* d_hyper, int ngroups,
                             float beta1, float beta2, float eps, const int* d_skip /*or NULL*/, const float* d_coef /*or NULL*/,
                             float* ema /*or NULL*/, const float* d_ema_one_minus_decay /*or NULL without ema*/, void* stream);
/* a[i] <-> b[i] for i < n in one pass (16-byte vector path when both pointers are 16-byte aligned, scalar otherwise); the ranges
 * must not overlap; n == 0 launches nothing.  Evaluation on the averaged weights swaps them in and out with this. */
int d2r_swap_f32(float* a, float* b, int64_t n, void* stream);
#define D2R_GRAD_NORM_PARTS 2048     /* fp64 partial sums one d2r_grad_sumsq call writes */
#define D2R_GRAD_NORM_MAX_RANGES 16  /* element ranges one d2r_grad_sumsq call takes */
/* slab[0..D2R_GRAD_NORM_PARTS) = fp64 partial sums of g[i]^2 over the element ranges h_ranges = host int64
 * {lo0, hi0, lo1, hi1, ...} (nranges of them, each lo a multiple of 4; g 16-byte aligned).  Every partial is written on
 * every call (zeros for empty ranges); the sum of the partials is the same bits on every run (no atomics). */
int d2r_grad_sumsq(const float* g, const int64_t* h_ranges, int nranges, double* slab, int64_t slab_len, void* stream);
/* total = fixed-order sum of slab[0..nparts) (the partials of one or more d2r_grad_sumsq calls, possibly gathered from
 * several ranks); d_out[0] = norm = sqrt(total) * unscale (unscale = *d_unscale when d_unscale is not NULL: the hipGraph form
 * reads d_hyper[3]), d_out[1] = coef = min(1, max_norm / (norm + 1e-6)) in fp32 as torch computes it (NaN stays NaN).
 * d_flag (or NULL): set to 1 when total is not finite, i.e. some gradient is an inf or a NaN - the loss-scaled step's
 * overflow flag, which this pass then raises instead of d2r_grad_nonfinite. */
int d2r_grad_norm_finish(const double* slab, int64_t nparts, float unscale, const float* d_unscale /*or NULL*/, float max_norm,
                         float* d_out, int* d_flag /*or NULL*/, void* stream);
/* dst[r][0..width) = src[r][0..width) for r < rows; pitches and width in BYTES (16-byte vector path when everything is 16-byte
 * aligned).  One launch - the runtime's device-to-device hipMemcpy2DAsync issues one blit kernel per row for these shapes. */
int d2r_copy_rows(void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width, int64_t rows, void* stream);
/* *d_flag |= 1 when g[0..n) holds an inf or a NaN (d_flag is device memory the caller zeroes; one pass over g). */
int d2r_grad_nonfinite(const float* g, int64_t n, int* d_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D2R_HIP_H */
