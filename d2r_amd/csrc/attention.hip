// attention.hip — K3 fused multi-head attention core: sequences up to 256 tokens with the whole head resident in LDS, longer ones
// (up to 1024) through the block loop described in attention_impl.inc; bf16 or fp16.
//
//   O = softmax(scale * Q K^T + mask) V (+ residual)      per (batch, head), head dim 64 or 48
//
// Replaces (reference file:line): BertSelfAttention scores/softmax/context (models/modeling_unimo.py:385-424),
// CLIPAttention (:150-215) and the 16-head self-attention of the intra-modal reasoning cell
// (models/SelfAttention.py:20-60) — there three launches (batched QK^T GEMM, softmax, batched PV GEMM) that write
// and re-read the [B,H,L,L] score and probability tensors; here one launch that keeps them in registers.
//
// Forward: one 512-thread workgroup per (b, h); K and V of the head sit in LDS ([key][64+8] bf16) and each wave
// takes 16 query rows per round.  A wave computes S^T = K Q^T for its 16 queries with v_mfma_f32_16x16x32_bf16 — in the MFMA C layout a lane then
// holds ONE query (col = lane&15) and 4 keys per tile, so the softmax is a per-lane loop plus two cross-lane steps
// (xor 16, 32), and the probabilities are already laid out as the B operand of O^T = V^T P^T (k-slot j of lane group
// g <-> key 32u + 4g + j, 32u + 16 + 4g + j-4); V^T fragments come from LDS through ds_read_b64_tr_b16 with the
// same key permutation.  No LDS round trip for P, no [L,L] tensor in HBM; the only extra output is the row
// log-sum-exp (fp32) the backward needs.
//
// Backward: one 512-thread workgroup per (b, h) with Q, K, V, dO resident in LDS.  Phase A (a wave owns 16
// queries): recompute P^T, dP^T = V dO^T, D = rowsum(P.dP), dS^T, dQ^T = K^T dS^T.  Phase B (a wave owns 16 keys):
// recompute P and dS in the other orientation (rows = queries), dV^T += dO^T P, dK^T += Q^T dS.  Fixed summation
// order, no atomics.
// K2 / K4: single-head attention over the full 768-wide feature (CrossModalAlignment, models/XModules.py:300-310 and
// models/Refinement.py:105-115, logit scale 100/sqrt(768); ContextRichCrossModalCell core, models/Cells.py:244-246,
// unscaled, residual Qs).  Algorithmic traffic B*(2Lq+2Lk)*768*2 bytes: HBM-bound on paper.
//
// Forward: a 512-thread workgroup owns 32 query rows of one sample.
//   phase 1  S^T = K Q^T over the 768-wide contraction: wave w computes the key tiles {w, w+8} x both 16-query
//            tiles; K fragments stream straight from global memory (each lane 16 contiguous bytes of one key row),
//            Q fragments come from LDS (staged once).  Row max / sum are combined across waves through LDS; the
//            normalised probabilities go to LDS as bf16 [query][key].
//   phase 2  O^T = V^T P^T: wave w owns output columns [96w, 96w+96); it streams ITS [32 keys x 96] sub-block of V
//            through a private double-buffered LDS slab (registers -> LDS, hardware-transposed back with
//            ds_read_b64_tr_b16), so phase 2 needs no workgroup barrier at all.
// Nothing of size [Lq, Lk] reaches HBM; the extra output is the row log-sum-exp for the backward pass.
//
#include <math.h>
#include <stdlib.h>

#include "attn_trace.h"
#include "gemm_args.h"
#include "ktimer.h"

extern "C" int d2r_mha_supported(int dtype, int Lq, int Lk, int head_dim) {
  return d2r_is16(dtype) && (head_dim == 64 || head_dim == 48) && Lq >= 1 && Lk >= 1 && Lq <= 1024 && Lk <= 1024;
}
extern "C" int d2r_xattn_supported(int dtype, int Lq, int Lk, int D) {
  return d2r_is16(dtype) && D == 768 && Lq >= 1 && Lk >= 1 && Lk <= 640;
}
int d2r_xattn2_fwd_try(int dtype, int ncore, const void* const* q, int64_t ldq, int64_t sqb, const void* const* k, int64_t ldk, int64_t skb,
                       const void* const* v, int64_t ldv, int64_t svb, void* const* o, int64_t ldo, int64_t sob, const void* const* residual,
                       int64_t ldr, int64_t srb, const float* mask, float* const* lse, int B, int Lq, int Lk, float scale, hipStream_t st);  // xattn2.hip
int d2r_xattn3_fwd_try(int dtype, int ncore, const void* const* q, int64_t ldq, int64_t sqb, const void* const* k, int64_t ldk, int64_t skb,
                       const void* const* v, int64_t ldv, int64_t svb, void* const* o, int64_t ldo, int64_t sob, const void* const* residual,
                       int64_t ldr, int64_t srb, const float* mask, float* const* lse, int B, int Lq, int Lk, float scale, hipStream_t st);  // xattn3.hip
int d2r_xattn3_bwd_try(int dtype, int ncore, const void* const* q, int64_t ldq, int64_t sqb, const void* const* k, int64_t ldk, int64_t skb,
                       const void* const* v, int64_t ldv, int64_t svb, const void* const* dO, int64_t ldg, int64_t sgb, const void* const* o,
                       int64_t ldo, int64_t sob, const void* const* residual, int64_t ldr, int64_t srb, const float* mask,
                       const float* const* lse, void* const* P, void* const* dS, int lkp, int B, int Lq, int Lk, float scale, hipStream_t st);
int d2r_xattn3_dkv_try(int dtype, int ngroup, const void* const* W, const void* const* X, void* const* out, const int64_t* ldx, const int64_t* sxb,
                       const int64_t* ldo, const int64_t* sob, const int* trans, int lkp, int B, int Lq, int Lk, hipStream_t st);
int d2r_gemm_tn_batched16(int dtype, int M, int m_store, int N, int K, int64_t lda, int64_t sAb, int64_t ldb, int64_t sBb, int64_t ldc,
                          int64_t sCb, const void* const* A, const void* const* B, void* const* C, int ngroups, int nb, void* stream);  // gemm.hip

// ---- record of the launched variants (attn_trace.h; d2r_attn_trace / _read / _codes of include/d2r_hip_probes.h) ----------------------
bool g_d2r_attn_trace = false;
namespace {
constexpr int ATTN_TRACE_CAP = 4096;
int g_attn_trace_n = 0;  // launches since arming (the list keeps the first ATTN_TRACE_CAP of them)
int g_attn_trace_codes[ATTN_TRACE_CAP];
}  // namespace
void d2r_attn_trace_push(int code) {
  if (g_attn_trace_n < ATTN_TRACE_CAP) g_attn_trace_codes[g_attn_trace_n] = code;
  ++g_attn_trace_n;
}
extern "C" void d2r_attn_trace(int on) {
  if (on) g_attn_trace_n = 0;
  g_d2r_attn_trace = on != 0;
}
extern "C" int d2r_attn_trace_read(int* codes, int capacity) {
  const int have = g_attn_trace_n < ATTN_TRACE_CAP ? g_attn_trace_n : ATTN_TRACE_CAP;
  for (int i = 0; codes && i < have && i < capacity; ++i) codes[i] = g_attn_trace_codes[i];
  return g_attn_trace_n;
}
extern "C" int d2r_attn_trace_codes(int* codes, int capacity) {
  int n = 0;
  auto put = [&](int code) {
    if (codes && n < capacity) codes[n] = code;
    ++n;
  };
  for (int dh : {64, 48}) {
    for (int nk32 = 1; nk32 <= 8; ++nk32) put(D2R_AV_MHA_FWD + dh * 100 + nk32), put(D2R_AV_MHA_BWD + dh * 100 + nk32);
    put(D2R_AV_MHA_LONG_FWD + dh * 100), put(D2R_AV_MHA_LONG_DQ + dh * 100), put(D2R_AV_MHA_LONG_DKV + dh * 100);
  }
  for (int code : {D2R_AV_X3_FWD, D2R_AV_X3_BWD, D2R_AV_X3_DKV, D2R_AV_X3_DKV2, D2R_AV_X2_FWD_2_256, D2R_AV_X2_FWD_1_256, D2R_AV_X2_FWD_1_640,
                   D2R_AV_XBWD_2, D2R_AV_XBWD_5, D2R_AV_KEYSIDE_GROUPED, D2R_AV_KEYSIDE_DV, D2R_AV_KEYSIDE_DK})
    put(code);
  return n;
}
// a key-side product of the second generation: recorded when the GEMM entry point took it
static int keyside(int code, int rc) {
  if (rc == 0) d2r_attn_note(code);
  return rc;
}

// one copy of the kernels per 16-bit element type
namespace att_bf16 {
typedef bf16_t E;
#include "attention_impl.inc"
}  // namespace att_bf16
namespace att_f16 {
typedef f16_t E;
#include "attention_impl.inc"
}  // namespace att_f16

#define D2R_BY_DTYPE(dtype, call) ((dtype) == D2R_F16 ? att_f16::call : att_bf16::call)

extern "C" int d2r_mha_fwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                           const void* v, int64_t ldv, int64_t svb, void* o, int64_t ldo, int64_t sob,
                           const void* residual, int64_t ldr, int64_t srb, const float* mask, float* lse, int B, int H,
                           int Lq, int Lk, int head_dim, float scale, float p_drop, uint64_t seed, void* stream) {
  return D2R_BY_DTYPE(dtype, mha_fwd_run(dtype, q, ldq, sqb, k, ldk, skb, v, ldv, svb, o, ldo, sob, residual, ldr, srb, mask, lse, B, H, Lq,
                                         Lk, head_dim, scale, p_drop, seed, stream));
}
extern "C" int d2r_mha_bwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                           const void* v, int64_t ldv, int64_t svb, const void* dO, int64_t ldg, int64_t sgb,
                           const float* mask, const float* lse, float* dsum, void* dq, int64_t lddq, int64_t sdqb, void* dk,
                           int64_t lddk, int64_t sdkb, void* dv, int64_t lddv, int64_t sdvb, int B, int H, int Lq, int Lk,
                           int head_dim, float scale, float p_drop, uint64_t seed, void* stream) {
  return D2R_BY_DTYPE(dtype, mha_bwd_run(dtype, q, ldq, sqb, k, ldk, skb, v, ldv, svb, dO, ldg, sgb, mask, lse, dsum, dq, lddq, sdqb, dk, lddk,
                                         sdkb, dv, lddv, sdvb, B, H, Lq, Lk, head_dim, scale, p_drop, seed, stream));
}
static bool x3_offsets_fit(int64_t ld, int L) { return ld * (int64_t)L < (int64_t)1 << 31; }  // per-sample element offsets are 32-bit in xattn3

extern "C" int d2r_xattn_fwd_multi(int dtype, int ncore, const void* const* h_q, int64_t ldq, int64_t sqb, const void* const* h_k, int64_t ldk,
                                   int64_t skb, const void* const* h_v, int64_t ldv, int64_t svb, void* const* h_o, int64_t ldo, int64_t sob,
                                   const void* const* h_residual, int64_t ldr, int64_t srb, const float* mask, float* const* h_lse, int B,
                                   int Lq, int Lk, int D, float scale, void* stream) {
  // (measurement aid, armed by d2r_gemm_timer: the launch in its real configuration, algorithmic bytes = q, k, v read and o written
  // once per problem)
  D2RTimerScope timed((hipStream_t)stream, 10001, 4.0 * ncore * B * (double)Lq * Lk * D,
                      (double)ncore * B * (2.0 * Lq + 2.0 * Lk) * D * (dtype == D2R_F32 ? 4 : 2));
  if (Lk <= 256 && d2r_xattn_supported(dtype, Lq, Lk, D) && B >= 1 && ncore >= 1 && ncore <= 4 && h_q && h_k && h_v && h_o && h_lse &&
      x3_offsets_fit(ldk, Lk) && x3_offsets_fit(ldv, Lk)) {
    bool ok = true;
    for (int c = 0; c < ncore; ++c)
      ok &= h_lse[c] && h_q[c] && h_k[c] && h_v[c] && h_o[c] && d2r_aligned16(h_q[c]) && d2r_aligned16(h_k[c]) && d2r_aligned16(h_v[c]) &&
            d2r_aligned16(h_o[c]) && (!h_residual || !h_residual[c] || d2r_aligned16(h_residual[c]));
    ok &= ldq % 8 == 0 && sqb % 8 == 0 && ldk % 8 == 0 && skb % 8 == 0 && ldv % 8 == 0 && svb % 8 == 0 && ldo % 8 == 0 && sob % 8 == 0 &&
          (!h_residual || (ldr % 8 == 0 && srb % 8 == 0));
    if (ok && d2r_xattn3_fwd_try(dtype, ncore, h_q, ldq, sqb, h_k, ldk, skb, h_v, ldv, svb, h_o, ldo, sob, h_residual, ldr, srb, mask, h_lse, B, Lq, Lk,
                                 scale, (hipStream_t)stream))
      return d2r_check_launch("d2r_xattn_fwd(v3)");
  }
  return D2R_BY_DTYPE(dtype, xattn_fwd_run(dtype, ncore, h_q, ldq, sqb, h_k, ldk, skb, h_v, ldv, svb, h_o, ldo, sob, h_residual, ldr, srb, mask,
                                           h_lse, B, Lq, Lk, D, scale, stream));
}
extern "C" int d2r_xattn_fwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                             const void* v, int64_t ldv, int64_t svb, void* o, int64_t ldo, int64_t sob,
                             const void* residual, int64_t ldr, int64_t srb, const float* mask, float* lse, int B, int Lq,
                             int Lk, int D, float scale, void* stream) {
  return d2r_xattn_fwd_multi(dtype, 1, &q, ldq, sqb, &k, ldk, skb, &v, ldv, svb, &o, ldo, sob, residual ? &residual : nullptr, ldr, srb, mask,
                             &lse, B, Lq, Lk, D, scale, stream);
}
extern "C" int d2r_xattn_bwd(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                             const void* v, int64_t ldv, int64_t svb, const void* dO, int64_t ldg, int64_t sgb,
                             const float* mask, const float* lse, void* dq, int64_t lddq, int64_t sdqb, void* P, void* dS,
                             int lkp, int B, int Lq, int Lk, int D, float scale, void* stream) {
  return D2R_BY_DTYPE(dtype, xattn_bwd_run(dtype, 1, &q, ldq, sqb, &k, ldk, skb, &v, ldv, svb, &dO, ldg, sgb, mask, &lse, &dq, lddq, sdqb, &P, &dS,
                                           lkp, B, Lq, Lk, D, scale, stream));
}
extern "C" int d2r_xattn_bwd_multi(int dtype, int ncore, const void* const* h_q, int64_t ldq, int64_t sqb, const void* const* h_k, int64_t ldk,
                                   int64_t skb, const void* const* h_v, int64_t ldv, int64_t svb, const void* const* h_dO, int64_t ldg,
                                   int64_t sgb, const void* const* h_o, int64_t ldo, int64_t sob, const void* const* h_residual, int64_t ldr,
                                   int64_t srb, const float* mask, const float* const* h_lse, void* const* h_dq, int64_t lddq, int64_t sdqb,
                                   void* const* h_dk, int64_t lddk, int64_t sdkb, void* const* h_dv, int64_t lddv, int64_t sdvb,
                                   void* const* h_P, void* const* h_dS, int lkp, int B, int Lq, int Lk, int D, float scale, void* stream) {
  D2R_REQUIRE(h_dk && h_dv && ncore >= 1 && ncore <= 4, "d2r_xattn_bwd_multi: null pointer array / 1..4 problems per launch");
  // (measurement aid: the whole backward op = query-side launch + product launch; algorithmic bytes = 2 x the forward's)
  D2RTimerScope timed((hipStream_t)stream, 10002, 10.0 * ncore * B * (double)Lq * Lk * D,
                      2.0 * ncore * B * (2.0 * Lq + 2.0 * Lk) * D * (dtype == D2R_F32 ? 4 : 2));
  bool x3 = Lk <= 256 && h_o && d2r_xattn_supported(dtype, Lq, Lk, D) && B >= 1 && h_q && h_k && h_v && h_dO && h_lse && h_dq &&
            h_P && h_dS && lkp >= Lk && lkp % 8 == 0 && x3_offsets_fit(ldk, Lk) && x3_offsets_fit(ldv, Lk);
  if (x3) {
    for (int c = 0; c < ncore; ++c)
      x3 &= h_lse[c] && h_q[c] && h_k[c] && h_v[c] && h_dO[c] && h_o[c] && h_dq[c] && h_P[c] && h_dS[c] && d2r_aligned16(h_q[c]) &&
            d2r_aligned16(h_k[c]) && d2r_aligned16(h_v[c]) && d2r_aligned16(h_dO[c]) && d2r_aligned16(h_o[c]) && d2r_aligned16(h_dq[c]) &&
            d2r_aligned16(h_P[c]) && d2r_aligned16(h_dS[c]) && (!h_residual || !h_residual[c] || d2r_aligned16(h_residual[c]));
    x3 &= ldq % 8 == 0 && sqb % 8 == 0 && ldk % 8 == 0 && skb % 8 == 0 && ldv % 8 == 0 && svb % 8 == 0 && ldg % 8 == 0 && sgb % 8 == 0 &&
          ldo % 8 == 0 && sob % 8 == 0 && lddq % 8 == 0 && sdqb % 8 == 0 && (!h_residual || (ldr % 8 == 0 && srb % 8 == 0)) &&
          lddk % 4 == 0 && sdkb % 4 == 0 && lddv % 4 == 0 && sdvb % 4 == 0;
    for (int c = 0; c < ncore && x3; ++c)
      x3 &= h_dk[c] && h_dv[c] && !(reinterpret_cast<uintptr_t>(h_dk[c]) & 7u) && !(reinterpret_cast<uintptr_t>(h_dv[c]) & 7u);
  }
  // third generation: the query-side kernel leaves P and dS; dV = P^T dO, dK = dS^T Q AND dQ = dS K of every sample and problem
  // are then ONE launch of the product kernel (it needs Lq, lkp <= 256)
  if (x3 && Lq <= 256 && lkp <= 256) {
    if (!d2r_xattn3_bwd_try(dtype, ncore, h_q, ldq, sqb, h_k, ldk, skb, h_v, ldv, svb, h_dO, ldg, sgb, h_o, ldo, sob, h_residual, ldr, srb, mask, h_lse,
                            h_P, h_dS, lkp, B, Lq, Lk, scale, (hipStream_t)stream))
      return d2r_fail(D2R_ERR_INVALID, "d2r_xattn_bwd_multi: the third-generation kernel refused an eligible shape");
    if (int rc = d2r_check_launch("d2r_xattn_bwd(v3)")) return rc;
    const void *W[12], *X[12];
    void* O[12];
    int64_t ldx[12], sxb_[12], ldo_[12], sob_[12];
    int tr[12];
    int ng = 0;
    for (int c = 0; c < ncore; ++c) {
      D2R_REQUIRE(h_dk[c] && h_dv[c], "d2r_xattn_bwd_multi: null dk / dv");
      W[ng] = h_P[c], X[ng] = h_dO[c], O[ng] = h_dv[c], ldx[ng] = ldg, sxb_[ng] = sgb, ldo_[ng] = lddv, sob_[ng] = sdvb, tr[ng++] = 0;
      W[ng] = h_dS[c], X[ng] = h_q[c], O[ng] = h_dk[c], ldx[ng] = ldq, sxb_[ng] = sqb, ldo_[ng] = lddk, sob_[ng] = sdkb, tr[ng++] = 0;
      W[ng] = h_dS[c], X[ng] = h_k[c], O[ng] = h_dq[c], ldx[ng] = ldk, sxb_[ng] = skb, ldo_[ng] = lddq, sob_[ng] = sdqb, tr[ng++] = 1;
    }
    if (!d2r_xattn3_dkv_try(dtype, ng, W, X, O, ldx, sxb_, ldo_, sob_, tr, lkp, B, Lq, Lk, (hipStream_t)stream))
      return d2r_fail(D2R_ERR_INVALID, "d2r_xattn_bwd_multi: the product kernel refused an eligible shape (alignment of dq / dk / dv?)");
    return d2r_check_launch("d2r_xattn_bwd(products)");
  }
  if (int rc = D2R_BY_DTYPE(dtype, xattn_bwd_run(dtype, ncore, h_q, ldq, sqb, h_k, ldk, skb, h_v, ldv, svb, h_dO, ldg, sgb, mask, h_lse, h_dq, lddq,
                                                 sdqb, h_P, h_dS, lkp, B, Lq, Lk, D, scale, stream)))
    return rc;
  // second generation: the key side as grouped, batched TN products of the LDS-DMA GEMM kernel.  The two outputs may have
  // different strides (k | v packed in one projection output have the same): one launch per distinct stride pair.
  const void* A[8];
  const void* Bm[8];
  void* C[8];
  if (lddk == lddv && sdkb == sdvb && ldg == ldq && sgb == sqb) {
    for (int c = 0; c < ncore; ++c) {
      D2R_REQUIRE(h_dk[c] && h_dv[c], "d2r_xattn_bwd_multi: null dk / dv");
      A[2 * c] = h_P[c], Bm[2 * c] = h_dO[c], C[2 * c] = h_dv[c];
      A[2 * c + 1] = h_dS[c], Bm[2 * c + 1] = h_q[c], C[2 * c + 1] = h_dk[c];
    }
    return keyside(D2R_AV_KEYSIDE_GROUPED,
                   d2r_gemm_tn_batched16(dtype, lkp, Lk, D, Lq, lkp, (int64_t)Lq * lkp, ldq, sqb, lddk, sdkb, A, Bm, C, 2 * ncore, B, stream));
  }
  for (int c = 0; c < ncore; ++c) A[c] = h_P[c], Bm[c] = h_dO[c], C[c] = h_dv[c];
  if (int rc = keyside(D2R_AV_KEYSIDE_DV,
                       d2r_gemm_tn_batched16(dtype, lkp, Lk, D, Lq, lkp, (int64_t)Lq * lkp, ldg, sgb, lddv, sdvb, A, Bm, C, ncore, B, stream)))
    return rc;
  for (int c = 0; c < ncore; ++c) A[c] = h_dS[c], Bm[c] = h_q[c], C[c] = h_dk[c];
  return keyside(D2R_AV_KEYSIDE_DK,
                 d2r_gemm_tn_batched16(dtype, lkp, Lk, D, Lq, lkp, (int64_t)Lq * lkp, ldq, sqb, lddk, sdkb, A, Bm, C, ncore, B, stream));
}
