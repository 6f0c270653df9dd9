// Host-side record of the attention kernel variants that were launched (measurement aid, include/d2r_hip_probes.h:
// d2r_attn_trace).  Every attention launch site calls d2r_attn_note(code) right after its launch; disarmed that is one
// predictable branch on a host global, and nothing on the device either way.  Process-global, not thread-safe.
//
//   MHA (attention_impl.inc):  family * 10000 + head_dim * 100 + NK32
//     family 1 / 2  short forward / backward (whole head in LDS; NK32 = the kernel's template argument, 1..8)
//     family 3 / 4 / 5  long forward / long dQ / long dK-dV (block loop; NK32 = 0)
//   single-head 768-wide cores: 60000 + n
#pragma once

enum {
  D2R_AV_MHA_FWD = 10000, D2R_AV_MHA_BWD = 20000, D2R_AV_MHA_LONG_FWD = 30000, D2R_AV_MHA_LONG_DQ = 40000, D2R_AV_MHA_LONG_DKV = 50000,
  D2R_AV_X3_FWD = 60001,       // xattn3_fwd_kernel
  D2R_AV_X3_BWD = 60002,       // xattn3_bwd_kernel (query side: P and dS)
  D2R_AV_X3_DKV = 60003,       // xattn3_dkv_kernel (dV, dK, dQ products, full)
  D2R_AV_X3_DKV2 = 60004,      // xattn3_dkv2_kernel (compact)
  D2R_AV_X2_FWD_2_256 = 60011, // xattn2_fwd_kernel<2, 256>
  D2R_AV_X2_FWD_1_256 = 60012, // xattn2_fwd_kernel<1, 256>
  D2R_AV_X2_FWD_1_640 = 60013, // xattn2_fwd_kernel<1, 640>
  D2R_AV_XBWD_2 = 60021,       // xattn_bwd_kernel<2> (second-generation query side, Lk <= 256)
  D2R_AV_XBWD_5 = 60022,       // xattn_bwd_kernel<5> (Lk <= 640)
  D2R_AV_KEYSIDE_GROUPED = 60031,  // second-generation key side: dV and dK of every problem as ONE grouped batched TN launch
  D2R_AV_KEYSIDE_DV = 60032,       // ... as two launches: dV = P^T dO
  D2R_AV_KEYSIDE_DK = 60033,       //                      dK = dS^T Q
};

extern bool g_d2r_attn_trace;         // attention.hip
void d2r_attn_trace_push(int code);  // attention.hip
static inline void d2r_attn_note(int code) {
  if (__builtin_expect(g_d2r_attn_trace, 0)) d2r_attn_trace_push(code);
}
