// attention_impl.inc — the device code and launch helpers of attention.hip, written against an element type `E` (bf16_t or f16_t)
// that the including namespace defines.  attention.hip includes this file once per 16-bit type: the kernels are the same
// instruction for instruction except for the MFMA opcode (H16<E>::mfma32) and the float <-> E conversions.
typedef H16<E>::v8 E8;
typedef H16<E>::v4 E4;

namespace {

struct MhaArgs {
  const E *q, *k, *v, *res, *dO;
  E *o, *dq, *dk, *dv;
  const float* mask;  // additive [B, Lk] or null
  float* lse;         // [B, H, Lq]
  float* dsum;        // [B, H, Lq] D = rowsum(P o dP): long-sequence backward only (dq kernel -> dkv kernel)
  // dropout on the probabilities (models/modeling_unimo.py:388): element (b, h, q, key) is kept iff
  // d2r_rand24(seed, ((b*H + h)*Lq + q)*lkp + key) >= drop_thresh and then scaled by drop_scale = 1/(1-p); lkp = Lk rounded up
  // to 8: the index of the same element in the [B,H,Lq,lkp] probability tensor of the unfused path, so both paths draw ONE mask
  uint32_t drop_thresh;
  float drop_scale;
  uint64_t drop_seed;
  int lkp;
  int64_t ldq, sqb, ldk, skb, ldv, svb, ldo, sob, ldr, srb, ldg, sgb, lddq, sdqb, lddk, sdkb, lddv, sdvb;
  int B, H, Lq, Lk;
  float scale;
};

constexpr int LDW = 72;  // LDS row stride in bf16: 64 columns + 8 pad (144 B: conflict-free b128 and tr16 reads)

// rows [0, TOTAL) x 64 columns of a head slice into LDS; rows >= valid and columns >= DH are zero.  All global
// loads of the slice are issued before the first LDS store (one latency, not one per 16 bytes).
template <int DH, int TOTAL, int NTHREADS>
struct RowStage {  // the register half of a staged slice: load() now, store() after the loads of the other slices are issued
  static constexpr int CHUNKS = TOTAL * 8, IT = (CHUNKS + NTHREADS - 1) / NTHREADS;
  Pack<E, 8> v[IT];
  __device__ __forceinline__ void load(const E* src, int64_t ld, int valid, int tid) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int c = tid + it * NTHREADS, row = c >> 3, col = (c & 7) * 8;
      // out-of-range chunks read element (0, 0) and are zeroed by a select: a branch around the load would put a full
      // memory wait behind every load
      const bool ok = c < CHUNKS && row < valid && col < DH;
      v[it] = ld_pack<E, 8>(src + (ok ? (int64_t)row * ld + col : 0));
#pragma unroll
      for (int j = 0; j < 8; ++j) v[it].v[j] = ok ? v[it].v[j] : (E)0.f;
    }
  }
  __device__ __forceinline__ void store(E* dst, int tid) const {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int c = tid + it * NTHREADS, row = c >> 3, col = (c & 7) * 8;
      if (CHUNKS % NTHREADS == 0 || c < CHUNKS) st_pack<E, 8>(dst + row * LDW + col, v[it]);
    }
  }
};

template <int DH, int TOTAL, int NTHREADS>
__device__ __forceinline__ void fill_rows(E* dst, const E* src, int64_t ld, int valid, int tid) {
  RowStage<DH, TOTAL, NTHREADS> r;
  r.load(src, ld, valid, tid);
  r.store(dst, tid);
}

// two slices: both sets of loads in flight before the first LDS store
template <int DH, int TOTAL, int NTHREADS>
__device__ __forceinline__ void fill_rows2(E* d0, const E* s0, int64_t ld0, int v0, E* d1, const E* s1, int64_t ld1, int v1, int tid) {
  RowStage<DH, TOTAL, NTHREADS> r0, r1;
  r0.load(s0, ld0, v0, tid);
  r1.load(s1, ld1, v1, tid);
  r0.store(d0, tid);
  r1.store(d1, tid);
}

__device__ __forceinline__ E8 lds_frag(const E* p) { return *reinterpret_cast<const E8*>(p); }

// A fragment of M^T for a matrix kept [k][col] in LDS: rows k0 + {0..3} and k0 + 16 + {0..3} of this lane group,
// column c0 + (lane & 15)
__device__ __forceinline__ E8 lds_frag_tr(const E* base, int k0, int c0, int tq, int tp) {
  const E* p0 = base + (k0 + tq) * LDW + c0 + tp * 4;
  const E4 lo = H16<E>::tr_read(p0);
  const E4 hi = H16<E>::tr_read(p0 + 16 * LDW);
  return E8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ E8 pack_frag(const f32x4& a, const f32x4& b) {
  return E8{(E)a[0], (E)a[1], (E)a[2], (E)a[3], (E)b[0], (E)b[1], (E)b[2], (E)b[3]};
}

__device__ __forceinline__ float group4_max(float v) {  // over the 4 lane groups holding one MFMA column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// dropout multiplier of probability (row, key) of (b, h): 0 or 1/(1-p); `row_base` = ((b*H + h)*Lq + q) * lkp
__device__ __forceinline__ float drop_mult(const MhaArgs& a, uint64_t row_base, int key) {
  return d2r_rand24(a.drop_seed, row_base + (uint64_t)key) >= a.drop_thresh ? a.drop_scale : 0.f;
}

template <int DH, int NK32>
__global__ __launch_bounds__(512) void mha_fwd_kernel(MhaArgs a) {
  constexpr int LKP = NK32 * 32, NKT = NK32 * 2, NDT = DH / 16, NW = 8;
  __shared__ __attribute__((aligned(16))) E Ks[LKP * LDW];
  __shared__ __attribute__((aligned(16))) E Vs[LKP * LDW];
  __shared__ __attribute__((aligned(16))) float Ms[LKP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
  const int nqt = (a.Lq + 15) / 16;
  // The kernel is a latency chain (tests/probes/mha_scaling.py: 24 workgroups take as long as 250): a wave's query fragments are
  // requested BEFORE the K / V staging (their latency runs under it), and the next round's during this round's arithmetic.
  E8 qn[2];
  auto loadq = [&](int qt) {
    const int qrow = min(qt * 16 + fr, a.Lq - 1);  // (clamped: rows past Lq are never stored)
    const E* Qg = a.q + b * a.sqb + h * DH + (int64_t)qrow * a.ldq;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int col = kk * 32 + fq * 8;
      if (col < DH) {
        qn[kk] = *reinterpret_cast<const E8*>(Qg + col);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qn[kk][j] = (E)0.f;
      }
    }
  };
  if (wave < nqt) loadq(wave);
  fill_rows2<DH, LKP, 512>(Ks, a.k + b * a.skb + h * DH, a.ldk, a.Lk, Vs, a.v + b * a.svb + h * DH, a.ldv, a.Lk, tid);
  for (int key = tid; key < LKP; key += 512)
    Ms[key] = key < a.Lk ? (a.mask ? a.mask[(int64_t)b * a.Lk + key] : 0.f) : -INFINITY;
  __syncthreads();
  for (int qt = wave; qt < nqt; qt += NW) {  // 16 queries per wave and round; no barrier below
    asm volatile("" ::: "memory");  // keep the (round-invariant) K/V fragment reads inside the round: no hoisting
    const int qrow = qt * 16 + fr;
    const bool qok = qrow < a.Lq;
    E8 qf[2] = {qn[0], qn[1]};
    if (qt + NW < nqt) loadq(qt + NW);
    f32x4 s[NKT];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        acc = H16<E>::mfma32(lds_frag(&Ks[(t * 16 + fr) * LDW + kk * 32 + fq * 8]), qf[kk], acc);
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(&Ms[t * 16 + fq * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r] = acc[r] * a.scale + m4[r];
        mx = fmaxf(mx, acc[r]);
      }
      s[t] = acc;
    }
    mx = group4_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = __expf(s[t][r] - mx);
        sum += s[t][r];
      }
    sum = group4_sum(sum);
    const float inv = 1.f / sum;
    if (fq == 0 && qok) a.lse[((int64_t)b * a.H + h) * a.Lq + qrow] = mx + logf(sum);
    if (a.drop_thresh) {
      const uint64_t rb = (((uint64_t)b * a.H + h) * a.Lq + (qok ? qrow : 0)) * a.lkp;
#pragma unroll
      for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] *= drop_mult(a, rb, t * 16 + fq * 4 + r);
    }
    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NK32; ++u) {
      const E8 pf = pack_frag(s[2 * u] * inv, s[2 * u + 1] * inv);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
        o[dt] = H16<E>::mfma32(lds_frag_tr(Vs, u * 32 + fq * 4, dt * 16, tq, tp), pf, o[dt]);
    }
    if (!qok) continue;
    E* Og = a.o + b * a.sob + h * DH + (int64_t)qrow * a.ldo;
    const E* Rg = a.res ? a.res + b * a.srb + h * DH + (int64_t)qrow * a.ldr : nullptr;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const int c = dt * 16 + fq * 4;
      Pack<E, 4> out;
      if (Rg) {
        const Pack<E, 4> rv = ld_pack<E, 4>(Rg + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) out.v[r] = (E)(o[dt][r] + (float)rv.v[r]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) out.v[r] = (E)o[dt][r];
      }
      st_pack<E, 4>(Og + c, out);
    }
  }
}

// fragment (16 rows x 32 columns of k-step kk, lane (fr, fq): 16 bytes of row r0 + fr) of a head slice straight from global memory;
// rows >= valid and columns >= DH are zero (what RowStage leaves in LDS for them)
template <int DH>
__device__ __forceinline__ E8 global_frag(const E* slice, int64_t ld, int row, int valid, int kk, int fq) {
  const int col = kk * 32 + fq * 8;
  const bool ok = row < valid && col < DH;
  E8 v = *reinterpret_cast<const E8*>(slice + (ok ? (int64_t)row * ld + col : 0));
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = ok ? v[j] : (E)0.f;
  return v;
}

// Round 3: TWO staged slices instead of four.  Phase A (dQ, D) walks all keys - K and V live in LDS, a wave's own 16 query rows of Q
// and dO come straight from global memory as fragments; phase B (dK, dV) walks all queries - the same two LDS regions are refilled
// with Q and dO, a wave's own 16 key rows of K and V come from global memory.  67 KB of LDS instead of 132 KB for 197 tokens: two
// workgroups per CU, so that the 384 (sample, head) workgroups of the vision encoder are all resident instead of running as one and
// a half rounds; the price is a second read of the four slices out of L2.
template <int DH, int NK32>
__global__ __launch_bounds__(512) void mha_bwd_kernel(MhaArgs a) {
  constexpr int LP = NK32 * 32, NT16 = NK32 * 2, NDT = DH / 16, NW = 8;
  __shared__ __attribute__((aligned(16))) E Xs[LP * LDW];  // phase A: K, phase B: Q
  __shared__ __attribute__((aligned(16))) E Ys[LP * LDW];  // phase A: V, phase B: dO
  __shared__ __attribute__((aligned(16))) float Ms[LP];
  __shared__ __attribute__((aligned(16))) float Ls[LP];
  __shared__ __attribute__((aligned(16))) float Ds[LP];
  E* const Ks = Xs;
  E* const Vs = Ys;
  E* const Qs = Xs;
  E* const Gs = Ys;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
  const E* Qg = a.q + b * a.sqb + h * DH;
  const E* Kg = a.k + b * a.skb + h * DH;
  const E* Vg = a.v + b * a.svb + h * DH;
  const E* Gg = a.dO + b * a.sgb + h * DH;
  const int nqt = (a.Lq + 15) / 16, nkt = (a.Lk + 15) / 16;
  // Latency chain (tests/probes/mha_scaling.py: one workgroup per CU or a tenth of that take the same time): the fragments a wave
  // fetches from global memory - its query rows of Q and dO in phase A, its key rows of K and V in phase B - are requested one
  // step early for a wave's FIRST round: before the staging of the phase's LDS slices (a second buffer for the later rounds costs 16
  // registers: 135 instead of 119 VGPRs, i.e. one workgroup per CU instead of two - not taken).
  E8 fx[2], fy[2];
  auto fetch = [&](const E* X, int64_t ldx, const E* Y, int64_t ldy, int row0, int valid) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      fx[kk] = global_frag<DH>(X, ldx, row0 + fr, valid, kk, fq);
      fy[kk] = global_frag<DH>(Y, ldy, row0 + fr, valid, kk, fq);
    }
  };
  if (wave < nqt) fetch(Qg, a.ldq, Gg, a.ldg, wave * 16, a.Lq);
  fill_rows2<DH, LP, 512>(Ks, Kg, a.ldk, a.Lk, Vs, Vg, a.ldv, a.Lk, tid);  // both slices' loads in flight before the first LDS store
  for (int i = tid; i < LP; i += 512) {
    Ms[i] = i < a.Lk ? (a.mask ? a.mask[(int64_t)b * a.Lk + i] : 0.f) : -INFINITY;
    Ls[i] = i < a.Lq ? a.lse[((int64_t)b * a.H + h) * a.Lq + i] : INFINITY;
    Ds[i] = 0.f;
  }
  __syncthreads();

  // ---- phase A: 16 queries per wave -> D, dQ ----------------------------------------------------------
  for (int qt = wave; qt < nqt; qt += NW) {
    const int q0 = qt * 16;
    if (qt != wave) fetch(Qg, a.ldq, Gg, a.ldg, q0, a.Lq);
    E8 (&qf)[2] = fx, (&gf)[2] = fy;
    const float lse = Ls[q0 + fr];
    const uint64_t rbA = (((uint64_t)b * a.H + h) * a.Lq + min(q0 + fr, a.Lq - 1)) * a.lkp;
    // P^T tile t (rows = keys t*16 + fq*4 + r, col = query fr) and dP^T = V dO^T in the same layout (with dropout: the
    // gradient w.r.t. the UNdropped probability, mask * dO V^T / (1-p)); computed twice (once for D, once for dS)
    // instead of keeping 2 x NT16 accumulator tiles live across the row reduction
    auto tile = [&](int t, f32x4& pv, f32x4& dpv) {
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        sa = H16<E>::mfma32(lds_frag(&Ks[(t * 16 + fr) * LDW + kk * 32 + fq * 8]), qf[kk], sa);
        da = H16<E>::mfma32(lds_frag(&Vs[(t * 16 + fr) * LDW + kk * 32 + fq * 8]), gf[kk], da);
      }
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(&Ms[t * 16 + fq * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) sa[r] = __expf(sa[r] * a.scale + m4[r] - lse);
      if (a.drop_thresh) {
#pragma unroll
        for (int r = 0; r < 4; ++r) da[r] *= drop_mult(a, rbA, t * 16 + fq * 4 + r);
      }
      pv = sa;
      dpv = da;
    };
    float dsum = 0.f;
#pragma unroll 2
    for (int t = 0; t < NT16; ++t) {
      f32x4 pv, dpv;
      tile(t, pv, dpv);
#pragma unroll
      for (int r = 0; r < 4; ++r) dsum += pv[r] * dpv[r];
    }
    dsum = group4_sum(dsum);
    if (fq == 0) Ds[q0 + fr] = dsum;
    f32x4 dq[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int u = 0; u < NK32; ++u) {
      f32x4 p0, p1, d0, d1;
      tile(2 * u, p0, d0);
      tile(2 * u + 1, p1, d1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d0[r] = p0[r] * (d0[r] - dsum) * a.scale;
        d1[r] = p1[r] * (d1[r] - dsum) * a.scale;
      }
      const E8 dsf = pack_frag(d0, d1);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
        dq[dt] = H16<E>::mfma32(lds_frag_tr(Ks, u * 32 + fq * 4, dt * 16, tq, tp), dsf, dq[dt]);
    }
    if (q0 + fr < a.Lq) {
      E* dQg = a.dq + b * a.sdqb + h * DH + (int64_t)(q0 + fr) * a.lddq;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        Pack<E, 4> out;
#pragma unroll
        for (int r = 0; r < 4; ++r) out.v[r] = (E)dq[dt][r];
        st_pack<E, 4>(dQg + dt * 16 + fq * 4, out);
      }
    }
  }
  if (wave < nkt) fetch(Kg, a.ldk, Vg, a.ldv, wave * 16, a.Lk);  // (phase B's first fragments: in flight across the barrier and the staging)
  __syncthreads();  // every wave is done with K and V (and D is complete)
  fill_rows2<DH, LP, 512>(Qs, Qg, a.ldq, a.Lq, Gs, Gg, a.ldg, a.Lq, tid);
  __syncthreads();

  // ---- phase B: 16 keys per wave -> dK, dV --------------------------------------------------------------
  for (int kt = wave; kt < nkt; kt += NW) {
    const int k0 = kt * 16;
    if (kt != wave) fetch(Kg, a.ldk, Vg, a.ldv, k0, a.Lk);
    E8 (&kf)[2] = fx, (&vf)[2] = fy;
    const float mk = Ms[k0 + fr];
    f32x4 dk[NDT], dv[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int u = 0; u < NK32; ++u) {
      f32x4 pt[2], dst[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int r0 = (u * 2 + half) * 16;
        f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          sa = H16<E>::mfma32(lds_frag(&Qs[(r0 + fr) * LDW + kk * 32 + fq * 8]), kf[kk], sa);
          da = H16<E>::mfma32(lds_frag(&Gs[(r0 + fr) * LDW + kk * 32 + fq * 8]), vf[kk], da);
        }
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(&Ls[r0 + fq * 4]);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(&Ds[r0 + fq * 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __expf(sa[r] * a.scale + mk - l4[r]);
          float mlt = 1.f;  // rows = queries r0 + fq*4 + r, column = key k0 + fr
          if (a.drop_thresh)
            mlt = drop_mult(a, (((uint64_t)b * a.H + h) * a.Lq + min(r0 + fq * 4 + r, a.Lq - 1)) * a.lkp, min(k0 + fr, a.Lk - 1));
          pt[half][r] = pv * mlt;                                   // dropped probability: dV = P_d^T dO
          dst[half][r] = pv * (da[r] * mlt - d4[r]) * a.scale;      // dS = P o (mask dP_d / (1-p) - D)
        }
      }
      const E8 pf = pack_frag(pt[0], pt[1]), dsf = pack_frag(dst[0], dst[1]);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        dv[dt] = H16<E>::mfma32(lds_frag_tr(Gs, u * 32 + fq * 4, dt * 16, tq, tp), pf, dv[dt]);
        dk[dt] = H16<E>::mfma32(lds_frag_tr(Qs, u * 32 + fq * 4, dt * 16, tq, tp), dsf, dk[dt]);
      }
    }
    if (k0 + fr < a.Lk) {
      E* dKg = a.dk + b * a.sdkb + h * DH + (int64_t)(k0 + fr) * a.lddk;
      E* dVg = a.dv + b * a.sdvb + h * DH + (int64_t)(k0 + fr) * a.lddv;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        Pack<E, 4> ok, ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ok.v[r] = (E)dk[dt][r];
          ov.v[r] = (E)dv[dt][r];
        }
        st_pack<E, 4>(dKg + dt * 16 + fq * 4, ok);
        st_pack<E, 4>(dVg + dt * 16 + fq * 4, ov);
      }
    }
  }
}

// =====================================================================================================
// Long sequences (257 .. 1024 tokens: BASELINE configs[3] has 577 image tokens, configs[4] 512 text tokens): the head's K / V
// (forward) or Q / K / V / dO (backward) no longer fit in LDS, so the same per-wave arithmetic runs over 128-row BLOCKS with the
// running row maximum / sum of the online softmax (forward) and the row statistics saved by the forward (backward):
//   mha_long_fwd     workgroup = 128 queries of one (b, h) (8 waves x 16), loop over 128-key blocks staged in LDS;
//   mha_long_bwd_dq  same ownership; pass 1 over the key blocks gives D = rowsum(P o dP) (written to `dsum` for the second
//                    kernel), pass 2 gives dS and dQ^T += K^T dS^T;
//   mha_long_bwd_dkv workgroup = 128 keys of one (b, h), loop over 128-query blocks (Q, dO, lse, D staged in LDS):
//                    dV^T += dO^T P, dK^T += Q^T dS.
// Fixed summation order (block after block), no atomics.
// =====================================================================================================
constexpr int LB = 128;  // rows per block

template <int DH>
__global__ __launch_bounds__(512) void mha_long_fwd_kernel(MhaArgs a) {
  constexpr int NKT = LB / 16, NK32 = LB / 32, NDT = DH / 16;
  __shared__ __attribute__((aligned(16))) E Ks[LB * LDW];
  __shared__ __attribute__((aligned(16))) E Vs[LB * LDW];
  __shared__ __attribute__((aligned(16))) float Ms[LB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
  const int qrow = blockIdx.x * LB + wave * 16 + fr;
  const bool qok = qrow < a.Lq;
  const E* Qg = a.q + b * a.sqb + h * DH + (int64_t)qrow * a.ldq;
  E8 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int col = kk * 32 + fq * 8;
    if (qok && col < DH) {
      qf[kk] = *reinterpret_cast<const E8*>(Qg + col);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[kk][j] = (E)0.f;
    }
  }
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.Lk; k0 += LB) {
    __syncthreads();  // the previous block's fragments have been read by every wave
    fill_rows2<DH, LB, 512>(Ks, a.k + b * a.skb + h * DH + (int64_t)k0 * a.ldk, a.ldk, a.Lk - k0,
                            Vs, a.v + b * a.svb + h * DH + (int64_t)k0 * a.ldv, a.ldv, a.Lk - k0, tid);
    for (int key = tid; key < LB; key += 512)
      Ms[key] = k0 + key < a.Lk ? (a.mask ? a.mask[(int64_t)b * a.Lk + k0 + key] : 0.f) : -INFINITY;
    __syncthreads();
    f32x4 s[NKT];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) acc = H16<E>::mfma32(lds_frag(&Ks[(t * 16 + fr) * LDW + kk * 32 + fq * 8]), qf[kk], acc);
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(&Ms[t * 16 + fq * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r] = acc[r] * a.scale + m4[r];
        mx = fmaxf(mx, acc[r]);
      }
      s[t] = acc;
    }
    mx = group4_max(mx);
    const float m_new = fmaxf(m_run, mx);  // finite: every block holds at least one real key, masks are finite
    const float alpha = __expf(m_run - m_new);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = __expf(s[t][r] - m_new);
        sum += s[t][r];
      }
    l_run = l_run * alpha + group4_sum(sum);
    m_run = m_new;
    if (a.drop_thresh) {  // dropout acts on the normalised probabilities: the running sum above stays undropped
      const uint64_t rb = (((uint64_t)b * a.H + h) * a.Lq + (qok ? qrow : 0)) * a.lkp;
#pragma unroll
      for (int t = 0; t < NKT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] *= drop_mult(a, rb, min(k0 + t * 16 + fq * 4 + r, a.Lk - 1));
    }
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
#pragma unroll
    for (int u = 0; u < NK32; ++u) {
      const E8 pf = pack_frag(s[2 * u], s[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) o[dt] = H16<E>::mfma32(lds_frag_tr(Vs, u * 32 + fq * 4, dt * 16, tq, tp), pf, o[dt]);
    }
  }
  if (!qok) return;
  const float inv = 1.f / l_run;
  if (fq == 0) a.lse[((int64_t)b * a.H + h) * a.Lq + qrow] = m_run + logf(l_run);
  E* Og = a.o + b * a.sob + h * DH + (int64_t)qrow * a.ldo;
  const E* Rg = a.res ? a.res + b * a.srb + h * DH + (int64_t)qrow * a.ldr : nullptr;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    const int c = dt * 16 + fq * 4;
    Pack<E, 4> out;
    if (Rg) {
      const Pack<E, 4> rv = ld_pack<E, 4>(Rg + c);
#pragma unroll
      for (int r = 0; r < 4; ++r) out.v[r] = (E)(o[dt][r] * inv + (float)rv.v[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) out.v[r] = (E)(o[dt][r] * inv);
    }
    st_pack<E, 4>(Og + c, out);
  }
}

template <int DH>
__global__ __launch_bounds__(512) void mha_long_bwd_dq_kernel(MhaArgs a) {
  constexpr int NT16 = LB / 16, NK32 = LB / 32, NDT = DH / 16;
  __shared__ __attribute__((aligned(16))) E Ks[LB * LDW];
  __shared__ __attribute__((aligned(16))) E Vs[LB * LDW];
  __shared__ __attribute__((aligned(16))) float Ms[LB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
  const int qrow = blockIdx.x * LB + wave * 16 + fr;
  const bool qok = qrow < a.Lq;
  const E* Qg = a.q + b * a.sqb + h * DH + (int64_t)qrow * a.ldq;
  const E* Gg = a.dO + b * a.sgb + h * DH + (int64_t)qrow * a.ldg;
  E8 qf[2], gf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int col = kk * 32 + fq * 8;
    if (qok && col < DH) {
      qf[kk] = *reinterpret_cast<const E8*>(Qg + col);
      gf[kk] = *reinterpret_cast<const E8*>(Gg + col);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[kk][j] = (E)0.f, gf[kk][j] = (E)0.f;
    }
  }
  const float lse = qok ? a.lse[((int64_t)b * a.H + h) * a.Lq + qrow] : INFINITY;
  const uint64_t rbq = (((uint64_t)b * a.H + h) * a.Lq + (qok ? qrow : 0)) * a.lkp;
  int kbase = 0;  // first key of the staged block
  auto tile = [&](int t, f32x4& pv, f32x4& dpv) {  // P^T and dP^T of key tile t of the staged block, for this wave's 16 queries
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      sa = H16<E>::mfma32(lds_frag(&Ks[(t * 16 + fr) * LDW + kk * 32 + fq * 8]), qf[kk], sa);
      da = H16<E>::mfma32(lds_frag(&Vs[(t * 16 + fr) * LDW + kk * 32 + fq * 8]), gf[kk], da);
    }
    const f32x4 m4 = *reinterpret_cast<const f32x4*>(&Ms[t * 16 + fq * 4]);
#pragma unroll
    for (int r = 0; r < 4; ++r) sa[r] = __expf(sa[r] * a.scale + m4[r] - lse);
    if (a.drop_thresh) {
#pragma unroll
      for (int r = 0; r < 4; ++r) da[r] *= drop_mult(a, rbq, min(kbase + t * 16 + fq * 4 + r, a.Lk - 1));
    }
    pv = sa;
    dpv = da;
  };
  auto stage = [&](int k0) {
    kbase = k0;
    __syncthreads();
    fill_rows2<DH, LB, 512>(Ks, a.k + b * a.skb + h * DH + (int64_t)k0 * a.ldk, a.ldk, a.Lk - k0,
                            Vs, a.v + b * a.svb + h * DH + (int64_t)k0 * a.ldv, a.ldv, a.Lk - k0, tid);
    for (int key = tid; key < LB; key += 512)
      Ms[key] = k0 + key < a.Lk ? (a.mask ? a.mask[(int64_t)b * a.Lk + k0 + key] : 0.f) : -INFINITY;
    __syncthreads();
  };
  float dsum = 0.f;
  for (int k0 = 0; k0 < a.Lk; k0 += LB) {  // pass 1: D = rowsum(P o dP)
    stage(k0);
#pragma unroll 2
    for (int t = 0; t < NT16; ++t) {
      f32x4 pv, dpv;
      tile(t, pv, dpv);
#pragma unroll
      for (int r = 0; r < 4; ++r) dsum += pv[r] * dpv[r];
    }
  }
  dsum = group4_sum(dsum);
  if (fq == 0 && qok) a.dsum[((int64_t)b * a.H + h) * a.Lq + qrow] = dsum;
  f32x4 dq[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.Lk; k0 += LB) {  // pass 2: dS, dQ
    stage(k0);
#pragma unroll 1
    for (int u = 0; u < NK32; ++u) {
      f32x4 p0, p1, d0, d1;
      tile(2 * u, p0, d0);
      tile(2 * u + 1, p1, d1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d0[r] = p0[r] * (d0[r] - dsum) * a.scale;
        d1[r] = p1[r] * (d1[r] - dsum) * a.scale;
      }
      const E8 dsf = pack_frag(d0, d1);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) dq[dt] = H16<E>::mfma32(lds_frag_tr(Ks, u * 32 + fq * 4, dt * 16, tq, tp), dsf, dq[dt]);
    }
  }
  if (!qok) return;
  E* dQg = a.dq + b * a.sdqb + h * DH + (int64_t)qrow * a.lddq;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    Pack<E, 4> out;
#pragma unroll
    for (int r = 0; r < 4; ++r) out.v[r] = (E)dq[dt][r];
    st_pack<E, 4>(dQg + dt * 16 + fq * 4, out);
  }
}

template <int DH>
__global__ __launch_bounds__(512) void mha_long_bwd_dkv_kernel(MhaArgs a) {
  constexpr int NK32 = LB / 32, NDT = DH / 16;
  __shared__ __attribute__((aligned(16))) E Qs[LB * LDW];
  __shared__ __attribute__((aligned(16))) E Gs[LB * LDW];
  __shared__ __attribute__((aligned(16))) float Ls[LB];
  __shared__ __attribute__((aligned(16))) float Ds[LB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
  const int krow = blockIdx.x * LB + wave * 16 + fr;
  const bool kok = krow < a.Lk;
  const E* Kg = a.k + b * a.skb + h * DH + (int64_t)krow * a.ldk;
  const E* Vg = a.v + b * a.svb + h * DH + (int64_t)krow * a.ldv;
  E8 kf[2], vf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int col = kk * 32 + fq * 8;
    if (kok && col < DH) {
      kf[kk] = *reinterpret_cast<const E8*>(Kg + col);
      vf[kk] = *reinterpret_cast<const E8*>(Vg + col);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[kk][j] = (E)0.f, vf[kk][j] = (E)0.f;
    }
  }
  const float mk = kok ? (a.mask ? a.mask[(int64_t)b * a.Lk + krow] : 0.f) : -INFINITY;
  f32x4 dk[NDT], dv[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int q0 = 0; q0 < a.Lq; q0 += LB) {
    __syncthreads();
    fill_rows2<DH, LB, 512>(Qs, a.q + b * a.sqb + h * DH + (int64_t)q0 * a.ldq, a.ldq, a.Lq - q0,
                            Gs, a.dO + b * a.sgb + h * DH + (int64_t)q0 * a.ldg, a.ldg, a.Lq - q0, tid);
    for (int i = tid; i < LB; i += 512) {
      const bool ok = q0 + i < a.Lq;
      Ls[i] = ok ? a.lse[((int64_t)b * a.H + h) * a.Lq + q0 + i] : INFINITY;  // exp(. - inf) = 0: padded queries contribute nothing
      Ds[i] = ok ? a.dsum[((int64_t)b * a.H + h) * a.Lq + q0 + i] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < NK32; ++u) {
      f32x4 pt[2], dst[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int r0 = (u * 2 + half) * 16;
        f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          sa = H16<E>::mfma32(lds_frag(&Qs[(r0 + fr) * LDW + kk * 32 + fq * 8]), kf[kk], sa);
          da = H16<E>::mfma32(lds_frag(&Gs[(r0 + fr) * LDW + kk * 32 + fq * 8]), vf[kk], da);
        }
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(&Ls[r0 + fq * 4]);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(&Ds[r0 + fq * 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __expf(sa[r] * a.scale + mk - l4[r]);
          float mlt = 1.f;
          if (a.drop_thresh)
            mlt = drop_mult(a, (((uint64_t)b * a.H + h) * a.Lq + min(q0 + r0 + fq * 4 + r, a.Lq - 1)) * a.lkp, kok ? krow : 0);
          pt[half][r] = pv * mlt;
          dst[half][r] = pv * (da[r] * mlt - d4[r]) * a.scale;
        }
      }
      const E8 pf = pack_frag(pt[0], pt[1]), dsf = pack_frag(dst[0], dst[1]);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        dv[dt] = H16<E>::mfma32(lds_frag_tr(Gs, u * 32 + fq * 4, dt * 16, tq, tp), pf, dv[dt]);
        dk[dt] = H16<E>::mfma32(lds_frag_tr(Qs, u * 32 + fq * 4, dt * 16, tq, tp), dsf, dk[dt]);
      }
    }
  }
  if (!kok) return;
  E* dKg = a.dk + b * a.sdkb + h * DH + (int64_t)krow * a.lddk;
  E* dVg = a.dv + b * a.sdvb + h * DH + (int64_t)krow * a.lddv;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    Pack<E, 4> ok, ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ok.v[r] = (E)dk[dt][r];
      ov.v[r] = (E)dv[dt][r];
    }
    st_pack<E, 4>(dKg + dt * 16 + fq * 4, ok);
    st_pack<E, 4>(dVg + dt * 16 + fq * 4, ov);
  }
}

bool aligned_slice(const void* p, int64_t ld, int64_t sb, int dh) {
  return p && (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && ld % 8 == 0 && sb % 8 == 0 && (dh * 2) % 16 == 0;
}

template <int DH>
void launch_fwd(const MhaArgs& a, int nk32, hipStream_t st) {
  const dim3 grid(a.B * a.H), block(512);
  switch (nk32) {
#define D2R_CASE(N) case N: hipLaunchKernelGGL((mha_fwd_kernel<DH, N>), grid, block, 0, st, a); break;
    D2R_CASE(1) D2R_CASE(2) D2R_CASE(3) D2R_CASE(4) D2R_CASE(5) D2R_CASE(6) D2R_CASE(7) D2R_CASE(8)
#undef D2R_CASE
  }
  d2r_attn_note(D2R_AV_MHA_FWD + DH * 100 + nk32);
}
template <int DH>
void launch_bwd(const MhaArgs& a, int nk32, hipStream_t st) {
  const dim3 grid(a.B * a.H), block(512);
  switch (nk32) {
#define D2R_CASE(N) case N: hipLaunchKernelGGL((mha_bwd_kernel<DH, N>), grid, block, 0, st, a); break;
    D2R_CASE(1) D2R_CASE(2) D2R_CASE(3) D2R_CASE(4) D2R_CASE(5) D2R_CASE(6) D2R_CASE(7) D2R_CASE(8)
#undef D2R_CASE
  }
  d2r_attn_note(D2R_AV_MHA_BWD + DH * 100 + nk32);
}

}  // namespace

int mha_fwd_run(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                           const void* v, int64_t ldv, int64_t svb, void* o, int64_t ldo, int64_t sob,
                           const void* residual, int64_t ldr, int64_t srb, const float* mask, float* lse, int B, int H,
                           int Lq, int Lk, int head_dim, float scale, float p_drop, uint64_t seed, void* stream) {
  D2R_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "d2r_mha_fwd: dropout probability must be in [0, 1)");
  D2R_REQUIRE(d2r_mha_supported(dtype, Lq, Lk, head_dim), "d2r_mha_fwd: unsupported (16-bit dtype, head_dim 64|48, L <= 1024 only)");
  D2R_REQUIRE(B >= 1 && H >= 1 && lse, "d2r_mha_fwd: bad arguments");
  D2R_REQUIRE(aligned_slice(q, ldq, sqb, head_dim) && aligned_slice(k, ldk, skb, head_dim) && aligned_slice(v, ldv, svb, head_dim) &&
                  aligned_slice(o, ldo, sob, head_dim) && (!residual || aligned_slice(residual, ldr, srb, head_dim)),
              "d2r_mha_fwd: pointers must be 16-byte aligned, strides multiples of 8 elements");
  MhaArgs a = {};
  a.q = (const E*)q, a.k = (const E*)k, a.v = (const E*)v, a.res = (const E*)residual, a.o = (E*)o;
  a.mask = mask, a.lse = lse;
  a.ldq = ldq, a.sqb = sqb, a.ldk = ldk, a.skb = skb, a.ldv = ldv, a.svb = svb, a.ldo = ldo, a.sob = sob, a.ldr = ldr, a.srb = srb;
  a.B = B, a.H = H, a.Lq = Lq, a.Lk = Lk, a.scale = scale;
  a.drop_thresh = p_drop > 0.f ? d2r_drop_threshold(p_drop) : 0u, a.drop_scale = 1.f / (1.f - p_drop), a.drop_seed = seed, a.lkp = (Lk + 7) / 8 * 8;
  if (Lq > 256 || Lk > 256) {  // block loop with the online softmax
    const dim3 grid(d2r_cdiv(Lq, LB), B * H);
    if (head_dim == 64) hipLaunchKernelGGL(mha_long_fwd_kernel<64>, grid, dim3(512), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(mha_long_fwd_kernel<48>, grid, dim3(512), 0, (hipStream_t)stream, a);
    d2r_attn_note(D2R_AV_MHA_LONG_FWD + head_dim * 100);
    return d2r_check_launch("d2r_mha_fwd(long)");
  }
  const int nk32 = d2r_cdiv(Lk, 32);
  if (head_dim == 64) launch_fwd<64>(a, nk32, (hipStream_t)stream);
  else launch_fwd<48>(a, nk32, (hipStream_t)stream);
  return d2r_check_launch("d2r_mha_fwd");
}

int mha_bwd_run(int dtype, const void* q, int64_t ldq, int64_t sqb, const void* k, int64_t ldk, int64_t skb,
                           const void* v, int64_t ldv, int64_t svb, const void* dO, int64_t ldg, int64_t sgb,
                           const float* mask, const float* lse, float* dsum, void* dq, int64_t lddq, int64_t sdqb, void* dk,
                           int64_t lddk, int64_t sdkb, void* dv, int64_t lddv, int64_t sdvb, int B, int H, int Lq, int Lk,
                           int head_dim, float scale, float p_drop, uint64_t seed, void* stream) {
  D2R_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "d2r_mha_bwd: dropout probability must be in [0, 1)");
  D2R_REQUIRE(d2r_mha_supported(dtype, Lq, Lk, head_dim), "d2r_mha_bwd: unsupported (16-bit dtype, head_dim 64|48, L <= 1024 only)");
  D2R_REQUIRE((Lq <= 256 && Lk <= 256) || dsum, "d2r_mha_bwd: sequences above 256 tokens need the dsum scratch ([B, H, Lq] fp32)");
  D2R_REQUIRE(B >= 1 && H >= 1 && lse, "d2r_mha_bwd: bad arguments");
  D2R_REQUIRE(aligned_slice(q, ldq, sqb, head_dim) && aligned_slice(k, ldk, skb, head_dim) && aligned_slice(v, ldv, svb, head_dim) &&
                  aligned_slice(dO, ldg, sgb, head_dim) && aligned_slice(dq, lddq, sdqb, head_dim) &&
                  aligned_slice(dk, lddk, sdkb, head_dim) && aligned_slice(dv, lddv, sdvb, head_dim),
              "d2r_mha_bwd: pointers must be 16-byte aligned, strides multiples of 8 elements");
  MhaArgs a = {};
  a.q = (const E*)q, a.k = (const E*)k, a.v = (const E*)v, a.dO = (const E*)dO;
  a.dq = (E*)dq, a.dk = (E*)dk, a.dv = (E*)dv;
  a.mask = mask, a.lse = const_cast<float*>(lse);
  a.ldq = ldq, a.sqb = sqb, a.ldk = ldk, a.skb = skb, a.ldv = ldv, a.svb = svb, a.ldg = ldg, a.sgb = sgb;
  a.lddq = lddq, a.sdqb = sdqb, a.lddk = lddk, a.sdkb = sdkb, a.lddv = lddv, a.sdvb = sdvb;
  a.B = B, a.H = H, a.Lq = Lq, a.Lk = Lk, a.scale = scale;
  a.dsum = dsum;
  a.drop_thresh = p_drop > 0.f ? d2r_drop_threshold(p_drop) : 0u, a.drop_scale = 1.f / (1.f - p_drop), a.drop_seed = seed, a.lkp = (Lk + 7) / 8 * 8;
  if (Lq > 256 || Lk > 256) {
    const dim3 gq(d2r_cdiv(Lq, LB), B * H), gk(d2r_cdiv(Lk, LB), B * H);
    if (head_dim == 64) {
      hipLaunchKernelGGL(mha_long_bwd_dq_kernel<64>, gq, dim3(512), 0, (hipStream_t)stream, a);
      hipLaunchKernelGGL(mha_long_bwd_dkv_kernel<64>, gk, dim3(512), 0, (hipStream_t)stream, a);
    } else {
      hipLaunchKernelGGL(mha_long_bwd_dq_kernel<48>, gq, dim3(512), 0, (hipStream_t)stream, a);
      hipLaunchKernelGGL(mha_long_bwd_dkv_kernel<48>, gk, dim3(512), 0, (hipStream_t)stream, a);
    }
    d2r_attn_note(D2R_AV_MHA_LONG_DQ + head_dim * 100);
    d2r_attn_note(D2R_AV_MHA_LONG_DKV + head_dim * 100);
    return d2r_check_launch("d2r_mha_bwd(long)");
  }
  const int nk32 = d2r_cdiv(Lq > Lk ? Lq : Lk, 32);
  if (head_dim == 64) launch_bwd<64>(a, nk32, (hipStream_t)stream);
  else launch_bwd<48>(a, nk32, (hipStream_t)stream);
  return d2r_check_launch("d2r_mha_bwd");
}

namespace {

constexpr int XB_MAXCORE = 4;  // attention problems ("cores") of one backward launch: same shapes and strides, own tensors
struct XbwdArgs {
  const E *q[XB_MAXCORE], *k[XB_MAXCORE], *v[XB_MAXCORE], *dO[XB_MAXCORE];
  E *dq[XB_MAXCORE], *p_out[XB_MAXCORE], *ds_out[XB_MAXCORE];
  const float* lse[XB_MAXCORE];
  const float* mask;
  int64_t ldq, sqb, ldk, skb, ldv, svb, ldg, sgb, lddq, sdqb;
  int B, Lq, Lk, lkp, ncore, ntile;
  float scale;
};
template <typename P>
__device__ __forceinline__ P xb_pick(P const (&arr)[XB_MAXCORE], int core) {  // wave-uniform select chain (no scratch)
  P r = arr[0];
#pragma unroll
  for (int c = 1; c < XB_MAXCORE; ++c) r = core == c ? arr[c] : r;
  return r;
}

constexpr int XD = 768, XQ = 32, XW = 8, XCOLS = XD / XW;  // 96 output columns per wave
constexpr int LDQ = XD + 8;                                  // Qs row stride (bf16)
constexpr int LDV = XCOLS + 8;                               // V slab row stride (bf16)

// S^T / dP^T style product for this wave's (up to NTI: tiles wave, wave + 8, ...) key tiles and both query tiles:
// acc[ti][qt] += sum_d X[key, d] * Y[q, d], X rows from global (clamped), Y rows from LDS
template <int NTI>
__device__ __forceinline__ void xattn_scores(const E* __restrict__ Xg, int64_t ldx, int Lk, const E* Ys, int wave,
                                             int nt16, int fr, int fq, f32x4 (&acc)[NTI][2]) {
  const E* xrow[NTI];
  bool act[NTI];
#pragma unroll
  for (int ti = 0; ti < NTI; ++ti) {
    const int t = wave + ti * XW;
    act[ti] = t < nt16 && t * 16 < Lk;
    const int key = min(t * 16 + fr, Lk - 1);
    xrow[ti] = Xg + (int64_t)key * ldx + fq * 8;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) acc[ti][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (!act[0]) return;  // tiles are assigned in order: no first tile, no second
  // The X rows come straight from global memory (L2), one 16-byte fragment per lane, tile and k-step: the loop is a latency
  // chain unless many of them are in flight.  CH k-steps of every tile are loaded as one batch, the next batch is issued
  // before the current one is multiplied (two register sets).  Tiles past the last key read the clamped last row and are
  // never used: no branch around a load (a branch puts a full memory wait after every load).
  constexpr int CH = NTI <= 2 ? 8 : 2, NCH = XD / 32 / CH;
  E8 xb[2][NTI][CH];
  auto fetch = [&](int c, E8 (&dst)[NTI][CH]) {
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
      for (int k = 0; k < CH; ++k) dst[ti][k] = *reinterpret_cast<const E8*>(xrow[ti] + (c * CH + k) * 32);
  };
  fetch(0, xb[0]);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c + 1 < NCH) fetch(c + 1, xb[(c + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);  // the batch is issued HERE (the scheduler otherwise sinks each load next to its use)
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int kk = c * CH + k;
      const E8 y0 = lds_frag(Ys + fr * LDQ + kk * 32 + fq * 8);
      const E8 y1 = lds_frag(Ys + (16 + fr) * LDQ + kk * 32 + fq * 8);
#pragma unroll
      for (int ti = 0; ti < NTI; ++ti) {
        acc[ti][0] = H16<E>::mfma32(xb[c & 1][ti][k], y0, acc[ti][0]);
        acc[ti][1] = H16<E>::mfma32(xb[c & 1][ti][k], y1, acc[ti][1]);
      }
    }
  }
}

// out^T[d, q] = sum_key M[key, d] * W[q, key] for this wave's 96 columns d and both query tiles; M rows stream from
// global through the wave's private LDS slab, W (16-bit [32][LDW_P]) is read from LDS.  acc[dt][qt].
template <int LDW_P>
__device__ __forceinline__ void xattn_apply(const E* __restrict__ Mg, int64_t ldm, int Lk, int nk32, const E* Ws,
                                            E* slab, int wave, int lane, f32x4 (&acc)[6][2]) {
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
#pragma unroll
  for (int dt = 0; dt < 6; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) acc[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // 32 rows x 96 columns = 384 16-byte chunks per step: 6 per lane; two register sets keep the loads of steps
  // u+1 and u+2 in flight while step u is multiplied (the loop is latency-bound, not bandwidth-bound)
  Pack<E, 8> stage[2][6];
  auto load = [&](int u, Pack<E, 8> (&st)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int c = lane + i * 64, row = c / 12, ch = c % 12;
      const int key = min(u * 32 + row, Lk - 1);  // clamped: the matching probabilities are exactly zero
      st[i] = ld_pack<E, 8>(Mg + (int64_t)key * ldm + wave * XCOLS + ch * 8);
    }
  };
  auto store = [&](E* dst, const Pack<E, 8> (&st)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int c = lane + i * 64, row = c / 12, ch = c % 12;
      st_pack<E, 8>(dst + row * LDV + ch * 8, st[i]);
    }
  };
  load(0, stage[0]);
  if (nk32 > 1) load(1, stage[1]);
#pragma unroll 2
  for (int u = 0; u < nk32; ++u) {
    E* cur = slab + (u & 1) * 32 * LDV;
    if (u & 1) {
      store(cur, stage[1]);
      if (u + 2 < nk32) load(u + 2, stage[1]);
    } else {
      store(cur, stage[0]);
      if (u + 2 < nk32) load(u + 2, stage[0]);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's slab stores have landed (wave-private region)
    __builtin_amdgcn_wave_barrier();
    const E8 w0 = lds_frag(Ws + fr * LDW_P + u * 32 + fq * 8);
    const E8 w1 = lds_frag(Ws + (16 + fr) * LDW_P + u * 32 + fq * 8);
#pragma unroll
    for (int dt = 0; dt < 6; ++dt) {
      const E* p0 = cur + (fq * 8 + tq) * LDV + dt * 16 + tp * 4;
      const E4 lo = H16<E>::tr_read(p0);
      const E4 hi = H16<E>::tr_read(p0 + 4 * LDV);
      const E8 m = E8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      acc[dt][0] = H16<E>::mfma32(m, w0, acc[dt][0]);
      acc[dt][1] = H16<E>::mfma32(m, w1, acc[dt][1]);
    }
  }
}

// 32 rows x 768 columns (rows clamped past `valid`) from global to LDS [32][LDQ]; all loads issued before the stores
__device__ __forceinline__ void xattn_stage_rows(E* dst, const E* __restrict__ src, int64_t ld, int row0, int valid, int tid) {
  Pack<E, 8> v[6];
#pragma unroll
  for (int it = 0; it < 6; ++it) {
    const int c = tid + it * 512, row = c / (XD / 8), ch = c % (XD / 8);
    v[it] = ld_pack<E, 8>(src + (int64_t)min(row0 + row, valid - 1) * ld + ch * 8);
  }
#pragma unroll
  for (int it = 0; it < 6; ++it) {
    const int c = tid + it * 512, row = c / (XD / 8), ch = c % (XD / 8);
    st_pack<E, 8>(dst + row * LDQ + ch * 8, v[it]);
  }
}

// Backward, first half: dS and P for 32 query rows (both to HBM as bf16 [B, Lq, lkp] for the two key-side products
// dK = dS^T Q and dV = P^T dO, which are plain batched GEMMs), and dQ = dS K in the same launch.
template <int NTI>  // key tiles per wave: 2 -> Lk <= 256, 5 -> Lk <= 640 (BASELINE configs[3]: 577 image tokens, configs[4]: 512 text tokens)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void xattn_bwd_kernel(XbwdArgs a) {
  constexpr int LKM = NTI * XW * 16, LDPK = LKM + 8;
  constexpr int SLAB = 2 * 32 * LDV;
  constexpr int REGION = (2 * XQ * LDQ > XW * SLAB) ? 2 * XQ * LDQ : XW * SLAB;
  __shared__ __attribute__((aligned(16))) E region[REGION];
  __shared__ __attribute__((aligned(16))) E DSs[XQ * LDPK];
  __shared__ __attribute__((aligned(16))) float Ms[LKM];
  __shared__ float red[XW][XQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  // all query tiles of a (core, sample) on one XCD (blocks b and b + 8 share one): the sample's K and V are then fetched into ONE
  // L2 (in plain order the 4 / 7 tiles of a sample spread over the XCDs and each pulled K and V past its own L2: 4x the bytes)
  const int id = blockIdx.x, xcd = id & 7, rr = id >> 3;
  const int tile = rr % a.ntile, unit = rr / a.ntile;
  const int core = unit % a.ncore, b = (unit / a.ncore) * 8 + xcd;
  if (b >= a.B) return;
  const int q0 = tile * XQ;
  const E* Kg = xb_pick(a.k, core) + b * a.skb;
  const E* Vg = xb_pick(a.v, core) + b * a.svb;
  const float* Lg = xb_pick(a.lse, core) + (int64_t)b * a.Lq;
  E* Pout = xb_pick(a.p_out, core);
  E* DSout = xb_pick(a.ds_out, core);
  const int nk32 = (a.Lk + 31) / 32, nt16 = nk32 * 2;
  E *Qs = region, *Gs = region + XQ * LDQ;
  {
    xattn_stage_rows(Qs, xb_pick(a.q, core) + b * a.sqb, a.ldq, q0, a.Lq, tid);
    xattn_stage_rows(Gs, xb_pick(a.dO, core) + b * a.sgb, a.ldg, q0, a.Lq, tid);
    for (int key = tid; key < LKM; key += 512)
      Ms[key] = key < a.Lk ? (a.mask ? a.mask[(int64_t)b * a.Lk + key] : 0.f) : -INFINITY;
  }
  __syncthreads();
  f32x4 s[NTI][2], dp[NTI][2];
  xattn_scores<NTI>(Kg, a.ldk, a.Lk, Qs, wave, nt16, fr, fq, s);
  xattn_scores<NTI>(Vg, a.ldv, a.Lk, Gs, wave, nt16, fr, fq, dp);
  float lse[2], dsum[2] = {0.f, 0.f};
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qrow = q0 + qt * 16 + fr;
    lse[qt] = qrow < a.Lq ? Lg[qrow] : INFINITY;  // padded query rows: p = 0
  }
#pragma unroll
  for (int ti = 0; ti < NTI; ++ti) {
    const int t = wave + ti * XW;
    if (t >= nt16) continue;
    const f32x4 m4 = *reinterpret_cast<const f32x4*>(&Ms[t * 16 + fq * 4]);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[ti][qt][r] = __expf(s[ti][qt][r] * a.scale + m4[r] - lse[qt]);
        dsum[qt] += s[ti][qt][r] * dp[ti][qt][r];
      }
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    dsum[qt] = group4_sum(dsum[qt]);
    if (fq == 0) red[wave][qt * 16 + fr] = dsum[qt];
  }
  __syncthreads();
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float t = red[0][qt * 16 + fr];
#pragma unroll
    for (int w = 1; w < XW; ++w) t += red[w][qt * 16 + fr];
    dsum[qt] = t;
  }
#pragma unroll
  for (int ti = 0; ti < NTI; ++ti) {
    const int t = wave + ti * XW;
    if (t >= nt16) continue;
    const int col = t * 16 + fq * 4;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      Pack<E, 4> pk, dk;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pk.v[r] = (E)s[ti][qt][r];
        dk.v[r] = (E)(s[ti][qt][r] * (dp[ti][qt][r] - dsum[qt]) * a.scale);
      }
      st_pack<E, 4>(DSs + (qt * 16 + fr) * LDPK + col, dk);
      const int qrow = q0 + qt * 16 + fr;
      if (qrow < a.Lq && col < a.lkp) {
        const int64_t off = ((int64_t)b * a.Lq + qrow) * a.lkp + col;
        st_pack<E, 4>(Pout + off, pk);
        st_pack<E, 4>(DSout + off, dk);
      }
    }
  }
  __syncthreads();  // DSs complete; Qs / Gs are dead: the region now holds the K slabs
  f32x4 dq[6][2];
  xattn_apply<LDPK>(Kg, a.ldk, a.Lk, nk32, DSs, region + wave * SLAB, wave, lane, dq);
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qrow = q0 + qt * 16 + fr;
    if (qrow >= a.Lq) continue;
    E* Dg = xb_pick(a.dq, core) + b * a.sdqb + (int64_t)qrow * a.lddq + wave * XCOLS;
#pragma unroll
    for (int dt = 0; dt < 6; ++dt) {
      Pack<E, 4> out;
#pragma unroll
      for (int r = 0; r < 4; ++r) out.v[r] = (E)dq[dt][qt][r];
      st_pack<E, 4>(Dg + dt * 16 + fq * 4, out);
    }
  }
}

}  // namespace

int xattn_fwd_run(int dtype, int ncore, const void* const* q, int64_t ldq, int64_t sqb, const void* const* k, int64_t ldk, int64_t skb,
                  const void* const* v, int64_t ldv, int64_t svb, void* const* o, int64_t ldo, int64_t sob, const void* const* residual,
                  int64_t ldr, int64_t srb, const float* mask, float* const* lse, int B, int Lq, int Lk, int D, float scale, void* stream) {
  D2R_REQUIRE(d2r_xattn_supported(dtype, Lq, Lk, D), "d2r_xattn_fwd: unsupported (16-bit dtype, D = 768, Lk <= 640 only)");
  D2R_REQUIRE(B >= 1 && ncore >= 1 && ncore <= 4 && q && k && v && o && lse, "d2r_xattn_fwd: bad arguments (1..4 problems per launch)");
  for (int c = 0; c < ncore; ++c)
    D2R_REQUIRE(lse[c] && aligned_slice(q[c], ldq, sqb, 768) && aligned_slice(k[c], ldk, skb, 768) && aligned_slice(v[c], ldv, svb, 768) &&
                    aligned_slice(o[c], ldo, sob, 768) && (!residual || !residual[c] || aligned_slice(residual[c], ldr, srb, 768)),
                "d2r_xattn_fwd: pointers must be non-null and 16-byte aligned, strides multiples of 8 elements");
  if (d2r_xattn2_fwd_try(dtype, ncore, q, ldq, sqb, k, ldk, skb, v, ldv, svb, o, ldo, sob, residual, ldr, srb, mask, lse, B, Lq, Lk,
                                   scale, (hipStream_t)stream))
    return d2r_check_launch("d2r_xattn_fwd(v2)");
  // (d2r_xattn2_fwd_try takes every shape the checks above let through: Lk <= 640, 1..4 problems)
  return d2r_fail(D2R_ERR_INVALID, "d2r_xattn_fwd: no kernel for the shape");
}

// `ncore` (1..4) backward problems of identical shape and strides in one launch: dS, P (16-bit [B, Lq, lkp] each) and dQ.
int xattn_bwd_run(int dtype, int ncore, const void* const* q, int64_t ldq, int64_t sqb, const void* const* k, int64_t ldk, int64_t skb,
                  const void* const* v, int64_t ldv, int64_t svb, const void* const* dO, int64_t ldg, int64_t sgb, const float* mask,
                  const float* const* lse, void* const* dq, int64_t lddq, int64_t sdqb, void* const* P, void* const* dS, int lkp, int B,
                  int Lq, int Lk, int D, float scale, void* stream) {
  D2R_REQUIRE(d2r_xattn_supported(dtype, Lq, Lk, D), "d2r_xattn_bwd: unsupported (16-bit dtype, D = 768, Lk <= 640 only)");
  D2R_REQUIRE(ncore >= 1 && ncore <= XB_MAXCORE && q && k && v && dO && lse && dq && P && dS, "d2r_xattn_bwd: 1..4 problems per launch, no null pointer array");
  D2R_REQUIRE(B >= 1 && lkp >= Lk && lkp % 8 == 0 && lkp <= 640, "d2r_xattn_bwd: bad arguments (lkp: Lk padded to a multiple of 8)");
  XbwdArgs a = {};
  for (int c = 0; c < ncore; ++c) {
    D2R_REQUIRE(lse[c] && aligned_slice(q[c], ldq, sqb, 768) && aligned_slice(k[c], ldk, skb, 768) && aligned_slice(v[c], ldv, svb, 768) &&
                    aligned_slice(dO[c], ldg, sgb, 768) && aligned_slice(dq[c], lddq, sdqb, 768) && P[c] && dS[c] && d2r_aligned16(P[c]) &&
                    d2r_aligned16(dS[c]),
                "d2r_xattn_bwd: pointers must be non-null and 16-byte aligned, strides multiples of 8 elements");
    a.q[c] = (const E*)q[c], a.k[c] = (const E*)k[c], a.v[c] = (const E*)v[c], a.dO[c] = (const E*)dO[c], a.dq[c] = (E*)dq[c];
    a.p_out[c] = (E*)P[c], a.ds_out[c] = (E*)dS[c], a.lse[c] = lse[c];
  }
  a.lkp = lkp, a.mask = mask, a.ncore = ncore, a.ntile = d2r_cdiv(Lq, XQ);
  a.ldq = ldq, a.sqb = sqb, a.ldk = ldk, a.skb = skb, a.ldv = ldv, a.svb = svb, a.ldg = ldg, a.sgb = sgb, a.lddq = lddq, a.sdqb = sdqb;
  a.B = B, a.Lq = Lq, a.Lk = Lk, a.scale = scale;
  const dim3 grid((B + 7) / 8 * 8 * a.ntile * ncore);
  if (Lk <= 256) hipLaunchKernelGGL(xattn_bwd_kernel<2>, grid, dim3(512), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(xattn_bwd_kernel<5>, grid, dim3(512), 0, (hipStream_t)stream, a);
  d2r_attn_note(Lk <= 256 ? D2R_AV_XBWD_2 : D2R_AV_XBWD_5);
  return d2r_check_launch("d2r_xattn_bwd");
}
