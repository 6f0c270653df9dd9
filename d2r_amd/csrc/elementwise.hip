// elementwise.hip — 16-byte vectorised elementwise kernels (activation fwd/bwd, squared difference, FiLM
// mul-add, gate lerp, axpby, casts, AdamW).  Grid-stride over 16-B packs with a scalar tail; when a pointer is
// not 16-B aligned the scalar path is used for everything.
#include <stdlib.h>
#include "common.h"

template <int NIN, int NOUT>
struct EwPtrs {
  const void* in[NIN > 0 ? NIN : 1];
  void* out[NOUT];
};

// F::apply(const float (&in)[NIN], float (&out)[NOUT])
template <typename T, int NIN, int NOUT, typename F>
__global__ __launch_bounds__(256) void ew_kernel(EwPtrs<NIN, NOUT> p, int64_t n, int vec_ok, F f) {
  constexpr int VEC = PackOf<T>::N;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t npk = vec_ok ? n / VEC : 0;
  for (int64_t k = tid; k < npk; k += nthreads) {
    Pack<T, VEC> pin[NIN > 0 ? NIN : 1], pout[NOUT];
#pragma unroll
    for (int a = 0; a < NIN; ++a) pin[a] = ld_pack<T, VEC>(reinterpret_cast<const T*>(p.in[a]) + k * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float x[NIN > 0 ? NIN : 1], y[NOUT];
#pragma unroll
      for (int a = 0; a < NIN; ++a) x[a] = to_f<T>(pin[a].v[j]);
      f.apply(x, y);
#pragma unroll
      for (int o = 0; o < NOUT; ++o) pout[o].v[j] = from_f<T>(y[o]);
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) st_pack<T, VEC>(reinterpret_cast<T*>(p.out[o]) + k * VEC, pout[o]);
  }
  for (int64_t e = npk * VEC + tid; e < n; e += nthreads) {
    float x[NIN > 0 ? NIN : 1], y[NOUT];
#pragma unroll
    for (int a = 0; a < NIN; ++a) x[a] = to_f<T>(reinterpret_cast<const T*>(p.in[a])[e]);
    f.apply(x, y);
#pragma unroll
    for (int o = 0; o < NOUT; ++o) reinterpret_cast<T*>(p.out[o])[e] = from_f<T>(y[o]);
  }
}

template <int NIN, int NOUT, typename F>
static int ew_launch(const char* name, int dtype, const EwPtrs<NIN, NOUT>& p, int64_t n, F f, void* stream) {
  if (n < 0) return d2r_fail(D2R_ERR_INVALID, "%s: negative size", name);
  if (n == 0) return D2R_OK;
  int vec_ok = 1;
  for (int a = 0; a < NIN; ++a) {
    if (!p.in[a]) return d2r_fail(D2R_ERR_INVALID, "%s: null input %d", name, a);
    vec_ok &= d2r_aligned16(p.in[a]);
  }
  for (int o = 0; o < NOUT; ++o) {
    if (!p.out[o]) return d2r_fail(D2R_ERR_INVALID, "%s: null output %d", name, o);
    vec_ok &= d2r_aligned16(p.out[o]);
  }
  const int64_t work = n / (dtype != D2R_F32 ? 8 : 4) + 1;
  int blocks = (int)((work + 255) / 256);
  if (blocks > 2048) blocks = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
  hipStream_t st = (hipStream_t)stream;
  if (dtype == D2R_BF16) hipLaunchKernelGGL((ew_kernel<bf16_t, NIN, NOUT, F>), dim3(blocks), dim3(256), 0, st, p, n, vec_ok, f);
  else if (dtype == D2R_F16) hipLaunchKernelGGL((ew_kernel<f16_t, NIN, NOUT, F>), dim3(blocks), dim3(256), 0, st, p, n, vec_ok, f);
  else if (dtype == D2R_F32) hipLaunchKernelGGL((ew_kernel<float, NIN, NOUT, F>), dim3(blocks), dim3(256), 0, st, p, n, vec_ok, f);
  else return d2r_fail(D2R_ERR_INVALID, "%s: bad dtype %d", name, dtype);
  return d2r_check_launch(name);
}

// ---- functors -----------------------------------------------------------------------------------------
struct ActFwdF {
  int act;
  __device__ void apply(const float (&x)[1], float (&y)[1]) const { y[0] = act_apply(act, x[0]); }
};
struct ActBwdF {  // in: dY, ref
  int act;
  __device__ void apply(const float (&x)[2], float (&y)[1]) const { y[0] = x[0] * act_grad(act, x[1]); }
};
struct SqDiffFwdF {
  __device__ void apply(const float (&x)[2], float (&y)[1]) const {
    const float d = x[0] - x[1];
    y[0] = d * d;
  }
};
struct SqDiffBwdF {  // in: a, b, dout -> da, db
  __device__ void apply(const float (&x)[3], float (&y)[2]) const {
    const float g = 2.f * (x[0] - x[1]) * x[2];
    y[0] = g;
    y[1] = -g;
  }
};
struct MulAddFwdF {  // a, s, h -> a*s + h
  __device__ void apply(const float (&x)[3], float (&y)[1]) const { y[0] = x[0] * x[1] + x[2]; }
};
struct MulAddBwdF {  // a, s, dout -> da, ds
  __device__ void apply(const float (&x)[3], float (&y)[2]) const {
    y[0] = x[2] * x[1];
    y[1] = x[2] * x[0];
  }
};
struct LerpFwdF {  // g, a, b -> g*a + (1-g)*b
  __device__ void apply(const float (&x)[3], float (&y)[1]) const { y[0] = x[0] * x[1] + (1.f - x[0]) * x[2]; }
};
struct LerpBwdF {  // g, a, b, dout -> dg, da, db
  __device__ void apply(const float (&x)[4], float (&y)[3]) const {
    y[0] = x[3] * (x[1] - x[2]);
    y[1] = x[3] * x[0];
    y[2] = x[3] * (1.f - x[0]);
  }
};
struct AddF {
  __device__ void apply(const float (&x)[2], float (&y)[1]) const { y[0] = x[0] + x[1]; }
};
struct AxpbyF {  // x, y_old -> alpha*x + beta*y_old
  float alpha, beta;
  __device__ void apply(const float (&x)[2], float (&y)[1]) const { y[0] = alpha * x[0] + (beta != 0.f ? beta * x[1] : 0.f); }
};

extern "C" int d2r_act_fwd(int dtype, int act, const void* X, void* Y, int64_t n, void* stream) {
  EwPtrs<1, 1> p{{X}, {Y}};
  return ew_launch("d2r_act_fwd", dtype, p, n, ActFwdF{act}, stream);
}
extern "C" int d2r_act_bwd(int dtype, int act, const void* dY, const void* ref, void* dX, int64_t n, void* stream) {
  EwPtrs<2, 1> p{{dY, ref}, {dX}};
  return ew_launch("d2r_act_bwd", dtype, p, n, ActBwdF{act}, stream);
}
extern "C" int d2r_sqdiff_fwd(int dtype, const void* a, const void* b, void* out, int64_t n, void* stream) {
  EwPtrs<2, 1> p{{a, b}, {out}};
  return ew_launch("d2r_sqdiff_fwd", dtype, p, n, SqDiffFwdF{}, stream);
}
extern "C" int d2r_sqdiff_bwd(int dtype, const void* a, const void* b, const void* dout, void* da, void* db,
                              int64_t n, void* stream) {
  EwPtrs<3, 2> p{{a, b, dout}, {da, db}};
  return ew_launch("d2r_sqdiff_bwd", dtype, p, n, SqDiffBwdF{}, stream);
}
extern "C" int d2r_muladd_fwd(int dtype, const void* a, const void* s, const void* h, void* out, int64_t n,
                              void* stream) {
  EwPtrs<3, 1> p{{a, s, h}, {out}};
  return ew_launch("d2r_muladd_fwd", dtype, p, n, MulAddFwdF{}, stream);
}
extern "C" int d2r_muladd_bwd(int dtype, const void* a, const void* s, const void* dout, void* da, void* ds,
                              int64_t n, void* stream) {
  EwPtrs<3, 2> p{{a, s, dout}, {da, ds}};
  return ew_launch("d2r_muladd_bwd", dtype, p, n, MulAddBwdF{}, stream);
}
extern "C" int d2r_lerp_fwd(int dtype, const void* g, const void* a, const void* b, void* out, int64_t n,
                            void* stream) {
  EwPtrs<3, 1> p{{g, a, b}, {out}};
  return ew_launch("d2r_lerp_fwd", dtype, p, n, LerpFwdF{}, stream);
}
extern "C" int d2r_lerp_bwd(int dtype, const void* g, const void* a, const void* b, const void* dout, void* dg,
                            void* da, void* db, int64_t n, void* stream) {
  EwPtrs<4, 3> p{{g, a, b, dout}, {dg, da, db}};
  return ew_launch("d2r_lerp_bwd", dtype, p, n, LerpBwdF{}, stream);
}
extern "C" int d2r_axpby(int dtype, float alpha, const void* x, float beta, void* y, int64_t n, void* stream) {
  EwPtrs<2, 1> p{{x, y}, {y}};
  return ew_launch("d2r_axpby", dtype, p, n, AxpbyF{alpha, beta}, stream);
}

// Two independent problems of one size in one launch (the per-sample chains of the routing cells come in text / image or a / b pairs of
// 32 x 768 elements: a launch each is 4-5 us of latency for microseconds of nothing): element for element the same arithmetic as two calls.
struct ActBwd2F {  // in: dY1, ref1, dY2, ref2
  int act;
  __device__ void apply(const float (&x)[4], float (&y)[2]) const {
    y[0] = x[0] * act_grad(act, x[1]);
    y[1] = x[2] * act_grad(act, x[3]);
  }
};
struct Add2F {  // in: a1, b1, a2, b2
  __device__ void apply(const float (&x)[4], float (&y)[2]) const {
    y[0] = x[0] + x[1];
    y[1] = x[2] + x[3];
  }
};
extern "C" int d2r_act_bwd2(int dtype, int act, const void* dY1, const void* ref1, void* dX1, const void* dY2, const void* ref2, void* dX2,
                            int64_t n, void* stream) {
  EwPtrs<4, 2> p{{dY1, ref1, dY2, ref2}, {dX1, dX2}};
  return ew_launch("d2r_act_bwd2", dtype, p, n, ActBwd2F{act}, stream);
}
extern "C" int d2r_add2(int dtype, const void* a1, const void* b1, void* out1, const void* a2, const void* b2, void* out2, int64_t n,
                        void* stream) {
  EwPtrs<4, 2> p{{a1, b1, a2, b2}, {out1, out2}};
  return ew_launch("d2r_add2", dtype, p, n, Add2F{}, stream);
}
extern "C" int d2r_add(int dtype, const void* a, const void* b, void* out, int64_t n, void* stream) {
  EwPtrs<2, 1> p{{a, b}, {out}};
  return ew_launch("d2r_add", dtype, p, n, AddF{}, stream);
}

// ---- dropout ------------------------------------------------------------------------------------------------
// nn.Dropout of the BERT path (models/modeling_unimo.py:330,388,413,468): y = keep(i) ? x / (1 - p) : 0 (+ add).
// keep(i) comes from a counter-based generator (splitmix64 finaliser of seed and element index), so the backward
// pass regenerates the mask from (seed, index) instead of storing it: dx = d2r_dropout(dy) with the same seed.
template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, const T* __restrict__ add, T* __restrict__ y,
                                                      int64_t n, uint32_t thresh, float scale, uint64_t seed, int vec_ok) {
  constexpr int VEC = PackOf<T>::N;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t npk = vec_ok ? n / VEC : 0;
  for (int64_t k = tid; k < npk; k += nthreads) {
    const Pack<T, VEC> px = ld_pack<T, VEC>(x + k * VEC);
    Pack<T, VEC> pa, po;
    if (add) pa = ld_pack<T, VEC>(add + k * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float v = d2r_rand24(seed, (uint64_t)(k * VEC + j)) >= thresh ? to_f<T>(px.v[j]) * scale : 0.f;
      if (add) v += to_f<T>(pa.v[j]);
      po.v[j] = from_f<T>(v);
    }
    st_pack<T, VEC>(y + k * VEC, po);
  }
  for (int64_t e = npk * VEC + tid; e < n; e += nthreads) {
    float v = d2r_rand24(seed, (uint64_t)e) >= thresh ? to_f<T>(x[e]) * scale : 0.f;
    if (add) v += to_f<T>(add[e]);
    y[e] = from_f<T>(v);
  }
}

extern "C" int d2r_dropout(int dtype, const void* x, const void* add, void* y, int64_t n, float p, uint64_t seed,
                           void* stream) {
  D2R_REQUIRE(x && y && n >= 0 && p >= 0.f && p < 1.f, "d2r_dropout: bad arguments (0 <= p < 1)");
  if (n == 0) return D2R_OK;
  const uint32_t thresh = d2r_drop_threshold(p);  // drop when the 24-bit uniform is below p * 2^24
  const float scale = 1.f / (1.f - p);
  const int vec_ok = d2r_aligned16(x) && d2r_aligned16(y) && d2r_aligned16(add);
  const int64_t work = n / (dtype != D2R_F32 ? 8 : 4) + 1;
  int blocks = (int)((work + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == D2R_BF16) hipLaunchKernelGGL((dropout_kernel<bf16_t>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)add, (bf16_t*)y, n, thresh, scale, seed, vec_ok);
  else if (dtype == D2R_F16) hipLaunchKernelGGL((dropout_kernel<f16_t>), dim3(blocks), dim3(256), 0, st, (const f16_t*)x, (const f16_t*)add, (f16_t*)y, n, thresh, scale, seed, vec_ok);
  else if (dtype == D2R_F32) hipLaunchKernelGGL((dropout_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)x, (const float*)add, (float*)y, n, thresh, scale, seed, vec_ok);
  else return d2r_fail(D2R_ERR_INVALID, "d2r_dropout: bad dtype %d", dtype);
  return d2r_check_launch("d2r_dropout");
}

// ---- stochastic depth (DropPath) ---------------------------------------------------------------------------
// y = add + keep_path(b) / (1 - p_path) * dropout_elem(x) over [B, per_sample]: the residual branch of sample b is dropped whole
// when d2r_rand24(seed_path, b) falls below the threshold (an extension: the reference has no DropPath).  The sample rides on
// blockIdx.y, so the decision is taken once per block and sample, is uniform over the wave, and costs no division per element.
// A dropped sample is a select: its rows become a bit copy of `add` (+0 without it) and its x is never read.  A kept element
// is d2r_dropout's value times 1/(1 - p_path), in the same order of fp32 operations on the vector and the scalar path (no FMA
// contraction: both paths, and the composite layer and the op-by-op path, must agree bit for bit).  x and y may be one buffer.
template <typename T>
__device__ __forceinline__ T drop_path_value(T x, bool keep, float scale_elem, float scale_path, bool has_add, T add) {
#pragma clang fp contract(off)
  float v = keep ? to_f<T>(x) * scale_elem : 0.f;
  v = v * scale_path;
  if (has_add) v = v + to_f<T>(add);
  return from_f<T>(v);
}

template <typename T>
__global__ __launch_bounds__(256) void drop_path_kernel(const T* x, const T* add, T* y, int64_t B, int64_t per_sample, uint32_t thresh_path,
                                                        float scale_path, uint64_t seed_path, uint32_t thresh_elem, float scale_elem,
                                                        uint64_t seed_elem, int vec_ok) {
  constexpr int VEC = PackOf<T>::N;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t npk = vec_ok ? per_sample / VEC : 0;  // vec_ok: per_sample is a multiple of VEC, every sample starts on 16 bytes
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t base = b * per_sample;
    const T* xb = x + base;
    const T* ab = add ? add + base : nullptr;
    T* yb = y + base;
    if (d2r_rand24(seed_path, (uint64_t)b) < thresh_path) {  // dropped: copy the skip connection, never touch x
      Pack<T, VEC> zero;
#pragma unroll
      for (int j = 0; j < VEC; ++j) zero.v[j] = from_f<T>(0.f);
      for (int64_t k = tid; k < npk; k += nthreads) st_pack<T, VEC>(yb + k * VEC, ab ? ld_pack<T, VEC>(ab + k * VEC) : zero);
      for (int64_t e = npk * VEC + tid; e < per_sample; e += nthreads) yb[e] = ab ? ab[e] : zero.v[0];
      continue;
    }
    for (int64_t k = tid; k < npk; k += nthreads) {
      const Pack<T, VEC> px = ld_pack<T, VEC>(xb + k * VEC);
      Pack<T, VEC> pa = px, po;
      if (ab) pa = ld_pack<T, VEC>(ab + k * VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const bool keep = d2r_rand24(seed_elem, (uint64_t)(base + k * VEC + j)) >= thresh_elem;
        po.v[j] = drop_path_value<T>(px.v[j], keep, scale_elem, scale_path, ab != nullptr, pa.v[j]);
      }
      st_pack<T, VEC>(yb + k * VEC, po);
    }
    for (int64_t e = npk * VEC + tid; e < per_sample; e += nthreads) {
      const bool keep = d2r_rand24(seed_elem, (uint64_t)(base + e)) >= thresh_elem;
      yb[e] = drop_path_value<T>(xb[e], keep, scale_elem, scale_path, ab != nullptr, ab ? ab[e] : xb[e]);
    }
  }
}

extern "C" int d2r_drop_path(int dtype, const void* x, const void* add, void* y, int64_t B, int64_t per_sample, float p_path,
                             uint64_t seed_path, float p_elem, uint64_t seed_elem, void* stream) {
  D2R_REQUIRE(x && y && B >= 0 && per_sample >= 0, "d2r_drop_path: bad arguments (null x or y, or a negative size)");
  D2R_REQUIRE(p_path >= 0.f && p_path < 1.f && p_elem >= 0.f && p_elem < 1.f, "d2r_drop_path: probabilities must be in [0, 1)");
  D2R_REQUIRE(dtype == D2R_BF16 || dtype == D2R_F16 || dtype == D2R_F32, "d2r_drop_path: bad dtype %d", dtype);
  if (B == 0 || per_sample == 0) return D2R_OK;
  D2R_REQUIRE(per_sample <= INT64_MAX / B, "d2r_drop_path: B * per_sample overflows");
  if (p_path == 0.f) return d2r_dropout(dtype, x, add, y, B * per_sample, p_elem, seed_elem, stream);  // no path mask: bit for bit d2r_dropout
  const int VEC = dtype != D2R_F32 ? 8 : 4;
  const int vec_ok = d2r_aligned16(x) && d2r_aligned16(y) && d2r_aligned16(add) && per_sample % VEC == 0;
  const uint32_t thresh_path = d2r_drop_threshold(p_path), thresh_elem = d2r_drop_threshold(p_elem);
  const float scale_path = 1.f / (1.f - p_path), scale_elem = 1.f / (1.f - p_elem);
  const int gy = (int)(B < 65535 ? B : 65535);  // the sample on blockIdx.y (strided beyond the grid limit)
  const int64_t need = (per_sample / VEC + 1 + 255) / 256;
  const int64_t cap = 2048 / gy > 0 ? 2048 / gy : 1;  // ~256 CUs x 8 blocks in all, grid-stride inside the sample for the rest
  const dim3 grid((unsigned)(need < cap ? need : cap), (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == D2R_BF16) hipLaunchKernelGGL((drop_path_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)add, (bf16_t*)y, B, per_sample, thresh_path, scale_path, seed_path, thresh_elem, scale_elem, seed_elem, vec_ok);
  else if (dtype == D2R_F16) hipLaunchKernelGGL((drop_path_kernel<f16_t>), grid, dim3(256), 0, st, (const f16_t*)x, (const f16_t*)add, (f16_t*)y, B, per_sample, thresh_path, scale_path, seed_path, thresh_elem, scale_elem, seed_elem, vec_ok);
  else hipLaunchKernelGGL((drop_path_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (const float*)add, (float*)y, B, per_sample, thresh_path, scale_path, seed_path, thresh_elem, scale_elem, seed_elem, vec_ok);
  return d2r_check_launch("d2r_drop_path");
}

// out[0] = sum_k coef[k] * x_k[0]  (scalar loss combination: CE + js terms, models/unimo_model.py:160,
// models/modeling_unimo.py:849)
struct LinCombArgs {
  const float* x[8];
  float c[8];
};
__global__ void lincomb_kernel(LinCombArgs a, int n, float* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < n; ++k) t += a.c[k] * a.x[k][0];
    out[0] = t;
  }
}
extern "C" int d2r_lincomb(const float* const* h_x, const float* h_coef, int n, float* out, void* stream) {
  D2R_REQUIRE(h_x && h_coef && out && n >= 1 && n <= 8, "d2r_lincomb: bad arguments");
  LinCombArgs a;
  for (int k = 0; k < 8; ++k) {
    a.x[k] = k < n ? h_x[k] : nullptr;
    a.c[k] = k < n ? h_coef[k] : 0.f;
    D2R_REQUIRE(k >= n || a.x[k], "d2r_lincomb: null input %d", k);
  }
  hipLaunchKernelGGL(lincomb_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, n, out);
  return d2r_check_launch("d2r_lincomb");
}

// ---- casts ---------------------------------------------------------------------------------------------
template <typename S, typename Dt>
__global__ __launch_bounds__(256) void cast_kernel(const S* __restrict__ src, Dt* __restrict__ dst, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = n / 4;
  for (int64_t k = tid; k < n4; k += nthreads) {
    Pack<S, 4> a = ld_pack<S, 4>(src + k * 4);
    Pack<Dt, 4> b;
#pragma unroll
    for (int j = 0; j < 4; ++j) b.v[j] = from_f<Dt>(to_f<S>(a.v[j]));
    st_pack<Dt, 4>(dst + k * 4, b);
  }
  for (int64_t e = n4 * 4 + tid; e < n; e += nthreads) dst[e] = from_f<Dt>(to_f<S>(src[e]));
}

extern "C" int d2r_cast(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n, void* stream) {
  D2R_REQUIRE(src && dst && n >= 0, "d2r_cast: bad arguments");
  D2R_REQUIRE(d2r_aligned16(src) && d2r_aligned16(dst), "d2r_cast: pointers must be 16-byte aligned");
  if (n == 0) return D2R_OK;
  int blocks = (int)((n / 4 + 256) / 256);
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == D2R_F32 && dst_dtype == D2R_BF16) hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3(blocks), dim3(256), 0, st, (const float*)src, (bf16_t*)dst, n);
  else if (src_dtype == D2R_F32 && dst_dtype == D2R_F16) hipLaunchKernelGGL((cast_kernel<float, f16_t>), dim3(blocks), dim3(256), 0, st, (const float*)src, (f16_t*)dst, n);
  else if (src_dtype == D2R_BF16 && dst_dtype == D2R_F32) hipLaunchKernelGGL((cast_kernel<bf16_t, float>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)src, (float*)dst, n);
  else if (src_dtype == D2R_F16 && dst_dtype == D2R_F32) hipLaunchKernelGGL((cast_kernel<f16_t, float>), dim3(blocks), dim3(256), 0, st, (const f16_t*)src, (float*)dst, n);
  else if (src_dtype == D2R_F32 && dst_dtype == D2R_F32) hipLaunchKernelGGL((cast_kernel<float, float>), dim3(blocks), dim3(256), 0, st, (const float*)src, (float*)dst, n);
  else if (src_dtype == D2R_BF16 && dst_dtype == D2R_BF16) hipLaunchKernelGGL((cast_kernel<bf16_t, bf16_t>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, n);
  else if (src_dtype == D2R_F16 && dst_dtype == D2R_F16) hipLaunchKernelGGL((cast_kernel<f16_t, f16_t>), dim3(blocks), dim3(256), 0, st, (const f16_t*)src, (f16_t*)dst, n);
  else return d2r_fail(D2R_ERR_INVALID, "d2r_cast: bad dtypes %d -> %d", src_dtype, dst_dtype);
  return d2r_check_launch("d2r_cast");
}

// ---- strided row copy: dst[r][0..width) = src[r][0..width) for r < rows (byte pitches) -------------------------------------
// (hipMemcpy2DAsync device-to-device is issued by the runtime as one blit kernel PER ROW for these shapes: 148 launches of
//  3 us per training step for the three gathers / scatters of a routing layer; this is one launch each.)
__global__ __launch_bounds__(256) void copy_rows_kernel(unsigned char* __restrict__ dst, int64_t dpitch, const unsigned char* __restrict__ src,
                                                        int64_t spitch, int64_t width, int64_t rows, int vec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  if (vec) {
    const int64_t per_row = width / 16, total = per_row * rows;
    for (int64_t i = tid; i < total; i += nthreads) {
      const int64_t r = i / per_row, c = i - r * per_row;
      *reinterpret_cast<uint4*>(dst + r * dpitch + c * 16) = *reinterpret_cast<const uint4*>(src + r * spitch + c * 16);
    }
  } else {
    const int64_t total = width * rows;
    for (int64_t i = tid; i < total; i += nthreads) {
      const int64_t r = i / width, c = i - r * width;
      dst[r * dpitch + c] = src[r * spitch + c];
    }
  }
}
extern "C" int d2r_copy_rows(void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width, int64_t rows, void* stream) {
  D2R_REQUIRE(dst && src && width >= 0 && rows >= 0 && dst_pitch >= width && src_pitch >= width, "d2r_copy_rows: bad arguments");
  if (width == 0 || rows == 0) return D2R_OK;
  const int vec = d2r_aligned16(dst) && d2r_aligned16(src) && dst_pitch % 16 == 0 && src_pitch % 16 == 0 && width % 16 == 0;
  const int64_t work = (vec ? width / 16 : width) * rows;
  int blocks = (int)((work + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (unsigned char*)dst, dst_pitch, (const unsigned char*)src,
                     src_pitch, width, rows, vec);
  return d2r_check_launch("d2r_copy_rows");
}

// ---- K14 AdamW over a flat fp32 range (modules/train.py:287-322; torch.optim.AdamW semantics) -----------
typedef float f32x4nt __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ Pack<float, 4> ld4(const float* p) {
  if constexpr (NT) {
    const f32x4nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x4nt*>(p));
    Pack<float, 4> r;
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    return r;
  } else {
    return ld_pack<float, 4>(p);
  }
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, const Pack<float, 4>& v) {
  if constexpr (NT) {
    f32x4nt t;
    t.x = v.v[0], t.y = v.v[1], t.z = v.v[2], t.w = v.v[3];
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4nt*>(p));
  } else {
    st_pack<float, 4>(p, v);
  }
}

// CLIP: the gradient is also multiplied by the clipping coefficient *d_coef (d2r_grad_norm_finish), AFTER the unscale, as
// clip_grad_norm_ multiplies the already unscaled gradient: (g * gscale) * coef, two roundings.  CLIP = false is the plain step.
// EMA: an exponential moving average of the weights rides along as one more fp32 stream, e += omd * (w_new - e) with
// omd = 1 - decay_t (by value, or *d_omd in the hipGraph form) and w_new the weight this thread has just computed; a dropped step
// leaves it alone like w, m and v.  EMA = false is the step without it: nothing of ema / omd / d_omd is read.
template <typename H, bool NT, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    H* __restrict__ w16, int64_t n, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float bc2_sqrt, float gscale,
                                                    const float* __restrict__ d_hyper, const int* __restrict__ d_skip,
                                                    const float* __restrict__ d_coef, float* __restrict__ ema, float omd,
                                                    const float* __restrict__ d_omd) {
  if (d_skip && *d_skip) return;  // overflowed loss-scaled gradients: this step is dropped
  if (d_hyper) {  // hipGraph-safe variant: per-step scalars live in device memory, refreshed before each replay
    lr = d_hyper[0];
    bc1 = d_hyper[1];
    bc2_sqrt = d_hyper[2];
    gscale = d_hyper[3];
  }
  float coef = 1.f;
  if constexpr (CLIP) coef = *d_coef;
  if constexpr (EMA) {
    if (d_omd) omd = *d_omd;
  }
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = n / 4;
  auto upd = [&](float& wi, float gi, float& mi, float& vi) {
    gi *= gscale;
    if constexpr (CLIP) gi *= coef;
    wi *= (1.f - lr * wd);                       // decoupled weight decay
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    wi -= (lr / bc1) * (mi / denom);
  };
  for (int64_t k = tid; k < n4; k += nthreads) {
    Pack<float, 4> pw = ld4<NT>(w + k * 4), pg = ld4<NT>(g + k * 4);
    Pack<float, 4> pm = ld4<NT>(m + k * 4), pv = ld4<NT>(v + k * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) upd(pw.v[j], pg.v[j], pm.v[j], pv.v[j]);
    st4<NT>(w + k * 4, pw);
    st4<NT>(m + k * 4, pm);
    st4<NT>(v + k * 4, pv);
    if constexpr (EMA) {
      Pack<float, 4> pe = ld4<NT>(ema + k * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) pe.v[j] += omd * (pw.v[j] - pe.v[j]);
      st4<NT>(ema + k * 4, pe);
    }
    if (w16) {
      Pack<H, 4> ph;
#pragma unroll
      for (int j = 0; j < 4; ++j) ph.v[j] = (H)pw.v[j];
      st_pack<H, 4>(w16 + k * 4, ph);
    }
  }
  for (int64_t e = n4 * 4 + tid; e < n; e += nthreads) {
    float wi = w[e], mi = m[e], vi = v[e];
    upd(wi, g[e], mi, vi);
    w[e] = wi; m[e] = mi; v[e] = vi;
    if (w16) w16[e] = (H)wi;
  }
  if constexpr (EMA) {
    // The tail's average (at most 3 elements of the launch) in a loop of its own, reading back the weight this thread has just
    // stored: with these operations inside the loop above the compiler packs pairs of upd()'s scalar multiplies and adds instead of
    // fusing them as it does in the plain kernel, and w, m, v must equal the plain step bit for bit (tests/test_gpu_ema.py).
    for (int64_t e = n4 * 4 + tid; e < n; e += nthreads) {
      const float ei = ema[e];
      ema[e] = ei + omd * (w[e] - ei);
    }
  }
}

static int g_adamw_nt = 0, g_adamw_blocks = 0;  // A/B (include/d2r_hip_probes.h): non-temporal loads / stores, grid cap
extern "C" void d2r_adamw_probe_mode(int nt, int blocks) { g_adamw_nt = nt, g_adamw_blocks = blocks; }

static int adamw_launch(const char* name, float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n, float lr,
                        float b1, float b2, float eps, float wd, float bc1, float bc2s, float gscale, const float* d_hyper,
                        const int* d_skip, const float* d_coef, float* ema, float omd, const float* d_omd, void* stream) {
  D2R_REQUIRE(d2r_aligned16(w) && d2r_aligned16(g) && d2r_aligned16(m) && d2r_aligned16(v), "%s: pointers must be 16-byte aligned", name);
  D2R_REQUIRE(!w16 || ((reinterpret_cast<uintptr_t>(w16) & 7u) == 0 && d2r_is16(w16_dtype)),
              "%s: the 16-bit shadow must be 8-byte aligned and D2R_BF16 or D2R_F16 (got dtype %d)", name, w16_dtype);
  D2R_REQUIRE(!ema || d2r_aligned16(ema), "%s: the EMA buffer must be 16-byte aligned", name);
  if (n == 0) return D2R_OK;
  int blocks = (int)((n / 4 + 256) / 256);
  const int cap = g_adamw_blocks > 0 ? g_adamw_blocks : 2048;
  if (blocks > cap) blocks = cap;
#define D2R_ADAMW_LAUNCH(H, NT, CLIP, EMA) \
  hipLaunchKernelGGL((adamw_kernel<H, NT, CLIP, EMA>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (H*)w16, n, lr, b1, b2, eps, \
                     wd, bc1, bc2s, gscale, d_hyper, d_skip, d_coef, ema, omd, d_omd)
#define D2R_ADAMW_LAUNCH_NT(H, CLIP, EMA)       \
  if (g_adamw_nt) D2R_ADAMW_LAUNCH(H, true, CLIP, EMA); \
  else D2R_ADAMW_LAUNCH(H, false, CLIP, EMA)
#define D2R_ADAMW_LAUNCH_EMA(H, CLIP)       \
  if (ema) { D2R_ADAMW_LAUNCH_NT(H, CLIP, true); } \
  else { D2R_ADAMW_LAUNCH_NT(H, CLIP, false); }
  if (w16 && w16_dtype == D2R_F16) {
    if (d_coef) { D2R_ADAMW_LAUNCH_EMA(f16_t, true) }
    else { D2R_ADAMW_LAUNCH_EMA(f16_t, false) }
  } else {
    if (d_coef) { D2R_ADAMW_LAUNCH_EMA(bf16_t, true) }
    else { D2R_ADAMW_LAUNCH_EMA(bf16_t, false) }
  }
#undef D2R_ADAMW_LAUNCH_EMA
#undef D2R_ADAMW_LAUNCH_NT
#undef D2R_ADAMW_LAUNCH
  return d2r_check_launch(name);
}

extern "C" int d2r_adamw_step(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int64_t step,
                              float grad_scale, const int* d_skip, void* stream) {
  D2R_REQUIRE(w && g && m && v && n >= 0 && step >= 1, "d2r_adamw_step: bad arguments");
  // double on the host, rounded once: FusedAdamW.stage_hyper (the hipGraph path) computes the very same values
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  return adamw_launch("d2r_adamw_step", w, g, m, v, w16, w16_dtype, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale,
                      nullptr, d_skip, nullptr, nullptr, 0.f, nullptr, stream);
}

// the eager step with gradient clipping: d_coef = the coefficient d2r_grad_norm_finish wrote (device float)
extern "C" int d2r_adamw_step_clip(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                                   const int* d_skip, const float* d_coef, void* stream) {
  D2R_REQUIRE(w && g && m && v && d_coef && n >= 0 && step >= 1, "d2r_adamw_step_clip: bad arguments");
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  return adamw_launch("d2r_adamw_step_clip", w, g, m, v, w16, w16_dtype, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale,
                      nullptr, d_skip, d_coef, nullptr, 0.f, nullptr, stream);
}

// hipGraph-capturable form: d_hyper = device float[4] {lr, 1-beta1^t, sqrt(1-beta2^t), grad_scale}
extern "C" int d2r_adamw_step_dev(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n,
                                  const float* d_hyper, float beta1, float beta2, float eps, float weight_decay,
                                  const int* d_skip, void* stream) {
  D2R_REQUIRE(w && g && m && v && d_hyper && n >= 0, "d2r_adamw_step_dev: bad arguments");
  return adamw_launch("d2r_adamw_step_dev", w, g, m, v, w16, w16_dtype, n, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, 1.f, d_hyper,
                      d_skip, nullptr, nullptr, 0.f, nullptr, stream);
}
extern "C" int d2r_adamw_step_dev_clip(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n,
                                       const float* d_hyper, float beta1, float beta2, float eps, float weight_decay,
                                       const int* d_skip, const float* d_coef, void* stream) {
  D2R_REQUIRE(w && g && m && v && d_hyper && d_coef && n >= 0, "d2r_adamw_step_dev_clip: bad arguments");
  return adamw_launch("d2r_adamw_step_dev_clip", w, g, m, v, w16, w16_dtype, n, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, 1.f,
                      d_hyper, d_skip, d_coef, nullptr, 0.f, nullptr, stream);
}

// the two steps above with the weight EMA riding along (d_coef optional: clipping and EMA compose): ema = fp32 shadow laid out
// like w, ema_one_minus_decay = 1 - decay_t, computed by the caller in double and rounded once
extern "C" int d2r_adamw_step_ema(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                                  const int* d_skip, const float* d_coef, float* ema, float ema_one_minus_decay, void* stream) {
  D2R_REQUIRE(w && g && m && v && n >= 0 && step >= 1, "d2r_adamw_step_ema: bad arguments");
  D2R_REQUIRE(ema && ema != w, "d2r_adamw_step_ema: ema must be a buffer of its own (not NULL, not w)");
  D2R_REQUIRE(ema_one_minus_decay >= 0.f && ema_one_minus_decay <= 1.f, "d2r_adamw_step_ema: 1 - decay = %g is outside [0, 1]",
              (double)ema_one_minus_decay);
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  return adamw_launch("d2r_adamw_step_ema", w, g, m, v, w16, w16_dtype, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale,
                      nullptr, d_skip, d_coef, ema, ema_one_minus_decay, nullptr, stream);
}
// hipGraph-capturable: the factor is read from the device float d_ema_one_minus_decay (d_hyper[4] keeps its layout)
extern "C" int d2r_adamw_step_dev_ema(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t n,
                                      const float* d_hyper, float beta1, float beta2, float eps, float weight_decay,
                                      const int* d_skip, const float* d_coef, float* ema, const float* d_ema_one_minus_decay,
                                      void* stream) {
  D2R_REQUIRE(w && g && m && v && d_hyper && n >= 0, "d2r_adamw_step_dev_ema: bad arguments");
  D2R_REQUIRE(ema && ema != w, "d2r_adamw_step_dev_ema: ema must be a buffer of its own (not NULL, not w)");
  D2R_REQUIRE(d_ema_one_minus_decay, "d2r_adamw_step_dev_ema: d_ema_one_minus_decay is NULL");
  return adamw_launch("d2r_adamw_step_dev_ema", w, g, m, v, w16, w16_dtype, n, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, 1.f,
                      d_hyper, d_skip, d_coef, ema, 0.f, d_ema_one_minus_decay, stream);
}

// ---- K14 with per-range hyper-parameters: one launch over the flat buffers, {lr scale, weight decay, group} from a device table ----
// (layer-wise lr decay, no decay on 1-D parameters: an extension beyond the reference.  Several hundred runs of equal
// hyper-parameters would otherwise be a launch each.)
extern "C" int d2r_adamw_table_check(const d2r_adamw_seg* host_table, int nseg, int64_t n, int ngroups) {
  D2R_REQUIRE(host_table, "d2r_adamw_table_check: host_table is NULL");
  D2R_REQUIRE(nseg >= 1 && nseg <= D2R_ADAMW_MAX_SEGMENTS, "d2r_adamw_table_check: nseg = %d is outside 1..%d", nseg,
              D2R_ADAMW_MAX_SEGMENTS);
  D2R_REQUIRE(ngroups >= 1 && ngroups <= D2R_ADAMW_MAX_GROUPS, "d2r_adamw_table_check: ngroups = %d is outside 1..%d", ngroups,
              D2R_ADAMW_MAX_GROUPS);
  int64_t prev = 0;
  for (int s = 0; s < nseg; ++s) {
    const d2r_adamw_seg& t = host_table[s];
    D2R_REQUIRE(t.end > prev, "d2r_adamw_table_check: segment %d ends at %lld, not beyond %lld where it begins (ends must increase strictly)",
                s, (long long)t.end, (long long)prev);
    D2R_REQUIRE(std::isfinite(t.lr_scale) && t.lr_scale >= 0.f, "d2r_adamw_table_check: segment %d has lr_scale %g (must be finite and >= 0)",
                s, (double)t.lr_scale);
    D2R_REQUIRE(std::isfinite(t.weight_decay) && t.weight_decay >= 0.f,
                "d2r_adamw_table_check: segment %d has weight_decay %g (must be finite and >= 0)", s, (double)t.weight_decay);
    D2R_REQUIRE(t.group >= 0 && t.group < ngroups, "d2r_adamw_table_check: segment %d names group %d of %d", s, t.group, ngroups);
    D2R_REQUIRE(t.reserved == 0, "d2r_adamw_table_check: segment %d has reserved = %d (must be 0)", s, t.reserved);
    prev = t.end;
  }
  D2R_REQUIRE(prev == n, "d2r_adamw_table_check: segment %d, the last, ends at %lld but the buffers hold %lld elements", nseg - 1,
              (long long)prev, (long long)n);
  return D2R_OK;
}

struct AdamwGroupLr { float lr[D2R_ADAMW_MAX_GROUPS]; };  // the eager form's per-group lr, by value

// The first segment at or after `lo` whose end lies beyond element i.  The last segment's end is the table's end, which lies beyond
// every element of a launch, so the answer is at most nseg - 1 and nothing past the table is read.
__device__ __forceinline__ int adamw_seg_of(const d2r_adamw_seg* __restrict__ t, int lo, int nseg, int64_t i) {
  int hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid].end > i) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// lr of group q: row q of d_hyper (hipGraph form), else a select chain over the by-value array (a dynamic index would spill it).
// q comes from a table the host has checked; it is clamped all the same, so that no table can make this read out of bounds.
__device__ __forceinline__ float adamw_group_lr(const AdamwGroupLr& a, const float* __restrict__ d_hyper, int ngroups, int q) {
  q = q < 0 ? 0 : (q >= ngroups ? ngroups - 1 : q);
  if (d_hyper) return d_hyper[4 * q];
  float r = a.lr[0];
#pragma unroll
  for (int k = 1; k < D2R_ADAMW_MAX_GROUPS; ++k) r = q == k ? a.lr[k] : r;
  return r;
}

// What the update needs of an element's hyper-parameters: keep = 1 - lr * wd (decoupled weight decay), step = lr / bc1, with
// lr = lr[group] * lr_scale.  Three single operations, each rounded on its own (no contraction; fp32 division is correctly rounded),
// so the values are the same bits whether a workgroup derived them once for a whole segment or a lane for one element.
struct AdamwHyp { float keep, step; };
__device__ __forceinline__ AdamwHyp adamw_hyp(float lr_group, float lr_scale, float wd, float bc1) {
#pragma clang fp contract(off)
  const float lr = lr_group * lr_scale;
  AdamwHyp h;
  h.keep = 1.f - lr * wd;
  h.step = lr / bc1;
  return h;
}

// A workgroup's pass covers the 1,024 contiguous elements [begin + 1024 p, +1024): 256 lanes x one 16-byte pack, and a workgroup
// takes CONSECUTIVE passes (an equal share of them per workgroup, not a grid stride), so it walks through the table once: it finds
// the segment of its first element by a binary search all lanes run alike (uniform addresses), keeps that segment's end and values
// in registers, and looks again only when a span starts beyond that end - the model's segments are hundreds of passes long.  When
// the span ends inside the segment every lane takes the uniform values.  Otherwise each lane searches on from there for its pack,
// and a pack that a boundary cuts resolves per element.  Whatever path found the hyper-parameters, the update below is ONE piece of
// code, compiled without floating-point contraction: a copy the compiler makes of it for one path cannot round differently from
// another (the note in adamw_kernel on what contraction does to the same source in different loops), and a pack cut by `end` goes
// through it masked instead of through a scalar loop.  So an element's result does not depend on how [0, n) is cut into launches -
// replicas and the sharded step rely on that.
template <typename H, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_table_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, H* __restrict__ w16, int64_t begin, int64_t end,
                                                          const d2r_adamw_seg* __restrict__ table, int nseg, AdamwGroupLr glr,
                                                          int ngroups, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                          float gscale, const float* __restrict__ d_hyper,
                                                          const int* __restrict__ d_skip, const float* __restrict__ d_coef,
                                                          float* __restrict__ ema, float omd, const float* __restrict__ d_omd) {
  if (d_skip && *d_skip) return;  // overflowed loss-scaled gradients: this step is dropped
  if (d_hyper) {  // the step's scalars are the same in every row
    bc1 = d_hyper[1];
    bc2_sqrt = d_hyper[2];
    gscale = d_hyper[3];
  }
  float coef = 1.f;
  if constexpr (CLIP) coef = *d_coef;
  if constexpr (EMA) {
    if (d_omd) omd = *d_omd;
  }
  const int64_t npass = (end - begin + 1023) / 1024;
  const int64_t per = (npass + gridDim.x - 1) / gridDim.x;
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < npass ? p0 + per : npass;
  if (p0 >= p1) return;
  auto hyp_of = [&](int s) { return adamw_hyp(adamw_group_lr(glr, d_hyper, ngroups, table[s].group), table[s].lr_scale, table[s].weight_decay, bc1); };
  int s0 = adamw_seg_of(table, 0, nseg, begin + p0 * 1024);
  int64_t e0 = table[s0].end;
  AdamwHyp hu = hyp_of(s0);
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t span = begin + p * 1024;
    if (span >= e0) {  // the workgroup has left its segment (all lanes alike)
      s0 = adamw_seg_of(table, s0 + 1 < nseg ? s0 + 1 : nseg - 1, nseg, span);
      e0 = table[s0].end;
      hu = hyp_of(s0);
    }
    const int64_t i = span + (int64_t)threadIdx.x * 4;
    if (i >= end) continue;
    const bool full = i + 4 <= end;
    Pack<float, 4> pw, pg, pm, pv, pe;
    if (full) {
      pw = ld_pack<float, 4>(w + i), pg = ld_pack<float, 4>(g + i), pm = ld_pack<float, 4>(m + i), pv = ld_pack<float, 4>(v + i);
      if constexpr (EMA) pe = ld_pack<float, 4>(ema + i);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = i + j < end;
        pw.v[j] = ok ? w[i + j] : 0.f, pg.v[j] = ok ? g[i + j] : 0.f, pm.v[j] = ok ? m[i + j] : 0.f, pv.v[j] = ok ? v[i + j] : 0.f;
        if constexpr (EMA) pe.v[j] = ok ? ema[i + j] : 0.f;
      }
    }
    // ---- lookup: the hyper-parameters of the pack's four elements
    AdamwHyp h[4];
    const int64_t span_last = (span + 1024 < end ? span + 1024 : end) - 1;
    if (e0 > span_last) {
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = hu;
    } else {
      int s = adamw_seg_of(table, s0, nseg, i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < end)
          while (s < nseg - 1 && table[s].end <= i + j) ++s;
        h[j] = hyp_of(s);
      }
    }
    // ---- the update: the one arithmetic body
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gi = pg.v[j] * gscale;
        if constexpr (CLIP) gi = gi * coef;
        float wi = pw.v[j] * h[j].keep;  // decoupled weight decay
        const float mi = b1 * pm.v[j] + (1.f - b1) * gi;
        const float vi = b2 * pv.v[j] + (1.f - b2) * gi * gi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        wi = wi - h[j].step * (mi / denom);
        pw.v[j] = wi, pm.v[j] = mi, pv.v[j] = vi;
        if constexpr (EMA) pe.v[j] = pe.v[j] + omd * (wi - pe.v[j]);
      }
    }
    Pack<H, 4> ph;
#pragma unroll
    for (int j = 0; j < 4; ++j) ph.v[j] = (H)pw.v[j];
    if (full) {
      st_pack<float, 4>(w + i, pw);
      st_pack<float, 4>(m + i, pm);
      st_pack<float, 4>(v + i, pv);
      if constexpr (EMA) st_pack<float, 4>(ema + i, pe);
      if (w16) st_pack<H, 4>(w16 + i, ph);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j < end) {
          w[i + j] = pw.v[j], m[i + j] = pm.v[j], v[i + j] = pv.v[j];
          if constexpr (EMA) ema[i + j] = pe.v[j];
          if (w16) w16[i + j] = ph.v[j];
        }
      }
    }
  }
}

static int adamw_table_launch(const char* name, float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t begin,
                              int64_t end, const d2r_adamw_seg* d_table, int nseg, int64_t n, const AdamwGroupLr& glr, int ngroups,
                              float b1, float b2, float eps, float bc1, float bc2s, float gscale, const float* d_hyper,
                              const int* d_skip, const float* d_coef, float* ema, float omd, const float* d_omd, void* stream) {
  D2R_REQUIRE(w && g && m && v && d_table, "%s: bad arguments (a NULL pointer)", name);
  D2R_REQUIRE(nseg >= 1 && nseg <= D2R_ADAMW_MAX_SEGMENTS, "%s: nseg = %d is outside 1..%d", name, nseg, D2R_ADAMW_MAX_SEGMENTS);
  D2R_REQUIRE(ngroups >= 1 && ngroups <= D2R_ADAMW_MAX_GROUPS, "%s: ngroups = %d is outside 1..%d", name, ngroups, D2R_ADAMW_MAX_GROUPS);
  D2R_REQUIRE(begin >= 0 && begin <= end && end <= n, "%s: [begin, end) = [%lld, %lld) must lie inside the table's [0, %lld)", name,
              (long long)begin, (long long)end, (long long)n);
  D2R_REQUIRE(begin % 4 == 0, "%s: begin = %lld must be a multiple of 4 (16-byte packs)", name, (long long)begin);
  D2R_REQUIRE(d2r_aligned16(w) && d2r_aligned16(g) && d2r_aligned16(m) && d2r_aligned16(v), "%s: pointers must be 16-byte aligned", name);
  D2R_REQUIRE(!w16 || ((reinterpret_cast<uintptr_t>(w16) & 7u) == 0 && d2r_is16(w16_dtype)),
              "%s: the 16-bit shadow must be 8-byte aligned and D2R_BF16 or D2R_F16 (got dtype %d)", name, w16_dtype);
  D2R_REQUIRE(!ema || (d2r_aligned16(ema) && ema != w), "%s: ema must be a 16-byte aligned buffer of its own (not w)", name);
  D2R_REQUIRE((reinterpret_cast<uintptr_t>(d_table) & 7u) == 0, "%s: d_table must be 8-byte aligned", name);
  if (end == begin) return D2R_OK;
  const int64_t npass = (end - begin + 1023) / 1024;
  const int cap = g_adamw_blocks > 0 ? g_adamw_blocks : 2048;
  const int blocks = (int)(npass < cap ? npass : cap);
#define D2R_ADAMW_TABLE_LAUNCH(H, CLIP, EMA)                                                                                        \
  hipLaunchKernelGGL((adamw_table_kernel<H, CLIP, EMA>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (H*)w16, begin, \
                     end, d_table, nseg, glr, ngroups, b1, b2, eps, bc1, bc2s, gscale, d_hyper, d_skip, d_coef, ema, omd, d_omd)
#define D2R_ADAMW_TABLE_LAUNCH_EMA(H, CLIP)         \
  if (ema) D2R_ADAMW_TABLE_LAUNCH(H, CLIP, true); \
  else D2R_ADAMW_TABLE_LAUNCH(H, CLIP, false)
  if (w16 && w16_dtype == D2R_F16) {
    if (d_coef) { D2R_ADAMW_TABLE_LAUNCH_EMA(f16_t, true); }
    else { D2R_ADAMW_TABLE_LAUNCH_EMA(f16_t, false); }
  } else {
    if (d_coef) { D2R_ADAMW_TABLE_LAUNCH_EMA(bf16_t, true); }
    else { D2R_ADAMW_TABLE_LAUNCH_EMA(bf16_t, false); }
  }
#undef D2R_ADAMW_TABLE_LAUNCH_EMA
#undef D2R_ADAMW_TABLE_LAUNCH
  return d2r_check_launch(name);
}

extern "C" int d2r_adamw_step_table(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t begin, int64_t end,
                                    const d2r_adamw_seg* d_table, int nseg, int64_t n, const float* lr, int ngroups, float beta1,
                                    float beta2, float eps, int64_t step, float grad_scale, const int* d_skip, const float* d_coef,
                                    float* ema, float ema_one_minus_decay, void* stream) {
  D2R_REQUIRE(lr && step >= 1, "d2r_adamw_step_table: bad arguments (lr is NULL or step < 1)");
  D2R_REQUIRE(ngroups >= 1 && ngroups <= D2R_ADAMW_MAX_GROUPS, "d2r_adamw_step_table: ngroups = %d is outside 1..%d", ngroups,
              D2R_ADAMW_MAX_GROUPS);
  D2R_REQUIRE(!ema || (ema_one_minus_decay >= 0.f && ema_one_minus_decay <= 1.f), "d2r_adamw_step_table: 1 - decay = %g is outside [0, 1]",
              (double)ema_one_minus_decay);
  AdamwGroupLr glr = {};
  for (int q = 0; q < ngroups; ++q) glr.lr[q] = lr[q];
  // double on the host, rounded once, as d2r_adamw_step does: FusedAdamW.stage_hyper computes the very same values
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  return adamw_table_launch("d2r_adamw_step_table", w, g, m, v, w16, w16_dtype, begin, end, d_table, nseg, n, glr, ngroups, beta1, beta2,
                            eps, bc1, bc2s, grad_scale, nullptr, d_skip, d_coef, ema, ema_one_minus_decay, nullptr, stream);
}
extern "C" int d2r_adamw_step_table_dev(float* w, const float* g, float* m, float* v, void* w16, int w16_dtype, int64_t begin,
                                        int64_t end, const d2r_adamw_seg* d_table, int nseg, int64_t n, const float* d_hyper,
                                        int ngroups, float beta1, float beta2, float eps, const int* d_skip, const float* d_coef,
                                        float* ema, const float* d_ema_one_minus_decay, void* stream) {
  D2R_REQUIRE(d_hyper, "d2r_adamw_step_table_dev: d_hyper is NULL");
  D2R_REQUIRE(!ema || d_ema_one_minus_decay, "d2r_adamw_step_table_dev: d_ema_one_minus_decay is NULL");
  const AdamwGroupLr glr = {};
  return adamw_table_launch("d2r_adamw_step_table_dev", w, g, m, v, w16, w16_dtype, begin, end, d_table, nseg, n, glr, ngroups, beta1,
                            beta2, eps, 1.f, 1.f, 1.f, d_hyper, d_skip, d_coef, ema, 0.f, d_ema_one_minus_decay, stream);
}

// ---- a[i] <-> b[i] over two disjoint fp32 ranges in one pass (evaluation on the averaged weights: FusedAdamW.ema_weights) -----
__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n, int vec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t k = tid; k < n4; k += nthreads) {
    const Pack<float, 4> pa = ld_pack<float, 4>(a + k * 4), pb = ld_pack<float, 4>(b + k * 4);
    st_pack<float, 4>(a + k * 4, pb);
    st_pack<float, 4>(b + k * 4, pa);
  }
  for (int64_t e = n4 * 4 + tid; e < n; e += nthreads) {
    const float x = a[e], y = b[e];
    a[e] = y;
    b[e] = x;
  }
}
extern "C" int d2r_swap_f32(float* a, float* b, int64_t n, void* stream) {
  D2R_REQUIRE(a && b && n >= 0, "d2r_swap_f32: bad arguments");
  const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * 4u;
  D2R_REQUIRE(ua + bytes <= ub || ub + bytes <= ua, "d2r_swap_f32: the two ranges overlap");
  if (n == 0) return D2R_OK;
  const int vec = d2r_aligned16(a) && d2r_aligned16(b);
  const int64_t work = vec ? n / 4 + 3 : n;  // (the tail of a vector launch: at most 3 elements)
  int blocks = (int)((work + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(swap_f32_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, n, vec);
  return d2r_check_launch("d2r_swap_f32");
}

// ---- overflow check of loss-scaled gradients (fp16 compute dtype): one streaming pass, flag |= any(!isfinite(g)) -----
__global__ __launch_bounds__(256) void nonfinite_kernel(const float* __restrict__ g, int64_t n, int* __restrict__ flag) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = n / 4;
  bool bad = false;
  for (int64_t k = tid; k < n4; k += nthreads) {
    const Pack<float, 4> p = ld_pack<float, 4>(g + k * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= !(fabsf(p.v[j]) <= 3.4028234e38f);  // false for inf and for NaN
  }
  for (int64_t e = n4 * 4 + tid; e < n; e += nthreads) bad |= !(fabsf(g[e]) <= 3.4028234e38f);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
extern "C" int d2r_grad_nonfinite(const float* g, int64_t n, int* d_flag, void* stream) {
  D2R_REQUIRE(g && d_flag && n >= 0 && d2r_aligned16(g), "d2r_grad_nonfinite: bad arguments");
  if (n == 0) return D2R_OK;
  int blocks = (int)((n / 4 + 256) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(nonfinite_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, d_flag);
  return d2r_check_launch("d2r_grad_nonfinite");
}

// ---- global L2 norm of the gradient for clipping (torch.nn.utils.clip_grad_norm_, norm type 2; an extension beyond the reference) --
// Pass 1, d2r_grad_sumsq: a fixed grid of D2R_GRAD_NORM_PARTS workgroups; every thread adds the squares of its grid-stride share of
// each range in fp64 (the square of an fp32 value is exact there and 3.5e8 squares of |g| <= 3.4e38 stay far below the fp64
// limit, so loss-scaled gradients cannot overflow the sum), and every workgroup stores ONE fp64 partial - no atomics, so the same
// gradients give the same bits on every run.  A partial is finite exactly when every gradient it covers is.
// Pass 2, d2r_grad_norm_finish: one workgroup sums the partials in a fixed order and writes {norm, coef}.
struct GradRanges {
  int64_t lo[D2R_GRAD_NORM_MAX_RANGES], hi[D2R_GRAD_NORM_MAX_RANGES];
  int n;
};

__device__ __forceinline__ void sumsq4(double& acc, const Pack<float, 4>& p) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double x = (double)p.v[j];
    acc = fma(x, x, acc);
  }
}

// fixed-order sum over a 256-thread workgroup (the xor butterfly leaves the same bits in every lane); every thread gets the sum
__device__ __forceinline__ double block_sum_f64_256(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, GradRanges r, double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int i = 0; i < r.n; ++i) {
    const float* p = g + r.lo[i];
    const int64_t n = r.hi[i] - r.lo[i], n4 = n / 4;
    int64_t k = tid;
    for (; k + 3 * nthreads < n4; k += 4 * nthreads) {  // four 16-byte loads in flight, added in index order
      const Pack<float, 4> a = ld_pack<float, 4>(p + k * 4), b = ld_pack<float, 4>(p + (k + nthreads) * 4);
      const Pack<float, 4> c = ld_pack<float, 4>(p + (k + 2 * nthreads) * 4), d = ld_pack<float, 4>(p + (k + 3 * nthreads) * 4);
      sumsq4(acc, a);
      sumsq4(acc, b);
      sumsq4(acc, c);
      sumsq4(acc, d);
    }
    for (; k < n4; k += nthreads) sumsq4(acc, ld_pack<float, 4>(p + k * 4));
    for (int64_t e = n4 * 4 + tid; e < n; e += nthreads) {
      const double x = (double)p[e];
      acc = fma(x, x, acc);
    }
  }
  acc = block_sum_f64_256(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

extern "C" int d2r_grad_sumsq(const float* g, const int64_t* h_ranges, int nranges, double* slab, int64_t slab_len, void* stream) {
  D2R_REQUIRE(slab && (h_ranges || nranges == 0), "d2r_grad_sumsq: null pointer");
  D2R_REQUIRE(nranges >= 0 && nranges <= D2R_GRAD_NORM_MAX_RANGES, "d2r_grad_sumsq: %d ranges (at most %d per call)", nranges,
              D2R_GRAD_NORM_MAX_RANGES);
  D2R_REQUIRE(slab_len >= D2R_GRAD_NORM_PARTS, "d2r_grad_sumsq: the slab holds %lld partials, a call writes %d", (long long)slab_len,
              D2R_GRAD_NORM_PARTS);
  GradRanges r;
  memset(&r, 0, sizeof(r));
  r.n = nranges;
  bool empty = true;
  for (int i = 0; i < nranges; ++i) {
    const int64_t lo = h_ranges[2 * i], hi = h_ranges[2 * i + 1];
    D2R_REQUIRE(lo >= 0 && hi >= lo, "d2r_grad_sumsq: range %d = [%lld, %lld) is not a range", i, (long long)lo, (long long)hi);
    D2R_REQUIRE(lo % 4 == 0, "d2r_grad_sumsq: range %d starts at element %lld, not on a 16-byte boundary", i, (long long)lo);
    r.lo[i] = lo, r.hi[i] = hi;
    empty &= hi == lo;
  }
  // (an empty buffer may have no address: g is only needed when there is something to read)
  D2R_REQUIRE(empty || (g && d2r_aligned16(g)), "d2r_grad_sumsq: the gradient must be a 16-byte aligned device pointer");
  // always the full grid, empty ranges included: every partial of the slab is written (zeros where there is nothing to add)
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(D2R_GRAD_NORM_PARTS), dim3(256), 0, (hipStream_t)stream, g, r, slab);
  return d2r_check_launch("d2r_grad_sumsq");
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ part, int64_t nparts, float unscale,
                                                               const float* __restrict__ d_unscale, float max_norm, float* __restrict__ out,
                                                               int* __restrict__ flag) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += 256) acc += part[i];
  const double total = block_sum_f64_256(acc, sh);
  if (threadIdx.x == 0) {
    const double us = (double)(d_unscale ? *d_unscale : unscale);
    const float norm = (float)(sqrt(total) * us);  // one rounding; with a power-of-two unscale the same bits as the unscaled sum's norm
    // torch: clamp(max_norm / (total_norm + 1e-6), max=1) in fp32, where `scalar / tensor` is reciprocal(tensor) * scalar;
    // clamp keeps a NaN
    const float q = (1.f / (norm + 1e-6f)) * max_norm;
    out[0] = norm;
    out[1] = (q < 1.f || q != q) ? q : 1.f;
    if (flag && !(total <= 1.7976931348623157e308)) *flag = 1;  // an inf or a NaN among the gradients: a dropped loss-scaled step
  }
}

extern "C" int d2r_grad_norm_finish(const double* slab, int64_t nparts, float unscale, const float* d_unscale, float max_norm, float* d_out,
                                    int* d_flag, void* stream) {
  D2R_REQUIRE(slab && d_out, "d2r_grad_norm_finish: null pointer");
  D2R_REQUIRE(nparts >= 1, "d2r_grad_norm_finish: no partials");
  D2R_REQUIRE(max_norm > 0.f, "d2r_grad_norm_finish: max_norm must be positive (got %g)", (double)max_norm);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, slab, nparts, unscale, d_unscale, max_norm, d_out,
                     d_flag);
  return d2r_check_launch("d2r_grad_norm_finish");
}
