// image.hip — CLIP image preprocessing on the device (processor/dataset.py:87-95): Pillow's antialiased fixed-point bicubic
// resize, center crop, rescale and normalisation of a batch of decoded uint8 RGB images of different sizes, bit-identical to
// CLIPImageProcessor.  Integer multiply-accumulate only; the float64 coefficient tables are built on the host.
//
// Pillow (ImagingResample, 8 bits per channel) resizes in two separable passes: horizontal first, into a uint8 image, then
// vertical from that image.  Each pass computes, per output pixel, 2^21 + sum_t in[xmin + t] * k[t] in int32 with 22-bit weights
// and clips (>> 22) to uint8.  An output pixel depends only on its own weights, so computing the crop alone is exact: pass 1 runs
// on the source rows the crop rows' vertical support touches, S crop columns wide, into the workspace; pass 2 runs the vertical
// weights over those rows and maps every (channel, uint8) pair through the normalisation table.
//
// The dataset cache (d2r_amd/cache.py) keeps pass 2's uint8 value instead of the table's: d2r_clip_preprocess_u8 writes the crop,
// planar [3, S, S], into a row of a device-resident cache, and d2r_clip_cache_gather maps rows picked by index through the table
// into the fp32 batch.  d2r_gather_rows does the same row pick for the token tensors.  d2r_clip_cache_augment is the gather with
// a per-sample box of the crop resampled bilinearly to S x S and an optional mirror (d2r_amd/augment.py: random resized crop, flip).
// d2r_clip_cache_augment_photo resamples the raw values instead of the table's and applies brightness, contrast, saturation, hue,
// grayscale, the normalisation and an erase box per sample (K22: colour jitter, random grayscale, random erasing).
// d2r_image_mix (K24) runs after all of them, on the finished fp32 batch: every sample is blended with, or gets a box pasted from,
// another sample of the batch (d2r_amd/mix.py: MixUp, CutMix).
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int HROWS = 4;  // source rows per pass-1 workgroup: each weight is loaded once for HROWS rows

__device__ __forceinline__ int clip8(int v) { return v >= (1 << 30) ? 255 : (v <= 0 ? 0 : v >> 22); }

// pass 1: ws[r, j, c] = clip8(sum_t src[row0 + r, xmin_j + t, c] * kx_j[t]) for r < nrows, j < S
__global__ __launch_bounds__(256) void clip_hpass_kernel(const uint8_t* __restrict__ src, const d2r_clip_image_desc* __restrict__ desc,
                                                         const int32_t* __restrict__ tab, int S, uint8_t* __restrict__ ws) {
  const d2r_clip_image_desc d = desc[blockIdx.y];
  const int r0 = blockIdx.x * HROWS;
  if (r0 >= d.nrows) return;
  const int nr = min(HROWS, d.nrows - r0);
  const int64_t pitch = (int64_t)d.W * 3;
  const uint8_t* in = src + d.src_offset + (int64_t)(d.row0 + r0) * pitch;
  uint8_t* o = ws + d.ws_offset + (int64_t)r0 * S * 3;
  for (int j = threadIdx.x; j < S; j += 256) {
    const int xmin = tab[d.bx + 2 * j], n = tab[d.bx + 2 * j + 1];
    const int32_t* k = tab + d.cx + (int64_t)j * d.kx;
    int acc[HROWS][3];
#pragma unroll
    for (int r = 0; r < HROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << 21;
    const uint8_t* p = in + xmin * 3;
    for (int t = 0; t < n; ++t, p += 3) {
      const int w = k[t];
#pragma unroll
      for (int r = 0; r < HROWS; ++r) {
        const uint8_t* q = p + (r < nr ? r : nr - 1) * pitch;  // rows past the image's last are read again, not written
        acc[r][0] += (int)q[0] * w;
        acc[r][1] += (int)q[1] * w;
        acc[r][2] += (int)q[2] * w;
      }
    }
#pragma unroll
    for (int r = 0; r < HROWS; ++r) {
      if (r < nr) {
        uint8_t* q = o + ((int64_t)r * S + j) * 3;
        q[0] = (uint8_t)clip8(acc[r][0]);
        q[1] = (uint8_t)clip8(acc[r][1]);
        q[2] = (uint8_t)clip8(acc[r][2]);
      }
    }
  }
}

// pass 2: out[b, c, i, j] = lut[c, clip8(sum_t ws[ymin_i - row0 + t, j, c] * ky_i[t])]; U8: the clip8 value itself, planar, into row
// slots[b] of the cache (no table)
template <bool U8>
__global__ __launch_bounds__(256) void clip_vpass_kernel(const d2r_clip_image_desc* __restrict__ desc, const int32_t* __restrict__ tab,
                                                         const uint8_t* __restrict__ ws, const float* __restrict__ lut, int S,
                                                         float* __restrict__ out, uint8_t* __restrict__ cache,
                                                         const int64_t* __restrict__ slots, int64_t row_bytes) {
  __shared__ float sl[U8 ? 1 : 3 * 256];
  if constexpr (!U8) {
    for (int i = threadIdx.x; i < 3 * 256; i += 256) sl[i] = lut[i];
    __syncthreads();
  }
  const d2r_clip_image_desc d = desc[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * S) return;
  const int i = idx / S, j = idx - i * S;
  const int ymin = tab[d.by + 2 * i] - d.row0, n = tab[d.by + 2 * i + 1];
  const int32_t* k = tab + d.cy + (int64_t)i * d.ky;
  const int64_t pitch = (int64_t)S * 3;
  const uint8_t* p = ws + d.ws_offset + (int64_t)ymin * pitch + j * 3;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int t = 0; t < n; ++t, p += pitch) {
    const int w = k[t];
    a0 += (int)p[0] * w;
    a1 += (int)p[1] * w;
    a2 += (int)p[2] * w;
  }
  const int64_t plane = (int64_t)S * S;
  if constexpr (U8) {
    uint8_t* o = cache + slots[blockIdx.y] * row_bytes + idx;
    o[0] = (uint8_t)clip8(a0);
    o[plane] = (uint8_t)clip8(a1);
    o[2 * plane] = (uint8_t)clip8(a2);
  } else {
    float* o = out + (int64_t)blockIdx.y * 3 * plane + idx;
    o[0] = sl[clip8(a0)];
    o[plane] = sl[256 + clip8(a1)];
    o[2 * plane] = sl[512 + clip8(a2)];
  }
}

// out[b, c, i, j] = lut[c][cache[idx[b]][c, i, j]]: one 16-byte chunk of the cache row per thread, four 16-byte stores.  A chunk
// that straddles two channels or the row's padding, or whose output is not 16-byte aligned (odd S), goes byte by byte.
__global__ __launch_bounds__(256) void clip_cache_gather_kernel(const uint8_t* __restrict__ cache, int64_t row_bytes,
                                                                const int64_t* __restrict__ idx, int S, const float* __restrict__ lut,
                                                                float* __restrict__ out) {
  __shared__ float sl[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) sl[i] = lut[i];
  __syncthreads();
  const int64_t row = idx[blockIdx.y];  // uniform: one scalar load per workgroup
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (p0 >= row_bytes) return;
  const int plane = S * S, n = 3 * plane;
  const uint4 v = *reinterpret_cast<const uint4*>(cache + row * row_bytes + p0);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float* o = out + (int64_t)blockIdx.y * n + p0;
  const int c = (int)(p0 / plane);
  if (p0 + 16 <= n && (int)((p0 + 15) / plane) == c && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
    const float* t = sl + c * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(o + 4 * q) =
          make_float4(t[w[q] & 255u], t[(w[q] >> 8) & 255u], t[(w[q] >> 16) & 255u], t[w[q] >> 24]);
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t p = p0 + q;
      if (p < n) o[q] = sl[(int)(p / plane) * 256 + ((w[q >> 2] >> (8 * (q & 3))) & 255u)];
    }
  }
}

// One axis of the bilinear resampling of a box of n source pixels to S output pixels (torch's interpolate, align_corners=False):
// output position o (already mirrored when flipped) reads the taps lo and hi of the box with weight f on hi.  Integers up to
// the one division into f, so that n == S gives lo == o and f == 0 exactly.
struct aug_tap {
  int lo, hi;
  float f;
};
__device__ __forceinline__ aug_tap aug_axis(int o, int n, int S) {
  const int num = (2 * o + 1) * n - S;  // < 2 * 4096 * 4096
  const unsigned nx = num < 0 ? 0u : (unsigned)num, den = 2u * (unsigned)S;
  const unsigned q = nx / den;
  aug_tap t;
  t.lo = (int)q;
  t.hi = min(t.lo + 1, n - 1);  // clamped to the box, not to the image
  t.f = (float)(nx - q * den) / (float)den;
  return t;
}

// fp32, every product and sum rounded on its own (no contraction into fma): (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c
// + fx * d).  With fx == fy == 0 this is a, bit for bit, for finite table entries.
__device__ __forceinline__ float aug_blend(float a, float b, float c, float d, float fx, float fy) {
#pragma clang fp contract(off)
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float top = gx * a + fx * b;
  const float bot = gx * c + fx * d;
  return gy * top + fy * bot;
}

// out[b, c, i, j] = the box aug[b] of lut[c][cache[idx[b]][c]] resampled bilinearly to S x S, mirrored when aug[b].flip: four
// consecutive columns of one output row per thread (quads = ceil(S / 4) per row), one float4 (compiled to a 12-byte and a 4-byte
// store) when S is a multiple of 4 and `out` 16-byte aligned, single stores otherwise.  The sixteen byte taps lie in two source rows.
__global__ __launch_bounds__(256) void clip_cache_augment_kernel(const uint8_t* __restrict__ cache, int64_t row_bytes,
                                                                 const int64_t* __restrict__ idx,
                                                                 const d2r_clip_augment_desc* __restrict__ aug, int S, int quads,
                                                                 const float* __restrict__ lut, float* __restrict__ out) {
  __shared__ float sl[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) sl[i] = lut[i];
  __syncthreads();
  const d2r_clip_augment_desc d = aug[blockIdx.y];  // uniform: scalar loads
  const int t = blockIdx.x * 256 + threadIdx.x;     // < 3 * 4096 * 1024
  if (t >= 3 * S * quads) return;
  const int line = t / quads, j0 = (t - line * quads) * 4;
  const int c = line / S, i = line - c * S;
  const int plane = S * S;
  const aug_tap ty = aug_axis(i, d.h, S);
  const uint8_t* p = cache + idx[blockIdx.y] * row_bytes + (int64_t)c * plane + d.x0;
  const uint8_t* r0 = p + (d.y0 + ty.lo) * S;
  const uint8_t* r1 = p + (d.y0 + ty.hi) * S;
  const float* tab = sl + c * 256;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = min(j0 + k, S - 1);  // columns past the row (S no multiple of 4) are computed again, not written
    const aug_tap tx = aug_axis(d.flip ? S - 1 - j : j, d.w, S);
    v[k] = aug_blend(tab[r0[tx.lo]], tab[r0[tx.hi]], tab[r1[tx.lo]], tab[r1[tx.hi]], tx.f, ty.f);
  }
  float* o = out + (int64_t)blockIdx.y * 3 * plane + (int64_t)line * S + j0;
  if ((S & 3) == 0 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < S) o[k] = v[k];
  }
}

// ---- K22: photometric augmentation (colour jitter, grayscale, erasing) of the resampled box, before the normalisation ----

constexpr int PHOTO_BLOCK = 256;  // threads per workgroup of both K22 kernels = pixels quads per partial sum of the statistics pass

__device__ __forceinline__ float photo_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }  // a NaN becomes 0

// g(x) = 0.299 R + 0.587 G + 0.114 B, summed left to right
__device__ __forceinline__ float photo_gray(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// K21's resample (aug_axis / aug_blend, the same taps) of the raw values P * rescale for columns j0 .. j0 + 3 of output row i, all
// three channels; `row` is the sample's cache row.  Columns past the row are computed again from column S - 1.
__device__ __forceinline__ void photo_resample(const uint8_t* __restrict__ row, const d2r_clip_augment_desc& d, int flip, int i, int j0,
                                               int S, float rescale, float x[3][4]) {
  const int plane = S * S;
  const aug_tap ty = aug_axis(i, d.h, S);
  const uint8_t* r0 = row + d.x0 + (d.y0 + ty.lo) * S;
  const uint8_t* r1 = row + d.x0 + (d.y0 + ty.hi) * S;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = min(j0 + k, S - 1);
    const aug_tap tx = aug_axis(flip ? S - 1 - j : j, d.w, S);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* p0 = r0 + c * plane;
      const uint8_t* p1 = r1 + c * plane;
      x[c][k] = aug_blend((float)p0[tx.lo] * rescale, (float)p0[tx.hi] * rescale, (float)p1[tx.lo] * rescale, (float)p1[tx.hi] * rescale,
                          tx.f, ty.f);
    }
  }
}

// step 1 (skipped by the caller when beta == 1)
__device__ __forceinline__ float photo_brightness(float x, float beta) { return photo_clamp01(beta * x); }

// step 4: RGB -> HSV (hexcone; h = 0 when max == min, s = 0 when max == 0), h <- frac(h + delta), HSV -> RGB
__device__ __forceinline__ void photo_hue(float& r, float& g, float& b, float delta) {
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float cr = mx - mn;
  const bool grey = cr == 0.0f;
  const float s = cr / (grey ? 1.0f : mx);  // mx > 0 when cr > 0
  const float inv = 1.0f / (grey ? 1.0f : cr);
  const float rc = (mx - r) * inv, gc = (mx - g) * inv, bc = (mx - b) * inv;
  const float h6 = mx == r ? bc - gc : (mx == g ? 2.0f + rc - bc : 4.0f + gc - rc);  // in [-1, 5]
  float h = h6 * (1.0f / 6.0f) + delta;                                              // in (-0.67, 1.34)
  h = h - floorf(h);                                                                 // in [0, 1]; 1 when h was a tiny negative
  const float hs = h * 6.0f, fl = floorf(hs), f = hs - fl;
  int sec = (int)fl;
  if (sec >= 6) sec -= 6;  // hs == 6 has f == 0, where sector 0 gives what sector 5 gives at f == 1
  const float p = photo_clamp01(mx * (1.0f - s)), q = photo_clamp01(mx * (1.0f - s * f)), t = photo_clamp01(mx * (1.0f - s * (1.0f - f)));
  r = sec == 0 || sec == 5 ? mx : (sec == 1 ? q : (sec == 4 ? t : p));
  g = sec == 1 || sec == 2 ? mx : (sec == 0 ? t : (sec == 3 ? q : p));
  b = sec == 3 || sec == 4 ? mx : (sec == 2 ? t : (sec == 5 ? q : p));
}

// Statistics pass of the contrast step: for every sample with contrast != 1, ws[b * gridDim.x + blockIdx.x] = the sum of g(x) after
// step 1 over this workgroup's PHOTO_BLOCK pixel quads, always in the same order: a thread adds its four pixels left to right, a
// wavefront halves six times (lane l += lane l + 32, 16, ... 1), thread 0 adds the four wavefronts' sums in order.  The resample is
// taken unmirrored: the mean over all pixels does not depend on the mirror, and so neither do its bits.
__global__ __launch_bounds__(PHOTO_BLOCK) void clip_photo_stats_kernel(const uint8_t* __restrict__ cache, int64_t row_bytes,
                                                                       const int64_t* __restrict__ idx,
                                                                       const d2r_clip_augment_desc* __restrict__ aug,
                                                                       const d2r_clip_photo_desc* __restrict__ photo, int S, int quads,
                                                                       float rescale, float* __restrict__ ws) {
  __shared__ float sw[PHOTO_BLOCK / 64];
  const d2r_clip_photo_desc ph = photo[blockIdx.y];  // uniform: scalar loads
  if (ph.contrast == 1.0f) return;                   // the whole workgroup: the apply kernel does not read this sample's partials
  const d2r_clip_augment_desc d = aug[blockIdx.y];
  const int t = blockIdx.x * PHOTO_BLOCK + threadIdx.x;  // < 4096 * 1024
  float s = 0.0f;
  if (t < S * quads) {
    const int i = t / quads, j0 = (t - i * quads) * 4;
    float x[3][4];
    photo_resample(cache + idx[blockIdx.y] * row_bytes, d, 0, i, j0, S, rescale, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (ph.brightness != 1.0f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c][k] = photo_brightness(x[c][k], ph.brightness);
      }
      if (j0 + k < S) s += photo_gray(x[0][k], x[1][k], x[2][k]);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ws[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// out[b, :, i, j0 .. j0 + 3] for one thread: the resample, steps 1 to 7 of K22 on the three channels together, three float4 under
// K21's alignment rule (single stores otherwise).  `parts` partial sums per sample are added in index order for the contrast mean.
struct photo_norm {
  float mean[3], std[3];
};
__global__ __launch_bounds__(PHOTO_BLOCK) void clip_photo_apply_kernel(const uint8_t* __restrict__ cache, int64_t row_bytes,
                                                                       const int64_t* __restrict__ idx,
                                                                       const d2r_clip_augment_desc* __restrict__ aug,
                                                                       const d2r_clip_photo_desc* __restrict__ photo, int S, int quads,
                                                                       float rescale, photo_norm nm, const float* __restrict__ ws,
                                                                       int parts, float* __restrict__ out) {
  const d2r_clip_augment_desc d = aug[blockIdx.y];   // uniform: scalar loads
  const d2r_clip_photo_desc ph = photo[blockIdx.y];
  const int t = blockIdx.x * PHOTO_BLOCK + threadIdx.x;
  if (t >= S * quads) return;
  const int i = t / quads, j0 = (t - i * quads) * 4;
  const int plane = S * S;
  float x[3][4];
  photo_resample(cache + idx[blockIdx.y] * row_bytes, d, d.flip, i, j0, S, rescale, x);
  float m = 0.0f;
  if (ph.contrast != 1.0f) {
    const float* w = ws + (int64_t)blockIdx.y * parts;
    m = w[0];
    for (int q = 1; q < parts; ++q) m += w[q];
    m = m / (float)plane;  // S * S <= 2^24 is exact
  }
  const bool erase_row = ph.ew > 0 && i >= ph.ey0 && i < ph.ey0 + ph.eh;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float r = x[0][k], g = x[1][k], b = x[2][k];
    if (ph.brightness != 1.0f) {
      r = photo_brightness(r, ph.brightness);
      g = photo_brightness(g, ph.brightness);
      b = photo_brightness(b, ph.brightness);
    }
    if (ph.contrast != 1.0f) {
      const float km = (1.0f - ph.contrast) * m;
      r = photo_clamp01(ph.contrast * r + km);
      g = photo_clamp01(ph.contrast * g + km);
      b = photo_clamp01(ph.contrast * b + km);
    }
    if (ph.saturation != 1.0f) {
      const float sg = (1.0f - ph.saturation) * photo_gray(r, g, b);
      r = photo_clamp01(ph.saturation * r + sg);
      g = photo_clamp01(ph.saturation * g + sg);
      b = photo_clamp01(ph.saturation * b + sg);
    }
    if (ph.hue != 0.0f) photo_hue(r, g, b, ph.hue);
    if (ph.gray) r = g = b = photo_gray(r, g, b);
    const bool erased = erase_row && j0 + k >= ph.ex0 && j0 + k < ph.ex0 + ph.ew;
    x[0][k] = erased ? 0.0f : (r - nm.mean[0]) / nm.std[0];
    x[1][k] = erased ? 0.0f : (g - nm.mean[1]) / nm.std[1];
    x[2][k] = erased ? 0.0f : (b - nm.mean[2]) / nm.std[2];
  }
  float* o = out + (int64_t)blockIdx.y * 3 * plane + (int64_t)i * S + j0;
  if ((S & 3) == 0 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {  // plane is a multiple of 4 then: all three channels aligned
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + (int64_t)c * plane) = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < S) o[(int64_t)c * plane + k] = x[c][k];
  }
}

// ---- K24: MixUp / CutMix of a finished pixel batch ----

// one component: the partner's value inside the box, the sample's own where a == 1, the blend otherwise
__device__ __forceinline__ float mix_pick(float own, float other, float a, bool boxed) {
#pragma clang fp contract(off)
  return boxed ? other : (a == 1.0f ? own : a * own + (1.0f - a) * other);
}

// out[b] = in[b] mixed with in[partner_b] (desc[b] = {partner, bits of a, x0, y0, w, h, 0, 0}): four consecutive columns of one row
// per thread, as in clip_cache_augment_kernel.  VEC (S a multiple of 4, in and out 16-byte aligned): one float4 load per input and
// one float4 store; a box edge inside the quad is a select per component.  The partner is read only where a != 1 or the row crosses
// the box, so an untouched sample costs one read and one write.
template <bool VEC>
__global__ __launch_bounds__(256) void image_mix_kernel(const float* __restrict__ in, float* __restrict__ out, int S, int quads,
                                                        const int32_t* __restrict__ desc) {
  const int32_t* d = desc + (int64_t)blockIdx.y * 8;  // uniform: scalar loads
  const int partner = d[0], x0 = d[2], y0 = d[3], x1 = d[2] + d[4], y1 = d[3] + d[5];
  const float a = __int_as_float(d[1]);
  const int t = blockIdx.x * 256 + threadIdx.x;  // < 3 * 4096 * 1024
  if (t >= 3 * S * quads) return;
  const int line = t / quads, j0 = (t - line * quads) * 4;
  const int i = line % S;
  const int64_t sample = (int64_t)3 * S * S, off = (int64_t)line * S + j0;
  const float* own = in + (int64_t)blockIdx.y * sample + off;
  const float* other = in + (int64_t)partner * sample + off;
  float* o = out + (int64_t)blockIdx.y * sample + off;
  const bool row_boxed = i >= y0 && i < y1 && x0 < x1;
  const bool need_other = a != 1.0f || (row_boxed && j0 < x1 && j0 + 4 > x0);
  if (VEC) {
    const float4 p = *reinterpret_cast<const float4*>(own);
    const float4 q = need_other ? *reinterpret_cast<const float4*>(other) : p;
    float4 r;
    r.x = mix_pick(p.x, q.x, a, row_boxed && j0 >= x0 && j0 < x1);
    r.y = mix_pick(p.y, q.y, a, row_boxed && j0 + 1 >= x0 && j0 + 1 < x1);
    r.z = mix_pick(p.z, q.z, a, row_boxed && j0 + 2 >= x0 && j0 + 2 < x1);
    r.w = mix_pick(p.w, q.w, a, row_boxed && j0 + 3 >= x0 && j0 + 3 < x1);
    *reinterpret_cast<float4*>(o) = r;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < S) {
        const float p = own[k];
        o[k] = mix_pick(p, need_other ? other[k] : p, a, row_boxed && j0 + k >= x0 && j0 + k < x1);
      }
  }
}

// dst[b] = src[idx[b]], rows of `elems` V-sized pieces
template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(V* __restrict__ dst, const V* __restrict__ src, int64_t elems,
                                                          const int64_t* __restrict__ idx) {
  const V* s = src + idx[blockIdx.y] * elems;
  V* d = dst + (int64_t)blockIdx.y * elems;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < elems; e += (int64_t)gridDim.x * blockDim.x) d[e] = s[e];
}

template <typename V>
int launch_gather_rows(void* dst, const void* src, int64_t row_bytes, const int64_t* idx, int B, hipStream_t st) {
  const int64_t elems = row_bytes / (int64_t)sizeof(V);
  const int block = elems <= 64 ? 64 : 256;
  const int gx = (int)std::min<int64_t>(d2r_cdiv(elems, block), 1024);
  hipLaunchKernelGGL(gather_rows_kernel<V>, dim3(gx, B), dim3(block), 0, st, (V*)dst, (const V*)src, elems, idx);
  return d2r_check_launch("d2r_gather_rows");
}

// h[0..B) inside [0, rows)
int check_rows(const char* who, const char* what, const int64_t* h, int B, int64_t rows) {
  for (int b = 0; b < B; ++b)
    D2R_REQUIRE(h[b] >= 0 && h[b] < rows, "%s: %s %d is %lld, outside the %lld rows", who, what, b, (long long)h[b], (long long)rows);
  return D2R_OK;
}

// every box inside the S x S crop, every flip 0 or 1
int check_boxes(const char* who, const d2r_clip_augment_desc* h, int B, int S) {
  for (int b = 0; b < B; ++b) {
    const d2r_clip_augment_desc& d = h[b];
    D2R_REQUIRE(d.x0 >= 0 && d.y0 >= 0 && d.w >= 1 && d.h >= 1 && d.w <= S && d.h <= S && d.x0 <= S - d.w && d.y0 <= S - d.h,
                "%s: sample %d: the %d x %d box at (%d, %d) does not lie inside the %d x %d crop", who, b, d.w, d.h, d.x0, d.y0, S, S);
    D2R_REQUIRE(d.flip == 0 || d.flip == 1, "%s: sample %d: flip is %d, not 0 or 1", who, b, d.flip);
  }
  return D2R_OK;
}

// every bound the kernels rely on, checked on the host copies; *max_rows = the largest nrows
int check_descs(const d2r_clip_image_desc* h, int B, int S, int64_t src_bytes, const int32_t* ht, int64_t tab_len, size_t ws_bytes,
                int* max_rows) {
  int64_t ws_end = 0;
  *max_rows = 0;
  for (int b = 0; b < B; ++b) {
    const d2r_clip_image_desc& d = h[b];
    D2R_REQUIRE(d.H >= 1 && d.W >= 1 && d.src_offset >= 0 && d.src_offset + (int64_t)d.H * d.W * 3 <= src_bytes,
                "d2r_clip_preprocess: image %d (%d x %d at byte %lld) lies outside the %lld source bytes", b, d.H, d.W,
                (long long)d.src_offset, (long long)src_bytes);
    D2R_REQUIRE(d.rh >= S && d.rw >= S && d.top >= 0 && d.left >= 0 && d.top + S <= d.rh && d.left + S <= d.rw,
                "d2r_clip_preprocess: image %d: the %d x %d crop at (%d, %d) does not fit the %d x %d resized image", b, S, S, d.top,
                d.left, d.rh, d.rw);
    D2R_REQUIRE(d.kx >= 1 && d.ky >= 1 && d.row0 >= 0 && d.nrows >= 1 && d.row0 + d.nrows <= d.H,
                "d2r_clip_preprocess: image %d: bad taps (%d, %d) or source rows [%d, %d)", b, d.kx, d.ky, d.row0, d.row0 + d.nrows);
    const int64_t spans[4][2] = {{d.bx, 2LL * S}, {d.cx, (int64_t)S * d.kx}, {d.by, 2LL * S}, {d.cy, (int64_t)S * d.ky}};
    for (const auto& s : spans)
      D2R_REQUIRE(s[0] >= 0 && s[0] + s[1] <= tab_len, "d2r_clip_preprocess: image %d: table span [%lld, %lld) outside %lld entries", b,
                  (long long)s[0], (long long)(s[0] + s[1]), (long long)tab_len);
    for (int j = 0; j < S; ++j) {
      const int lo = ht[d.bx + 2 * j], n = ht[d.bx + 2 * j + 1];
      D2R_REQUIRE(lo >= 0 && n >= 1 && n <= d.kx && (int64_t)lo + n <= d.W,
                  "d2r_clip_preprocess: image %d, column %d: support [%d, +%d) outside the %d columns or over %d taps", b, j, lo, n, d.W, d.kx);
    }
    for (int i = 0; i < S; ++i) {
      const int lo = ht[d.by + 2 * i], n = ht[d.by + 2 * i + 1];
      D2R_REQUIRE(lo >= d.row0 && n >= 1 && n <= d.ky && (int64_t)lo + n <= (int64_t)d.row0 + d.nrows,
                  "d2r_clip_preprocess: image %d, row %d: support [%d, +%d) outside the rows [%d, %d) or over %d taps", b, i, lo, n,
                  d.row0, d.row0 + d.nrows, d.ky);
    }
    D2R_REQUIRE(d.ws_offset >= ws_end, "d2r_clip_preprocess: image %d: workspace region overlaps the previous image's", b);
    ws_end = d.ws_offset + (int64_t)d.nrows * S * 3;
    if (ws_end > (int64_t)ws_bytes)
      return d2r_fail(D2R_ERR_WORKSPACE, "d2r_clip_preprocess: workspace of %zu bytes, image %d needs %lld", ws_bytes, b, (long long)ws_end);
    if (d.nrows > *max_rows) *max_rows = d.nrows;
  }
  return D2R_OK;
}

}  // namespace

extern "C" size_t d2r_clip_preprocess_ws_bytes(const d2r_clip_image_desc* h_desc, int B, int S) {
  int64_t end = 0;
  for (int b = 0; h_desc && b < B; ++b) {
    const int64_t e = h_desc[b].ws_offset + (int64_t)h_desc[b].nrows * S * 3;
    if (e > end) end = e;
  }
  return (size_t)end;
}

extern "C" int d2r_clip_preprocess(const uint8_t* src, int64_t src_bytes, const d2r_clip_image_desc* h_desc,
                                   const d2r_clip_image_desc* desc, int B, int S, const int32_t* h_tab, const int32_t* tab,
                                   int64_t tab_len, const float* lut, float* out, void* ws, size_t ws_bytes, void* stream) {
  D2R_REQUIRE(src && h_desc && desc && h_tab && tab && lut && out && ws, "d2r_clip_preprocess: null pointer");
  D2R_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096 && tab_len >= 0 && tab_len <= INT32_MAX,
              "d2r_clip_preprocess: bad batch %d, crop size %d or table length %lld", B, S, (long long)tab_len);
  D2R_REQUIRE((reinterpret_cast<uintptr_t>(desc) & 7u) == 0 && (reinterpret_cast<uintptr_t>(tab) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(lut) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
              "d2r_clip_preprocess: desc must be 8-byte, tab / lut / out 4-byte aligned");
  int max_rows = 0;
  if (int rc = check_descs(h_desc, B, S, src_bytes, h_tab, tab_len, ws_bytes, &max_rows)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_hpass_kernel, dim3(d2r_cdiv(max_rows, HROWS), B), dim3(256), 0, st, src, desc, tab, S, (uint8_t*)ws);
  if (int rc = d2r_check_launch("d2r_clip_preprocess (horizontal pass)")) return rc;
  hipLaunchKernelGGL(clip_vpass_kernel<false>, dim3(d2r_cdiv((int64_t)S * S, 256), B), dim3(256), 0, st, desc, tab,
                     (const uint8_t*)ws, lut, S, out, (uint8_t*)nullptr, (const int64_t*)nullptr, (int64_t)0);
  return d2r_check_launch("d2r_clip_preprocess (vertical pass)");
}

extern "C" size_t d2r_clip_cache_row_bytes(int S) { return S < 1 ? 0 : ((size_t)3 * S * S + 15) / 16 * 16; }

extern "C" int d2r_clip_preprocess_u8(const uint8_t* src, int64_t src_bytes, const d2r_clip_image_desc* h_desc,
                                      const d2r_clip_image_desc* desc, int B, int S, const int32_t* h_tab, const int32_t* tab,
                                      int64_t tab_len, uint8_t* cache, int64_t cache_rows, const int64_t* h_slots, const int64_t* slots,
                                      void* ws, size_t ws_bytes, void* stream) {
  D2R_REQUIRE(src && h_desc && desc && h_tab && tab && cache && h_slots && slots && ws, "d2r_clip_preprocess_u8: null pointer");
  D2R_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096 && tab_len >= 0 && tab_len <= INT32_MAX && cache_rows >= 1,
              "d2r_clip_preprocess_u8: bad batch %d, crop size %d, table length %lld or %lld cache rows", B, S, (long long)tab_len,
              (long long)cache_rows);
  D2R_REQUIRE((reinterpret_cast<uintptr_t>(desc) & 7u) == 0 && (reinterpret_cast<uintptr_t>(tab) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(slots) & 7u) == 0,
              "d2r_clip_preprocess_u8: desc / slots must be 8-byte, tab 4-byte aligned");
  if (int rc = check_rows("d2r_clip_preprocess_u8", "slot", h_slots, B, cache_rows)) return rc;
  std::vector<int64_t> sorted(h_slots, h_slots + B);
  std::sort(sorted.begin(), sorted.end());
  for (int b = 1; b < B; ++b)
    D2R_REQUIRE(sorted[b] != sorted[b - 1], "d2r_clip_preprocess_u8: slot %lld is named twice in one call", (long long)sorted[b]);
  int max_rows = 0;
  if (int rc = check_descs(h_desc, B, S, src_bytes, h_tab, tab_len, ws_bytes, &max_rows)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(clip_hpass_kernel, dim3(d2r_cdiv(max_rows, HROWS), B), dim3(256), 0, st, src, desc, tab, S, (uint8_t*)ws);
  if (int rc = d2r_check_launch("d2r_clip_preprocess_u8 (horizontal pass)")) return rc;
  hipLaunchKernelGGL(clip_vpass_kernel<true>, dim3(d2r_cdiv((int64_t)S * S, 256), B), dim3(256), 0, st, desc, tab, (const uint8_t*)ws,
                     (const float*)nullptr, S, (float*)nullptr, cache, slots, (int64_t)d2r_clip_cache_row_bytes(S));
  return d2r_check_launch("d2r_clip_preprocess_u8 (vertical pass)");
}

extern "C" int d2r_clip_cache_gather(const uint8_t* cache, int64_t cache_rows, const int64_t* h_idx, const int64_t* idx, int B, int S,
                                     const float* lut, float* out, void* stream) {
  D2R_REQUIRE(cache && h_idx && idx && lut && out, "d2r_clip_cache_gather: null pointer");
  D2R_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096 && cache_rows >= 1, "d2r_clip_cache_gather: bad batch %d, crop size %d or %lld cache rows",
              B, S, (long long)cache_rows);
  D2R_REQUIRE(d2r_aligned16(cache) && (reinterpret_cast<uintptr_t>(idx) & 7u) == 0 && (reinterpret_cast<uintptr_t>(lut) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
              "d2r_clip_cache_gather: cache must be 16-byte, idx 8-byte, lut / out 4-byte aligned");
  if (int rc = check_rows("d2r_clip_cache_gather", "index", h_idx, B, cache_rows)) return rc;
  const int64_t row_bytes = (int64_t)d2r_clip_cache_row_bytes(S);
  hipLaunchKernelGGL(clip_cache_gather_kernel, dim3(d2r_cdiv(row_bytes / 16, 256), B), dim3(256), 0, (hipStream_t)stream, cache, row_bytes,
                     idx, S, lut, out);
  return d2r_check_launch("d2r_clip_cache_gather");
}

extern "C" int d2r_clip_cache_augment(const uint8_t* cache, int64_t cache_rows, const int64_t* h_idx, const int64_t* idx,
                                      const d2r_clip_augment_desc* h_aug, const d2r_clip_augment_desc* aug, int B, int S,
                                      const float* lut, float* out, void* stream) {
  D2R_REQUIRE(cache && h_idx && idx && h_aug && aug && lut && out, "d2r_clip_cache_augment: null pointer");
  D2R_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096 && cache_rows >= 1, "d2r_clip_cache_augment: bad batch %d, crop size %d or %lld cache rows",
              B, S, (long long)cache_rows);
  D2R_REQUIRE(d2r_aligned16(cache) && (reinterpret_cast<uintptr_t>(idx) & 7u) == 0 && (reinterpret_cast<uintptr_t>(aug) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(lut) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
              "d2r_clip_cache_augment: cache must be 16-byte, idx 8-byte, aug / lut / out 4-byte aligned");
  if (int rc = check_rows("d2r_clip_cache_augment", "index", h_idx, B, cache_rows)) return rc;
  if (int rc = check_boxes("d2r_clip_cache_augment", h_aug, B, S)) return rc;
  const int quads = (S + 3) / 4;
  hipLaunchKernelGGL(clip_cache_augment_kernel, dim3(d2r_cdiv((int64_t)3 * S * quads, 256), B), dim3(256), 0, (hipStream_t)stream, cache,
                     (int64_t)d2r_clip_cache_row_bytes(S), idx, aug, S, quads, lut, out);
  return d2r_check_launch("d2r_clip_cache_augment");
}

// partial sums per sample of the statistics pass: one per workgroup of PHOTO_BLOCK pixel quads
static int photo_parts(int S) { return d2r_cdiv((int64_t)S * ((S + 3) / 4), PHOTO_BLOCK); }

extern "C" size_t d2r_clip_cache_augment_photo_ws_bytes(int B, int S) {
  return B < 1 || S < 1 || S > 4096 ? 0 : (size_t)B * photo_parts(S) * sizeof(float);
}

extern "C" int d2r_clip_cache_augment_photo(const uint8_t* cache, int64_t cache_rows, const int64_t* h_idx, const int64_t* idx,
                                            const d2r_clip_augment_desc* h_aug, const d2r_clip_augment_desc* aug,
                                            const d2r_clip_photo_desc* h_photo, const d2r_clip_photo_desc* photo, int B, int S,
                                            const float* h_norm, float rescale, float* out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "d2r_clip_cache_augment_photo";
  D2R_REQUIRE(cache && h_idx && idx && h_aug && aug && h_photo && photo && h_norm && out && ws, "%s: null pointer", who);
  D2R_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096 && cache_rows >= 1, "%s: bad batch %d, crop size %d or %lld cache rows", who, B, S,
              (long long)cache_rows);
  D2R_REQUIRE(d2r_aligned16(cache) && (reinterpret_cast<uintptr_t>(idx) & 7u) == 0 && (reinterpret_cast<uintptr_t>(aug) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(photo) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(ws) & 3u) == 0,
              "%s: cache must be 16-byte, idx 8-byte, aug / photo / out / ws 4-byte aligned", who);
  photo_norm nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = h_norm[c];
    nm.std[c] = h_norm[3 + c];
    D2R_REQUIRE(std::isfinite(nm.mean[c]) && std::isfinite(nm.std[c]) && nm.std[c] > 0.0f, "%s: channel %d: mean %g, std %g (finite, std > 0)",
                who, c, (double)nm.mean[c], (double)nm.std[c]);
  }
  D2R_REQUIRE(std::isfinite(rescale) && rescale > 0.0f, "%s: rescale is %g, not finite and > 0", who, (double)rescale);
  if (int rc = check_rows(who, "index", h_idx, B, cache_rows)) return rc;
  if (int rc = check_boxes(who, h_aug, B, S)) return rc;
  bool stats = false;
  for (int b = 0; b < B; ++b) {
    const d2r_clip_photo_desc& p = h_photo[b];
    const float f[3] = {p.brightness, p.contrast, p.saturation};
    for (int k = 0; k < 3; ++k)
      D2R_REQUIRE(std::isfinite(f[k]) && f[k] >= 0.0f, "%s: sample %d: %s factor %g is not finite and >= 0", who, b,
                  k == 0 ? "brightness" : (k == 1 ? "contrast" : "saturation"), (double)f[k]);
    D2R_REQUIRE(std::fabs(p.hue) <= 0.5f, "%s: sample %d: hue shift %g is outside [-0.5, 0.5]", who, b, (double)p.hue);
    D2R_REQUIRE(p.gray == 0 || p.gray == 1, "%s: sample %d: gray is %d, not 0 or 1", who, b, p.gray);
    D2R_REQUIRE(p.ew == 0 || (p.ex0 >= 0 && p.ey0 >= 0 && p.ew >= 1 && p.eh >= 1 && p.ew <= S && p.eh <= S && p.ex0 <= S - p.ew &&
                              p.ey0 <= S - p.eh),
                "%s: sample %d: the %d x %d erase box at (%d, %d) is neither empty (ew = 0) nor inside the %d x %d output", who, b, p.ew,
                p.eh, p.ex0, p.ey0, S, S);
    D2R_REQUIRE(p.reserved[0] == 0 && p.reserved[1] == 0 && p.reserved[2] == 0, "%s: sample %d: reserved fields must be zero", who, b);
    stats = stats || p.contrast != 1.0f;
  }
  const size_t need = d2r_clip_cache_augment_photo_ws_bytes(B, S);
  if (ws_bytes < need) return d2r_fail(D2R_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
  const int quads = (S + 3) / 4, parts = photo_parts(S);
  const int64_t row_bytes = (int64_t)d2r_clip_cache_row_bytes(S);
  hipStream_t st = (hipStream_t)stream;
  if (stats) {  // only when some sample's contrast factor is not 1
    hipLaunchKernelGGL(clip_photo_stats_kernel, dim3(parts, B), dim3(PHOTO_BLOCK), 0, st, cache, row_bytes, idx, aug, photo, S, quads,
                       rescale, (float*)ws);
    if (int rc = d2r_check_launch("d2r_clip_cache_augment_photo (statistics pass)")) return rc;
  }
  hipLaunchKernelGGL(clip_photo_apply_kernel, dim3(parts, B), dim3(PHOTO_BLOCK), 0, st, cache, row_bytes, idx, aug, photo, S, quads,
                     rescale, nm, (const float*)ws, parts, out);
  return d2r_check_launch("d2r_clip_cache_augment_photo");
}

extern "C" int d2r_image_mix(const float* in, float* out, int B, int S, const int32_t* h_desc, const int32_t* desc, void* stream) {
  const char* who = "d2r_image_mix";
  D2R_REQUIRE(in && out && h_desc && desc, "%s: null pointer", who);
  D2R_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 4096, "%s: bad batch %d or crop size %d", who, B, S);
  const uintptr_t pi = reinterpret_cast<uintptr_t>(in), po = reinterpret_cast<uintptr_t>(out);
  D2R_REQUIRE(((pi | po | reinterpret_cast<uintptr_t>(desc)) & 3u) == 0, "%s: in / out / desc must be 4-byte aligned", who);
  const uintptr_t bytes = (uintptr_t)B * 3 * S * S * sizeof(float);
  D2R_REQUIRE(po >= pi + bytes || pi >= po + bytes, "%s: out overlaps in (sample b reads its partner: the call cannot run in place)", who);
  for (int b = 0; b < B; ++b) {
    const int32_t* d = h_desc + (size_t)b * 8;
    float a;
    std::memcpy(&a, d + 1, sizeof a);
    D2R_REQUIRE(d[0] >= 0 && d[0] < B, "%s: sample %d: partner is %d, outside the %d samples", who, b, d[0], B);
    D2R_REQUIRE(std::isfinite(a) && a >= 0.0f && a <= 1.0f, "%s: sample %d: a is %g, not a finite value in [0, 1]", who, b, (double)a);
    D2R_REQUIRE(d[4] >= 0 && d[5] >= 0, "%s: sample %d: w is %d and h is %d, negative", who, b, d[4], d[5]);
    D2R_REQUIRE(d[2] >= 0 && d[3] >= 0 && d[4] <= S && d[5] <= S && d[2] <= S - d[4] && d[3] <= S - d[5],
                "%s: sample %d: the %d x %d box at (%d, %d) does not lie inside [0, %d] x [0, %d]", who, b, d[4], d[5], d[2], d[3], S, S);
  }
  const int quads = (S + 3) / 4;
  const dim3 grid(d2r_cdiv((int64_t)3 * S * quads, 256), B);
  if ((S & 3) == 0 && ((pi | po) & 15u) == 0)
    hipLaunchKernelGGL(image_mix_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, out, S, quads, desc);
  else
    hipLaunchKernelGGL(image_mix_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, out, S, quads, desc);
  return d2r_check_launch("d2r_image_mix");
}

extern "C" int d2r_gather_rows(void* dst, const void* src, int64_t src_rows, int64_t row_bytes, const int64_t* h_idx, const int64_t* idx,
                               int B, void* stream) {
  D2R_REQUIRE(dst && src && h_idx && idx, "d2r_gather_rows: null pointer");
  D2R_REQUIRE(B >= 1 && B <= 65535 && src_rows >= 1 && row_bytes >= 1, "d2r_gather_rows: bad batch %d, %lld source rows or %lld bytes per row", B,
              (long long)src_rows, (long long)row_bytes);
  D2R_REQUIRE((reinterpret_cast<uintptr_t>(idx) & 7u) == 0, "d2r_gather_rows: idx must be 8-byte aligned");
  if (int rc = check_rows("d2r_gather_rows", "index", h_idx, B, src_rows)) return rc;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src) | (uintptr_t)row_bytes;
  hipStream_t st = (hipStream_t)stream;
  if ((bits & 15u) == 0) return launch_gather_rows<uint4>(dst, src, row_bytes, idx, B, st);
  if ((bits & 7u) == 0) return launch_gather_rows<uint2>(dst, src, row_bytes, idx, B, st);
  if ((bits & 3u) == 0) return launch_gather_rows<uint32_t>(dst, src, row_bytes, idx, B, st);
  return launch_gather_rows<uint8_t>(dst, src, row_bytes, idx, B, st);
}
