// jpeg.hip — baseline JPEG decoding of a batch of images (processor/dataset.py:89, Image.open(p).convert("RGB")), bit-identical to
// libjpeg-turbo's default path as Pillow calls it.  The host (d2r_amd/jpeg.py) has parsed the markers, removed byte stuffing and
// split the scan into restart segments; six launches on the caller's stream do the rest, with no host read-back between them:
//
//   1. jpeg_sync_kernel     — self-synchronising parallel Huffman decoding (Weißenberger & Schmidt, ICPP 2018 / HiPC 2021).  Each
//      lane owns a chunk of D2R_JPEG_CHUNK_BITS bits of one segment and decodes it from a guessed state to the first symbol boundary
//      at or past the chunk's end.  The guess: start WARM chunks earlier (bit position = that chunk's start, first block of an MCU,
//      DC coefficient next) and decode up to the own chunk's start; a wrong start usually falls into step within a few MCUs.  The state there is
//      (bit position, block within the MCU, coefficient index).  In rounds separated by barriers, a lane whose start state differs
//      from its left neighbour's end state (in LDS) decodes again from that state, until no lane changes.  A segment's first chunk
//      starts from the true state, so after round r the first r chunks of a segment are right: at worst the rounds are serial.
//   2. jpeg_boundary_kernel — one lane per segment walks the workgroup boundaries inside its segment in order and decodes chunks
//      again, one by one, until a chunk's start state equals its left neighbour's end state (the chunks after it were synchronised
//      to it in pass 1).  No workgroup waits for another; the result does not depend on dispatch order.
//   3. jpeg_scan_kernel     — per image, segmented exclusive scans over the chunks (reset at every segment: restart intervals are
//      independent) of the blocks each chunk finished and of its DC differences per component: each chunk's first block index
//      and DC predictors.
//   4. jpeg_write_kernel    — every chunk decodes once more from its final state and writes its coefficients (natural order,
//      int16 as libjpeg's JCOEF) into the zeroed coefficient planes, and flags malformed data in the image's status.
//   5. jpeg_idct_kernel     — dequantisation and jpeg_idct_islow per 8 x 8 block (13-bit constants, 2 pass-1 bits, the 10-bit
//      wrap-around of the range-limit table) into uint8 component planes.
//   6. jpeg_color_kernel    — fancy h2v1 / h2v2 upsampling (jdsample.c, edge samples replicated as the context rows do; plain
//      replication when a chroma plane is at most 2 samples wide) and ycc_rgb_convert's fixed-point tables, into HWC RGB.
//
// Malformed entropy data never moves a read or a write outside its buffers: the bit reader returns zeros past a segment's padded
// end, table lookups are masked, coefficients past the 64th go to position 63 (libjpeg's jpeg_natural_order padding), and only
// blocks below the segment's block count are written; blocks a segment's data does not reach stay zero.  A bad code reads as symbol
// 0 after 17 bits, as in libjpeg's jpeg_huff_decode, and decoding goes on: it must not stop a chain, or a wrong guess that meets
// one would pass its error on to every later chunk, one round at a time.
#include "common.h"

namespace {

constexpr int CB = D2R_JPEG_CHUNK_BITS;
constexpr int HI = D2R_JPEG_HUFF_INTS;
constexpr int NT = 256;                  // chunks per workgroup of passes 1 and 4
constexpr int LOOK = 9;
constexpr int WARM = 4;                  // chunks a pass-1 lane decodes before its own to improve its guess

struct Rec {                             // 48 bytes per chunk at ws_rec
  int st_pos, st_bk, en_pos, en_bk;      // start / end state: bit position, (block in MCU << 8) | coefficient index
  int done;                              // blocks finished in the chunk
  int dc[3];                             // sum of the DC differences per component
  int blk0;                              // (pass 3) index of the block at the chunk's start within its segment
  int pred[3];                           // (pass 3) DC predictors at the chunk's start
};
static_assert(sizeof(Rec) == 48, "Rec layout");

__constant__ uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Bits {  // big-endian bit reader over a segment's 32-bit words; words at or past nw read as zero
  const uint32_t* w;
  int nw, widx, nb;
  uint64_t buf;
  __device__ __forceinline__ uint32_t word(int i) const { return i < nw ? __builtin_bswap32(w[i]) : 0u; }
  __device__ __forceinline__ void seek(int pos) {
    widx = pos >> 5;
    buf = ((uint64_t)word(widx) << 32) << (pos & 31);
    nb = 32 - (pos & 31);
    ++widx;
  }
  __device__ __forceinline__ uint32_t peek() {  // the next 32 bits; afterwards nb >= 32
    if (nb < 32) {
      buf |= (uint64_t)word(widx++) << (32 - nb);
      nb += 32;
    }
    return (uint32_t)(buf >> 32);
  }
  __device__ __forceinline__ void skip(int n) {
    buf <<= n;
    nb -= n;
  }
};

// one Huffman symbol from the 32 bits `w`: false if no code of at most 16 bits matches (then, as libjpeg's jpeg_huff_decode, the
// symbol reads as 0 after 17 bits)
__device__ __forceinline__ bool huff(const int* t, uint32_t w, int& len, int& sym) {
  const int e = t[w >> (32 - LOOK)];
  if (e >> 8) {
    len = (e >> 8) & 15;
    sym = e & 255;
    return true;
  }
  for (int l = LOOK + 1; l <= 16; ++l) {
    const int code = (int)(w >> (32 - l));
    if (code <= t[512 + l]) {
      len = l;
      sym = t[546 + ((code + t[529 + l]) & 255)];
      return true;
    }
  }
  len = 17;
  sym = 0;
  return false;
}

struct Seg {
  int idx, bits, chunk0, nchunk;
  const uint32_t* words;
  int nw;
};

__device__ __forceinline__ Seg find_seg(const d2r_jpeg_image_desc& d, const d2r_jpeg_segment* __restrict__ seg, const uint8_t* data, int c) {
  int lo = 0, hi = d.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[d.seg0 + mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  const d2r_jpeg_segment s = seg[d.seg0 + lo];
  const int next = lo + 1 < d.nseg ? seg[d.seg0 + lo + 1].chunk0 : d.nchunk;
  return Seg{lo, s.bits, s.chunk0, next - s.chunk0, reinterpret_cast<const uint32_t*>(data + s.offset),
             (int)(((int64_t)(s.bits + 7) / 8 + D2R_JPEG_SEG_PAD) / 4)};
}

// the image's Huffman tables (DC of components 0..2, then AC) and MCU map in LDS
struct Lds {
  int tab[6 * HI];
  int map[10];
  int64_t coef_off[3];
};

__device__ void load_tables(Lds& L, const d2r_jpeg_image_desc& d, const int32_t* __restrict__ tab) {
  for (int i = threadIdx.x; i < 6 * HI; i += blockDim.x) {
    const int which = i / HI, c = which % 3;
    L.tab[i] = c < d.ncomp ? tab[(which < 3 ? d.dc[c] : d.ac[c]) + i % HI] : 0;
  }
  if (threadIdx.x < 10) L.map[threadIdx.x] = d.mcu_map[threadIdx.x];
  if (threadIdx.x == 0) {
    int64_t o = 0;
    for (int c = 0; c < 3; ++c) {
      L.coef_off[c] = o;
      if (c < d.ncomp) o += (int64_t)d.bw[c] * d.bh[c] * 64;
    }
  }
}

struct Acc {
  int done;
  int dc[3];
  int status;
};

// Decodes one chunk from state (pos, bk) up to the first symbol boundary at or past cend.  WRITE: g = index of the block at the
// start, pred = DC predictors; blocks g < gend are written to coef and malformed data is flagged in acc.status.
template <bool WRITE>
__device__ void decode_chunk(const Lds& L, const d2r_jpeg_image_desc& d, const Seg& s, int& pos, int& bk, int cend, Acc& acc,
                             int g = 0, int gend = 0, int* pred = nullptr, int mcu0 = 0, int16_t* coef = nullptr) {
  acc.done = acc.dc[0] = acc.dc[1] = acc.dc[2] = acc.status = 0;
  if (pos >= cend) return;
  Bits br;
  br.w = s.words;
  br.nw = s.nw;
  br.seek(pos);
  int blk = (bk >> 8) & 15, k = bk & 255;
  if (blk >= d.mcu_blocks) blk = 0;  // only a corrupt guess can get here
  int16_t* bp = nullptr;
  auto block_ptr = [&](int gi) -> int16_t* {
    const int mcu = mcu0 + gi / d.mcu_blocks, m = L.map[gi % d.mcu_blocks];
    const int c = m & 3, my = mcu / d.mcux, mx = mcu - my * d.mcux;
    const int by = my * d.v[c] + ((m >> 8) & 15), bx = mx * d.h[c] + ((m >> 4) & 15);
    return coef + L.coef_off[c] + ((int64_t)by * d.bw[c] + bx) * 64;
  };
  if (WRITE && g < gend) bp = block_ptr(g);
  while (pos < cend) {
    if (WRITE && g >= gend) break;
    const int comp = L.map[blk] & 3;
    const uint32_t w = br.peek();
    int len, sym;
    if (!huff(L.tab + (k == 0 ? comp : 3 + comp) * HI, w, len, sym) && WRITE) acc.status |= D2R_JPEG_BAD_CODE;
    const int sz = sym & 15, r = k == 0 ? 0 : sym >> 4;
    int v = 0;
    if (sz) {
      const uint32_t x = (w << len) >> (32 - sz);
      v = x < (1u << (sz - 1)) ? (int)x - (1 << sz) + 1 : (int)x;
    }
    br.skip(len + sz);
    pos += len + sz;
    if (WRITE && pos > s.bits) acc.status |= D2R_JPEG_SHORT;
    if (k == 0) {
      acc.dc[comp] = (int)((unsigned)acc.dc[comp] + (unsigned)v);
      if (WRITE) {
        pred[comp] = (int)((unsigned)pred[comp] + (unsigned)v);
        bp[0] = (int16_t)pred[comp];
      }
      k = 1;
    } else if (sz) {
      k += r;
      if (k > 63) {
        if (WRITE) acc.status |= D2R_JPEG_BAD_RUN;
        k = 63;  // libjpeg: jpeg_natural_order[64..79] == 63
      }
      if (WRITE) bp[kNatural[k]] = (int16_t)v;
      k += 1;
    } else if (r == 15) {
      k += 16;
    } else {
      k = 64;  // end of block
    }
    if (k >= 64) {
      k = 0;
      blk = blk + 1 == d.mcu_blocks ? 0 : blk + 1;
      ++acc.done;
      if (WRITE && ++g < gend) bp = block_ptr(g);
    }
  }
  bk = (blk << 8) | k;
}

__device__ __forceinline__ Rec* recs(uint8_t* ws, const d2r_jpeg_image_desc& d) { return reinterpret_cast<Rec*>(ws + d.ws_rec); }

// pass 1: decode every chunk from a guess and synchronise the chunks of a workgroup through LDS
__global__ __launch_bounds__(NT) void jpeg_sync_kernel(const uint8_t* __restrict__ data, const d2r_jpeg_image_desc* __restrict__ desc,
                                                       const d2r_jpeg_segment* __restrict__ seg, const int32_t* __restrict__ tab,
                                                       uint8_t* __restrict__ ws, int32_t* __restrict__ stats) {
  __shared__ Lds L;
  __shared__ int e_pos[NT], e_bk[NT];
  const d2r_jpeg_image_desc& d = desc[blockIdx.y];
  if ((int)blockIdx.x * NT >= d.nchunk) return;
  load_tables(L, d, tab);
  __syncthreads();
  const int c = blockIdx.x * NT + threadIdx.x;
  const bool valid = c < d.nchunk;
  Seg s{};
  int st_pos = 0, st_bk = 0, pos = 0, bk = 0, cend = 0;
  bool first = true;
  Acc acc{};
  if (valid) {
    s = find_seg(d, seg, data, c);
    first = c == s.chunk0;
    // the guess: decode from WARM chunks earlier (or the segment's start) up to this chunk's start, so that the guessed chain has
    // had time to fall into step with the true one (position, block in the MCU, coefficient index)
    const int w0 = max(s.chunk0, c - WARM);
    pos = (w0 - s.chunk0) * CB;
    if (w0 < c) decode_chunk<false>(L, d, s, pos, bk, (c - s.chunk0) * CB, acc);
    st_pos = pos;
    st_bk = bk;
    cend = min((c - s.chunk0 + 1) * CB, s.bits);
    decode_chunk<false>(L, d, s, pos, bk, cend, acc);
  }
  int rounds = 1;
  for (;;) {
    e_pos[threadIdx.x] = pos;
    e_bk[threadIdx.x] = bk;
    __syncthreads();
    bool redo = false;
    if (valid && !first && threadIdx.x > 0 && (e_pos[threadIdx.x - 1] != st_pos || e_bk[threadIdx.x - 1] != st_bk)) {
      st_pos = pos = e_pos[threadIdx.x - 1];
      st_bk = bk = e_bk[threadIdx.x - 1];
      redo = true;
    }
    if (!__syncthreads_or(redo)) break;
    if (redo) decode_chunk<false>(L, d, s, pos, bk, cend, acc);
    ++rounds;
  }
  if (valid) {
    Rec& r = recs(ws, d)[c];
    r.st_pos = st_pos;
    r.st_bk = st_bk;
    r.en_pos = pos;
    r.en_bk = bk;
    r.done = acc.done;
    r.dc[0] = acc.dc[0];
    r.dc[1] = acc.dc[1];
    r.dc[2] = acc.dc[2];
  }
  if (stats && threadIdx.x == 0) atomicMax(stats + 2 * blockIdx.y, rounds);
}

// pass 2: per segment, repair the chunks after each workgroup boundary, serially, until they agree with pass 1
__global__ __launch_bounds__(64) void jpeg_boundary_kernel(const uint8_t* __restrict__ data, const d2r_jpeg_image_desc* __restrict__ desc,
                                                           const d2r_jpeg_segment* __restrict__ seg, const int32_t* __restrict__ tab,
                                                           uint8_t* __restrict__ ws, int32_t* __restrict__ stats) {
  __shared__ Lds L;
  const d2r_jpeg_image_desc& d = desc[blockIdx.x];
  if (d.nchunk <= NT) return;  // one workgroup per image in pass 1: nothing to repair
  load_tables(L, d, tab);
  __syncthreads();
  Rec* rec = recs(ws, d);
  int redone = 0;
  for (int si = threadIdx.x; si < d.nseg; si += 64) {
    const d2r_jpeg_segment sg = seg[d.seg0 + si];
    const Seg s = find_seg(d, seg, data, sg.chunk0);
    const int end = s.chunk0 + s.nchunk;
    for (int c = (s.chunk0 / NT + 1) * NT; c < end; c += NT) {
      int pos = rec[c - 1].en_pos, bk = rec[c - 1].en_bk;
      for (int cur = c; cur < end && (pos != rec[cur].st_pos || bk != rec[cur].st_bk); ++cur) {
        Rec& r = rec[cur];
        r.st_pos = pos;
        r.st_bk = bk;
        Acc acc;
        decode_chunk<false>(L, d, s, pos, bk, min((cur - s.chunk0 + 1) * CB, s.bits), acc);
        r.en_pos = pos;
        r.en_bk = bk;
        r.done = acc.done;
        r.dc[0] = acc.dc[0];
        r.dc[1] = acc.dc[1];
        r.dc[2] = acc.dc[2];
        ++redone;
      }
    }
  }
  if (stats && redone) atomicAdd(stats + 2 * blockIdx.x + 1, redone);
}

// pass 3: per image, segmented exclusive scans of (done, dc[0..2]) over its chunks
__global__ __launch_bounds__(NT) void jpeg_scan_kernel(const uint8_t* __restrict__ data, const d2r_jpeg_image_desc* __restrict__ desc,
                                                       const d2r_jpeg_segment* __restrict__ seg, uint8_t* __restrict__ ws) {
  __shared__ unsigned v[4][NT];
  __shared__ int f[NT];
  __shared__ unsigned carry[4];
  const d2r_jpeg_image_desc& d = desc[blockIdx.x];
  Rec* rec = recs(ws, d);
  const int t = threadIdx.x;
  if (t < 4) carry[t] = 0;
  for (int base = 0; base < d.nchunk; base += NT) {
    const int c = base + t;
    unsigned own[4] = {0, 0, 0, 0};
    int flag = 1;
    if (c < d.nchunk) {
      const Rec& r = rec[c];
      own[0] = (unsigned)r.done;
      own[1] = (unsigned)r.dc[0];
      own[2] = (unsigned)r.dc[1];
      own[3] = (unsigned)r.dc[2];
      flag = find_seg(d, seg, data, c).chunk0 == c;
    }
    unsigned acc[4] = {own[0], own[1], own[2], own[3]};
    int fl = flag;
    for (int off = 1; off < NT; off <<= 1) {
      __syncthreads();
      for (int j = 0; j < 4; ++j) v[j][t] = acc[j];
      f[t] = fl;
      __syncthreads();
      if (t >= off) {
        if (!fl)
          for (int j = 0; j < 4; ++j) acc[j] += v[j][t - off];
        fl |= f[t - off];
      }
    }
    if (c < d.nchunk) {
      Rec& r = rec[c];
      unsigned ex[4];
      for (int j = 0; j < 4; ++j) ex[j] = flag ? 0u : acc[j] - own[j] + (fl ? 0u : carry[j]);
      r.blk0 = (int)ex[0];
      r.pred[0] = (int)ex[1];
      r.pred[1] = (int)ex[2];
      r.pred[2] = (int)ex[3];
    }
    __syncthreads();
    if (t == NT - 1)
      for (int j = 0; j < 4; ++j) carry[j] = fl ? acc[j] : carry[j] + acc[j];
    __syncthreads();
  }
}

// pass 4: decode every chunk from its synchronised state and write its coefficients
__global__ __launch_bounds__(NT) void jpeg_write_kernel(const uint8_t* __restrict__ data, const d2r_jpeg_image_desc* __restrict__ desc,
                                                        const d2r_jpeg_segment* __restrict__ seg, const int32_t* __restrict__ tab,
                                                        uint8_t* __restrict__ ws, int32_t* __restrict__ status) {
  __shared__ Lds L;
  const d2r_jpeg_image_desc& d = desc[blockIdx.y];
  if ((int)blockIdx.x * NT >= d.nchunk) return;
  load_tables(L, d, tab);
  __syncthreads();
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= d.nchunk) return;
  const Seg s = find_seg(d, seg, data, c);
  const Rec r = recs(ws, d)[c];
  const int total = d.mcux * d.mcuy;
  const int mcu0 = d.restart ? s.idx * d.restart : 0;
  const int gend = (d.restart ? min(d.restart, total - mcu0) : total) * d.mcu_blocks;
  int pos = r.st_pos, bk = r.st_bk, pred[3] = {r.pred[0], r.pred[1], r.pred[2]};
  Acc acc;
  decode_chunk<true>(L, d, s, pos, bk, min((c - s.chunk0 + 1) * CB, s.bits), acc, r.blk0, gend, pred, mcu0,
                     reinterpret_cast<int16_t*>(ws + d.ws_coef));
  int st = acc.status;
  if (c == s.chunk0 + s.nchunk - 1 && r.blk0 + acc.done < gend) st |= D2R_JPEG_SHORT;
  if (st) atomicOr(status + blockIdx.y, st);
}

// jpeg_idct_islow's 1-D butterfly (jidctint.c) in 64-bit arithmetic, as the C code's JLONG: in[0..7] -> out[0..7] descaled by
// `shift` and cast to int as the C code stores them (its workspace is int)
__device__ __forceinline__ int descale(int64_t x, int n) { return (int)((x + ((int64_t)1 << (n - 1))) >> n); }

__device__ __forceinline__ void islow_1d(const int* in, int* out, int shift) {
  int64_t z2 = in[2], z3 = in[6];
  int64_t z1 = (z2 + z3) * 4433;
  int64_t tmp2 = z1 + z3 * -15137;
  int64_t tmp3 = z1 + z2 * 6270;
  int64_t tmp0 = ((int64_t)in[0] + in[4]) * 8192;  // LEFT_SHIFT(z2 + z3, CONST_BITS)
  int64_t tmp1 = ((int64_t)in[0] - in[4]) * 8192;
  const int64_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int64_t z4 = tmp1 + tmp3;
  const int64_t z5 = (z3 + z4) * 9633;
  tmp0 *= 2446;
  tmp1 *= 16819;
  tmp2 *= 25172;
  tmp3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = descale(t10 + tmp3, shift);
  out[7] = descale(t10 - tmp3, shift);
  out[1] = descale(t11 + tmp2, shift);
  out[6] = descale(t11 - tmp2, shift);
  out[2] = descale(t12 + tmp1, shift);
  out[5] = descale(t12 - tmp1, shift);
  out[3] = descale(t13 + tmp0, shift);
  out[4] = descale(t13 - tmp0, shift);
}

__device__ __forceinline__ uint32_t range_limit(int x) {  // libjpeg's idct range-limit table: a 10-bit wrap, then the clamp
  int v = x & 1023;
  v = (v >= 512 ? v - 1024 : v) + 128;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// pass 5: one lane per 8 x 8 block of any component
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const d2r_jpeg_image_desc* __restrict__ desc, const int32_t* __restrict__ tab,
                                                        uint8_t* __restrict__ ws) {
  __shared__ int q[3][64];
  const d2r_jpeg_image_desc& d = desc[blockIdx.y];
  for (int i = threadIdx.x; i < 3 * 64; i += 256) q[i / 64][i % 64] = i / 64 < d.ncomp ? tab[d.qt[i / 64] + i % 64] : 0;
  __syncthreads();
  int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, poff = 0;
  int c = 0;
  for (; c < d.ncomp; ++c) {
    const int64_t n = (int64_t)d.bw[c] * d.bh[c];
    if (j < n) break;
    j -= n;
    poff += n * 64;
  }
  if (c >= d.ncomp) return;
  const int by = (int)(j / d.bw[c]), bx = (int)(j - (int64_t)by * d.bw[c]);
  const int16_t* in = reinterpret_cast<const int16_t*>(ws + d.ws_coef) + (poff + j * 64);
  int x[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const Pack<int16_t, 8> p = ld_pack<int16_t, 8>(in + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[i * 8 + e] = (int)p.v[e] * q[c][i * 8 + e];
  }
  int wsp[64];
#pragma unroll
  for (int col = 0; col < 8; ++col) {  // pass 1: columns
    int a[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) a[r] = x[r * 8 + col];
    islow_1d(a, o, 13 - 2);
#pragma unroll
    for (int r = 0; r < 8; ++r) wsp[r * 8 + col] = o[r];
  }
  const int64_t pitch = (int64_t)d.bw[c] * 8;
  uint8_t* out = ws + d.ws_plane + poff + (int64_t)by * 8 * pitch + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {  // pass 2: rows
    int o[8];
    islow_1d(wsp + r * 8, o, 13 + 2 + 3);
    uint2 pk;
    pk.x = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
    pk.y = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
    *reinterpret_cast<uint2*>(out + r * pitch) = pk;
  }
}

// pass 6: one lane per output pixel
__global__ __launch_bounds__(256) void jpeg_color_kernel(const d2r_jpeg_image_desc* __restrict__ desc, const uint8_t* __restrict__ ws,
                                                         uint8_t* __restrict__ dst) {
  const d2r_jpeg_image_desc& d = desc[blockIdx.y];
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)d.H * d.W) return;
  const int y = (int)(idx / d.W), x = (int)(idx - (int64_t)y * d.W);
  const uint8_t* py = ws + d.ws_plane;
  const int64_t p0 = (int64_t)d.bw[0] * 8;
  uint8_t* o = dst + d.dst_offset + idx * 3;
  const int Y = py[y * p0 + x];
  if (d.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)Y;
    return;
  }
  const int64_t p1 = (int64_t)d.bw[1] * 8;
  const uint8_t* pcb = py + (int64_t)d.bw[0] * d.bh[0] * 64;
  const uint8_t* pcr = pcb + (int64_t)d.bw[1] * d.bh[1] * 64;
  const int cw = (d.W + d.hs - 1) / d.hs, ch = (d.H + d.vs - 1) / d.vs;
  int cb, cr;
  if (d.hs == 1 && d.vs == 1) {
    cb = pcb[y * p1 + x];
    cr = pcr[y * p1 + x];
  } else if (!d.fancy) {
    const int64_t o1 = (int64_t)(y / d.vs) * p1 + x / d.hs;
    cb = pcb[o1];
    cr = pcr[o1];
  } else {
    const int i = x >> 1, odd = x & 1;
    const int in = odd ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (d.vs == 1) {  // h2v1_fancy_upsample
      const uint8_t *rb = pcb + (int64_t)y * p1, *rr = pcr + (int64_t)y * p1;
      cb = (3 * rb[i] + rb[in] + 1 + odd) >> 2;
      cr = (3 * rr[i] + rr[in] + 1 + odd) >> 2;
    } else {  // h2v2_fancy_upsample: column sums of this row and the nearer neighbour row, then the horizontal triangle
      const int j = y >> 1, jn = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
      const uint8_t *b0 = pcb + (int64_t)j * p1, *b1 = pcb + (int64_t)jn * p1;
      const uint8_t *r0 = pcr + (int64_t)j * p1, *r1 = pcr + (int64_t)jn * p1;
      const int sb = 3 * b0[i] + b1[i], sbn = 3 * b0[in] + b1[in];
      const int sr = 3 * r0[i] + r1[i], srn = 3 * r0[in] + r1[in];
      cb = (3 * sb + sbn + 8 - odd) >> 4;
      cr = (3 * sr + srn + 8 - odd) >> 4;
    }
  }
  const int xcb = cb - 128, xcr = cr - 128;  // ycc_rgb_convert (jdcolor.c), SCALEBITS = 16
  const int r = Y + ((91881 * xcr + 32768) >> 16);
  const int g = Y + ((-22554 * xcb + 32768 - 46802 * xcr) >> 16);
  const int b = Y + ((116130 * xcb + 32768) >> 16);
  o[0] = (uint8_t)min(max(r, 0), 255);
  o[1] = (uint8_t)min(max(g, 0), 255);
  o[2] = (uint8_t)min(max(b, 0), 255);
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
inline int64_t blocks_of(const d2r_jpeg_image_desc& d) {
  int64_t n = 0;
  for (int c = 0; c < d.ncomp && c < 3; ++c) n += (int64_t)d.bw[c] * d.bh[c];
  return n;
}

// every bound the kernels rely on, checked on the host copies
int check_jpeg(const uint8_t* data, int64_t data_bytes, const d2r_jpeg_image_desc* h, int B, const d2r_jpeg_segment* hs, int nseg,
               const int32_t* ht, int64_t tab_len, int64_t dst_bytes, size_t ws_bytes, int* max_chunk_groups, int64_t* max_blocks,
               int64_t* max_pixels, int64_t* coef_lo, int64_t* coef_hi) {
  (void)ht;
  int64_t dst_end = 0, rec_end = 0, coef_end = 0, plane_end = 0;
  *max_chunk_groups = 0;
  *max_blocks = *max_pixels = 0;
  for (int k = 0; k < 3; ++k) {  // the three kinds of workspace regions, each kind after the previous one, in image order
    for (int b = 0; b < B; ++b) {
      const d2r_jpeg_image_desc& d = h[b];
      if (k == 0) {
        D2R_REQUIRE(d.ws_rec >= rec_end && d.ws_rec % 256 == 0, "d2r_jpeg_decode: image %d: chunk states at %lld overlap or are misaligned", b,
                    (long long)d.ws_rec);
        rec_end = d.ws_rec + (int64_t)d.nchunk * (int64_t)sizeof(Rec);
      } else if (k == 1) {
        D2R_REQUIRE(d.ws_coef >= (b ? coef_end : rec_end) && d.ws_coef % 256 == 0,
                    "d2r_jpeg_decode: image %d: coefficients at %lld overlap or are misaligned", b, (long long)d.ws_coef);
        if (b == 0) *coef_lo = d.ws_coef;
        coef_end = d.ws_coef + blocks_of(d) * 128;
      } else {
        D2R_REQUIRE(d.ws_plane >= (b ? plane_end : coef_end) && d.ws_plane % 256 == 0,
                    "d2r_jpeg_decode: image %d: sample planes at %lld overlap or are misaligned", b, (long long)d.ws_plane);
        plane_end = d.ws_plane + blocks_of(d) * 64;
      }
      if (k) continue;
      D2R_REQUIRE(d.H >= 1 && d.W >= 1 && d.H <= 65535 && d.W <= 65535 && (int64_t)d.H * d.W <= (1LL << 28),
                  "d2r_jpeg_decode: image %d: bad size %d x %d", b, d.H, d.W);
      D2R_REQUIRE(d.dst_offset >= dst_end && d.dst_offset + (int64_t)d.H * d.W * 3 <= dst_bytes,
                  "d2r_jpeg_decode: image %d: pixels at %lld overlap the previous image or lie outside the %lld output bytes", b,
                  (long long)d.dst_offset, (long long)dst_bytes);
      dst_end = d.dst_offset + (int64_t)d.H * d.W * 3;
      D2R_REQUIRE((d.ncomp == 1 || d.ncomp == 3) && (d.fancy == 0 || d.fancy == 1) &&
                      ((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2)),
                  "d2r_jpeg_decode: image %d: %d components, ratio h%dv%d, fancy %d not supported", b, d.ncomp, d.hs, d.vs, d.fancy);
      D2R_REQUIRE(d.mcux >= 1 && d.mcuy >= 1 && (int64_t)d.mcux * d.mcuy <= (1LL << 26) && d.mcu_blocks >= 1 && d.mcu_blocks <= 10,
                  "d2r_jpeg_decode: image %d: bad MCU grid %d x %d of %d blocks", b, d.mcux, d.mcuy, d.mcu_blocks);
      int per_comp[3] = {0, 0, 0};
      for (int c = 0; c < d.ncomp; ++c) {
        D2R_REQUIRE(d.h[c] >= 1 && d.h[c] <= 4 && d.v[c] >= 1 && d.v[c] <= 4 && d.bw[c] == d.mcux * d.h[c] && d.bh[c] == d.mcuy * d.v[c],
                    "d2r_jpeg_decode: image %d, component %d: sampling %d x %d, planes of %d x %d blocks disagree with the MCU grid", b,
                    c, d.h[c], d.v[c], d.bw[c], d.bh[c]);
        const int64_t spans[3][2] = {{d.qt[c], 64}, {d.dc[c], D2R_JPEG_HUFF_INTS}, {d.ac[c], D2R_JPEG_HUFF_INTS}};
        for (const auto& s : spans)
          D2R_REQUIRE(s[0] >= 0 && s[0] + s[1] <= tab_len, "d2r_jpeg_decode: image %d, component %d: table at %lld outside %lld entries",
                      b, c, (long long)s[0], (long long)tab_len);
      }
      for (int j = 0; j < d.mcu_blocks; ++j) {
        const int m = d.mcu_map[j], c = m & 15, dx = (m >> 4) & 15, dy = (m >> 8) & 15;
        D2R_REQUIRE(m >= 0 && m < (1 << 12) && c < d.ncomp && dx < d.h[c] && dy < d.v[c],
                    "d2r_jpeg_decode: image %d: bad MCU map entry %d (%d)", b, j, m);
        ++per_comp[c];
      }
      for (int c = 0; c < d.ncomp; ++c)
        D2R_REQUIRE(per_comp[c] == d.h[c] * d.v[c], "d2r_jpeg_decode: image %d: the MCU map has %d blocks of component %d, not %d", b,
                    per_comp[c], c, d.h[c] * d.v[c]);
      D2R_REQUIRE((int64_t)d.bw[0] * 8 >= d.W && (int64_t)d.bh[0] * 8 >= d.H,
                  "d2r_jpeg_decode: image %d: the first component's planes do not cover the image", b);
      if (d.ncomp == 3)
        for (int c = 1; c < 3; ++c)
          D2R_REQUIRE(d.bw[c] == d.bw[1] && d.bh[c] == d.bh[1] && (int64_t)d.bw[c] * 8 * d.hs >= d.W && (int64_t)d.bh[c] * 8 * d.vs >= d.H,
                      "d2r_jpeg_decode: image %d: chroma planes do not cover the image", b);
      const int64_t total = (int64_t)d.mcux * d.mcuy;
      D2R_REQUIRE(d.restart >= 0 && d.nseg == (d.restart ? (total + d.restart - 1) / d.restart : 1) && d.seg0 >= 0 &&
                      (int64_t)d.seg0 + d.nseg <= nseg,
                  "d2r_jpeg_decode: image %d: segments [%d, +%d) disagree with the restart interval %d or lie outside the %d given", b,
                  d.seg0, d.nseg, d.restart, nseg);
      int64_t chunks = 0;
      for (int si = 0; si < d.nseg; ++si) {
        const d2r_jpeg_segment& s = hs[d.seg0 + si];
        D2R_REQUIRE(s.bits >= 0 && s.bits <= (1 << 30) && s.offset >= 0 && s.offset % 4 == 0 &&
                        s.offset + ((int64_t)s.bits + 7) / 8 + D2R_JPEG_SEG_PAD <= data_bytes && s.chunk0 == chunks,
                    "d2r_jpeg_decode: image %d, segment %d: %d bits at byte %lld (chunk %d) outside the %lld data bytes or out of order", b,
                    si, s.bits, (long long)s.offset, s.chunk0, (long long)data_bytes);
        chunks += s.bits > 0 ? ((int64_t)s.bits + CB - 1) / CB : 1;
      }
      D2R_REQUIRE(chunks == d.nchunk && chunks <= (1LL << 24), "d2r_jpeg_decode: image %d: %d chunks declared, the segments make %lld", b,
                  d.nchunk, (long long)chunks);
      *max_chunk_groups = std::max(*max_chunk_groups, d2r_cdiv(d.nchunk, NT));
      *max_blocks = std::max(*max_blocks, blocks_of(d));
      *max_pixels = std::max(*max_pixels, (int64_t)d.H * d.W);
    }
  }
  *coef_hi = coef_end;
  if (plane_end > (int64_t)ws_bytes)
    return d2r_fail(D2R_ERR_WORKSPACE, "d2r_jpeg_decode: workspace of %zu bytes, the batch needs %lld", ws_bytes, (long long)plane_end);
  return D2R_OK;
}

}  // namespace

extern "C" size_t d2r_jpeg_decode_ws_bytes(const d2r_jpeg_image_desc* h_desc, int B) {
  int64_t end = 0;
  for (int b = 0; h_desc && b < B; ++b) end = std::max(end, h_desc[b].ws_plane + blocks_of(h_desc[b]) * 64);
  return (size_t)end;
}

extern "C" int d2r_jpeg_decode(const uint8_t* data, int64_t data_bytes, const d2r_jpeg_image_desc* h_desc, const d2r_jpeg_image_desc* desc,
                               int B, const d2r_jpeg_segment* h_seg, const d2r_jpeg_segment* seg, int nseg, const int32_t* h_tab,
                               const int32_t* tab, int64_t tab_len, uint8_t* dst, int64_t dst_bytes, int32_t* status, int32_t* stats,
                               void* ws, size_t ws_bytes, void* stream) {
  D2R_REQUIRE(data && h_desc && desc && h_seg && seg && h_tab && tab && dst && status && ws, "d2r_jpeg_decode: null pointer");
  D2R_REQUIRE(B >= 1 && B <= 65535 && nseg >= 1 && tab_len >= 0 && tab_len <= INT32_MAX && data_bytes >= 0 && dst_bytes >= 0,
              "d2r_jpeg_decode: bad batch %d, %d segments or table length %lld", B, nseg, (long long)tab_len);
  D2R_REQUIRE((reinterpret_cast<uintptr_t>(data) & 3u) == 0 && (reinterpret_cast<uintptr_t>(desc) & 7u) == 0 &&
                  (reinterpret_cast<uintptr_t>(seg) & 7u) == 0 && (reinterpret_cast<uintptr_t>(tab) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(status) & 3u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3u) == 0 && d2r_aligned16(ws),
              "d2r_jpeg_decode: data / tab / status / stats must be 4-byte, desc / seg 8-byte, ws 16-byte aligned");
  int groups = 0;
  int64_t max_blocks = 0, max_pixels = 0, coef_lo = 0, coef_hi = 0;
  if (int rc = check_jpeg(data, data_bytes, h_desc, B, h_seg, nseg, h_tab, tab_len, dst_bytes, ws_bytes, &groups, &max_blocks, &max_pixels,
                          &coef_lo, &coef_hi))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  if (hipMemsetAsync(status, 0, sizeof(int32_t) * B, st) != hipSuccess ||
      (stats && hipMemsetAsync(stats, 0, sizeof(int32_t) * 2 * B, st) != hipSuccess) ||
      (coef_hi > coef_lo && hipMemsetAsync(w + coef_lo, 0, (size_t)(coef_hi - coef_lo), st) != hipSuccess))
    return d2r_fail(D2R_ERR_LAUNCH, "d2r_jpeg_decode: hipMemsetAsync failed");
  hipLaunchKernelGGL(jpeg_sync_kernel, dim3(groups, B), dim3(NT), 0, st, data, desc, seg, tab, w, stats);
  if (int rc = d2r_check_launch("d2r_jpeg_decode (sync)")) return rc;
  hipLaunchKernelGGL(jpeg_boundary_kernel, dim3(B), dim3(64), 0, st, data, desc, seg, tab, w, stats);
  if (int rc = d2r_check_launch("d2r_jpeg_decode (boundaries)")) return rc;
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(B), dim3(NT), 0, st, data, desc, seg, w);
  if (int rc = d2r_check_launch("d2r_jpeg_decode (scan)")) return rc;
  hipLaunchKernelGGL(jpeg_write_kernel, dim3(groups, B), dim3(NT), 0, st, data, desc, seg, tab, w, status);
  if (int rc = d2r_check_launch("d2r_jpeg_decode (coefficients)")) return rc;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(d2r_cdiv(max_blocks, 256), B), dim3(256), 0, st, desc, tab, w);
  if (int rc = d2r_check_launch("d2r_jpeg_decode (idct)")) return rc;
  hipLaunchKernelGGL(jpeg_color_kernel, dim3(d2r_cdiv(max_pixels, 256), B), dim3(256), 0, st, desc, (const uint8_t*)w, dst);
  return d2r_check_launch("d2r_jpeg_decode (colour)");
}
