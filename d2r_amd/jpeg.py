"""Baseline JPEG decoding on the device, bit-identical to Pillow (``np.asarray(Image.open(p).convert("RGB"))``), for the real-data
loader (``MSDDataset(image_decode="device")``).

Pillow decodes with libjpeg-turbo, whose default path is integer-exact: Huffman decoding, ISLOW IDCT (13-bit constants, 2 pass-1
bits) with its 10-bit wrap-around range-limit table, "fancy" triangular chroma upsampling (h2v1 / h2v2) and fixed-point
YCbCr -> RGB tables.  The device path (``d2r_jpeg_decode``, csrc/jpeg.hip) restates each step in the same integer arithmetic;
``reference_decode`` restates it in numpy so that the exactness can be checked against Pillow on a CPU.

This module is the host side, run in the loader workers:
  * ``parse`` walks the markers and decides per file: device (baseline / extended sequential Huffman, 8-bit, one scan, grayscale
    or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, optional restart intervals) or host (everything else, decoded by Pillow as before);
  * it builds the Huffman decode tables (cached by DHT bytes), removes the byte stuffing and splits the scan at RSTn markers with
    numpy (no Python loop over the entropy bytes);
  * ``plan_jpeg_batch`` packs a batch into one uint8 buffer of zero-padded restart segments plus descriptors and an int32 table.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import _lib

CHUNK_BITS = 1024  # entropy bits per device lane (D2R_JPEG_CHUNK_BITS)
SEG_PAD = 8        # zero bytes after every restart segment: the device bit reader may look that far past its end
HUFF_INTS = 802    # int32 per Huffman table: look[512] ((len << 8) | symbol, len <= 9; 0 = longer code), maxcode[17], valoff[17], vals[256]
LOOKAHEAD = 9

# zigzag index -> natural (row-major) index, libjpeg's jpeg_natural_order
NATURAL_ORDER = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                          60, 61, 54, 47, 55, 62, 63], np.int64)

SEG_DTYPE = np.dtype([("offset", "<i8"), ("bits", "<i4"), ("chunk0", "<i4")])
DESC_DTYPE = np.dtype([("dst_offset", "<i8"), ("ws_rec", "<i8"), ("ws_coef", "<i8"), ("ws_plane", "<i8")] +
                      [(n, "<i4") for n in ("H", "W", "ncomp", "hs", "vs", "fancy", "mcux", "mcuy", "mcu_blocks", "restart",
                                            "seg0", "nseg", "nchunk")] +
                      [(n, "<i4", (3,)) for n in ("h", "v", "bw", "bh", "qt", "dc", "ac")] + [("mcu_map", "<i4", (10,))])
assert DESC_DTYPE.itemsize == C.sizeof(_lib.JpegImageDesc) and SEG_DTYPE.itemsize == C.sizeof(_lib.JpegSegment)

MAX_PIXELS = 1 << 28                 # d2r_jpeg_decode refuses larger images
MAX_SEGMENT_BYTES = (1 << 30) // 8   # ... and larger restart segments


def max_pixels() -> int:
    """The largest H * W decoded on the device: what Pillow opens without DecompressionBombError (more than twice
    Image.MAX_IMAGE_PIXELS is an error there; the host path keeps that behaviour and its inf.png fallback), and at most
    MAX_PIXELS."""
    from PIL import Image
    limit = Image.MAX_IMAGE_PIXELS
    return MAX_PIXELS if limit is None else min(MAX_PIXELS, 2 * int(limit))


# status bits the device writes per image (d2r_jpeg_decode)
STATUS_BAD_CODE, STATUS_SHORT, STATUS_BAD_RUN = 1, 2, 4


class HostPath(Exception):
    """The file is not decoded on the device (the message says why); the loader decodes it with Pillow."""


@functools.lru_cache(maxsize=256)
def huffman_table(dht: bytes, is_dc: bool) -> np.ndarray:
    """libjpeg's jpeg_make_d_derived_tbl for one DHT entry (16 counts + symbols): int32 [HUFF_INTS].  Raises HostPath where libjpeg
    raises JERR_BAD_HUFF_TABLE."""
    counts = list(dht[:16])
    vals = list(dht[16:])
    if sum(counts) > 256 or sum(counts) != len(vals):
        raise HostPath("bad Huffman table")
    if is_dc and any(v > 15 for v in vals):
        raise HostPath("DC symbol above 15")
    look = np.zeros(1 << LOOKAHEAD, np.int32)
    maxcode = np.full(17, -1, np.int32)
    valoff = np.zeros(17, np.int32)
    code, p = 0, 0
    for l in range(1, 17):
        n = counts[l - 1]
        if n:
            valoff[l] = p - code
            for i in range(n):
                if l <= LOOKAHEAD:
                    lo = (code + i) << (LOOKAHEAD - l)
                    look[lo:lo + (1 << (LOOKAHEAD - l))] = (l << 8) | vals[p + i]
            code += n
            p += n
            maxcode[l] = code - 1
            if code >= (1 << l):  # libjpeg: the all-ones code of a length may not be used
                raise HostPath("bad Huffman table")
        code <<= 1
    v = np.zeros(256, np.int32)
    v[:len(vals)] = vals
    out = np.concatenate([look, maxcode, valoff, v]).astype(np.int32)
    out.flags.writeable = False
    return out


class JpegInfo:
    """What the device needs of one accepted file: geometry, tables and the unstuffed restart segments."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _u16(b, i):
    return (b[i] << 8) | b[i + 1]


def parse(data: bytes) -> JpegInfo:
    """Walks the markers of `data`; returns a JpegInfo for a file the device decodes, raises HostPath otherwise."""
    b = memoryview(data)
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise HostPath("not a JPEG")
    i = 2
    qt, dht, frame, restart, jfif, adobe = {}, {}, None, 0, False, None
    while True:
        if i + 4 > n:
            raise HostPath("truncated")
        if b[i] != 0xFF:
            raise HostPath("junk between markers")
        m = b[i + 1]
        if m == 0xFF:
            raise HostPath("fill bytes before a marker")
        L = _u16(b, i + 2)
        seg = bytes(b[i + 4:i + 2 + L])
        if L < 2 or i + 2 + L > n:
            raise HostPath("truncated")
        i += 2 + L
        if m == 0xE0 and L >= 16 and seg[:5] == b"JFIF\0":  # libjpeg-turbo: an APP0 of at least 14 data bytes
            jfif = True
        elif m == 0xEE and L >= 14 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or p + 1 + size > len(seg):
                    raise HostPath("bad DQT")
                q = np.frombuffer(seg[p + 1:p + 1 + size], ">u2" if pq else "u1").astype(np.int32)
                if q.max() > 32767:
                    raise HostPath("quantiser above 32767")
                nat = np.zeros(64, np.int32)
                nat[NATURAL_ORDER] = q
                qt[tq] = nat
                p += 1 + size
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    raise HostPath("bad DHT")
                tc, th = seg[p] >> 4, seg[p] & 15
                cnt = sum(seg[p + 1:p + 17])
                if tc > 1 or th > 3 or p + 17 + cnt > len(seg):
                    raise HostPath("bad DHT")
                dht[(tc, th)] = bytes(seg[p + 1:p + 17 + cnt])
                p += 17 + cnt
        elif m in (0xC0, 0xC1):
            if frame is not None or len(seg) < 6:
                raise HostPath("bad SOF")
            P, H, W, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if P != 8 or H == 0 or W == 0 or nf not in (1, 3) or len(seg) < 6 + 3 * nf:
                raise HostPath(f"unsupported frame (precision {P}, {H} x {W}, {nf} components)")
            if H * W > max_pixels():
                raise HostPath(f"{H} x {W} pixels: above Pillow's decompression-bomb limit or the device's")
            comps = [dict(id=seg[6 + 3 * k], h=seg[7 + 3 * k] >> 4, v=seg[7 + 3 * k] & 15, tq=seg[8 + 3 * k]) for k in range(nf)]
            if any(not (1 <= c["h"] <= 4 and 1 <= c["v"] <= 4) for c in comps):
                raise HostPath("bad sampling factors")
            frame = (H, W, comps)
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise HostPath(f"SOF{m - 0xC0} (not baseline / extended sequential Huffman)")
        elif m == 0xCC:
            raise HostPath("arithmetic coding")
        elif m == 0xDD:
            if L != 4:
                raise HostPath("bad DRI")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            break
        else:
            raise HostPath(f"marker {m:02X} before the scan")
    if frame is None:
        raise HostPath("no frame before the scan")
    H, W, comps = frame
    ns = seg[0] if len(seg) else 0
    if ns != len(comps) or len(seg) != 4 + 2 * ns:
        raise HostPath("multi-scan")
    ss, se, ahal = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
    if ss != 0 or se != 63 or ahal != 0:
        raise HostPath("not a sequential scan")
    ids = [c["id"] for c in comps]
    order = []
    for k in range(ns):
        cid, t = seg[1 + 2 * k], seg[2 + 2 * k]
        if cid not in ids or ids.index(cid) in order:
            raise HostPath("bad scan components")
        order.append(ids.index(cid))
        comps[ids.index(cid)]["td"], comps[ids.index(cid)]["ta"] = t >> 4, t & 15
    if len(comps) == 3:
        # libjpeg's colour-space guess (jdapimin.c default_decompress_parms): RGB files and YCCK-like guesses go to the host
        if jfif:
            ycc = True
        elif adobe is not None:
            ycc = adobe == 1
        else:
            ycc = ids == [1, 2, 3]
        if not ycc:
            raise HostPath("colour transform is not YCbCr")
    # tables
    qtabs, dtabs, atabs = [], [], []
    for c in comps:
        if c["tq"] not in qt:
            raise HostPath("missing quantisation table")
        if (0, c["td"]) not in dht or (1, c["ta"]) not in dht:
            raise HostPath("missing Huffman table")
        qtabs.append(qt[c["tq"]])
        dtabs.append(huffman_table(dht[(0, c["td"])], True))
        atabs.append(huffman_table(dht[(1, c["ta"])], False))
    # geometry
    if len(comps) == 1:
        hs = vs = 1
        mcux, mcuy = -(-W // 8), -(-H // 8)
        hv = [(1, 1)]
        mcu_map = [0]
        bw, bh = [mcux], [mcuy]
    else:
        (hy, vy), (hb, vb), (hr, vr) = [(c["h"], c["v"]) for c in comps]
        hmax, vmax = max(hy, hb, hr), max(vy, vb, vr)
        if (hb, vb) != (hr, vr) or (hy, vy) != (hmax, vmax) or hy % hb or vy % vb:
            raise HostPath("unsupported chroma sampling")
        hs, vs = hy // hb, vy // vb
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
            raise HostPath(f"chroma ratio h{hs}v{vs}")
        mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
        hv = [(c["h"], c["v"]) for c in comps]
        mcu_map = [ci | (dx << 4) | (dy << 8) for ci in order for dy in range(hv[ci][1]) for dx in range(hv[ci][0])]
        if len(mcu_map) > 10:
            raise HostPath("more than 10 blocks per MCU")
        bw, bh = [mcux * h for h, _ in hv], [mcuy * v for _, v in hv]
    # scan data: the first marker other than RSTn and stuffing must be EOI
    start = i
    scan = np.frombuffer(data, np.uint8, offset=start)
    ff = np.flatnonzero(scan[:-1] == 0xFF)
    nxt = scan[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    ends = np.flatnonzero((nxt != 0) & ~is_rst)
    if ends.size == 0:
        raise HostPath("truncated (no EOI)")
    e = int(ff[ends[0]])
    if nxt[ends[0]] != 0xD9:
        raise HostPath("more than one scan" if nxt[ends[0]] != 0xFF else "fill bytes in the scan")
    before = ff < e
    stuff = ff[before & (nxt == 0)]
    rst = ff[before & is_rst]
    total = mcux * mcuy
    nseg = -(-total // restart) if restart else 1
    if rst.size != nseg - 1:
        raise HostPath("restart markers do not match the restart interval")
    if rst.size and not np.array_equal(scan[rst + 1], 0xD0 + (np.arange(rst.size) & 7)):
        raise HostPath("restart markers out of sequence")
    segments = unstuff(scan[:e], stuff, rst)
    if max(s.size for s in segments) > MAX_SEGMENT_BYTES:
        raise HostPath("restart segment above the device's limit")
    return JpegInfo(H=H, W=W, ncomp=len(comps), hs=hs, vs=vs, fancy=int(-(-W // hs) > 2), mcux=mcux, mcuy=mcuy, restart=restart,
                    hv=hv, bw=bw, bh=bh, mcu_map=mcu_map, qt=qtabs, dc=dtabs, ac=atabs, segments=segments)


def unstuff(scan: np.ndarray, stuff: np.ndarray, rst: np.ndarray):
    """Entropy-coded bytes `scan` (up to the final marker) without the stuffed zeros after `stuff` positions, split at the RSTn
    markers at `rst` positions: a list of uint8 arrays, one per restart segment."""
    keep = np.ones(scan.size, bool)
    keep[stuff + 1] = False
    keep[rst] = False
    keep[rst + 1] = False
    out = scan[keep]
    cuts = np.cumsum(keep)[rst] - 1 if rst.size else np.zeros(0, np.int64)  # kept bytes before each marker
    return np.split(out, cuts + 1) if rst.size else [out]


def route(data: bytes):
    """(JpegInfo, None) when the device decodes `data`, (None, reason) otherwise."""
    try:
        return parse(data), None
    except HostPath as e:
        return None, str(e)


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatement of the device decode
def _entropy_decode(info: JpegInfo) -> list:
    """Coefficient planes int16 [bh * 8 rows of blocks ...] per component: list of int32 [bh, bw, 64] (natural order).  A Python
    loop over the symbols (slow; tests only)."""
    coef = [np.zeros((info.bh[c], info.bw[c], 64), np.int32) for c in range(info.ncomp)]
    nb = len(info.mcu_map)
    total = info.mcux * info.mcuy
    per_seg = info.restart if info.restart else total
    for s, seg in enumerate(info.segments):
        b = np.concatenate([seg, np.zeros(SEG_PAD, np.uint8)]).astype(np.int64)
        w40 = ((b[:-4] << 32) | (b[1:-3] << 24) | (b[2:-2] << 16) | (b[3:-1] << 8) | b[4:]).tolist()
        pos = 0
        pred = [0, 0, 0]
        mcu0 = s * per_seg
        for g in range(min(per_seg, total - mcu0) * nb):
            mcu, m = mcu0 + g // nb, info.mcu_map[g % nb]
            ci, dx, dy = m & 15, (m >> 4) & 15, (m >> 8) & 15
            blk = coef[ci][(mcu // info.mcux) * info.hv[ci][1] + dy, (mcu % info.mcux) * info.hv[ci][0] + dx]
            k = 0
            while k < 64:
                tab = info.dc[ci] if k == 0 else info.ac[ci]
                w = (w40[pos >> 3] >> (8 - (pos & 7))) & 0xFFFFFFFF
                e = int(tab[w >> (32 - LOOKAHEAD)])
                if e >> 8:
                    l, sym = e >> 8, e & 255
                else:
                    for l in range(LOOKAHEAD + 1, 17):
                        code = w >> (32 - l)
                        if code <= tab[512 + l]:
                            sym = int(tab[546 + ((code + int(tab[529 + l])) & 255)])
                            break
                    else:
                        raise ValueError("invalid Huffman code")
                r, sz = (0, sym & 15) if k == 0 else (sym >> 4, sym & 15)
                v = 0
                if sz:
                    v = ((w << l) & 0xFFFFFFFF) >> (32 - sz)
                    if v < (1 << (sz - 1)):
                        v += 1 - (1 << sz)
                pos += l + sz
                if pos > len(seg) * 8:
                    raise ValueError("segment ends early")
                if k == 0:
                    pred[ci] += v
                    blk[0] = ((pred[ci] + 32768) & 0xFFFF) - 32768
                    k = 1
                elif sz:
                    k += r
                    blk[NATURAL_ORDER[min(k, 63)]] = v
                    k += 1
                elif r == 15:
                    k += 16
                else:
                    break
    return coef


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(s):
    """One ISLOW pass over the 8 int64 arrays s[0..7] (jidctint.c): (tmp10, tmp11, tmp12, tmp13, tmp0, tmp1, tmp2, tmp3)."""
    z1 = (s[2] + s[6]) * 4433
    tmp2 = z1 + s[6] * -15137
    tmp3 = z1 + s[2] * 6270
    tmp0 = (s[0] + s[4]) << 13
    tmp1 = (s[0] - s[4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    a0, a1, a2, a3 = s[7], s[5], s[3], s[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return t10, t11, t12, t13, a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4


def _idct_pass(x, shift):
    t10, t11, t12, t13, o0, o1, o2, o3 = _idct_1d([x[..., i] for i in range(8)])
    return np.stack([_descale(t10 + o3, shift), _descale(t11 + o2, shift), _descale(t12 + o1, shift), _descale(t13 + o0, shift),
                     _descale(t13 - o0, shift), _descale(t12 - o1, shift), _descale(t11 - o2, shift), _descale(t10 - o3, shift)], -1)


def idct_islow(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """libjpeg-turbo's jpeg_idct_islow (its C code) of int [..., 64] natural-order blocks with quantisers q [64]: uint8 [..., 8, 8].
    Its SIMD forms compute in 16-bit lanes; they agree with the C code for every coefficient 8-bit samples produce, not for
    arbitrary crafted ones."""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    ws = _idct_pass(np.swapaxes(x, -1, -2), 13 - 2)        # columns: ws[..., col, row], 64-bit as the C code's JLONG
    ws = ws.astype(np.int32).astype(np.int64)               # ... stored in its int workspace
    out = _idct_pass(np.swapaxes(ws, -1, -2), 13 + 2 + 3)  # rows
    v = out & 1023
    v = np.where(v >= 512, v - 1024, v) + 128               # the 10-bit wrap of the range-limit table, then the clamp
    return np.clip(v, 0, 255).astype(np.uint8)


def _plane(coef, q):
    bh, bw, _ = coef.shape
    return idct_islow(coef, q).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample(c: np.ndarray, cw: int, ch: int, hs: int, vs: int, fancy: bool, W: int, H: int) -> np.ndarray:
    """libjpeg-turbo's upsampling of the real cw x ch samples of chroma plane `c` to H x W (jdsample.c)."""
    c = c[:ch, :cw].astype(np.int32)
    if hs == 1 and vs == 1:
        return c[:H, :W]
    if not fancy:
        return np.repeat(np.repeat(c, vs, 0), hs, 1)[:H, :W]
    if vs == 2:
        up = np.concatenate([c[:1], c[:-1]], 0)
        dn = np.concatenate([c[1:], c[-1:]], 0)
        rows = np.stack([3 * c + up, 3 * c + dn], 1).reshape(2 * ch, cw)  # column sums of output rows 2j, 2j+1
        left = np.concatenate([rows[:, :1], rows[:, :-1]], 1)
        right = np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
        out = np.stack([(3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4], 2).reshape(2 * ch, 2 * cw)
    else:
        left = np.concatenate([c[:, :1], c[:, :-1]], 1)
        right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
        out = np.stack([(3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2], 2).reshape(ch, 2 * cw)
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr) -> np.ndarray:
    """jdcolor.c ycc_rgb_convert with its 16-bit fixed-point tables."""
    y, cb, cr = (np.asarray(a, np.int64) for a in (y, cb, cr))
    r = y + ((91881 * (cr - 128) + 32768) >> 16)
    g = y + ((-22554 * (cb - 128) + 32768 - 46802 * (cr - 128)) >> 16)
    b = y + ((116130 * (cb - 128) + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def reference_decode(data: bytes) -> np.ndarray:
    """numpy restatement of the whole device decode: uint8 [H, W, 3].  Raises HostPath for a file the device does not decode."""
    info = parse(data)
    coef = _entropy_decode(info)
    planes = [_plane(coef[c], info.qt[c]) for c in range(info.ncomp)]
    H, W = info.H, info.W
    if info.ncomp == 1:
        return np.repeat(planes[0][:H, :W, None], 3, 2)
    cw, ch = -(-W // info.hs), -(-H // info.vs)
    cb = upsample(planes[1], cw, ch, info.hs, info.vs, info.fancy, W, H)
    cr = upsample(planes[2], cw, ch, info.hs, info.vs, info.fancy, W, H)
    return ycc_to_rgb(planes[0][:H, :W], cb, cr)


# ---------------------------------------------------------------------------------------------------------------------------
# packing and the device call
def _align(v, a):
    return -(-v // a) * a


def plan_jpeg_batch(infos, dst_offsets):
    """Packs accepted files for d2r_jpeg_decode; image b's pixels go to byte dst_offsets[b] of the output buffer.  Returns
    (data uint8 [N], descriptors DESC_DTYPE [B], segments SEG_DTYPE [S], table int32 [T])."""
    B = len(infos)
    if B == 0:
        raise ValueError("empty batch")
    desc = np.zeros(B, DESC_DTYPE)
    segs, parts, dlen = [], [], 0
    tabs, tlen, seen = [], 0, {}

    def table(arr):
        nonlocal tlen
        key = arr.tobytes()
        if key not in seen:
            seen[key] = tlen
            tabs.append(arr)
            tlen += arr.size
        return seen[key]

    for b, info in enumerate(infos):
        d = desc[b]
        d["dst_offset"] = int(dst_offsets[b])
        for k in ("H", "W", "ncomp", "hs", "vs", "fancy", "mcux", "mcuy", "restart"):
            d[k] = getattr(info, k)
        d["mcu_blocks"] = len(info.mcu_map)
        d["mcu_map"][:len(info.mcu_map)] = info.mcu_map
        d["seg0"], d["nseg"] = len(segs), len(info.segments)
        chunks = 0
        for s in info.segments:
            bits = int(s.size) * 8
            segs.append((dlen, bits, chunks))
            padded = _align(s.size + SEG_PAD, 4)
            parts += [s, np.zeros(padded - s.size, np.uint8)]
            dlen += padded
            chunks += max(1, -(-bits // CHUNK_BITS))
        d["nchunk"] = chunks
        for c in range(info.ncomp):
            d["h"][c], d["v"][c] = info.hv[c]
            d["bw"][c], d["bh"][c] = info.bw[c], info.bh[c]
            d["qt"][c], d["dc"][c], d["ac"][c] = table(info.qt[c]), table(info.dc[c]), table(info.ac[c])
    # workspace: every image's chunk states, then every image's coefficients, then every image's sample planes
    end = 0
    for field, size in (("ws_rec", lambda d: 48 * int(d["nchunk"])), ("ws_coef", lambda d: 128 * _blocks(d)),
                        ("ws_plane", lambda d: 64 * _blocks(d))):
        for d in desc:
            d[field] = end = _align(end, 256)
            end += size(d)
    return np.concatenate(parts), desc, np.array(segs, SEG_DTYPE), np.concatenate(tabs).astype(np.int32)


def _blocks(d):
    return int(sum(int(d["bw"][c]) * int(d["bh"][c]) for c in range(int(d["ncomp"]))))


def ws_bytes(h_desc: np.ndarray) -> int:
    return int(_lib.load().d2r_jpeg_decode_ws_bytes(C.cast(h_desc.ctypes.data, C.POINTER(_lib.JpegImageDesc)), len(h_desc)))


def jpeg_decode(data: torch.Tensor, h_desc: np.ndarray, desc: torch.Tensor, h_seg: np.ndarray, seg: torch.Tensor, h_tab: torch.Tensor,
                tab: torch.Tensor, dst: torch.Tensor, status: torch.Tensor = None, stats: torch.Tensor = None,
                ws: torch.Tensor = None) -> torch.Tensor:
    """d2r_jpeg_decode on the current stream: writes every image's HWC RGB pixels into dst (uint8) at its dst_offset.  data / desc /
    seg / tab live on the device, h_desc / h_seg / h_tab are their host copies (every bound is checked on them before anything is
    enqueued).  Returns status, int32 [B] on the device (0 = decoded; see STATUS_*)."""
    B = len(h_desc)
    dev = data.device
    if not (data.dtype == desc.dtype == seg.dtype == dst.dtype == torch.uint8 and tab.dtype == h_tab.dtype == torch.int32):
        raise TypeError("data / desc / seg / dst uint8, tab int32 expected")
    if h_desc.dtype != DESC_DTYPE or h_seg.dtype != SEG_DTYPE or desc.numel() != h_desc.nbytes or seg.numel() != h_seg.nbytes or \
            h_tab.numel() != tab.numel():
        raise ValueError("descriptor / segment / table sizes disagree")
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() for t in (desc, seg, tab, dst)) or h_tab.is_cuda:
        raise ValueError("device tensors must be contiguous on one GPU, h_tab on the host")
    for name, t, n in (("status", status, B), ("stats", stats, 2 * B)):
        if t is not None and not (t.dtype == torch.int32 and t.is_cuda and t.device == dev and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"{name} must be a contiguous int32 tensor of {n} elements on {dev}")
    if ws is not None and not (ws.dtype == torch.uint8 and ws.is_cuda and ws.device == dev and ws.is_contiguous()):
        raise ValueError(f"ws must be a contiguous uint8 tensor on {dev}")
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    if ws is None:
        ws = torch.empty(max(ws_bytes(h_desc), 1), dtype=torch.uint8, device=dev)
    from .functional import _stream
    _lib.call("d2r_jpeg_decode", data.data_ptr(), data.numel(), C.cast(h_desc.ctypes.data, C.POINTER(_lib.JpegImageDesc)),
              desc.data_ptr(), B, C.cast(h_seg.ctypes.data, C.POINTER(_lib.JpegSegment)), seg.data_ptr(), len(h_seg),
              h_tab.data_ptr(), tab.data_ptr(), tab.numel(), dst.data_ptr(), dst.numel(), status.data_ptr(),
              None if stats is None else stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return status


def decode_batch(infos, device, stats: torch.Tensor = None):
    """Decodes accepted files into one device buffer, back to back: (pixels uint8 [N], byte offsets [B], status int32 [B])."""
    offsets = np.cumsum([0] + [i.H * i.W * 3 for i in infos])
    data, desc, segs, tab = plan_jpeg_batch(infos, offsets[:-1])
    meta = _meta(desc, segs, tab)
    dst = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=device)
    status = _decode_meta(torch.from_numpy(data).to(device), meta.to(device), desc, segs, meta, dst, stats)
    return dst, offsets[:-1], status


def _meta(desc, segs, tab) -> torch.Tensor:
    return torch.from_numpy(np.concatenate([desc.view(np.uint8), segs.view(np.uint8), tab.view(np.uint8)]))


def _decode_meta(data, meta, h_desc, h_seg, h_meta, dst, stats=None):
    nd, ns = h_desc.nbytes, h_seg.nbytes
    return jpeg_decode(data, h_desc, meta[:nd], h_seg, meta[nd:nd + ns], h_meta[nd + ns:].view(torch.int32),
                       meta[nd + ns:].view(torch.int32), dst, stats=stats)


class PackedJpegImages:
    """A collated batch in which some images are JPEG files the device decodes and the others were decoded on the host (Pillow).
    Host pixels come first in the device pixel buffer, then the device-decoded images; the CLIP descriptors point at both.
    ``to_pixel_values(device)`` runs d2r_jpeg_decode, then d2r_clip_preprocess, on the current stream and keeps the decode
    status (int32 per device-decoded image, on the device) in ``self.status`` for the trainer to read when it syncs anyway."""

    def __init__(self, host_pixels, data, jmeta, nd, ns, clip_meta, batch, S, norm, total):
        self.host_pixels, self.data, self.jmeta, self.nd, self.ns = host_pixels, data, jmeta, nd, ns
        self.clip_meta, self.batch, self.S, self.norm, self.total = clip_meta, batch, S, norm, total
        self.status = None

    @property
    def n_device(self):
        return self.nd // DESC_DTYPE.itemsize

    @property
    def n_host(self):
        return self.batch - self.n_device

    @classmethod
    def from_items(cls, items, R: int, S: int, mean, std, rescale):
        from .image import DESC_DTYPE as CLIP_DESC, as_rgb_array, plan_layout
        host = [(b, as_rgb_array(x)) for b, x in enumerate(items) if not isinstance(x, JpegInfo)]
        dev = [(b, x) for b, x in enumerate(items) if isinstance(x, JpegInfo)]
        offsets = np.zeros(len(items), np.int64)
        shapes = [None] * len(items)
        pos = 0
        for b, im in host:
            offsets[b], shapes[b] = pos, im.shape[:2]
            pos += im.size
        nhost = pos
        for b, info in dev:
            offsets[b], shapes[b] = pos, (info.H, info.W)
            pos += info.H * info.W * 3
        cdesc, ctab = plan_layout(shapes, offsets, R, S)
        clip_meta = torch.from_numpy(np.concatenate([cdesc.view(np.uint8), ctab.view(np.uint8)]))
        host_pixels = torch.from_numpy(np.concatenate([im.reshape(-1) for _, im in host]) if host else np.zeros(0, np.uint8))
        if dev:
            data, desc, segs, tab = plan_jpeg_batch([x for _, x in dev], offsets[[b for b, _ in dev]])
            data, jmeta = torch.from_numpy(data), _meta(desc, segs, tab)
            nd, ns = desc.nbytes, segs.nbytes
        else:
            data, jmeta, nd, ns = torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8), 0, 0
        assert clip_meta.numel() >= len(items) * CLIP_DESC.itemsize and nhost == host_pixels.numel()
        return cls(host_pixels, data, jmeta, nd, ns, clip_meta, len(items), S,
                   (tuple(float(v) for v in mean), tuple(float(v) for v in std), float(rescale)), pos)

    def __len__(self):
        return self.batch

    def pin_memory(self, device=None):
        return PackedJpegImages(self.host_pixels.pin_memory(), self.data.pin_memory(), self.jmeta.pin_memory(), self.nd, self.ns,
                                self.clip_meta.pin_memory(), self.batch, self.S, self.norm, self.total)

    def jpeg_host_parts(self):
        h = self.jmeta.numpy()
        return h[:self.nd].view(DESC_DTYPE), h[self.nd:self.nd + self.ns].view(SEG_DTYPE)

    def decode(self, device, stats: torch.Tensor = None) -> torch.Tensor:
        """The batch's uint8 source pixels on `device` (host-decoded copied, the rest decoded there)."""
        pixels = torch.empty(max(self.total, 1), dtype=torch.uint8, device=device)
        if self.host_pixels.numel():
            pixels[:self.host_pixels.numel()].copy_(self.host_pixels, non_blocking=True)
        if self.nd:
            h_desc, h_seg = self.jpeg_host_parts()
            self.status = _decode_meta(self.data.to(device, non_blocking=True), self.jmeta.to(device, non_blocking=True), h_desc,
                                       h_seg, self.jmeta, pixels, stats)
        return pixels

    def to_pixel_values(self, device) -> torch.Tensor:
        from .image import DESC_DTYPE as CLIP_DESC, _device_table, clip_preprocess
        pixels = self.decode(device)
        nd = self.batch * CLIP_DESC.itemsize
        meta = self.clip_meta.to(device, non_blocking=True)
        h_desc = self.clip_meta.numpy()[:nd].view(CLIP_DESC)
        return clip_preprocess(pixels, h_desc, meta[:nd], self.clip_meta[nd:].view(torch.int32), meta[nd:].view(torch.int32), self.S,
                               _device_table(str(pixels.device), self.norm))

    def to_cache(self, device, cache: torch.Tensor, h_slots: torch.Tensor) -> None:
        """d2r_jpeg_decode, then d2r_clip_preprocess_u8: the batch's uint8 crops into rows h_slots (host int64 [B]) of the crop
        cache on `device` (d2r_amd.cache); ``self.status`` as after to_pixel_values."""
        from .image import _crops_to_cache
        _crops_to_cache(self.decode(device), self.clip_meta, self.batch, self.S, cache, h_slots)


class DecodeLog:
    """Counts, per epoch, the images decoded on the device and on the host and the device decodes with a nonzero status.  The
    status tensors are only read in ``poll()``, which the trainer calls right after a host sync it makes anyway.  Batches served
    from the device cache (d2r_amd.cache.CachedBatch) decode nothing and are counted by their ``cached_images``."""

    def __init__(self, logger):
        self.logger, self.device, self.host, self.bad, self.pending, self.cached = logger, 0, 0, 0, [], 0

    def note(self, batch):
        self.cached += getattr(batch, "cached_images", 0)
        for t in batch:
            if isinstance(t, PackedJpegImages):
                self.device += t.n_device
                self.host += t.n_host
                if t.status is not None:
                    self.pending.append(t.status)

    def poll(self):
        if self.pending:
            n = int(torch.cat([s.view(-1) for s in self.pending]).ne(0).sum().item())
            self.pending = []
            if n:
                self.bad += n
                self.logger.warning("%d JPEG image(s) had corrupt entropy data (%d so far this epoch): their pixels are not what "
                                    "Pillow would give", n, self.bad)

    def end_epoch(self, epoch):
        self.end_pass("epoch %d" % epoch)

    def end_pass(self, what):
        self.poll()
        if self.device or self.host:
            self.logger.info("%s images: %d decoded on the device, %d on the host, %d device decode(s) with corrupt data", what,
                             self.device, self.host, self.bad)
        if self.cached:
            self.logger.info("%s images: %d images from the device cache", what, self.cached)
        self.device = self.host = self.bad = self.cached = 0
