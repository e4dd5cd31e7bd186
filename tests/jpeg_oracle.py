"""Python restatement of the contract of sfmba_jpeg_decode and sfmba_resize_images (include/sfmba.h): header parse, Huffman decode,
the two-pass integer inverse DCT, the triangle chroma upsampling, the fixed-point colour conversion and the bilinear resize with
host-built 11-bit weight tables.  Written from the contract, independent of csrc/: the tests hold it to libjpeg's stored output
(tests/golden/jpeg_small, tests/golden/crazyhorse_half) and hold the product to it.  numpy only."""
import re

import numpy as np

OK, UNSUPPORTED, CORRUPT = 0, 1, 2

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])


class Corrupt(Exception):
    pass


class Unsupported(Exception):
    pass


def _huffman_lookup(bits, vals):
    """16-bit look-ahead -> (length << 8) | symbol as a list; 0 where no code matches."""
    look = np.zeros(1 << 16, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if code >= (1 << length):
                raise Corrupt("not a prefix code")
            first = code << (16 - length)
            look[first:first + (1 << (16 - length))] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return look.tolist()


def parse(data):
    """The header up to the scan: dict(width, height, ncomp, comps=[dict(id, h, v, tq, td, ta, cw, ch, bw, bh)], quant={tq: [64] natural},
    huff={(tc, th): lookup}, restart, scan, mcus_x, mcus_y).  Raises Unsupported / Corrupt."""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Corrupt("no SOI")
    pos, hdr = 2, dict(restart=0, quant={}, huff={}, comps=None)
    while True:
        if pos >= len(data) or data[pos] != 0xFF:
            raise Corrupt("no marker")
        while pos < len(data) and data[pos] == 0xFF:
            pos += 1
        if pos >= len(data):
            raise Corrupt("truncated")
        m = data[pos]
        pos += 1
        if m in (0, 1) or 0xD0 <= m <= 0xD9:
            raise Corrupt("marker without a segment")
        if pos + 2 > len(data):
            raise Corrupt("truncated")
        ln = (data[pos] << 8) | data[pos + 1]
        if ln < 2 or pos + ln > len(data):
            raise Corrupt("segment runs past the end")
        p = data[pos + 2:pos + ln]
        if m == 0xC0:
            if hdr["comps"] is not None or len(p) < 6:
                raise Corrupt("frame")
            prec, h, w, nc = p[0], (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            if len(p) != 6 + 3 * nc or w == 0 or h == 0 or nc == 0:
                raise Corrupt("frame")
            if prec != 8 or nc not in (1, 3) or w > 16384 or h > 16384:
                raise Unsupported("frame")
            comps = [dict(id=p[6 + 3 * c], h=p[7 + 3 * c] >> 4, v=p[7 + 3 * c] & 15, tq=p[8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            elif (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
                raise Unsupported("sampling")
            hdr.update(width=w, height=h, ncomp=nc, comps=comps)
        elif (0xC1 <= m <= 0xCF and m != 0xC4) or m in (0xDC, 0xDE, 0xDF):
            raise Unsupported("marker %02x" % m)
        elif m == 0xDB:
            o = 0
            while o < len(p):
                pq, tq = p[o] >> 4, p[o] & 15
                if pq == 1:
                    raise Unsupported("16-bit quantisation table")
                if pq > 1 or tq > 3 or o + 65 > len(p):
                    raise Corrupt("DQT")
                q = np.zeros(64, np.int32)
                q[ZIGZAG] = np.frombuffer(p[o + 1:o + 65], np.uint8)
                hdr["quant"][tq] = q
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(p):
                tc, th = p[o] >> 4, p[o] & 15
                if tc > 1 or th > 3 or o + 17 > len(p):
                    raise Corrupt("DHT")
                bits = list(p[o + 1:o + 17])
                if sum(bits) > 256 or o + 17 + sum(bits) > len(p):
                    raise Corrupt("DHT")
                hdr["huff"][(tc, th)] = _huffman_lookup(bits, list(p[o + 17:o + 17 + sum(bits)]))
                o += 17 + sum(bits)
        elif m == 0xDD:
            hdr["restart"] = (p[0] << 8) | p[1]
        elif m == 0xDA:
            if hdr["comps"] is None:
                raise Corrupt("scan before frame")
            ns = p[0]
            if ns != hdr["ncomp"]:
                raise Unsupported("several scans")
            for c, comp in enumerate(hdr["comps"]):
                if p[1 + 2 * c] != comp["id"]:
                    raise Unsupported("component order")
                comp["td"], comp["ta"] = p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15
                if (0, comp["td"]) not in hdr["huff"] or (1, comp["ta"]) not in hdr["huff"] or comp["tq"] not in hdr["quant"]:
                    raise Corrupt("missing table")
            hdr["scan"] = pos + ln
            break
        pos += ln
    hmax, vmax = hdr["comps"][0]["h"], hdr["comps"][0]["v"]
    hdr.update(hmax=hmax, vmax=vmax, mcus_x=-(-hdr["width"] // (8 * hmax)), mcus_y=-(-hdr["height"] // (8 * vmax)))
    for comp in hdr["comps"]:
        comp.update(cw=-(-hdr["width"] * comp["h"] // hmax), ch=-(-hdr["height"] * comp["v"] // vmax),
                    bw=hdr["mcus_x"] * comp["h"], bh=hdr["mcus_y"] * comp["v"])
    return hdr


def info(data):
    """(status, width, height, channels, h_samp, v_samp, restart_interval) as sfmba_jpeg_info reports them."""
    try:
        h = parse(data)
    except Unsupported:
        return (UNSUPPORTED,)
    except Corrupt:
        return (CORRUPT,)
    return (OK, h["width"], h["height"], h["ncomp"], h["hmax"], h["vmax"], h["restart"])


def coefficients(data, hdr):
    """One int16 array [bh, bw, 64] (natural order) per component."""
    body = data[hdr["scan"]:]
    end = re.search(rb"\xff[^\x00\xd0-\xd7\xff]", body)            # the first marker that is neither stuffing nor RSTn
    body = body[:end.start()] if end else body
    segments = re.split(rb"\xff+[\xd0-\xd7]", body)
    comps = hdr["comps"]
    out = [np.zeros((c["bh"] * c["bw"], 64), np.int16) for c in comps]
    ri = hdr["restart"] or hdr["mcus_x"] * hdr["mcus_y"]
    order = []                                                   # (component, block-in-MCU row, column) of an MCU
    for ci, c in enumerate(comps):
        order += [(ci, v, u) for v in range(c["v"]) for u in range(c["h"])]
    tables = [(hdr["huff"][(0, c["td"])], hdr["huff"][(1, c["ta"])]) for c in comps]
    zz = ZIGZAG.tolist()
    mcu = 0
    total = hdr["mcus_x"] * hdr["mcus_y"]
    for seg in segments:
        if mcu >= total:
            break
        buf = seg.replace(b"\xff\x00", b"\xff") + b"\x00\x00\x00\x00"
        limit = 8 * (len(buf) - 4)
        pos = 0
        pred = [0] * len(comps)
        for _ in range(min(ri, total - mcu)):
            my, mx = divmod(mcu, hdr["mcus_x"])
            for ci, v, u in order:
                c = comps[ci]
                dc, ac = tables[ci]
                blk = [0] * 64
                i = pos >> 3
                e = dc[(((buf[i] << 16) | (buf[i + 1] << 8) | buf[i + 2]) >> (8 - (pos & 7))) & 0xFFFF]
                if e == 0:
                    raise Corrupt("code not in the table")
                pos += e >> 8
                s = e & 0xFF
                if s:
                    i = pos >> 3
                    val = ((((buf[i] << 16) | (buf[i + 1] << 8) | buf[i + 2]) >> (8 - (pos & 7))) & 0xFFFF) >> (16 - s)
                    pos += s
                    pred[ci] += val if val >= (1 << (s - 1)) else val - (1 << s) + 1
                blk[0] = pred[ci]
                k = 1
                while k < 64:
                    i = pos >> 3
                    e = ac[(((buf[i] << 16) | (buf[i + 1] << 8) | buf[i + 2]) >> (8 - (pos & 7))) & 0xFFFF]
                    if e == 0:
                        raise Corrupt("code not in the table")
                    pos += e >> 8
                    r, s = (e >> 4) & 15, e & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise Corrupt("coefficient index past 63")
                    i = pos >> 3
                    val = ((((buf[i] << 16) | (buf[i + 1] << 8) | buf[i + 2]) >> (8 - (pos & 7))) & 0xFFFF) >> (16 - s)
                    pos += s
                    blk[zz[k]] = val if val >= (1 << (s - 1)) else val - (1 << s) + 1
                    k += 1
                if pos > limit:
                    raise Corrupt("scan data ends early")
                out[ci][(my * c["v"] + v) * c["bw"] + mx * c["h"] + u] = blk
            mcu += 1
    if mcu < total:
        raise Corrupt("scan data ends early")
    return [o.reshape(c["bh"], c["bw"], 64) for o, c in zip(out, comps)]


def _idct_1d(v, shift):
    """The 8-point pass over the LAST axis of an int32 array (32-bit wrap-around), descaled by `shift`."""
    i = [v[..., k].astype(np.int32) for k in range(8)]
    c = np.int32
    with np.errstate(over="ignore"):
        z1 = (i[2] + i[6]) * c(4433)
        e2 = z1 - i[6] * c(15137)
        e3 = z1 + i[2] * c(6270)
        e0 = (i[0] + i[4]) << c(13)
        e1 = (i[0] - i[4]) << c(13)
        t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
        o0, o1, o2, o3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
        z5 = (z3 + z4) * c(9633)
        o0, o1, o2, o3 = o0 * c(2446), o1 * c(16819), o2 * c(25172), o3 * c(12299)
        z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
        o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
        outs = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
        half = c(1 << (shift - 1))
        return np.stack([(o + half) >> c(shift) for o in outs], axis=-1)


def idct_blocks(coef, quant):
    """coef [..., 64] int16 (natural order), quant [64] -> samples [..., 8, 8] uint8."""
    with np.errstate(over="ignore"):
        x = (coef.astype(np.int32) * quant.astype(np.int32)).reshape(coef.shape[:-1] + (8, 8))
    ws = np.swapaxes(_idct_1d(np.swapaxes(x, -1, -2), 11), -1, -2)         # columns
    out = _idct_1d(ws, 18)                                                   # rows
    with np.errstate(over="ignore"):
        return np.clip(out + np.int32(128), 0, 255).astype(np.uint8)


def planes(hdr, coefs):
    """One uint8 plane [8 bh, 8 bw] per component."""
    out = []
    for c, co in zip(hdr["comps"], coefs):
        s = idct_blocks(co, hdr["quant"][c["tq"]])                           # [bh, bw, 8, 8]
        out.append(np.ascontiguousarray(s.transpose(0, 2, 1, 3).reshape(8 * c["bh"], 8 * c["bw"])))
    return out


def upsample_h2v1(p):
    """[ch, cw] -> [ch, 2 cw]"""
    a = p.astype(np.int32)
    left = np.concatenate([a[:, :1], a[:, :-1]], axis=1)
    right = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)
    out = np.empty((a.shape[0], 2 * a.shape[1]), np.int32)
    out[:, 0::2] = (3 * a + left + 1) >> 2
    out[:, 1::2] = (3 * a + right + 2) >> 2
    out[:, 0] = a[:, 0]
    out[:, -1] = a[:, -1]
    return out


def upsample_h2v2(p):
    """[ch, cw] -> [2 ch, 2 cw]"""
    a = p.astype(np.int32)
    up = np.concatenate([a[:1], a[:-1]], axis=0)
    down = np.concatenate([a[1:], a[-1:]], axis=0)
    out = np.empty((2 * a.shape[0], 2 * a.shape[1]), np.int32)
    for parity, far in ((0, up), (1, down)):
        s = 3 * a + far
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[parity::2, 0::2] = (3 * s + left + 8) >> 4
        out[parity::2, 1::2] = (3 * s + right + 7) >> 4
        out[parity::2, 0] = (4 * s[:, 0] + 8) >> 4
        out[parity::2, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def pixels(hdr, pl):
    """[H, W] for one component, [H, W, 3] B, G, R for three."""
    H, W = hdr["height"], hdr["width"]
    if hdr["ncomp"] == 1:
        return pl[0][:H, :W].copy()
    full = []
    for c, p in zip(hdr["comps"][1:], pl[1:]):
        p = p[:c["ch"], :c["cw"]]
        if (hdr["hmax"], hdr["vmax"]) == (2, 1):
            p = upsample_h2v1(p)
        elif (hdr["hmax"], hdr["vmax"]) == (2, 2):
            p = upsample_h2v2(p)
        full.append(p[:H, :W].astype(np.int32) - 128)
    y = pl[0][:H, :W].astype(np.int32)
    cb, cr = full
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """(status, pixels or None)"""
    try:
        hdr = parse(data)
        return OK, pixels(hdr, planes(hdr, coefficients(data, hdr)))
    except Unsupported:
        return UNSUPPORTED, None
    except Corrupt:
        return CORRUPT, None


# ---- resize ----------------------------------------------------------------------------------------------------------------------
def resized_size(w, h, factor):
    """(ow, oh) = lrint(w f), lrint(h f) in double with f the float32 of the factor (round half to even, as lrint does)."""
    f = float(np.float32(factor))
    return int(np.rint(w * f)), int(np.rint(h * f))


def axis_table(n_out, n_in, factor):
    """(index, w1) per output position."""
    inv = 1.0 / float(np.float32(factor))
    f = (np.arange(n_out, dtype=np.float64) + 0.5) * inv - 0.5
    s = np.floor(f)
    a = f - s
    edge = (s < 0) | (s >= n_in - 1)
    a[edge] = 0.0
    s = np.clip(s, 0, n_in - 1).astype(np.int64)
    return s, np.rint(2048.0 * a).astype(np.int64)


def resize(img, factor):
    """The contract's bilinear resize of [h, w] or [h, w, c] uint8."""
    h, w = img.shape[:2]
    ow, oh = resized_size(w, h, factor)
    assert ow >= 1 and oh >= 1
    sx, wx1 = axis_table(ow, w, factor)
    sy, wy1 = axis_table(oh, h, factor)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    a = img.astype(np.int64).reshape(h, w, -1)
    wx1 = wx1[None, :, None]
    wy1 = wy1[:, None, None]
    top = (2048 - wx1) * a[sy][:, sx] + wx1 * a[sy][:, sx1]
    bot = (2048 - wx1) * a[sy1][:, sx] + wx1 * a[sy1][:, sx1]
    out = ((2048 - wy1) * top + wy1 * bot + (1 << 21)) >> 22
    return out.astype(np.uint8).reshape((oh, ow) + img.shape[2:])


def resize_float(img, factor):
    """The exact bilinear value at the same sampling positions, in float64 (not rounded)."""
    h, w = img.shape[:2]
    ow, oh = resized_size(w, h, factor)
    inv = 1.0 / float(np.float32(factor))

    def axis(n_out, n_in):
        f = (np.arange(n_out, dtype=np.float64) + 0.5) * inv - 0.5
        s = np.floor(f)
        a = f - s
        edge = (s < 0) | (s >= n_in - 1)
        a[edge] = 0.0
        s = np.clip(s, 0, n_in - 1).astype(np.int64)
        return s, np.minimum(s + 1, n_in - 1), a
    sx, sx1, ax = axis(ow, w)
    sy, sy1, ay = axis(oh, h)
    a = img.astype(np.float64).reshape(h, w, -1)
    ax, ay = ax[None, :, None], ay[:, None, None]
    top = (1 - ax) * a[sy][:, sx] + ax * a[sy][:, sx1]
    bot = (1 - ax) * a[sy1][:, sx] + ax * a[sy1][:, sx1]
    return ((1 - ay) * top + ay * bot).reshape((oh, ow) + img.shape[2:])
