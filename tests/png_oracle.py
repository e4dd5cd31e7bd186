"""The PNG contract of include/sfmba.h (sfmba_png_info, sfmba_png_decode) restated in numpy, plainly and slowly, and a small PNG WRITER
-- TEST INFRASTRUCTURE ONLY.  Standard library and numpy alone, so it runs wherever the tests run.

Reader:  walk(data) -> header dict (the chunk walk: signature, CRCs, IHDR, PLTE, the IDAT list, IEND, the size gate), status in ["status"]
         stream(data, hdr) -> (status, inflated scanline stream)        zlib.decompress stands in for the project's inflate
         unfilter(stream, hdr) -> [h, rowbytes] uint8                   the five predictors, byte by byte
         pixels(rows, hdr) -> [h, w] or [h, w, 3] (B, G, R) uint8
         decode(data) -> (status, pixels or None);  info(data) -> the tuple sfmba_png_info reports
Writer:  write_png(samples, colour_type, depth, ...) -> bytes           any accepted type / depth, a filter type per row (given or
         random), stored / fixed / dynamic deflate blocks or a token list of its own, IDAT split at given positions, ancillary chunks
         before and between, and the faults the refusal fixtures need."""
import struct
import zlib

import numpy as np

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 16384
PAIRS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ALL_PAIRS = [(ct, d) for ct in sorted(PAIRS) for d in PAIRS[ct]]


# ---- reader ---------------------------------------------------------------------------------------------------------------------------
def _refused(status):
    return dict(status=status)


def walk(data):
    """The chunk walk.  Returns a dict with "status"; the other keys exist only with OK."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        return _refused(CORRUPT)
    at, first, ended, unsupported = 8, True, False, False
    hdr, plte, idat, idat_open, idat_closed = None, None, [], False, False
    while not ended:
        if len(data) - at < 12:
            return _refused(CORRUPT)
        length, = struct.unpack(">I", data[at:at + 4])
        ctype = data[at + 4:at + 8]
        if length > 0x7FFFFFFF or length > len(data) - at - 12:
            return _refused(CORRUPT)
        body = data[at + 8:at + 8 + length]
        if zlib.crc32(data[at + 4:at + 8 + length]) != struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0]:
            return _refused(CORRUPT)
        if first != (ctype == b"IHDR"):
            return _refused(CORRUPT)
        if ctype != b"IDAT" and idat_open:
            idat_open, idat_closed = False, True
        if ctype == b"IHDR":
            if length != 13:
                return _refused(CORRUPT)
            w, h, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF:
                return _refused(CORRUPT)
            if ct not in PAIRS or depth not in PAIRS[ct] or comp != 0 or filt != 0 or lace > 1:
                return _refused(CORRUPT)
            if lace == 1 or w > MAX_SIDE or h > MAX_SIDE:
                unsupported = True
            else:
                s = SAMPLES[ct]
                rowbytes = (w * s * depth + 7) // 8
                hdr = dict(status=OK, width=w, height=h, bit_depth=depth, colour_type=ct, interlace=0, samples=s,
                           channels=1 if ct in (0, 4) else 3, bpp=max(1, s * depth // 8), rowbytes=rowbytes, stream_bytes=h * (1 + rowbytes))
            first = False
        elif ctype == b"PLTE":
            if plte is not None or idat_closed or idat or length == 0 or length % 3 or length > 768:
                return _refused(CORRUPT)
            plte = body
        elif ctype == b"IDAT":
            if idat_closed:
                return _refused(CORRUPT)
            idat_open = True
            idat.append(body)
        elif ctype == b"IEND":
            ended = True
        elif not ctype[0] & 0x20:
            unsupported = True
        at += length + 12
    if not idat:
        return _refused(CORRUPT)
    if unsupported:
        return _refused(UNSUPPORTED)
    if hdr["colour_type"] == 3 and plte is None:
        return _refused(CORRUPT)
    palette = np.zeros((256, 3), np.uint8)
    if hdr["colour_type"] == 3:
        palette[:len(plte) // 3] = np.frombuffer(plte, np.uint8).reshape(-1, 3)
    hdr["n_palette"] = len(plte) // 3 if hdr["colour_type"] == 3 else 0
    hdr["palette"] = palette
    hdr["idat"] = b"".join(idat)
    if hdr["stream_bytes"] > 1032 * len(hdr["idat"]) + 64:
        return _refused(CORRUPT)
    return hdr


def info(data):
    """(status, width, height, channels, bit_depth, colour_type, interlace) as sfmba_png_info reports it (zeros when refused)."""
    h = walk(data)
    if h["status"] != OK:
        return (h["status"], 0, 0, 0, 0, 0, 0)
    return (OK, h["width"], h["height"], h["channels"], h["bit_depth"], h["colour_type"], 0)


def stream(data, hdr):
    """(status, the inflated scanline stream) of a file whose walk ended OK."""
    z = hdr["idat"]
    if len(z) < 2 or z[0] & 15 != 8 or z[0] >> 4 > 7 or z[1] & 0x20 or (z[0] * 256 + z[1]) % 31:
        return CORRUPT, None
    d = zlib.decompressobj(15)
    try:
        out = d.decompress(z, hdr["stream_bytes"] + 1)
    except zlib.error:
        return CORRUPT, None
    if len(out) != hdr["stream_bytes"] or not d.eof:            # too short, too long, or the stream (Adler-32 included) did not end
        return CORRUPT, None
    stride = hdr["rowbytes"] + 1
    if max(out[0::stride]) > 4:
        return CORRUPT, None
    return OK, out


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a, 0
    if pb <= pc:
        return b, 1
    return c, 2


def unfilter(stream_bytes, hdr, branches=None):
    """[h, rowbytes] reconstructed bytes.  branches (a list of three counts) receives how often Paeth took a, b and c."""
    h, rb, bpp = hdr["height"], hdr["rowbytes"], hdr["bpp"]
    s = np.frombuffer(stream_bytes, np.uint8).reshape(h, rb + 1)
    rec = np.zeros((h, rb), np.uint8)
    zero = np.zeros(rb, np.int64)
    for y in range(h):
        ft = int(s[y, 0])
        x = s[y, 1:].astype(np.int64)
        up = rec[y - 1].astype(np.int64) if y else zero
        if ft == 0:
            row = x
        elif ft == 2:
            row = (x + up) & 255
        else:
            row = np.zeros(rb, np.int64)
            xl, ul, out = x.tolist(), up.tolist(), [0] * rb
            for i in range(rb):
                a = out[i - bpp] if i >= bpp else 0
                b = ul[i]
                c = ul[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    pred, which = paeth(a, b, c)
                    if branches is not None:
                        branches[which] += 1
                out[i] = (xl[i] + pred) & 255
            row = np.asarray(out, np.int64)
        rec[y] = row.astype(np.uint8)
    return rec


def pixels(rec, hdr):
    w, h, ct, depth, s = hdr["width"], hdr["height"], hdr["colour_type"], hdr["bit_depth"], hdr["samples"]
    if depth == 16:
        v = rec.reshape(h, w * s, 2)[:, :, 0]                  # the high byte
    elif depth == 8:
        v = rec
    else:
        bits = np.unpackbits(rec, axis=1)[:, :w * depth].reshape(h, w, depth)        # MSB first
        v = np.zeros((h, w), np.int64)
        for k in range(depth):
            v = v * 2 + bits[:, :, k]
    v = np.asarray(v, np.int64).reshape(h, w, s)
    if ct in (0, 4):
        scale = {1: 255, 2: 85, 4: 17}.get(depth, 1)
        return (v[:, :, 0] * scale).astype(np.uint8)
    if ct == 3:
        return hdr["palette"][v[:, :, 0]][:, :, ::-1].copy()   # entries at and past the PLTE length are zero
    return v[:, :, 2::-1].astype(np.uint8).copy()             # B, G, R; alpha dropped


def decode(data):
    hdr = walk(data)
    if hdr["status"] != OK:
        return hdr["status"], None
    status, st = stream(data, hdr)
    if status != OK:
        return status, None
    return OK, pixels(unfilter(st, hdr), hdr)


# ---- writer ---------------------------------------------------------------------------------------------------------------------------
def chunk(ctype, body, crc=None):
    c = zlib.crc32(ctype + body) if crc is None else crc
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", c & 0xFFFFFFFF)


def pack_rows(samples, depth):
    """[h, w, s] sample values (< 2^depth) -> [h, rowbytes] bytes as the file packs them."""
    samples = np.asarray(samples, np.int64)
    h = samples.shape[0]
    flat = samples.reshape(h, -1)
    if depth == 16:
        return np.stack([flat >> 8, flat & 255], axis=2).reshape(h, -1).astype(np.uint8)
    if depth == 8:
        return flat.astype(np.uint8)
    bits = ((flat[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1).astype(np.uint8)
    return np.packbits(bits, axis=1)                            # the last byte of a row is padded with zero bits


def filter_rows(raw, bpp, types):
    """The scanline stream of [h, rowbytes] bytes with filter type types[y] on row y."""
    h, rb = raw.shape
    r = raw.astype(np.int64)
    out = np.zeros((h, rb + 1), np.uint8)
    for y in range(h):
        a = np.concatenate([np.zeros(min(bpp, rb), np.int64), r[y, :max(rb - bpp, 0)]])
        b = r[y - 1] if y else np.zeros(rb, np.int64)
        c = np.concatenate([np.zeros(min(bpp, rb), np.int64), b[:max(rb - bpp, 0)]])
        ft = int(types[y])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) >> 1
        elif ft == 4:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:
            pred = 0                                            # an illegal type byte, for the refusal fixtures
        out[y, 0] = ft
        out[y, 1:] = (r[y] - pred) & 255
    return out.tobytes()


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def deflate_tokens(tokens):
    """One final fixed-Huffman block from a token list: an int is a literal, (length, distance) a match.  zlib's own compressor never
    writes a distance above 32506, so the distance-32768 fixture comes from here."""
    acc, n, out = 0, 0, bytearray()

    def put(value, bits):                                       # LSB first
        nonlocal acc, n
        acc |= value << n
        n += bits
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8

    def code(value, bits):                                      # a Huffman code goes in MSB first
        put(int(format(value, "0%db" % bits)[::-1], 2), bits)

    def literal(sym):
        if sym < 144:
            code(0x30 + sym, 8)
        elif sym < 256:
            code(0x190 + sym - 144, 9)
        elif sym < 280:
            code(sym - 256, 7)
        else:
            code(0xC0 + sym - 280, 8)

    put(1, 1)
    put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            li = max(i for i in range(29) if _LEN_BASE[i] <= length and (i < 28 or length == 258))
            if length == 258:
                li = 28
            literal(257 + li)
            put(length - _LEN_BASE[li], _LEN_EXTRA[li])
            di = max(i for i in range(30) if _DIST_BASE[i] <= dist)
            code(di, 5)
            put(dist - _DIST_BASE[di], _DIST_EXTRA[di])
        else:
            literal(int(t))
    literal(256)
    if n:
        put(0, 8 - n)
    return bytes(out)


def zlib_stream(raw, mode="dynamic", tokens=None):
    """mode: "stored" (level 0), "fixed" (Z_FIXED), "dynamic" (level 9), "tokens" (deflate_tokens over `tokens`)."""
    if mode == "tokens":
        return b"\x78\x9c" + deflate_tokens(tokens) + struct.pack(">I", zlib.adler32(raw))
    if mode == "stored":
        c = zlib.compressobj(0)
    elif mode == "fixed":
        c = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    else:
        c = zlib.compressobj(9)
    return c.compress(raw) + c.flush()


def write_png(samples, colour_type, depth, filters=None, rng=None, mode="dynamic", tokens=None, splits=(), palette=None, before=(), between=(),
              ihdr=None, stream_edit=None, z_edit=None, with_iend=True):
    """samples [h, w, s] (or [h, w] for one sample per pixel), values below 2^depth.
    filters      a type per row, one type for all rows, or None for random types from rng
    mode         see zlib_stream
    splits       positions at which the zlib stream is cut into IDAT chunks; "bytes" = one chunk per byte
    palette      [n, 3] R, G, B: a PLTE chunk
    before       (type, body) ancillary chunks between IHDR and PLTE;  between: those between PLTE and the first IDAT
    ihdr         fields of IHDR to overwrite (width, height, depth, colour_type, interlace), stream_edit / z_edit: functions on the
                 scanline stream before deflate / on the zlib stream after it -- for the refusal fixtures"""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w, s = samples.shape
    assert s == SAMPLES[colour_type] and depth in PAIRS[colour_type]
    raw = pack_rows(samples, depth)
    bpp = max(1, s * depth // 8)
    if filters is None:
        types = (rng or np.random.default_rng(0)).integers(0, 5, h)
    elif np.isscalar(filters):
        types = [int(filters)] * h
    else:
        types = list(filters)
    st = filter_rows(raw, bpp, types)
    if stream_edit:
        st = stream_edit(st)
    z = zlib_stream(st, mode, tokens)
    if z_edit:
        z = z_edit(z)
    f = dict(width=w, height=h, depth=depth, colour_type=colour_type, interlace=0)
    f.update(ihdr or {})
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", f["width"], f["height"], f["depth"], f["colour_type"], 0, 0, f["interlace"]))
    for ctype, body in before:
        out += chunk(ctype, body)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    for ctype, body in between:
        out += chunk(ctype, body)
    cuts = list(range(1, len(z))) if splits == "bytes" else [c for c in splits if 0 < c < len(z)]
    edges = [0] + cuts + [len(z)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        out += chunk(b"IDAT", z[lo:hi])
    if with_iend:
        out += chunk(b"IEND", b"")
    return out


def random_samples(rng, w, h, colour_type, depth):
    return rng.integers(0, 1 << depth, (h, w, SAMPLES[colour_type]))


def random_palette(rng, n):
    return rng.integers(0, 256, (n, 3)).astype(np.uint8)
