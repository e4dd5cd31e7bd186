"""Writes tests/golden/png_small: about forty PNG files of a few hundred bytes to a few KB from the writer of tests/png_oracle.py, and
decoded.npz with the restatement's pixels of every decodable one.  Where Pillow is importable every decodable file is also decoded
by Pillow (convert("L" / "RGB"), >> 8 for 16-bit gray) and must agree; Pillow is not needed to run the tests.

    python tests/golden/make_png_golden.py

What the set covers: all 15 colour type / depth pairs; heights 1, 63, 64, 65 and 129 (the edges of the unfilter kernel's bands of 64
rows); widths 1, 2 and 3; a packed row that ends mid-byte at depth 1, 2 and 4; one file per filter type using it in every row;
random types per row; Paeth with all three tie-break branches; Average with a + b >= 256; stored, fixed and dynamic deflate blocks;
a match at distance 32768; IDAT in 1-byte chunks; a palette shorter than the indices used; ancillary chunks; and the refusals of
tests/png_cases.REFUSALS."""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_oracle as po  # noqa: E402

OUT = os.path.join(HERE, "png_small")


def build():
    rng = np.random.default_rng(20261019)
    files = {}

    def add(name, w, h, ct, depth, **kw):
        n_pal = kw.pop("n_palette", None)
        if ct == 3 and "palette" not in kw:
            kw["palette"] = po.random_palette(rng, n_pal or (1 << depth))
        samples = kw.pop("samples", None)
        if samples is None:
            samples = po.random_samples(rng, w, h, ct, depth)
        kw.setdefault("rng", rng)
        files[name] = po.write_png(samples, ct, depth, **kw)

    # all 15 pairs, the band edges, rows that end mid-byte
    add("t0_d1_13x65", 13, 65, 0, 1)
    add("t0_d2_13x63", 13, 63, 0, 2)
    add("t0_d4_13x64", 13, 64, 0, 4)
    add("t0_d8_37x129", 37, 129, 0, 8)
    add("t0_d16_37x70", 37, 70, 0, 16)
    add("t2_d8_37x70_two_idat", 37, 70, 2, 8, splits=(1000,))
    add("t2_d16_21x33", 21, 33, 2, 16)
    add("t3_d1_37x20", 37, 20, 3, 1)
    add("t3_d2_37x20", 37, 20, 3, 2)
    add("t3_d4_37x20", 37, 20, 3, 4)
    add("t3_d8_37x70", 37, 70, 3, 8)
    add("t4_d8_37x70", 37, 70, 4, 8)
    add("t4_d16_21x33", 21, 33, 4, 16)
    add("t6_d8_37x70", 37, 70, 6, 8)
    add("t6_d16_21x33", 21, 33, 6, 16)
    # height 1 and widths 1, 2, 3: the skew of the wavefront is wider than the row
    add("h1_t2_d8_50x1", 50, 1, 2, 8, filters=4)
    add("w1_t2_d8_1x70", 1, 70, 2, 8)
    add("w2_t6_d16_2x70", 2, 70, 6, 16)
    add("w3_t0_d8_3x70", 3, 70, 0, 8)
    # one filter type in every row, row 0 included
    for ft in range(5):
        bright = po.random_samples(rng, 29, 40, 2, 8) // 2 + 128 if ft == 3 else None          # Average with a + b >= 256
        add("f%d_t2_d8_29x40" % ft, 29, 40, 2, 8, filters=ft, samples=bright)
    # block types
    add("stored_t0_d8_40x30", 40, 30, 0, 8, mode="stored")
    # (zlib falls back to stored blocks for noise, and to a fixed block where that is shorter: a skewed alphabet makes each form win)
    skewed = lambda: rng.choice([0, 1, 2, 3, 50, 200], (30, 40, 3), p=[0.5, 0.2, 0.1, 0.1, 0.05, 0.05])
    add("fixed_t2_d8_40x30", 40, 30, 2, 8, mode="fixed", samples=skewed(), filters=0)
    add("dynamic_t2_d8_40x30", 40, 30, 2, 8, samples=skewed(), filters=0)
    # a match at distance 32768: 130 rows of 1 + 255 bytes, rows 128 and 129 repeat rows 0 and 1, everything between is zero
    img = np.zeros((130, 255, 1), np.int64)
    img[0] = rng.integers(0, 256, (255, 1))
    img[1] = rng.integers(0, 256, (255, 1))
    img[1, 254] = 0                                             # the run of zeros that follows starts as a copy of this byte
    img[128:130] = img[0:2]
    st = po.filter_rows(po.pack_rows(img, 8), 1, [0] * 130)
    tokens = list(st[:512]) + [(258, 1)] * ((32768 - 512) // 258) + [((32768 - 512) % 258, 1)] + [(258, 32768), (254, 32768)]
    add("dist32768_t0_d8_255x130", 255, 130, 0, 8, samples=img, filters=0, mode="tokens", tokens=tokens)
    add("idat1_t0_d8_20x10", 20, 10, 0, 8, splits="bytes")
    add("shortplte_t3_d8_30x20", 30, 20, 3, 8, n_palette=10)
    add("ancillary_t3_d4_20x20", 20, 20, 3, 4, before=[(b"gAMA", struct.pack(">I", 45455)), (b"sRGB", b"\0"), (b"tEXt", b"Comment\0png fixtures")],
        between=[(b"tRNS", bytes(range(16))), (b"bKGD", b"\x03")])
    # the refusals
    add("bad_interlaced", 20, 10, 2, 8, ihdr=dict(interlace=1))
    good = po.write_png(po.random_samples(rng, 20, 10, 2, 8), 2, 8, rng=rng)
    at = good.index(b"IDAT")
    files["bad_crc"] = good[:at + 10] + bytes([good[at + 10] ^ 0x40]) + good[at + 11:]
    files["bad_cut_file"] = good[:at + 40]
    add("bad_no_plte", 20, 10, 3, 8, palette=None)
    add("bad_depth3", 20, 10, 0, 4, ihdr=dict(depth=3))
    add("bad_adler", 20, 10, 2, 8, z_edit=lambda z: z[:-1] + bytes([z[-1] ^ 1]))
    add("bad_truncated_idat", 20, 10, 2, 8, z_edit=lambda z: z[:len(z) // 2])
    add("bad_filter5", 20, 10, 2, 8, filters=[0, 1, 2, 3, 4, 5, 0, 1, 2, 3])
    add("bad_surplus", 20, 10, 2, 8, stream_edit=lambda s: s + b"\0\0\0")
    return files


def pillow_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    ct = data[25]
    if ct in (0, 4):
        if im.mode.startswith("I;16") or im.mode == "I":
            return (np.asarray(im).astype(np.int64) >> 8).astype(np.uint8)
        return np.asarray(im.convert("L"))
    return np.asarray(im.convert("RGB"))[:, :, ::-1]


def main():
    import png_cases as pc
    files = build()
    assert sorted(n for n in files if n.startswith("bad_")) == sorted(pc.REFUSALS)
    os.makedirs(OUT, exist_ok=True)
    decoded = {}
    try:
        import PIL
        have_pillow = True
        print("cross-checking against Pillow", PIL.__version__)
    except ImportError:
        have_pillow = False
    for name, data in sorted(files.items()):
        status, px = po.decode(data)
        if name in pc.REFUSALS:
            assert (status, po.info(data)[0]) == pc.REFUSALS[name], (name, status, po.info(data)[0])
        else:
            assert status == po.OK, name
            decoded[name] = px
            if have_pillow:
                want = pillow_decode(data)
                assert want.shape == px.shape and np.array_equal(want, px), name
        with open(os.path.join(OUT, name + ".png"), "wb") as f:
            f.write(data)
        print("%-32s %6d bytes  status %d" % (name, len(data), status))
    np.savez_compressed(os.path.join(OUT, "decoded.npz"), **decoded)
    print("%d files, %d decodable, %d bytes" % (len(files), len(decoded), sum(len(d) for d in files.values())))


if __name__ == "__main__":
    main()
