"""CPU-side checks of the PNG reader's contract (include/sfmba.h: sfmba_png_info, sfmba_png_decode): no GPU needed.

  restatement     tests/png_oracle.py (chunk walk, zlib.decompress, the five predictors, the sample rules) equals the stored pixels of
                  every decodable file of tests/golden/png_small, and Pillow's decode where Pillow is importable; the fixtures cover
                  what their names say (all 15 pairs, every filter type, the three Paeth branches, Average with a 9-bit sum, stored /
                  fixed / dynamic blocks, a distance of 32768)
  host program    tools/micro/png_math_host.hip (csrc/png_inflate.cpp and csrc/png_math.h, the arithmetic the kernels run, compiled
                  for the host) equals the restatement in the inflated stream, the unfiltered bytes and the pixels, and in the status
                  of every refusal
  C ABI           sfmba_png_info through ctypes: geometry of every fixture, the status of every refusal as far as the chunk walk can
                  know it, further malformed files, the 1032x size gate
  program         the usage text of sfmtoy names png
  symbols         the libraries export the new entry points"""
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as pc
import png_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-toy-library_amd", "csrc")


@pytest.fixture(scope="module")
def decoded_small():
    """name -> (header, stream, unfiltered rows, pixels) of the restatement, computed once."""
    out = {}
    for name in pc.decodable_names():
        data = pc.small_file(name)
        hdr = po.walk(data)
        assert hdr["status"] == po.OK, name
        status, st = po.stream(data, hdr)
        assert status == po.OK, name
        rec = po.unfilter(st, hdr)
        out[name] = (hdr, st, rec, po.pixels(rec, hdr))
    return out


# ---- the restatement and the fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.decodable_names())
def test_restatement_equals_the_stored_pixels(decoded_small, name):
    px = decoded_small[name][3]
    want = pc.small_pixels(name)
    assert px.dtype == np.uint8 and px.shape == want.shape and np.array_equal(px, want), name


def test_restatement_equals_pillow(decoded_small):
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow is not importable here")
    for name in pc.decodable_names():
        data = pc.small_file(name)
        im = Image.open(io.BytesIO(data))
        hdr = decoded_small[name][0]
        if hdr["colour_type"] in (0, 4):
            want = (np.asarray(im).astype(np.int64) >> 8).astype(np.uint8) if im.mode.startswith("I") else np.asarray(im.convert("L"))
        else:
            want = np.asarray(im.convert("RGB"))[:, :, ::-1]
        assert np.array_equal(decoded_small[name][3], want), name


def test_fixtures_cover_what_the_issue_lists(decoded_small):
    hdrs = {n: v[0] for n, v in decoded_small.items()}
    assert {(h["colour_type"], h["bit_depth"]) for h in hdrs.values()} == set(po.ALL_PAIRS) and len(po.ALL_PAIRS) == 15
    assert {1, 63, 64, 65, 129} <= {h["height"] for h in hdrs.values()}
    assert {1, 2, 3} <= {h["width"] for h in hdrs.values()}
    for depth in (1, 2, 4):                                            # a packed row that ends mid-byte
        assert any(h["bit_depth"] == depth and (h["width"] * depth) % 8 for h in hdrs.values()), depth
    assert {h["bpp"] for h in hdrs.values()} == {1, 2, 3, 4, 6, 8}
    for ft in range(5):
        hdr, st = decoded_small["f%d_t2_d8_29x40" % ft][:2]
        assert set(st[0::hdr["rowbytes"] + 1]) == {ft}
    types = set()
    for hdr, st, _, _ in decoded_small.values():
        types |= set(st[0::hdr["rowbytes"] + 1])
    assert types == {0, 1, 2, 3, 4}
    # Paeth: all three tie-break branches
    hdr, st = decoded_small["f4_t2_d8_29x40"][:2]
    branches = [0, 0, 0]
    po.unfilter(st, hdr, branches)
    print("Paeth took a, b, c %s times" % branches)
    assert min(branches) > 0
    # Average: the 9-bit sum
    hdr, st, rec, _ = decoded_small["f3_t2_d8_29x40"]
    r = rec.astype(np.int64)
    assert ((r[1:, :-3] + r[:-1, 3:]) >= 256).any()
    # block types: the first block of each stream
    first = {n: (po.walk(pc.small_file(n))["idat"][2] >> 1) & 3 for n in ("stored_t0_d8_40x30", "fixed_t2_d8_40x30", "dynamic_t2_d8_40x30")}
    assert first == {"stored_t0_d8_40x30": 0, "fixed_t2_d8_40x30": 1, "dynamic_t2_d8_40x30": 2}
    # the distance-32768 file: rows 128 and 129 repeat rows 0 and 1 and the stream is far shorter than 32768 bytes
    px = pc.small_pixels("dist32768_t0_d8_255x130")
    assert np.array_equal(px[128:130], px[0:2]) and px[0].any() and not px[2:128].any() and len(pc.small_file("dist32768_t0_d8_255x130")) < 1000
    assert pc.small_file("idat1_t0_d8_20x10").count(b"IDAT") > 200
    hdr, _, rec, px = decoded_small["shortplte_t3_d8_30x20"]
    assert hdr["n_palette"] == 10 and rec.max() > 10 and not px[rec >= 10].any()
    assert b"gAMA" in pc.small_file("ancillary_t3_d4_20x20") and b"tRNS" in pc.small_file("ancillary_t3_d4_20x20")


def test_restatement_reports_the_refusals():
    for name, (status, walk_status) in pc.REFUSALS.items():
        data = pc.small_file(name)
        assert po.decode(data) == (status, None), name
        assert po.info(data)[0] == walk_status, name


# ---- the device arithmetic and the inflate on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("png") / "png_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "png_math_host.hip"), os.path.join(CSRC, "png_inflate.cpp")])
    return exe


def host_decode(exe, tmp_path, data):
    """(status, stream, unfiltered rows, pixels) as the host program writes them."""
    src, dst = tmp_path / "in.png", tmp_path / "out.bin"
    src.write_bytes(data)
    subprocess.check_call([exe, "decode", str(src), str(dst)])
    raw = dst.read_bytes()
    head = np.frombuffer(raw[:32], np.int32)
    if head[0] != 0:
        assert len(raw) == 32 and not head[1:].any()
        return int(head[0]), None, None, None
    w, h, ch, _, _, rb, _ = (int(v) for v in head[1:])
    n_stream, n_rec = h * (rb + 1), h * rb
    st = raw[32:32 + n_stream]
    rec = np.frombuffer(raw[32 + n_stream:32 + n_stream + n_rec], np.uint8).reshape(h, rb)
    px = np.frombuffer(raw[32 + n_stream + n_rec:], np.uint8).reshape((h, w) if ch == 1 else (h, w, 3))
    return 0, st, rec, px


@pytest.mark.parametrize("name", pc.decodable_names())
def test_host_inflate_and_device_arithmetic_against_the_restatement(host_exe, tmp_path, decoded_small, name):
    hdr, st, rec, px = decoded_small[name]
    status, hst, hrec, hpx = host_decode(host_exe, tmp_path, pc.small_file(name))
    assert status == 0
    assert hst == st, (name, "inflated stream")
    assert np.array_equal(hrec, rec), (name, "unfiltered bytes")
    assert hpx.shape == px.shape and np.array_equal(hpx, px), (name, "pixels")


def test_host_program_refuses_what_the_restatement_refuses(host_exe, tmp_path):
    for name, (status, _) in pc.REFUSALS.items():
        assert host_decode(host_exe, tmp_path, pc.small_file(name))[0] == status, name


def _idat_edit(data, edit):
    """The file with its (single) zlib stream replaced by edit(stream), chunk CRCs rewritten."""
    hdr = po.walk(data)
    at = data.index(b"IDAT") - 4
    end = data.index(b"IEND") - 4
    return data[:at] + po.chunk(b"IDAT", edit(hdr["idat"])) + data[end:]


def test_host_inflate_refuses_malformed_zlib_and_deflate_streams(host_exe, tmp_path):
    """Each of these keeps every chunk CRC right, so that it is the zlib wrapper or the inflate that has to refuse."""
    data = pc.small_file("dynamic_t2_d8_40x30")
    raw = zlib.decompress(po.walk(data)["idat"])
    adler = struct.pack(">I", zlib.adler32(raw))
    cases = {
        "method 7": lambda z: bytes([0x77, 0x01 + (31 - (0x7701 % 31)) % 31]) + z[2:],
        "window 64 K": lambda z: bytes([0x88, (31 - (0x8800 % 31)) % 31]) + z[2:],
        "preset dictionary": lambda z: bytes([0x78, 0x20 + (31 - (0x7820 % 31)) % 31]) + z[2:],
        "header check bits": lambda z: bytes([z[0], z[1] ^ 1]) + z[2:],
        "reserved block type": lambda z: z[:2] + b"\x07" + z[3:],
        "stored length check": lambda z: z[:2] + b"\x01\x05\x00\x05\x00" + raw[:5] + adler,
        "distance before the start": lambda z: z[:2] + po.deflate_tokens([1, 2, 3, (3, 4)] + list(raw[6:])) + adler,
        "stream ends early": lambda z: z[:len(z) - 9],
        "one byte too few": lambda z: z[:2] + po.deflate_tokens(list(raw[:-1])) + struct.pack(">I", zlib.adler32(raw[:-1])),
        "one byte too many": lambda z: z[:2] + po.deflate_tokens(list(raw) + [0]) + struct.pack(">I", zlib.adler32(raw + b"\0")),
        # a dynamic block whose code-length code is over-subscribed: HLIT 0, HDIST 0, HCLEN 15 (19 lengths), all of them 4
        "over-subscribed code": lambda z: z[:2] + bytes([0x05, 0xE0]) + b"\x49\x92\x24" * 3 + adler,
    }
    for what, edit in cases.items():
        bad = _idat_edit(data, edit)
        assert po.info(bad)[0] == po.OK, what                          # the chunk walk has nothing to object to
        assert po.decode(bad)[0] == po.CORRUPT, what
        assert host_decode(host_exe, tmp_path, bad)[0] == po.CORRUPT, what
    same = _idat_edit(data, lambda z: z[:2] + po.deflate_tokens(list(raw)) + adler + b"trailing bytes")
    status, _, _, px = host_decode(host_exe, tmp_path, same)
    assert status == 0 and np.array_equal(px, pc.small_pixels("dynamic_t2_d8_40x30"))


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    return capi


KEYS = ("status", "width", "height", "channels", "bit_depth", "colour_type", "interlace")


def test_png_info_reports_the_geometry_of_every_fixture_and_every_refusal(capi):
    names = pc.small_names()
    infos = capi.png_info([pc.small_file(n) for n in names])
    for n, d in zip(names, infos):
        want = po.info(pc.small_file(n))
        assert tuple(d[k] for k in KEYS) == want, n
        if n in pc.REFUSALS:
            assert d["status"] == pc.REFUSALS[n][1], n
            if d["status"] != 0:
                assert not any(d[k] for k in KEYS[1:]), n
        else:
            assert d["status"] == 0 and (d["height"], d["width"]) == pc.small_pixels(n).shape[:2]
            assert d["channels"] == (1 if pc.small_pixels(n).ndim == 2 else 3), n
    assert capi.png_info([]) == []


def test_png_info_refuses_what_is_broken_in_the_chunks(capi):
    data = pc.small_file("t3_d4_37x20")
    ihdr, plte, idat, iend = data.index(b"IHDR") - 4, data.index(b"PLTE") - 4, data.index(b"IDAT") - 4, data.index(b"IEND") - 4
    plte_chunk, idat_chunk = data[plte:idat], data[idat:iend]
    text = po.chunk(b"tEXt", b"k\0v")

    def with_ihdr(**f):
        w, h, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", data[ihdr + 8:ihdr + 21])
        v = dict(w=w, h=h, depth=depth, ct=ct, comp=comp, filt=filt, lace=lace)
        v.update(f)
        return data[:ihdr] + po.chunk(b"IHDR", struct.pack(">IIBBBBB", v["w"], v["h"], v["depth"], v["ct"], v["comp"], v["filt"], v["lace"])) + data[plte:]

    files = [
        (data, 0), (b"", 2), (data[:7], 2), (b"\x88" + data[1:], 2),                                      # the file; no or a bad signature
        (data[:8] + text + data[8:], 2),                                                                  # IHDR not first
        (data[:plte] + data[ihdr:plte] + data[plte:], 2),                                                 # IHDR twice
        (data[:ihdr] + po.chunk(b"IHDR", data[ihdr + 8:ihdr + 20]) + data[plte:], 2),                     # IHDR of 12 bytes
        (with_ihdr(w=0), 2), (with_ihdr(h=0), 2), (with_ihdr(depth=16), 2), (with_ihdr(ct=5), 2),
        (with_ihdr(comp=1), 2), (with_ihdr(filt=1), 2), (with_ihdr(lace=2), 2), (with_ihdr(lace=1), 1),
        (with_ihdr(w=16385), 1), (with_ihdr(w=16384, h=16384), 2),                                        # too wide; the size gate (134 MB from a few hundred bytes)
        (data[:idat] + po.chunk(b"PLTE", b"\0" * 10) + data[idat:], 2),                                   # a second PLTE, and not a multiple of 3
        (data[:plte] + po.chunk(b"PLTE", b"\0" * 771) + data[idat:], 2), (data[:plte] + po.chunk(b"PLTE", b"") + data[idat:], 2),
        (data[:plte] + data[idat:iend] + plte_chunk + data[iend:], 2),                                    # PLTE after IDAT
        (data[:idat] + data[iend:], 2),                                                                   # no IDAT
        (data[:iend] + text + idat_chunk + data[iend:], 2),                                               # IDAT chunks not consecutive
        (data[:iend], 2), (data[:iend + 11], 2),                                                          # IEND missing or cut
        (data[:idat] + struct.pack(">I", 0x80000000) + data[idat + 4:], 2),                               # a chunk length past everything
        (data[:idat] + text + po.chunk(b"tIME", b"1234567") + data[idat:] + b"bytes after IEND", 0),     # ancillary chunks are skipped
        (data[:idat] + po.chunk(b"FRAm", b"") + data[idat:], 1),                                          # a critical chunk nobody knows
    ]
    status = [d["status"] for d in capi.png_info([f for f, _ in files])]
    assert status == [s for _, s in files]
    assert [po.info(f)[0] for f, _ in files] == status


def test_an_image_its_file_cannot_hold_is_corrupt_before_anything_is_sized(capi):
    """A file of a few hundred bytes that declares 16384 x 16384 x 8 bytes (2 GB of scanlines): a deflate stream expands at most 1032
    times, so the walk refuses it; at the gate itself the walk accepts."""
    data = pc.small_file("h1_t2_d8_50x1")
    ihdr = data.index(b"IHDR") - 4
    huge = data[:ihdr] + po.chunk(b"IHDR", struct.pack(">IIBBBBB", 16384, 16384, 16, 6, 0, 0, 0)) + data[ihdr + 25:]
    assert len(huge) < 300 and capi.png_info([huge, data]) == [dict.fromkeys(KEYS, 0) | dict(status=2), capi.png_info([data])[0]]
    limit = 1032 * len(po.walk(data)["idat"]) + 64                     # height x (1 + rowbytes) may reach this and no more
    rows = limit // 16                                                 # gray, 8 bits, 15 wide: 16 bytes of stream per row
    assert rows < 16384
    for h, want in ((rows, 0), (rows + 1, 2)):
        f = data[:ihdr] + po.chunk(b"IHDR", struct.pack(">IIBBBBB", 15, h, 8, 0, 0, 0, 0)) + data[ihdr + 25:]
        assert (16 * h > limit) == (want == 2)
        assert capi.png_info([f])[0]["status"] == want and po.info(f)[0] == want, h


# ---- the program and the symbols --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_dir():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    return os.path.join(ROOT, "sfm-toy-library_amd", "host")


def test_sfmtoy_usage_names_png(host_dir):
    ok = subprocess.run([os.path.join(host_dir, "sfmtoy"), "-h"], capture_output=True, text=True)
    assert ok.returncode == 0 and ".png" in ok.stdout and ".jpg" in ok.stdout


def test_libraries_export_the_symbols(host_dir):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(CSRC, "libsfmba_hip.so")]).decode()
    for sym in ("sfmba_png_info", "sfmba_png_decode", "sfmba_jpeg_info", "sfmba_jpeg_decode", "sfmba_resize_images"):
        assert " T %s\n" % sym in exported, sym
    hdr = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert "#define SFMBA_ABI_VERSION 6" in hdr and "sfmba_png_decode(" in hdr
    assert ".png" in open(os.path.join(host_dir, "SfM.h")).read()
