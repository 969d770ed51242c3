"""Level 1 of the PNG encoder on the host: the twin (yogo_amd.png_encode.encode_png_host(level=1)) against zlib, PIL and the
repository's own pure-Python inflate; what each small case exercises, from the twin's tokens; the Huffman limits over the two new
alphabets; the size the level is for; the public surface.  No GPU."""
import io
import struct
import zlib

import numpy as np
import pytest

import _draw_ref as R
import _png_match_cases as M
from yogo_amd import png_encode as E

CASES = M.match_cases()


@pytest.fixture(scope="module")
def encoded():
    """{name: (file, stored per band, tokens per band)} at level 1, made once"""
    return {name: E.encode_png_host(px, level=1, return_bands=True, return_tokens=True) for name, px in CASES.items()}


def _idat(png: bytes) -> bytes:
    assert png[:8] == E.SIGNATURE
    at, out = 8, b""
    while at < len(png):
        (n,), kind = struct.unpack(">I", png[at: at + 4]), png[at + 4: at + 8]
        assert zlib.crc32(png[at + 4: at + 8 + n]) & 0xFFFFFFFF == struct.unpack(">I", png[at + 8 + n: at + 12 + n])[0]
        if kind == b"IDAT":
            out += png[at + 8: at + 8 + n]
        at += 12 + n
    return out


def _matches(tokens):
    """[m, 2] (length, distance) of every match of a file"""
    rows = [t[t[:, 2] > 0][:, 1:] for t in tokens]
    return np.concatenate(rows) if rows else np.zeros((0, 2), dtype=np.int64)


@pytest.mark.parametrize("name", list(CASES))
def test_round_trip(encoded, name):
    from PIL import Image

    from yogo_amd import inflate

    px = CASES[name]
    H, W, bpp = px.shape
    png = encoded[name][0]
    scan = E.filter_scanlines(px).tobytes()
    stream = _idat(png)
    assert zlib.decompress(stream) == scan
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert np.array_equal(got.reshape(H, W, bpp), px)
    off, length, adler = inflate.split_zlib(stream)
    assert inflate.inflate_status(stream[off: off + length], len(scan), adler) == (0, scan)
    assert len(png) <= E.encode_bound(H, W, bpp)


def test_level_0_is_untouched():
    rendered = np.random.default_rng(5).integers(0, 256, (48, 64, 4), dtype=np.uint8)
    for name, px in R.encoder_cases(rendered).items():
        assert E.encode_png_host(px) == E.encode_png_host(px, level=0), name
        assert E.encode_png_host(px, return_bands=True) == E.encode_png_host(px, level=0, return_bands=True), name
    with pytest.raises(ValueError):
        E.encode_png_host(rendered, level=2)


def test_constant_is_overlapping_copies_cut_at_piece_ends(encoded):
    _, stored, tokens = encoded["constant"]
    assert stored == [False] * 3
    m = _matches(tokens)
    assert (m[:, 1] < m[:, 0]).any() and m[:, 1].min() == 4, "a constant row is a copy from inside itself, one pixel back"
    # (a scanline of 257 bytes starts with its filter type, which no candidate of this shape repeats: no match is longer than the
    # rest of its row; 258 is the `runs` case's)
    assert 248 <= m[:, 0].max() <= 256
    for t in tokens:   # no match passes its piece's end, and one ends on it in every piece
        ends = t[:, 0] + t[:, 1]
        assert (t[:, 0] // E.PIECE == (ends - 1) // E.PIECE).all()
        assert set(range(E.PIECE, int(ends.max()) + 1, E.PIECE)) <= set(ends.tolist())


def test_one_pixel_has_no_match(encoded):
    _, stored, tokens = encoded["one_pixel"]
    assert stored == [True] and len(tokens[0]) == 0   # five bytes do not pay a header: stored, as at level 0
    assert encoded["one_pixel"][0] == E.encode_png_host(CASES["one_pixel"])


def test_runs_sit_on_both_sides_of_every_length_boundary(encoded):
    _, stored, tokens = encoded["runs"]
    assert stored == [False]
    lengths = set(_matches(tokens)[:, 0].tolist())
    for pair in ((10, 11), (18, 19), (34, 35), (66, 67), (130, 131), (257, 258)):
        assert set(pair) <= lengths, pair
    assert set(M.RUN_TARGETS) <= lengths


def test_repeats_sit_on_both_sides_of_every_distance_boundary(encoded):
    for name, want in (("distances_bpp1", M.DISTANCES_BPP1), ("distances_bpp4", M.DISTANCES_BPP4)):
        _, stored, tokens = encoded[name]
        assert stored == [False]
        assert set(want) <= set(_matches(tokens)[:, 1].tolist()), name
    assert 1 in M.DISTANCES_BPP1 and E.WINDOW in M.DISTANCES_BPP1 and 4 * E.WINDOW in M.DISTANCES_BPP4


def test_single_match_gives_a_single_distance_code(encoded):
    png, stored, tokens = encoded["single_match"]
    assert stored == [False] and len(_matches(tokens)) == 1
    data = np.frombuffer(E.filter_scanlines(CASES["single_match"]).tobytes(), dtype=np.uint8)
    body, st, _ = E.encode_band_matches(data.tobytes(), 1, True)
    assert not st and zlib.decompress(E.ZLIB_HEADER + body + struct.pack(">I", zlib.adler32(data.tobytes()))) == data.tobytes()


def test_a_band_without_a_match_is_coded_with_one_empty_distance_code():
    """32 values in an order that repeats no triple within reach: coded, no match, HDIST = 0"""
    data = (np.random.default_rng(0).integers(0, 32, 600, dtype=np.uint8) * 8).tobytes()
    body, stored, tok = E.encode_band_matches(data, 1, True)
    assert not stored and len(tok) == 600 and (tok[:, 2] == 0).all()
    assert body[0] >> 3 == 29 and body[1] & 31 == 0   # HLIT 29 (286 codes), HDIST 0 (one code)
    assert zlib.decompress(E.ZLIB_HEADER + body + struct.pack(">I", zlib.adler32(data))) == data


def test_cases_use_every_length_and_distance_symbol(encoded):
    m = np.concatenate([_matches(tokens) for _, _, tokens in encoded.values()])
    assert m[:, 0].min() >= E.MIN_MATCH and m[:, 0].max() == E.MAX_MATCH
    assert {E.length_symbol(int(v)) for v in m[:, 0]} == set(range(29))
    reach = {E.distance_symbol(bpp * k) for bpp in (1, 2, 3, 4) for k in range(1, E.WINDOW + 1)}
    assert reach == set(range(16))
    assert {E.distance_symbol(int(v)) for v in m[:, 1]} == reach


def test_ragged_bands(encoded):
    assert len(encoded["ragged_height"][1]) == 3 and len(encoded["last_band_one_row"][1]) == 2
    assert len(encoded["last_band_one_row"][2][1]) > 0   # the band of one row is coded
    assert encoded["wide_band"][1] == [True, False]
    t = encoded["wide_band"][2][1]
    assert 16 * 4121 > E.MAX_STORED and (t[:, 2] > 0).any()


def test_no_candidate_from_the_row_above_when_a_scanline_passes_the_window(encoded):
    px = CASES["long_rows"]
    assert px.shape[1] * px.shape[2] + 1 > 32768
    _, stored, tokens = encoded["long_rows"]
    assert stored == [False]
    m = _matches(tokens)
    assert len(m) and m[:, 1].max() <= 4 * E.WINDOW
    for t in tokens:   # nothing reaches back before the band's first byte
        assert (t[:, 0] - t[:, 2] >= 0).all()


@pytest.mark.parametrize("name,bpp", [("grey", 1), ("grey_alpha", 2), ("rgb", 3)])
def test_other_pixel_sizes_step_by_the_pixel(encoded, name, bpp):
    _, stored, tokens = encoded[name]
    m = _matches(tokens)
    assert not any(stored) and len(m) and (m[:, 1] % bpp == 0).all() and m[:, 1].max() <= bpp * E.WINDOW


def test_noise_is_the_file_of_level_0(encoded):
    png, stored, _ = encoded["noise"]
    assert all(stored) and png == E.encode_png_host(CASES["noise"]) and len(png) == E.encode_bound(48, 64, 4)


@pytest.mark.parametrize("nsym", [286, 30])
def test_huffman_limits_hold_for_fibonacci_counts(nsym):
    fib = [1, 1]
    while len(fib) < nsym:
        fib.append(min(fib[-1] + fib[-2], 1 << 40))
    rng = np.random.default_rng(nsym)
    for counts in (fib, fib[::-1], list(rng.permutation(fib)), fib[:40] + [0] * (nsym - 40) if nsym > 40 else fib[:20] + [0] * (nsym - 20)):
        lens = E.huffman_lengths(counts, E.LIT_LIMIT)
        used = [b for b, f in zip(lens, counts) if f]
        assert len(lens) == nsym and all(1 <= b <= 15 for b in used) and all(b == 0 for b, f in zip(lens, counts) if not f)
        assert sum(1 << (15 - b) for b in used) == 1 << 15
        codes = E.canonical_codes(lens, E.LIT_LIMIT)
        assert len({(c, b) for c, b in zip(codes, lens) if b}) == len(used)


def test_size_condition_on_the_benchmark_frame():
    """rows 0 .. 63 of the benchmark's first frame: at most 0.70 of level 0 (pieces of 16 bytes give 0.72) and at most 1.25 of
    PIL's compress_level=1 file (they give 1.30)"""
    from PIL import Image

    px = M.bench_frame_rows(64)
    level0, level1 = len(E.encode_png_host(px)), len(E.encode_png_host(px, level=1))
    buf = io.BytesIO()
    Image.fromarray(px, mode="RGBA").save(buf, format="PNG", compress_level=1)
    pil = len(buf.getvalue())
    print(f"level 0 {level0}, level 1 {level1}, PIL {pil}: {level1 / level0:.3f} of level 0, {level1 / pil:.3f} of PIL")
    assert level1 <= 0.70 * level0
    assert level1 <= 1.25 * pil


def test_public_surface():
    import inspect
    import re
    from pathlib import Path

    from yogo_amd import draw
    from yogo_amd.infer import predict
    from yogo_amd.utils.argparsers import global_parser

    header = (Path(__file__).resolve().parent.parent / "include" / "yogo_hip.h").read_text()
    assert re.search(r"int yogo_png_encode_bound_level\(int H, int W, int bpp, int level, size_t\* slot_bytes, size_t\* work_bytes\);", header)
    assert re.search(r"int yogo_png_encode_level\(const unsigned char\* pixels, int B, int H, int W, int bpp, int level,", header)
    assert "int yogo_png_encode_bound(int H, int W, int bpp, size_t* slot_bytes, size_t* work_bytes);" in header
    assert inspect.signature(E.encode_png_host).parameters["level"].default == 0
    assert inspect.signature(E.encode_png_host).parameters["return_tokens"].default is False
    for fn in (draw.encode_bound, draw.encode_png, draw.DrawSink.__init__):
        assert inspect.signature(fn).parameters["level"].default == 0
    assert inspect.signature(predict).parameters["device_draw_level"].default == 0
    assert (E.PIECE, E.WINDOW, E.MIN_MATCH, E.MAX_MATCH) == (512, 64, 3, 258)

    parser = global_parser()
    base = ["infer", "m.pth", "--path-to-images", "imgs", "--draw-boxes", "--output-dir", "out"]
    assert parser.parse_args(base + ["--device-draw"]).device_draw_level == 0
    assert parser.parse_args(base + ["--device-draw", "--device-draw-level", "1"]).device_draw_level == 1
    for bad in (base + ["--device-draw-level", "1"],                                                    # without --device-draw
                base + ["--device-draw", "--device-draw-level", "2"],
                base + ["--device-draw", "--device-draw-level", "1", "--output-img-filetype", ".tif"],
                base + ["--device-draw", "--device-draw-level", "1", "--output-img-filetype", ".tiff"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    for kw in (dict(device_draw=False, device_draw_level=1), dict(device_draw=True, device_draw_level=2),
               dict(device_draw=True, device_draw_level=1, output_img_ftype=".tif"),
               dict(device_draw=True, device_draw_level=1, output_img_ftype=".tiff")):
        with pytest.raises(ValueError):   # (raised before the checkpoint is opened or a device touched)
            predict("no_such.pth", path_to_images="imgs", draw_boxes=True, output_dir="out_never_made", **kw)
    with pytest.raises(ValueError):
        draw.check_level(True)
