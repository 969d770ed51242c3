"""`yogo_png_unpack_any` (csrc/png_unpack_any.hip) on the MI355X and the routes behind ``--device-image-decode-all``: every PNG colour
type and bit depth, plain and Adam7, bit for bit what ``read_image(file, rgb)`` (PIL) and ``yogo_amd.png.decode_any`` give of the
same file; the statuses the kernel sets itself; ``PngDeviceFeed(all_types=True)``, ``predict`` with an RGB model and the cache
prefill with ``device_decode_all=True`` against the host routes.

Shapes (H x W): 67 x 37 -- one band of 64 rows plus three, an odd width so that 1 / 2 / 4-bit rows end in a partial byte and the
four-pixel fetch has a tail; 9 x 5 and 5 x 3 -- Adam7 passes that are empty or one pixel wide, W below the fetch width; 1 x 1.
The references of a shape are computed once (``cases``) and shared."""
import zlib

import numpy as np
import pytest
import torch

import _png_types_write as TW

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ALIGN = 16
FILL = 0xA5


def _inflated(data, info):
    return zlib.decompress(b"".join(data[o:o + n] for o, n in info.idat))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """shape -> [case]: one file of every format, plain and Adam7 (tRNS on every second one), with its parsed header, its inflated
    scanlines and the pixels ``read_image`` gives (1 and 3 planes), which ``decode_any`` has to give too"""
    from yogo_amd import png
    from yogo_amd.yogo_dataset import read_image

    root = tmp_path_factory.mktemp("png_types")
    out = {}
    for H, W in TW.SHAPES:
        rng = np.random.default_rng(H * 1000 + W)
        out[(H, W)] = []
        for k, fmt in enumerate(TW.FORMATS):
            for lace in (False, True):
                name = f"{TW.format_id(fmt)}{'_adam7' if lace else ''}_{H}x{W}"
                data, _, _ = TW.make_png(rng, H, W, *fmt, interlace=lace, trns=(k + lace) % 2 == 1)
                path = root / f"{name}.png"
                path.write_bytes(data)
                info = png.parse_png(data)
                ref = {C: read_image(path, rgb=C == 3) for C in (1, 3)}
                for C in (1, 3):
                    assert np.array_equal(png.decode_any(data, rgb=C == 3), ref[C].numpy()), (name, C)
                out[(H, W)].append(dict(name=name, data=data, info=info, ref=ref, path=path))
    return out


def _stage(blobs):
    """[(scanline bytes, format code, palette uint8 [768] or None)] -> (scan uint8 array, table rows): every image at a multiple of
    ALIGN, its palette behind its scanlines"""
    rows, parts, at = [], [], 0
    for scan, code, pal in blobs:
        need = -(-len(scan) // ALIGN) * ALIGN
        rows.append((at, code, at + need if pal is not None else 0))
        parts.append((at, np.frombuffer(scan, dtype=np.uint8)))
        if pal is not None:
            parts.append((at + need, pal))
            need += len(pal)
        at += -(-need // ALIGN) * ALIGN
    buf = np.zeros(max(at, 1), dtype=np.uint8)
    for o, b in parts:
        buf[o:o + len(b)] = b
    return buf, rows


def _blob(case):
    from yogo_amd import png

    info = case["info"]
    return _inflated(case["data"], info), info.format_code, png.palette_table(case["data"], info) if info.color_type == 3 else None


def _launch(scan_np, table, hw, out_shape, dtype=torch.uint8, top=0, left=0):
    from yogo_amd.device_decode import png_unpack_any

    scan = torch.from_numpy(scan_np.copy()).to(DEV)   # (the kernel writes into the scanlines: every launch has its own)
    out = torch.full(out_shape, FILL, dtype=dtype, device=DEV)
    status = torch.full((out_shape[0],), -1, dtype=torch.int32, device=DEV)
    png_unpack_any(scan, torch.tensor(table, dtype=torch.int64, device=DEV).reshape(-1, 3), hw, out, status, top, left)
    torch.cuda.synchronize()
    return out.cpu(), status.cpu()


def _variants():
    for hw in TW.SHAPES:
        yield pytest.param(hw, None, id=f"{hw[0]}x{hw[1]}")
    yield pytest.param((67, 37), (12, 33), id="67x37_crop12x33")


@pytest.mark.parametrize("fp32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw,crop", list(_variants()))
def test_every_format_in_one_launch_equals_read_image(cases, hw, crop, C, fp32):
    from yogo_amd import png
    from yogo_amd.device_decode import center_crop_origin

    H, W = hw
    group = cases[hw]
    planar = np.random.default_rng(7).integers(0, 256, size=(C, H, W), dtype=np.uint8)   # an image the host decoded
    scan, table = _stage([_blob(c) for c in group] + [(planar.tobytes(), png.FMT_PLANAR, None)])
    want = [c["ref"][C] for c in group] + [torch.from_numpy(planar)]
    OH, OW = crop or hw
    top, left = center_crop_origin(H, W, OH, OW)
    B = len(want)
    out, status = _launch(scan, table, hw, (B, C, OH, OW), torch.float32 if fp32 else torch.uint8, top, left)
    assert status.tolist() == [0] * B
    for b in range(B):
        w = want[b][:, top:top + OH, left:left + OW]
        w = w / 255 if fp32 else w
        assert torch.equal(out[b], w), (group[b]["name"] if b < len(group) else "planar", C, fp32, crop)


@pytest.mark.parametrize("C", [1, 3])
def test_grey8_and_rgb8_equal_the_existing_kernels(cases, C):
    from yogo_amd.device_decode import center_crop_origin, png_unpack, png_unpack_planes

    hw = (67, 37)
    group = [c for c in cases[hw] if c["info"].color_type in (0, 2) and c["info"].bit_depth == 8 and not c["info"].interlace]   # (tRNS or not)
    assert sorted(c["info"].color_type for c in group) == [0, 2]
    scan, table = _stage([_blob(c) for c in group])
    B = len(group)
    out, status = _launch(scan, table, hw, (B, C, *hw))
    old = torch.full((B, C, *hw), FILL, dtype=torch.uint8, device=DEV)
    st = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    kinds = [(off, 2 if c["info"].color_type == 2 else 0) for (off, _, _), c in zip(table, group)]
    png_unpack_planes(torch.from_numpy(scan.copy()).to(DEV), torch.tensor(kinds, dtype=torch.int64, device=DEV), hw, old, st)
    assert status.tolist() == st.tolist() == [0] * B and torch.equal(out, old.cpu())
    if C == 1:   # the grey file, cropped and divided, against yogo_png_unpack
        g = [b for b, c in enumerate(group) if c["info"].color_type == 0]
        top, left = center_crop_origin(*hw, 12, 33)
        for dtype in (torch.uint8, torch.float32):
            new, s1 = _launch(scan, [table[b] for b in g], hw, (len(g), 1, 12, 33), dtype, top, left)
            was = torch.full((len(g), 1, 12, 33), FILL, dtype=dtype, device=DEV)
            s0 = torch.full((len(g),), -1, dtype=torch.int32, device=DEV)
            png_unpack(torch.from_numpy(scan.copy()).to(DEV), torch.tensor([(table[b][0], 0) for b in g], dtype=torch.int64, device=DEV), hw, was, s0,
                       top, left)
            assert s1.tolist() == s0.tolist() == [0] * len(g) and torch.equal(new, was.cpu())


@pytest.mark.parametrize("C", [1, 3])
def test_statuses_are_per_image(cases, tmp_path, C):
    """a filter byte of 9 in row 65, one inside Adam7 pass 4, an image past ``scan``, a palette past ``scan``, format codes outside
    the table: each is that image's status alone, the good images between them are right"""
    from yogo_amd import png
    from yogo_amd.yogo_dataset import read_image

    hw = H, W = 67, 37
    by_name = {c["name"]: c for c in cases[hw]}
    good = [by_name[f"{n}_{H}x{W}"] for n in ("ct0d8", "ct6d16_adam7", "ct3d4", "ct2d8_adam7")]
    rng = np.random.default_rng(11)
    bad = []
    for fmt, lace, where in (((6, 8), False, (0, 65, 9)), ((0, 16), True, (3, 2, 9))):
        clean, samples, _ = TW.make_png(rng, H, W, *fmt, interlace=lace)
        broken, _, _ = TW.make_png(rng, H, W, *fmt, interlace=lace, bad=where, samples=samples)
        p = tmp_path / f"clean_{fmt[0]}_{fmt[1]}.png"
        p.write_bytes(clean)
        bad.append((broken, png.parse_png(broken), read_image(p, rgb=C == 3)))
    blobs = [_blob(good[0]), (_inflated(bad[0][0], bad[0][1]), bad[0][1].format_code, None), _blob(good[1]),
             (_inflated(bad[1][0], bad[1][1]), bad[1][1].format_code, None), _blob(good[2]), _blob(good[3])]
    scan, table = _stage(blobs)
    n = len(scan)
    grey8 = by_name[f"ct0d8_{H}x{W}"]["info"]
    pal_row = table[4]
    table = table + [
        (n + 4096, grey8.format_code, 0),                      # past the end
        (n - grey8.inflated_bytes + 1, grey8.format_code, 0),  # ends one byte after the end
        (-16, grey8.format_code, 0),
        (pal_row[0], pal_row[1], n - 767),                     # its palette ends one byte after the end
        (pal_row[0], pal_row[1], -1),
        (table[0][0], 5 | 8 << 8, 0),                          # no colour type 5
        (table[0][0], 0 | 3 << 8, 0),                          # no 3-bit greyscale
        (table[0][0], 2 | 4 << 8, 0),                          # no 4-bit RGB
        (table[0][0], 0 | 8 << 8 | 2 << 16, 0),                # no interlace method 2
        (table[0][0], -1, 0),
    ]
    B = len(table)
    out, status = _launch(scan, table, hw, (B, C, H, W))
    assert status.tolist() == [0, 1, 0, 1, 0, 0] + [2] * (B - 6)
    for b, c in ((0, good[0]), (2, good[1]), (4, good[2]), (5, good[3])):
        assert torch.equal(out[b], c["ref"][C]), c["name"]
    # row 65 lies in the second band: the first band's 64 rows are written, nothing after
    assert torch.equal(out[1][:, :64], bad[0][2][:, :64]) and bool((out[1][:, 64:] == FILL).all())
    # Adam7 passes 1 .. 3 are written (their pixels: rows 0 mod 8, columns 0 mod 4), pass 4 has one band: nothing of it or after it
    done = torch.zeros(H, W, dtype=torch.bool)
    done[0::8, 0::4] = True
    done[4::8, 0::4] = True
    assert torch.equal(out[3][:, done], bad[1][2][:, done]) and bool((out[3][:, ~done] == FILL).all())
    for b in range(6, B):
        assert bool((out[b] == FILL).all()), b


# ---- the routes behind the switch -------------------------------------------------------------------------------------------
CLASSES = ["you", "only", "glance", "once"]
FEED_HW = (23, 29)


@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    """one 23 x 29 file of every format, plain and Adam7, tRNS on every second one, plus a BMP under a .png name"""
    from PIL import Image

    d = tmp_path_factory.mktemp("feed_types")
    rng = np.random.default_rng(17)
    k = 0
    for fmt in TW.FORMATS:
        for lace in (False, True):
            data, _, _ = TW.make_png(rng, *FEED_HW, *fmt, interlace=lace, trns=k % 2 == 1)
            (d / f"img_{k:02d}_{TW.format_id(fmt)}{'_adam7' if lace else ''}.png").write_bytes(data)
            k += 1
    Image.fromarray(rng.integers(0, 256, size=(*FEED_HW, 3), dtype=np.uint8)).save(d / "img_15_bmp.png", format="BMP")
    return d, sorted(str(p) for p in d.glob("*.png"))


def _feed(d, batch, **kw):
    from yogo_amd.image_path_dataset import ImagePathDataset
    from yogo_amd.png_feed import PngDeviceFeed

    return PngDeviceFeed(ImagePathDataset(d), batch, "cuda", **kw)


@pytest.mark.parametrize("rgb", [False, True])
def test_feed_all_types_equals_read_image(png_dir, rgb):
    from yogo_amd import _hip, png
    from yogo_amd.yogo_dataset import read_image

    d, paths = png_dir
    n, batch = len(paths), 7
    assert n == 31
    want = torch.stack([read_image(p, rgb=rgb) for p in paths])
    _hip.launch_log(True)
    try:
        feed = _feed(d, batch, all_types=True, rgb=rgb)
        batches = list(feed)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert [b.shape[0] for b, _ in batches] == [min(batch, n - lo) for lo in range(0, n, batch)]
    assert all(b.is_cuda and b.dtype == torch.uint8 and b.shape[1] == (3 if rgb else 1) for b, _ in batches)
    assert [p for _, names in batches for p in names] == paths
    assert torch.equal(torch.cat([b.cpu() for b, _ in batches]), want)
    assert feed.host_decoded == 1                                                  # the BMP alone
    assert sum(ln.startswith("png_unpack_any_kernel") for ln in log) == len(batches) == 5
    assert sum(ln.startswith("inflate_zlib_kernel") for ln in log) == len(batches)
    assert not any(ln.startswith(("png_unpack_kernel", "png_unpack_planes_kernel")) for ln in log)
    f32 = torch.cat([b.cpu() for b, _ in _feed(d, batch, all_types=True, rgb=rgb, normalize=True, crop=(12, 25))])
    assert f32.dtype == torch.float32 and torch.equal(f32, want[:, :, 6:18, 2:27] / 255)
    if not rgb:   # without the switch: the same batches, and every file but the plain 8-bit grey one without tRNS goes through the host
        old = _feed(d, batch)
        assert torch.equal(torch.cat([b.cpu() for b, _ in old]), want)
        plain = sum(1 for p in paths if not p.endswith("bmp.png") and png.parse_png(open(p, "rb").read()).device_decodable)
        assert plain == 1 and old.host_decoded == n - plain
    else:
        with pytest.raises(ValueError, match="all_types"):
            _feed(d, batch, rgb=True)


def test_feed_palette_without_plte_stays_on_the_host(tmp_path):
    """colour type 3 without a PLTE chunk: whatever PIL makes of it, PIL makes it"""
    from yogo_amd.yogo_dataset import read_image

    rng = np.random.default_rng(5)
    for k in range(3):
        data, _, _ = TW.make_png(rng, *FEED_HW, 3, 8, plte_entries=0 if k == 1 else None)
        (tmp_path / f"img_{k}.png").write_bytes(data)
    try:
        want = read_image(tmp_path / "img_1.png")
    except Exception:
        want = None
    feed = _feed(tmp_path, 3, all_types=True)
    if want is None:
        with pytest.raises(RuntimeError, match="img_1"):
            next(feed)
    else:
        batch, _ = next(feed)
        assert torch.equal(batch[1].cpu(), want) and feed.host_decoded == 1


def _make_checkpoint(tmp_path, seed=3, is_rgb=False):
    """as tests/test_gpu_png_feed.py::_make_checkpoint"""
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4, is_rgb=is_rgb).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        net.model[7].bias[4] += 1.5
    p = tmp_path / "m.pth"
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, p)
    return p


def test_predict_rgb_model_with_the_switch_equals_predict_without(tmp_path, capsys):
    from yogo_amd import _hip
    from yogo_amd.infer import predict

    pth = _make_checkpoint(tmp_path, is_rgb=True)
    imgdir = tmp_path / "run" / "images"
    imgdir.mkdir(parents=True)
    rng = np.random.default_rng(23)
    for k, (fmt, lace) in enumerate((((2, 8), False), ((3, 8), False), ((6, 16), True), ((0, 4), False), ((4, 8), True), ((0, 16), False))):
        (imgdir / f"img_{k}.png").write_bytes(TW.make_png(rng, 64, 96, *fmt, interlace=lace, trns=k == 1)[0])
    kw = dict(save_npy=True, count_predictions=True, batch_size=4, obj_thresh=0.4, iou_thresh=0.5, class_names=CLASSES)
    predict(str(pth), path_to_images=imgdir, output_dir=str(tmp_path / "host"), **kw)
    host_out = capsys.readouterr().out
    _hip.launch_log(True)
    try:
        predict(str(pth), path_to_images=imgdir, output_dir=str(tmp_path / "dev"), device_image_decode=True, device_image_decode_all=True, **kw)
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    assert capsys.readouterr().out == host_out and "you" in host_out
    a, b = sorted((tmp_path / "host").glob("*.npy")), sorted((tmp_path / "dev").glob("*.npy"))
    assert len(a) == 1 and [p.name for p in a] == [p.name for p in b] and a[0].read_bytes() == b[0].read_bytes()
    assert np.load(a[0]).shape[1] > 0
    assert sum(ln.startswith("png_unpack_any_kernel<3,u8>") for ln in log) == 2
    with pytest.raises(ValueError, match="RGB"):      # without the new switch an RGB model is refused, as before
        predict(str(pth), path_to_images=imgdir, device_image_decode=True)
    with pytest.raises(ValueError, match="needs device_image_decode"):
        predict(str(pth), path_to_images=imgdir, device_image_decode_all=True)


PREFILL_HW = (35, 37)
Sx, Sy = 12, 8


@pytest.fixture(scope="module")
def prefill_data(tmp_path_factory):
    """15 files at 35 x 37, one of every format (plain and Adam7 in turn, tRNS on every third), then a JPEG under a .png name and a
    truncated file"""
    from PIL import Image

    root = tmp_path_factory.mktemp("prefill_types")
    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir()
    lab_dir.mkdir()
    rng = np.random.default_rng(29)
    files = [TW.make_png(rng, *PREFILL_HW, *fmt, interlace=k % 2 == 1, trns=k % 3 == 0)[0] for k, fmt in enumerate(TW.FORMATS)]
    for k, data in enumerate(files):
        (img_dir / f"img_{k:04d}.png").write_bytes(data)
    Image.fromarray(rng.integers(0, 256, size=(*PREFILL_HW, 3), dtype=np.uint8)).save(img_dir / "img_0015.png", format="JPEG")
    (img_dir / "img_0016.png").write_bytes(files[3][:len(files[3]) // 2])
    for k in range(17):
        lines = [f"{int(rng.integers(0, len(CLASSES)))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} "
                 f"{rng.uniform(0.05, 0.3):.6f} {rng.uniform(0.05, 0.3):.6f}" for _ in range(2 + k % 3)]
        (lab_dir / f"img_{k:04d}.txt").write_text("".join(ln + "\n" for ln in lines))
    return img_dir, lab_dir


@pytest.mark.filterwarnings("ignore:could not read")
@pytest.mark.parametrize("rgb", [False, True])
def test_cache_prefill_all_types_equals_the_host_route(prefill_data, rgb):
    from yogo_amd.image_cache import ImageCache
    from yogo_amd.yogo_dataset import ObjectDetectionDataset

    img_dir, lab_dir = prefill_data
    split = ObjectDetectionDataset(img_dir, lab_dir, Sx, Sy, CLASSES, image_hw=PREFILL_HW, rgb=rgb)
    N = len(split)
    assert N == 17
    caches = {}
    for name, kw in (("host", {}), ("old", dict(device_decode=True)), ("all", dict(device_decode=True, device_decode_all=True))):
        c = ImageCache(split, N, (3 if rgb else 1, *PREFILL_HW), False, device=DEV, num_workers=0, batch_size=4, decode_batch=6, **kw)
        c.images.fill_(0x5A)
        c.prefill()
        caches[name] = c
    host = caches["host"]
    assert host.resident.tolist() == [True] * 16 + [False]                       # the truncated file alone is unreadable
    for name in ("old", "all"):
        c = caches[name]
        assert np.array_equal(c.resident, host.resident) and torch.equal(c.images.cpu(), host.images.cpu()), name
        assert torch.equal(c.rows, host.rows) and c.rows.dtype == host.rows.dtype and np.array_equal(c.row_offsets, host.row_offsets), name
        assert len(c.decode_stats["unpack_ms"]) == 3                            # chunks of 6, 6 and 5: one unpack launch each
    assert caches["all"].decode_stats["host_decoded"] == 2                       # the JPEG and the truncated file
    # without the switch only 8-bit grey / RGB files without interlace and tRNS stay on the device, as before
    from yogo_amd import png

    plain = sum(1 for k in range(15) if png.parse_png((img_dir / f"img_{k:04d}.png").read_bytes()).prefill_decodable)
    assert caches["old"].decode_stats["host_decoded"] == N - plain
    with pytest.raises(ValueError, match="needs --device-image-decode"):
        ImageCache(split, N, (3 if rgb else 1, *PREFILL_HW), False, device=DEV, device_decode_all=True)


@pytest.mark.parametrize("rgb", [False, True])
def test_cache_prefill_resizes_other_size_files_of_any_type(tmp_path, rgb):
    """a palette file, an interlaced 2-bit grey one and a 16-bit RGBA one at other sizes than the cache's 24 x 33, and a grey+alpha one
    at it: with --device-image-resize the new kernel writes the staging tensor and yogo_resize_aa_u8 runs unchanged -- the slots hold
    the fp64 oracle of tests/_resize_ref.py applied to ``read_image``'s pixels, under the resize kernel's own rule"""
    import _resize_ref as R
    from yogo_amd import _hip
    from yogo_amd.image_cache import ImageCache
    from yogo_amd.yogo_dataset import ObjectDetectionDataset, read_image

    HW = (24, 33)
    files = (((48, 70), (3, 8), False), ((35, 20), (0, 2), True), ((48, 70), (6, 16), False), (HW, (4, 8), True))
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir()
    lab_dir.mkdir()
    rng = np.random.default_rng(31)
    for k, (hw, fmt, lace) in enumerate(files):
        (img_dir / f"img_{k:04d}.png").write_bytes(TW.make_png(rng, *hw, *fmt, interlace=lace)[0])
        (lab_dir / f"img_{k:04d}.txt").write_text("1 0.500000 0.500000 0.200000 0.200000\n2 0.300000 0.300000 0.200000 0.200000\n")
    split = ObjectDetectionDataset(img_dir, lab_dir, Sx, Sy, CLASSES, image_hw=HW, rgb=rgb)
    N = len(files)
    v = np.stack([R.exact(read_image(str(split._image_paths[k]), rgb=rgb).numpy(), HW) for k in range(N)])
    R.assert_cap(v[:3])
    _hip.launch_log(True)
    try:
        c = ImageCache(split, N, (3 if rgb else 1, *HW), False, device=DEV, num_workers=0, batch_size=4, decode_batch=4, device_decode=True,
                       device_resize=True, device_decode_all=True)
        c.images.fill_(0x5A)
        c.prefill()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    got = c.images.cpu().numpy()
    assert c.resident.all() and c.decode_stats["host_decoded"] == 0 and c.decode_stats["device_resized"] == 3
    assert np.array_equal(got[3], read_image(str(split._image_paths[3]), rgb=rgb).numpy())
    R.assert_rule(got[:3], v[:3], R.TOL_FP32, "resized from every type")
    # the chunk's launch and one per other size (48 x 70, 35 x 20), all by the new kernel; the resize kernel as before
    assert sum(ln.startswith("png_unpack_any_kernel") for ln in log) == 3 and not any(ln.startswith("png_unpack_planes_kernel") for ln in log)
    assert len(c.decode_stats["resize_ms"]) == 2
