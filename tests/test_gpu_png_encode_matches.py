"""Level 1 of the PNG encoder on the device (yogo_amd/csrc/png_encode_matches.hip): byte for byte its host twin on the cases of
tests/_png_match_cases.py (tests/test_png_encode_matches_host.py asserts what each exercises), batches, the round trip through the
repository's own device decoders, a slot that is too small, refused arguments, level 0 through the new symbol, and ``predict`` end to
end against the host route."""
import ctypes

import numpy as np
import pytest
import torch

import _png_match_cases as M
from yogo_amd import draw
from yogo_amd import png_encode as E

pytestmark = pytest.mark.gpu
CASES = M.match_cases()
CLASSES = ["you", "only", "glance", "once"]


@pytest.fixture(scope="module")
def twin():
    """{name: the twin's level-1 file}, made once"""
    return {name: E.encode_png_host(px, level=1) for name, px in CASES.items()}


def _files(files, offsets, status, slot=None):
    off = offsets.cpu().numpy()
    assert status.cpu().tolist() == [0] * (len(off) - 1)
    data = files.cpu().numpy()
    if slot is None:
        return [data[off[b]: off[b + 1]].tobytes() for b in range(len(off) - 1)]
    return [data[b * slot: b * slot + off[b + 1] - off[b]].tobytes() for b in range(len(off) - 1)]


@pytest.mark.parametrize("name", list(CASES))
def test_encoder_equals_twin(twin, name):
    px = CASES[name]
    H, W, bpp = px.shape
    slot, work1 = draw.encode_bound(H, W, bpp, level=1)
    slot0, work0 = draw.encode_bound(H, W, bpp)
    assert slot == slot0 == E.encode_bound(H, W, bpp) and work1 > work0
    want = twin[name]
    got = _files(*draw.encode_png(torch.from_numpy(px[None]).cuda(), level=1), slot=slot)
    assert len(got[0]) == len(want) and got[0] == want


@pytest.mark.parametrize("packed", [False, True])
def test_batch_of_three(twin, packed):
    """stored bands, constant rows and a smooth frame (40 x 50, its edge repeated to 48 x 64) side by side"""
    batch = np.stack([CASES["noise"], CASES["constant"], np.pad(CASES["smooth"], ((0, 8), (0, 14), (0, 0)), mode="edge")])
    slot, _ = draw.encode_bound(48, 64, 4, level=1)
    files, offsets, status = draw.encode_png(torch.from_numpy(batch).cuda(), packed=packed, level=1)
    got = _files(files, offsets, status, slot=None if packed else slot)
    assert got == [E.encode_png_host(px, level=1) for px in batch]
    assert got[0] == twin["noise"] and got[1] == twin["constant"]


def test_round_trip_through_the_device_decoders(twin):
    """the level-1 IDAT bytes through yogo_inflate_zlib and yogo_png_unpack_any give the planes the host decoder gives for the file"""
    from yogo_amd import device_decode as DD
    from yogo_amd import png
    from yogo_amd.inflate import split_zlib

    for name in ("smooth", "ragged_height", "constant", "distances_bpp4"):
        px = CASES[name]
        H, W, _ = px.shape
        files, offsets, status = draw.encode_png(torch.from_numpy(px[None]).cuda(), packed=True, level=1)
        assert int(status[0]) == 0
        data = files[: int(offsets[1])]
        host = data.cpu().numpy().tobytes()
        assert host == twin[name]
        info = png.parse_png(host)
        assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (W, H, 8, 6, 0)
        stream = torch.cat([data[o: o + n] for o, n in info.idat])          # stays on the device
        off, length, adler = split_zlib(stream.cpu().numpy().tobytes())
        scan = torch.zeros((info.inflated_bytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        table = torch.tensor([[off, length, 0, info.inflated_bytes, adler]], dtype=torch.int64, device="cuda")
        st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        DD.inflate_streams(stream.contiguous(), table, scan, st)
        assert int(st[0]) == 0
        out = torch.zeros(1, 3, H, W, dtype=torch.uint8, device="cuda")
        st2 = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        DD.png_unpack_any(scan, torch.tensor([[0, info.format_code, 0]], dtype=torch.int64, device="cuda"), (H, W), out, st2)
        assert int(st2[0]) == 0
        want = png.decode_any(host, rgb=True)
        assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(want, px[:, :, :3].transpose(2, 0, 1))


@pytest.mark.parametrize("packed", [False, True])
def test_slot_one_byte_too_small(twin, packed):
    """the noise frame needs the whole bound at level 1 too: one byte less is refused with a status and nothing is written, in or
    past the slot"""
    batch = np.stack([CASES["constant"], CASES["noise"]])
    slot, _ = draw.encode_bound(48, 64, 4, level=1)
    assert len(twin["noise"]) == slot
    small, guard = slot - 1, 4096
    files = torch.full((2 * small + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _, offsets, status = draw.encode_png(torch.from_numpy(batch).cuda(), files=files, packed=packed, slot_bytes=small, level=1)
    want = twin["constant"]
    assert status.cpu().tolist() == [0, E.ST_SLOT] and offsets.cpu().tolist() == [0, len(want), len(want)]
    host = files.cpu().numpy()
    assert host[: len(want)].tobytes() == want and (host[len(want):] == 0xA5).all()


def test_refuses_bad_arguments():
    from yogo_amd import _hip

    px = torch.zeros(2, 20, 24, 4, dtype=torch.uint8, device="cuda")
    slot, work0 = draw.encode_bound(20, 24, 4)
    _, work1 = draw.encode_bound(20, 24, 4, level=1)
    assert work1 > work0
    for level in (-1, 2, True, 1.0):
        with pytest.raises(ValueError):
            draw.encode_png(px, level=level)
        with pytest.raises(ValueError):
            draw.encode_bound(20, 24, 4, level=level)
    out = ctypes.c_size_t(0)
    for level in (-1, 2):
        with pytest.raises(RuntimeError):
            _hip.call("yogo_png_encode_bound_level", 20, 24, 4, level, ctypes.addressof(out), ctypes.addressof(out))
    # work space sized for level 0 handed to level 1: refused by the wrapper, and by the library itself (a guard page's worth of
    # 0xA5 behind the short work space stays as it was)
    with pytest.raises(ValueError):
        draw.encode_png(px, work=torch.zeros(2 * work0, dtype=torch.uint8, device="cuda"), level=1)
    work = torch.full((2 * work0 + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    files = torch.full((2 * slot,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets, status = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    for level, size in ((1, 2 * work0), (2, 2 * work1), (-1, 2 * work1)):
        with pytest.raises(RuntimeError):
            _hip.call("yogo_png_encode_level", px, 2, 20, 24, 4, level, files, slot, 0, offsets, status, work, size, _hip.stream_ptr())
    torch.cuda.synchronize()
    assert (work.cpu().numpy() == 0xA5).all() and (files.cpu().numpy() == 0xA5).all()


def test_level_0_through_the_new_symbol_is_the_old_symbol():
    from yogo_amd import _hip

    batch = np.stack([CASES["noise"], CASES["constant"], CASES["noise"][::-1].copy()])
    px = torch.from_numpy(batch).cuda()
    slot, work_per = draw.encode_bound(48, 64, 4)
    outs = []
    for symbol in ("yogo_png_encode", "yogo_png_encode_level"):
        files = torch.zeros(3 * slot, dtype=torch.uint8, device="cuda")
        work = torch.zeros(3 * work_per, dtype=torch.uint8, device="cuda")
        offsets, status = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.full((3,), -1, dtype=torch.int32, device="cuda")
        level = () if symbol == "yogo_png_encode" else (0,)
        _hip.call(symbol, px, 3, 48, 64, 4, *level, files, slot, 1, offsets, status, work, int(work.numel()), _hip.stream_ptr())
        outs.append(_files(files, offsets, status))
    assert outs[0] == outs[1] == [E.encode_png_host(p) for p in batch]
    assert outs[1] == _files(*draw.encode_png(px, packed=True))
    sizes = [ctypes.c_size_t(0) for _ in range(4)]
    _hip.call("yogo_png_encode_bound", 48, 64, 4, ctypes.addressof(sizes[0]), ctypes.addressof(sizes[1]))
    _hip.call("yogo_png_encode_bound_level", 48, 64, 4, 0, ctypes.addressof(sizes[2]), ctypes.addressof(sizes[3]))
    assert (sizes[0].value, sizes[1].value) == (sizes[2].value, sizes[3].value) == (slot, work_per)


# ---- end to end (the fixture of tests/test_gpu_draw_boxes.py restated) --------------------------------------------------------------
def _make_checkpoint(tmp_path, seed=3):
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4).cuda()
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


def test_predict_at_level_1_writes_the_same_pixels_in_no_more_bytes(tmp_path):
    from PIL import Image

    from yogo_amd.infer import predict

    frames = np.random.default_rng(6).integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    (tmp_path / "png").mkdir()
    for i in range(10):
        Image.fromarray(frames[:, :, i]).save(tmp_path / "png" / f"img_{i:02d}.png")
    pth = _make_checkpoint(tmp_path)
    kw = dict(path_to_images=tmp_path / "png", draw_boxes=True, batch_size=4, obj_thresh=0.4, iou_thresh=0.5, class_names=CLASSES)
    predict(str(pth), output_dir=str(tmp_path / "host"), **kw)
    predict(str(pth), output_dir=str(tmp_path / "level0"), device_draw=True, **kw)
    predict(str(pth), output_dir=str(tmp_path / "level1"), device_draw=True, device_draw_level=1, **kw)
    names = sorted(p.name for p in (tmp_path / "host").iterdir())
    assert len(names) == 10 and all(n.endswith(".png") for n in names)
    drawn = 0
    for d in ("level0", "level1"):
        assert sorted(p.name for p in (tmp_path / d).iterdir()) == names
    for f in names:
        want = np.asarray(Image.open(tmp_path / "host" / f))
        got = Image.open(tmp_path / "level1" / f)
        assert got.mode == "RGBA" and got.size == (96, 64)
        assert np.array_equal(np.asarray(got), want), f
        data = (tmp_path / "level1" / f).read_bytes()
        assert data == E.encode_png_host(want, level=1), f
        assert len(data) <= (tmp_path / "level0" / f).stat().st_size, f
        drawn += int((want[:, :, 0] != want[:, :, 1]).any() or (want[:, :, 1] != want[:, :, 2]).any())
    assert drawn > 0, "no image has a box: the comparison shows nothing"
    for kw_bad in (dict(device_draw_level=1), dict(device_draw=True, device_draw_level=1, output_img_ftype=".tif")):
        with pytest.raises(ValueError):
            predict(str(pth), output_dir=str(tmp_path / "never"), **kw, **kw_bad)
