"""The host plumbing the device decoders' feeds share (yogo_amd/device_decode.py): the prefetching iterator on a stand-in that loads
integers, and the copy of a PNG file's IDAT payloads into its room.  No GPU is needed; nothing here touches torch.cuda."""
import threading

import numpy as np
import pytest

from _png_write import png_bytes


def _feed_class():
    from yogo_amd.device_decode import PrefetchFeed

    class Feed(PrefetchFeed):
        """loads n * 10 for batch n; batch `bad` raises RuntimeError; every load after batch 0's waits for `gate` where one is given"""

        def __init__(self, count, bad=None, gate=None):
            self.bad, self.gate, self.loads, self.ahead, self.closed = bad, gate, [], [], 0
            self.started = threading.Event()
            super().__init__(count, 1, "test-feed")

        def close(self):
            super().close()
            self.closed += 1

        def _load(self, n):
            if self.gate is not None and n:
                self.started.set()
                self.gate.wait()
            self.loads.append((n, threading.current_thread().name))
            if n == self.bad:
                raise RuntimeError(f"batch {n} is bad")
            return n * 10

        def _deliver(self, n, loaded):
            self.ahead.append(n + 1 >= len(self.batches) or n + 1 in self._pending)   # the next load is under way by now
            return n, loaded

    return Feed


def test_prefetch_feed_loads_one_batch_ahead():
    feed = _feed_class()(4)
    assert len(feed) == 4 and iter(feed) is feed
    assert list(feed) == [(0, 0), (1, 10), (2, 20), (3, 30)]
    assert feed.ahead == [True] * 4
    assert [n for n, _ in feed.loads] == [0, 1, 2, 3] and all(name.startswith("test-feed") for _, name in feed.loads)
    assert feed.closed == 1 and not feed._pending
    with pytest.raises(RuntimeError, match="after shutdown"):   # close() has run: the loader takes nothing more
        feed._loader.submit(int)


def test_prefetch_feed_a_bad_batch_costs_exactly_that_batch():
    feed = _feed_class()(3, bad=1)
    assert next(feed) == (0, 0)
    with pytest.raises(RuntimeError, match="batch 1 is bad"):
        next(feed)
    assert next(feed) == (2, 20)
    with pytest.raises(StopIteration):
        next(feed)
    assert feed.closed == 1 and [n for n, _ in feed.loads] == [0, 1, 2]


def test_prefetch_feed_closed_early_with_a_load_pending():
    gate = threading.Event()
    feed = _feed_class()(3, gate=gate)
    assert next(feed) == (0, 0)
    assert 1 in feed._pending and feed.started.wait(30)   # batch 1's load runs and is held
    closer = threading.Thread(target=feed.close)
    closer.start()
    assert feed.closed == 0           # close() waits for the load
    gate.set()
    closer.join(timeout=30)
    assert not closer.is_alive() and feed.closed == 1 and not feed._pending
    with pytest.raises(RuntimeError, match="after shutdown"):
        feed._loader.submit(int)


@pytest.mark.parametrize("rgb", [False, True])
def test_png_stream_into(tmp_path, rgb):
    from yogo_amd import inflate, png
    from yogo_amd.device_decode import png_stream_into

    rng = np.random.default_rng(7 + rgb)
    img = rng.integers(0, 256, size=(3, 5, 3) if rgb else (3, 5), dtype=np.uint8)
    one = png_bytes(img, [1, 4, 3])
    stream = png.parse_png(one)
    stream = one[stream.idat[0][0]:stream.idat[0][0] + stream.idat[0][1]]   # the zlib stream, from the file with one IDAT chunk
    data = png_bytes(img, [1, 4, 3], idat_sizes=[1, 7, 100])
    info = png.parse_png(data)
    assert [n for _, n in info.idat] == [1, 7, min(100, len(stream) - 8), max(0, len(stream) - 108)] and info.idat_bytes == len(stream)
    assert info.prefill_decodable and info.device_decodable is (not rgb) and info.bytes_per_pixel == (3 if rgb else 1)
    room = np.full(len(stream) + 5, 0xEE, dtype=np.uint8)
    stored, off, ln, adler = png_stream_into(data, info, room)
    assert stored == len(stream) and room[:stored].tobytes() == stream and bool((room[stored:] == 0xEE).all())
    assert (off, ln, adler) == inflate.split_zlib(stream)
    assert (off, ln, adler) == inflate.split_zlib(b"".join(data[o:o + n] for o, n in info.idat))

    # a room one byte short: the callers refuse before they copy -- the prefill hands the sample to the host decoder
    from yogo_amd import png_prefill

    class Dataset:
        _image_paths = [tmp_path / "a.png"]
        asked = []

        def image_uint8(self, j):
            self.asked.append(j)
            return None

    Dataset._image_paths[0].write_bytes(data)
    short = np.full(len(stream) - 1, 0xEE, dtype=np.uint8)
    s = png_prefill._read(Dataset(), 0, short, (3, 5))
    assert s.host and s.stored == 0 and Dataset.asked == [0] and bool((short == 0xEE).all())
    s = png_prefill._read(Dataset(), 0, room, (3, 5))
    assert not s.host and (s.stored, s.deflate, s.adler, s.bpp) == (stored, (off, ln), adler, 3 if rgb else 1) and Dataset.asked == [0]
    if not rgb:   # ... and the inference feed decodes the file on the host; its first batch (no room yet) keeps the stream as bytes
        from yogo_amd.png_feed import PngDeviceFeed

        feed, path = object.__new__(PngDeviceFeed), str(Dataset._image_paths[0])
        im = feed._read(path, short)
        assert im.stored == 0 and np.array_equal(im.pixels, img) and bool((short == 0xEE).all())
        im = feed._read(path, room)
        assert im.pixels is None and im.stream is None and (im.hw, im.stored, im.deflate, im.adler) == ((3, 5), stored, (off, ln), adler)
        im = feed._read(path, None)
        assert im.pixels is None and im.stream == stream and (im.hw, im.stored, im.deflate, im.adler) == ((3, 5), stored, (off, ln), adler)
