"""A read-only reader for Zarr v2 stores of uint8 image stacks (standard library + numpy only).

Written against the published Zarr v2 storage specification: a store maps keys to bytes; an array is the JSON document under
``.zarray`` plus one value per chunk under the key ``i.j.k`` (or ``i/j/k``); a group is the JSON document under ``.zgroup`` and
its members live under ``<name>/``.  Every chunk is stored at the full chunk shape (edge chunks are padded), in C or F order,
after the compressor.  What `yogo infer --path-to-zarr` needs of it (yogo/data/image_path_dataset.py:97-120):

* the root is an array of shape ``[H, W, N]`` (frame ``idx`` is ``array[:, :, idx]``), or a group whose members ``"0"``, ``"1"``, ...
  are 2-D arrays (frame ``idx`` is ``group[idx][:]``);
* ``len(array)`` is the number of chunk keys present in the store (``zarr.Array.initialized``), ``len(group)`` its member count;
* stores: a directory, or a ``.zip`` file (members stored or deflated; of two members with one name the last one wins).

``dtype`` must be ``|u1``; ``filters`` must be null; the compressors ``null`` / ``zlib`` / ``gzip`` / ``bz2`` come from the standard
library, any other id goes through ``numcodecs.get_codec`` when numcodecs imports; without it ``blosc`` (zarr's default) is decoded
by yogo_amd/blosc.py when its document is complete (``cname``, ``clevel``, ``shuffle``, ``blocksize``: what numcodecs writes;
``cname`` ``zstd`` included) and ``zstd`` by yogo_amd/zstd.py (libzstd through ctypes where it loads, else a pure-Python decoder),
and everything else raises ``NotImplementedError``.
A chunk that cannot be read or decoded raises ``RuntimeError`` naming its key -- the class `predict`'s loop tolerates.
"""
from __future__ import annotations

import bz2
import json
import os
import re
import zipfile
import zlib
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np


class DirectoryStore:
    """keys are the files below ``path``, with ``/`` between the parts"""

    def __init__(self, path: Union[str, Path]):
        self.path = str(path)

    def clone(self) -> "DirectoryStore":
        return DirectoryStore(self.path)

    def close(self) -> None:
        pass

    def _file(self, key: str) -> str:
        return os.path.join(self.path, *key.split("/"))

    def __contains__(self, key: str) -> bool:
        return os.path.isfile(self._file(key))

    def keys(self) -> List[str]:
        out = []
        for root, _, files in os.walk(self.path):
            rel = os.path.relpath(root, self.path)
            pre = "" if rel == "." else rel.replace(os.sep, "/") + "/"
            out.extend(pre + f for f in files)
        return out

    def get(self, key: str) -> bytes:
        try:
            with open(self._file(key), "rb") as f:
                return f.read()
        except FileNotFoundError:
            raise KeyError(key) from None

    def nbytes(self, key: str) -> int:
        """the stored size of the value of ``key``"""
        try:
            return os.path.getsize(self._file(key))
        except FileNotFoundError:
            raise KeyError(key) from None

    def readinto(self, key: str, out: memoryview) -> int:
        """the value of ``key`` straight into ``out`` (one copy); -> bytes written (short when the value is shorter than out);
        ValueError when it is longer"""
        try:
            f = open(self._file(key), "rb", buffering=0)
        except FileNotFoundError:
            raise KeyError(key) from None
        with f:
            if os.fstat(f.fileno()).st_size > len(out):
                raise ValueError(f"{os.fstat(f.fileno()).st_size} bytes stored, {len(out)} expected")
            n = 0
            while n < len(out):
                got = f.readinto(out[n:])
                if not got:
                    break
                n += got
            return n


class ZipStore:
    """keys are the member names of a zip file, as zarr's ZipStore writes them"""

    def __init__(self, path: Union[str, Path]):
        self.path = str(path)
        self._zf = zipfile.ZipFile(self.path, "r")
        # of two members with one name the LAST one wins (a zip is appended to; zipfile's own name table agrees)
        self._info: Dict[str, zipfile.ZipInfo] = {i.filename: i for i in self._zf.infolist() if not i.filename.endswith("/")}
        self._fd: Optional[int] = None
        self._data_off: Dict[str, int] = {}

    def clone(self) -> "ZipStore":
        return ZipStore(self.path)

    def close(self) -> None:
        self._zf.close()
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None

    def __del__(self):   # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __contains__(self, key: str) -> bool:
        return key in self._info

    def keys(self) -> List[str]:
        return list(self._info)

    def get(self, key: str) -> bytes:
        info = self._info.get(key)
        if info is None:
            raise KeyError(key)
        return self._zf.read(info)   # inflates a deflated member; checks length and CRC

    def nbytes(self, key: str) -> int:
        info = self._info.get(key)
        if info is None:
            raise KeyError(key)
        return info.file_size

    def readinto(self, key: str, out: memoryview) -> int:
        info = self._info.get(key)
        if info is None:
            raise KeyError(key)
        if info.file_size > len(out):
            raise ValueError(f"{info.file_size} bytes stored, {len(out)} expected")
        if info.compress_type != zipfile.ZIP_STORED or info.flag_bits & 0x1:
            data = self._zf.read(info)
            out[:len(data)] = data
            return len(data)
        # a stored member: its bytes lie in the file as they are -> pread them into `out`, no intermediate object
        if self._fd is None:
            self._fd = os.open(self.path, os.O_RDONLY)
        off = self._data_off.get(key)
        if off is None:
            hdr = os.pread(self._fd, 30, info.header_offset)
            if len(hdr) != 30 or hdr[:4] != b"PK\x03\x04":
                raise zipfile.BadZipFile(f"bad local header of member {key!r}")
            off = info.header_offset + 30 + int.from_bytes(hdr[26:28], "little") + int.from_bytes(hdr[28:30], "little")
            self._data_off[key] = off
        n, size = 0, info.file_size
        while n < size:
            got = os.preadv(self._fd, [out[n:size]], off + n)
            if got <= 0:
                raise EOFError(f"member {key!r} ends after {n} of {size} bytes")
            n += got
        if zlib.crc32(out[:size]) != info.CRC:
            raise zipfile.BadZipFile(f"bad CRC-32 of member {key!r}")
        return size


Store = Union[DirectoryStore, ZipStore]


def _open_store(path: Union[str, Path]) -> Store:
    p = Path(path)
    if not p.exists():
        raise FileNotFoundError(f"{p} does not exist")
    if p.is_dir():
        return DirectoryStore(p)
    if zipfile.is_zipfile(p):
        return ZipStore(p)
    raise ValueError(f"{p} is neither a directory store nor a zip store")


def _blosc_document(compressor: Optional[dict]) -> bool:
    """a Blosc compressor document as numcodecs writes it, every key of its configuration present (zarr never writes less).
    Only such a one is read here without numcodecs: the defaults of a shorter document are numcodecs' to choose."""
    return bool(compressor) and compressor.get("id") == "blosc" and all(k in compressor for k in ("cname", "clevel", "shuffle", "blocksize"))


def _decoder(compressor: Optional[dict], where: str, chunk_nbytes: int) -> Optional[Callable[[bytes], bytes]]:
    """compressed chunk bytes -> decoded bytes for a ``compressor`` document of .zarray (None: the chunk is stored raw)"""
    if compressor is None:
        return None
    cid = compressor.get("id")
    if cid == "zlib":
        return zlib.decompress
    if cid == "gzip":
        return lambda data: zlib.decompress(data, 16 + zlib.MAX_WBITS)
    if cid == "bz2":
        return bz2.decompress
    try:
        import numcodecs
    except ImportError:
        if _blosc_document(compressor):
            from yogo_amd import blosc, zstd

            frame = zstd.frame_decoder() if compressor.get("cname") == "zstd" else None
            return lambda data: blosc.decompress(data, chunk_nbytes, zstd=frame)
        if cid == "zstd":
            from yogo_amd import zstd

            frame = zstd.frame_decoder()
            return lambda data: frame(bytes(data), chunk_nbytes)
        raise NotImplementedError(f"zarr store {where}: compressor {cid!r} needs the numcodecs package, which is not installed "
                                  "(null, zlib, gzip and bz2 are read without it)") from None
    codec = numcodecs.get_codec(dict(compressor))
    return lambda data: bytes(codec.decode(data))


_READ_ERRORS = (zlib.error, OSError, EOFError, zipfile.BadZipFile, ValueError)


class ChunkTooLong(Exception):
    """ZarrArray.read_stored_into: the stored chunk is longer than the caller's buffer"""


class ZarrArray:
    """One uint8 array of a store: 3-D ``[H, W, N]`` (``a[:, :, idx]`` -> frame) or 2-D ``[H, W]`` (``a[:]`` -> frame)."""

    def __init__(self, store: Store, prefix: str = ""):
        self.store, self.prefix = store, prefix
        self.where = store.path + (f" ({prefix.rstrip('/')})" if prefix else "")
        try:
            meta = json.loads(store.get(prefix + ".zarray"))
        except KeyError:
            raise ValueError(f"zarr store {self.where}: no .zarray") from None
        if meta.get("zarr_format") != 2:
            raise ValueError(f"zarr store {self.where}: zarr_format {meta.get('zarr_format')!r}, only 2 is read")
        if meta.get("dtype") != "|u1":
            raise ValueError(f"zarr store {self.where}: dtype {meta.get('dtype')!r}, only '|u1' (uint8) is read")
        if meta.get("filters"):
            names = ", ".join(str(f.get("id")) for f in meta["filters"])
            raise NotImplementedError(f"zarr store {self.where}: filters are not supported (got {names})")
        self.shape = tuple(int(v) for v in meta["shape"])
        self.chunks = tuple(int(v) for v in meta["chunks"])
        if len(self.shape) not in (2, 3) or len(self.chunks) != len(self.shape) or min(self.chunks) < 1 or min(self.shape) < 0:
            raise ValueError(f"zarr store {self.where}: shape {self.shape} / chunks {self.chunks}: an [H, W, N] or [H, W] array is expected")
        self.ndim = len(self.shape)
        self.order = meta.get("order", "C")
        if self.order not in ("C", "F"):
            raise ValueError(f"zarr store {self.where}: order {self.order!r}")
        fill = meta.get("fill_value")
        self.fill_value = 0 if fill is None else int(fill)
        if not 0 <= self.fill_value <= 255:
            raise ValueError(f"zarr store {self.where}: fill_value {fill!r} is no uint8")
        self.separator = meta.get("dimension_separator", ".")
        if self.separator not in (".", "/"):
            raise ValueError(f"zarr store {self.where}: dimension_separator {self.separator!r}")
        self.compressor = meta.get("compressor")
        self.chunk_nbytes = int(np.prod(self.chunks, dtype=np.int64))
        self._decode = _decoder(self.compressor, self.where, self.chunk_nbytes)
        self.grid = tuple(-(-s // c) for s, c in zip(self.shape, self.chunks))
        sep = re.escape(self.separator)
        self._key_re = re.compile(re.escape(prefix) + r"\d+(?:" + sep + r"\d+){" + str(self.ndim - 1) + r"}$")

    def with_store(self, store: Store) -> "ZarrArray":
        """the same array read through another handle of the store (one per thread: a ZipFile handle is not to be shared)"""
        other = ZarrArray.__new__(ZarrArray)
        other.__dict__.update(self.__dict__)
        other.store = store
        return other

    @property
    def raw(self) -> bool:
        """chunks are stored as they are (no compressor)"""
        return self._decode is None

    @property
    def device_decodable(self) -> bool:
        """Blosc only: the stored chunks may be handed to yogo_blosc_lz4_decode (Blosc with LZ4 blocks, not bit-shuffled).  The
        feed asks ``device_codec``, which also knows the zlib codec's device route."""
        c = self.compressor
        return _blosc_document(c) and c.get("cname") in ("lz4", "lz4hc") and c.get("shuffle") in (0, 1)

    @property
    def device_codec(self) -> Optional[str]:
        """which device decoder the feed hands the stored chunks to: "blosc" (device_decodable), "zlib" (the zlib codec: one
        stream per chunk for yogo_inflate_zlib), "blosc-zstd" (Blosc with one Zstandard frame per block, not bit-shuffled) or
        "zstd" (the zstd codec: one frame per chunk), both for yogo_zstd_decode, or None"""
        if self.device_decodable:
            return "blosc"
        c = self.compressor
        if _blosc_document(c) and c.get("cname") == "zstd" and c.get("shuffle") in (0, 1):
            return "blosc-zstd"
        if c and c.get("id") == "zstd":
            return "zstd"
        if self.compressor and self.compressor.get("id") == "zlib":
            return "zlib"
        return None

    def chunk_key(self, coords: Sequence[int]) -> str:
        return self.prefix + self.separator.join(str(int(c)) for c in coords)

    def has_chunk(self, coords: Sequence[int]) -> bool:
        return self.chunk_key(coords) in self.store

    @property
    def initialized(self) -> int:
        """the number of chunk keys present in the store"""
        return sum(1 for k in self.store.keys() if self._key_re.match(k))

    def __len__(self) -> int:
        return self.initialized

    def read_chunk_into(self, coords: Sequence[int], out) -> None:
        """the decoded bytes of one chunk (chunk_nbytes of them, in the array's order) into the writable buffer ``out``.
        KeyError when the key is absent; RuntimeError naming the key when it cannot be read or decoded."""
        key = self.chunk_key(coords)
        mv = memoryview(out).cast("B")
        n = self.chunk_nbytes
        if len(mv) != n:
            raise ValueError(f"read_chunk_into: a buffer of {len(mv)} bytes for a chunk of {n}")
        try:
            if self._decode is None:
                got = self.store.readinto(key, mv)
            else:
                data = self._decode(self.store.get(key))
                got = len(data)
                if got == n:
                    mv[:] = data
            if got != n:
                raise ValueError(f"{got} bytes after decoding, {n} expected")
        except KeyError:
            raise
        except _READ_ERRORS as e:
            raise RuntimeError(f"zarr store {self.where}: chunk {key!r} could not be read ({type(e).__name__}: {e})") from e
        except Exception as e:   # a numcodecs codec raises its own classes
            raise RuntimeError(f"zarr store {self.where}: chunk {key!r} could not be decoded ({type(e).__name__}: {e})") from e

    def read_stored_into(self, coords: Sequence[int], out) -> int:
        """the stored bytes of one chunk as they are (before the compressor) into the front of the writable buffer ``out`` ->
        how many.  KeyError when the key is absent; ChunkTooLong when ``out`` is too short; RuntimeError naming the key when the
        chunk cannot be read."""
        key = self.chunk_key(coords)
        mv = memoryview(out).cast("B")
        try:
            stored = self.store.nbytes(key)
            if stored > len(mv):
                raise ChunkTooLong(f"zarr store {self.where}: chunk {key!r} holds {stored} bytes, the buffer {len(mv)}")
            return self.store.readinto(key, mv[:stored])
        except (KeyError, ChunkTooLong):
            raise
        except _READ_ERRORS as e:
            raise RuntimeError(f"zarr store {self.where}: chunk {key!r} could not be read ({type(e).__name__}: {e})") from e

    def read_chunk(self, coords: Sequence[int]) -> Optional[np.ndarray]:
        """one chunk as an array of the chunk shape, or None when its key is absent"""
        buf = np.empty(self.chunk_nbytes, dtype=np.uint8)
        try:
            self.read_chunk_into(coords, buf)
        except KeyError:
            return None
        return buf.reshape(self.chunks, order=self.order)

    def frame(self, idx: Optional[int] = None) -> np.ndarray:
        """frame ``idx`` of an [H, W, N] array, or the whole of an [H, W] array, as a uint8 [H, W] array"""
        H, W = self.shape[:2]
        ch, cw = self.chunks[:2]
        if self.ndim == 3:
            if idx is None:
                raise IndexError("a frame index is needed for a 3-D array")
            idx = int(idx)
            if idx < 0:
                idx += self.shape[2]
            if not 0 <= idx < self.shape[2]:
                raise IndexError(f"index {idx} is out of bounds for axis 2 with size {self.shape[2]}")
            tk, k = divmod(idx, self.chunks[2])
        out = np.full((H, W), self.fill_value, dtype=np.uint8)
        for ty in range(self.grid[0]):
            for tx in range(self.grid[1]):
                c = self.read_chunk((ty, tx, tk) if self.ndim == 3 else (ty, tx))
                if c is None:
                    continue
                y0, x0 = ty * ch, tx * cw
                h, w = min(ch, H - y0), min(cw, W - x0)
                out[y0:y0 + h, x0:x0 + w] = c[:h, :w, k] if self.ndim == 3 else c[:h, :w]
        return out

    def __getitem__(self, item) -> np.ndarray:
        full = slice(None)
        if self.ndim == 3 and isinstance(item, tuple) and len(item) == 3 and item[0] == full and item[1] == full \
                and isinstance(item[2], (int, np.integer)):
            return self.frame(int(item[2]))
        if self.ndim == 2 and (item is Ellipsis or item == full or item == (full, full)):
            return self.frame()
        raise NotImplementedError(f"ZarrArray: only a[:, :, idx] (3-D) and a[:] (2-D) are read, got {item!r}")


class ZarrGroup:
    """A group whose members "0", "1", ... are 2-D arrays: ``g[idx][:]`` is frame idx."""

    def __init__(self, store: Store):
        self.store = store
        self.where = store.path
        meta = json.loads(store.get(".zgroup"))
        if meta.get("zarr_format") != 2:
            raise ValueError(f"zarr store {self.where}: zarr_format {meta.get('zarr_format')!r}, only 2 is read")
        self.members = sorted((k[:-len("/.zarray")] for k in store.keys() if k.endswith("/.zarray") and k.count("/") == 1),
                              key=lambda s: (not s.isdigit(), int(s) if s.isdigit() else 0, s))
        self._arrays: Dict[str, ZarrArray] = {}

    def __len__(self) -> int:
        return len(self.members)

    def __getitem__(self, idx: Union[int, str]) -> ZarrArray:
        name = str(idx)
        if name not in self._arrays:
            if name + "/.zarray" not in self.store:
                raise IndexError(f"zarr store {self.where}: the group has no member {name!r}")
            self._arrays[name] = ZarrArray(self.store, name + "/")
        return self._arrays[name]


def open_zarr(path: Union[str, Path]) -> Union[ZarrArray, ZarrGroup]:
    """``zarr.open(path, mode="r")`` for the two kinds of root the reference reads.  FileNotFoundError for a missing path,
    ValueError for a store that holds neither an array nor a group (an empty one)."""
    store = _open_store(path)
    if ".zarray" in store:
        return ZarrArray(store)
    if ".zgroup" in store:
        return ZarrGroup(store)
    raise ValueError(f"zarr store {store.path}: neither .zarray nor .zgroup at its root (an empty store?)")

