"""A small Zarr v2 writer for the tests, after the published storage specification (the `zarr` package is not needed): the
`.zarray` / `.zgroup` JSON documents and one value per chunk under `i.j.k` / `i/j/k`, every chunk at the full chunk shape
(edge chunks padded with the fill value), in C or F order, raw or through zlib / gzip.  Directory or zip stores.

The reader under test (yogo_amd/zarr_store.py) and this writer share an author; tests/test_zarr_store_host.py holds one test
against the real package for the machines that have it."""
import gzip
import itertools
import json
import os
import zipfile
import zlib

import numpy as np


def _encode(raw: bytes, compressor):
    if compressor is None:
        return raw
    if compressor == "zlib":
        return zlib.compress(raw, 1)
    if compressor == "gzip":
        return gzip.compress(raw, 1)
    raise ValueError(compressor)


def _compressor_doc(compressor):
    if compressor is None or isinstance(compressor, dict):
        return compressor
    return {"id": compressor, "level": 1}


def array_members(a, chunks, *, compressor=None, order="C", separator=".", fill_value=0, skip=(), shape=None, dtype="|u1",
                  filters=None, write_separator=True, prefix=""):
    """{key: bytes} of one array.  a: uint8 array (2-D or 3-D); skip: chunk coordinates left out of the store; shape: the
    declared shape when it is to be larger than what is written; compressor: None, "zlib", "gzip", or a document written as it
    is (its chunks are then stored raw)."""
    a = np.asarray(a, dtype=np.uint8)
    chunks = tuple(int(c) for c in chunks)
    meta = {"zarr_format": 2, "shape": list(shape or a.shape), "chunks": list(chunks), "dtype": dtype, "order": order,
            "fill_value": fill_value, "filters": filters, "compressor": _compressor_doc(compressor)}
    if write_separator:
        meta["dimension_separator"] = separator
    out = {prefix + ".zarray": json.dumps(meta).encode()}
    grid = [-(-s // c) for s, c in zip(a.shape, chunks)]
    for coords in itertools.product(*(range(g) for g in grid)):
        if tuple(coords) in {tuple(s) for s in skip}:
            continue
        block = np.full(chunks, 0 if fill_value is None else fill_value, dtype=np.uint8)
        sl = tuple(slice(c * n, min((c + 1) * n, s)) for c, n, s in zip(coords, chunks, a.shape))
        part = a[sl]
        block[tuple(slice(0, d) for d in part.shape)] = part
        raw = block.tobytes(order=order)
        out[prefix + separator.join(map(str, coords))] = _encode(raw, None if isinstance(compressor, dict) else compressor)
    return out


def write_members(path, members, *, as_zip=False, deflate=False):
    """a {key: bytes} mapping as a directory store, or as a zip store (members stored, or deflated)"""
    path = str(path)
    if as_zip:
        with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED if deflate else zipfile.ZIP_STORED) as zf:
            for k, v in members.items():
                zf.writestr(k, v)
    else:
        for k, v in members.items():
            f = os.path.join(path, *k.split("/"))
            os.makedirs(os.path.dirname(f), exist_ok=True)
            with open(f, "wb") as fh:
                fh.write(v)
    return path


def write_stack(path, stack, chunks, *, as_zip=False, deflate=False, **kw):
    """an [H, W, N] stack as an array at the root of a store"""
    return write_members(path, array_members(stack, chunks, **kw), as_zip=as_zip, deflate=deflate)


def write_group(path, frames, chunks, *, as_zip=False, **kw):
    """2-D frames as the members "0", "1", ... of a group at the root of a store"""
    members = {".zgroup": json.dumps({"zarr_format": 2}).encode()}
    for i, f in enumerate(frames):
        members.update(array_members(f, chunks, prefix=f"{i}/", **kw))
    return write_members(path, members, as_zip=as_zip)
