"""The fp64 oracle of the antialiased bilinear resize (``resize_image``: torchvision's ``Resize(image_hw, antialias=True)``), in
dense-matrix form, and the rules the tests hold the implementations to.  A restatement of the definition that shares nothing with
yogo_amd/resize.py; product code does not import it.

Definition, one axis n_in -> n_out (torch._upsample_bilinear2d_aa, align_corners=False): scale = n_in / n_out, support =
max(scale, 1); output i has its centre at c = scale * (i + 0.5) and takes the source indices lo <= j < hi, lo = max(0, int(c -
support + 0.5)), hi = min(n_in, int(c + support + 0.5)), with the triangle weights max(0, 1 - |j + 0.5 - c| / support) divided by
their sum.  ``aa_matrix`` is that as an [n_out, n_in] matrix; the resized image is ``Wy @ img @ Wx.T`` (``exact``), the result
``rint`` of it (half-even; a convex combination of 0 .. 255 needs no clamp).

With v the exact value of a pixel and f = |v - floor(v) - 0.5| its distance to the rounding edge:
  rule D / H (``assert_rule``)  the output equals rint(v) wherever f >= tol, and differs from it by at most 1 elsewhere.
      tol = 1e-3 for the fp32 implementations (the kernel, its numpy twin): two fp32 passes of K fused multiply-adds on values up to
      255 with weights rounded to fp32 err by at most about 2 (K + 2) 2^-24 255 = 3.7e-4 at K = 10 (scales up to 4 x, which the
      tests stay within); tol = 2e-3 for ``resize_image`` itself, whose fp32 weights deviate by up to 1.24e-3 (measured).
  rule E (``assert_exact_interior``)  on an exact 2 x down-scale the interior taps are 1/8, 3/8, 3/8, 1/8 and fp32 is exact: every
      output pixel outside the first and last row and column equals rint(v), ties included -- what tells rintf from floor(x + 0.5).
  cap (``assert_cap``)  the pixels rule D excuses (0 < f < 1e-3; the exact ties are rule E's) are at most 1 % of an image; it is
      asserted on the oracle before anything is compared, so that the excuse cannot grow into the rule.
"""
import numpy as np

TOL_FP32 = 1e-3
TOL_TORCH = 2e-3
CAP = 0.01


def aa_matrix(n_in: int, n_out: int) -> np.ndarray:
    W = np.zeros((n_out, n_in), dtype=np.float64)
    scale = n_in / n_out
    support = max(scale, 1.0)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        for j in range(lo, hi):
            W[i, j] = max(0.0, 1.0 - abs(j + 0.5 - c) / support)
        W[i] /= W[i].sum()
    return W


def exact(img: np.ndarray, hw) -> np.ndarray:
    """uint8 [..., Hs, Ws] -> float64 [..., hw[0], hw[1]]"""
    Wy, Wx = aa_matrix(img.shape[-2], hw[0]), aa_matrix(img.shape[-1], hw[1])
    return Wy @ img.astype(np.float64) @ Wx.T


def edge_distance(v: np.ndarray) -> np.ndarray:
    return np.abs(v - np.floor(v) - 0.5)


def assert_cap(v: np.ndarray) -> None:
    """v: [n, C, H, W].  Per image: at most CAP of its pixels lie within TOL_FP32 of a rounding edge without being on it"""
    f = edge_distance(v)
    near = ((f < TOL_FP32) & (f != 0)).reshape(v.shape[0], -1).mean(axis=1)
    assert float(near.max()) <= CAP, near


def assert_rule(got: np.ndarray, v: np.ndarray, tol: float, what: str = "") -> int:
    """-> the number of pixels that used the excuse"""
    want = np.rint(v).astype(np.int64)
    d = np.abs(got.astype(np.int64) - want)
    f = edge_distance(v)
    firm = f >= tol
    print(f"{what}: {int((d != 0).sum())} of {d.size} pixels differ from rint(v), {int((d[firm] != 0).sum())} of them at f >= {tol}; "
          f"largest difference {int(d.max())}")
    assert not (d[firm] != 0).any(), (what, int((d[firm] != 0).sum()), float(f[firm & (d != 0)].max()))
    assert int(d.max()) <= 1, (what, int(d.max()))
    return int((d != 0).sum())


def assert_exact_interior(got: np.ndarray, v: np.ndarray, min_ties: int, rows: bool = True, cols: bool = True, what: str = "") -> None:
    """rule E on the pixels that are not in the first / last row (``rows``) or column (``cols``); the input must put at least
    ``min_ties`` exact ties there"""
    sl = (Ellipsis, slice(1, -1) if rows else slice(None), slice(1, -1) if cols else slice(None))
    vi, gi = v[sl], got[sl].astype(np.int64)
    ties = int((edge_distance(vi) == 0).sum())
    print(f"{what}: {ties} exact ties among {vi.size} interior pixels")
    assert ties >= min_ties, (what, ties)
    assert np.array_equal(gi, np.rint(vi).astype(np.int64)), (what, int((gi != np.rint(vi)).sum()))


def images(n: int, C: int, H: int, W: int, seed: int) -> np.ndarray:
    """uint8 [n, C, H, W]: image 0 noise, image 1 smooth plus noise, the others noise again"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(n, C, H, W), dtype=np.uint8)
    if n > 1:
        y, x = np.mgrid[0:H, 0:W]
        for c in range(C):
            smooth = 128 + 100 * np.sin(x / (7.0 + c) + 0.3 * c) * np.cos(y / (5.0 + 2 * c))
            out[1, c] = np.clip(np.rint(smooth + rng.normal(0, 6, size=(H, W))), 0, 255).astype(np.uint8)
    return out
