"""The case set of tests/_loss_cases.py on the host: the two references take the same branches, the per-cell reference is the reference
program, a numpy float32 transcription of decode_loss.hip meets the bound that the kernels are held to on the GPU
(tests/test_gpu_loss_edges.py), and thirteen wrong variants of that transcription, plus the log-softmax that
always folds max + log(sum), do not.
"""
import numpy as np
import pytest
import torch

import _loss_cases as L
import yogo_oracle as O
from _util import LOSS_EDGE_M as M, as_t, load_npz

F32 = np.float32


def _raw_decoded(dtype):
    rb = L.raw_batch()
    x = torch.from_numpy(rb.raw.copy()).to(dtype)
    return L.cells_first(O.decode(x, rb.cxs.to(dtype), rb.cys.to(dtype), *L.ANCHORS).numpy())


def test_case_set_holds_what_it_promises():
    fams = {f.split("/")[0] for g in L.groups() for f in g.fam}
    for want in ("generic", "identical", "pred_contains_label", "label_contains_pred", "tie_x1", "tie_y1", "tie_x2", "tie_y2", "touching", "disjoint",
                 "corner_on_border", "corner_just_outside", "clamp_meets_label_on_border", "all_four_clamped", "size_2^33", "pred_beside_image",
                 "tiny_size", "square", "zero_area", "hp0", "ce_equal_logits", "ce_logits_+-1e4", "ce_logits_2^-20_apart", "ce_max_at_fold", "ce_max_past_fold", "ce_max_at_-fold",
                 "ce_max_past_-fold", "objectness_pred=mask"):
        assert want in fams, want
    assert {g.P - 5 for g in L.groups()} == {1, 2, 7, 64}
    assert {g.w[3] for g in L.groups()} == {0.0, 0.01, 0.1} and {g.w[0] for g in L.groups()} == {0.0, 0.25, 0.5, 1.0}
    assert sum(int(g.hp0.sum()) for g in L.groups()[:1]) == 1
    g = L.groups()[0]
    z = [i for i, f in enumerate(g.fam) if f.startswith("zero_area")]
    p64 = g.pred[z].astype(np.float64)
    assert not L.live32(g.pred, g.label)[z].any()                    # filtered in float32 ...
    assert (p64[:-1, 0] - 0.5 * p64[:-1, 2] != p64[:-1, 0] + 0.5 * p64[:-1, 2]).any()   # ... where float64 alone would not filter
    rb = L.raw_batch()
    assert float(rb.raw[:, 2:4].max()) == 90.0 and (rb.raw[:, 2:4] == F32(L.T80_UP)).any() and (rb.raw[:, 2:4] == 80.0).any()
    assert L.T80_UP > 80.0


def test_both_precisions_take_the_same_branches():
    """clamp masks (and corners exactly on 0 / 1), `has`, the max / min orderings with their ties, and the exp clamp: float32 and float64
    decide alike on EVERY case -- none is left out.  The zero-area filter is float32's by construction."""
    seen = np.zeros(13, dtype=bool)
    for g in L.groups():
        live = L.live32(g.pred, g.label)
        d32, d64 = L.decisions(g.pred, g.label, F32, live), L.decisions(g.pred, g.label, np.float64, live)
        assert np.array_equal(d32, d64), g.name
        seen |= (d32 != 0).any(0)
    assert seen.all()
    # raw level: the float32 decode against the float64 decode
    rb = L.raw_batch()
    p32, p64 = _raw_decoded(torch.float32), _raw_decoded(torch.float64)
    assert p32.dtype == F32 and p64.dtype == np.float64
    lab = L.cells_first(rb.label)
    live = L.live32(p32, lab)
    d32, d64 = L.decisions(p32, lab, F32, live), L.decisions(p64, lab, np.float64, live)
    assert np.array_equal(d32, d64), np.nonzero((d32 != d64).any(1))[0][:10]
    raw = L.cells_first(rb.raw)
    assert np.array_equal(raw[:, 2:4] <= F32(80), raw[:, 2:4].astype(np.float64) <= 80.0)
    # the raw cases do reach the edges: boxes that leave the image tie with labels on its border, inside `has`
    tie = (d32[:, 9:] == 0) & live[:, None]
    assert tie[:, 0].sum() > 100 and tie[:, 2].sum() > 100 and (tie.all(1) & (d32[:, 8] == 1)).sum() > 50
    assert (~live & (lab[:, 0] != 0)).sum() > 100                    # zero-area boxes from t = -20 / -100
    assert live.sum() > 500


@pytest.mark.parametrize("fix", ["loss_2x12x13x17", "loss_3x9x24x33"])
def test_per_cell_reference_is_the_reference_program(fix):
    """ref32 per cell, summed and weighted as yogo_loss.py does, reproduces the fixtures that the reference's own yogo_loss.py wrote"""
    z = load_npz(fix + ".npz")
    B = z["pred"].shape[0]
    for suffix in ("", "_w2"):
        zz = load_npz(fix + suffix + ".npz")
        w = tuple(float(v) for v in zz["weights"])
        r = L.ref_cells(z["pred"], z["label"], w, torch.float32, 1.0 / B)
        iou, obj, cls = (float(v) for v in r["val"].sum(1) / B)
        comps = [w[1] * iou, obj, w[2] * cls]
        np.testing.assert_allclose(comps, zz["comps"], rtol=2e-5)
        assert abs(sum(comps) - float(zz["loss"])) <= 2e-5 * abs(float(zz["loss"]))
        grad = torch.from_numpy(r["grad"].reshape(B, -1, z["pred"].shape[1]).transpose(0, 2, 1).reshape(z["pred"].shape).copy()).float()
        torch.testing.assert_close(grad, as_t(zz["grad"]), rtol=2e-4, atol=1e-6)


def test_per_cell_reference_is_the_oracle_loss():
    B, C, Sy, Sx = 3, 7, 12, 16
    raw = torch.randn(B, 5 + C, Sy, Sx, generator=torch.Generator().manual_seed(5))
    pred = O.decode(raw, *O.make_grids(Sx, Sy), 0.0425, 0.0555).requires_grad_(True)
    label = O.synthetic_labels(B, Sx, Sy, K=20, num_classes=C, seed=6)
    loss, comps = O.yogo_loss(pred, label)
    loss.backward()
    r = L.ref_cells(pred.detach().numpy(), label.numpy(), L.DEFAULT_W, torch.float32, 1.0 / B)
    iou, obj, cls = (float(v) for v in r["val"].sum(1) / B)
    np.testing.assert_allclose([5.0 * iou, obj, cls], [comps["iou_loss"], comps["objectness_loss"], comps["classification_loss"]], rtol=2e-5)
    grad = torch.from_numpy(r["grad"].reshape(B, Sy * Sx, 5 + C).transpose(0, 2, 1).reshape(pred.shape).copy()).float()
    torch.testing.assert_close(grad, pred.grad, rtol=2e-4, atol=1e-6)


def _transcription_ratios(var=()):
    """-> {family: [gradient ratio, value ratio]} of the numpy transcription (with the wrong variants `var`) over every case"""
    out = {}

    def note(fam, r, k):
        for f, v in L.by_family(fam, r).items():
            out.setdefault(f, [0.0, 0.0])[k] = max(out.setdefault(f, [0.0, 0.0])[k], v)

    for i, g in enumerate(L.groups()):
        r32, r64 = L.group_refs(i)
        val, grad = L.k_loss(g.pred, g.label, g.w, 1.0, var)
        note(g.fam, L.ratios(grad, r32["grad"], r64["grad"]), 0)
        note(g.fam, L.ratios(val.T, r32["val"].T, r64["val"].T), 1)
    rb = L.raw_batch()
    r32, r64 = L.raw_refs()
    val, graw, _ = L.k_chain(rb, var)
    note(rb.fam, L.ratios(graw, r32["grad"], r64["grad"]), 0)
    note(rb.fam, L.ratios(val.T, r32["val"].T, r64["val"].T), 1)
    raw = L.cells_first(rb.raw)
    cxs, cys = np.tile(rb.cxs.numpy().reshape(-1), rb.B), np.tile(rb.cys.numpy().reshape(-1), rb.B)
    inv_sx, inv_sy = F32(1.0 / rb.Sx), F32(1.0 / rb.Sy)
    for inference in (0, 1):
        gout, ((o32, g32), (o64, g64)) = L.decode_refs(inference)
        o = L.k_decode(raw, cxs, cys, inv_sx, inv_sy, L.ANCHORS, inference)
        d = L.k_decode_bwd(raw, o, L.cells_first(gout), inv_sx, inv_sy, inference, var)
        fam = [f"decode_inference{inference}/" + f.split("/")[1] for f in rb.fam]
        note(fam, L.ratios(d, g32, g64), 0)
        note(fam, L.ratios(o, o32, o64), 1)
    return out


def test_transcription_meets_the_bound():
    """the kernels' statements in numpy float32 (CIoU, cross-entropy, objectness, decode, decode backward in both modes, the chain)
    stay within M s of float64 on every case"""
    table = _transcription_ratios()
    for f, (rg, rv) in sorted(table.items()):
        print(f"{f:40s} gradient {rg:7.2f}  value {rv:7.2f}")
    worst = max(max(v) for v in table.values())
    assert worst <= M, sorted(table.items(), key=lambda kv: -max(kv[1]))[:5]


@pytest.mark.parametrize("var", L.VARIANTS)
def test_wrong_variant_is_rejected(var):
    table = _transcription_ratios((var,))
    worst = max(max(v) for v in table.values())
    print(var, worst)
    assert worst >= 4 * M, (var, worst)


def test_eps_in_alpha_cannot_be_seen():
    """Dropping eps from alpha's denominator is not a wrong variant that this bound could reject, and here is why.  I <= U, so
    iou = I / (U + eps) <= 1 - eps / (U + eps): the denominator 1 - iou + v is positive without its eps, and at least
    delta + v with delta = eps / (U + eps).  alpha v = v^2 / (delta' + v + eps) then moves by at most eps (v / (v + delta'))^2 <= eps
    = 1e-7, below the float32 spacing of a loss of order one, and the gradient by the same relative amount.  Asserted: the inequality
    on every case, and that the variant stays inside the bound."""
    for g in L.groups():
        live = L.live32(g.pred, g.label)
        p, lb = g.pred.astype(np.float64), g.label.astype(np.float64)
        c = np.stack([p[:, 0] - 0.5 * p[:, 2], p[:, 1] - 0.5 * p[:, 3], p[:, 0] + 0.5 * p[:, 2], p[:, 1] + 0.5 * p[:, 3]], 1).clip(0, 1)
        iw = np.minimum(c[:, 2], lb[:, 3]) - np.maximum(c[:, 0], lb[:, 1])
        ih = np.minimum(c[:, 3], lb[:, 4]) - np.maximum(c[:, 1], lb[:, 2])
        I = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
        U = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1]) + (lb[:, 3] - lb[:, 1]) * (lb[:, 4] - lb[:, 2]) - I
        iou = I / (U + L.EPS)
        ok = 1 - iou >= L.EPS / (U + L.EPS) - 2.0 ** -50          # (the float64 roundings of two quotients that are at most 1)
        assert ok[live].all(), g.name
    table = _transcription_ratios(("no_eps_alpha",))
    assert max(max(v) for v in table.values()) <= M


def test_zero_height_clamp_is_the_stated_deviation():
    """hp == 0 (a box clamped to zero height, non-zero width): reference autograd gives NaN in the x components (0 * inf in the
    atan(w / h) chain); the kernel's arithmetic gives the finite limit.  The decode cannot produce it (cy lies inside [Y1, Y2])."""
    g = L.groups()[0]
    i = int(np.nonzero(g.hp0)[0][0])
    r32, r64 = L.group_refs(0)
    assert np.isnan(r64["grad"][i, [0, 2]]).all() and np.isfinite(r64["grad"][i, [1, 3, 4, 5, 6]]).all() and np.isfinite(r64["val"][:, i]).all()
    val, grad = L.k_loss(g.pred, g.label, g.w)
    assert np.isfinite(grad[i]).all()
    assert L.ratios(grad[i:i + 1], r32["grad"][i:i + 1], r64["grad"][i:i + 1])[0] <= M      # y, objectness and class components
    assert L.ratios(val.T[i:i + 1], r32["val"].T[i:i + 1], r64["val"].T[i:i + 1])[0] <= M
