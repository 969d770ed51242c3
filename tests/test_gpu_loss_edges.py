"""decode_loss.hip against float64 at its branch edges: the cases, references and bound of tests/_loss_cases.py (the host side of the
same set is tests/test_loss_edges_host.py).  Every cell of every launch is held to |kernel - ref64| <= M s, s = max(|ref32 - ref64|,
ulp32(max |ref64|)) over the cell's components; each test prints its largest ratio per family before it asserts (pytest -s), which is
where the table in DESIGN.md section 4 and LOSS_EDGE_M come from.
"""
import functools

import numpy as np
import pytest
import torch

import _loss_cases as L
from _util import LOSS_EDGE_M as M

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -768.0                   # (a bf16 value)
TAIL = 1024
SUM_ROUNDINGS = 12 * 2.0 ** -24     # an 8-level float32 tree within a workgroup and its 3 adds, the weighting and the store; then float64


def H():
    from yogo_amd import _hip

    return _hip


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def show(what, table):
    for f, v in sorted(table.items()):
        print(f"[{what}] {f:40s} {v:8.2f}")


def run_loss(pred, label, w):
    """yogo_loss_fwd_bwd on a packed batch -> (grad [n, P] numpy, loss_out [4] numpy); the gradient buffer starts as NaN, the TAIL floats
    behind it and behind loss_out as a sentinel that must survive"""
    h = H()
    B, P, Sy, Sx = pred.shape
    n = pred.size
    buf = torch.full((n + TAIL,), float("nan"), device="cuda")
    buf[n:] = SENTINEL
    out = torch.full((4 + TAIL,), SENTINEL, device="cuda")
    ws = torch.zeros(h.query_size("yogo_loss_workspace_bytes", B, Sy, Sx) // 4, device="cuda")
    h.call("yogo_loss_fwd_bwd", dev(pred), dev(label), buf, out, ws, B, P, Sy, Sx, *w, h.stream_ptr())
    torch.cuda.synchronize()
    buf, out = buf.cpu(), out.cpu()
    assert bool((buf[n:] == SENTINEL).all()) and bool((out[4:] == SENTINEL).all()), "a write past the end of the gradient / loss buffer"
    return L.cells_first(buf[:n].view(B, P, Sy, Sx).numpy()), out[:4].numpy()


@functools.lru_cache(maxsize=None)
def packed(i):
    """group i packed onto the 17 x 19 grid with its two references (computed once, read-only)"""
    g = L.groups()[i]
    pred, label, case = L.pack(g, fill=None if i <= 1 else "cycle")     # (the geometry groups fill the grid themselves and leave empty cells)
    B = pred.shape[0]
    refs = tuple(L.ref_cells(pred, label, g.w, dt, 1.0 / B) for dt in (torch.float32, torch.float64))
    for a in (pred, label, case):
        a.setflags(write=False)
    return pred, label, case, refs


def sum_bound(r32, r64, weights, inv_batch):
    """-> (want [4], bound [4]) of loss_out = (total, iou, objectness, classification): every term is non-negative, so a component lies
    within sum_cells M s_value + 12 * 2^-24 * sum ref64 of the float64 sum; the total adds two float32 additions"""
    assert (r64["val"] >= 0).all()
    s = L.scale(r32["val"].T, r64["val"].T)
    wk = np.asarray([weights[1], 1.0, weights[2]]) * inv_batch
    want = r64["val"].sum(1) * wk
    bound = (M * s.sum() + SUM_ROUNDINGS * r64["val"].sum(1)) * wk
    return np.concatenate([[want.sum()], want]), np.concatenate([[bound.sum() + 2 * 2.0 ** -24 * want.sum()], bound])


@pytest.mark.parametrize("i", range(len(L.groups())), ids=[g.name for g in L.groups()])
def test_loss_gradient_of_every_case(i):
    g = L.groups()[i]
    pred, label, case, (r32, r64) = packed(i)
    B, P, Sy, Sx = pred.shape
    assert B >= 2 and Sy * Sx == 323 and (i > 1 or all(case[c] >= 0 for c in (0, 63, 64, 255, 256, 322, 323 + 63)))
    grad, out = run_loss(pred, label, g.w)
    assert not np.isnan(grad).any(), "an element of the gradient was not written"
    assert np.isfinite(grad).all()
    fam = [g.fam[c] if c >= 0 else "empty_cell" for c in case]
    r = L.ratios(grad, r32["grad"], r64["grad"])
    show(f"loss gradient {g.name}", L.by_family(fam, r))
    assert r.max() <= M, (g.name, fam[int(r.argmax())], float(r.max()))
    lab = L.cells_first(label)
    empty = lab[:, 0] == 0
    assert empty.any() or i > 1
    assert (np.delete(grad[empty], 4, axis=1).view(np.int32) == 0).all(), "mask == 0: box and class gradients are exact zeros"
    hp0 = np.asarray([c >= 0 and g.hp0[c] for c in case])
    if hp0.any():      # the stated deviation: finite x components where reference autograd gives NaN
        assert np.isnan(r64["grad"][hp0][:, [0, 2]]).all() and np.isfinite(grad[hp0]).all()
    want, bound = sum_bound(r32, r64, g.w, 1.0 / B)
    print(f"[loss sums {g.name}] |d| / bound", np.abs(out - want) / bound)
    assert (np.abs(out - want) <= bound).all(), (out, want, bound)


def _value_cases():
    """one case per family and scale: (group index, case index)"""
    pick = []
    for i, g in enumerate(L.groups()):
        if i == 1:
            continue     # the C = 1 copy of the geometry group
        seen = set()
        for c, f in enumerate(g.fam):
            if f not in seen:
                seen.add(f)
                pick.append((i, c))
    return pick


def test_loss_value_of_a_cell_alone():
    """B = 1 on a 1 x 1 grid: loss_out[1..3] divided by its weight is that cell's term"""
    h = H()
    pick = _value_cases()
    assert 300 <= len(pick) <= 600, len(pick)
    outs = torch.full((len(pick), 4), SENTINEL, device="cuda")
    ws = torch.zeros(len(pick), 4, device="cuda")
    grads = torch.full((len(pick), 69), float("nan"), device="cuda")
    keep = []
    for k, (i, c) in enumerate(pick):
        g = L.groups()[i]
        p, lb = dev(g.pred[c]), dev(g.label[c])
        keep.append((p, lb))
        h.call("yogo_loss_fwd_bwd", p, lb, grads[k], outs[k], ws[k], 1, g.P, 1, 1, *g.w, h.stream_ptr())
    torch.cuda.synchronize()
    outs = outs.cpu().double().numpy()
    table, worst = {}, (0.0, None)
    for k, (i, c) in enumerate(pick):
        g = L.groups()[i]
        r32, r64 = L.group_refs(i)
        got = np.asarray([[outs[k, 1] / g.w[1], outs[k, 2], outs[k, 3] / g.w[2]]])
        r = float(L.ratios(got, r32["val"].T[c:c + 1], r64["val"].T[c:c + 1])[0])
        f = g.fam[c].split("/")[0]
        table[f] = max(table.get(f, 0.0), r)
        if r > worst[0]:
            worst = (r, (g.name, g.fam[c], got, r64["val"].T[c]))
    show("loss value", table)
    assert worst[0] <= M, worst


@pytest.mark.parametrize("shape", [(300, 2, 3, 0), (1, 260, 260, 1)], ids=["300_rows", "265_rows"])
def test_finalize_sums_more_than_256_partial_rows(shape):
    B, Sy, Sx, gi = shape
    g = L.groups()[gi]
    assert (g.P == 6) == (gi == 1)
    pred, label, case = L.pack(g, grid=(Sy, Sx), min_batch=B, fill="cycle")
    assert pred.shape == (B, g.P, Sy, Sx) and B * ((Sy * Sx + 255) // 256) in (300, 265)
    r32, r64 = L.group_refs(gi)
    r32, r64 = ({"val": r["val"][:, case]} for r in (r32, r64))
    want, bound = sum_bound(r32, r64, g.w, 1.0 / B)
    grad, out = run_loss(pred, label, g.w)
    print(f"[finalize {B}x{Sy}x{Sx}] |d| / bound", np.abs(out - want) / bound, "values", out)
    assert (np.abs(out - want) <= bound).all(), (out, want, bound)
    grad2, out2 = run_loss(pred, label, g.w)
    assert np.array_equal(out.view(np.int32), out2.view(np.int32)) and np.array_equal(grad.view(np.int32), grad2.view(np.int32))


@pytest.mark.parametrize("inference", [0, 1])
def test_decode_forward_and_backward(inference):
    h = H()
    rb = L.raw_batch()
    B, P, Sy, Sx = rb.raw.shape
    gout, ((o32, g32), (o64, g64)) = L.decode_refs(inference)
    raw, go = dev(rb.raw), dev(gout)
    cxs, cys = rb.cxs.cuda(), rb.cys.cuda()
    assert tuple(cxs.shape) == (Sy, Sx) and cxs.is_contiguous() and cys.is_contiguous()
    st = h.stream_ptr()
    out = torch.full_like(raw, float("nan"))
    h.call("yogo_decode_fwd", raw, out, cxs, cys, B, P, Sy, Sx, *L.ANCHORS, inference, st)
    g32k = torch.full_like(raw, float("nan"))
    h.call("yogo_decode_bwd", raw, out, go, g32k, B, P, Sy, Sx, inference, st)
    Pb = ((P + 15) // 16) * 2
    g16 = torch.full((B, Pb, Sy, Sx, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    h.call("yogo_decode_bwd_bf16", raw, out, go, g16, B, P, Sy, Sx, inference, st)
    torch.cuda.synchronize()
    o, d = L.cells_first(out.cpu().numpy()), L.cells_first(g32k.cpu().numpy())
    assert np.isfinite(o).all() and np.isfinite(d).all()
    fam = [f"decode_inference{inference}/" + f.split("/")[1] for f in rb.fam]
    ro, rd = L.ratios(o, o32, o64), L.ratios(d, g32, g64)
    show("decode forward", L.by_family(fam, ro))
    show("decode backward", L.by_family(fam, rd))
    assert ro.max() <= M, (fam[int(ro.argmax())], float(ro.max()))
    assert rd.max() <= M, (fam[int(rd.argmax())], float(rd.max()))
    # the exp clamp, exactly: the gradient passes at t == 80 and is zero above
    r, gf = L.cells_first(rb.raw), L.cells_first(gout)
    for k in (2, 3):
        at, above = r[:, k] == F32(80), r[:, k] > F32(80)
        assert at.sum() > 100 and (r[above, k] == F32(L.T80_UP)).sum() > 100 and (r[above, k] == F32(90)).sum() > 100
        assert np.array_equal(d[at, k], gf[at, k] * o[at, k]) and (np.abs(d[at, k]) > 1e25).all()
        assert (d[above, k].view(np.int32) == 0).all()
    # bf16 form: one bf16 rounding on top, padding channels zero
    full = g16.float().permute(0, 1, 4, 2, 3).reshape(B, Pb * 8, Sy, Sx).cpu()
    assert bool((full[:, P:].view(torch.int32) == 0).all())
    d16 = L.cells_first(full[:, :P].numpy()).astype(np.float64)
    s = L.scale(g32, g64)
    excess = np.abs(d16 - g64) - 2.0 ** -8 * np.abs(g64)
    r16 = excess.max(axis=1) / s
    show("decode backward bf16", L.by_family(fam, np.maximum(r16, 0)))
    assert r16.max() <= M, (fam[int(r16.argmax())], float(r16.max()))


def test_fused_decode_loss_backward_at_the_edges():
    """yogo_decode_loss_bwd_bf16, the kernel the trainer runs, on the raw-level cases under edge labels: bit-identical to the three calls
    (as tests/test_gpu_round2.py holds it on random inputs) and within one bf16 rounding + M s of the float64 chain
    decode -> loss -> decode backward"""
    h = H()
    rb = L.raw_batch()
    B, P, Sy, Sx = rb.raw.shape
    r32, r64 = L.raw_refs()
    raw, lab = dev(rb.raw), dev(rb.label)
    cxs, cys = rb.cxs.cuda(), rb.cys.cuda()
    st = h.stream_ptr()
    nws = h.query_size("yogo_loss_workspace_bytes", B, Sy, Sx) // 4
    Pb = ((P + 15) // 16) * 2
    pred = torch.empty_like(raw)
    h.call("yogo_decode_fwd", raw, pred, cxs, cys, B, P, Sy, Sx, *L.ANCHORS, 0, st)
    gpred, out3, ws3 = torch.full_like(raw, float("nan")), torch.empty(4, device="cuda"), torch.zeros(nws, device="cuda")
    h.call("yogo_loss_fwd_bwd", pred, lab, gpred, out3, ws3, B, P, Sy, Sx, *rb.w, st)
    g3 = torch.full((B, Pb, Sy, Sx, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    h.call("yogo_decode_bwd_bf16", raw, pred, gpred, g3, B, P, Sy, Sx, 0, st)
    g1 = torch.full((B, Pb, Sy, Sx, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    out1, ws1 = torch.full((4 + TAIL,), SENTINEL, device="cuda"), torch.zeros(nws, device="cuda")
    h.call("yogo_decode_loss_bwd_bf16", raw, lab, cxs, cys, g1, out1, ws1, B, P, Sy, Sx, *L.ANCHORS, *rb.w, st)
    torch.cuda.synchronize()
    assert torch.equal(g1.view(torch.int16), g3.view(torch.int16))
    assert torch.equal(out1[:4], out3) and bool((out1[4:] == SENTINEL).all())
    # the fp32 gradient of the three calls against the chain, then the bf16 units
    g32k = torch.full_like(raw, float("nan"))
    h.call("yogo_decode_bwd", raw, pred, gpred, g32k, B, P, Sy, Sx, 0, st)
    torch.cuda.synchronize()
    d = L.cells_first(g32k.cpu().numpy())
    rd = L.ratios(d, r32["grad"], r64["grad"])
    show("chain gradient fp32", L.by_family(rb.fam, rd))
    full = g1.float().permute(0, 1, 4, 2, 3).reshape(B, Pb * 8, Sy, Sx).cpu()
    assert bool((full[:, P:].view(torch.int32) == 0).all())
    d16 = L.cells_first(full[:, :P].numpy()).astype(np.float64)
    assert np.isfinite(d16).all()
    s = L.scale(r32["grad"], r64["grad"])
    r16 = (np.abs(d16 - r64["grad"]) - 2.0 ** -8 * np.abs(r64["grad"])).max(axis=1) / s
    show("chain gradient bf16", L.by_family(rb.fam, np.maximum(r16, 0)))
    assert rd.max() <= M, (rb.fam[int(rd.argmax())], float(rd.max()))
    assert r16.max() <= M, (rb.fam[int(r16.argmax())], float(r16.max()))
    want, bound = sum_bound(r32, r64, rb.w, 1.0 / B)
    out = out1[:4].cpu().numpy()
    print("[chain sums] |d| / bound", np.abs(out - want) / bound)
    assert (np.abs(out - want) <= bound).all(), (out, want, bound)


def test_class_count_limit():
    """64 classes (P = 69) run; P = 70 is refused with the ABI's error and nothing is written"""
    h = H()
    st = h.stream_ptr()
    g = next(g for g in L.groups() if g.P == 69)
    pred, label, case = L.pack(g, grid=(2, 3), min_batch=8)
    grad, out = run_loss(pred, label, g.w)
    assert np.isfinite(grad).all() and np.isfinite(out).all()
    B, Sy, Sx = 2, 2, 3
    for P in (69, 70):
        raw = torch.zeros(B, P, Sy, Sx, device="cuda")
        lab = torch.zeros(B, 6, Sy, Sx, device="cuda")
        cxs, cys = (t.cuda() for t in L.O.make_grids(Sx, Sy))
        outs = [torch.full((B, P, Sy, Sx), SENTINEL, device="cuda"), torch.full((B, P, Sy, Sx), SENTINEL, device="cuda"),
                torch.full((B, 10, Sy, Sx, 8), SENTINEL, dtype=torch.bfloat16, device="cuda")]
        lo = [torch.full((4,), SENTINEL, device="cuda") for _ in range(2)]
        ws = torch.zeros(64, device="cuda")
        calls = [lambda: h.call("yogo_decode_fwd", raw, outs[0], cxs, cys, B, P, Sy, Sx, *L.ANCHORS, 0, st),
                 lambda: h.call("yogo_loss_fwd_bwd", raw, lab, outs[1], lo[0], ws, B, P, Sy, Sx, *L.DEFAULT_W, st),
                 lambda: h.call("yogo_decode_loss_bwd_bf16", raw, lab, cxs, cys, outs[2], lo[1], ws, B, P, Sy, Sx, *L.ANCHORS, *L.DEFAULT_W, st)]
        for fn in calls:
            if P == 69:
                fn()
            else:
                with pytest.raises(RuntimeError, match="bad shape"):
                    fn()
        torch.cuda.synchronize()
        for t in outs + lo:
            untouched = bool((t.float() == SENTINEL).all())
            assert untouched == (P == 70), (P, tuple(t.shape))
