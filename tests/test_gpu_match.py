"""Prediction <-> label matching and the class statistics on the device (yogo_amd/csrc/match.hip) against the host path and the
oracle: reference-written fixtures, batches on the production grid in both orientations, empty images, the dense case (wide
workgroup, LDS and workspace state), scipy's ValueError as a status, ``Metrics(device_matching=True)`` against ``Metrics()``,
run-to-run bit identity, the launch log, ``Trainer.test`` and the command line.  No image is handed back to the host solver."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import yogo_oracle as O
from _util import load_npz

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HW = (64, 96)
CLASSES = ["you", "only", "glance", "once"]


def _oracle_concat(preds, labels, thr):
    parts = [O.format_preds_and_labels_v2(p.clone(), l.clone(), 0.5, thr) for p, l in zip(preds.cpu(), labels.cpu())]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(4))


def _assert_match_equals_oracle(preds, labels, thr, what):
    from yogo_amd.utils import format_preds_and_labels_v2_device

    got = format_preds_and_labels_v2_device(preds.cuda(), labels, 0.5, thr)
    want = _oracle_concat(preds, labels, thr)
    for name, g, w in zip(("preds", "labels", "missed", "extra"), (got.preds, got.labels, got.missed_labels, got.extra_predictions), want):
        assert g.is_cuda and g.shape == w.shape, (what, name, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.cpu(), w), (what, name)
    return got


@pytest.mark.parametrize("name", ["sparse_0", "dense_0", "sparse_9", "dense_9"])
def test_reference_fixtures(name):
    from yogo_amd.utils import format_preds_and_labels_v2_device

    z = load_npz(f"match_{name}.npz")
    thr = float(name.split("_")[1]) / 10
    got = format_preds_and_labels_v2_device(torch.from_numpy(z["pred"])[None].cuda(), torch.from_numpy(z["label"])[None], 0.5, thr)
    for key, g in (("preds", got.preds), ("labels", got.labels), ("missed", got.missed_labels), ("extra", got.extra_predictions)):
        assert torch.equal(g.cpu(), torch.from_numpy(z[key])), (name, key)


def _dense_predictions(B, Sy, Sx, C, seed):
    """random-init-like: nearly every cell passes the objectness threshold, small boxes that rarely suppress each other"""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(B, 5 + C, Sy, Sx)
    p[:, 0] = (torch.arange(Sx).float()[None, None, :] + 0.5) / Sx + 0.3 / Sx * torch.randn(B, Sy, Sx, generator=g)
    p[:, 1] = (torch.arange(Sy).float()[None, :, None] + 0.5) / Sy + 0.3 / Sy * torch.randn(B, Sy, Sx, generator=g)
    p[:, 2] = 0.01 + 0.02 * torch.rand(B, Sy, Sx, generator=g)
    p[:, 3] = 0.01 + 0.02 * torch.rand(B, Sy, Sx, generator=g)
    p[:, 4] = 0.45 + 0.55 * torch.rand(B, Sy, Sx, generator=g)
    p[:, 5:] = torch.softmax(torch.randn(B, C, Sy, Sx, generator=g), dim=1)
    return p


@pytest.mark.parametrize("B,Sy,Sx,KL,KP,thr", [(3, 24, 33, 25, 30, 0.0), (8, 97, 129, 96, 100, 0.0), (8, 97, 129, 200, 60, 0.0),
                                               (4, 97, 129, 60, 200, 0.9)])
def test_batches_equal_oracle(B, Sy, Sx, KL, KP, thr):
    preds = O.synthetic_predictions(B, Sx, Sy, num_classes=7, K=KP, seed=11)
    labels = O.synthetic_labels(B, Sx, Sy, K=KL, num_classes=7, seed=12)
    got = _assert_match_equals_oracle(preds, labels, thr, (B, Sy, Sx, KL, KP, thr))
    assert got.preds.shape[0] > 0
    if KL > KP:
        assert got.missed_labels.shape[0] > 0      # more labels than rows: the transposed problem


def test_images_without_labels_or_rows_inside_a_batch():
    B, Sy, Sx = 4, 24, 33
    preds = O.synthetic_predictions(B, Sx, Sy, num_classes=7, K=30, seed=21)
    labels = O.synthetic_labels(B, Sx, Sy, K=25, num_classes=7, seed=22)
    labels[1, 0] = 0          # no label
    preds[2, 4] = 0.1         # no kept row
    labels[3, 0] = 0          # neither
    preds[3, 4] = 0.1
    got = _assert_match_equals_oracle(preds, labels, 0.0, "empty images")
    assert got.preds.shape[0] > 0 and got.missed_labels.shape[0] > 0 and got.extra_predictions.shape[0] > 0


@pytest.mark.parametrize("Sy,Sx", [(48, 65), (60, 80)])
def test_dense_case(Sy, Sx):
    """well over a thousand kept rows against 100 labels: the whole workgroup scans; at 48x65 the solver state fits the LDS, at 60x80
    (more than 4000 columns) it lives in the workspace"""
    from yogo_amd.utils.prediction_formatting import format_preds_batched

    preds = _dense_predictions(2, Sy, Sx, 7, seed=31)
    labels = O.synthetic_labels(2, Sx, Sy, K=100, num_classes=7, seed=32)
    _, _, counts = format_preds_batched(preds.cuda(), 0.5, 0.5, "xyxy")
    kept = counts.cpu().tolist()
    print("kept rows", kept)
    assert min(kept) > (2500 if Sy == 48 else 4000)
    got = _assert_match_equals_oracle(preds, labels, 0.0, ("dense", Sy, Sx))
    assert got.extra_predictions.shape[0] > 2000


def test_raw_predictions_input_equals_decoded_tensor():
    from yogo_amd.utils import format_preds_and_labels_v2_device
    from yogo_amd.utils.prediction_formatting import RawPredictions

    g = torch.Generator().manual_seed(41)
    B, Sy, Sx = 3, 24, 33
    raw = torch.randn(B, 12, Sy, Sx, generator=g)
    raw[:, 4] = torch.randn(B, Sy, Sx, generator=g) - 1.0
    labels = O.synthetic_labels(B, Sx, Sy, K=25, num_classes=7, seed=42)
    cxs, cys = (t.cuda() for t in O.make_grids(Sx, Sy))
    rp = RawPredictions(raw.cuda(), cxs, cys, 0.0425, 0.0555, 1.0, 1.0, True)
    a = format_preds_and_labels_v2_device(rp, labels)
    b = format_preds_and_labels_v2_device(rp.decoded(), labels)
    assert a.preds.shape[0] > 0
    for x, y in ((a.preds, b.preds), (a.labels, b.labels), (a.missed_labels, b.missed_labels), (a.extra_predictions, b.extra_predictions)):
        assert torch.equal(x, y)


def test_invalid_cost_is_a_status_and_raises_scipys_error():
    """a zero-area label over a zero-area kept row: IoU = 0 / 0, scipy refuses the matrix; the device reports status 1 for that image
    and leaves the other images' results alone"""
    from yogo_amd.utils import format_preds_and_labels_v2_batched, format_preds_and_labels_v2_device
    from yogo_amd.utils.prediction_formatting import format_preds_batched, match_rows_to_labels_device

    B, Sy, Sx = 3, 24, 33
    preds = O.synthetic_predictions(B, Sx, Sy, num_classes=7, K=30, seed=51)
    labels = O.synthetic_labels(B, Sx, Sy, K=25, num_classes=7, seed=52)
    labels[1, :, 3, 4] = torch.tensor([1.0, 0.5, 0.5, 0.5, 0.5, 2.0])
    preds[1, :5, 10, 10] = torch.tensor([0.25, 0.25, 0.0, 0.0, 0.99])
    with pytest.raises(ValueError, match="invalid numeric entries"):
        format_preds_and_labels_v2_batched(preds.cuda(), labels)
    with pytest.raises(ValueError, match="invalid numeric entries"):
        format_preds_and_labels_v2_device(preds.cuda(), labels)
    rows, _, counts = format_preds_batched(preds.cuda(), 0.5, 0.5, "xyxy")
    dm = match_rows_to_labels_device(rows, counts, labels.cuda())
    meta = dm.meta.cpu()
    assert meta[:, 5].tolist() == [0, 1, 0] and meta[1, 2:5].tolist() == [0, 0, 0]
    for b in (0, 2):
        wp, wl, wm, we = O.format_preds_and_labels_v2(preds[b].clone(), labels[b].clone(), 0.5, 0.0)
        n, nm, ne = meta[b, 2:5].tolist()
        assert (n, nm, ne) == (wp.shape[0], wm.shape[0], we.shape[0])
        assert torch.equal(dm.rows[b][dm.pair_pred[b, :n].long()].cpu(), wp) and torch.equal(dm.labels[b][dm.pair_label[b, :n].long()].cpu(), wl)
        assert torch.equal(dm.labels[b][dm.un_label[b, :nm].long()].cpu(), wm) and torch.equal(dm.rows[b][dm.un_pred[b, :ne].long()].cpu(), we)
    # Metrics on the device reads nothing back in update: the error surfaces in compute() at the latest
    import yogo_amd.metrics as M

    m = M.Metrics([str(i) for i in range(7)], include_mAP=False, include_background=False, min_class_confidence_threshold=0.0,
                  device_matching=True)
    m.update(preds.cuda(), labels.cuda())
    with pytest.raises(ValueError, match="invalid numeric entries"):
        m.compute()


# ---- Metrics(device_matching=True) against Metrics() ----------------------------------------------------------------------------------------
def _assert_same_compute(ra, rb, what):
    assert set(ra[0]) == set(rb[0])
    for k in ra[0]:
        assert torch.equal(ra[0][k], rb[0][k]), (what, "mAP", k, ra[0][k], rb[0][k])
    assert torch.equal(ra[1], rb[1]), (what, "confusion matrix")
    for i, name in ((2, "accuracy"), (4, "precision"), (5, "recall"), (7, "missed"), (8, "extra"), (9, "total")):
        assert torch.equal(ra[i], rb[i]), (what, name, ra[i], rb[i])
    for x, y, name in zip(ra[3], rb[3], ("fpr", "tpr", "thresholds")):
        assert torch.equal(x, y), (what, "ROC", name)
    print(what, "calibration error host", ra[6], "device", rb[6])
    assert abs(ra[6] - rb[6]) <= 1e-12 * abs(ra[6]), (what, "calibration error", ra[6], rb[6])


def _metric_batches(kind):
    out = []
    for i in range(3):
        B, Sy, Sx = (4, 48, 65) if i < 2 else (2, 97, 129)
        preds = O.synthetic_predictions(B, Sx, Sy, num_classes=7, K=70, seed=60 + i)
        labels = O.synthetic_labels(B, Sx, Sy, K=60, num_classes=7, seed=70 + i)
        g = torch.Generator().manual_seed(5 + i % 2)
        if kind == "logits":                 # the softmax branch
            preds[:, 5:] = 3 * torch.randn(B, 7, Sy, Sx, generator=g)
        else:                                # already probabilities; ties at the ROC thresholds / calibration edges on purpose
            flat = preds.view(B, 12, -1)
            cls = torch.randint(0, 7, (B, Sy * Sx), generator=g)
            onehot = torch.nn.functional.one_hot(cls, 7).float().permute(0, 2, 1)
            half = torch.zeros(B, 7, Sy * Sx)
            half[:, 0], half[:, 3] = 0.5, 0.5
            sel = torch.arange(Sy * Sx)
            flat[:, 5:, sel % 3 == 0] = onehot[:, :, sel % 3 == 0]
            flat[:, 5:, sel % 3 == 1] = half[:, :, sel % 3 == 1]
        out.append((preds, labels))
    return out


def _assert_precondition(preds, labels, thr, stats):
    """no probability within 1e-12 of a ROC threshold (other than threshold 0) or of a calibration edge, on the HOST values -- the
    only place where a device exp that differs from the host's by an ulp can move a count"""
    import yogo_amd.metrics as M
    from yogo_amd.utils import PredictionLabelMatch, format_preds_and_labels_v2_batched

    plm = PredictionLabelMatch.concat(format_preds_and_labels_v2_batched(preds.cuda(), labels, min_class_confidence_threshold=thr))
    prob = M._as_probabilities(plm.preds[:, 5:].cpu().double())
    d_thr = (prob.reshape(-1, 1) - stats.thresholds[1:].reshape(1, -1)).abs().min()
    edges = torch.linspace(0, 1, stats.n_bins + 1, dtype=torch.float64)
    d_edge = (prob.max(1).values.reshape(-1, 1) - edges.reshape(1, -1)).abs().min()
    print("closest approach to a ROC threshold", float(d_thr), "to a calibration edge", float(d_edge))
    assert float(d_thr) > 1e-12 and float(d_edge) > 1e-12


@pytest.mark.parametrize("kind", ["probabilities", "logits"])
@pytest.mark.parametrize("thr", [0.0, 0.9])
def test_device_metrics_equal_host_metrics(kind, thr):
    import yogo_amd.metrics as M

    names = [str(i) for i in range(7)]
    host = M.Metrics(names, include_mAP=True, include_background=False, min_class_confidence_threshold=thr)
    dev = M.Metrics(names, include_mAP=True, include_background=False, min_class_confidence_threshold=thr, device_matching=True)
    for preds, labels in _metric_batches(kind):
        if kind == "logits":
            _assert_precondition(preds, labels, thr, host._stats)
        host.update(preds.cuda(), labels.cuda())
        dev.update(preds.cuda(), labels.cuda())
    ra, rb = host.compute(), dev.compute()
    assert int(ra[9]) > 100 and int(ra[1].sum()) == int(ra[9])
    _assert_same_compute(ra, rb, (kind, thr))
    _assert_same_compute(ra, dev.compute(), (kind, thr, "second compute"))
    # reset keeps what the host's reset keeps (the missed / extra / total counters) and clears the rest
    host.reset()
    dev.reset()
    preds, labels = _metric_batches(kind)[0]
    _assert_same_compute(host.forward(preds.cuda(), labels.cuda()), dev.forward(preds.cuda(), labels.cuda()), (kind, thr, "after reset"))


def test_device_metrics_with_background_class():
    import yogo_amd.metrics as M

    B, C, Sy, Sx = 6, 4, 24, 33
    preds = O.synthetic_predictions(B, Sx, Sy, num_classes=C, K=12, seed=4)
    labels = O.synthetic_labels(B, Sx, Sy, K=12, num_classes=C, seed=5)
    kw = dict(include_mAP=True, include_background=True, min_class_confidence_threshold=0.3)
    ra = M.Metrics(CLASSES, **kw).forward(preds.cuda(), labels.cuda())
    rb = M.Metrics(CLASSES, device_matching=True, **kw).forward(preds.cuda(), labels.cuda())
    assert int(ra[9]) == 71 and int(ra[8].sum()) == 1 and int(ra[7].sum()) == 0
    _assert_same_compute(ra, rb, "background")
    # missed labels beside the matched rows: the reference's conversion raises on the mixed row widths -- the same way on both paths
    z = load_npz("match_sparse_9.npz")
    p, l = torch.from_numpy(z["pred"])[None], torch.from_numpy(z["label"])[None]
    kw = dict(include_mAP=False, include_background=True, min_class_confidence_threshold=0.9)
    with pytest.raises(Exception) as host_err:
        M.Metrics([str(i) for i in range(7)], **kw).update(p.cuda(), l.cuda())
    with pytest.raises(Exception) as dev_err:
        M.Metrics([str(i) for i in range(7)], device_matching=True, **kw).update(p.cuda(), l.cuda())
    assert type(host_err.value) is type(dev_err.value), (host_err.value, dev_err.value)


def test_more_classes_than_seven():
    """12 classes: the accumulate kernel's LDS histograms go past 64 KB (the limit is 31 classes, and beyond it an error)"""
    import yogo_amd.metrics as M

    C, B, Sy, Sx = 12, 4, 48, 65
    names = [str(i) for i in range(C)]
    preds = O.synthetic_predictions(B, Sx, Sy, num_classes=C, K=70, seed=80)
    labels = O.synthetic_labels(B, Sx, Sy, K=60, num_classes=C, seed=81)
    kw = dict(include_mAP=True, include_background=False, min_class_confidence_threshold=0.0)
    ra = M.Metrics(names, **kw).forward(preds.cuda(), labels.cuda())
    rb = M.Metrics(names, device_matching=True, **kw).forward(preds.cuda(), labels.cuda())
    assert int(ra[9]) > 100 and int((ra[1].sum(1) > 0).sum()) >= 10
    _assert_same_compute(ra, rb, "12 classes")
    wide = O.synthetic_predictions(1, 33, 24, num_classes=40, K=12, seed=82)
    with pytest.raises(RuntimeError, match="classes"):
        M.Metrics([str(i) for i in range(40)], device_matching=True, **kw).update(wide.cuda(), O.synthetic_labels(1, 33, 24, K=12, num_classes=40, seed=83))


def test_map_row_buffer_grows_after_a_small_first_batch():
    """the buffer is sized by the first update; a larger batch afterwards makes it grow, keeping the rows written so far"""
    import yogo_amd.metrics as M

    names = [str(i) for i in range(7)]
    kw = dict(include_mAP=True, include_background=False, min_class_confidence_threshold=0.0)
    host, dev = M.Metrics(names, **kw), M.Metrics(names, device_matching=True, **kw)
    (p0, l0), (p1, l1), _ = _metric_batches("probabilities")
    first = None
    for preds, labels in ((p0[:1], l0[:1]), (p1, l1), (p0, l0)):
        host.update(preds.cuda(), labels.cuda())
        dev.update(preds.cuda(), labels.cuda())
        first = first or dev._dev.map_rows.shape[0]
    assert first == 2 * 48 * 65 and dev._dev.map_rows.shape[0] > first
    ra, rb = host.compute(), dev.compute()
    assert int(ra[9]) > 300
    _assert_same_compute(ra, rb, "grown mAP buffer")


def test_reset_clears_a_refused_batch():
    """after a batch with an invalid cost matrix compute() raises; reset() makes the object usable again"""
    import yogo_amd.metrics as M

    names = [str(i) for i in range(7)]
    kw = dict(include_mAP=True, include_background=False, min_class_confidence_threshold=0.0)
    preds, labels = _metric_batches("probabilities")[0]
    bad_p, bad_l = preds.clone(), labels.clone()
    bad_l[1, :, 3, 4] = torch.tensor([1.0, 0.5, 0.5, 0.5, 0.5, 2.0])
    bad_p[1, :5, 10, 10] = torch.tensor([0.25, 0.25, 0.0, 0.0, 0.99])
    host, dev = M.Metrics(names, **kw), M.Metrics(names, device_matching=True, **kw)
    dev.update(bad_p.cuda(), bad_l.cuda())
    for _ in range(2):
        with pytest.raises(ValueError, match="invalid numeric entries"):
            dev.compute()
    dev.reset()
    host.update(preds.cuda(), labels.cuda())
    dev.update(preds.cuda(), labels.cuda())
    ra, rb = host.compute(), dev.compute()
    for i in (1, 2, 4, 5):                       # (missed / extra / total are not reset, on either path)
        assert torch.equal(ra[i], rb[i])
    for k in ra[0]:
        assert torch.equal(ra[0][k], rb[0][k])


def test_two_runs_give_identical_accumulator_bits():
    import yogo_amd.metrics as M

    states = []
    for _ in range(2):
        dev = M.Metrics([str(i) for i in range(7)], include_mAP=True, include_background=False, min_class_confidence_threshold=0.0,
                        device_matching=True)
        for preds, labels in _metric_batches("logits"):
            dev.update(preds.cuda(), labels.cuda())
        torch.cuda.synchronize()
        d = dev._dev
        n = int(d.acc[d.off_map_count])
        states.append((d.acc.cpu(), d.bin_conf.cpu(), d.map_rows[:n].cpu()))
    assert int(states[0][0][: 49].sum()) > 100 and float(states[0][1].sum()) > 0
    assert torch.equal(states[0][0], states[1][0])
    assert torch.equal(states[0][1].view(torch.int64), states[1][1].view(torch.int64))        # the fp64 sums, bit for bit
    assert torch.equal(states[0][2].view(torch.int32), states[1][2].view(torch.int32))


def test_update_launches_the_kernels_and_never_calls_scipy(monkeypatch):
    import scipy.optimize

    import yogo_amd.metrics as M
    from yogo_amd import _hip

    def refuse(*a, **k):
        raise AssertionError("the device path called scipy.optimize.linear_sum_assignment")

    preds, labels = _metric_batches("probabilities")[0]
    dev = M.Metrics([str(i) for i in range(7)], include_mAP=True, include_background=False, min_class_confidence_threshold=0.0,
                    device_matching=True)
    monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", refuse)
    _hip.launch_log(True)
    try:
        dev.update(preds.cuda(), labels.cuda())
        torch.cuda.synchronize()
    finally:
        _hip.launch_log(False)
    launched = [ln.split("|")[0].split("<")[0].strip() for ln in _hip.read_launch_log()]
    assert launched == ["nms_batched_kernel", "match_kernel", "metrics_accumulate_kernel", "metrics_finalize_kernel"], launched
    res = dev.compute()
    assert int(res[9]) > 100
    # the seam of the host path stays the one `update` calls with the flag off
    host = M.Metrics([str(i) for i in range(7)], include_mAP=False, include_background=False, min_class_confidence_threshold=0.0)
    with pytest.raises(AssertionError, match="called scipy"):
        host.update(preds.cuda(), labels.cuda())


# ---- Trainer.test and the command line -------------------------------------------------------------------------------------------------------
def _make_checkpoint(tmp_path, seed=3):
    """'trained-like' weights so that some predictions pass the thresholds (as tests/test_gpu_cli.py builds them)"""
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO(HW, 0.0425, 0.0555, 4).cuda()
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
    return p, net


def test_trainer_test_returns_the_same_tuple(monkeypatch, tmp_path):
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.trainer import Trainer
    from yogo_amd.yogo_dataloader import get_dataloader

    monkeypatch.chdir(ROOT)
    _, net = _make_checkpoint(tmp_path)
    net.inference = False
    d = DatasetDefinition.from_yaml(Path("tests/fake-data/defns/literal_tests_123.yml"))
    Sx, Sy = net.get_grid_size()
    config = {"class_names": CLASSES, "no_obj_weight": 0.5, "iou_weight": 1, "label_smoothing": 0.0001, "half": True}
    res = []
    for flag in (False, True):
        loaders = get_dataloader(d, 2, Sx, Sy, training=False, image_hw=HW)
        res.append(Trainer.test(loaders["test"], "cuda", config, net, include_mAP=True, include_background=False, device_metrics=flag))
    a, b = res
    print("test split: matched", int(a[10]), "missed", a[8].tolist(), "extra", a[9].tolist())
    assert a[0] == b[0] and a[2] == b[2] and a[11] == b[11]
    host = (a[1], torch.tensor([[r[2] for r in a[2]]]), a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10])
    dev = (b[1], torch.tensor([[r[2] for r in b[2]]]), b[3], b[4], b[5], b[6], b[7], b[8], b[9], b[10])
    _assert_same_compute(host, dev, "Trainer.test")


def test_console_test_with_device_metrics(tmp_path):
    pth, _ = _make_checkpoint(tmp_path)
    defn = tmp_path / "defn.yml"
    data = ROOT / "tests" / "fake-data" / "data"
    defn.write_text(
        "class_names: [you, only, glance, once]\n"
        "dataset_split_fractions: {train: 0.75, val: 0.25}\n"
        f"dataset_paths:\n  a: {{image_path: {data}/images1, label_path: {data}/labels1}}\n  b: {{image_path: {data}/images2, label_path: {data}/labels2}}\n"
        f"test_paths:\n  c: {{image_path: {data}/images3, label_path: {data}/labels3}}\n")
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    # the console entry point with the library's launch log on around it: which kernels the command ran
    script = tmp_path / "run_cli.py"
    script.write_text(
        "import sys\n"
        "from yogo_amd import _hip\n"
        "from yogo_amd.__main__ import main\n"
        "if __name__ == '__main__':\n"
        "    _hip.launch_log(True)\n"
        "    main(sys.argv[1:])\n"
        "    _hip.launch_log(False)\n"
        "    print('LAUNCHED', ' '.join(sorted({ln.split('|')[0].split('<')[0].strip() for ln in _hip.read_launch_log()})))\n")
    outs, launched = [], []
    for extra in ([], ["--device-metrics"]):
        r = subprocess.run([sys.executable, str(script), "test", str(pth), str(defn), "--include-mAP", *extra], cwd=tmp_path, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if "test loss" in ln])
        launched.append([ln for ln in r.stdout.splitlines() if ln.startswith("LAUNCHED")][0].split()[1:])
    assert outs[0] and outs[0] == outs[1], outs
    assert "nms_batched_kernel" in launched[0] and "match_kernel" not in launched[0] and "metrics_accumulate_kernel" not in launched[0]
    assert "match_kernel" in launched[1] and "metrics_accumulate_kernel" in launched[1], launched[1]
    # ... and the module entry point itself
    r = subprocess.run([sys.executable, "-m", "yogo_amd", "test", str(pth), str(defn), "--device-metrics"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test loss" in r.stdout, r.stdout + r.stderr


def test_device_update_stays_under_the_slowest_feed():
    """the gate of the feature: one device-path update of the benchmark tool's 128-image batch (host clock, synchronised, mAP off and
    on) takes less than the 111 ms the slowest feed this project has measured needs to produce that batch (profiles/loader_cache.log)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_metrics", ROOT / "tools" / "bench_metrics.py")
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    batches = [bm.make_batch(300)]
    for include_mAP in (False, True):
        r = bm.time_path(batches, True, include_mAP, warmup=2, reps=10)
        print(f"include_mAP={include_mAP}: {r['host_clock'] * 1e3:.3f} ms per update (host clock), {r['events'] * 1e3:.3f} ms (events), "
              f"{r['pairs']} pairs")
        assert r["pairs"] > 10 * 128 * 50
        assert r["host_clock"] * 1e3 < bm.LOADER_MS
