"""Host-side checks of the device matching / device metrics feature (no GPU): the restated assignment solver against scipy, the
array form of the mAP bookkeeping against the per-row form, and the new public surface (symbols, flags, the no-fallback error)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import yogo_oracle as O
from _lsap_ref import lsap, lsap_par


def _boxes(rng, k):
    c = rng.random((k, 2)).astype(np.float32)
    s = (rng.random((k, 2)) * 0.15 + 0.02).astype(np.float32)
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def _box_cost(L, P):
    return (1 - O.box_iou(torch.from_numpy(L), torch.from_numpy(P))).numpy()


def _same_as_scipy(cost):
    r0, c0 = linear_sum_assignment(cost)
    for solver in (lsap, lsap_par):
        r1, c1 = solver(cost)
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (solver.__name__, cost.shape)


@pytest.mark.parametrize("kind", ["boxes", "small_integers", "uniform"])
def test_restated_solver_equals_scipy_on_random_cases(kind):
    rng = np.random.default_rng({"boxes": 0, "small_integers": 1, "uniform": 2}[kind])
    sizes = [(n, m) for n in (0, 1, 2, 3, 5, 8, 13, 21, 34, 40) for m in (0, 1, 2, 4, 7, 12, 20, 33, 40)]
    sizes += [(int(rng.integers(0, 41)), int(rng.integers(0, 41))) for _ in range(160)]
    for N, M in sizes:
        if kind == "boxes":       # mostly zero IoU -> cost exactly 1: heavy ties; some predictions are jittered labels
            while True:           # every case with at least two entries holds more than one cost of exactly 1.0 (redrawn until it does)
                L, P = _boxes(rng, N), _boxes(rng, M)
                k = min(N, M)
                if N * M - k >= 2 and rng.random() < 0.7:      # (the jittered copies take k entries away from the ties)
                    P[:k] = L[rng.permutation(N)[:k]] + (rng.random((k, 4)).astype(np.float32) - 0.5) * 0.03
                cost = _box_cost(L, P) if N and M else np.zeros((N, M), np.float32)
                if N * M < 2 or int((cost == 1).sum()) > 1:
                    break
            assert cost.dtype == np.float32
            if N * M >= 2:        # (0 x M, N x 0 and 1 x 1 cannot hold two)
                assert int((cost == 1).sum()) > 1, "the tie rule is not exercised by this case"
        elif kind == "small_integers":
            cost = rng.integers(0, 3, (N, M)).astype(np.float32)
        else:
            cost = rng.random((N, M)).astype(np.float32)
        _same_as_scipy(cost)      # N x M and, through the (N, M) / (M, N) pairs of `sizes`, both orientations


def test_restated_solver_equals_scipy_on_production_grid_problems():
    n = 0
    for seed, (K, KL, thr) in enumerate([(30, 25, 0.0), (100, 96, 0.0), (100, 120, 0.9), (60, 200, 0.0), (200, 60, 0.0), (96, 96, 0.3)]):
        preds = O.synthetic_predictions(2, 129, 97, num_classes=7, K=K, seed=100 + seed)
        labels = O.synthetic_labels(2, 129, 97, K=KL, num_classes=7, seed=200 + seed)
        for b in range(2):
            rows = O.format_preds(preds[b], 0.5, 0.5, "xyxy", thr)
            lab = labels[b].reshape(6, -1).T
            fl = lab[lab[:, 0].bool()]
            jit = fl[:, 1:5] + 0.003 * torch.randn(fl.shape[0], 4, generator=torch.Generator().manual_seed(seed))
            for P in (rows[:, :4], torch.cat([jit[: len(jit) * 3 // 4], rows[:40, :4]])):
                if fl.shape[0] == 0 or P.shape[0] == 0:
                    continue
                cost = (1 - O.box_iou(fl[:, 1:5], P)).numpy()
                assert cost.dtype == np.float32 and not np.isnan(cost).any()
                assert int((cost == 1).sum()) > 1
                _same_as_scipy(cost)
                n += 1
    assert n >= 20


# ---- mAP bookkeeping: arrays in place of one dict per matched row --------------------------------------------------------------------
def _pairs(K, seed, C=5):
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(K, 6)
    c = torch.rand(K, 2, generator=g)
    wh = 0.03 + 0.1 * torch.rand(K, 2, generator=g)
    lab[:, 0] = 1
    lab[:, 1:3], lab[:, 3:5] = c - wh / 2, c + wh / 2
    lab[:, 5] = torch.randint(0, C, (K,), generator=g).float()
    pred = torch.zeros(K, 5 + C)
    pred[:, :4] = lab[:, 1:5] + 0.02 * torch.randn(K, 4, generator=g)
    pred[:, 4] = (torch.rand(K, generator=g) * 8).round() / 8          # repeated scores: the stable sort's order matters
    pred[:, 5:] = torch.randn(K, C, generator=g)
    pred[torch.arange(K) % 3 == 0, 5:] = torch.nn.functional.one_hot(lab[:, 5].long(), C).float()[torch.arange(K) % 3 == 0] * 4
    return pred, lab


def _same_mAP(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, a[k], b[k])


def _feed_pairs(m, pred, lab):
    m.update_pairs(pred[:, :4], pred[:, 4], pred[:, 5:].argmax(1), lab[:, 1:5], lab[:, 5].long())


def test_update_pairs_equals_update_on_one_box_dicts():
    import yogo_amd.metrics as M

    pred, lab = _pairs(300, seed=1)
    met = M.Metrics([str(i) for i in range(5)], include_mAP=True, include_background=False)
    fp, fl = met._format_for_mAP(pred, lab)
    a, b, c = M.MeanAveragePrecision(), M.MeanAveragePrecision(), M.MeanAveragePrecision()
    a.update(fp, fl)
    _feed_pairs(b, pred, lab)
    ra = a.compute()
    assert float(ra["map"]) > 0
    _same_mAP(ra, b.compute())
    _same_mAP(a.compute(_general=True), b.compute(_general=True))
    _same_mAP(ra, b.compute(_general=True))
    # one object fed half by each method, in the same order
    c.update(fp[:150], fl[:150])
    _feed_pairs(c, pred[150:], lab[150:])
    _same_mAP(ra, c.compute())
    _same_mAP(ra, c.compute(_general=True))
    # ... and a general image (two detections) beside pair blocks takes the general path
    d, e = M.MeanAveragePrecision(), M.MeanAveragePrecision()
    extra_p = {"boxes": pred[:2, :4], "scores": pred[:2, 4], "labels": torch.tensor([1, 2])}
    extra_t = {"boxes": lab[:1, 1:5], "labels": torch.tensor([1])}
    d.update(fp + [extra_p], fl + [extra_t])
    _feed_pairs(e, pred, lab)
    e.update([extra_p], [extra_t])
    _same_mAP(d.compute(), e.compute())
    b.reset()
    assert float(b.compute()["map"]) == -1.0


# ---- the new surface ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_resolve_and_answer_without_a_gpu():
    from yogo_amd import _hip

    protos = _hip.prototypes()
    for name in ("yogo_match_workspace_bytes", "yogo_match_preds_labels_batched", "yogo_match_gather", "yogo_metrics_accumulate",
                 "yogo_metrics_state_layout"):
        assert name in protos, name
    assert _hip.lib().yogo_hip_abi_version() == 7
    small = _hip.query_size("yogo_match_workspace_bytes", 1, 24, 33, 24 * 33)
    big = _hip.query_size("yogo_match_workspace_bytes", 128, 97, 129, 97 * 129)
    # u, v, shortest-path costs in fp64 and four int32 arrays per side of the problem, for problems as large as the grid
    assert small >= 24 * 33 * (3 * 8 + 4 * 4) and big >= 128 * small * (97 * 129) // (24 * 33) * 0.99
    with pytest.raises(RuntimeError):
        _hip.query_size("yogo_match_workspace_bytes", 0, 24, 33, 24 * 33)
    layout = (ctypes.c_longlong * 12)()
    _hip.call("yogo_metrics_state_layout", 7, 500, 30, ctypes.addressof(layout))
    sizes = [7 * 7, 7, 1, 7, 7, 1, 30, 30, 501 * 7 * 2, 1, 2]      # confmat, pos, n, missed, extra, total, bins x 2, hist, mAP rows, statuses
    assert list(layout) == [sum(sizes[:k]) for k in range(12)]


def test_device_metrics_flag_parses_and_defaults_to_false():
    from yogo_amd.trainer import build_config
    from yogo_amd.utils.argparsers import global_parser

    p = global_parser()
    train = ["train", "tests/fake-data/defns/train_val_test.yml"]
    test = ["test", "m.pth", "defn.yml"]
    assert p.parse_args(train).device_metrics is False and p.parse_args(test).device_metrics is False
    assert p.parse_args(train + ["--device-metrics"]).device_metrics is True
    assert p.parse_args(test + ["--device-metrics"]).device_metrics is True
    assert p.parse_args(test + ["--no-device-metrics"]).device_metrics is False
    assert build_config(p.parse_args(train))["device_metrics"] is False
    assert build_config(p.parse_args(train + ["--device-metrics"]))["device_metrics"] is True


def test_device_matching_has_no_host_fallback():
    import inspect

    import yogo_amd.metrics as M
    from yogo_amd.trainer import Trainer
    from yogo_amd.utils import format_preds_and_labels_v2_device

    assert inspect.signature(Trainer.test).parameters["device_metrics"].default is False
    assert inspect.signature(M.Metrics.__init__).parameters["device_matching"].default is False
    preds = O.synthetic_predictions(2, 33, 24, num_classes=4, K=12, seed=4)
    labels = O.synthetic_labels(2, 33, 24, K=12, num_classes=4, seed=5)
    m = M.Metrics(["a", "b", "c", "d"], include_mAP=True, include_background=False, device_matching=True)
    with pytest.raises(RuntimeError, match="must live on an MI355X device"):
        m.update(preds, labels)
    with pytest.raises(RuntimeError, match="must live on an MI355X device"):
        format_preds_and_labels_v2_device(preds, labels)
    assert int(m._stats.n) == 0 and m._dev is None


def test_device_metrics_scope_turns_the_flag_on_for_trainer_test(monkeypatch):
    """`yogo test --device-metrics`: the entry point opens the scope, and `Trainer.test` inside it builds device-matching Metrics"""
    import yogo_amd.trainer as T

    seen = []

    class Stop(Exception):
        pass

    def fake_metrics(*a, device_matching=False, **k):
        seen.append(device_matching)
        raise Stop

    monkeypatch.setattr(T, "Metrics", fake_metrics)
    monkeypatch.setattr(T.Trainer, "_dataset_size", staticmethod(lambda dl: 1))
    cfg = {"class_names": ["a"], "no_obj_weight": 0.5, "iou_weight": 1, "label_smoothing": 0.0, "half": False}
    net = torch.nn.Identity()
    for scope, flag in ((False, False), (True, False), (False, True)):
        with T.device_metrics_scope(scope), pytest.raises(Stop):
            T.Trainer.test([], "cpu", cfg, net, device_metrics=flag)
    assert seen == [False, True, True] and T._device_metrics_scope is False


def test_console_test_task_opens_the_scope(monkeypatch):
    import yogo_amd.__main__ as main_mod
    import yogo_amd.trainer as T
    import yogo_amd.utils.test_model as tm

    seen = []
    monkeypatch.setattr(tm, "do_model_test", lambda args: seen.append(T._device_metrics_scope))
    monkeypatch.setattr(torch.multiprocessing, "set_start_method", lambda *a, **k: None)
    main_mod.main(["test", "m.pth", "defn.yml", "--device-metrics"])
    main_mod.main(["test", "m.pth", "defn.yml"])
    assert seen == [True, False] and T._device_metrics_scope is False
