"""Seconds per ``Metrics.update`` on the host path and on the device path (``Metrics(device_matching=True)``), one process, one GPU.

Synthetic but realistic batches: 128 images on the 97x129 grid, 7 classes, 96 labelled objects per image (oracle.synthetic_labels),
predictions made from those labels (95 % of them, boxes jittered, class logits 3 * randn) plus four spurious rows per image.

  python tools/bench_metrics.py                  host and device path, include_mAP off and on, compute() after the timed batches,
                                                 then the kernels alone from a rocprofv3 --kernel-trace --stats run of its own
  python tools/bench_metrics.py --kernels-only   the device path alone (what the rocprofv3 child runs)

The host path is the comparison (the same process, the path every earlier version runs); the device path must stay under the
111 ms the uncached loader needs to produce such a batch (profiles/loader_cache.log).  Results: profiles/metrics_device.log.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, C, SY, SX, K = 128, 7, 97, 129, 96
LOADER_MS = 111.0   # profiles/loader_cache.log: 128 images / 1 151 img/s, the slowest feed measured


def make_batch(seed: int):
    import yogo_oracle as O

    g = torch.Generator().manual_seed(seed)
    labels = O.synthetic_labels(B, SX, SY, K=K, num_classes=C, seed=seed)
    preds = torch.zeros(B, 5 + C, SY, SX)
    preds[:, 4] = 0.1
    mask = labels[:, 0] != 0
    keep = mask & (torch.rand(B, SY, SX, generator=g) < 0.95)
    x1, y1, x2, y2 = (labels[:, k] + 0.004 * torch.randn(B, SY, SX, generator=g) for k in (1, 2, 3, 4))
    box = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1).abs(), (y2 - y1).abs()), 1)
    preds[:, :4] = torch.where(keep[:, None], box, preds[:, :4])
    preds[:, 4] = torch.where(keep, 0.6 + 0.4 * torch.rand(B, SY, SX, generator=g), preds[:, 4])
    preds[:, 5:] = 3 * torch.randn(B, C, SY, SX, generator=g)
    for b in range(B):                       # spurious rows on unlabelled cells
        free = torch.nonzero(~mask[b].flatten()).flatten()
        for cell in free[torch.randperm(len(free), generator=g)[:4]].tolist():
            y, x = divmod(cell, SX)
            preds[b, :5, y, x] = torch.tensor([(x + 0.5) / SX, (y + 0.5) / SY, 0.05, 0.05, 0.9])
    return preds.cuda(), labels.cuda()


def new_metrics(device_matching: bool, include_mAP: bool):
    from yogo_amd.metrics import Metrics

    return Metrics([str(i) for i in range(C)], include_mAP=include_mAP, include_background=False, device_matching=device_matching)


def time_path(batches, device_matching: bool, include_mAP: bool, warmup: int, reps: int):
    m = new_metrics(device_matching, include_mAP)
    for i in range(warmup):
        m.update(*batches[i % len(batches)])
    torch.cuda.synchronize()
    m.reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(reps):
        m.update(*batches[i % len(batches)])
    t_issue = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    t_host = time.perf_counter() - t0
    t_ev = e0.elapsed_time(e1) / 1e3
    t0 = time.perf_counter()
    res = m.compute()
    t_compute = time.perf_counter() - t0
    return {"host_clock": t_host / reps, "events": t_ev / reps, "issue": t_issue / reps, "compute": t_compute, "pairs": int(res[9]),
            "map": float(res[0]["map"]), "confmat": res[1]}


def kernel_stats(reps: int):
    """the match and accumulate kernels alone: a rocprofv3 --kernel-trace --stats run of this file with --kernels-only"""
    out = tempfile.mkdtemp(prefix="metrics_prof_")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
           sys.executable, os.path.abspath(__file__), "--kernels-only", "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return f"rocprofv3 run failed (exit {r.returncode}): {r.stderr[-400:]}", r.returncode
    lines = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if any(k in name for k in ("match_kernel", "metrics_accumulate", "metrics_finalize", "nms_batched", "match_gather")):
                lines.append(f"  {name.split('(')[0]:44s} calls {row.get('Calls', '?'):>4s}  average {float(row.get('AverageNs', 'nan')) / 1e3:10.1f} us  "
                             f"min {float(row.get('MinNs', 'nan')) / 1e3:10.1f} us  max {float(row.get('MaxNs', 'nan')) / 1e3:10.1f} us")
    return "\n".join(lines) if lines else f"no kernel_stats.csv under {out}", 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 10 and args.warmup >= 2
    batches = [make_batch(300 + i) for i in range(2)]
    if args.kernels_only:
        r = time_path(batches, True, True, args.warmup, args.reps)
        print("device path", r["host_clock"])
        return 0
    print(f"tools/bench_metrics.py on one MI355X: {B} images, grid {SY}x{SX}, {C} classes, {K} labelled objects per image, "
          f"{args.reps} batches after {args.warmup} warm-up batches; torch threads {torch.get_num_threads()}")
    res = {}
    for include_mAP in (False, True):
        for dm in (False, True):
            res[(dm, include_mAP)] = time_path(batches, dm, include_mAP, args.warmup, args.reps)
    print(f"matched pairs over the warm-up and timed batches: {res[(False, True)]['pairs']}")
    print("seconds per Metrics.update (host clock around the loop and a final synchronise | HIP events | host time to issue)")
    ok = True
    for include_mAP in (False, True):
        h, d = res[(False, include_mAP)], res[(True, include_mAP)]
        assert torch.equal(h["confmat"], d["confmat"]) and h["pairs"] == d["pairs"] and h["map"] == d["map"], "the two paths disagree"
        print(f"  include_mAP={include_mAP!s:5s} host path   {h['host_clock']:9.4f} | {h['events']:9.4f} | {h['issue']:9.4f}")
        print(f"  include_mAP={include_mAP!s:5s} device path {d['host_clock']:9.4f} | {d['events']:9.4f} | {d['issue']:9.4f}   "
              f"host / device = {h['host_clock'] / d['host_clock']:.0f}x; {d['host_clock'] * 1e3:.2f} ms against the {LOADER_MS:.0f} ms of the slowest feed")
        ok = ok and d["host_clock"] * 1e3 < LOADER_MS
    print(f"compute() after {args.reps} batches: " + "  ".join(
        f"{'device' if dm else 'host'} path mAP={mp!s}: {res[(dm, mp)]['compute']:.3f} s" for mp in (False, True) for dm in (False, True)))
    text, rc = kernel_stats(args.reps)
    print(f"kernels alone (rocprofv3 --kernel-trace --stats, a run of its own: {args.warmup + args.reps} device-path updates)")
    print(text)
    print("gate (device-path update under the slowest feed's batch time):", "met" if ok else "MISSED")
    return 0 if ok and rc == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
