"""In-process timing of a bf16 training step through autograd against HipTrainer (bench.py's workload: base_model, 772x1032 gray,
B = 128), HIP events around blocks of steps, the configurations interleaved round by round:
    hip_trainer_half   HipTrainer(half=True).step
    module_bf16        zero_grad(set_to_none=True), model(x) + YOGOLoss under bf16 autocast, loss.backward(),
                       torch.optim.AdamW(foreach=True).step(), CosineAnnealingLR.step()
    module_fp32        the same loop without autocast (the fp32 kernels)
    module_bf16_top    module_bf16 with layers < 5 frozen (AdamW over the trainable parameters)
    python tools/ab_autograd_bf16.py [--rounds R] [--steps K] [--warmup W] [--only NAME[,NAME]]"""
import argparse
import contextlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import yogo_oracle as O  # noqa: E402
from yogo_amd.engine import get_engine  # noqa: E402
from yogo_amd.model import YOGO  # noqa: E402
from yogo_amd.train import HipTrainer  # noqa: E402
from yogo_amd.yogo_loss import YOGOLoss  # noqa: E402

B, HI, WI, C, LR, T_MAX = 128, 772, 1032, 7, 3e-4, 100000
NAMES = ("hip_trainer_half", "module_bf16", "module_fp32", "module_bf16_top")


def make_step(name, sd, x, lab):
    m = YOGO((HI, WI), 0.0425, 0.0555, C).cuda()
    m.load_state_dict(sd)
    m.train()
    loss_fn = YOGOLoss().cuda()
    if name == "hip_trainer_half":
        tr = HipTrainer(m, loss_fn, learning_rate=LR, total_steps=T_MAX, half=True)
        return lambda: tr.step(x, lab)
    if name == "module_bf16_top":
        for L in get_engine(m.model).layers[:5]:
            for mod in (L.conv, L.bn):
                if mod is not None:
                    for p in mod.parameters():
                        p.requires_grad_(False)
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=LR, weight_decay=5e-2, foreach=True)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_MAX, eta_min=LR / 10.0)
    dtype = None if name == "module_fp32" else torch.bfloat16

    def step():
        opt.zero_grad(set_to_none=True)
        with (torch.autocast("cuda", dtype=dtype) if dtype is not None else contextlib.nullcontext()):
            loss, _ = loss_fn(m(x), lab)
        loss.backward()
        opt.step()
        sched.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=",".join(NAMES))
    a = ap.parse_args()
    names = [n for n in a.only.split(",") if n]
    for n in names:
        if n not in NAMES:
            raise SystemExit(f"unknown configuration {n}; one of {', '.join(NAMES)}")
    torch.manual_seed(0)
    m0 = YOGO((HI, WI), 0.0425, 0.0555, C).cuda()
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    x = torch.randint(0, 256, (B, 1, HI, WI), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    lab = O.synthetic_labels(B, m0.Sx, m0.Sy, K=30, num_classes=C, seed=2).cuda()
    del m0
    steps = {n: make_step(n, sd, x, lab) for n in names}
    for n in names:
        for _ in range(a.warmup):
            steps[n]()
    torch.cuda.synchronize()
    res = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                steps[n]()
            e1.record()
            e1.synchronize()
            res[n].append(e0.elapsed_time(e1) / a.steps)
    print(f"{torch.cuda.get_device_name()}  base_model {HI}x{WI} gray, B = {B}; {a.rounds} rounds x {a.steps} steps after {a.warmup} "
          f"warm-up steps, HIP events, configurations interleaved per round")
    med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
    for n in names:
        rel = f"  {med[n] / med['hip_trainer_half']:.3f} x hip_trainer_half" if "hip_trainer_half" in med else ""
        print(f"{n:18s} " + " ".join(f"{v:7.3f}" for v in res[n]) + f"   median {med[n]:7.3f} ms/step{rel}")


if __name__ == "__main__":
    main()
