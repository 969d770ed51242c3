"""In-process A/B of builds of yogo_amd/csrc/bn.hip: every extern "C" entry of the file on seeded inputs under each library, every buffer
the call writes compared for equal bits against the first tag's; then the entries whose kernels changed, at their large cases, alternating
between the libraries (device events around 10 launches, first round dropped): a tag's median must lie inside the first tag's min-max.
    python tools/ab_bn.py TAG1,TAG2,... [rounds]      (TAG "base" = the product library, TAG t = yogo_amd/lib/libyogo_hip_t.so)
A build of another commit: bash yogo_amd/csrc/build.sh in a worktree of it, its libyogo_hip.so copied to yogo_amd/lib/libyogo_hip_parent.so."""
import collections
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from yogo_amd import _hip as H
from ab_variants import load

LEAKY, SILU = 1, 2
EPS, MOM = 1e-5, 0.1
PER_ROW = 3                         # values behind one partial row of the yogo_bn_finalize cases: count = PER_ROW * rows
STEP = (128, 128, 97 * 129)          # layers 4 and 5 of base_model at 772 x 1032, batch 128


def cb_of(C):
    return ((C + 15) // 16) * 2


def rnd(*shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, device="cuda") * scale).to(dtype)


def poisoned(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def chan(C):
    """mean, invstd, var, gamma (both signs), beta"""
    gamma = 0.5 + torch.rand(C, device="cuda")
    gamma[::3] = -gamma[::3]
    var = torch.rand(C, device="cuda") + 0.5
    return rnd(C, scale=0.3), 1.0 / torch.sqrt(var + EPS), var, gamma, rnd(C, scale=0.3)


class Case:
    """name; alloc() -> the buffers a call writes (poisoned); launch(outs); timed: alternate it between the libraries"""

    def __init__(self, name, alloc, launch, timed=False):
        self.name, self.alloc, self.launch, self.timed = name, alloc, launch, timed


def cases():
    st = H.stream_ptr()
    out = []
    # ---- bf16 NCHW8c entries and the head entry
    for (B, C, HW), big in ((STEP, True), ((3, 20, 1025), False)):
        Cb = cb_of(C)
        tag = f"B={B} C={C} HW={HW}"
        z, g = rnd(B, Cb, HW, 8, dtype=torch.bfloat16), rnd(B, Cb, HW, 8, scale=0.3, dtype=torch.bfloat16)
        mean, invstd, var, gamma, beta = chan(C)
        rows = H.query_ints("yogo_bn_bwd_bf16_rows", 1, B, HW)[0]
        for act in (LEAKY, SILU):
            for siv in (0, 1):
                out.append(Case(f"yogo_bn_apply_act_bf16 {tag} act={act} stat_is_var={siv}", lambda z=z: dict(y=poisoned(*z.shape, dtype=torch.bfloat16)),
                                lambda o, a=(z, mean, invstd, var, gamma, beta, B, C, HW), act=act, siv=siv:
                                H.call("yogo_bn_apply_act_bf16", a[0], o["y"], a[1], a[3] if siv else a[2], siv, EPS, a[4], a[5], a[6], a[7], a[8], act, st),
                                timed=big and siv == 0))
            for training in (1, 0):
                alloc = lambda z=z, rows=rows, C=C: dict(dz=poisoned(*z.shape, dtype=torch.bfloat16), part=poisoned(rows * C * 2), sums=poisoned(2 * C),
                                                         dgamma=poisoned(C), dbeta=poisoned(C))
                out.append(Case(f"yogo_bn_bwd_bf16 {tag} act={act} training={training}", alloc,
                                lambda o, a=(g, z, mean, invstd, gamma, beta, B, C, HW), act=act, training=training:
                                H.call("yogo_bn_bwd_bf16", a[0], a[1], o["dz"], a[2], a[3], a[4], a[5], act, o["dgamma"], o["dbeta"], o["part"], o["sums"],
                                       a[6], a[7], a[8], training, 0.25, st), timed=big))
        out.append(Case(f"yogo_bn_stats_bf16 {tag}", lambda rows=rows, C=C: dict(part=poisoned(rows * C * 2)),
                        lambda o, a=(z, B, C, HW): H.call("yogo_bn_stats_bf16", a[0], o["part"], a[1], a[2], a[3], st), timed=big))
        # conversions (the fp32 side of the large case: 8 images of it)
        Bc = 8 if big else B
        x = rnd(Bc, C, HW)
        out.append(Case(f"yogo_nchw_f32_to_bf16_8c B={Bc} C={C} HW={HW}", lambda Bc=Bc, Cb=Cb, HW=HW: dict(out=poisoned(Bc, Cb, HW, 8, dtype=torch.bfloat16)),
                        lambda o, a=(x, Bc, C, HW): H.call("yogo_nchw_f32_to_bf16_8c", a[0], o["out"], a[1], a[2], a[3], st), timed=big))
        out.append(Case(f"yogo_bf16_8c_to_nchw_f32 B={Bc} C={C} HW={HW}", lambda Bc=Bc, C=C, HW=HW: dict(out=poisoned(Bc, C, HW)),
                        lambda o, a=(z, Bc, C, HW): H.call("yogo_bf16_8c_to_nchw_f32", a[0], o["out"], a[1], a[2], a[3], st), timed=big))
        # the head entry: C a multiple of 16, P = 12 outputs in two channel blocks of gh (channels >= P zero)
        Ch, P = (C, 12) if C % 16 == 0 else (32, 12)
        zh = z if Ch == C else rnd(B, cb_of(Ch), HW, 8, dtype=torch.bfloat16)
        mh = (mean, invstd, gamma, beta) if Ch == C else tuple(chan(Ch)[i] for i in (0, 1, 3, 4))
        gh = rnd(B, 2, HW, 8, scale=0.3, dtype=torch.bfloat16)
        gh[:, 1, :, P - 8:] = 0
        w = rnd(P, Ch, scale=0.2)
        for act in (LEAKY, SILU):
            for training in (1, 0):
                alloc = lambda zh=zh, rows=rows, Ch=Ch: dict(dz=poisoned(*zh.shape, dtype=torch.bfloat16), part=poisoned(rows * Ch * 2), sums=poisoned(2 * Ch),
                                                             dgamma=poisoned(Ch), dbeta=poisoned(Ch))
                out.append(Case(f"yogo_bn_bwd_bf16_head B={B} C={Ch} P={P} HW={HW} act={act} training={training}", alloc,
                                lambda o, a=(gh, w, P, zh) + mh + (B, Ch, HW), act=act, training=training:
                                H.call("yogo_bn_bwd_bf16_head", a[0], a[1], a[2], a[3], o["dz"], a[4], a[5], a[6], a[7], act, o["dgamma"], o["dbeta"],
                                       o["part"], o["sums"], a[8], a[9], a[10], training, 0.25, st), timed=big))
    # ---- fp32 entries
    for (B, C, HW), big in (((8, 128, 97 * 129), True), ((4, 16, 386 * 516), True), ((3, 5, 2049), False)):
        tag = f"B={B} C={C} HW={HW}"
        z, g = rnd(B, C, HW), rnd(B, C, HW, scale=0.3)
        mean, invstd, var, gamma, beta = chan(C)
        rows = H.query_ints("yogo_bn_bwd_rows", 1, B, HW)[0]
        for act in (LEAKY, SILU):
            for siv in (0, 1):
                out.append(Case(f"yogo_bn_apply_act {tag} act={act} stat_is_var={siv}", lambda z=z: dict(y=poisoned(*z.shape)),
                                lambda o, a=(z, mean, invstd, var, gamma, beta, B, C, HW), act=act, siv=siv:
                                H.call("yogo_bn_apply_act", a[0], o["y"], a[1], a[3] if siv else a[2], siv, EPS, a[4], a[5], a[6], a[7], a[8], act, st),
                                timed=big and siv == 0))
            for training in (1, 0):
                alloc = lambda z=z, rows=rows, C=C: dict(dz=poisoned(*z.shape), part=poisoned(rows * C * 2), sums=poisoned(2 * C), dgamma=poisoned(C),
                                                         dbeta=poisoned(C))
                out.append(Case(f"yogo_bn_bwd {tag} act={act} training={training}", alloc,
                                lambda o, a=(g, z, mean, invstd, gamma, beta, B, C, HW), act=act, training=training:
                                H.call("yogo_bn_bwd", a[0], a[1], o["dz"], a[2], a[3], a[4], a[5], act, o["dgamma"], o["dbeta"], o["part"], o["sums"],
                                       a[6], a[7], a[8], training, 0.25, st), timed=big))
        out.append(Case(f"yogo_bn_invstd C={C}", lambda C=C: dict(invstd=poisoned(C)),
                        lambda o, a=(var, C): H.call("yogo_bn_invstd", a[0], EPS, o["invstd"], a[1], st)))
    # ---- the reductions, at the rows / HW of tests/test_gpu_bn_edges.py and the step's
    step_rows = H.query_ints("yogo_bn_bwd_bf16_rows", 1, STEP[0], STEP[2])[0]
    for rows in (1, 31, 32, 33, 255, 256, 257, 289, 8192, step_rows):
        for C, stride in ((20, 32), (128, 128)):
            # every row as a producer's: the sum s of PER_ROW values and a sum of squares of at least s^2 / PER_ROW (no negative variance)
            part = torch.empty(rows, stride, 2, device="cuda")
            part[..., 0] = rnd(rows, stride, scale=5.0) + 2.0
            part[..., 1] = part[..., 0] ** 2 / PER_ROW + torch.rand(rows, stride, device="cuda") * 10.0
            rm0, rv0 = rnd(C), torch.rand(C, device="cuda") + 0.5

            def alloc(C=C, rm0=rm0, rv0=rv0):
                return dict(mean=poisoned(C), invstd=poisoned(C), running_mean=rm0.clone(), running_var=rv0.clone(),
                            nbt=torch.full((1,), 5, dtype=torch.int64, device="cuda"))
            out.append(Case(f"yogo_bn_finalize rows={rows} C={C} stride={stride}", alloc,
                            lambda o, a=(part, rows, stride, C): H.call("yogo_bn_finalize", a[0], a[1], a[2], a[3], PER_ROW * a[1], EPS, MOM, o["mean"], o["invstd"],
                                                                        o["running_mean"], o["running_var"], o["nbt"], st)))
    for rows in (1, 7, 8, 9, 64, 65, 128, 129, 513, 577, step_rows):
        for N in (255, 257):
            part = rnd(rows, N, scale=3.0)
            out.append(Case(f"yogo_partials_reduce rows={rows} N={N}", lambda part=part, N=N: dict(part=part.clone(), out=poisoned(N)),   # (folds part in place)
                            lambda o, a=(rows, N): H.call("yogo_partials_reduce", o["part"], a[0], a[1], 1.5, o["out"], st)))
    for B, C, HW, big in [(b, 5, hw, False) for b in (1, 3) for hw in (1, 255, 257, 2049)] + [(STEP[0], 12, STEP[2], True)]:
        g = rnd(B, C, HW)
        out.append(Case(f"yogo_channel_sum B={B} C={C} HW={HW}", lambda C=C: dict(out=poisoned(C)),
                        lambda o, a=(g, B, C, HW): H.call("yogo_channel_sum", a[0], a[1], a[2], a[3], 0.0, o["out"], st), timed=big))
    return out


def raw(t):
    return t.contiguous().view(-1).view(torch.uint8)


if __name__ == "__main__":
    tags = sys.argv[1].split(",")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    libs = {t: load(t) for t in tags}
    bad = 0
    for t in tags:   # the *_rows queries: the same answers
        H._lib = libs[t]
        q = [H.query_ints(n, 1, b, hw)[0] for n in ("yogo_bn_bwd_rows", "yogo_bn_bwd_bf16_rows") for b in (1, 3, 128) for hw in (1, 1024, 1025, 2048, 2049, 12513, 199176)]
        if t == tags[0]:
            q0 = q
        bad += q != q0
        print(f"rows  yogo_bn_bwd_rows / yogo_bn_bwd_bf16_rows under {t}: {'same' if q == q0 else 'DIFFER'}")
    H._lib = libs[tags[0]]
    torch.manual_seed(20)
    cs = cases()
    print(f"# {len(cs)} cases; device {torch.cuda.get_device_name(0)}; tags {tags}, bits against {tags[0]}")
    nbits = nsame = 0
    for c in cs:
        ref = None
        for t in tags:
            H._lib = libs[t]
            o = c.alloc()
            c.launch(o)
            torch.cuda.synchronize()
            if ref is None:
                ref = o
                continue
            diff = {n: int((raw(o[n]) != raw(ref[n])).sum()) for n in o}
            nbytes = sum(raw(v).numel() for v in o.values())
            ok = not any(diff.values())
            bad += 0 if ok else 1
            nbits += 1
            nsame += ok
            print(f"bits  {c.name:86s} {t:8s} {'same' if ok else 'DIFFER ' + str(diff)}  ({nbytes} bytes in {'/'.join(o)})")
        del ref, o
    print(f"# bits: {nsame} of {nbits} comparisons identical to {tags[0]}")
    # ---- speed
    res = collections.defaultdict(list)
    timed = [c for c in cs if c.timed]
    outs = {c.name: c.alloc() for c in timed}
    for r in range(rounds + 1):   # round 0 warms the clocks and is dropped
        for c in timed:
            for t in tags:
                H._lib = libs[t]
                o = outs[c.name]
                c.launch(o); c.launch(o)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    c.launch(o)
                e1.record()
                torch.cuda.synchronize()
                if r > 0:
                    res[(c.name, t)].append(e0.elapsed_time(e1) * 100.0)   # us per launch
    slow = 0
    print(f"# speed: us per call, {rounds} rounds of 10 calls (first round dropped); a tag's median must lie inside {tags[0]}'s min-max")
    for c in timed:
        p = res[(c.name, tags[0])]
        print(f"speed {c.name:86s} {tags[0]:8s} " + "/".join(f"{v:.1f}" for v in p))
        for t in tags[1:]:
            v = res[(c.name, t)]
            med = sorted(v)[len(v) // 2]
            verdict = "ok" if med <= max(p) else "SLOWER"
            where = "inside" if min(p) <= med <= max(p) else ("below" if med < min(p) else "ABOVE")
            slow += verdict != "ok"
            print(f"speed {'':86s} {t:8s} " + "/".join(f"{x:.1f}" for x in v) + f"   median {med:.1f} {where} [{min(p):.1f}, {max(p):.1f}] {verdict}")
    print(f"# speed: {len(timed) * (len(tags) - 1) - slow} of {len(timed) * (len(tags) - 1)} within {tags[0]}'s own spread")
    sys.exit(1 if bad or slow else 0)
