"""thumbnail ("blob") augmentation on the device: HIP-event time of BlobDataset.generate for B images at H x W, n thumbnails per
image, about 1 000 thumbnails of 23-80 px -- written into the rows of a batch tensor, as the train loader does.  Also the
placement launch alone.   usage: bench_blobgen.py [B] [n] [H] [W]"""
import os, sys, tempfile
import numpy as np
import torch
from PIL import Image
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yogo_amd.blobgen import BlobDataset

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
H = int(sys.argv[3]) if len(sys.argv) > 3 else 772
W = int(sys.argv[4]) if len(sys.argv) > 4 else 1032
rng = np.random.default_rng(0)
with tempfile.TemporaryDirectory() as tmp:
    dirs = {}
    for c in ("healthy", "ring", "trophozoite", "schizont"):
        d = os.path.join(tmp, c)
        os.makedirs(d)
        for k in range(250):
            h, w = (int(v) for v in rng.integers(23, 81, size=2))
            Image.fromarray(np.clip(rng.normal(200, 40, size=(h, w)), 0, 255).astype(np.uint8), mode="L").save(os.path.join(d, f"{k}.png"))
        dirs[c] = [d]
    bd = BlobDataset(dirs, 129, 97, ["healthy", "ring", "trophozoite", "schizont"], n=N, length=1 << 20, background_img_shape=(H, W))
out = torch.empty(B, 1, H, W, dtype=torch.uint8, device="cuda")
pos = list(range(B))


def timed(fn, iters=20):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(iters):
        fn(it + 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


gen = timed(lambda e: bd.generate(range(B), e, out_imgs=out, positions=pos))
place = timed(lambda e: bd.place(range(B), e))
_, _, _, counts = bd.generate(range(B), 0, out_imgs=out, positions=pos)
print(f"blobgen: {bd.num_thumbnails} thumbnails, B={B} n={N} {H}x{W}: generate {gen * 1e3:.0f} us per launch sequence, "
      f"{gen * 1e3 / B:.2f} us per image ({B / gen * 1e3:.0f} img/s); placement alone {place * 1e3:.0f} us; "
      f"mean placed {counts.float().mean().item():.1f}; {B * H * W / gen / 1e6:.0f} GB/s of image bytes")
