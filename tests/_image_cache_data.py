"""Small PNG datasets for the device image cache tests (yogo_amd/image_cache.py): random images and YOLO label files written
into a temporary directory, and a dataset definition over them."""
from pathlib import Path
from typing import Iterable, Optional, Tuple

import numpy as np
from PIL import Image

CLASSES = ["you", "only", "glance", "once"]


def write_images(root: Path, n: int, hw: Tuple[int, int] = (64, 96), rgb: bool = False, seed: int = 0,
                 truncated: Iterable[int] = ()) -> Tuple[Path, Path]:
    """n images img_0000.png ... (random pixels; the ones in `truncated` cut in half) and their label files (0 or 2-5 rows)"""
    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir(parents=True, exist_ok=True)
    lab_dir.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    cut = set(truncated)
    for k in range(n):
        arr = rng.integers(0, 256, size=(hw[0], hw[1], 3) if rgb else tuple(hw), dtype=np.uint8)
        p = img_dir / f"img_{k:04d}.png"
        Image.fromarray(arr).save(p)
        if k in cut:
            data = p.read_bytes()
            p.write_bytes(data[:len(data) // 2])
        m = int(rng.choice([0, 2, 3, 4, 5]))
        lines = [f"{int(rng.integers(0, len(CLASSES)))} {rng.uniform(0.05, 0.95):.6f} {rng.uniform(0.05, 0.95):.6f} "
                 f"{rng.uniform(0.05, 0.3):.6f} {rng.uniform(0.05, 0.3):.6f}" for _ in range(m)]
        (lab_dir / f"img_{k:04d}.txt").write_text("".join(ln + "\n" for ln in lines))
    return img_dir, lab_dir


def write_defn(root: Path, img_dir: Path, lab_dir: Path, thumbnails: Optional[dict] = None) -> Path:
    """a definition with train 0.75 / val 0.25 over one image folder (and thumbnail augmentation if given)"""
    text = ("class_names: [you, only, glance, once]\n"
            "dataset_split_fractions: {train: 0.75, val: 0.25}\n"
            f"dataset_paths:\n  a: {{image_path: {img_dir}, label_path: {lab_dir}}}\n")
    if thumbnails:
        text += "thumbnail_augmentation:\n" + "".join(f"  {k}: {v}\n" for k, v in thumbnails.items())
    defn = root / "defn.yml"
    defn.write_text(text)
    return defn
