"""Inference datasets (yogo/data/image_path_dataset.py:17-159): a directory (or one file) of .png images -> (image, path), or
a zarr stack of uint8 frames -> (image, made-up name).  The zarr store is read by yogo_amd/zarr_store.py (the `zarr` package
is not needed); `predict` does not index a ZarrDataset per image but hands it to yogo_amd/zarr_feed.py."""
from __future__ import annotations

import math
from functools import partial
from pathlib import Path
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch
from torch.utils.data import Dataset

from yogo_amd.yogo_dataset import read_image
from yogo_amd.zarr_store import ZarrArray, open_zarr


class ImageAndIdDataset(Dataset):
    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, str]:
        raise NotImplementedError

    def __len__(self) -> int:
        raise NotImplementedError


class ImagePathDataset(ImageAndIdDataset):
    def __init__(self, root: Union[str, Path], image_transforms: Optional[List[Callable]] = None,
                 loader: Callable[[Union[str, Path]], torch.Tensor] = read_image, normalize_images: bool = False):
        self.root = Path(root)
        if not self.root.exists():
            raise FileNotFoundError(f"{self.root} does not exist")
        self.image_paths = self.make_dataset(self.root)
        self.transforms = list(image_transforms or [])
        self.loader = loader
        self.normalize_images = normalize_images

    def make_dataset(self, path_to_data: Path) -> np.ndarray:
        if path_to_data.is_file() and path_to_data.suffix == ".png":
            img_paths = [path_to_data]
        else:
            img_paths = sorted(p for p in path_to_data.glob("*.png") if not p.name.startswith("."))
        if len(img_paths) == 0:
            raise FileNotFoundError(f"{str(path_to_data)} does not contain any images")
        return np.array([str(p) for p in img_paths]).astype(np.str_)

    def __len__(self) -> int:
        return len(self.image_paths)

    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, str]:
        image_path = str(self.image_paths[idx])
        image = self.loader(image_path)
        for t in self.transforms:
            image = t(image)
        if self.normalize_images:
            image = image / 255
        return image, image_path


class ZarrDataset(ImageAndIdDataset):
    """yogo/data/image_path_dataset.py:76-126: frame idx of an [H, W, N] array (or member idx of a group of 2-D arrays) as a
    uint8 [1, H, W] tensor, with the name ``img_<idx, zero padded>.png``.  ``len`` is what the reference's is: the number of
    chunks present in the store for an array (``zarr.Array.initialized``), the member count for a group."""

    def __init__(self, zarr_path: Union[str, Path], image_name_from_idx: Optional[Callable[[int], str]] = None,
                 image_transforms: Optional[List[Callable]] = None, normalize_images: bool = False):
        self.zarr_path = Path(zarr_path)
        if not self.zarr_path.exists():
            raise FileNotFoundError(f"{self.zarr_path} does not exist")
        self.zarr_store = open_zarr(self.zarr_path)
        self.image_name_from_idx = image_name_from_idx or self._image_name_from_idx
        self.transforms = list(image_transforms or [])
        self.normalize_images = normalize_images
        self._len = len(self.zarr_store)
        if self._len == 0:   # (the reference: math.log(0) -> ValueError)
            raise ValueError(f"{self.zarr_path} holds no images")
        self._N = int(math.log(self._len, 10) + 1)

    def _image_name_from_idx(self, idx: int) -> str:
        return f"img_{idx:0{self._N}}.png"

    def __len__(self) -> int:
        return self._len

    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, str]:
        frame = self.zarr_store[:, :, idx] if isinstance(self.zarr_store, ZarrArray) else self.zarr_store[idx][:]
        image = torch.from_numpy(frame[None, ...])
        for t in self.transforms:
            image = t(image)
        if self.normalize_images:
            image = image / 255
        return image, self.image_name_from_idx(idx)


class CenterCrop:
    """torchvision.transforms.CenterCrop((h, w)) for [C, H, W] tensors no smaller than the crop (yogo/infer.py:221-226)"""

    def __init__(self, size: Tuple[int, int]):
        self.size = (int(size[0]), int(size[1]))

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        h, w = img.shape[-2:]
        ch, cw = self.size
        if ch > h or cw > w:
            raise ValueError(f"crop {self.size} larger than the image {(h, w)}")
        top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
        return img[..., top:top + ch, left:left + cw].contiguous()


def collate_fn(batch: List[Tuple[torch.Tensor, str]]) -> Tuple[torch.Tensor, Tuple[str, ...]]:
    images, fnames = zip(*batch)
    return torch.stack(images), tuple(fnames)


def get_dataset(path_to_images: Optional[Path] = None, path_to_zarr: Optional[Path] = None,
                image_transforms: Optional[List[Callable]] = None, normalize_images: bool = False, rgb: bool = False) -> ImageAndIdDataset:
    """rgb: the files of ``path_to_images`` are read as 3 planes (an RGB model); a zarr stack holds single planes"""
    if path_to_images is not None and path_to_zarr is not None:
        raise ValueError("can only take one of 'path_to_images' or 'path_to_zarr', but got both")
    if path_to_images is not None:
        return ImagePathDataset(path_to_images, image_transforms=image_transforms, normalize_images=normalize_images,
                                **({"loader": partial(read_image, rgb=True)} if rgb else {}))
    if path_to_zarr is not None:
        return ZarrDataset(path_to_zarr, image_transforms=image_transforms, normalize_images=normalize_images)
    raise ValueError("one of 'path_to_images' or 'path_to_zarr' must not be None")
