"""``predict`` / ``do_infer`` -- the driver behind `yogo infer` (yogo/infer.py:139-451) on the HIP path.

Same arguments, output files and return value as the reference.  Per batch: ONE forward (fp32, or the bf16 matrix-core path
under ``half`` -- the reference's bf16 autocast, infer.py:313-317) and, per requested output, ONE batched threshold + NMS
launch for the whole batch (``save_predictions`` / ``format_to_numpy_batched`` / ``get_prediction_class_counts``) instead of the
reference's per-image Python loops over ``format_preds`` (infer.py:45,73); unless the decoded tensor itself is asked for, the box
decode runs inside that launch's loads (``YOGO.forward_raw``).  No ``torch.compile``: there is no graph to trace,
the model is already a fixed sequence of hand-written kernels.

``device_outputs=True`` (``yogo infer --device-outputs``) keeps what those launches leave on the device: a ``PredictionSink`` per
requested output (yogo_amd/pred_sink.py) compacts and counts the kept rows in HBM, and the host reads them when a sink is drained --
after the loop, or when ``flush_rows`` records have piled up -- instead of copying the padded rows of every batch.  The text of
``save_preds`` is formatted on the device too (yogo_amd/csrc/pred_text.hip): the host writes ready byte ranges.  Same files, same
counts.

``device_image_decode=True`` (``yogo infer --path-to-images DIR --device-image-decode``) replaces the DataLoader and its PIL-decoding
workers by a ``PngDeviceFeed`` (yogo_amd/png_feed.py): the files' zlib streams are inflated and their PNG filters reversed on the
device, crop and ``/ 255`` included.  Same batches and names; ``ValueError`` with ``path_to_zarr`` and for an RGB model.

``device_draw=True`` (``yogo infer --draw-boxes --device-draw --output-dir DIR``) draws the boxes and encodes the PNG files on the
device (yogo_amd/draw.py): per batch one threshold + NMS launch, one render launch, one encode call, one read of the finished file
bytes; the files are written on a small pool of threads.  Same file names, and every file decodes to the same pixels as the host
route's; the PNG bytes are compressed differently.  Independent of ``device_outputs``.
"""
from __future__ import annotations

import datetime
import json
import warnings
from pathlib import Path
from typing import List, Optional, Union

import numpy as np
import torch
from torch.utils.data import DataLoader

from yogo_amd.image_path_dataset import CenterCrop, ZarrDataset, collate_fn, get_dataset
from yogo_amd.model import YOGO
from yogo_amd.pred_sink import PredictionSink, npy_columns
from yogo_amd.utils import format_to_numpy_batched, get_prediction_class_counts, save_predictions  # noqa: F401
from yogo_amd.utils.prediction_formatting import format_preds_batched, prediction_rows_to_text  # noqa: F401  (the text's definition; the host path calls it in save_predictions)
from yogo_amd.utils.utils import choose_device, draw_yogo_prediction
from yogo_amd.yogo_dataloader import choose_dataloader_num_workers


def get_model_name_from_pth(path_to_pth: Union[str, Path]) -> Optional[str]:
    return torch.load(Path(path_to_pth), map_location="cpu", weights_only=False).get("model_name", None)


def write_metadata(metadata_path: Path, **kwargs) -> None:
    """a json file with the kwargs, next to the .npy (yogo/infer.py:129-135)"""
    with open(Path(metadata_path).with_suffix(".json"), "w") as f:
        json.dump(kwargs, f, indent=4)


@torch.no_grad()
def predict(
    path_to_pth: str,
    *,
    path_to_images: Optional[Path] = None,
    path_to_zarr: Optional[Path] = None,
    output_dir: Optional[str] = None,
    draw_boxes: bool = False,
    save_preds: bool = False,
    save_npy: bool = False,
    class_names: Optional[List[str]] = None,
    count_predictions: bool = False,
    batch_size: int = 64,
    obj_thresh: float = 0.5,
    iou_thresh: float = 0.5,
    vertical_crop_height: Optional[float] = None,
    use_tqdm: bool = False,
    device: Optional[Union[str, torch.device]] = None,
    output_img_ftype: str = ".png",
    requested_num_workers: Optional[int] = None,
    min_class_confidence_threshold: float = 0.0,
    half: bool = False,
    return_full_predictions: bool = False,
    device_outputs: bool = False,
    device_image_decode: bool = False,
    device_image_decode_all: bool = False,
    device_image_decode_jpeg: bool = False,
    device_draw: bool = False,
    device_draw_level: int = 0,
) -> Optional[torch.Tensor]:
    if device_draw_level != 0:   # (0 is valid everywhere: it asks for nothing)
        from yogo_amd.draw import check_level

        check_level(device_draw_level)
        if not device_draw:
            raise ValueError("device_draw_level is the level of device_draw's PNG encoder: it needs device_draw")
        if output_img_ftype != ".png":
            raise ValueError(f"device_draw_level is the level of the PNG encoder: nothing is encoded for {output_img_ftype} files")
    if device_draw:   # (before anything touches a device or the output directory)
        from yogo_amd.draw import check_labels

        if not draw_boxes:
            raise ValueError("device_draw draws what draw_boxes asks for: it needs draw_boxes")
        if output_dir is None:
            raise ValueError("device_draw writes files: it needs output_dir (showing the images interactively stays on the host)")
        check_labels(class_names or [])
    if save_preds and draw_boxes:
        raise ValueError("cannot save predictions in YOGO format and draw_boxes at the same time")
    elif output_dir is not None and not (save_preds or draw_boxes or save_npy):
        warnings.warn(f"output dir is not None (is {output_dir}), but it will not be used since save_preds and draw_boxes are both false")
    elif output_dir is not None:
        Path(output_dir).mkdir(exist_ok=True, parents=False)
    elif save_preds:
        raise ValueError("output_dir must not be None if save_preds is True")
    elif output_img_ftype not in [".png", ".tif", ".tiff"]:
        raise ValueError(f"only .png, .tif, and .tiff are supported for output img filetype; got {output_img_ftype}")

    if device_image_decode_all and not device_image_decode:
        raise ValueError("device_image_decode_all widens what device_image_decode takes: it needs device_image_decode")
    if device_image_decode_jpeg and not device_image_decode:
        raise ValueError("device_image_decode_jpeg widens what device_image_decode takes: it needs device_image_decode")
    if device_image_decode and path_to_zarr is not None:
        raise ValueError("device_image_decode decodes the PNG files of path_to_images; a zarr stack has its own device route")
    device = torch.device(device or choose_device())
    if device.type != "cuda":
        raise RuntimeError(f"yogo_amd: inference runs on an MI355X (got device {device}); there is no CPU compute path")
    model, cfg = YOGO.from_pth(Path(path_to_pth), inference=True)
    model.eval()
    model.to(device)

    transforms = []
    img_h, img_w = (int(v) for v in model.get_img_size())
    if vertical_crop_height:
        crop_px = int(round(vertical_crop_height * img_h))
        transforms.append(CenterCrop((crop_px, img_w)))
        model.resize_model(crop_px)
        img_h = crop_px
    assert model.img_size.numel() == 2, f"YOGO model must be 2D, is {model.img_size}"
    if device_image_decode and bool(model.is_rgb) and not device_image_decode_all:
        raise ValueError("device_image_decode reads 8-bit greyscale images; this model takes RGB input (device_image_decode_all converts "
                         "every PNG colour type to RGB planes on the device)")
    num_classes = int(model.num_classes)
    if class_names is not None and len(class_names) != num_classes:
        raise ValueError(f"expected {num_classes} class names, got {len(class_names)}")

    image_dataset = get_dataset(path_to_images=path_to_images, path_to_zarr=path_to_zarr, image_transforms=transforms,
                                normalize_images=bool(model.normalize_images), rgb=bool(model.is_rgb))
    if isinstance(image_dataset, ZarrDataset):
        # no workers and none of the reference's slow-path warning (infer.py:257-265): chunks are read on threads and unpacked
        # on the device, crop and / 255 included (yogo_amd/zarr_feed.py); the batches arrive on the device
        from yogo_amd.zarr_feed import ZarrDeviceFeed

        with torch.cuda.device(device):
            loader = ZarrDeviceFeed(image_dataset, batch_size, device, crop=(img_h, img_w) if vertical_crop_height else None,
                                    normalize=bool(model.normalize_images))
    elif device_image_decode:
        # the files' zlib streams are inflated and unfiltered on the device, crop and / 255 included (yogo_amd/png_feed.py)
        from yogo_amd.png_feed import PngDeviceFeed

        with torch.cuda.device(device):
            loader = PngDeviceFeed(image_dataset, batch_size, device, crop=(img_h, img_w) if vertical_crop_height else None,
                                   normalize=bool(model.normalize_images), all_types=bool(device_image_decode_all),
                                   rgb=bool(model.is_rgb), **({"jpeg": True} if device_image_decode_jpeg else {}))
    else:
        num_workers = choose_dataloader_num_workers(len(image_dataset), requested_num_workers=requested_num_workers)
        loader = DataLoader(image_dataset, batch_size=batch_size, shuffle=False, drop_last=False, pin_memory=True, collate_fn=collate_fn,
                            num_workers=num_workers)
    try:
        from tqdm import tqdm

        pbar = tqdm(disable=not use_tqdm, unit="images", total=len(image_dataset))
    except ImportError:   # pragma: no cover
        pbar = None

    results = torch.zeros((len(image_dataset), 5 + num_classes, model.Sy, model.Sx)) if return_full_predictions else None
    np_results: list = []
    tot_counts = torch.zeros((num_classes,)) if count_predictions else None
    # device_outputs: one sink per requested output; the names of the images a sink still holds stay here
    npy_sink = PredictionSink(device, num_classes, "npy", img_hw=(img_h, img_w)) if device_outputs and save_npy else None
    txt_sink = PredictionSink(device, num_classes, "rows") if device_outputs and save_preds else None
    count_sink = PredictionSink(device, num_classes, "rows") if device_outputs and count_predictions else None
    txt_names: List[Path] = []
    npy_chunks: list = []   # (records, per-image counts) per drain
    draw_sink = None
    if device_draw:
        from yogo_amd.draw import DrawSink

        draw_sink = DrawSink(device, class_names or [str(c) for c in range(num_classes)], bool(model.normalize_images), output_dir,
                             output_img_ftype, level=device_draw_level)

    def drain_txt() -> None:
        # the files' bytes come ready from the device (PredictionSink.drain_text: what prediction_rows_to_text gives, byte for byte)
        text, offsets = txt_sink.drain_text()
        assert len(offsets) - 1 == len(txt_names), f"{len(offsets) - 1} images drained, {len(txt_names)} file names held"
        data = memoryview(text)
        for k, fname in enumerate(txt_names):
            with open(fname, "wb") as f:
                f.write(data[offsets[k]: offsets[k + 1]])
        txt_names.clear()

    file_iterator = enumerate(loader)
    while True:
        # forgiving to malformed images, as the reference (infer.py:300-309)
        try:
            i, (img_batch, fnames) = next(file_iterator)
        except StopIteration:
            break
        except RuntimeError as e:
            warnings.warn(f"got error {e}; continuing")
            continue
        x = img_batch.to(device, non_blocking=True)
        if draw_boxes and img_batch.is_cuda and not device_draw:
            img_batch = img_batch.cpu()   # (zarr / PNG feed) drawing is host work
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(half)):
            # the decoded tensor itself is only needed for drawing and for return_full_predictions; every other output goes
            # through the threshold + NMS kernel, which decodes the head's raw output as it loads it
            res = model(x) if ((draw_boxes and not device_draw) or return_full_predictions) else model.forward_raw(x)
        # the fused launch re-runs the decode per consumer: with more than one post-process output of this batch, decode ONCE
        if sum(map(bool, (save_preds, save_npy, count_predictions))) > 1 and hasattr(res, "decoded"):
            res = res.decoded()
        if device_draw:
            # the rows of the per-image _format_tensor_for_rects in the same order, for the whole batch; drawn, encoded and read
            # back by the sink (yogo_amd/draw.py), the batch as the model saw it: nothing of it is copied to the host
            rows, _, counts = format_preds_batched(res, obj_thresh, iou_thresh, "xyxy", min_class_confidence_threshold)
            draw_sink.submit(x, rows, counts, fnames)
        elif draw_boxes:
            for k in range(img_batch.shape[0]):
                bbox_img = draw_yogo_prediction(img=img_batch[k, ...], prediction=res[k, ...], obj_thresh=obj_thresh, iou_thresh=iou_thresh,
                                                min_class_confidence_threshold=min_class_confidence_threshold, labels=class_names,
                                                images_are_normalized=bool(model.normalize_images))
                if output_dir is not None:
                    bbox_img.save(Path(output_dir) / Path(fnames[k]).with_suffix(output_img_ftype).name, compress_level=1)
                else:   # pragma: no cover  (interactive display)
                    import matplotlib.pyplot as plt

                    fig, ax = plt.subplots()
                    ax.set_axis_off()
                    ax.imshow(bbox_img)
                    plt.show()
                    plt.close()
        if device_outputs:
            # the launches of the default path below with the same arguments (--save-npy's fixed 0.5 / 0.5 / xyxy included); the
            # rows and counts go to the sinks instead of to the host, and nothing in here waits for the device
            if save_preds:
                assert output_dir is not None, "output_dir must not be None if save_preds is True"
                rows, _, counts = format_preds_batched(res, obj_thresh, iou_thresh)
                txt_sink.append(rows, counts, i * batch_size)
                txt_names.extend(Path(output_dir) / Path(f).with_suffix(".txt").name for f in fnames)
                if txt_sink.should_flush():
                    drain_txt()
            if save_npy:
                rows, _, counts = format_preds_batched(res, box_format="xyxy")
                npy_sink.append(rows, counts, i * batch_size)
                if npy_sink.should_flush():
                    npy_chunks.append(npy_sink.drain())
            if count_predictions:
                rows, _, counts = format_preds_batched(res, obj_thresh, iou_thresh, "cxcywh", min_class_confidence_threshold)
                count_sink.add_counts(rows, counts)
        if save_preds and not device_outputs:
            assert output_dir is not None, "output_dir must not be None if save_preds is True"
            save_predictions([Path(output_dir) / Path(f).with_suffix(".txt").name for f in fnames], res, obj_thresh=obj_thresh, iou_thresh=iou_thresh)
        if save_npy and not device_outputs:
            ids = [i * batch_size + j for j in range(res.shape[0])]
            np_results.extend(format_to_numpy_batched(ids, res, img_h, img_w))
        if count_predictions and not device_outputs:
            tot_counts += get_prediction_class_counts(res, obj_thresh=obj_thresh, iou_thresh=iou_thresh,
                                                      min_class_confidence_threshold=min_class_confidence_threshold)
        if return_full_predictions:
            results[i * batch_size: i * batch_size + res.shape[0], ...] = res.cpu()
        if pbar is not None:
            pbar.update(res.shape[0])
    if pbar is not None:
        pbar.close()

    if txt_sink is not None:
        drain_txt()
    if draw_sink is not None:
        draw_sink.close()
    if count_sink is not None:
        tot_counts = count_sink.class_counts()
    if count_predictions:
        print(list(zip(class_names or range(num_classes), map(int, tot_counts))))
    if save_npy:
        if npy_sink is not None:   # records [N, 8 + C] in image order -> the (8 + C) x N array np.hstack gives below
            npy_chunks.append(npy_sink.drain())
            pred_tensors = npy_columns(npy_chunks, num_classes)
        else:
            pred_tensors = np.hstack(np_results) if np_results else np.zeros((8 + num_classes, 0), dtype=np.float32)
        filename = Path(path_to_images).resolve().parent.stem if path_to_images else Path(path_to_zarr).resolve().stem
        base = Path(output_dir).resolve() if output_dir is not None else Path.cwd().resolve()
        fp = base / Path(filename).with_suffix(".npy")
        np.save(fp, pred_tensors)
        write_metadata(fp.with_suffix(".json"), run_name=fp.with_suffix("").name, model_name=get_model_name_from_pth(path_to_pth),
                       obj_thresh=obj_thresh, iou_thresh=iou_thresh, vertical_crop_height_px=img_h,
                       write_date=datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"))
    return results if return_full_predictions else None


def do_infer(args) -> None:
    predict(
        args.pth_path, path_to_images=args.path_to_images, path_to_zarr=args.path_to_zarr, output_dir=args.output_dir,
        draw_boxes=args.draw_boxes, save_preds=args.save_preds, save_npy=args.save_npy, class_names=args.class_names,
        obj_thresh=args.obj_thresh, iou_thresh=args.iou_thresh, batch_size=args.batch_size, device=args.device, use_tqdm=args.use_tqdm,
        vertical_crop_height=args.crop_height, count_predictions=args.count, output_img_ftype=args.output_img_filetype,
        min_class_confidence_threshold=args.min_class_confidence_threshold, half=args.half, device_outputs=args.device_outputs,
        device_image_decode=args.device_image_decode, device_image_decode_all=args.device_image_decode_all,
        device_image_decode_jpeg=args.device_image_decode_jpeg,
        device_draw=args.device_draw,
        device_draw_level=args.device_draw_level,
    )
