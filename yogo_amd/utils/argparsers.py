"""Command-line surface of `yogo train | test | infer` (yogo/utils/argparsers.py:74-489): the same sub-commands, flags,
defaults and validation, built on this package's model registry.  `yogo export` (ONNX / OpenVINO, another deployment target)
is accepted by the parser and answered with an explanation by yogo_amd.__main__."""
from __future__ import annotations

import argparse
import math
import os
from pathlib import Path

from yogo_amd.dataset_definition_file import SplitFractions

try:
    boolean_action = argparse.BooleanOptionalAction
except AttributeError:   # python < 3.9
    boolean_action = "store_true"   # type: ignore


def uint(val: str) -> int:
    try:
        v = int(val)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{val} is not a valid integer")
    if v < 0:
        raise argparse.ArgumentTypeError(f"{val} is not a positive integer")
    return v


def unsigned_float(val: str) -> float:
    try:
        v = float(val)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{val} is not a valid float")
    if v < 0:
        raise argparse.ArgumentTypeError(f"{val} must be greater than or equal to 0")
    return v


def unitary_float(val: str) -> float:
    v = unsigned_float(val)
    if not 0 <= v <= 1:
        raise argparse.ArgumentTypeError(f"{val} must be in [0,1]")
    return v


def super_unitary_float(val: str) -> float:
    try:
        v = float(val)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{val} is not a valid float")
    if v < 1:
        raise argparse.ArgumentTypeError(f"{val} must be greater than or equal to 1")
    return v


def positive_gib(val: str) -> float:
    """a budget in GiB: a finite float > 0 (NaN, 0 and negative values are refused)"""
    try:
        v = float(val)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{val} is not a valid float")
    if not (math.isfinite(v) and v > 0):
        raise argparse.ArgumentTypeError(f"{val} must be a finite number of GiB greater than 0")
    return v


class SplitFractionsAction(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        try:
            setattr(namespace, self.dest, SplitFractions.from_list(list(map(float, values)), test_paths_present=False))
        except Exception as e:
            parser.error(str(e))


class CheckedParser(argparse.ArgumentParser):
    """ArgumentParser that, after parsing, runs the checks registered on it (``checks``: namespace -> an error message or None):
    the place for a condition that spans two flags of one sub-command.  A parser runs its own checks only."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.checks = []

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        for check in self.checks:
            message = check(ns)
            if message:
                self.error(message)
        return ns, rest


def _decode_needs_cache(ns):
    if ns.device_image_decode and ns.device_image_cache is None:
        return "--device-image-decode fills the device image cache: it needs --device-image-cache GIB"
    return None


def _resize_needs_decode(ns):
    if ns.device_image_resize and not (ns.device_image_decode or getattr(ns, "device_image_stream", False)):
        return "--device-image-resize resizes what the device decoded: it needs --device-image-decode"
    return None


def _decode_all_needs_decode(ns):
    if ns.device_image_decode_all and not (ns.device_image_decode or getattr(ns, "device_image_stream", False)):
        return "--device-image-decode-all widens what --device-image-decode takes: it needs --device-image-decode"
    return None


def _decode_jpeg_needs_decode(ns):
    if ns.device_image_decode_jpeg and not (ns.device_image_decode or getattr(ns, "device_image_stream", False)):
        return "--device-image-decode-jpeg widens what --device-image-decode takes: it needs --device-image-decode"
    return None


JPEG_HELP = ("also decode baseline JPEG files on the GPU (found by their first bytes, whatever their name: Huffman sequential, 8 bits, grey "
             "or YCbCr 4:4:4 / 4:2:2 / 4:2:0, up to 1040 pixels wide); progressive, arithmetic, 12-bit, CMYK and damaged files stay on "
             "the host; the same pixels as the host's decoder (default: False)")


def _test_widening_needs_stream(ns):
    for flag, on in (("--device-image-decode-all", ns.device_image_decode_all), ("--device-image-resize", ns.device_image_resize),
                     ("--device-image-decode-jpeg", ns.device_image_decode_jpeg)):
        if on and not ns.device_image_stream:
            return f"{flag} widens what --device-image-stream decodes on the GPU: it needs --device-image-stream"
    return None


STREAM_HELP = ("decode on the GPU, every epoch, the labelled images that are not resident in the device image cache (all of them without "
               "one; the test split always) instead of PIL-decoding them in DataLoader workers: no workers are started, the PNG files "
               "are inflated and unfiltered in groups of 1024 images (8-bit greyscale and RGB; other files on the host) and the batches "
               "are gathered from there; same batches.  Costs, outside the --device-image-cache budget and for as long as the loaders "
               "live: two staging tensors of 1024 images in GPU memory (1.5 GiB at 772 x 1032 greyscale) plus the decoder's scratch "
               "(about as much again, and 0.5-0.8 GiB of pinned host memory), and the first batch waits for the first whole group, "
               "0.6-1.0 s there "
               "(default: False)")


def _device_draw_needs(ns):
    if ns.device_draw and not ns.draw_boxes:
        return "--device-draw draws what --draw-boxes asks for: it needs --draw-boxes"
    if ns.device_draw and ns.output_dir is None:
        return "--device-draw writes files: it needs --output-dir (showing the images interactively stays on the host)"
    if ns.device_draw and any("\n" in n or "\r" in n for n in (ns.class_names or [])):
        return "--device-draw: a class name contains a line break; PIL lays such text out as several lines, which the device route does not do"
    if ns.device_draw_level != 0 and not ns.device_draw:
        return "--device-draw-level is the level of --device-draw's PNG encoder: it needs --device-draw"
    if ns.device_draw_level != 0 and ns.output_img_filetype != ".png":
        return f"--device-draw-level is the level of the PNG encoder: nothing is encoded for {ns.output_img_filetype} files"
    return None


def global_parser():
    parser = argparse.ArgumentParser(description="what can yogo do for you today?", allow_abbrev=False)
    sub = parser.add_subparsers(help="here is what you can do", dest="task", parser_class=CheckedParser)
    train_parser(parser=sub.add_parser("train", help="train a model", allow_abbrev=False))
    test_parser(parser=sub.add_parser("test", help="test a model", allow_abbrev=False))
    export_parser(parser=sub.add_parser("export", help="export a model", allow_abbrev=False))
    infer_parser(parser=sub.add_parser("infer", help="infer images using a model", allow_abbrev=False))
    return parser


def train_parser(parser=None):
    from yogo_amd.model_defns import MODELS
    from yogo_amd.utils.default_hyperparams import DefaultHyperparams as df

    if parser is None:
        parser = CheckedParser(description="commence a training run", allow_abbrev=False)
    parser.add_argument("dataset_descriptor_file", type=str, help="path to yml dataset descriptor file")
    parser.add_argument("--from-pretrained", type=Path, help="start training from the provided pth file", default=None)
    parser.add_argument("--dataset-split-override", action=SplitFractionsAction, nargs=3,
                        help="override dataset split fractions, in 'train val test' order - e.g. '0.7 0.2 0.1'. All of the data, "
                             "including paths specified in 'test_paths', will be randomly assigned to training, validation, and test.")
    parser.add_argument("-bs", "--batch-size", type=uint, help=f"batch size for training (default: {df.BATCH_SIZE})", default=df.BATCH_SIZE)
    parser.add_argument("-lr", "--learning-rate", "--lr", type=unitary_float, default=df.LEARNING_RATE,
                        help=f"learning rate for training (default: {df.LEARNING_RATE})")
    parser.add_argument("--lr-decay-factor", type=super_unitary_float, default=df.DECAY_FACTOR,
                        help=f"factor by which to decay lr - e.g. '2' will give a final learning rate of `lr` / 2 (default: {df.DECAY_FACTOR})")
    parser.add_argument("--label-smoothing", type=unitary_float, default=df.LABEL_SMOOTHING, help=f"label smoothing (default: {df.LABEL_SMOOTHING})")
    parser.add_argument("-wd", "--weight-decay", type=unitary_float, default=df.WEIGHT_DECAY, help=f"weight decay for training (default: {df.WEIGHT_DECAY})")
    parser.add_argument("--epochs", type=uint, default=df.EPOCHS, help=f"number of epochs to train (default: {df.EPOCHS})")
    parser.add_argument("--no-obj-weight", type=float, default=df.NO_OBJ_WEIGHT, help=f"weight for the objectness loss when there isn't an object (default: {df.NO_OBJ_WEIGHT})")
    parser.add_argument("--iou-weight", type=float, default=df.IOU_WEIGHT, help=f"weight for the iou loss (default: {df.IOU_WEIGHT})")
    parser.add_argument("--classify-weight", type=float, default=df.CLASSIFY_WEIGHT, help=f"weight for the classification loss (default: {df.CLASSIFY_WEIGHT})")
    parser.add_argument("--normalize-images", default=False, action=boolean_action, help="normalize images into [0,1] (default: False)")
    parser.add_argument("--image-hw", default=(772, 1032), nargs=2, type=int, help="height and width of the images (default: 772 1032)")
    parser.add_argument("--rgb-images", default=False, action=boolean_action, help="use RGB images instead of grayscale (default: False)")
    parser.add_argument("--model", default=None, const=None, nargs="?", choices=list(MODELS.keys()), help="model version to use - do not use with --from-pretrained")
    parser.add_argument("--half", default=False, action=boolean_action,
                        help="half precision (bf16 activations and gradients on the bf16 matrix cores, fp32 master weights) (default: False)")
    parser.add_argument("--device-image-cache", default=None, type=positive_gib, metavar="GIB",
                        help="keep decoded images resident in GPU memory within this many GiB per rank: the train split first, the val "
                             "split gets what is left (default: off)")
    parser.add_argument("--device-image-decode", default=False, action=boolean_action,
                        help="with --device-image-cache: fill the cache from PNG files inflated and unfiltered on the GPU (8-bit greyscale "
                             "and RGB) instead of a pool of PIL workers; other files are decoded on the host; same batches.  Its scratch "
                             "memory (pinned staging, stored streams, scanlines) is freed after the prefill and is not counted in the "
                             "GIB budget (default: False)")
    parser.add_argument("--device-image-decode-jpeg", default=False, action=boolean_action, help="with --device-image-decode: " + JPEG_HELP)
    parser.add_argument("--device-image-decode-all", default=False, action=boolean_action,
                        help="with --device-image-decode: also decode on the GPU every other PNG colour type and bit depth (palette, 1 / 2 / "
                             "4-bit and 16-bit, grey+alpha, RGBA, with tRNS, Adam7-interlaced) instead of handing those files to the host; "
                             "the same pixels as the host's decoder (default: False)")
    parser.add_argument("--device-image-resize", default=False, action=boolean_action,
                        help="with --device-image-decode: also resize on the GPU the 8-bit greyscale and RGB PNG files whose size is not "
                             "--image-hw (down to 1/8 per axis, or up) instead of handing them to the host; a few pixels of such an image "
                             "may differ by one grey level from the host's resize (default: False)")
    parser.add_argument("--device-image-stream", default=False, action=boolean_action, help=STREAM_HELP + ".  Independent of "
                        "--device-image-cache and composes with it; --device-image-decode-all and --device-image-resize widen what it decodes")
    parser.add_argument("--device-metrics", default=False, action=boolean_action,
                        help="match predictions to labels and accumulate the test metrics on the GPU instead of per image on the host; "
                             "same results (default: False)")
    parser.add_argument("--device", default=None, nargs="?", type=str, help="set a device for the run (accepted for compatibility; training uses one rank per visible GPU)")
    parser.add_argument("--note", default=None, type=str, help="note for the run (e.g. 'run on a TI-82')")
    parser.add_argument("--name", default=None, type=str, help="name for the run (e.g. 'ti-82_run')")
    parser.add_argument("--tags", default=None, type=str, nargs="*", help="tags for the run (e.g. '--tags test fine-tune')")
    parser.add_argument("--wandb-entity", type=str, default=os.getenv("wandb_entity"), help="wandb entity - defaults to the environment variable wandb_entity")
    parser.add_argument("--wandb-project", type=str, default=os.getenv("wandb_project"), help="wandb project name - defaults to the environment variable wandb_project")
    parser.checks.append(_decode_needs_cache)
    parser.checks.append(_resize_needs_decode)
    parser.checks.append(_decode_all_needs_decode)
    parser.checks.append(_decode_jpeg_needs_decode)
    return parser


def test_parser(parser=None):
    if parser is None:
        parser = CheckedParser(description="test a model", allow_abbrev=False)
    parser.add_argument("pth_path", type=Path)
    parser.add_argument("dataset_defn_path", type=Path)
    parser.add_argument("--wandb", default=False, action=boolean_action, help="log to wandb - this will create a new run. If neither this nor --wandb-resume-id are provided, the run will be saved to a new folder")
    parser.add_argument("--wandb-entity", type=str, default=os.getenv("WANDB_ENTITY"), help="wandb entity - defaults to the environment variable WANDB_ENTITY")
    parser.add_argument("--wandb-project", type=str, default=os.getenv("WANDB_PROJECT"), help="wandb project name - defaults to the environment variable WANDB_PROJECT")
    parser.add_argument("--wandb-resume-id", type=str, default=None, help="wandb run id - this will essentially append the results to an existing run, given by this run id")
    parser.add_argument("--dump-to-disk", action=boolean_action, default=False, help="dump results to disk as a pkl file")
    parser.add_argument("--include-mAP", action=boolean_action, default=False, help="calculate mAP as well - just a bit slower (default: False)")
    parser.add_argument("--include-background", action=boolean_action, default=False, help="include 'backround' in confusion matrix (default: False)")
    parser.add_argument("--device-metrics", default=False, action=boolean_action,
                        help="match predictions to labels and accumulate the test metrics on the GPU instead of per image on the host; "
                             "same results (default: False)")
    parser.add_argument("--device-image-stream", default=False, action=boolean_action, help=STREAM_HELP)
    parser.add_argument("--device-image-decode-jpeg", default=False, action=boolean_action, help="with --device-image-stream: " + JPEG_HELP)
    parser.add_argument("--device-image-decode-all", default=False, action=boolean_action,
                        help="with --device-image-stream: also decode on the GPU every other PNG colour type and bit depth (palette, 1 / 2 / "
                             "4-bit and 16-bit, grey+alpha, RGBA, with tRNS, Adam7-interlaced); the same pixels as the host's decoder "
                             "(default: False)")
    parser.add_argument("--device-image-resize", default=False, action=boolean_action,
                        help="with --device-image-stream: also resize on the GPU the PNG files whose size is not the model's (down to 1/8 "
                             "per axis, or up); a few pixels of such an image may differ by one grey level from the host's resize "
                             "(default: False)")
    parser.add_argument("--note", default=None, type=str, help="note for the run (e.g. 'run on a TI-82')")
    parser.add_argument("--tags", default=None, type=str, nargs="*", help="tags for the run (e.g. '--tags test fine-tune')")
    if hasattr(parser, "checks"):
        parser.checks.append(_test_widening_needs_stream)
    return parser


def export_parser(parser=None):
    if parser is None:
        parser = argparse.ArgumentParser(description="convert a pth file to onnx or Intel IR", allow_abbrev=False)
    parser.add_argument("input", type=str, help="path to input pth file")
    parser.add_argument("--crop-height", type=unitary_float, help="crop image verically - '-c 0.25' will crop images to (round(0.25 * height), width)")
    parser.add_argument("--output-filename", type=str, help="output filename")
    parser.add_argument("--simplify", default=True, action=boolean_action, help="attempt to simplify the onnx model")
    return parser


def infer_parser(parser=None):
    if parser is None:
        parser = CheckedParser(description="infer results over some dataset", allow_abbrev=False)
    parser.add_argument("pth_path", type=Path, help="path to .pth file defining the model")
    data_source = parser.add_mutually_exclusive_group(required=True)
    data_source.add_argument("--path-to-images", "--path-to-image", type=Path, default=None,
                             help="path to image or images; if path is a single image, run inference on that image; if path is a directory, "
                                  "run inference on all images in that directory")
    data_source.add_argument("--path-to-zarr", type=Path, default=None, help="path to zarr file")
    parser.add_argument("--draw-boxes", default=False, action=boolean_action,
                        help="plot and either save (if --output-dir is set) or show each image (default: False)")
    parser.add_argument("--save-preds", default=False, action=boolean_action,
                        help="save predictions in YOGO label format - requires `--output-dir` to be set (default: False)")
    parser.add_argument("--save-npy", default=False, action=boolean_action,
                        help="Parse and save predictions in the same format as on scope - requires `--output-dir` to be set (default: False)")
    parser.add_argument("--count", action=boolean_action, default=False,
                        help="display the final predicted counts per-class (default: False)")
    parser.add_argument("--device-outputs", default=False, action=boolean_action,
                        help="compact and count the kept predictions of --save-preds / --save-npy / --count on the GPU and read them once "
                             "instead of copying every batch's padded rows to the host; same files and counts (default: False)")
    parser.add_argument("--device-image-decode", default=False, action=boolean_action,
                        help="with --path-to-images: inflate and unfilter 8-bit greyscale PNG files on the GPU instead of decoding them "
                             "in DataLoader workers; other files are decoded on the host; same outputs (default: False)")
    parser.add_argument("--device-image-decode-jpeg", default=False, action=boolean_action, help="with --device-image-decode: " + JPEG_HELP)
    parser.add_argument("--device-image-decode-all", default=False, action=boolean_action,
                        help="with --device-image-decode: decode on the GPU every PNG colour type and bit depth (palette, 1 / 2 / 4-bit and "
                             "16-bit, grey+alpha, RGBA, RGB, with tRNS, Adam7-interlaced), converted as the host's decoder converts them, "
                             "and accept an RGB model; only files that are no PNG stay on the host (default: False)")
    parser.add_argument("--device-draw", default=False, action=boolean_action,
                        help="with --draw-boxes and --output-dir: draw the boxes and encode the PNG files on the GPU, one launch each per "
                             "batch, instead of PIL on the host image by image; the files decode to the same pixels, their bytes are "
                             "compressed differently.  With --output-img-filetype .tif / .tiff only the drawing moves: an uncompressed "
                             "TIFF has nothing to encode, PIL writes the file from the pixels read back (default: False)")
    parser.add_argument("--device-draw-level", type=int, choices=[0, 1], default=0,
                        help="with --device-draw and PNG output: 0 codes every band of a file as Huffman-coded literals, 1 adds LZ77 "
                             "matches -- smaller files, so less to read back and write, for a longer encode launch and four times the "
                             "encoder's work space (default: 0)")
    parser.add_argument("--output-dir", type=Path, default=None,
                        help="path to directory for results, either --draw-boxes or --save-preds")
    parser.add_argument("--class-names", help="list of class names - will default to integers if not provided", nargs="*", type=str, default=None)
    parser.add_argument("--batch-size", type=uint, help="batch size for inference (default: 64)", default=64)
    parser.add_argument("--device", type=str, nargs="?", help="set a device for the run - the hot path needs an MI355X ('cuda')", default=None)
    parser.add_argument("--half", default=False, action=boolean_action, help="half precision (bf16) inference (default: False)")
    parser.add_argument("--crop-height", type=unitary_float,
                        help="crop image verically - '-c 0.25' will crop images to (round(0.25 * height), width)")
    parser.add_argument("--output-img-filetype", type=str, choices=[".png", ".tif", ".tiff"], default=".png",
                        help="filetype for output images (default: .png)")
    parser.add_argument("--obj-thresh", type=unsigned_float, default=0.5, help="objectness threshold for predictions (default: 0.5)")
    parser.add_argument("--iou-thresh", type=unsigned_float, default=0.5, help="intersection over union threshold for predictions (default: 0.5)")
    parser.add_argument("--min-class-confidence-threshold", type=unitary_float, default=0.0,
                        help="minimum confidence for a class to be considered - i.e. the max confidence must be greater than this value (default: 0.0)")
    parser.add_argument("--heatmap-mask-path", type=Path, default=None,
                        help="path to heatmap mask for the run (accepted for compatibility, unused -- as in the reference)")
    parser.add_argument("--use-tqdm", default=True, action=boolean_action, help="use tqdm progress bar (default: True)")
    parser.checks.append(_decode_all_needs_decode)
    parser.checks.append(_decode_jpeg_needs_decode)
    parser.checks.append(_device_draw_needs)
    return parser
