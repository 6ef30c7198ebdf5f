"""CLI entry (mirror of the reference's main.py:17-161) on the HIP UNet path.

Same flags as the reference (``--dataset_path``, ``--checkpoint_path``, ``--bce_ratio`` ...
``--use_data_parallel``), with four additions (``--mfma {fp32,bf16}`` selects the GEMM
arithmetic of ModUNet / ResUNet; ``--use_amp_autocast`` stays parsed and ignored):
``--pp_largest`` / ``--pp_min_area`` / ``--pp_fill_holes`` / ``--pp_connectivity`` / ``--lesion_metrics``
add connected-component post-processing and lesion-level detection to the test report;
``--tta {none,hflip,flips,d4}`` / ``--tta_merge {prob,logit}`` add flip / rotation test-time
augmentation to it (a ``TTA`` block after the unchanged raw one);
``--curve_metrics`` / ``--curve_bins`` add a threshold sweep (AUROC, AP, best Dice and its threshold)
and ``--threshold`` the metrics at another operating point (an ``OPT`` block);
``--mode predict --input_dir DIR --output_dir DIR`` segments frames that have no masks and writes
source-size mask and contour-overlay PNGs and a ``predictions.csv`` (``--contour_width``,
``--overlay_alpha``, ``--save_prob``), and ``--save_overlays`` writes the test split's overlays
(``test_overlay_<index>.png``) without matplotlib: the device-side successor of the reference's
contour plot (utils/trainer.py:262-299);
``--model_type`` picks the network
(``ResUNet``: models/mod.py:88-131, what the reference hard-codes at main.py:120-122;
``ModUNet``: models/mod.py:9-66; ``UNet``: models/model.py, the BASELINE network and the
default here; ``--base_filters`` / ``--depth`` for the mod.py ones, default 64 / 5 as
there), ``--mode {train,test,both,predict}`` replaces the commented-out
``trainer.train()`` / hard-wired ``trainer.test()`` (:156-157), and ``--synthetic N`` runs
on N synthetic samples per split when the DDTI images are not on disk.

Multi-GPU: launch one process per GPU, e.g.
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 main.py --mode train ...
(RCCL backend; replaces nn.DataParallel of utils/trainer.py:28-30).
"""
import argparse
import logging
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from data.data_loader import (DataParallelShardSampler, DecodeU8, DeviceResizeLoader,  # noqa: E402
                              MedicalDataset, SyntheticSegmentation, create_dataloader,
                              decode_u8, dp_collate, u8_collate)
from models.mod import ResUNet  # noqa: E402
from models.mod import UNet as ModUNet  # noqa: E402
from models.model import UNet  # noqa: E402
from utils.trainer import Trainer  # noqa: E402
from utils.transforms import Compose, Resize, ToTensor, build_train_transform  # noqa: E402
from utils.utils import Config, create_logger, set_seed  # noqa: E402


def _flag(v):
    # the reference uses type=bool (main.py:59-60), which turns any string into True
    return bool(v)


def _threshold(v):
    from unet_hip.functional import THRESHOLD_CRITERIA, parse_threshold
    if v in THRESHOLD_CRITERIA:
        return v
    try:
        parse_threshold(float(v))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return float(v)


def get_parser(argv=None):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--dataset_path", default="data/dataset", type=str)
    p.add_argument("--dataset", default="DDTI", type=str)
    p.add_argument("--checkpoint_path", default="", type=str)
    p.add_argument("--config_path", default=None, type=str)
    p.add_argument("--p_crop", default=0, type=float)
    for f in ("--use_elastic", "--use_speckle", "--use_tgc", "--use_clahe", "--use_mixup"):
        p.add_argument(f, action="store_true")
    p.add_argument("--mixup_alpha", type=float, default=0.2)
    p.add_argument("--mixup_prob", type=float, default=0.3)
    p.add_argument("--model_type", default="UNet", type=str, help="UNet | ModUNet | ResUNet")
    p.add_argument("--base_filters", default=64, type=int, help="ModUNet / ResUNet (mod.py:13)")
    p.add_argument("--gpu_transforms", action="store_true",
                   help="decode on the host, Resize + ToTensor on the GPU (bit-identical)")
    p.add_argument("--gpu_augment", action="store_true",
                   help="implies --gpu_transforms; the training augmentations (Flip, Rotate, "
                        "AdjustBrightness, TGC, CLAHE) run on the GPU too (bit-identical); the "
                        "host workers decode and draw the parameters")
    p.add_argument("--gpu_augment_all", action="store_true",
                   help="implies --gpu_augment; ElasticDeform and SpeckleNoise run on the GPU too "
                        "(bit-identical): the host workers draw their float64 fields and send "
                        "them with the planes, and touch no pixel")
    p.add_argument("--depth", default=5, type=int, help="ModUNet / ResUNet (mod.py:14)")
    p.add_argument("--bce_ratio", type=float, default=1)
    p.add_argument("--dice_ratio", type=float, default=0)
    p.add_argument("--focal_ratio", type=float, default=1)
    p.add_argument("--boundary_ratio", type=float, default=0)
    p.add_argument("--lovasz_ratio", type=float, default=0,
                   help="weight of the Lovasz hinge loss (the Jaccard surrogate), sorted on the GPU; 0: off")
    p.add_argument("--num_workers", default=4, type=int)
    p.add_argument("--epochs", type=int, default=10000)
    p.add_argument("--batch_size", default=16, type=int)
    p.add_argument("--lr", type=float, default=1e-5)
    p.add_argument("--weight_decay", type=float, default=1e-2)  # unused, as in the reference
    p.add_argument("--save_interval", default=20, type=int)
    p.add_argument("--early_stop_patience", default=50, type=int)
    p.add_argument("--alpha", type=float, default=2)
    p.add_argument("--use_data_parallel", type=_flag, default=True)
    p.add_argument("--use_amp_autocast", type=_flag, default=False)
    p.add_argument("--mfma", default="fp32", choices=("fp32", "bf16"),
                   help="ModUNet / ResUNet: conv GEMM arithmetic (bf16: operands rounded to "
                        "bf16, f32 accumulate; base_filters 64, 128 or 256)")
    p.add_argument("--mode", choices=["train", "test", "both", "predict"], default="test")
    p.add_argument("--input_dir", default="", type=str, help="predict: the directory of image files to segment")
    p.add_argument("--output_dir", default="", type=str,
                   help="predict: where <stem>_mask.png, <stem>_overlay.png and predictions.csv go")
    p.add_argument("--contour_width", type=int, default=1, choices=(1, 2, 3),
                   help="predict / --save_overlays: contour width in pixels")
    p.add_argument("--overlay_alpha", type=int, default=0, metavar="A",
                   help="predict / --save_overlays: red tint of the predicted region, 0..256 (0: none)")
    p.add_argument("--save_prob", action="store_true",
                   help="predict: also write <stem>_score.npy, the score plane at the source size")
    p.add_argument("--save_overlays", action="store_true",
                   help="test: write test_overlay_<index>.png (prediction red, ground truth blue) for every "
                        "test sample, rendered on the GPU; needs neither matplotlib nor scikit-image")
    p.add_argument("--image_size", type=int, default=512)
    p.add_argument("--synthetic", type=int, default=0, help="synthetic samples per split")
    p.add_argument("--surface_metrics", action="store_true",
                   help="test: also report HD95, HD and ASSD (pixels) of the predicted contours, "
                        "computed on the GPU")
    p.add_argument("--pp_largest", action="store_true",
                   help="test: also report the metrics of the masks cleaned on the GPU; keep only "
                        "the largest connected component")
    p.add_argument("--pp_min_area", type=int, default=0, metavar="N",
                   help="test: ... drop the components with fewer than N pixels")
    p.add_argument("--pp_fill_holes", action="store_true", help="test: ... fill the holes")
    p.add_argument("--pp_connectivity", type=int, default=1, choices=(1, 2),
                   help="connectivity of the components (1: 4 neighbours, 2: 8)")
    p.add_argument("--lesion_metrics", action="store_true",
                   help="test: also report lesion-level recall, precision and false-positive "
                        "components per image (of the cleaned masks when a --pp_* option is set)")
    p.add_argument("--lesion_table", action="store_true",
                   help="predict: also write lesions.csv, one line per connected component of every frame's "
                        "final mask (size, position, Feret diameter, axes, perimeter, holes, taller-than-wide), "
                        "measured on the GPU at --pp_connectivity")
    p.add_argument("--pixel_spacing", type=float, default=None, metavar="MM",
                   help="--lesion_table: millimetres per pixel; adds feret_max_mm and area_mm2")
    p.add_argument("--lesion_echo", action="store_true",
                   help="--lesion_table: also measure every component's grey values on the GPU (histogram, a ring "
                        "of surrounding tissue, co-occurrence texture) and append the echo columns: mean, spread, "
                        "quantiles, entropy, lesion-to-ring ratio and contrast, hypo- / iso- / hyperechoic class, "
                        "GLCM contrast, homogeneity, energy, correlation, entropy")
    p.add_argument("--echo_ring", type=int, default=None, metavar="W",
                   help="--lesion_echo: width in pixels of the ring of surrounding tissue, 0..16 (0: no ring; "
                        f"default {ECHO_RING_DEFAULT})")
    p.add_argument("--echo_levels", type=int, default=None, choices=(8, 16, 32),
                   help=f"--lesion_echo: grey levels of the co-occurrence matrix (default {ECHO_LEVELS_DEFAULT})")
    p.add_argument("--lesion_shape", action="store_true",
                   help="test: also report how the largest predicted lesion's size and shape agree with the "
                        "annotated one's (Feret diameter, area, centroid, taller-than-wide), measured on the GPU")
    p.add_argument("--tta", default="none", choices=("none", "hflip", "flips", "d4"),
                   help="test: also predict the flipped (hflip: 2 views, flips: 4) or flipped and "
                        "rotated (d4: 8) images, un-warp and merge on the GPU; a second block reports "
                        "the merged masks, and --surface_metrics / --pp_* / --lesion_metrics read them")
    p.add_argument("--tta_merge", default="prob", choices=("prob", "logit"),
                   help="--tta: average the views' probabilities (prob) or their logits (logit)")
    p.add_argument("--curve_metrics", action="store_true",
                   help="test: also sweep the threshold on the GPU and report AUROC, average precision, "
                        "the best global and mean per-image Dice with their thresholds")
    p.add_argument("--curve_bins", type=int, default=256, metavar="B",
                   help="operating points of the sweep: thresholds k / B (a power of two in 2..1024)")
    p.add_argument("--threshold", type=_threshold, default=0.5, metavar="T",
                   help="test: also report the metrics at another threshold: a probability in (0, 1) "
                        "(snapped to k / B), or val-dice / val-image-dice to let the validation split "
                        "pick the threshold of the best global / mean per-image Dice (not with --tta)")
    args = p.parse_args(argv)
    if not 0 <= args.overlay_alpha <= 256:
        p.error(f"--overlay_alpha must be in 0..256, got {args.overlay_alpha}")
    e = lesion_args_error(args)
    if e:
        p.error(e)
    if args.echo_ring is None:
        args.echo_ring = ECHO_RING_DEFAULT
    if args.echo_levels is None:
        args.echo_levels = ECHO_LEVELS_DEFAULT
    if args.mode == "predict":
        e = predict_args_error(args, int(os.environ.get("WORLD_SIZE", "1")))
        if e:
            p.error(e)
    return args


ECHO_RING_DEFAULT, ECHO_LEVELS_DEFAULT = 8, 16  # what --echo_ring / --echo_levels are when not given


def lesion_args_error(args):
    """What the lesion-table flags refuse, as a message (None: nothing)."""
    if args.lesion_table and args.mode != "predict":
        return f"--lesion_table writes lesions.csv in --mode predict only (got --mode {args.mode})"
    if args.pixel_spacing is not None and not args.pixel_spacing > 0:
        return f"--pixel_spacing must be positive millimetres per pixel, got {args.pixel_spacing}"
    if args.pixel_spacing is not None and not args.lesion_table:
        return "--pixel_spacing scales the columns of --lesion_table; pass that too"
    if args.lesion_echo and not args.lesion_table:
        return "--lesion_echo adds columns to lesions.csv: it needs --mode predict --lesion_table"
    if not args.lesion_echo and (args.echo_ring is not None or args.echo_levels is not None):
        return "--echo_ring and --echo_levels tune --lesion_echo; pass that too"
    if args.echo_ring is not None and not 0 <= args.echo_ring <= 16:
        return f"--echo_ring must be in 0..16, got {args.echo_ring}"
    return None


def predict_args_error(args, world=1):
    """What --mode predict refuses, as a message (None: nothing)."""
    from unet_hip.predict import check_predict_options
    if world > 1:
        return "--mode predict is single-process; launch it without torchrun"
    if not args.input_dir or not args.output_dir:
        return "--mode predict needs --input_dir and --output_dir"
    if not args.checkpoint_path:
        return "--mode predict needs --checkpoint_path: it segments with trained weights only"
    try:
        check_predict_options(args.tta, args.threshold)
    except ValueError as e:
        return f"--mode predict: {e}"
    return None


def build_model(args):
    if args.model_type == "ResUNet":
        return ResUNet(base_filters=args.base_filters, depth=args.depth, mfma_dtype=args.mfma)
    if args.model_type == "ModUNet":
        return ModUNet(base_filters=args.base_filters, depth=args.depth, mfma_dtype=args.mfma)
    if args.mfma != "fp32":
        raise SystemExit("--mfma bf16: models/model.py UNet has no bf16 path (UNET_ERR_UNSUPPORTED); "
                         "use --model_type ModUNet or ResUNet")
    return UNet()


IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def same_stem(names):
    """The file names of ``names`` whose stem another one has too (their outputs would collide)."""
    stems = [os.path.splitext(n)[0] for n in names]
    return [n for n, st in zip(names, stems) if stems.count(st) > 1]


def predict(args):
    """--mode predict: every image file of --input_dir through unet_hip.Predictor in batches of
    --batch_size; masks, overlays and predictions.csv into --output_dir."""
    from PIL import Image

    from unet_hip.predict import CSV_HEADER, Predictor, lesion_csv_header, lesion_lines, save_predictions
    if args.model_type not in ("UNet", "ModUNet", "ResUNet"):
        raise SystemExit(f"model_type {args.model_type!r}: the HIP path has UNet, ModUNet and ResUNet")
    set_seed(seed=42)
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(args)
    if not os.path.isfile(args.checkpoint_path):
        raise SystemExit(f"--checkpoint_path {args.checkpoint_path!r}: no such file")
    model.load_state_dict(torch.load(args.checkpoint_path, weights_only=True))
    names = sorted(n for n in os.listdir(args.input_dir) if n.lower().endswith(IMAGE_SUFFIXES))
    if not names:
        raise SystemExit(f"--input_dir {args.input_dir!r} holds no image file ({', '.join(IMAGE_SUFFIXES)})")
    clash = same_stem(names)
    if clash:  # <stem>_mask.png of one would overwrite the other's
        raise SystemExit(f"--input_dir {args.input_dir!r}: files share a stem and would share their outputs: "
                         f"{', '.join(clash)}")
    os.makedirs(args.output_dir, exist_ok=True)
    pred = Predictor(model, args.image_size, device, tta=args.tta, tta_merge=args.tta_merge,
                     threshold=args.threshold,
                     pp=dict(keep_largest=args.pp_largest, min_area=args.pp_min_area, fill_holes=args.pp_fill_holes,
                             connectivity=args.pp_connectivity),
                     width=args.contour_width, alpha=args.overlay_alpha, bins=args.curve_bins,
                     lesion_table=args.lesion_table, lesion_echo=args.lesion_echo, echo_ring=args.echo_ring,
                     echo_levels=args.echo_levels)
    lines = [",".join(CSV_HEADER)]
    lesions = [",".join(lesion_csv_header(args.pixel_spacing, args.lesion_echo))]
    for start in range(0, len(names), args.batch_size):
        chunk = names[start:start + args.batch_size]
        planes = [decode_u8(Image.open(os.path.join(args.input_dir, n))) for n in chunk]
        out = pred(planes, return_scores=args.save_prob)
        lines += save_predictions(out, chunk, args.output_dir, save_scores=args.save_prob)
        if args.lesion_table:
            lesions += lesion_lines(out, chunk, args.pixel_spacing, args.pp_connectivity)
    with open(os.path.join(args.output_dir, "predictions.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.lesion_table:
        with open(os.path.join(args.output_dir, "lesions.csv"), "w") as f:
            f.write("\n".join(lesions) + "\n")
    print(f"[PREDICT] {len(names)} images -> {args.output_dir}")


def main(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.mode == "predict":
        e = predict_args_error(args, world)
        if e:
            raise SystemExit(e)
        from unet_hip import HipError
        try:
            return predict(args)
        except (HipError, ValueError) as e:
            raise SystemExit(f"--mode predict: {e}")
    if world > 1 and not torch.distributed.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        torch.distributed.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    set_seed(seed=42)
    rank = torch.distributed.get_rank() if world > 1 else 0
    if rank:
        # per-rank host augmentation streams (utils/transforms.py draws from random / numpy
        # in the main process when num_workers == 0): otherwise every shard would get rank 0's
        # Flip / Rotate / ... sequence.  torch's stream stays shared (identical model init;
        # parameters are broadcast from rank 0 anyway) and the mixup draws come from rank 0.
        random.seed(42 + rank)
        np.random.seed(42 + rank)
    stamp = [None]
    if world > 1:  # one experiments/<model>_<stamp>/ tree for the job: rank 0's
        stamp = [Config.make_stamp()] if rank == 0 else [None]
        torch.distributed.broadcast_object_list(stamp, src=0)
    config = Config(args, stamp=stamp[0])
    if torch.cuda.is_available():
        config.device = torch.device("cuda", torch.cuda.current_device())
    if rank == 0:
        logger = create_logger(os.path.join(config.log_dir, "train_log.log"))
    else:  # one writer of the shared log file (the Trainer also logs from rank 0 only)
        logger = logging.getLogger(f"unet_hip.rank{rank}")
        logger.addHandler(logging.NullHandler())
        logger.propagate = False
    if args.model_type not in ("UNet", "ModUNet", "ResUNet"):
        raise SystemExit(f"model_type {args.model_type!r}: the HIP path has UNet (models/model.py), "
                         "ModUNet and ResUNet (models/mod.py)")

    S = args.image_size
    args.gpu_augment = args.gpu_augment or args.gpu_augment_all
    gpu_tf = (args.gpu_transforms or args.gpu_augment) and not args.synthetic
    if args.synthetic:
        splits = [SyntheticSegmentation(args.synthetic, S, seed=s) for s in range(3)]
    else:
        # main.py:99-100: augmentations on the training split only
        tf = DecodeU8() if gpu_tf else Compose([Resize((S, S)), ToTensor()])
        if args.gpu_augment:
            train_tf = build_train_transform(config, (S, S),
                                             device_augment="all" if args.gpu_augment_all else True)
        else:
            train_tf = build_train_transform(config, (S, S), tail=[DecodeU8()] if gpu_tf else None)
        root = config.dataset_path
        splits = [MedicalDataset(os.path.join(root, d), os.path.join(root, d + "_mask"),
                                 train_tf if d == "train" else tf)
                  for d in ("train", "val", "test")]
    loaders = []
    for i, ds in enumerate(splits):
        kw = dict(batch_size=config.batch_size, num_workers=config.num_workers)
        if gpu_tf:
            kw["collate_fn"] = u8_collate
        if world > 1:
            # nn.DataParallel's split of every global batch (utils/trainer.py:28-30):
            # --batch_size stays the GLOBAL batch, as in the reference
            bs = DataParallelShardSampler(len(ds), config.batch_size, i != 1, rank, world, seed=42)
            # per-rank worker seeds (the sampler's shared order seed is separate): DataLoader
            # derives each worker's random / numpy / torch seeds from this generator
            dl = torch.utils.data.DataLoader(ds, batch_sampler=bs, num_workers=config.num_workers,
                                             collate_fn=dp_collate(u8_collate if gpu_tf else None),
                                             generator=torch.Generator().manual_seed(42 + rank))
        elif gpu_tf:
            dl = torch.utils.data.DataLoader(ds, shuffle=(i != 1), **kw)
        else:
            dl = create_dataloader(ds, config, shuffle=(i != 1))
        loaders.append(DeviceResizeLoader(dl, (S, S), config.device) if gpu_tf else dl)

    if args.use_amp_autocast:  # parsed and ignored, as before
        logger.info("--use_amp_autocast is ignored; the reduced-precision mode of this path is "
                    "--mfma bf16")
    model = build_model(args)
    if args.mfma != "fp32":  # a width the library refuses: its message now, no fallback
        from unet_hip.runtime import UNetRuntime
        try:
            UNetRuntime.get(config.device, *model._native_cfg())
        except Exception as e:
            raise SystemExit(f"--mfma {args.mfma} with {args.model_type}(base_filters="
                             f"{args.base_filters}, depth={args.depth}): {e}")
    if config.checkpoint_path and os.path.isfile(config.checkpoint_path):
        model.load_state_dict(torch.load(config.checkpoint_path, weights_only=True))
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    logger.info(f"Model: {config.model_type} | Trainable params: {n / 1e6:.2f}M ({n:,})")
    if rank == 0:
        print(f"[PARAMS] {config.model_type},{n}")

    trainer = Trainer(config, tuple(loaders), logger, model)
    if args.mode in ("train", "both"):
        trainer.train()
    if args.mode in ("test", "both"):
        if args.tta == "none":
            trainer.test()
        else:
            from unet_hip import HipError
            try:
                trainer.test()
            except (HipError, ValueError) as e:  # e.g. a rotated view of a non-square batch
                raise SystemExit(f"--tta {args.tta} --tta_merge {args.tta_merge}: {e}")


if __name__ == "__main__":
    main(get_parser())
