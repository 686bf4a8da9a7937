"""Command-line flags of the entry scripts -- same names and defaults as the reference's args.py:30-65
(+ ``--synthetic`` because neither datasets nor checkpoints ship with the reference)."""
import argparse
from pprint import pprint

import torch


def parse_precision(prec):
    """args.py:17-28: 64 silently maps to float32."""
    if prec in (32, 64):
        return torch.float32
    if prec == 16:
        return torch.float16
    print('Invalid precision. Reverting to float32.')
    return torch.float32


# (flag, type, default, help).  Names and defaults are the drop-in surface (reference args.py:30-65); the table form, the
# grouping and the help texts are this repo's.
_TRAINING = (
    ("lr", float, 5e-4, "Adam step size (train.py)"),
    ("epochs", int, 40, "upper bound on training epochs"),
    ("batchsize", int, 12, "frames per optimiser step and per rank"),
    ("workers", int, 0, "DataLoader worker processes"),
    ("overfit", int, 0, "N > 0: stop every epoch after N batches"),
    ("resume", int, 0, "1: continue from --loadfile"),
    ("selfCorr", int, 0, "1: add 10 * the self-consistency term to the loss (loss.py:187-219: the ellipses of elPred rasterised into soft masks "
                          "and held against the softmax; forward and backward on the device; off in the reference pipeline)"),
    ("disentangle", int, 1, "dataset-identity confusion loss on the latent"),
    ("track_scores", int, 0, "1: the per-batch scores of the reference's training loop (per-class IoU, centre and angular distances, axis "
                             "scale ratios; train.py:289-338) for the training and the validation set, computed on the device behind every "
                             "step (egne_amd.scores: two small launches, no copy of a map, nothing synchronises); per epoch 'Train IoU' is "
                             "printed and one JSON line goes to logs/<model>/<expname>/scores.jsonl under the reference's TensorBoard tags"),
)
_MODEL = (
    ("model", str, "ritnet_v2", "key into modelSummary.model_dict"),
    ("setting", str, "error", "path of the yaml with the 10 model switches (configs/*.yaml)"),
    ("prec", int, 32, "16 | 32 | 64 (64 maps to float32, as in the reference)"),
    ("edge_thres", int, 0, "1: binarise the edge map at 0.1 before it enters the network"),
    ("loadfile", str, "./weights/all.git_ok", "checkpoint to load"),
)
_DATA = (
    ("curObj", str, None, "name of the pickled curriculum object (cond_<name>.pkl)"),
    ("path2data", str, "/media/rakshit/Monster", "dataset root"),
    ("test_mode", str, "leaveoneout", "evaluation split strategy"),
    ("synthetic", int, 0, "N > 0: run on N synthetic TEyeD-shaped frames (no dataset / checkpoint needed)"),
    ("pipeline", int, 1, "1 (default): the frozen edge network of a batch on a second HIP stream next to the previous batch's training "
                         "step (egne_amd.pipeline; the logged loss is then the previous batch's); 0: back to back, with the reference's "
                         "per-stage timers"),
    ("device_prep", int, 0, "1: distance maps computed from the labels on the GPU (egne_amd.dataprep) instead of taken "
                            "from the Dataset (CurriculumLib.py:131-136); 2: the boundary weights of CurriculumLib.py:128-129 too "
                            "(parity unpinned: restated from OpenCV's published Canny / dilate); 3: pupil_center, elNorm and cond "
                            "too, from the reference's ElliFit + RANSAC on the label's boundaries (egne_amd.dataprep.ellipse_targets): "
                            "(image, label) pairs are then enough"),
    ("device_loader", int, 0, "1: the Dataset hands out RAW samples (uint8 image, stored label, ellipses) and every batch is prepared on "
                              "the GPU (egne_amd.loader.device_batch: pad, augmentation -- training only --, label remap, z-score, "
                              "weights, distance maps, ellipse normalisation); --synthetic N then uses SyntheticRawEyes, otherwise "
                              "--raw_archive names the data"),
    ("raw_archive", str, None, "with --device_loader 1: an .npz with the arrays of the reference's H5 archives (Images, Masks_noSkin, "
                               "pupil_loc, Fits_pupil, Fits_iris; egne_amd.loader.RawArchive), or one that holds the TEyeD annotations "
                               "instead of masks (ann_ball, ann_iris, ann_pupil, ann_lid; egne_amd.loader.AnnotationArchive: the labels "
                               "are then painted on the GPU per batch).  python -m egne_amd.make_archive writes either kind"),
    ("loader_size", str, "240x320", "with --device_loader 1: pad2Size's canvas ROWSxCOLUMNS (the reference trains its 480x640 archives "
                                    "with 480x640 and --loader_scale 0.5)"),
    ("loader_scale", float, 0.0, "with --device_loader 1: scaleFn's factor behind the pad (0: none)"),
)
_OUTPUT = (
    ("expname", str, "dev", "sub-directory of logs/<model>/"),
    ("disp", int, 0, "1: prediction overlay grids drawn on the device (egne_amd.dispgrid, the reference's generateImageGrid: the frame "
                     "histogram-equalised, the predicted classes painted in, the predicted ellipses outlined).  test.py writes the grid "
                     "of the first four frames of every batch to img/<curObj or 'synthetic'>_<method>_disp/batch_%%05d.jpg; train.py "
                     "writes the grid of every epoch's last training batch (the reference's train/op image) to "
                     "logs/<model>/<expname>/disp/epoch_%%03d.jpg, rank 0 only.  Nothing is drawn per training batch: there is no "
                     "window to show it in"),
    ("test_save_op_masks", int, 0, "1: write predicted masks"),
    ("record_iou", int, 0, "1 (test.py, needs --device_metrics 1): write the per-sample IoUs [N,3] to img/<curObj>_<method>_ious.pkl"),
    ("device_metrics", int, 0, "1 (test.py): IoU and centre distances from the class map and the labels on the device (egne_amd.scores) "
                               "instead of host copies of both maps per batch; the same prints and return values, bit for bit"),
    ("ellipse_metrics", int, 0, "1 (test.py, needs --device_metrics 1): score the ellipses of elPred against elNorm on the device "
                                "(egne_amd.scores.EllipseLedger): the reference's bounding-box IoU and absolute parameter errors "
                                "(test.py:108-155, off in its source), the IoU of the ellipses themselves and of either against the class "
                                "map; with --record_iou 1 the per-sample rows go to img/<curObj>_<method>_ellipses.pkl"),
    ("ellipse_search", int, 0, "1 (test.py, needs --ellipse_metrics 1): score the ellipses after the search against the predicted class "
                               "map (the reference's search_flag) instead of the regressed ones"),
    ("record_img", int, 0, None),
    ("iou_filename", str, "test.pkl", None),
    ("visual_dir", str, "iris", None),
    ("method", str, "baseline", None),
    ("test_normal", int, 0, None),
    ("id", int, 0, None),
)


def build_parser():
    p = argparse.ArgumentParser(description="entry scripts of the MI355X hot path (test.py / train.py / evaluate.py)")
    for title, table in (("training", _TRAINING), ("model", _MODEL), ("data", _DATA), ("output", _OUTPUT)):
        grp = p.add_argument_group(title)
        for name, typ, default, text in table:
            grp.add_argument("--" + name, type=typ, default=default, help=text)
    return p


def ellipse_metrics_note(args):
    """What test.py says when the ellipse flags ask for something their prerequisites do not give (it then does without), or None."""
    if getattr(args, "ellipse_metrics", 0) and not getattr(args, "device_metrics", 0):
        return '--ellipse_metrics 1 needs --device_metrics 1: the ellipse scores are rows of a device ledger; nothing is scored'
    if getattr(args, "ellipse_search", 0) and not getattr(args, "ellipse_metrics", 0):
        return '--ellipse_search 1 needs --ellipse_metrics 1: without it no ellipse is scored; nothing is searched'
    return None


def loader_geometry(args):
    """(size, scale) of loader.device_batch from --loader_size / --loader_scale."""
    try:
        r, c = (int(v) for v in str(getattr(args, "loader_size", "240x320")).lower().split("x"))
    except ValueError:
        raise SystemExit('--loader_size must be ROWSxCOLUMNS, e.g. 480x640')
    return (r, c), (float(getattr(args, "loader_scale", 0.0)) or False)


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    loader_geometry(args)
    if args.device_loader and not args.synthetic and not args.raw_archive:
        raise SystemExit('--device_loader 1 needs --raw_archive PATH (or --synthetic N)')
    if args.curObj is None and not args.synthetic and not (args.device_loader and args.raw_archive):
        raise SystemExit('--curObj is required (or use --synthetic N)')
    print('------')
    print('parsed arguments:')
    pprint(vars(args))
    args.prec = parse_precision(args.prec)
    return args
