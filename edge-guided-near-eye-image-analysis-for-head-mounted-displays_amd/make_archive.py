"""Prepare data: frames plus TEyeD annotation files -> an archive that train.py / test.py --device_loader 1 --raw_archive consume.

    python -m egne_amd.make_archive --frames VIDEO.avi|DIR --annotations PREFIX --out X.npz [--every N] [--max_frames M]
                                    [--row_offset 0|1] [--canvas RxC] [--store masks|annotations] [--batch 64]

The job of the reference's dataset_generation/Extract_TEyeD_{LPW,NvGaze_AR}_histo.py, without their H5 / deepdish output:

    frames        a Motion-JPEG .avi (mjpeg.mjpeg_frames; any other codec is refused: TEyeD's H.264 .mp4 files cannot be decoded
                  here and have to be transcoded or extracted first), or a directory of images read through PIL .convert('L') in the
                  order of their sorted names, as the NvGaze script reads them
    annotations   PREFIXiris_eli.txt, PREFIXpupil_eli.txt, PREFIXeye_ball.txt, PREFIXlid_lm_2D.txt: ';'-separated floats, the first
                  line skipped, a trailing ';' tolerated.  Frame k (from 0) reads row k (--row_offset 0, the LPW script) or row k + 1
                  (--row_offset 1, the NvGaze script).  The lid is fields 2..35 step 2 (upper), then 68..36 step -2 (lower): 34 points
    selection     every --every-th frame by the scripts' 1-based running count (count % every == 0), then dataprep.annotation_keep
    --store masks        the label maps are rasterised on the device in batches (dataprep.labels_from_annotations) and the archive holds
                         Images, Masks, Masks_noSkin, pupil_loc, Fits_pupil, Fits_iris, Fits_ball, Info, resolution: loader.RawArchive
    --store annotations  the archive holds Images, ann_ball, ann_iris, ann_pupil, ann_lid, Info, resolution: loader.AnnotationArchive,
                         whose labels are painted on the device per batch

The pixels of the maps are this project's rules (include/egne_hip.h), not OpenCV's: the arguments of the reference's cv2 calls are
pinned (tests/golden/annot.npz), their boundary pixels are not.  Out of scope: the Fuhl script, which resizes the image without
touching the annotation; stratified splits (CurriculumLib.py).
"""
import argparse
import os

import numpy as np

LID_FIELDS = list(range(2, 35, 2)) + list(range(68, 35, -2))          # the x fields of the 34 landmarks, in the scripts' order


def read_rows(path):
    """The rows of an annotation file as float64 [rows, fields]: the first line skipped, empty fields (a trailing ';') dropped."""
    rows = []
    with open(path, "r") as f:
        for k, line in enumerate(f):
            if k == 0:
                continue
            vals = [float(v) for v in line.split(";") if v.strip()]
            if vals:
                rows.append(vals)
    width = {len(r) for r in rows}
    if len(width) > 1:
        raise SystemExit("make_archive: %s has rows of %s fields" % (path, sorted(width)))
    return np.array(rows, np.float64).reshape(len(rows), -1)


def read_annotations(prefix):
    """(ball [N,3], iris [N,5], pupil [N,5], lid [N,34,2]) float64 from the four files behind ``prefix``."""
    tabs = {}
    for name, fields in (("eye_ball", 4), ("iris_eli", 6), ("pupil_eli", 6), ("lid_lm_2D", 70)):
        path = prefix + name + ".txt"
        if not os.path.exists(path):
            raise SystemExit("make_archive: annotation file %s is missing" % path)
        tabs[name] = read_rows(path)
        if tabs[name].shape[1] < fields:
            raise SystemExit("make_archive: %s has %d fields per row, %d are needed" % (path, tabs[name].shape[1], fields))
    n = min(len(t) for t in tabs.values())
    lm = tabs["lid_lm_2D"][:n]
    lid = np.stack([lm[:, LID_FIELDS], lm[:, [i + 1 for i in LID_FIELDS]]], axis=2)
    return tabs["eye_ball"][:n, 1:4], tabs["iris_eli"][:n, 1:6], tabs["pupil_eli"][:n, 1:6], lid


def avi_codec(path):
    """The fourcc of the first video stream of a RIFF AVI file (upper case), or None when the file is no AVI."""
    with open(path, "rb") as f:
        head = f.read(1 << 16)
    if head[:4] != b"RIFF" or head[8:12] != b"AVI ":
        return None
    at = head.find(b"strh")
    if at < 0 or head[at + 8:at + 12] != b"vids":
        return None
    return head[at + 12:at + 16].upper()


def iter_frames(path):
    """Grey uint8 frames of ``path`` in order."""
    if os.path.isdir(path):
        from PIL import Image
        for name in sorted(os.listdir(path)):
            yield lambda name=name: np.asarray(Image.open(os.path.join(path, name)).convert("L"))
        return
    codec = avi_codec(path)
    if codec != b"MJPG":
        raise SystemExit("make_archive: %s is not a Motion-JPEG .avi (%s): only Motion-JPEG can be decoded here; transcode the video to "
                         "MJPEG or extract its frames into a directory" % (path, "codec %r" % codec.decode("latin1") if codec else "no AVI video stream"))
    from .mjpeg import mjpeg_frames
    for frame in mjpeg_frames(path):
        yield lambda frame=frame: frame


def parse_size(text, what):
    try:
        r, c = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise SystemExit("make_archive: %s must be ROWSxCOLUMNS, not %r" % (what, text))
    return r, c


def build_parser():
    p = argparse.ArgumentParser(prog="python -m egne_amd.make_archive", description=__doc__.split("\n\n")[0])
    p.add_argument("--frames", required=True, help="a Motion-JPEG .avi or a directory of images")
    p.add_argument("--annotations", required=True, help="prefix of the four TEyeD annotation files")
    p.add_argument("--out", required=True, help="the .npz to write")
    p.add_argument("--every", type=int, default=1, help="keep every N-th frame (1-based running count % N == 0)")
    p.add_argument("--max_frames", type=int, default=0, help="stop after M kept frames (0: no limit)")
    p.add_argument("--row_offset", type=int, default=0, choices=(0, 1), help="frame k reads annotation row k (LPW) or k + 1 (NvGaze)")
    p.add_argument("--canvas", default=None, help="ROWSxCOLUMNS of the label maps (default: the frames' size; the reference's scripts use "
                                                  "480x640).  Frames of another size are refused: an archive holds maps of its frames' size")
    p.add_argument("--store", default="masks", choices=("masks", "annotations"))
    p.add_argument("--batch", type=int, default=64, help="frames rasterised per launch (--store masks)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.every < 1 or args.batch < 1:
        raise SystemExit("make_archive: --every and --batch must be positive")
    from . import dataprep
    ball, iris, pupil, lid = read_annotations(args.annotations)
    keep = dataprep.annotation_keep(ball, iris, pupil)
    canvas = parse_size(args.canvas, "--canvas") if args.canvas else None
    images, rows, info = [], [], []
    for k, load in enumerate(iter_frames(args.frames)):
        count, row = k + 1, k + args.row_offset
        if args.max_frames and len(images) == args.max_frames:
            break
        if count % args.every != 0:
            continue
        if row >= len(keep):
            raise SystemExit("make_archive: frame %d needs annotation row %d, the files hold %d" % (k, row, len(keep)))
        if not keep[row]:
            continue
        frame = np.ascontiguousarray(load(), dtype=np.uint8)
        canvas = canvas or frame.shape
        if frame.shape != tuple(canvas):
            raise SystemExit("make_archive: frame %d is %dx%d, the label maps are %dx%d" % (k, frame.shape[0], frame.shape[1], canvas[0], canvas[1]))
        images.append(frame)
        rows.append(row)
        info.append(str(count))
    if not images:
        raise SystemExit("make_archive: no frame was kept")
    rows = np.array(rows)
    ball, iris, pupil, lid = ball[rows], iris[rows], pupil[rows], lid[rows]
    out = {"Images": np.stack(images), "Info": np.array(info), "resolution": np.array([im.shape for im in images], np.int64)}
    if args.store == "annotations":
        dataprep.pack_annotations(ball, iris, pupil, lid)          # (refuses what the loader would refuse, now)
        out.update(ann_ball=ball, ann_iris=iris, ann_pupil=pupil, ann_lid=lid)
    else:
        import torch
        records = dataprep.pack_annotations(ball, iris, pupil, lid)
        n = len(records)
        noskin, skin = np.zeros((n,) + tuple(canvas), np.int8), np.zeros((n,) + tuple(canvas), np.int8)
        status = np.zeros(n, np.int32)
        for a in range(0, n, args.batch):
            (m0, m1), st = dataprep.labels_from_annotations(records[a:a + args.batch], canvas, with_skin=True, return_status=True)
            noskin[a:a + args.batch], skin[a:a + args.batch], status[a:a + args.batch] = m0.cpu().numpy(), m1.cpu().numpy(), st.cpu().numpy()
        torch.cuda.synchronize()
        flat = int(np.count_nonzero(status & (dataprep.ANNOT_IRIS_ZERO_AXIS | dataprep.ANNOT_PUPIL_ZERO_AXIS)))
        if flat:
            print("make_archive: %d frames hold an ellipse with a zero half-axis: nothing is painted for it (OpenCV would draw a segment)" % flat)
        pupil_loc, fits_pupil, fits_iris = dataprep.annotation_fits(iris, pupil)
        fits_ball = np.stack([ball[:, 1], ball[:, 2], ball[:, 0], ball[:, 0], np.zeros(n)], axis=1)
        out.update(Masks=skin, Masks_noSkin=noskin, pupil_loc=pupil_loc, Fits_pupil=fits_pupil, Fits_iris=fits_iris, Fits_ball=fits_ball)
    np.savez_compressed(args.out, **out)
    print("make_archive: %d frames of %dx%d -> %s (%s)" % (len(images), canvas[0], canvas[1], args.out, args.store))
    return out


if __name__ == "__main__":
    main()
