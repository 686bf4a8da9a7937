#!/usr/bin/env python3
"""Record what the REFERENCE's dataset_generation/Extract_TEyeD_NvGaze_AR_histo.py does with a made-up, seeded dataset.

    python tests/golden/make_golden_annot.py        # writes tests/golden/annot.npz

The script is driven as a program (runpy) in a temporary directory that holds one recording folder of frames and the four
annotation files.  It keeps every 202nd frame (its fix_interval) and opens only those, so the other frame files are empty.  OpenCV,
deepdish, scikit-image and scikit-learn are not installed: on top of _ref_shim's stubs, cv2.circle / ellipse / fillPoly record their
arguments and paint through tests/annot_refs.py (include/egne_hip.h states the rules), deepdish.io.save captures the Data dict,
scipy.io.savemat captures keydict, sklearn is inert.

The script as published does not run: it imports Circle_Fit, which helperfunctions does not define, and appends to
Data['Fits']['ball'], which generateEmptyStorage does not create.  The recorder supplies exactly these two things, a placeholder
attribute and an empty list (``supplied`` in the file says so); nothing else of the script is altered.

Pinned by the reference (``pinned_by_reference``): which frames are kept, the arguments of every cv2 call in call order, pupil_loc,
Fits, resolution, the paint values and the way Masks is cut out of Masks_noSkin.  NOT pinned (``pixels_from``): the pixels of the
circle, the ellipses and the polygon -- they come from the stand-ins.

Runs only where the reference is present; holds none of its text, and the file it writes holds data only.
"""
import contextlib
import io
import os
import runpy
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_shim  # noqa: E402
import annot_refs as R  # noqa: E402

INTERVAL = 202            # the script's fix_interval (2265127 // 11200)
CANDIDATES, SEED = 17, 20240521
REJECT = {2: ("ball", 0), 5: ("ball", 1), 9: ("iris", 2), 14: ("pupil", 1)}         # candidate -> (file, column of the row behind the frame number)


class Recorder:
    def __init__(self):
        self.order, self.circle, self.ellipse, self.poly = [], [], [], []

    def do_circle(self, img, center, radius, color, thickness):
        assert img.dtype == np.int8 and all(type(v) is int for v in (*center, radius)) and thickness == -1
        self.order.append("circle")
        self.circle.append((center[0], center[1], radius, color, thickness))
        img[R.circle_map(img.shape[0], img.shape[1], center[0], center[1], radius)] = color
        return img

    def do_ellipse(self, img, center, axes, angle, start, end, color, thickness):
        assert img.dtype == np.int8 and all(type(v) is int for v in (*center, *axes)) and (start, end, thickness) == (0, 360, -1)
        self.order.append("ellipse")
        self.ellipse.append((center[0], center[1], axes[0], axes[1], float(angle), start, end, color, thickness))
        t = np.radians(np.float64(angle))
        img[R.ellipse_map(img.shape[0], img.shape[1], center[0], center[1], axes[0], axes[1], np.cos(t), np.sin(t))] = color
        return img

    def do_fillPoly(self, img, pts, color):
        assert img.dtype == np.int8 and len(pts) == 1 and pts[0].shape == (34, 2) and pts[0].dtype.kind == "i"
        self.order.append("fillPoly")
        self.poly.append(np.asarray(pts[0], np.int64).copy())
        img[R.polygon_map(img.shape[0], img.shape[1], pts[0])] = color
        return img


def write_rows(path, rows):
    with open(path, "w") as f:
        f.write("FRAME;VALUES;\n")
        for r in rows:
            f.write(";".join(repr(float(v)) for v in r) + ";\n")


def main():
    from PIL import Image
    _ref_shim.install()
    warnings.simplefilter("ignore")
    rec, saved = Recorder(), {}
    cv2 = sys.modules["cv2"]
    cv2.circle, cv2.ellipse, cv2.fillPoly = rec.do_circle, rec.do_ellipse, rec.do_fillPoly
    for name in ("deepdish", "deepdish.io", "sklearn", "sklearn.cluster"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["deepdish"].io = sys.modules["deepdish.io"]
    sys.modules["deepdish.io"].save = lambda path, data: saved.__setitem__("Data", data)
    sys.modules["sklearn"].cluster = sys.modules["sklearn.cluster"]
    sys.modules["sklearn.cluster"].KMeans = object
    import scipy.io
    scipy.io.savemat = lambda path, d, **kw: saved.__setitem__("keydict", d)
    with contextlib.redirect_stdout(io.StringIO()):
        import helperfunctions as hf
    supplied = []
    if not hasattr(hf, "Circle_Fit"):
        hf.Circle_Fit = None
        supplied.append("helperfunctions.Circle_Fit = None (imported by the script, defined nowhere)")
    make_storage = hf.generateEmptyStorage

    def storage(*a, **k):
        data, keydict = make_storage(*a, **k)
        if "ball" not in data["Fits"]:
            data["Fits"]["ball"] = []
            supplied.append("Data['Fits']['ball'] = [] (appended to by the script, not created by generateEmptyStorage)")
        return data, keydict
    hf.generateEmptyStorage = storage

    # ---- the made-up dataset ------------------------------------------------------------------------------------------------------------
    ball, iris, pupil, lid = R.seeded_annotations(CANDIDATES, SEED)
    for k, (which, col) in REJECT.items():
        {"ball": ball, "iris": iris, "pupil": pupil}[which][k, col] = -1.5 - k
    frames = CANDIDATES * INTERVAL
    fr = np.arange(1, CANDIDATES + 1) * INTERVAL           # the script's fr_num of the candidates: the row it reads
    rows = frames + 2
    tab = {"eye_ball": np.zeros((rows, 4)), "iris_eli": np.zeros((rows, 6)), "pupil_eli": np.zeros((rows, 6)), "lid_lm_2D": np.zeros((rows, 70))}
    for t in tab.values():
        t[:, 0] = np.arange(rows)
    tab["eye_ball"][fr, 1:] = ball
    tab["iris_eli"][fr, 1:] = iris
    tab["pupil_eli"][fr, 1:] = pupil
    # landmarks: fields 2..35 step 2 hold the upper lid, fields 68..36 step -2 the lower lid, 34 points in the order the script reads them
    order = list(range(2, 35, 2)) + list(range(68, 35, -2))
    for k, i in enumerate(order):
        tab["lid_lm_2D"][fr, i] = lid[:, k, 0]
        tab["lid_lm_2D"][fr, i + 1] = lid[:, k, 1]
    rng = np.random.RandomState(SEED + 1)
    images = rng.randint(0, 256, (CANDIDATES, 480, 640)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        vid = os.path.join(tmp, "NvGaze-AR", "1")
        lab = os.path.join(tmp, "NvGaze-AR-ANNOTATIONS")
        for d in (vid, lab, os.path.join(tmp, "Histogram"), os.path.join(tmp, "Histogram_mat")):
            os.makedirs(d)
        for i in range(1, frames + 1):
            path = os.path.join(vid, "%06d.png" % i)
            if i % INTERVAL == 0:
                Image.fromarray(images[i // INTERVAL - 1]).save(path)
            else:
                open(path, "w").close()
        for name, t in tab.items():
            write_rows(os.path.join(lab, "NVIDIAAR_1_1.mp4%s.txt" % name), t)          # (behind the header line the script skips: its row j is t[j])
        argv, cwd = sys.argv, os.getcwd()
        sys.argv = ["Extract_TEyeD_NvGaze_AR_histo.py", "--path2ds", tmp, "--noDisp", "1"]
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                runpy.run_path(os.path.join(_ref_shim.REF, "dataset_generation", "Extract_TEyeD_NvGaze_AR_histo.py"), run_name="__main__")
        finally:
            sys.argv = argv
            os.chdir(cwd)
    Data, keydict = saved["Data"], saved["keydict"]
    kept = np.array([int(s) for s in Data["Info"]]) // INTERVAL - 1           # Info holds the script's running count
    n = len(kept)
    assert n >= 12 and sorted(set(range(CANDIDATES)) - set(kept.tolist())) == sorted(REJECT), kept
    assert rec.order == ["circle", "ellipse", "ellipse", "fillPoly"] * n
    assert np.array_equal(Data["Images"], images[kept])
    masks, noskin = np.asarray(Data["Masks"]), np.asarray(Data["Masks_noSkin"])
    assert masks.dtype == np.int8 and masks.shape == (n, 480, 640)
    full = [0, n - 1]
    arrs = {
        "pixels_from": np.array("tests/annot_refs.py, NOT OpenCV: the pixels of cv2.circle, cv2.ellipse and cv2.fillPoly (circle_map, "
                                "ellipse_map, polygon_map: the rules of include/egne_hip.h)"),
        "pinned_by_reference": np.array("kept (which candidate frames the script keeps), call_order, circle_args (cx, cy, r, colour, "
                                        "thickness), ellipse_args (cx, cy, ax, ay, angle, start, end, colour, thickness), fillpoly_pts, "
                                        "pupil_loc, Fits_pupil, Fits_iris, Fits_ball, resolution, and through the masks the paint values, "
                                        "the paint order and the cut of Masks out of Masks_noSkin"),
        "supplied": np.array(supplied),
        "interval": np.array(INTERVAL), "frame_rows": fr,
        "ann_ball": ball, "ann_iris": iris, "ann_pupil": pupil, "ann_lid": lid,
        "kept": kept, "info": np.array([str(s) for s in Data["Info"]]),
        "call_order": np.array(rec.order),
        "circle_args": np.array(rec.circle, np.int64), "ellipse_args": np.array(rec.ellipse, np.float64), "fillpoly_pts": np.stack(rec.poly),
        "pupil_loc": np.asarray(Data["pupil_loc"], np.float64), "keydict_pupil_loc": np.asarray(keydict["pupil_loc"], np.float64),
        "Fits_pupil": np.asarray(Data["Fits"]["pupil"], np.float64), "Fits_iris": np.asarray(Data["Fits"]["iris"], np.float64),
        "Fits_ball": np.asarray(Data["Fits"]["ball"], np.float64),
        "resolution": np.asarray(keydict["resolution"], np.int64), "archive": np.array([str(s) for s in keydict["archive"]]),
        "full": np.array(full), "Masks_full": masks[full], "Masks_noSkin_full": noskin[full],
        "Masks_sha": np.array(R.sha(masks)), "Masks_noSkin_sha": np.array(R.sha(noskin)),
    }
    path = os.path.join(HERE, "annot.npz")
    np.savez_compressed(path, **arrs)
    print("kept %d of %d candidates; %d cv2 calls; wrote %s %.1f KB" % (n, CANDIDATES, len(rec.order), path, os.path.getsize(path) / 1024))
    print("supplied:", supplied)


if __name__ == "__main__":
    main()
