#!/usr/bin/env python3
"""Record the REFERENCE's item path (CurriculumLib.DataLoader_riteyes.__getitem__) on raw samples, augmentation off.

    python tests/golden/make_golden_loader.py        # writes tests/golden/loader.npz

Runs only where the reference is present; holds none of its text.  The reference's own __getitem__ (with pad2Size, scaleFn,
get_ellipse_info and one_hot2dist behind it) is driven on the samples of tests/loader_refs.py with ``readImage`` patched to hand them
out.  h5py is not installed (an empty stand-in module lets CurriculumLib import; readImage is the only user), and neither is OpenCV:
cv2.Canny, cv2.dilate and cv2.resize are the RECORDING stand-ins of loader_refs.Cv2Recorder, which keep the arguments the reference
hands them and answer with this project's restatements.  So the fixture pins, from the reference itself: the order of operations,
padding, label remap, distance maps, z-score, all the centre / ellipse geometry, cond, imInfo, dtypes, and every argument of the
three OpenCV calls; the PIXELS those calls return (spatial weights, the resized image and label) are restatement-derived, not
OpenCV's (``pixels_from`` in the file says so).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_shim  # noqa: E402
import loader_refs as R  # noqa: E402


def main():
    _ref_shim.install()
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    rec = R.Cv2Recorder()
    cv2 = sys.modules["cv2"]
    cv2.Canny, cv2.dilate, cv2.resize = rec.Canny, rec.dilate, rec.resize
    cv2.INTER_LANCZOS4, cv2.INTER_NEAREST = R.INTER_LANCZOS4, R.INTER_NEAREST
    with contextlib.redirect_stdout(io.StringIO()):
        import CurriculumLib as REF
    arrs = {"pixels_from": np.array("tests/loader_refs.py Cv2Recorder (restatements of OpenCV's documented behaviour, NOT OpenCV): "
                                    "spatWts, and img / label / distMap of the scaled group"),
            "pinned_by_reference": np.array("everything else, the arguments of cv2.Canny / dilate / resize (calls) included")}
    for group, cases, size, scale in (("p", R.CASES_PLAIN, R.SIZE_PLAIN, False), ("s", R.CASES_SCALED, R.SIZE_SCALED, R.SCALE)):
        ds = object.__new__(REF.DataLoader_riteyes)
        ds.scale, ds.augFlag, ds.size = scale, False, size
        import torch
        ds.prec = torch.float32
        for n, case in enumerate(cases):
            sample = R.raw_case(*case)
            img, mask, el, pc, cond, info = (a.copy() for a in sample)
            ds.readImage = lambda idx, s=(img, mask, [el[0], el[1]], pc, cond, info): s
            rec.calls = []
            out = ds[0]
            p = "%s%d_" % (group, n)
            for name, t in zip(R.OUTPUTS, out):
                arrs[p + name] = t.numpy()
                arrs[p + name + "_dtype"] = np.array(str(t.dtype))
            arrs[p + "calls"] = np.array(rec.calls)
            for name, a in zip(("raw_img", "raw_label", "raw_el", "raw_pc", "raw_cond", "raw_info"), sample):
                arrs[p + name] = a
    path = os.path.join(HERE, "loader.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
