#!/usr/bin/env python3
"""Record what the REFERENCE's ellipse block of test.py (:108-155, :240-247, behind bbox_iou_flag) computes on the seeded cases of
tests/ellipse_scores_refs.py.

    python tests/golden/make_golden_ellipse_scores.py        # writes tests/golden/ellipse_scores.npz

OpenCV is not installed, so the stub ``cv2`` module of _ref_shim gets recording stand-ins for fillPoly, bitwise_and and bitwise_or;
the stand-in for fillPoly fills by the closed-quadrilateral rule of tests/ellipse_scores_refs.py (include/egne_hip.h states it).  The
reference's own program text then runs: my_ellipse(...).transform(H), calc_bbox and calc_ell_bbox_iou (calc_box_iou.py),
search_proper_parameter_iou and calc_ell_iou (utils.py); the loop around them and the reductions are re-enacted here line for line
over the recorded per-sample values.

Pinned by the reference (``pinned_by_reference`` in the file): the integer corners handed to fillPoly, the pixel and the searched
ellipses, the parameter differences, the reductions, the calc_ell_iou scores.  NOT pinned (``pixels_from``): which pixels a box
covers -- the counts and box IoUs in the file come from the restated fill, not from OpenCV.

Two things to know about the cases:
  * every ellipse is drawn again while a float64 corner coordinate of its box lies within 1e-6 of an integer, or a pixel's wtMat
    within 1e-9 of zero (ellipse_scores_refs.inputs; checked again here for the searched ellipses): device and host cos / sin differ
    in the last place there, and the truncation to int32 would turn that into a whole pixel;
  * the float32 vectors are widened to float64 BEFORE my_ellipse sees them, which is what egne_ellipse_init_from_pred does; handed
    float32 arrays, the reference's param2mat rounds 1 / a ** 2 and the rotation's cos / sin to float32 (a difference of about 1e-5
    relative, tests/test_gpu_batch.py), and that is not reproduced.
calc_bbox_iou always draws on its default 240 x 320 canvas; ``<case>_canvas`` records it, and for a case of another frame size the box
counts in the file are those of that canvas.

Runs only where the reference is present; holds none of its text, and the file it writes holds data only.
"""
import contextlib
import hashlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_shim  # noqa: E402
import ellipse_scores_refs as R  # noqa: E402


class Recorder:
    """cv2.fillPoly / bitwise_and / bitwise_or: what the reference hands over, filled by the restated rule."""

    def __init__(self):
        self.boxes, self.shapes = [], []

    def fillPoly(self, im, pts, colour):
        pts = np.asarray(pts)
        assert pts.dtype == np.int32 and pts.shape == (1, 4, 2) and colour == 255 and im.dtype == np.uint8
        self.boxes.append(pts.reshape(8).copy())
        self.shapes.append(im.shape)
        im[R.quad_fill(pts.reshape(8), *im.shape)] = 255
        return im

    @staticmethod
    def bitwise_and(a, b):
        return a & b

    @staticmethod
    def bitwise_or(a, b):
        return a | b

    def take(self):
        (a, b), shapes = self.boxes, self.shapes
        assert shapes[0] == shapes[1]
        self.boxes, self.shapes = [], []
        return a, b, shapes[0]


def main():
    _ref_shim.install()
    rec = Recorder()
    cv2 = sys.modules["cv2"]
    cv2.fillPoly, cv2.bitwise_and, cv2.bitwise_or = rec.fillPoly, rec.bitwise_and, rec.bitwise_or
    with contextlib.redirect_stdout(io.StringIO()):
        import calc_box_iou as CB
        import helperfunctions as HF
        import utils as U
    arrs = {"pixels_from": np.array("tests/ellipse_scores_refs.py quad_fill (the closed-quadrilateral rule, NOT cv2.fillPoly): "
                                    "box_iou, box_and, box_or and their _search forms, and the reductions over them"),
            "pinned_by_reference": np.array("l_pred, l_gt, l_search, corners_pred, corners_gt, corners_search, para, para_search, "
                                            "ell_iou, ell_iou_search, map_iou_pred, map_iou_gt, map_iou_search, and the reductions "
                                            "bbiou_batches, bbiou, para_mean (and _search) given the per-sample values")}
    warnings.simplefilter("ignore", category=RuntimeWarning)
    for name, (H, W, N, B, seed) in R.FIXTURE_CASES.items():
        inp = R.fixture_inputs(name)
        mask, elPred, elNorm = torch.from_numpy(inp["mask"]), inp["elPred"], inp["elNorm"]
        Hm = np.array([[W / 2, 0, W / 2], [0, H / 2, H / 2], [0, 0, 1]])
        mesh = U.create_meshgrid(H, W, normalized_coordinates=True)
        per = {k: [] for k in ("l_pred", "l_gt", "l_search", "corners_pred", "corners_gt", "corners_search", "box_iou", "box_and", "box_or",
                               "box_iou_search", "box_and_search", "box_or_search", "para", "para_search", "ell_iou", "ell_iou_search",
                               "map_iou_pred", "map_iou_gt", "map_iou_search")}
        canvas = None

        def ell_iou(seg, l):
            el = np.array([l[0], l[1], l[2], l[3], l[4] * 180. / 3.14159])      # (calc_ell_iou turns the angle back in place)
            return U.calc_ell_iou(seg, el, mesh, False, True)

        def counts(a, b, shape):
            fa, fb = R.quad_fill(a, *shape), R.quad_fill(b, *shape)
            return int(np.count_nonzero(fa & fb)), int(np.count_nonzero(fa | fb))
        bb = {False: [], True: []}          # test.py:70-71 bbiou_iris / bbiou_pupil as [iris, pupil] per batch, without and with the search
        for b0 in range(0, N, B):
            for search in (False, True):
                acc = [0, 0]                # test.py:110-111
                for i in range(b0, b0 + B):
                    row = {k: [] for k in per}
                    for k in (0, 1):        # iris, pupil: test.py:117-121 (on the widened vectors, see above)
                        l = HF.my_ellipse(elPred[i, 5 * k:5 * k + 5].astype(np.float64)).transform(Hm)[0]
                        l_gt = HF.my_ellipse(elNorm[i, k].astype(np.float64)).transform(Hm)[0]
                        seg = mask[i] == 1 + k
                        if not search:      # test.py:122-126
                            iou = CB.calc_ell_bbox_iou(l[:5], l_gt[:5])
                            ca, cb, shape = rec.take()
                            assert not R.near_integer(l) and not R.near_integer(l_gt), (name, i, k)
                            n_and, n_or = counts(ca, cb, shape)
                            assert (np.isnan(iou) and n_or == 0) or iou == n_and / n_or
                            row["l_pred"].append(l[:5]); row["l_gt"].append(l_gt[:5])
                            row["corners_pred"].append(ca); row["corners_gt"].append(cb)
                            row["box_iou"].append(iou); row["box_and"].append(n_and); row["box_or"].append(n_or)
                            row["para"].append(abs(np.array(l[:5]) - np.array(l_gt[:5])))
                            gmap = torch.from_numpy(R.ell_map(H, W, l_gt[:5]))      # the restated ground-truth ellipse map
                            row["ell_iou"].append(ell_iou(gmap, l))
                            row["map_iou_pred"].append(ell_iou(seg, l)); row["map_iou_gt"].append(ell_iou(seg, l_gt))
                        else:               # test.py:127-141
                            iou, new = U.search_proper_parameter_iou(seg, elPred[i, 5 * k:5 * k + 5].copy(), elNorm[i, k].copy(), l, l_gt)
                            ca, cb, shape = rec.take()
                            assert not R.near_integer(new), (name, i, k, "searched: change the case's seed")
                            assert not np.any(np.abs(R.membership_margin(H, W, new)) < R.NEAR_ZERO), (name, i, k)
                            n_and, n_or = counts(ca, cb, shape)
                            row["l_search"].append(new[:5]); row["corners_search"].append(ca)
                            row["box_iou_search"].append(iou); row["box_and_search"].append(n_and); row["box_or_search"].append(n_or)
                            row["para_search"].append(abs(np.array(new) - np.array(l_gt[:5])))
                            gmap = torch.from_numpy(R.ell_map(H, W, l_gt[:5]))
                            row["ell_iou_search"].append(ell_iou(gmap, new)); row["map_iou_search"].append(ell_iou(seg, new))
                        assert canvas in (None, shape)
                        canvas = shape
                        acc[k] += iou
                    for key, v in row.items():
                        if v:
                            per[key].append(np.array(v))
                bb[search].append([acc[0] / B, acc[1] / B])         # test.py:151-155
        p = name + "_"
        for key, v in per.items():
            arrs[p + key] = np.stack(v)
        arrs[p + "canvas"] = np.array(canvas)
        arrs[p + "mask_sha"] = np.array(hashlib.sha256(inp["mask"].tobytes()).hexdigest())
        for key in ("elPred", "elNorm", "cond"):
            arrs[p + key] = inp[key]
        for search, sfx in ((False, ""), (True, "_search")):
            arrs[p + "bbiou_batches" + sfx] = np.array(bb[search], np.float64)
            arrs[p + "bbiou" + sfx] = np.array([np.nanmean([b[k] for b in bb[search]]) for k in (0, 1)])      # test.py:240-241
            pm = []
            for k in (0, 1):                # test.py:242-245
                m = np.nanmean([q[k] for q in per["para" + sfx]], 0)
                m[4] *= 180.0 / 3.1415
                pm.append(m)
            arrs[p + "para_mean" + sfx] = np.stack(pm)
        print("%s: %dx%d, %d samples in batches of %d: bbiou %s, searched %s" % (name, H, W, N, B, arrs[p + "bbiou"], arrs[p + "bbiou_search"]))
    path = os.path.join(HERE, "ellipse_scores.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
