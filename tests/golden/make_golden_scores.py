#!/usr/bin/env python3
"""Record the REFERENCE's own scores on the seeded cases of tests/scores_refs.py.

    python tests/golden/make_golden_scores.py        # writes tests/golden/scores.npz

Runs only where the reference is present (and scikit-learn, which its utils.py goes through); holds none of its text, and the file
it writes holds outputs only.

  seg_<case>_{miou,perclass,scorelist}   utils.getSeg_metrics on the label / prediction / cond of scores_refs.seg_case
  ang_{mean,dist}_<k>                    utils.getAng_metric on float32 elNorm[:, k, 4] / elOut[:, 4 or 9] under cond[:, 1]
  pt_{mean,dist}_<which>                 utils.getPoint_metric(..., do_unnorm=True) on the float32 centres

The scale ratios are lines of the reference's train.py, not a function: nothing here can call them, and nothing is recorded.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (installs the shim, imports the reference's modules)
import scores_refs as R  # noqa: E402


def main():
    U = MG.REF["utils"]
    arrs = {}
    for name in R.SEG_CASES:
        yt, yp, cond = R.seg_case(name)
        miou, per, sl = U.getSeg_metrics(yt, yp, cond)
        arrs["seg_%s_miou" % name], arrs["seg_%s_perclass" % name], arrs["seg_%s_scorelist" % name] = np.float64(miou), np.asarray(per, np.float64), sl
        print("%-22s mIoU %r" % (name, miou))
    elOut, elPred, pc, ic, elNorm, cond = (t.numpy() for t in R.vec_inputs(R.VEC_B, R.VEC_SEED, R.VEC_HW))
    c = cond.astype(np.float32)
    for k, (name, col) in enumerate((("iris", 4), ("pupil", 9))):
        m, d = U.getAng_metric(elNorm[:, k, 4], elOut[:, col], c[:, 1])
        arrs["ang_mean_" + name], arrs["ang_dist_" + name] = np.float64(m), d
    for which, gt, pred, fc in (("pupil_latent", pc, elOut[:, 5:7], 0), ("pupil_seg", pc, elPred[:, 5:7], 0),
                                ("iris_latent", ic, elOut[:, 0:2], 1), ("iris_seg", ic, elPred[:, 0:2], 1)):
        m, d = U.getPoint_metric(gt, pred.copy(), c[:, fc], R.VEC_HW, True)
        arrs["pt_mean_" + which], arrs["pt_dist_" + which] = np.float64(m), np.asarray(d, np.float64)
    path = os.path.join(HERE, "scores.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
