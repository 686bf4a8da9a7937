"""CPU: the restatement of the score rows (tests/scores_refs.py, the reference of tests/test_gpu_scores.py) and the host reductions
of egne_amd.scores against what the REFERENCE's own utils.getSeg_metrics / getAng_metric / getPoint_metric gave on the same seeded
inputs (tests/golden/scores.npz, written by tests/golden/make_golden_scores.py).

Bounds: the IoU rows and the angular distances are integer counts, one float64 division, and float32 operations the reference performs
in the same order -- they must be EQUAL, NaNs in the same places.  The reference's getPoint_metric goes through scikit-learn's
expanded-square pairwise distances and is not bit-comparable: rtol 1e-6, the bound tests/test_host_cpu.py::test_metrics_match_reference
holds the project's getPoint_metric to.  The scale ratios are not pinned by the reference (lines of a script, scores_refs' docstring)."""
import os

import numpy as np
import pytest
import torch

import scores_refs as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scores.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def vec():
    """The fixture's ellipse vectors with random maps: inputs and their rows, computed once and never modified."""
    elOut, elPred, pc, ic, elNorm, cond = R.vec_inputs(R.VEC_B, R.VEC_SEED, R.VEC_HW)
    yt, yp = R.maps(R.VEC_B, 6, 10, seed=5, stray=False)
    rows = R.rows_ref(yt, yp, elOut, elPred, pc, ic, elNorm, cond, hw=R.VEC_HW)
    return dict(elOut=elOut.numpy(), elPred=elPred.numpy(), pc=pc.numpy(), ic=ic.numpy(), elNorm=elNorm.numpy(), cond=cond.numpy(), rows=rows)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_module_surface():
    from egne_amd import _lib, scores
    from egne_amd.args import build_parser, _OUTPUT, _TRAINING
    assert "egne_seg_confusion_counts" in _lib.SIGNATURES and "egne_score_rows" in _lib.SIGNATURES
    assert (scores.FIELDS, scores.IOU, scores.COND1, scores.BATCH) == (R.FIELDS, R.IOU, R.COND1, R.BATCH)
    assert scores.DIST_PUPIL_LATENT == R.DIST and scores.ANG_IRIS == R.ANG and scores.SCALE_IRIS == R.SCALE
    assert any(f[0] == "device_metrics" and f[3] for f in _OUTPUT) and any(f[0] == "track_scores" and f[3] for f in _TRAINING)
    d = build_parser().parse_args(["--synthetic", "1"])
    assert d.device_metrics == 0 and d.track_scores == 0 and d.record_iou == 0
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egne_hip.h")).read()
    for name in ("IOU", "DIST_PUPIL_LATENT", "DIST_PUPIL_SEG", "DIST_IRIS_LATENT", "DIST_IRIS_SEG", "ANG_IRIS", "ANG_PUPIL", "SCALE_IRIS",
                 "SCALE_PUPIL", "COND0", "COND1", "LOSS", "BATCH", "SAMPLE", "FIELDS"):
        assert "#define EGNE_SCORE_%s %d\n" % (name, getattr(scores, name)) in hdr, name
    assert "#define EGNE_SCORES_CHUNK %d\n" % scores.CHUNK in hdr


@pytest.mark.parametrize("case", R.SEG_CASES)
def test_iou_rows_equal_the_reference(gold, case):
    from egne_amd import scores, utils
    yt, yp, cond = R.seg_case(case)
    want = gold["seg_%s_scorelist" % case]
    got = R.iou_ref(R.counts_ref(yt, yp), cond)
    assert _same(got, want), (got, want)
    rows = np.full((yt.shape[0], R.FIELDS), np.nan)
    rows[:, R.IOU:R.IOU + 3], rows[:, R.COND1] = got, cond
    miou, per, sl = scores.seg_metrics(rows)
    assert _same(miou, gold["seg_%s_miou" % case]) and _same(per, gold["seg_%s_perclass" % case]) and _same(sl, want)
    h = utils.getSeg_metrics(yt, yp, cond)          # the project's host function: the same triple, the same bits
    assert _same(h[0], miou) and _same(h[1], per) and _same(h[2], sl)


def test_cases_cover_what_they_name():
    """The seeded cases do contain what the issue lists: absent classes, a single-class frame, a predicted class the truth lacks."""
    yt, yp, _ = R.seg_case("all_present")
    assert all(set(np.unique(f)) == {0, 1, 2} for f in yt)
    yt, yp, _ = R.seg_case("no_pupil")
    assert 2 not in yt[1] and 2 in yp[1]
    yt, yp, _ = R.seg_case("one_class")
    assert set(np.unique(yt[0])) == {0} and set(np.unique(yt[2])) == {1}
    yt, yp, _ = R.seg_case("pred_has_extra_class")
    assert 2 not in yt[0] and 2 in yp[0] and 0 not in yt[3] and 0 in yp[3]
    assert [int(R.seg_case(n)[2].sum()) for n in ("cond_some", "cond_all", "cond_none")] == [2, 4, 0]


@pytest.mark.parametrize("which,k", [("iris", 0), ("pupil", 1)])
def test_angular_distances_equal_the_reference(gold, vec, which, k):
    from egne_amd import scores, utils
    m, d = scores.ang_metric(vec["rows"], which)
    assert _same(d, gold["ang_dist_" + which]) and _same(m, gold["ang_mean_" + which])
    h = utils.getAng_metric(vec["elNorm"][:, k, 4], vec["elOut"][:, (4, 9)[k]], vec["cond"][:, 1].astype(np.float32))
    assert _same(h[0], m) and _same(h[1], d)
    # the kernel multiplies by 180 / pi in float64: np.rad2deg's own constant
    x = vec["rows"][:, R.ANG + k] / (180.0 / np.pi)
    assert np.array_equal(np.rad2deg(x), x * (180.0 / 3.141592653589793238462643383279502884))


@pytest.mark.parametrize("which,gt,pred,cols,fc", [("pupil_latent", "pc", "elOut", (5, 7), 0), ("pupil_seg", "pc", "elPred", (5, 7), 0),
                                                    ("iris_latent", "ic", "elOut", (0, 2), 1), ("iris_seg", "ic", "elPred", (0, 2), 1)])
def test_centre_distances(gold, vec, which, gt, pred, cols, fc):
    from egne_amd import scores, utils
    m, d = scores.point_metric(vec["rows"], which, fc)
    # the project's host function on the same float32 arrays: the same bits
    h = utils.getPoint_metric(vec[gt], vec[pred][:, cols[0]:cols[1]], vec["cond"][:, fc].astype(np.float32), R.VEC_HW, True)
    assert _same(h[0], m) and _same(h[1], d)
    # the reference (scikit-learn's pairwise distances): rtol 1e-6
    np.testing.assert_allclose(m, gold["pt_mean_" + which], rtol=1e-6)
    np.testing.assert_allclose(d, gold["pt_dist_" + which], rtol=1e-6, atol=1e-9)


def test_scale_ratios_meet_zero_denominators(vec):
    r = vec["rows"]
    assert np.isposinf(r[0, R.SCALE]) and np.isnan(r[1, R.SCALE + 1]) and np.isfinite(r[2:, R.SCALE:R.SCALE + 2]).all()


def test_scale_ratios_against_the_script_in_torch(vec):
    """train.py:323-329 as written, in torch float32 on this host: inf and NaN in the same places, finite values within 2 float32 ulps
    of the IEEE restatement (torch's CPU square root is not correctly rounded and differs between hosts: scores_refs' docstring)."""
    for k, c0 in ((0, 2), (1, 7)):
        d = R.ulps32(vec["rows"][:, R.SCALE + k], R.scale_torch(vec["elNorm"][:, k, 2:4], vec["elOut"][:, c0:c0 + 2]))
        print("scale ratio %d: torch differs by %d ulp" % (k, d))
        assert d <= 2


def test_epoch_summary_is_the_host_loop(vec):
    """epoch_summary over three batches of different sizes against the reference's loop (train.py:289-338, :387-427) written out with
    the project's host functions on the tensors themselves."""
    from egne_amd import scores, utils
    sizes, rows, want, ious = (5, 4, 3), [], {k: [] for k in ("iri_c", "iri_ang", "iri_sc", "pup_c", "pup_ang", "pup_sc")}, []
    lo = 0
    for bn, n in enumerate(sizes):
        s = slice(lo, lo + n)
        lo += n
        yt, yp = R.maps(n, 7, 9, seed=40 + bn, stray=False)
        if bn == 1:
            yt[0][yt[0] == 2] = 0
        eo, ep, pc, ic, en, cond = (vec[k][s] for k in ("elOut", "elPred", "pc", "ic", "elNorm", "cond"))
        cf = cond.astype(np.float32)
        rows.append(R.rows_ref(yt, yp, eo, ep, pc, ic, en, cond, loss=0.5 + bn, batch_no=bn))
        ious.append(utils.getSeg_metrics(yt, yp, cf[:, 1])[1])
        want["iri_c"].append(utils.getPoint_metric(ic, eo[:, 0:2], cf[:, 1], (7, 9), True)[0])
        want["pup_c"].append(utils.getPoint_metric(pc, eo[:, 5:7], cf[:, 0], (7, 9), True)[0])
        want["iri_ang"].append(utils.getAng_metric(en[:, 0, 4], eo[:, 4], cf[:, 1])[0])
        want["pup_ang"].append(utils.getAng_metric(en[:, 1, 4], eo[:, 9], cf[:, 1])[0])
        for name, k, c0 in (("iri_sc", 0, 2), ("pup_sc", 1, 7)):       # train.py:323-330 with the IEEE root (scores_refs' docstring)
            sc = torch.from_numpy(R.scale_ref(en[:, k, 2:4], eo[:, c0:c0 + 2])).to(torch.float32)
            want[name].append(torch.sum(sc * (~torch.from_numpy(cond[:, 1])).to(torch.float32)).item())
    rows = np.concatenate(rows)
    assert [len(b) for b in scores.batches(rows)] == list(sizes)
    got = scores.epoch_summary(rows)
    with np.errstate(all="ignore"):
        for k, v in want.items():
            assert _same(got[k + "/mu"], np.nanmean(v)) and _same(got[k + "/std"], np.nanstd(v)), k
        assert _same(got["train_iou"], np.nanmean(np.stack(ious, axis=0), axis=0))
    assert sorted(got) == sorted([k + s for k in want for s in ("/mu", "/std")] + ["train_iou"])
