"""CPU: the restatement of the ellipse scores (tests/ellipse_scores_refs.py) against the reference's recorded values
(tests/golden/ellipse_scores.npz), the fill rule against PIL, egne_amd.scores.ellipse_summary against the recorded reductions, and the
new flags of args.py."""
import hashlib
import os

import numpy as np
import pytest

import ellipse_scores_refs as R
from oracle import fit as ofit


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ellipse_scores.npz")))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", sorted(R.FIXTURE_CASES))
def test_restatement_reproduces_the_fixture(gold, name):
    """Every per-sample array of the fixture from the seeded inputs: pixel ellipses (1e-12: the reference inverts H numerically),
    corners, box counts on the reference's canvas, parameter differences, the searched ellipses and the calc_ell_iou scores exactly."""
    H, W, N, B, seed = R.FIXTURE_CASES[name]
    g = {k[len(name) + 1:]: v for k, v in gold.items() if k.startswith(name + "_")}
    inp = R.fixture_inputs(name)
    assert hashlib.sha256(inp["mask"].tobytes()).hexdigest() == str(g["mask_sha"])
    for k in ("elPred", "elNorm", "cond"):
        assert np.array_equal(inp[k], g[k]) and inp[k].dtype == g[k].dtype, k
    cH, cW = (int(v) for v in g["canvas"])
    assert (cH, cW) == (240, 320)
    for i in range(N):
        for k in (0, 1):
            seg = inp["mask"][i] == 1 + k
            l, l_gt, l_s = g["l_pred"][i, k], g["l_gt"][i, k], g["l_search"][i, k]
            np.testing.assert_allclose(R.to_pixels(inp["elPred"][i, 5 * k:5 * k + 5], H, W), l, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(R.to_pixels(inp["elNorm"][i, k], H, W), l_gt, rtol=1e-12, atol=1e-12)
            assert np.array_equal(R.box_corners(l), g["corners_pred"][i, k]) and np.array_equal(R.box_corners(l_gt), g["corners_gt"][i, k])
            assert np.array_equal(R.box_corners(l_s), g["corners_search"][i, k])
            for sfx, el in (("", l), ("_search", l_s)):
                iou, n_and, n_or = R.box_iou(R.box_corners(el), R.box_corners(l_gt), cH, cW)
                assert _same(iou, g["box_iou" + sfx][i, k]) and (n_and, n_or) == (g["box_and" + sfx][i, k], g["box_or" + sfx][i, k])
                assert np.array_equal(np.abs(el - l_gt), g["para" + sfx][i, k])
                gmap = R.ell_map(H, W, l_gt)
                assert _same(ofit.score_of_counts(*R.ell_counts(gmap, el)), g["ell_iou" + sfx][i, k])
            assert _same(ofit.score_of_counts(*R.ell_counts(seg, l)), g["map_iou_pred"][i, k])
            assert _same(ofit.score_of_counts(*R.ell_counts(seg, l_gt)), g["map_iou_gt"][i, k])
            assert _same(ofit.score_of_counts(*R.ell_counts(seg, l_s)), g["map_iou_search"][i, k])
            with np.errstate(all="ignore"):
                assert np.array_equal(ofit.fit_ellipse(seg, list(l)), l_s)
            for el in (l, l_gt, l_s):      # the guards the fixture's docstring states
                assert not R.near_integer(el)
                wt = R.membership_margin(H, W, el)
                assert np.array_equal(wt <= 0, R.ell_map(H, W, el)) and not np.any(np.abs(wt) < R.NEAR_ZERO)
    if name in R.OFF_CANVAS:
        assert np.all(np.isnan(g["box_iou"][R.OFF_CANVAS[name]])) and np.all(g["box_or"][R.OFF_CANVAS[name]] == 0)
    for sfx in ("", "_search"):
        for k in (0, 1):
            bb, mean, para = R.summary(g["box_iou" + sfx][:, k], g["para" + sfx][:, k], [B] * (N // B))
            assert _same(bb, g["bbiou_batches" + sfx][:, k]) and _same(mean, g["bbiou" + sfx][k]) and _same(para, g["para_mean" + sfx][k])


def test_ellipse_summary_matches_the_reference_reductions(gold):
    """egne_amd.scores.ellipse_summary over rows built from the fixture's per-sample values: the per-batch means (one batch of case a
    holds a NaN sample and is NaN), their nanmean and the parameter means, bit for bit; the plain means leave flagged samples out."""
    from egne_amd import scores
    for name, (H, W, N, B, seed) in R.FIXTURE_CASES.items():
        for sfx in ("", "_search"):
            rows = np.full((N, scores.ELL_FIELDS), np.nan)
            for k in (0, 1):
                o = k * scores.ELL_REGION_FIELDS
                rows[:, o + scores.ELL_BOX_IOU] = gold[name + "_box_iou" + sfx][:, k]
                rows[:, o + scores.ELL_PARA:o + scores.ELL_PARA + 5] = gold[name + "_para" + sfx][:, k]
                rows[:, o + scores.ELL_AREA:o + scores.ELL_AREA + 3] = (3, 2, 1)
            rows[:, scores.ELL_BATCH] = np.arange(N) // B
            rows[:, scores.ELL_COND1] = gold[name + "_cond"][:, 1]
            s = scores.ellipse_summary(rows)
            for k, r in enumerate(scores.ELL_REGIONS):
                assert _same(s["bbiou_batches_" + r], gold[name + "_bbiou_batches" + sfx][:, k])
                assert _same(s["bbiou_" + r], gold[name + "_bbiou" + sfx][k])
                assert _same(s["para_" + r], gold[name + "_para_mean" + sfx][k])
                v = gold[name + "_box_iou" + sfx][:, k]
                ok = gold[name + "_cond"][:, 1] == 0
                assert _same(s["box_iou_" + r], np.nanmean(v)) and _same(s["box_iou_" + r + "_valid"], np.nanmean(v[ok]))
                assert s["ell_iou_" + r] == 1 / 4 and np.isnan(s["map_iou_pred_" + r])
        if name in R.OFF_CANVAS:
            assert np.isnan(s["bbiou_batches_iris"][R.OFF_CANVAS[name] // B]) and np.isfinite(s["bbiou_iris"])
    assert len(scores.ell_field_names()) == scores.ELL_FIELDS


def test_row_layout_matches_the_header():
    """The ELL_* constants of egne_amd.scores are the EGNE_ELLSCORE_* of include/egne_hip.h."""
    import re
    from egne_amd import scores
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "egne_hip.h")) as f:
        hdr = dict(re.findall(r"#define EGNE_ELLSCORE_(\w+) (\d+)", f.read()))
    names = {"ELL_PRED": "ELL_PRED", "ELL_GT": "ELL_GT", "CORNERS_PRED": "ELL_CORNERS_PRED", "CORNERS_GT": "ELL_CORNERS_GT", "BOX_IOU": "ELL_BOX_IOU",
             "BOX_AND": "ELL_BOX_AND", "BOX_OR": "ELL_BOX_OR", "PARA": "ELL_PARA", "AREA": "ELL_AREA", "MAP_PRED": "ELL_MAP_PRED",
             "MAP_GT": "ELL_MAP_GT", "REGION_FIELDS": "ELL_REGION_FIELDS", "COND0": "ELL_COND0", "COND1": "ELL_COND1", "BATCH": "ELL_BATCH",
             "SAMPLE": "ELL_SAMPLE", "FIELDS": "ELL_FIELDS"}
    assert set(hdr) == set(names)
    for h, p in names.items():
        assert int(hdr[h]) == getattr(scores, p), h


def test_fill_rule_stays_within_one_pixel_of_pil_edges():
    """Independent of OpenCV: the closed-quadrilateral fill against PIL's ImageDraw.polygon(fill, outline) on random rotated boxes
    (240 x 320 canvas, centres up to 20 pixels outside it, half axes 0.3 to 120, all angles).  The two differ -- PIL fills spans between
    rounded edge crossings -- but only on pixels within Chebyshev distance 1 of a pixel of the PIL-drawn edges; an exact match is not
    asked for."""
    from PIL import Image, ImageDraw
    H, W = 240, 320
    rng = np.random.RandomState(5)
    differing = 0
    for _ in range(400):
        el = (rng.uniform(-20, W + 20), rng.uniform(-20, H + 20), rng.uniform(0.3, 120), rng.uniform(0.3, 120), rng.uniform(-np.pi, np.pi))
        c = R.box_corners(el)
        pts = [(int(c[2 * k]), int(c[2 * k + 1])) for k in range(4)]
        im = Image.new("L", (W, H), 0)
        ImageDraw.Draw(im).polygon(pts, fill=255, outline=255)
        edge = Image.new("L", (W + 2, H + 2), 0)          # the drawn edges on a canvas one pixel larger all round, then their 3x3 neighbourhood
        ImageDraw.Draw(edge).polygon([(x + 1, y + 1) for x, y in pts], fill=0, outline=255)
        e = np.asarray(edge) > 0
        band = np.zeros((H, W), bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                band |= e[dy:dy + H, dx:dx + W]
        diff = (np.asarray(im) > 0) != R.quad_fill(c, H, W)
        differing += bool(diff.any())
        assert not np.any(diff & ~band), (el, pts, np.argwhere(diff & ~band)[:5])
    print("boxes that differ from PIL somewhere: %d of 400" % differing)


def test_corner_conversion_and_degenerate_boxes():
    """Truncation toward zero (not floor), NumPy's INT_MIN for values outside int32, and the segment rule of a box without area."""
    assert R.to_i32([-0.7, -1.2, 1.9, 2147483647.5, 2147483648.0, -2147483648.9, -2147483649.0, np.nan]).tolist() == \
        [0, -1, 1, 2147483647, -2147483648, -2147483648, -2147483648, -2147483648]
    assert R.box_corners((-0.5, -0.5, 1.25, 0.25, 0.0)).tolist() == [-1, 0, -1, 0, 0, 0, 0, 0]
    line = R.quad_fill([1, 1, 1, 1, 4, 4, 4, 4], 6, 6)
    assert np.argwhere(line).tolist() == [[1, 1], [2, 2], [3, 3], [4, 4]]
    assert R.quad_fill([2, 3, 2, 3, 2, 3, 2, 3], 6, 6).sum() == 1
    big = R.quad_fill([-(1 << 31), -(1 << 31), -(1 << 31), (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, -(1 << 31)], 4, 5)
    assert big.all()
    for order in ([0, 0, 0, 3, 4, 3, 4, 0], [0, 0, 4, 0, 4, 3, 0, 3]):      # both orientations
        assert R.quad_fill(order, 6, 6).sum() == 20


def test_args_flags_and_dependency_notes(capsys):
    from egne_amd.args import ellipse_metrics_note, parse_args
    base = ["--synthetic", "4", "--setting", "configs/baseline_edge.yaml"]
    a = parse_args(base)
    assert a.ellipse_metrics == 0 and a.ellipse_search == 0 and ellipse_metrics_note(a) is None
    a = parse_args(base + ["--ellipse_metrics", "1"])
    assert a.ellipse_metrics == 1 and "needs --device_metrics 1" in ellipse_metrics_note(a)
    a = parse_args(base + ["--device_metrics", "1", "--ellipse_search", "1"])
    assert a.ellipse_search == 1 and "needs --ellipse_metrics 1" in ellipse_metrics_note(a)
    a = parse_args(base + ["--device_metrics", "1", "--ellipse_metrics", "1", "--ellipse_search", "1"])
    assert ellipse_metrics_note(a) is None
    capsys.readouterr()
