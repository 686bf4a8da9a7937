"""-m gpu: csrc/ellipse_scores.hip through egne_amd.scores (EllipseLedger, ellipse_box_corners, box_iou_counts) against the restatement
in tests/ellipse_scores_refs.py (held to the reference's recorded values by tests/test_host_ellipse_scores.py) and against the fixture
itself.  Corners, counts and box IoUs must be equal exactly, NaNs in the same places; parameter differences within 4 ulps.

The device forms its pixel ellipses itself (egne_ellipse_init_from_pred's transform: within 1e-11 of the host's, tests/test_gpu_fit.py),
so a row is checked in two steps: its own ELL_PRED / ELL_GT columns against the host transform within that bound, and every other
column against the restatement applied to those very columns.  The inputs keep every float64 corner 1e-6 away from an integer, which
is what makes the second step exact (tests/ellipse_scores_refs.py)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import ellipse_scores_refs as R
from oracle import fit as ofit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2), (24, 40), (37, 53), (240, 320)]          # neither 24 x 40 nor 37 x 53 is a multiple of the wave size


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ellipse_scores.npz")))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _dev(inp):
    return {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def _append(ledger, d, lo=0, hi=None, **kw):
    ledger.append(d["mask"][lo:hi], d["elPred"][lo:hi], d["elNorm"][lo:hi], d["cond"][lo:hi], **kw)


def _rows(inp, classes=(1, 2), **kw):
    from egne_amd import scores
    led = scores.EllipseLedger(len(inp["mask"]), DEV, classes=classes)
    _append(led, _dev(inp), **kw)
    return led.rows()


def _region(rows, i, k):
    from egne_amd import scores
    return rows[i, k * scores.ELL_REGION_FIELDS:(k + 1) * scores.ELL_REGION_FIELDS]


def _check_region(S, reg, seg, what):
    """Every column of a region against the restatement applied to the region's own two pixel ellipses."""
    pred, gt = reg[S.ELL_PRED:S.ELL_PRED + 5], reg[S.ELL_GT:S.ELL_GT + 5]
    assert not R.near_integer(pred) and not R.near_integer(gt), what      # (else the exact comparison of the corners is not owed)
    want = R.region_scores(pred, gt, seg)
    assert np.array_equal(reg[S.ELL_CORNERS_PRED:S.ELL_CORNERS_PRED + 8], want["corners_pred"]), what
    assert np.array_equal(reg[S.ELL_CORNERS_GT:S.ELL_CORNERS_GT + 8], want["corners_gt"]), what
    assert (reg[S.ELL_BOX_AND], reg[S.ELL_BOX_OR]) == (want["box_and"], want["box_or"]), (what, reg[S.ELL_BOX_AND:S.ELL_BOX_OR + 1], want)
    assert _same(reg[S.ELL_BOX_IOU], want["box_iou"]), what
    np.testing.assert_array_max_ulp(reg[S.ELL_PARA:S.ELL_PARA + 5], want["para"], maxulp=4)
    assert tuple(reg[S.ELL_AREA:S.ELL_AREA + 3]) == want["area"], (what, reg[S.ELL_AREA:S.ELL_AREA + 3], want["area"])
    assert tuple(reg[S.ELL_MAP_PRED:S.ELL_MAP_PRED + 3]) == want["map_pred"], what
    assert tuple(reg[S.ELL_MAP_GT:S.ELL_MAP_GT + 3]) == want["map_gt"], what
    assert reg[S.ELL_MAP_GT + 1] == reg[S.ELL_AREA + 1], what              # the ellipse's map pixel by pixel == the search's row intervals


# ---- boxes made by hand ---------------------------------------------------------------------------------------------------------
def _hand_boxes(H, W):
    """name -> pixel ellipse whose box is the case; the coordinates keep clear of integers (checked by the test)."""
    mx, my = float(W // 2), float(H // 2)
    return {
        "middle": (mx + 0.3137, my + 0.4142, 0.2 * W + 0.2071, 0.15 * H + 0.1183, 0.0),            # theta 0: horizontal and vertical edges
        "middle_quarter_turn": (mx + 0.3137, my + 0.4142, 0.15 * H + 0.1183, 0.2 * W + 0.2071, np.pi / 2),
        "tilted": (0.45 * W + 0.1337, 0.55 * H + 0.2113, 0.3 * W + 0.1571, 0.2 * H + 0.3491, 0.6),
        "corner00": (0.45, 0.55, 0.3, 0.3, 0.0),                                                     # the pixel (0, 0): no area
        "cornerHW": (W - 0.55, H - 0.45, 0.3, 0.3, 0.0),                                             # the pixel (W-1, H-1): disjoint from it
        "outside_a": (5.3 * W + 0.0713, 4.2 * H + 0.0419, 0.2 * W + 0.3, 0.2 * H + 0.3, 0.3),
        "outside_b": (-3.1 * W - 0.0713, -2.7 * H - 0.0419, 0.3 * W + 0.2, 0.1 * H + 0.4, -0.8),
        "cover": (mx + 0.2137, my + 0.3142, 2.0 * (H + W) + 0.4071, 2.0 * (H + W) + 0.3183, 0.0),
        "negative_corner": (0.3, 0.4, 0.9, 0.9, 0.0),                                                # -0.6 and -0.5 truncate to 0, floor gives -1
        "past_all_sides": (mx + 0.3137, my + 0.2142, 1.0 * W + 0.3071, 1.0 * H + 0.4183, 0.7),
        "flat": (mx + 0.3137, my + 0.5, 0.25 * W + 0.4571, 0.3, 0.0),                               # half axis below 1: a row segment
        "one_wide": (mx + 0.6, my + 0.3142, 0.5, 0.2 * H + 0.4183, 0.0),                             # x corners n and n + 1
    }


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hand_made_boxes(shape):
    """Every pair of the hand-made boxes in one launch of each wrapper: corners, n_and, n_or and the IoU against the restatement, and
    the values the cases are there for."""
    from egne_amd import scores
    H, W = shape
    cases = _hand_boxes(H, W)
    names = list(cases)
    ell = np.array([cases[n] for n in names], np.float64)
    for n, e in zip(names, ell):
        assert not R.near_integer(e), n
    want_c = np.stack([R.box_corners(e) for e in ell])
    got_c = scores.ellipse_box_corners(torch.from_numpy(ell).to(DEV))
    assert got_c.dtype == torch.int32 and np.array_equal(got_c.cpu().numpy(), want_c)
    assert want_c[names.index("negative_corner")].min() == 0 and np.floor(R.box_corners_f64(cases["negative_corner"])).min() == -1
    ia, ib = np.divmod(np.arange(len(names) ** 2), len(names))
    got = scores.box_iou_counts(got_c[torch.from_numpy(ia).to(DEV)], got_c[torch.from_numpy(ib).to(DEV)], H, W).cpu().numpy()
    fills = [R.quad_fill(c, H, W) for c in want_c]
    for j, (a, b) in enumerate(zip(ia, ib)):
        n_and, n_or = int(np.count_nonzero(fills[a] & fills[b])), int(np.count_nonzero(fills[a] | fills[b]))
        assert (got[j, 1], got[j, 2]) == (n_and, n_or), (names[a], names[b], got[j], n_and, n_or)
        assert _same(got[j, 0], n_and / n_or if n_or else np.nan), (names[a], names[b])
    pair = lambda a, b: got[names.index(a) * len(names) + names.index(b)]      # noqa: E731
    for n in names:
        if not n.startswith("outside"):
            assert pair(n, n)[0] == 1.0, n                                     # identical boxes
    assert pair("corner00", "cornerHW")[0] == 0.0 and pair("corner00", "cornerHW")[2] == 2          # disjoint: one pixel each
    assert np.isnan(pair("outside_a", "outside_b")[0]) and pair("outside_a", "outside_b")[2] == 0   # nothing on the canvas: 0 / 0
    assert pair("cover", "cover")[2] == H * W and pair("past_all_sides", "cover")[1] == fills[names.index("past_all_sides")].sum()
    assert fills[names.index("flat")].sum() > 0 and len(set(want_c[names.index("flat")][1::2])) == 1          # no area, yet its pixels count
    xs = want_c[names.index("one_wide")][0::2]
    assert xs.max() - xs.min() == 1


def test_boxes_of_absurd_ellipses():
    """Corners beyond int32 become INT_MIN as in NumPy, and the fill of such a box (128-bit cross products) is the restatement's."""
    from egne_amd import scores
    H, W = 24, 40
    ell = np.array([[1e12, 3.5, 10.3, 4.2, 0.0], [20.3, 11.6, 2.1e9, 2e9, 0.0], [np.nan, 1.5, 2.5, 3.5, 0.1], [20.3, 11.6, 7.7, 5.2, 0.4]])
    want_c = np.stack([R.box_corners(e) for e in ell])
    got_c = scores.ellipse_box_corners(torch.from_numpy(ell).to(DEV))
    assert np.array_equal(got_c.cpu().numpy(), want_c) and want_c.min() == -2 ** 31
    got = scores.box_iou_counts(got_c, got_c[[3, 3, 3, 3]], H, W).cpu().numpy()
    for j in range(4):
        want = R.box_iou(want_c[j], want_c[3], H, W)
        assert _same(got[j], want), (j, got[j], want)


# ---- whole rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", [(2, 2, 1), (24, 40, 3), (37, 53, 65), (240, 320, 3)])
def test_rows_equal_the_restatement(H, W, B):
    from egne_amd import scores as S, utils
    inp = R.inputs(H, W, B, seed=3)
    rows = _rows(inp)
    assert rows.shape == (B, S.ELL_FIELDS) and not np.isnan(rows).any()
    d = _dev(inp)
    seeds = utils.ellipse_seeds_from_pred(d["elPred"], H, W)[0].cpu().numpy().reshape(B, 2, 5)
    ell, fo, cl, want_counts = [], [], [], []
    for i in range(B):
        for k in (0, 1):
            reg = _region(rows, i, k)
            assert np.array_equal(reg[S.ELL_PRED:S.ELL_PRED + 5], seeds[i, k])
            np.testing.assert_allclose(reg[S.ELL_GT:S.ELL_GT + 5], R.to_pixels(inp["elNorm"][i, k], H, W), rtol=1e-11, atol=1e-11)
            _check_region(S, reg, inp["mask"][i] == 1 + k, (H, W, i, k))
            for o, c in ((S.ELL_PRED, S.ELL_MAP_PRED), (S.ELL_GT, S.ELL_MAP_GT)):
                ell.append(R.deg(reg[o:o + 5])); fo.append(i); cl.append(1 + k); want_counts.append(reg[c:c + 3])
    # (e) through the entry point the search's evaluation is tested by
    got = utils.ellipse_iou_counts(d["mask"], fo, cl, np.array(ell))
    assert np.array_equal(got.astype(np.float64), np.array(want_counts))
    assert np.array_equal(rows[:, S.ELL_COND0], inp["cond"][:, 0]) and np.array_equal(rows[:, S.ELL_COND1], inp["cond"][:, 1])
    assert np.array_equal(rows[:, S.ELL_BATCH], np.zeros(B)) and np.array_equal(rows[:, S.ELL_SAMPLE], np.arange(B))


def test_ellipse_area_counts_through_ellipse_iou_counts():
    """(d): the ground-truth ellipse's own map (rasterised on the host by the oracle) as the class map of utils.ellipse_iou_counts gives
    the AREA triple of the row."""
    from egne_amd import scores as S, utils
    H, W, B = 37, 53, 3
    inp = R.inputs(H, W, B, seed=4)
    rows = _rows(inp)
    maps, ell, fo = [], [], []
    for i in range(B):
        for k in (0, 1):
            reg = _region(rows, i, k)
            maps.append(R.ell_map(H, W, reg[S.ELL_GT:S.ELL_GT + 5]).astype(np.int64))
            ell.append(R.deg(reg[S.ELL_PRED:S.ELL_PRED + 5])); fo.append(len(maps) - 1)
    got = utils.ellipse_iou_counts(torch.from_numpy(np.stack(maps)).to(DEV), fo, [1] * len(fo), np.array(ell))
    for j, (n_gt, n_pred, n_both) in enumerate(got.tolist()):
        assert tuple(_region(rows, j // 2, j % 2)[S.ELL_AREA:S.ELL_AREA + 3]) == (n_pred, n_gt, n_both)


@pytest.mark.parametrize("name", sorted(R.FIXTURE_CASES))
def test_fixture_cases(gold, name):
    """The reference's recorded values: corners, box counts, IoUs and reductions exactly; pixel ellipses and parameter differences within
    the bound of the pixel transform (1e-11 relative, tests/test_gpu_fit.py; a difference of two such values: twice that); the searched
    ellipses bit for bit from the recorded seeds and within that bound from the device's own."""
    from egne_amd import scores as S, utils
    H, W, N, B, seed = R.FIXTURE_CASES[name]
    g = {k[len(name) + 1:]: v for k, v in gold.items() if k.startswith(name + "_")}
    inp = R.fixture_inputs(name)
    d = _dev(inp)
    same_canvas = tuple(g["canvas"]) == (H, W)
    tol = lambda v: 2 * (1e-11 * np.abs(v) + 1e-11)      # noqa: E731
    for search, sfx in ((False, ""), (True, "_search")):
        led = S.EllipseLedger(N, DEV)
        for b0 in range(0, N, B):
            _append(led, d, b0, b0 + B, search=search)
        rows = led.rows()
        assert np.array_equal(rows[:, S.ELL_BATCH], np.arange(N) // B) and np.array_equal(rows[:, S.ELL_SAMPLE], np.arange(N) % B)
        l_ref = g["l_search"] if search else g["l_pred"]
        for i in range(N):
            for k in (0, 1):
                reg = _region(rows, i, k)
                pred, gt = reg[S.ELL_PRED:S.ELL_PRED + 5], reg[S.ELL_GT:S.ELL_GT + 5]
                assert np.all(np.abs(pred - l_ref[i, k]) <= tol(l_ref[i, k])) and np.all(np.abs(gt - g["l_gt"][i, k]) <= tol(g["l_gt"][i, k]))
                assert np.array_equal(reg[S.ELL_CORNERS_PRED:S.ELL_CORNERS_PRED + 8], g["corners" + ("_search" if search else "_pred")][i, k])
                assert np.array_equal(reg[S.ELL_CORNERS_GT:S.ELL_CORNERS_GT + 8], g["corners_gt"][i, k])
                p_ref = g["para" + sfx][i, k]
                assert np.all(np.abs(reg[S.ELL_PARA:S.ELL_PARA + 5] - p_ref) <= tol(l_ref[i, k]) + tol(g["l_gt"][i, k]))
                if same_canvas:
                    assert _same(reg[S.ELL_BOX_IOU:S.ELL_BOX_OR + 1], [g["box_iou" + sfx][i, k], g["box_and" + sfx][i, k], g["box_or" + sfx][i, k]])
                assert _same(ofit.score_of_counts(reg[S.ELL_AREA + 1], reg[S.ELL_AREA], reg[S.ELL_AREA + 2]), g["ell_iou" + sfx][i, k])
                assert _same(ofit.score_of_counts(*reg[S.ELL_MAP_PRED:S.ELL_MAP_PRED + 3]), g["map_iou_search" if search else "map_iou_pred"][i, k])
                assert _same(ofit.score_of_counts(*reg[S.ELL_MAP_GT:S.ELL_MAP_GT + 3]), g["map_iou_gt"][i, k])
                _check_region(S, reg, inp["mask"][i] == 1 + k, (name, search, i, k))
        if not same_canvas:      # calc_bbox_iou's fixed 240 x 320 canvas, through the wrapper
            c = torch.from_numpy(np.ascontiguousarray(np.concatenate([g["corners" + ("_search" if search else "_pred")], g["corners_gt"]], 0).reshape(-1, 8))).to(DEV)
            got = S.box_iou_counts(c[:2 * N], c[2 * N:], *(int(v) for v in g["canvas"])).cpu().numpy().reshape(N, 2, 3)
            assert _same(got, np.stack([g["box_iou" + sfx], g["box_and" + sfx], g["box_or" + sfx]], -1))
        s = S.ellipse_summary(rows)
        for k, r in enumerate(S.ELL_REGIONS):
            if same_canvas:
                assert _same(s["bbiou_batches_" + r], g["bbiou_batches" + sfx][:, k]) and _same(s["bbiou_" + r], g["bbiou" + sfx][k])
            np.testing.assert_allclose(s["para_" + r], g["para_mean" + sfx][k], rtol=1e-9, atol=1e-9)
    if name in R.OFF_CANVAS:
        assert np.isnan(s["bbiou_batches_iris"][R.OFF_CANVAS[name] // B])
    # the search from the RECORDED seeds: the reference's searched ellipses bit for bit
    fo, cl = np.repeat(np.arange(N), 2), np.tile([1, 2], N)
    assert np.array_equal(utils.fit_ellipses(d["mask"], fo, cl, g["l_pred"].reshape(-1, 5)), g["l_search"].reshape(-1, 5))


def test_search_rows_are_the_fit_rows():
    """search=True is utils.fit_ellipses_from_pred followed by the scoring of its output (fit=): the same code on both routes."""
    from egne_amd import scores as S, utils
    inp = R.inputs(24, 40, 3, seed=5)
    d = _dev(inp)
    fit = utils.fit_ellipses_from_pred(d["mask"], d["elPred"])
    a, b = _rows(inp, search=True), _rows(inp, fit=fit)
    assert _same(a, b) and np.array_equal(_region(a, 1, 1)[S.ELL_PRED:S.ELL_PRED + 5], fit[1, 1].cpu().numpy())
    assert not _same(a, _rows(inp))


def test_pupil_only_map():
    """DeepVOG's two-class map: classes (-1, 1) leave the iris columns NaN and hold the pupil against class 1, searched or not."""
    from egne_amd import scores as S
    inp = R.inputs(24, 40, 3, seed=6)
    inp["mask"] = (inp["mask"] == 2).astype(np.int64)
    for search in (False, True):
        rows = _rows(inp, classes=(-1, 1), search=search)
        assert np.isnan(rows[:, :S.ELL_REGION_FIELDS]).all() and not np.isnan(rows[:, S.ELL_REGION_FIELDS:]).any()
        for i in range(3):
            _check_region(S, _region(rows, i, 1), inp["mask"][i] == 1, (search, i))


def test_ledger():
    from egne_amd import scores as S
    inp = R.inputs(24, 40, 5, seed=7)
    d = _dev(inp)
    whole = _rows(inp)
    led = S.EllipseLedger(5, DEV)
    _append(led, d, 0, 2)
    _append(led, d, 2, 5)
    two = led.rows()
    assert two[:, S.ELL_BATCH].tolist() == [0, 0, 1, 1, 1] and two[:, S.ELL_SAMPLE].tolist() == [0, 1, 0, 1, 2]
    assert _same(two[:, :S.ELL_BATCH], whole[:, :S.ELL_BATCH])
    with pytest.raises(RuntimeError, match="do not fit"):
        _append(led, d, 0, 1)
    led.reset()
    assert led.rows().shape == (0, S.ELL_FIELDS) and torch.isnan(led.buf).all()
    _append(led, d, 0, 2)
    _append(led, d, 2, 5)
    assert _same(led.rows(), two), "two runs differ"
    led.reset()
    with pytest.raises(TypeError, match="float32"):
        led.append(d["mask"][:1], d["elPred"][:1], d["elNorm"][:1].double(), d["cond"][:1])
    with pytest.raises(TypeError, match="float32"):
        led.append(d["mask"][:1], d["elPred"][:1].double(), d["elNorm"][:1], d["cond"][:1])
    assert led.n == 0 and led.batches == 0
    with pytest.raises(RuntimeError, match="do not fit LDS"):
        S.EllipseLedger(1, DEV).append(torch.zeros((1, 512, 640), dtype=torch.int64, device=DEV), d["elPred"][:1], d["elNorm"][:1], d["cond"][:1])


# ---- test.py ---------------------------------------------------------------------------------------------------------------------
def _run_test_py(cwd, *flags):
    script = os.path.join(ROOT, "edge-guided-near-eye-image-analysis-for-head-mounted-displays_amd", "test.py")
    cmd = [sys.executable, script, "--synthetic", "12", "--batchsize", "4", "--setting", "configs/baseline_edge.yaml", "--device_metrics", "1"] + list(flags)
    r = subprocess.run(cmd, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_test_py_ellipse_metrics(tmp_path):
    """test.py in child processes on 12 synthetic frames: the reference's four lines and the three added per region, the pickle of 12
    rows, other numbers with the search; with --ellipse_metrics 0 the output is that of a command line without the flag, byte for byte."""
    from egne_amd import scores as S
    four = ("Bounding box Pupil IoU. Mean : ", "Bounding box Iris IoU. Mean : ", "ABS Pupil parameters : ", "ABS Iris parameters : ")
    outs = {}
    for key, flags in (("plain", ["--ellipse_metrics", "1", "--record_iou", "1"]), ("search", ["--ellipse_metrics", "1", "--ellipse_search", "1", "--record_iou", "1"])):
        cwd = tmp_path / key
        cwd.mkdir()
        out = outs[key] = _run_test_py(cwd, *flags)
        for line in four:
            assert sum(l.startswith(line) for l in out.splitlines()) == 1, (key, line)
        assert sum(l.startswith("Ellipse area ") for l in out.splitlines()) == 2 and sum(l.startswith("Class map ") for l in out.splitlines()) == 2
        with open(cwd / "img" / "synthetic_baseline_ellipses.pkl", "rb") as f:
            rec = pickle.load(f)
        assert rec["rows"].shape == (12, S.ELL_FIELDS) and rec["fields"] == S.ell_field_names()
        assert rec["rows"][:, S.ELL_BATCH].tolist() == [0] * 4 + [1] * 4 + [2] * 4 and not np.isnan(rec["rows"][:, S.ELL_PRED:S.ELL_PRED + 5]).any()
        s = S.ellipse_summary(rec["rows"])
        assert "Bounding box Pupil IoU. Mean : {}".format(s["bbiou_pupil"]) in out.splitlines()
        with open(cwd / "img" / "synthetic_baseline_ious.pkl", "rb") as f:
            assert pickle.load(f).shape == (12, 3)
    tail = lambda s: [l for l in s.splitlines() if l.startswith(("mIoU", "Latent", "Segmentation"))]      # noqa: E731
    assert len(tail(outs["plain"])) == 5 and tail(outs["plain"]) == tail(outs["search"])
    assert [l for l in outs["plain"].splitlines() if l.startswith("ABS")] != [l for l in outs["search"].splitlines() if l.startswith("ABS")]
    off = _run_test_py(tmp_path, "--ellipse_metrics", "0")
    absent = _run_test_py(tmp_path)
    assert "Bounding box" not in off and off == absent and tail(off) == tail(outs["plain"])
