"""-m gpu: ellipse seeds from the class map (csrc/mask_seed.hip, evaluate.py --ellipse_seed mask) against the NumPy restatement of
tests/mask_seed_refs.py.  Every comparison of the integer statistics is exact; the five doubles are compared with the restatement's
float64 block evaluated on the DEVICE's own statistics (identical inputs to sqrt / atan2: only libm's last bits may differ)."""
import ctypes

import numpy as np
import pytest
import torch

import mask_seed_refs as R
import video_harness as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_AREA = 7


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def nets():
    from common import bdcn_module, esf_module
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device(DEV)
    return bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()


def _rows(mask, frame_of, class_bits, search_cls, min_area=MIN_AREA):
    """egne_ellipse_init_from_mask on arbitrary rows -> host arrays (init, out_frame_of, out_cls, stats, status)."""
    from egne_amd import _lib
    from egne_amd.utils import _seeds_from_mask_rows
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(DEV)      # noqa: E731  (bit patterns)
    res = _seeds_from_mask_rows(_lib.lib(), torch.from_numpy(np.ascontiguousarray(mask)).to(DEV), t(frame_of), t(class_bits),
                                t(search_cls), int(min_area), True)
    return tuple(r.cpu().numpy() for r in res)


def _check(got, want, H, W, what):
    init, fo, cl, stats, status = got
    w_init, w_fo, w_cl, w_stats = want
    assert int(status[0]) == 0, "%s: status %d" % (what, status[0])
    assert np.array_equal(stats, w_stats), "%s: stats\n%s\nwant\n%s" % (what, stats, w_stats)
    assert np.array_equal(fo, w_fo) and np.array_equal(cl, w_cl), "%s: frame_of %s cls %s" % (what, fo, cl)
    for i in range(len(fo)):
        mine = R.seed_from_stats(stats[i], H, W)             # from the device's own sums
        if fo[i] < 0:
            assert np.array_equal(init[i], np.full(5, -1.0)) and np.array_equal(mine, init[i]), "%s row %d: %s" % (what, i, init[i])
            continue
        assert np.all(np.abs(init[i, :4] - mine[:4]) <= 1e-12 * np.abs(mine[:4])), "%s row %d: %s vs %s" % (what, i, init[i], mine)
        assert abs(init[i, 4] - mine[4]) <= 1e-12, "%s row %d: theta %r vs %r" % (what, i, init[i, 4], mine[4])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_patterns(shape):
    """Every pattern that fits the shape, one frame each, in one call: region = class 1, searched against class 1."""
    H, W = shape
    names = [k for k, (h, w, _) in R.CASES.items() if (h, w) == (H, W)]
    mask = np.stack([R.CASES[k][2] for k in names])
    F = len(names)
    want = R.seeds(mask, ((0b10, 1),), MIN_AREA)
    got = _rows(mask, np.arange(F), [0b10] * F, [1] * F)
    for i, k in enumerate(names):
        print(k, got[3][i].tolist())
    _check(got, want, H, W, "%dx%d %s" % (H, W, names))
    by = dict(zip((k.split("_", 1)[1] for k in names), range(F)))
    assert got[1][by["empty"]] == -1 and got[3][by["empty"], 6] == 0
    assert got[3][by["checkerboard"], 6] == 1 and got[3][by["diagonal_join"], 6] == 1
    if "area_6" in by:
        assert got[1][by["area_6"]] == -1 and got[3][by["area_6"], 7] == 6 and got[3][by["area_7"], 0] == 7
    if "two_equal_blobs" in by and got[3][by["two_equal_blobs"], 7] >= 2 * MIN_AREA:          # (3x5: two blobs of one pixel, absent)
        i = by["two_equal_blobs"]
        assert got[3][i, 6] == 2 and 2 * got[3][i, 0] == got[3][i, 7] and got[3][i, 2] * 2 < got[3][i, 0] * H      # the upper blob


def _class_maps(H, W, F):
    """F class maps, a different pattern pair per frame: classes 1 | 2 = pattern a, class 2 = a & b."""
    pats = list(R.patterns(H, W).values())
    return np.stack([pats[f % len(pats)].astype(np.int64) + (pats[f % len(pats)] & pats[(3 * f + 5) % len(pats)]) for f in range(F)])


@pytest.mark.parametrize("F,shape", [(1, (240, 320)), (3, (240, 320)), (65, (61, 83))])
def test_batches_with_the_default_regions(F, shape):
    from egne_amd.utils import ellipse_seeds_from_mask
    H, W = shape
    mask = _class_maps(H, W, F)
    got = ellipse_seeds_from_mask(torch.from_numpy(mask).to(DEV), return_stats=True)
    assert got[0].dtype == torch.float64 and tuple(got[0].shape) == (2 * F, 5) and got[1].dtype == torch.int32
    _check(tuple(t.cpu().numpy() for t in got), R.seeds(mask, R.DEFAULT_REGIONS, MIN_AREA), H, W, "F=%d %dx%d" % (F, H, W))
    three = ellipse_seeds_from_mask(torch.from_numpy(mask).to(DEV))
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, got[:3]))


def test_rows_with_other_classes_absent_frames_and_empty_bits():
    """A frame with class ids 0..7 (and a few ids outside 0..31) and class_bits selecting {3, 5}; a frame_of outside [0, F) in the
    middle, on both sides; class_bits == 0: those rows are -1 five times with out_frame_of -1, their neighbours as the restatement."""
    H, W = 65, 129
    rng = np.random.RandomState(7)
    mask = _class_maps(H, W, 8)[[4, 1, 6]]                  # two blobs / (replaced below) / comb
    mask[1] = np.kron(rng.randint(0, 8, (13, 26)), np.ones((5, 5), np.int64))[:H, :W]      # 5x5 tiles of ids 0..7
    mask[1, 10:14, 3:9] = 35
    mask[1, 30:33, 100:120] = -2
    mask[1, 40, 40:60] = 2 ** 40 + 3                                                        # not id 3
    assert set(np.unique(mask[1])) >= set(range(8))
    frame_of = [0, 1, 7, 1, -1, 2, 2, 1, 3]
    bits = [0b110, 0b101000, 0b110, 0xffffffff, 0b110, 0, 0b100, 0b110, 0b10]
    cls = [1, 3, 1, 5, 1, 2, 2, 1, 1]
    want = R.seeds_rows(mask, frame_of, bits, cls, MIN_AREA)
    assert want[1][[0, 1, 3, 7]].tolist() == [0, 1, 1, 1] and want[1][[2, 4, 5, 8]].tolist() == [-1] * 4
    got = _rows(mask, frame_of, bits, cls)
    _check(got, want, H, W, "mixed rows")
    assert got[3][3, 7] == np.count_nonzero((mask[1] >= 0) & (mask[1] < 32))


def test_min_area_is_an_argument():
    H, W, m = R.CASES["61x83_area_7"]
    for min_area, present in ((7, True), (8, False), (0, True), (1, True)):
        got = _rows(m[None], [0], [0b10], [1], min_area)
        _check(got, R.seeds_rows(m[None], [0], [0b10], [1], min_area), H, W, "min_area %d" % min_area)
        assert (got[1][0] == 0) == present


@pytest.mark.parametrize("H,W", [(1025, 1024), (8, 1025), (8, 1)])
def test_refusals_write_nothing(H, W):
    """H*W > 2^20, W > 1024, W < 2: an error code, and no output is touched (the mask is never read either)."""
    from egne_amd import _lib
    L = _lib.lib()
    assert L.egne_mask_seed_workspace_bytes(1, H, W) < 0
    mask = torch.zeros((1, 2, 2), dtype=torch.int64, device=DEV)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)                 # noqa: E731
    fo, cb, sc = one(0), one(2), one(1)
    init = torch.full((1, 5), 77.0, dtype=torch.float64, device=DEV)
    ofo, ocl, status = one(77), one(77), one(77)
    stats = torch.full((1, 8), 77, dtype=torch.int64, device=DEV)
    ws = torch.full((64,), 77, dtype=torch.int64, device=DEV)
    rc = L.egne_ellipse_init_from_mask(mask.data_ptr(), 1, fo.data_ptr(), cb.data_ptr(), sc.data_ptr(), 1, H, W, MIN_AREA, init.data_ptr(),
                                       ofo.data_ptr(), ocl.data_ptr(), stats.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0
    for t in (init, ofo, ocl, status, stats, ws):
        assert bool((t == 77).all())
    with pytest.raises(ValueError):
        from egne_amd.utils import ellipse_seeds_from_mask
        ellipse_seeds_from_mask(torch.zeros((1, H, W), dtype=torch.int64, device=DEV))


# ---- the search on top ---------------------------------------------------------------------------------------------------------------
def _same_row(got, want):
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


def _ring_and_pupil():
    H, W = 240, 320
    ring = R.patterns(H, W)["ring_with_blob"]
    yy, xx = np.mgrid[0:H, 0:W]
    pupil = np.hypot(yy - (H - 1) / 2.0, xx - (W - 1) / 2.0) <= 0.12 * H
    a = ring.astype(np.int64) + (ring & pupil)                      # iris ring = class 1, pupil disc = class 2
    b = np.roll(np.roll(a, 17, axis=0), -31, axis=1)
    return np.stack([a, np.zeros_like(a), b])


def test_fit_from_mask_equals_the_oracle_search_on_the_device_seeds():
    from egne_amd.pipeline import WindowedFit
    from egne_amd.utils import ellipse_seeds_from_mask, fit_ellipses_from_mask
    from oracle import fit as ofit
    mask = _ring_and_pupil()
    m = torch.from_numpy(mask).to(DEV)
    init, fo, cl = (t.cpu().numpy() for t in ellipse_seeds_from_mask(m))
    assert fo.tolist() == [0, 0, -1, -1, 2, 2] and cl.tolist() == [1, 2] * 3
    fit = fit_ellipses_from_mask(m)
    assert fit.dtype == torch.float64 and tuple(fit.shape) == (3, 2, 5)
    got = fit.cpu().numpy().reshape(6, 5)
    for i in range(6):
        if fo[i] < 0:
            assert np.array_equal(got[i], np.full(5, -1.0)), (i, got[i])
            continue
        want = ofit.fit_ellipse(mask[fo[i]] == cl[i], list(init[i]))
        assert _same_row(got[i], want), "row %d: device %s, oracle %s" % (i, got[i].tolist(), want.tolist())
    out = torch.zeros((3, 2, 5), dtype=torch.float64, device=DEV)
    assert fit_ellipses_from_mask(m, out=out) is out and torch.equal(out, fit)
    h = WindowedFit(DEV, windowed=False).submit(m, None, seed="mask")
    h.synchronize()
    assert _same_row(h.result.cpu().numpy(), fit.cpu().numpy())
    with pytest.raises(ValueError):
        WindowedFit(DEV, windowed=False).submit(m, None, seed="canny")


# ---- script level --------------------------------------------------------------------------------------------------------------------
def _video(vid, tmp_path, nets, extra, method):
    """The ellipse dictionary of a run, equal to the one on disk (a class map without a region gives NaN rows: equal_nan)."""
    r = V.run(vid, tmp_path, nets, extra, method)
    V.same_ellipses(r.files[0], r.res, equal_nan=True)
    return r.res


def _equal(res_a, res_b):
    V.same_ellipses(res_a, res_b, equal_nan=True)


def test_video_mask_seed_same_ellipses_through_three_paths(tmp_path, nets):
    """--ellipse_seed mask on the clip of test_evaluate_video_end_to_end: the host path, --device_io 1 and --device_io 1 --low_latency 1
    (seed step inside the captured graph) write the same ellipses.  A first run calibrates the plans."""
    vid = V.clip(tmp_path)
    _video(vid, tmp_path, nets, ["--ellipse_seed", "mask"], "warm")
    host = _video(vid, tmp_path, nets, ["--ellipse_seed", "mask"], "host")
    dev = _video(vid, tmp_path, nets, ["--ellipse_seed", "mask", "--device_io", "1"], "dev")
    live = _video(vid, tmp_path, nets, ["--ellipse_seed", "mask", "--device_io", "1", "--low_latency", "1"], "live")
    assert set(k for k in host if isinstance(k, int)) == {0, 1, 2, 3} and all((j, i) in host for j in range(4) for i in range(2))
    for k in host:
        print(k, host[k][0].tolist(), dev[k][0].tolist(), live[k][0].tolist())
    _equal(host, dev)
    _equal(host, live)


def test_video_default_seed_is_pred(tmp_path, nets):
    """The flag left at its default writes what --ellipse_seed pred writes; --ellipse_seed mask writes something else."""
    from egne_amd import evaluate as E
    vid = V.clip(tmp_path)
    _video(vid, tmp_path, nets, [], "warm")
    a = _video(vid, tmp_path, nets, [], "default")
    b = _video(vid, tmp_path, nets, ["--ellipse_seed", "pred"], "pred")
    _equal(a, b)
    assert E.parse_args([]).ellipse_seed == "pred"
    c = _video(vid, tmp_path, nets, ["--ellipse_seed", "mask"], "mask")
    assert any(not np.array_equal(a[k][0], c[k][0], equal_nan=True) for k in a)


def test_deepvog_pupils_come_from_the_class_map(monkeypatch):
    """--model deepvog --ellipse_seed mask: pupil ellipses = fit_ellipses_from_mask of the class maps {0, 1 = pupil} with the model's
    regions, iris rows -1 five times."""
    from egne_amd import evaluate as E
    from egne_amd.utils import fit_ellipses_from_mask
    seen = []
    real = E.evaluate_ellseg_on_image

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(E, "evaluate_ellseg_on_image", spy)
    pup, iri = E.main(["--synthetic", "2", "--model", "deepvog", "--ellipse_seed", "mask"])
    edge, seg, pup2, iri2 = seen[0]
    assert np.array_equal(pup, pup2) and set(np.unique(seg)) <= {0, 1}
    assert np.array_equal(iri, np.full((2, 5), -1.0))
    want = fit_ellipses_from_mask(torch.from_numpy(np.ascontiguousarray(seg)).to(DEV), E.SEED_REGIONS["deepvog"]).cpu().numpy()
    assert np.array_equal(want[:, 0], iri) and _same_row(pup, want[:, 1])
    print("deepvog pupils from the class map:", pup.tolist(), "pupil pixels:", [int((s == 1).sum()) for s in seg])
