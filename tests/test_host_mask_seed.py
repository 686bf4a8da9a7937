"""CPU: the NumPy restatement of the mask seeds (tests/mask_seed_refs.py) against scipy's labelling, what the moment seed recovers of
drawn ellipses, and why the seed matters to the search (oracle.fit.fit_ellipse keeps the centre and walks the axes by at most a pixel
per sweep)."""
import numpy as np
import pytest

import mask_seed_refs as R


def _iou(a, b):
    return np.count_nonzero(a & b) / np.count_nonzero(a | b)


def _raster(el, H=240, W=320):
    from oracle import fit as ofit
    return np.array(ofit.ell_inside((H, W), [el[0], el[1], el[2], el[3], el[4] * 180.0 / ofit.PI_REF], ofit.mesh_f32(H, W)))


@pytest.fixture(scope="module")
def drawn():
    return R.drawn_ellipses()


def test_components_equal_scipy_label():
    ndi = pytest.importorskip("scipy.ndimage")
    for name, (H, W, m) in R.CASES.items():
        want, n = ndi.label(m == 1, structure=np.ones((3, 3)))
        got = R.components8(m == 1)
        assert got.max() == n and np.array_equal(got, want), name


def test_every_pattern_family_is_present_and_stats_are_consistent():
    names = set(k.split("_", 1)[1] for k in R.CASES)
    assert names >= {"empty", "one_pixel", "full", "two_equal_blobs", "diagonal_join", "comb", "spiral", "checkerboard", "ring_with_blob",
                     "straddle", "borders", "noise_0.4", "noise_0.6", "area_6", "area_7"}
    H, W, m = R.CASES["240x320_two_equal_blobs"]
    st = R.seed_stats(m == 1, 7)
    assert st[6] == 2 and st[0] * 2 == st[7] and st[2] < st[0] * H // 2          # the raster-first (upper) blob won the tie
    assert R.seed_stats(R.CASES["3x5_diagonal_join"][2] == 1, 1)[6] == 1
    assert R.seed_stats(R.CASES["240x320_checkerboard"][2] == 1, 7)[6] == 1
    assert R.seed_stats(R.CASES["61x83_area_6"][2] == 1, 7)[0] == 0 and R.seed_stats(R.CASES["61x83_area_7"][2] == 1, 7)[0] == 7
    assert np.array_equal(R.seed_from_stats(R.seed_stats(R.CASES["64x64_empty"][2] == 1, 7), 64, 64), np.full(5, -1.0))


def test_region_bits_and_batch_rows():
    m = np.arange(40, dtype=np.int64).reshape(1, 5, 8) - 4              # ids -4 .. 35: outside 0..31 never belongs
    reg = R.region_of(m[0], 0xffffffff)
    assert np.array_equal(reg, (m[0] >= 0) & (m[0] < 32))
    assert np.array_equal(R.region_of(m[0], 0b101000), (m[0] == 3) | (m[0] == 5))
    init, fo, cl, st = R.seeds_rows(m, [0, 7, 0], [0b110000, 0b10, 0], [3, 1, 2], 1)       # ids 4 and 5 are neighbours
    assert fo.tolist() == [0, -1, -1] and cl.tolist() == [3, 1, 2] and st[0, 0] == 2 and not st[1:].any()
    assert np.array_equal(init[1:], np.full((2, 5), -1.0))


def test_moment_seed_recovers_drawn_ellipses(drawn):
    """12 drawn ellipses at 240x320 with a 7x9 stray blob and a stray pixel.  Measured with this restatement: centre within 0.066 px,
    axes within 0.091 px, angle within 0.58 degrees, IoU of the seed against the clean ellipse >= 0.9953, after the oracle's search
    >= 0.9953.  The bounds are the issue's (about 2.5 times its own measurement: 0.071 px, 0.097 px, 0.86 degrees, 0.9854, 0.9951)."""
    from oracle import fit as ofit
    worst = dict(centre=0.0, axes=0.0, angle=0.0, iou_seed=1.0, iou_fit=1.0)
    for true, clean, dirty in drawn:
        st = R.seed_stats(dirty, 7)
        assert st[6] == 3 and st[0] == np.count_nonzero(clean)
        seed = R.seed_from_stats(st, 240, 320)
        dth = (seed[4] - true[4] + np.pi / 2) % np.pi - np.pi / 2
        fit = ofit.fit_ellipse(dirty, list(seed))
        worst["centre"] = max(worst["centre"], float(np.abs(seed[:2] - true[:2]).max()))
        worst["axes"] = max(worst["axes"], float(np.abs(seed[2:4] - true[2:4]).max()))
        worst["angle"] = max(worst["angle"], float(np.degrees(abs(dth))))
        worst["iou_seed"] = min(worst["iou_seed"], _iou(_raster(seed), clean))
        worst["iou_fit"] = min(worst["iou_fit"], _iou(_raster(fit), clean))
    print("moment seed, extremes over the 12 cases:", worst)
    assert worst["centre"] <= 0.25 and worst["axes"] <= 0.25 and worst["angle"] <= 2.0
    assert worst["iou_seed"] >= 0.97 and worst["iou_fit"] >= 0.99


def test_random_axes_seed_leaves_the_search_short(drawn):
    """Why the feature exists: the true centre with DeepVOG-style uniform [0,1) axes and angle (normalised units, un-normalised as
    evaluate.py does it) ends below IoU 0.9 after the oracle's search on at least half of the same masks."""
    from oracle import fit as ofit
    rng = np.random.RandomState(1)
    H, W = 240, 320
    Hm = np.array([[W / 2, 0, W / 2], [0, H / 2, H / 2], [0, 0, 1.0]])
    ious = []
    for true, clean, dirty in drawn:
        a, b, th = rng.rand(3)
        seed = ofit.transform(np.array([2 * true[0] / W - 1, 2 * true[1] / H - 1, a, b, th]), Hm)
        ious.append(_iou(_raster(ofit.fit_ellipse(dirty, list(seed))), clean))
    print("random-axes seed, IoU after the search:", np.round(ious, 3))
    assert sum(v < 0.9 for v in ious) >= len(ious) // 2
