"""Host side of the OpenCV branches of the augmentation (egne_amd.data_augment with on_cv2="device") against the reference's own
decisions (tests/golden/augment_cv2.npz), and the NumPy restatement of the pixels (tests/augment_cv2_refs.py) against independent
statements, so that a wrong restatement cannot vouch for the kernels in tests/test_gpu_augment_cv2.py.  CPU only; every comparison
is exact."""
from fractions import Fraction

import numpy as np
import pytest

import augment_cv2_refs as R
from common import gold
from egne_amd import data_augment as DA, synth


def fixture_cases():
    g = gold("augment_cv2")
    for n, (choice, seed, npseed) in enumerate(g["cases"].tolist()):
        yield n, choice, seed, npseed, {k[len("c%d_" % n):]: g[k] for k in g.files if k.startswith("c%d_" % n)}


def test_draws_arguments_and_geometry_equal_the_reference():
    """draw(on_cv2="device") makes the reference's draws (same generator state afterwards), derives the arguments the reference hands
    to OpenCV (sigma; truncated end points before clipping; centre and angle) and rotate_geometry returns the reference's centre and
    ellipse arrays bit for bit -- including the rotated (-1, -1) centre and untouched -1 angle of an absent ellipse.  The constants
    the restatement assumes are the ones the reference passed: 7x7 kernel, colour 255, thickness 4, scale 1, LANCZOS4 for the image
    and NEAREST for the mask, dsize (W, H)."""
    seen = set()
    for n, choice, seed, npseed, f in fixture_cases():
        base, mask, pc, el = synth.augment_case(seed)
        H, W = base.shape
        np.random.seed(npseed)
        cv = {}
        ch, param, lut, noise = DA.draw(1, base.shape, None if choice < 0 else [choice], host_noise=True, on_cv2="device", cv2_params=cv)
        assert R.rng_state_hash() == str(f["rng"]), "case %d leaves another np.random state" % n
        k = choice if choice >= 0 else -1 - choice
        assert ch[0] == k
        seen.add((k, choice < 0))
        assert f["dtypes"].tolist() == ["uint8", "int64", "float64", "float64", "float64"]
        want_pc, want_el = f["pc"], f["el"]
        if k == 1:
            assert cv["sigma"][0] == int(f["sigma"]) and f["ksize"].tolist() == [7, 7]
        if k == 5:
            assert np.array_equal(np.array(cv["lines"][0], np.int64).reshape(-1, 4), f["lines"])
            assert (f["colour"] == 255).all() and (f["thickness"] == 4).all() and 1 <= len(f["lines"]) <= DA.MAX_LINES
        if k == 6:
            assert cv["ang_deg"][0] == float(f["angle"]) and list(cv["centre"]) == f["centre"].tolist() and float(f["scale"]) == 1.0
            assert f["flags"].tolist() == [4, 0] and f["dsize"].tolist() == [[W, H], [W, H]]
            got_pc, pup, iri = DA.rotate_geometry(pc, el[0], el[1], cv["ang_rad"][0], cv["centre"])
            assert np.array_equal(got_pc, want_pc) and np.array_equal(np.stack([pup, iri]), want_el)
            if seed % 3 == 0:                                   # absent pupil: centre rotated all the same, the rest stays -1
                assert not np.array_equal(want_el[0, :2], [-1, -1]) and (want_el[0, 2:] == -1).all()
        else:
            assert np.array_equal(want_pc, pc) and np.array_equal(want_el, el)
    assert seen == {(k, r) for k in (1, 5, 6) for r in (False, True)}


def test_fixture_pixels_are_the_restatement():
    """The image / mask hashes of the fixture are restatement-derived (its ``pixels_from`` says so): R.augment reproduces them."""
    assert "NOT OpenCV" in str(gold("augment_cv2")["pixels_from"])
    for n, choice, seed, npseed, f in fixture_cases():
        if n % 3 and choice >= 0:
            continue                                           # (a subset: one explicit case per branch and every drawn one)
        base, mask, pc, el = synth.augment_case(seed)
        np.random.seed(npseed)
        ob, om, opc, (pup, iri) = R.augment(base, mask, pc, el, None if choice < 0 else choice)
        assert np.array_equal(ob[::16], f["img_rows"]) and np.array_equal(om[::16], f["mask_rows"])
        assert np.array_equal(opc, f["pc"]) and np.array_equal(np.stack([pup, iri]), f["el"])
        assert R.rng_state_hash() == str(f["rng"])


def test_blur_tables():
    want = {2: [18, 34, 49, 54, 49, 34, 18], 3: [27, 36, 42, 46, 42, 36, 27], 4: [31, 36, 40, 42, 40, 36, 31],
            5: [33, 36, 39, 40, 39, 36, 33], 6: [34, 37, 38, 38, 38, 37, 34]}
    for s, q in want.items():
        assert DA.gaussian_q8(s).tolist() == q and sum(q) == 256
    assert np.array_equal(DA.gaussian_q8_tables(), np.array([want[s] for s in range(2, 7)]))


@pytest.mark.parametrize("shape", [(5, 7), (33, 65), (240, 320)])
def test_blur_restatement_vs_scipy(shape):
    """Independent route: scipy.ndimage.correlate1d(mode="mirror") on int64 along each axis with the same taps, same rounding."""
    from scipy.ndimage import correlate1d
    rng = np.random.RandomState(shape[0])
    img = rng.randint(0, 256, shape).astype(np.uint8)
    for sigma in range(2, 7):
        q = DA.gaussian_q8(sigma).astype(np.int64)
        s = correlate1d(correlate1d(img.astype(np.int64), q, axis=1, mode="mirror"), q, axis=0, mode="mirror")
        assert np.array_equal(R.gaussian_blur(img, sigma), ((s + 32768) >> 16).astype(np.uint8))
        for v in (0, 1, 200, 255):
            flat = np.full(shape, v, np.uint8)
            assert np.array_equal(R.gaussian_blur(flat, sigma), flat)


def test_phase_table():
    t = DA.lanczos4_phase_table()
    assert t.shape == (32, 8) and t.dtype == np.float64
    assert t[0, 3] == 1.0 and np.abs(np.delete(t[0], 3)).max() < 1e-16
    assert np.allclose(t[16, :4], [-0.01263, 0.05976, -0.16601, 0.61888], atol=5e-6) and np.array_equal(t[16], t[16, ::-1])
    from egne_amd import evaluate
    idx, w = evaluate.lanczos4_table(4, 8)                     # the same expression: output 1 of a 2x upscale sits at phase 8
    assert np.array_equal(w[1], t[8])


def test_rotation_restatement_properties():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (33, 47)).astype(np.uint8)
    lab = rng.randint(0, 4, (33, 47)).astype(np.int64)
    oi, ol = R.rotate(img, lab, 0.0)
    assert np.array_equal(oi, img) and np.array_equal(ol, lab)
    # 90 degrees: OpenCV's positive angle is counter-clockwise (origin top-left), as np.rot90(m, 1)
    sq = rng.randint(0, 256, (9, 9)).astype(np.uint8)
    sl = rng.randint(1, 4, (9, 9)).astype(np.int64)
    oi, ol = R.rotate(sq, sl, 90.0)
    assert np.array_equal(oi, np.rot90(sq, 1)) and np.array_equal(ol, np.rot90(sl, 1))
    # the label only holds source values and 0 (nearest, constant border)
    lab7 = 7 * (1 + rng.randint(0, 3, (33, 47))).astype(np.int64)
    for ang in (-30.0, 13.7, 30.0):
        _, ol = R.rotate(img, lab7, ang)
        assert set(np.unique(ol).tolist()) <= {0, 7, 14, 21} and (ol == 0).any()


@pytest.mark.parametrize("ang", [-30.0, 13.7, 30.0])
def test_rotation_matrix_convention_matches_the_reference_geometry(ang):
    """A bright 5x5 block centred on pupil_c lands with its intensity centroid within 0.5 px of the reference's rotated pupil_c."""
    H, W = 120, 160
    pc = np.array([101.0, 47.0])
    img = np.zeros((H, W), np.uint8)
    img[45:50, 99:104] = 255
    out, _ = R.rotate(img, np.zeros((H, W), np.int64), ang)
    y, x = np.mgrid[0:H, 0:W]
    wsum = out.astype(np.float64).sum()
    cen = np.array([(out * x).sum() / wsum, (out * y).sum() / wsum])
    el = np.array([101.0, 47.0, 5.0, 4.0, 0.3])
    got, _, _ = DA.rotate_geometry(pc, el, el, np.deg2rad(ang), DA.rotation_centre((H, W)))
    assert np.abs(cen - got).max() < 0.5, (cen, got)


def _capsule_exact(shape, lines):
    H, W = shape
    hit = np.zeros((H, W), bool)
    for x1, y1, x2, y2 in lines:
        dx, dy = Fraction(x2 - x1), Fraction(y2 - y1)
        len2 = dx * dx + dy * dy
        for y in range(H):
            for x in range(W):
                px, py = Fraction(x - x1), Fraction(y - y1)
                t = Fraction(0) if len2 == 0 else min(max((px * dx + py * dy) / len2, Fraction(0)), Fraction(1))
                ex, ey = px - t * dx, py - t * dy
                hit[y, x] |= ex * ex + ey * ey <= 4
    return hit


LINE_SHAPE = (24, 40)
_xc, _yc, _tan = 20.5, 11.25, np.tan(np.pi / 2 - 1e-9)
LINE_CASES = {
    "horizontal": [(5, 12, 30, 12)],
    "diagonal": [(5, 3, 30, 20)],
    "near_vertical": [(int(_xc - 30.0), int((-30.0) * _tan + _yc), int(_xc + 12.5), int(12.5 * _tan + _yc))],
    "zero_length": [(17, 9, 17, 9)],
    "outside": [(-60, -30, -10, -9), (50, 3, 90, 40)],
    "partly_outside": [(-40, 2, 25, 15), (38, -20, 33, 60)],
    "nine": [(3 * i, 1 + i, 35 - 2 * i, 22 - 2 * i) for i in range(9)],
}


@pytest.mark.parametrize("name", sorted(LINE_CASES))
def test_lines_restatement_vs_exact_capsule(name):
    """The float64 capsule test (through the host's clipping, as the product runs it) equals the definition evaluated in exact
    rational arithmetic on the reference's integer end points; clipping leaves the frame's pixels as the unclipped segment has them."""
    lines = LINE_CASES[name]
    img = np.full(LINE_SHAPE, 7, np.uint8)
    got = R.draw_lines(img, lines)
    want = np.where(_capsule_exact(LINE_SHAPE, lines), 255, 7).astype(np.uint8)
    assert np.array_equal(got, want)
    n, _ = DA.clip_segments(lines, LINE_SHAPE)
    if name == "outside":
        assert n == 0 and (got == 7).all()
    if name != "near_vertical":                                # moderate end points: the unclipped float64 test is well conditioned
        assert np.array_equal(R.draw_lines(img, lines, clip=False), got)
    else:
        assert abs(lines[0][1]) > 10 ** 9 and (got == 255).any()


def test_default_modes_are_untouched():
    base = synth.augment_case(8)[0]
    for c in DA.CV2_CHOICES:
        with pytest.raises(NotImplementedError):
            DA.draw(1, base.shape, [c])
        with pytest.raises(NotImplementedError):
            DA.draw(1, base.shape, [c], on_cv2="raise")
        ch, param, lut, noise = DA.draw(1, base.shape, [c], on_cv2="skip")
        assert ch[0] == 7 and param[0] == 0 and noise is None
    assert DA.CV2_CHOICES == (1, 5, 6) and len(DA.draw(2, base.shape, [7, 0])) == 4
    for seed in range(12):
        first = int(np.random.RandomState(seed).randint(0, 8))
        if first in DA.CV2_CHOICES:
            np.random.seed(seed)
            with pytest.raises(NotImplementedError):
                DA.draw(1, base.shape)
            np.random.seed(seed)
            assert DA.draw(1, base.shape, on_cv2="skip")[0][0] == 7
            np.random.seed(seed)
            assert DA.draw(1, base.shape, on_cv2="device")[0][0] == first
