"""The OpenCV branches of the device augmentation (csrc/augment_cv.hip, egne_augment_cv; egne_amd.data_augment with on_cv2="device")
against the NumPy restatement in tests/augment_cv2_refs.py, byte for byte, and against what the reference itself decides
(tests/golden/augment_cv2.npz: draws, OpenCV arguments, geometry).  No tolerances anywhere."""
import hashlib

import numpy as np
import pytest
import torch

import augment_cv2_refs as R
from common import gold
from egne_amd import _lib, data_augment as DA, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch.device("cuda:0")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _params(B, shape):
    """The dict draw() fills, neutral."""
    return dict(sigma=np.zeros(B, np.int32), nlines=np.zeros(B, np.int32), segs=np.zeros((B, DA.MAX_LINES, 4)),
                rot=np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (B, 1)))


def _run(dev, img, lab, choice, cv):
    """egne_augment_cv on outputs that hold a copy (what egne_augment leaves for these frames); returns NumPy (image, label)."""
    img_d, lab_d = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    oi, ol = img_d.clone(), lab_d.clone()
    DA.augment_cv(img_d, lab_d, oi, ol, np.asarray(choice, np.int32), cv)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), ol.cpu().numpy()


def _frames(B, shape, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (B,) + shape).astype(np.uint8)
    lab = rng.randint(0, 4, (B,) + shape).astype(np.int64)
    lab[:, 0, 0] = 2 ** 40 + 3                                  # the label travels as int64
    return img, lab


@pytest.mark.parametrize("shape", [(5, 7), (33, 65), (17, 130), (240, 320)])
def test_blur(G, shape):
    """Every sigma at 5x7 (every pixel reflects), 33x65 (a tile and a partial one in both directions) and 17x130; one 240x320 frame.
    A frame of another choice in the same launch stays as it is."""
    sigmas = [3] if shape == (240, 320) else [2, 3, 4, 5, 6]
    B = len(sigmas) + 1
    img, lab = _frames(B, shape, 1)
    cv = _params(B, shape)
    cv["sigma"][:B - 1] = sigmas
    oi, ol = _run(G, img, lab, [1] * (B - 1) + [7], cv)
    for b, s in enumerate(sigmas):
        want = R.gaussian_blur(img[b], s)
        assert np.array_equal(oi[b], want), "sigma %d: %d pixels differ" % (s, (oi[b] != want).sum())
    assert np.array_equal(oi[B - 1], img[B - 1]) and np.array_equal(ol, lab)


ANGLES = (0.0, 30.0, -30.0, 13.7, -29.486)


@pytest.mark.parametrize("shape", [(9, 11), (33, 47), (240, 320)])
def test_rotation(G, shape):
    """Image (Lanczos) and label (nearest) at 9x11 (frame smaller than the tap footprint), 33x47 and 240x320."""
    B = len(ANGLES)
    img, lab = _frames(B, shape, 2)
    cv = _params(B, shape)
    for b, ang in enumerate(ANGLES):
        cv["rot"][b] = DA.invert_affine(DA.rotation_matrix(DA.rotation_centre(shape), np.deg2rad(ang)))
    oi, ol = _run(G, img, lab, [6] * B, cv)
    for b, ang in enumerate(ANGLES):
        wi, wl = R.rotate(img[b], lab[b], ang)
        assert np.array_equal(oi[b], wi), "angle %g: %d pixels differ" % (ang, (oi[b] != wi).sum())
        assert np.array_equal(ol[b], wl), "angle %g: %d labels differ" % (ang, (ol[b] != wl).sum())


def test_rotation_outside_the_staged_box(G):
    """A matrix that is no rotation (scale 3: the source box of a tile is wider than the staged one) takes the taps from memory."""
    shape = (70, 90)
    img, lab = _frames(1, shape, 3)
    M = np.array([[1 / 3.0, 0.02, 5.0], [-0.02, 1 / 3.0, 7.0]])
    cv = _params(1, shape)
    cv["rot"][0] = DA.invert_affine(M)
    oi, ol = _run(G, img, lab, [6], cv)
    assert np.array_equal(oi[0], R.warp_affine_lanczos4(img[0], M)) and np.array_equal(ol[0], R.warp_affine_nearest(lab[0], M))


def _line_sets(shape):
    H, W = shape
    tan = np.tan(np.pi / 2 - 1e-9)
    xc, yc = 0.5 * W + 0.5, 0.47 * H
    return [
        [(W // 8, H // 2, W - 5, H // 2 + 3)],                                                          # one segment
        [(3 * i, 1 + i, W - 5 - 2 * i, H - 2 - 2 * i) for i in range(9)],                               # nine
        [(-5000, H // 2 - 3000, 4000, H // 2 + 2400), (W // 2, -10 ** 6, W // 2 + 7, 10 ** 6)],         # end points far outside
        [(int(xc - 30.0), int(-30.0 * tan + yc), int(xc + 12.5), int(12.5 * tan + yc))],                # near-vertical
        [(W // 3, H // 3, W // 3, H // 3), (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1)],                 # zero length: discs
        [(-60, -30, -10, -9), (W + 10, 3, W + 90, 40), (5, H + 6, W, H + 6)],                           # all dropped
    ]


@pytest.mark.parametrize("shape", [(24, 40), (240, 320)])
def test_lines(G, shape):
    sets = _line_sets(shape)
    B = len(sets)
    img, lab = _frames(B, shape, 4)
    img[img == 255] = 254
    cv = _params(B, shape)
    for b, lines in enumerate(sets):
        cv["nlines"][b], cv["segs"][b] = DA.clip_segments(lines, shape)
    assert cv["nlines"].tolist() == [1, 9, 2, 1, 3, 0]
    oi, ol = _run(G, img, lab, [5] * B, cv)
    for b, lines in enumerate(sets):
        want = R.draw_lines(img[b], lines)
        assert np.array_equal(oi[b], want), "set %d: %d pixels differ" % (b, (oi[b] != want).sum())
        assert (want == 255).any() == (b != B - 1)
    assert np.array_equal(ol, lab)


def test_mixed_batch_and_throughput(G):
    """One augment_batch(on_cv2="device") over B = 16 frames with every branch twice and host-drawn noise: every frame equals the
    per-frame expectation (oracle restatement for the NumPy branches, tests/augment_cv2_refs.py for 1, 5, 6), geometry included, and
    the frames of the NumPy branches are what the default path (on_cv2="skip") computes for them.  Then the cost of a B = 256 batch
    with uniformly drawn branches, with and without the OpenCV branches (printed, not asserted)."""
    choices = list(range(8)) * 2
    samples = [synth.augment_case(7 + b % 6) for b in range(16)]
    img = torch.from_numpy(np.stack([s[0] for s in samples])).to(G)
    lab = torch.from_numpy(np.stack([s[1] for s in samples])).to(G)
    pcs = torch.from_numpy(np.stack([s[2] for s in samples]))
    els = torch.from_numpy(np.stack([s[3] for s in samples]))
    np.random.seed(11)
    oi, ol, pc, el, ch = DA.augment_batch(img, lab, pcs, els, choices=choices, host_noise=True, on_cv2="device")
    end_state = R.rng_state_hash()
    oi, ol = oi.cpu().numpy(), ol.cpu().numpy()
    assert ch.tolist() == choices
    np.random.seed(11)
    for b, s in enumerate(samples):
        before = np.random.get_state()
        wb, wm, wpc, (wp, wi) = R.augment(*s, choices[b])
        assert np.array_equal(oi[b], wb), "frame %d (branch %d): %d pixels differ" % (b, choices[b], (oi[b] != wb).sum())
        assert np.array_equal(ol[b], wm), "frame %d (branch %d): label" % (b, choices[b])
        assert np.array_equal(pc[b].numpy(), wpc) and np.array_equal(el[b].numpy(), np.stack([wp, wi])), "frame %d geometry" % b
        if choices[b] not in DA.CV2_CHOICES:                    # the parent's path on this frame, from the same generator state
            after = np.random.get_state()
            np.random.set_state(before)
            si, sl, spc, sel, _ = DA.augment_batch(img[b:b + 1], lab[b:b + 1], pcs[b:b + 1], els[b:b + 1], choices=[choices[b]],
                                                   host_noise=True, on_cv2="skip")
            assert np.array_equal(si[0].cpu().numpy(), oi[b]) and np.array_equal(sl[0].cpu().numpy(), ol[b])
            assert torch.equal(spc[0], pc[b]) and torch.equal(sel[0], el[b])
            np.random.set_state(after)
    assert R.rng_state_hash() == end_state
    # throughput, B = 256 at 240x320, branches uniform (device-drawn noise); "skip" is the path without the OpenCV branches
    B = 256
    big_i, big_l = img.repeat(B // 16, 1, 1), lab.repeat(B // 16, 1, 1)
    big_pc, big_el = pcs.repeat(B // 16, 1), els.repeat(B // 16, 1, 1)
    uniform = np.random.RandomState(5).randint(0, 8, B).tolist()
    fps = {}
    for mode in ("device", "skip"):
        for rep in range(2):                                    # the first call warms up (tables, allocator)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            DA.augment_batch(big_i, big_l, big_pc, big_el, choices=uniform, on_cv2=mode)
            e1.record()
            torch.cuda.synchronize()
        fps[mode] = B / (e0.elapsed_time(e1) * 1e-3)
    print("augment_batch B=256 240x320: on_cv2=device %.0f frames/s (%.2f ms), on_cv2=skip %.0f frames/s (%.2f ms)"
          % (fps["device"], 1e3 * B / fps["device"], fps["skip"], 1e3 * B / fps["skip"]))


def test_fixture_cases_through_augment(G):
    """augment(..., on_cv2="device") on the fixture's cases: the reference's geometry and generator state, the restatement's pixels."""
    g = gold("augment_cv2")
    for n, (choice, seed, npseed) in enumerate(g["cases"].tolist()):
        base, mask, pc, el = synth.augment_case(seed)
        np.random.seed(npseed)
        ob, om, opc, (pup, iri) = DA.augment(base, mask, pc, el, None if choice < 0 else choice, on_cv2="device")
        p = "c%d_" % n
        assert R.rng_state_hash() == str(g[p + "rng"])
        assert ob.dtype == np.uint8 and _sha(ob) == str(g[p + "img_sha"]), "case %d: %d pixels differ in the sampled rows" % (
            n, (ob[::16] != g[p + "img_rows"]).sum())
        assert _sha(om.astype(np.int64)) == str(g[p + "mask_sha"]), "case %d mask" % n
        assert np.array_equal(opc, g[p + "pc"]) and np.array_equal(np.stack([pup, iri]), g[p + "el"]), "case %d geometry" % n


def test_every_seed_returns(G):
    """The reference's own call (choice=None) returns for every seed with on_cv2="device"; three in eight raise by default."""
    base, mask, pc, el = synth.augment_case(8, 48, 64)
    firsts = set()
    for seed in range(24):
        np.random.seed(seed)
        ob, om, _, _ = DA.augment(base, mask, pc, el, on_cv2="device")
        assert ob.shape == base.shape and om.shape == mask.shape
        firsts.add(int(np.random.RandomState(seed).randint(0, 8)))
    assert firsts == set(range(8))


def test_error_paths(G):
    """Errors, not faults: a blurred 3x3 frame, in-place buffers, a sigma or a line count out of range."""
    img, lab = _frames(1, (3, 3), 6)
    cv = _params(1, (3, 3))
    cv["sigma"][0] = 3
    with pytest.raises(RuntimeError, match="H, W >= 4"):
        _run(G, img, lab, [1], cv)
    img, lab = _frames(1, (8, 8), 6)
    cv = _params(1, (8, 8))
    cv["sigma"][0] = 3
    i_d, l_d = torch.from_numpy(img).to(G), torch.from_numpy(lab).to(G)
    with pytest.raises(RuntimeError, match="in place"):
        DA.augment_cv(i_d, l_d, i_d, l_d.clone(), np.array([1], np.int32), cv)
    with pytest.raises(RuntimeError, match="in place"):
        DA.augment_cv(i_d, l_d, i_d.clone(), l_d, np.array([1], np.int32), cv)
    cv["sigma"][0] = 7
    with pytest.raises(RuntimeError, match="sigma"):
        _run(G, img, lab, [1], cv)
    cv["nlines"][0] = 10
    with pytest.raises(RuntimeError, match="lines"):
        _run(G, img, lab, [5], cv)
    torch.cuda.synchronize()
