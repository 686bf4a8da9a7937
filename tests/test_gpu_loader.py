"""The device-side training loader (csrc/loader.hip, egne_amd.loader): stage and finish kernels byte for byte against NumPy and the
existing device functions, device_batch against what the reference recorded (tests/golden/loader.npz) and against the step-by-step
composition of the public functions.  The only tolerance is the fixture's: elNorm within one float32 ulp."""
import numpy as np
import pytest
import torch

import loader_refs as R
from common import gold
from egne_amd import _lib, data_augment as DA, dataprep, evaluate, loader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch.device("cuda:0")


def _raw_frames(sizes, R_, C_, seed):
    """A [B,R_,C_] raw buffer whose frames hold random pixels and labels -1..3 and whose padding holds GARBAGE (it must be ignored)."""
    rng = np.random.RandomState(seed)
    B = len(sizes)
    img = np.full((B, R_, C_), 0xAB, np.uint8)
    lab = np.full((B, R_, C_), 0x55, np.int8)
    srcs = []
    for b, (r, c) in enumerate(sizes):
        si, sl = rng.randint(0, 256, (r, c)).astype(np.uint8), rng.randint(-1, 4, (r, c)).astype(np.int8)
        img[b, :r, :c], lab[b, :r, :c] = si, sl
        srcs.append((si, sl))
    return img, lab, np.array(sizes, np.int32), srcs


def _padded(src, size):
    ur, uc = (size[0] - src.shape[0]) // 2, (size[1] - src.shape[1]) // 2
    return np.pad(src, ((ur, ur), (uc, uc)))


def _stage(G, img, lab, hw, size, scale=False):
    oi, ol = loader.stage(torch.from_numpy(img).to(G), torch.from_numpy(lab).to(G), hw, size, scale)
    torch.cuda.synchronize()
    assert oi.dtype == torch.uint8 and ol.dtype == torch.int64
    return oi.cpu().numpy(), ol.cpu().numpy()


# canvas, sources: 24x36 (rows of 4 1/2 eight-pixel chunks: per-pixel stores), 24x40 and 32x48 (whole chunks: 8-byte image and 16-byte
# label stores; sources narrower than the canvas), 24x20 (the last chunk of a row is half filled, the raw buffer is wider than the canvas)
STAGE_CASES = [((24, 36), [(24, 36), (20, 28), (16, 36), (24, 20), (2, 2)]),
               ((24, 40), [(24, 36), (20, 28), (16, 36), (24, 20), (2, 2)]),
               ((32, 48), [(24, 36), (20, 28), (16, 36), (24, 20), (2, 2)]),
               ((24, 20), [(24, 20), (20, 12), (16, 20), (24, 4), (2, 2)]),
               ((24, 36), [(20, 28)])]


@pytest.mark.parametrize("size,sizes", STAGE_CASES, ids=["%dx%d_B%d" % (s + (len(z),)) for s, z in STAGE_CASES])
def test_stage_pads_like_numpy(G, size, sizes):
    img, lab, hw, srcs = _raw_frames(sizes, 24, 36, 3)
    oi, ol = _stage(G, img, lab, hw, size)
    assert oi.shape == (len(sizes),) + size
    for b, (si, sl) in enumerate(srcs):
        assert np.array_equal(oi[b], _padded(si, size)), "frame %d image" % b
        assert np.array_equal(ol[b], _padded(sl, size).astype(np.int64)), "frame %d label" % b


def test_stage_refuses_what_pad2size_asserts(G):
    img, lab, hw, _ = _raw_frames([(24, 36), (19, 28)], 24, 36, 4)
    with pytest.raises(ValueError, match="pad2Size"):
        loader.stage(torch.from_numpy(img).to(G), torch.from_numpy(lab).to(G), hw, (24, 36))
    with pytest.raises(ValueError, match="pad2Size"):
        loader.stage(torch.from_numpy(img).to(G), torch.from_numpy(lab).to(G), np.array([[24, 36], [20, 28]]), (22, 36))
    with pytest.raises(ValueError, match="raw buffer"):
        loader.stage(torch.from_numpy(img).to(G), torch.from_numpy(lab).to(G), np.array([[24, 36], [26, 36]]), (26, 36))


def test_stage_scaled(G):
    """scale 0.5, 48x64 -> 24x32: the image byte-identical to resize_lanczos4 of the PADDED frame, the label to resize_nearest, -1
    kept through the int64 conversion.  A second factor resizes to odd extents (0.4: 19x25)."""
    size = (48, 64)
    img, lab, hw, srcs = _raw_frames([(48, 64), (44, 60), (40, 64), (2, 2)], 48, 64, 5)
    for scale in (0.5, 0.4):
        dsize = (int(scale * size[1]), int(scale * size[0]))
        oi, ol = _stage(G, img, lab, hw, size, scale)
        assert oi.shape == (4, dsize[1], dsize[0])
        for b, (si, sl) in enumerate(srcs):
            assert np.array_equal(oi[b], evaluate.resize_lanczos4(_padded(si, size), dsize)), "scale %s frame %d image" % (scale, b)
            want = evaluate.resize_nearest(_padded(sl, size), dsize).astype(np.int64)
            assert np.array_equal(ol[b], want), "scale %s frame %d label" % (scale, b)
        assert (ol == -1).any()


@pytest.mark.parametrize("shape", [(3, 24, 32), (2, 5, 7), (2, 240, 320), (1, 3, 6)])
def test_finish(G, shape):
    """Label remap on -1, 0..3 and 7; z-score bit-identical to dataprep.zscore of the float image (the same float64 statistics, the
    same order of additions), a constant image included (whatever zscore yields there).  5x7: an odd pixel count (no wide accesses)."""
    rng = np.random.RandomState(6)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    img[-1] = 93                                            # a constant image
    lab = rng.choice(np.array([-1, 0, 1, 2, 3, 7], np.int64), shape)
    lab.reshape(-1)[:6] = [-1, 0, 1, 2, 3, 7]
    img_d = torch.from_numpy(img).to(G)
    x, ol = loader.finish(img_d, torch.from_numpy(lab).to(G))
    want_x = dataprep.zscore(img_d.float())
    torch.cuda.synchronize()
    assert x.shape == (shape[0], 1) + shape[1:] and x.dtype == torch.float32 and ol.dtype == torch.int64
    want_l = lab.copy()
    want_l[lab == 1], want_l[lab == 2], want_l[lab == 3] = 0, 1, 2
    assert np.array_equal(ol.cpu().numpy(), want_l)
    assert torch.equal(x.reshape(shape).view(torch.int32), want_x.reshape(shape).view(torch.int32))
    assert torch.isfinite(x[:-1]).all()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a,
                                                                         b.view(np.uint8) if b.dtype.kind == "f" else b)


@pytest.mark.parametrize("group", ["plain", "scaled"])
def test_device_batch_equals_the_reference(G, group):
    """Augmentation off, against what the reference's own __getitem__ returned for the same raw samples: same tolerances as the host
    test of the restatement (bits everywhere, elNorm within one float32 ulp); the spatial weights are dataprep.spatial_weights of
    the remapped label."""
    g = gold("loader")
    p, cases, size, scale = ("p", R.CASES_PLAIN, R.SIZE_PLAIN, False) if group == "plain" else ("s", R.CASES_SCALED, R.SIZE_SCALED, R.SCALE)
    raw = loader.collate_raw([R.raw_case(*c) for c in cases])
    out = loader.device_batch(raw, size=size, scale=scale, augment=False)
    sw = dataprep.spatial_weights(out[1])
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in out) and torch.equal(out[2], sw)
    for b in range(len(cases)):
        for name, t in zip(R.OUTPUTS, out):
            got, want = t[b].cpu().numpy(), g["%s%d_%s" % (p, b, name)]
            if name == "elNorm":
                d = int(R.ulp32_distance(got, want).max())
                print("%s%d elNorm: %d ulp" % (p, b, d))
                assert got.dtype == want.dtype and d <= 1, "sample %d: elNorm %d float32 ulp from the reference" % (b, d)
            else:
                if not _same_bits(got, want) and got.shape == want.shape:
                    at = np.argwhere(got != want)[:5]
                    print("%s%d %s: %d values differ (%d more only in the sign of zero), first at %s: %s / %s"
                          % (p, b, name, int((got != want).sum()), int((np.signbit(got) != np.signbit(want)).sum()) if got.dtype.kind == "f" else 0,
                             at.tolist(), [got[tuple(i)] for i in at], [want[tuple(i)] for i in at]))
                assert _same_bits(got, want), "sample %d: %s differs from the reference" % (b, name)


def test_device_batch_is_the_composition_of_its_stages(G):
    """Augmentation on (one frame per branch, host-drawn parameters, fixed seed): every tensor equals the public functions applied one
    after the other in the reference's order -- pad, augment the STORED labels, remap and z-score, weights and distance maps, and the
    geometry normalised AFTER the augmentation moved it."""
    choices = [0, 1, 2, 3, 5, 6, 7]
    size = (48, 64)
    cases = [(7, 48, 64, None), (8, 44, 60, None), (9, 48, 64, "pupil"), (10, 40, 64, None), (11, 48, 60, "ellipses"), (13, 48, 64, "mask"),
             (14, 46, 62, None)]
    samples = [R.raw_case(*c) for c in cases]
    raw = loader.collate_raw(samples)
    np.random.seed(77)
    out = loader.device_batch(raw, size=size, augment=True, choices=choices, on_cv2="device", host_noise=True)
    # step by step
    B = len(cases)
    img0 = torch.from_numpy(np.stack([_padded(s[0], size) for s in samples])).to(G)
    lab0 = torch.from_numpy(np.stack([_padded(s[1], size) for s in samples]).astype(np.int64)).to(G)
    el0, pc0 = np.stack([s[2] for s in samples]), np.stack([s[3] for s in samples])
    for b, s in enumerate(samples):
        shift = np.array([(size[1] - s[0].shape[1]) // 2, (size[0] - s[0].shape[0]) // 2], np.float64)
        for k in range(2):
            if not np.all(el0[b, k] == -1):
                el0[b, k, :2] += shift
        if not np.all(pc0[b] == -1):
            pc0[b] += shift
    np.random.seed(77)
    img1, lab1, pc1, el1, ch = DA.augment_batch(img0, lab0, torch.from_numpy(pc0), torch.from_numpy(el0), choices, host_noise=True, on_cv2="device")
    assert list(ch) == choices
    assert not torch.equal(img1, img0) and not torch.equal(lab1, lab0) and not torch.equal(el1, torch.from_numpy(el0))
    lab2 = torch.where((lab1 >= 1) & (lab1 <= 3), lab1 - 1, lab1)
    cond = torch.from_numpy(raw.cond).to(G)
    gone = cond[:, [3, 2]][..., None]
    el_d, pc_d = el1.to(G), pc1.to(G)
    eln = torch.where(gone, -torch.ones_like(el_d), dataprep._ellipse_info(torch.where(gone, torch.ones_like(el_d), el_d), size[0], size[1]))
    want = (dataprep.zscore(img1.float()).reshape(B, 1, *size), lab2, dataprep.spatial_weights(lab2), dataprep.dist_maps(lab2), pc_d.float(),
            torch.where(cond[:, 3:4], pc_d, el_d[:, 0, :2]).float(), eln.float(), cond, torch.from_numpy(raw.imInfo).to(G))
    torch.cuda.synchronize()
    for name, a, b in zip(R.OUTPUTS, out, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
        assert same, "%s differs from the step-by-step composition" % name
    assert (out[1] == -1).any() and not (out[1] == 3).any()


def test_device_batch_ransac_targets(G):
    """ellipse="ransac": centres, elNorm and cond are dataprep.ellipse_targets of the labels the batch itself holds."""
    ds = loader.SyntheticRawEyes(2, seed=21)
    raw = loader.collate_raw([ds[0], ds[1]])
    out = loader.device_batch(raw, ellipse="ransac")
    pc, ic, eln, cond = dataprep.ellipse_targets(out[1])
    torch.cuda.synchronize()
    assert out[0].shape == (2, 1, 240, 320) and out[7].dtype == torch.bool
    for name, a, b in (("pupil_center", out[4], pc), ("iris_center", out[5], ic), ("elNorm", out[6], eln), ("cond", out[7].float(), cond)):
        assert torch.equal(a, b), name
    with pytest.raises(ValueError):
        loader.device_batch(raw, ellipse="fit")
