"""Host side of the device loader (egne_amd.loader): the NumPy restatement of the reference's item path against the fixture the
reference recorded (tests/golden/loader.npz, make_golden_loader.py), the raw datasets and the collate function.  No GPU."""
import numpy as np
import pytest

import loader_refs as R
from common import gold
from egne_amd import loader

GROUPS = [("p", n, case, R.SIZE_PLAIN, False) for n, case in enumerate(R.CASES_PLAIN)] + \
         [("s", n, case, R.SIZE_SCALED, R.SCALE) for n, case in enumerate(R.CASES_SCALED)]


@pytest.fixture(scope="module")
def fixture():
    return gold("loader")


def test_fixture_covers_what_it_should(fixture):
    sizes = {tuple(fixture["p%d_raw_img" % n].shape) for n in range(len(R.CASES_PLAIN))}
    assert sizes == {(24, 32), (20, 28), (16, 32)}
    conds = np.stack([fixture["p%d_raw_cond" % n] for n in range(len(R.CASES_PLAIN))])
    assert any(c[0] and c[2] and not c[3] for c in conds), "no sample with the pupil absent"
    assert any(c[2] and c[3] for c in conds), "no sample with both ellipses absent"
    assert any(c[1] for c in conds), "no sample with the mask absent"
    assert all(tuple(fixture["s%d_img" % n].shape) == (1, 24, 32) for n in range(len(R.CASES_SCALED)))


@pytest.mark.parametrize("group,n,case,size,scale", GROUPS, ids=["%s%d" % g[:2] for g in GROUPS])
def test_restatement_equals_the_reference(fixture, group, n, case, size, scale):
    """image, label, weights and distance maps bit-identical, centres exact, elNorm within one float32 ulp (both sides compute in
    float64 and round once), cond and imInfo exact, and the cv2 calls are handed what the reference hands them."""
    p = "%s%d_" % (group, n)
    sample = R.raw_case(*case)
    for a, name in zip(sample, ("raw_img", "raw_label", "raw_el", "raw_pc", "raw_cond", "raw_info")):
        assert np.array_equal(a, fixture[p + name]) and a.dtype == fixture[p + name].dtype, name
    out, calls = R.item(sample, size, scale)
    for name, a in zip(R.OUTPUTS, out):
        want = fixture[p + name]
        assert a.shape == want.shape and a.dtype == want.dtype, (name, a.dtype, want.dtype)
        if name == "elNorm":
            d = int(R.ulp32_distance(a, want).max())
            print("%s elNorm: %d ulp" % (p, d))
            assert d <= 1, "%s: elNorm %d float32 ulp from the reference" % (p, d)
        else:
            assert np.array_equal(a.view(np.uint8) if a.dtype.kind == "f" else a, want.view(np.uint8) if a.dtype.kind == "f" else want), name
    assert calls == list(fixture[p + "calls"])
    assert len(calls) == (4 if scale else 2)


def test_stage_geometry_equals_the_restatement():
    """loader.stage_geometry (pad shift, scale through the conic, scaleFn's first-ellipse quirk) next to the per-sample restatement."""
    for cases, size, scale in ((R.CASES_PLAIN, R.SIZE_PLAIN, False), (R.CASES_SCALED, R.SIZE_SCALED, R.SCALE)):
        raw = loader.collate_raw([R.raw_case(*c) for c in cases])
        el, pc = loader.stage_geometry(raw.elParam, raw.pupil_center, raw.src_hw, size, scale)
        for b, c in enumerate(cases):
            s = R.raw_case(*c)
            e, q = s[2].copy(), s[3].copy()
            up_r, up_c = (size[0] - s[0].shape[0]) // 2, (size[1] - s[0].shape[1]) // 2
            for k in range(2):
                if not np.all(e[k] == -1):
                    e[k, :2] += (up_c, up_r)
            if not np.all(q == -1):
                q = q + (up_c, up_r)
            if scale:
                first_absent = np.all(e[0] == -1)
                e = np.stack([e[0], e[0]]) if first_absent else np.stack([R.ellipse_transform(e[k], np.diag([scale, scale, 1.0])) for k in range(2)])
                q = q if np.all(q == -1) else scale * q
                if c[3] == "iris":
                    assert first_absent and np.all(el[b].numpy() == -1), "scaleFn's quirk: an absent first ellipse replaces the second"
            np.testing.assert_array_equal(pc[b].numpy(), q)
            for k in range(2):
                if np.all(e[k] == -1):
                    assert np.all(el[b, k].numpy() == -1)
                elif not np.all(s[2][k] == -1):       # (an absent second ellipse next to a present first one goes through the conic: cond masks it)
                    np.testing.assert_allclose(el[b, k].numpy(), e[k], rtol=1e-12, atol=1e-12)


def test_collate_raw_mixed_sizes():
    samples = [R.raw_case(*c) for c in R.CASES_PLAIN]
    raw = loader.collate_raw(samples)
    B = len(samples)
    assert raw.images.shape == (B, 24, 32) and raw.images.dtype == np.uint8 and raw.labels.shape == (B, 24, 32) and raw.labels.dtype == np.int8
    assert raw.src_hw.dtype == np.int32 and raw.src_hw.tolist() == [list(s[0].shape) for s in samples]
    assert raw.elParam.shape == (B, 2, 5) and raw.elParam.dtype == np.float64 and raw.pupil_center.shape == (B, 2)
    assert raw.cond.shape == (B, 4) and raw.cond.dtype == bool and raw.imInfo.shape == (B, 3) and raw.imInfo.dtype == np.int64
    for b, s in enumerate(samples):
        r, c = s[0].shape
        assert np.array_equal(raw.images[b, :r, :c], s[0]) and np.array_equal(raw.labels[b, :r, :c], s[1])
        assert not raw.images[b, r:].any() and not raw.images[b, :, c:].any() and not raw.labels[b, r:].any() and not raw.labels[b, :, c:].any()
        assert np.array_equal(raw.elParam[b], s[2]) and np.array_equal(raw.pupil_center[b], s[3]) and np.array_equal(raw.cond[b], s[4])


def test_raw_archive_round_trip(tmp_path):
    samples = [R.raw_case(7 + i, 20, 28) for i in range(3)]
    full = dict(Images=np.stack([s[0] for s in samples]), Masks_noSkin=np.stack([s[1] for s in samples]),
                pupil_loc=np.stack([s[3] for s in samples]), Fits_pupil=np.stack([s[2][1] for s in samples]),
                Fits_iris=np.stack([s[2][0] for s in samples]))
    np.savez(tmp_path / "full.npz", **full)
    ds = loader.RawArchive(str(tmp_path / "full.npz"))
    assert len(ds) == 3
    for i, s in enumerate(samples):
        got = ds[i]
        for a, b in zip(got[:5], s[:5]):
            assert np.array_equal(a, b) and a.dtype == b.dtype
        assert got[5].tolist() == [i, 0, 0] and got[5].dtype == np.int64
    # an EMPTY array means "absent for all frames" (readImage, CurriculumLib.py:182-185), and cond follows :189-193
    empty = dict(full, Masks_noSkin=np.zeros((0,), np.int8), pupil_loc=np.zeros((0, 2)), Fits_pupil=np.zeros((0, 5)))
    np.savez(tmp_path / "empty.npz", **empty)
    ds = loader.RawArchive(str(tmp_path / "empty.npz"), index=[2, 0])
    assert len(ds) == 2 and ds.imList[:, 0].tolist() == [2, 0]
    img, mask, el, pc, cond, info = ds[0]
    assert np.array_equal(img, samples[2][0]) and mask.dtype == np.int8 and mask.shape == img.shape and np.all(mask == -1)
    assert np.all(pc == -1) and np.all(el[1] == -1) and np.array_equal(el[0], samples[2][2][0])
    assert cond.tolist() == [True, True, True, False]
    # a mask of zeros counts as absent too
    np.savez(tmp_path / "zero.npz", **dict(full, Masks_noSkin=np.zeros_like(full["Masks_noSkin"])))
    assert loader.RawArchive(str(tmp_path / "zero.npz"))[1][4].tolist() == [False, True, False, False]
    with pytest.raises(ValueError, match="missing"):
        np.savez(tmp_path / "bad.npz", Images=full["Images"])
        loader.RawArchive(str(tmp_path / "bad.npz"))
    raw = loader.collate_raw([ds[0], ds[1]])
    assert raw.images.shape == (2, 20, 28)


def test_synthetic_raw_eyes_sizes():
    ds = loader.SyntheticRawEyes(4, seed=5, sizes=[(24, 32), (20, 28)], target=(24, 32))
    assert len(ds) == 4 and [ds[i][0].shape for i in range(4)] == [(24, 32), (20, 28), (24, 32), (20, 28)]
    img, mask, el, pc, cond, info = ds[1]                      # seed 6: every third seed has no pupil annotation
    assert img.dtype == np.uint8 and mask.dtype == np.int8 and set(np.unique(mask)) <= {0, 1, 2, 3} and el.shape == (2, 5)
    assert np.all(pc == -1) and np.all(el[1] == -1) and not np.all(el[0] == -1) and cond.tolist() == [True, False, True, False]
    assert ds.imList.shape == (4, 3)
    with pytest.raises(ValueError):
        loader.SyntheticRawEyes(1, sizes=[(26, 32)], target=(24, 32))


def test_script_flags():
    """--device_loader / --raw_archive: off by default, and the loader needs to be told where its data is."""
    from egne_amd.args import parse_args
    a = parse_args(["--synthetic", "4", "--setting", "configs/baseline_edge.yaml"])
    assert a.device_loader == 0 and a.raw_archive is None
    a = parse_args(["--device_loader", "1", "--raw_archive", "frames.npz", "--setting", "configs/baseline_edge.yaml"])
    assert a.device_loader == 1 and a.raw_archive == "frames.npz"
    with pytest.raises(SystemExit):
        parse_args(["--device_loader", "1", "--setting", "configs/baseline_edge.yaml"])


@pytest.mark.parametrize("hw", [(23, 32), (24, 31), (26, 32), (24, 34)])
def test_odd_or_negative_differences_are_refused(hw):
    """pad2Size asserts an even difference (helperfunctions.py:416-417); a frame larger than the canvas cannot be padded at all."""
    with pytest.raises(ValueError, match="pad2Size"):
        loader.pad_offsets(np.array([[24, 32], list(hw)]), (24, 32))
    with pytest.raises(ValueError, match="pad2Size"):
        loader.stage_geometry(-np.ones((1, 2, 5)), -np.ones((1, 2)), np.array([list(hw)]), (24, 32))
    with pytest.raises(ValueError, match="pad2Size"):
        R.item(R.raw_case(7, hw[0], hw[1]), (24, 32))
    with pytest.raises(ValueError, match="pad2Size"):         # refused on the host, before anything touches the device
        loader.device_batch(loader.collate_raw([R.raw_case(7, hw[0], hw[1])]), size=(24, 32))
    assert loader.pad_offsets(np.array([[20, 28]]), (24, 32)).tolist() == [[2, 2]]
