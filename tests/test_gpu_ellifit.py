"""-m gpu: ElliFit + RANSAC on class-map boundaries (csrc/ellifit.hip) against the reference's own outputs
(tests/golden/ellifit.npz, written by tests/golden/make_golden_ellifit.py) and the NumPy restatement in tests/ellifit_refs.py.

Integers (points, N, best iteration, inlier count, candidate count, generated draws, status bits) must be equal.  Floats follow the
rule of the fixture: the truth is the reference's formulas applied in float64 to the exact-rational Phi of the chosen point set, the
reference's own deviation from that truth is stored per case, and the device must stay within 16 times that deviation, with the
largest deviation of any case as the floor (16: the device sums in another order and factorises instead of inverting).  The error
and verify figures are compared relative to the reference's at 1e-9: both are means of a few hundred O(1) terms of a model that
is within 1e-13 of the reference's, and the decisions they feed have gaps of 1e-6 (error) or are re-tested as integers.
Measured on an MI355X when this was written: worst ratio of a parameter's deviation to its bound 0.06 on the all-points fits
(largest deviation 3.6e-14 px against the reference's own 5.7e-14 on that case) and 0.12 on the RANSAC winners; in generated
mode the largest difference to the restatement was 3.4e-13 against a tolerance of 4.0e-12."""
import os

import numpy as np
import pytest
import torch

import ellifit_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ellifit.npz"))


@pytest.fixture(scope="module")
def nets():
    from common import bdcn_module, esf_module
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device(DEV)
    return bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()


KEYS = ("init", "frame_of", "cls", "raw", "stats_i", "stats_f", "status", "points", "draws")


def call(mask, **kw):
    """utils.ellipse_ransac_from_mask(return_stats=True) -> dict of host arrays."""
    from egne_amd.utils import ellipse_ransac_from_mask
    res = ellipse_ransac_from_mask(torch.from_numpy(np.ascontiguousarray(mask).astype(np.int64)).to(DEV), return_stats=True, **kw)
    torch.cuda.synchronize()
    return dict(zip(KEYS, (r.cpu().numpy() for r in res)))


def groups(fx):
    """Fixture cases grouped by map shape: one call per group, one frame per case (its region is the call's region for ALL frames, so
    a case is row (frame = its index in the group, region = its own) -- regions are per call, hence one call per distinct region)."""
    out = {}
    for i in range(len(fx["case_names"])):
        m = fx["map%d" % fx["case_map"][i]]
        key = (m.shape, int(fx["case_bits"][i]), int(fx["case_cls"][i]), int(fx["case_excl"][i]))
        out.setdefault(key, []).append(i)
    return out


def run_cases(fx, iters):
    """Every fixture case through the device with the recorded draws: {case index: row dict}."""
    n_min, thres, n_good = int(fx["params"][0]), float(fx["params"][2]), int(fx["params"][3])
    rows = {}
    for (shape, cb, sc, eb), idx in groups(fx).items():
        masks = np.stack([fx["map%d" % fx["case_map"][i]] for i in idx])
        kw = dict(regions=((cb, sc, eb),), n_min=n_min, iters=iters, thres=thres, n_good=n_good)
        if iters >= 0:
            kw["draws"] = np.maximum(np.stack([fx["draws"][i][:iters + 1] for i in idx]), 0)      # (-1 rows: N <= n_min, never read)
        res = call(masks, **kw)
        assert res["status"][0] == 0
        for k, i in enumerate(idx):
            rows[i] = {key: res[key][k] for key in KEYS if key != "status"}
    return rows


@pytest.fixture(scope="module")
def device_rows(fx):
    return run_cases(fx, int(fx["params"][1]))


def bounds(fx):
    ok = fx["valid"]
    par_floor = max(np.max(fx["dev_par"][ok]), np.max(fx["dev_par_all"]))
    return np.maximum(16 * fx["dev_par"].max(axis=1), par_floor), np.maximum(16 * fx["dev_par_all"].max(axis=1), par_floor)


# ---- boundary points -----------------------------------------------------------------------------------------------------------------
def _points_equal(res, masks, regions, max_pts):
    Rn = len(regions)
    for i in range(len(masks) * Rn):
        f, r = divmod(i, Rn)
        reg = tuple(regions[r]) + (0,) * (3 - len(regions[r]))
        want = R.boundary_points(masks[f], reg[0], reg[2]) if reg[0] else np.zeros((0, 2), np.int64)
        assert res["stats_i"][i, 0] == len(want), (i, res["stats_i"][i, 0], len(want))
        k = min(len(want), max_pts)
        assert np.array_equal(res["points"][i, :k], want[:k]), i
        assert np.all(res["points"][i, k:] == -1), i


@pytest.mark.parametrize("shape", [(24, 40), (70, 130), (240, 320)], ids=lambda s: "%dx%d" % s)
def test_boundary_points(fx, shape):
    H, W = shape
    rng = np.random.default_rng(H)
    names = list(fx["case_names"])
    maps = [fx["map%d" % fx["case_map"][i]].astype(np.int64) for i in range(len(names)) if fx["map%d" % fx["case_map"][i]].shape == shape][:3]
    if shape != (240, 320):
        odd = maps[0].copy()
        odd[rng.random(shape) < 0.1] = 40                      # ids outside 0..31: never in a region, never exclude
        odd[rng.random(shape) < 0.1] = -3
        maps.append(odd)
    if shape == (24, 40):
        maps.append((rng.random(shape) < 0.6).astype(np.int64) * 2)      # Bernoulli noise
        maps.append(fx["map%d" % fx["case_map"][names.index("alledges")]].astype(np.int64))
    masks = np.stack(maps)
    regions = ((0b110, 1, 0), (0b100, 2, 0b001), (0b010, 1, 0b100), (0b10, 1), (0, 1))
    res = call(masks, regions=regions, iters=-1)
    assert res["status"][0] == 0
    _points_equal(res, masks, regions, 4096)


def test_boundary_points_beyond_max_pts(fx):
    rng = np.random.default_rng(3)
    noise = (rng.random((24, 40)) < 0.6).astype(np.int64) * 2           # ~500 boundary points
    small = fx["map%d" % fx["case_map"][list(fx["case_names"]).index("small_iris")]].astype(np.int64)
    masks = np.stack([noise, small])
    regions = ((0b100, 2, 0),)
    assert len(R.boundary_points(noise, 0b100)) > 256 > len(R.boundary_points(small, 0b100)) >= 7
    res = call(masks, regions=regions, iters=-1, max_pts=256)
    assert res["status"][0] == 2
    assert res["frame_of"].tolist() == [-1, 1] and np.all(res["init"][0] == -1) and np.all(res["raw"][0] == -1)
    _points_equal(res, masks, regions, 256)
    want = R.ransac_from_mask(masks, regions, iters=-1, max_pts=256)
    assert want["status"] == 2 and want["frame_of"].tolist() == [-1, 1]


def test_largest_sizes_and_the_large_lds_path(fx):
    """1024 x 1000 (16 words per row, 64 words per thread of the scan) with 4290 boundary points: absent at the default max_pts,
    fitted at max_pts = 16384, where the fit kernel's LDS (67 088 bytes) needs its limit raised.  Float rule as for the fixture, with
    the truth and the reference's deviation computed here (1.7e-12 px on this set)."""
    H, W = 1024, 1000
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def inside(cx, cy, a, b, t):
        dx, dy = xx - cx, yy - cy
        return ((dx * np.cos(t) + dy * np.sin(t)) / a) ** 2 + ((dy * np.cos(t) - dx * np.sin(t)) / b) ** 2 <= 1

    m = np.zeros((H, W), np.int64)
    m[inside(500, 510, 495, 470, 0.4)] = 1
    m[inside(480, 500, 300, 250, -0.3)] = 2
    regions = ((0b010, 1, 0),)
    pts = R.boundary_points(m, 0b010)
    N = len(pts)
    assert 4096 < N < 16384
    small = call(m[None], regions=regions, iters=-1)
    assert small["status"][0] == 2 and small["frame_of"].tolist() == [-1] and small["stats_i"][0, 0] == N
    res = call(m[None], regions=regions, iters=-1, max_pts=16384)
    assert res["status"][0] == 0 and res["stats_i"][0].tolist() == [N, -1, N, 1] and res["frame_of"].tolist() == [0]
    assert np.array_equal(res["points"][0, :N], pts) and np.all(res["points"][0, N:] == -1)
    _, ref_model, ok = R.fit(pts)
    truth = R.model_of_phi(*R.exact_phi(pts))
    bound = max(16 * np.max(np.abs(ref_model - truth)), np.max(fx["dev_par"]), np.max(fx["dev_par_all"]))
    dev = np.max(np.abs(res["raw"][0] - truth))
    print("1024x1000, %d points: deviation %.2e, reference %.2e, bound %.2e" % (N, dev, np.max(np.abs(ref_model - truth)), bound))
    assert ok and dev <= bound
    a = call(m[None], regions=regions, max_pts=16384, seed=3)
    b = call(m[None], regions=regions, max_pts=16384, seed=3)
    assert a["status"][0] == 0 and np.array_equal(a["draws"][0], R.generated_draws(3, 0, N))
    assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS)
    # a row gives the same bits whatever the cap
    frame = _frames(fx, (24, 40))
    c, d = call(frame, seed=1), call(frame, seed=1, max_pts=16384)
    assert all(c[k].tobytes() == d[k].tobytes() for k in KEYS if k != "points")


# ---- fits ----------------------------------------------------------------------------------------------------------------------------
def test_all_points_fit(fx):
    rows = run_cases(fx, -1)
    _, bound_all = bounds(fx)
    worst = 0.0
    for i, name in enumerate(fx["case_names"]):
        row, N = rows[i], int(fx["ints"][i, 0])
        assert row["stats_i"][0] == N, name
        ref = fx["model_all_ref"][i]
        if N < 7 or np.all(ref == -1):
            assert row["frame_of"] == -1 and np.all(row["raw"] == -1) and np.all(row["init"] == -1), name
            continue
        assert row["frame_of"] >= 0 and tuple(row["stats_i"][1:]) == (-1, N, 1), (name, row["stats_i"])
        dev = np.max(np.abs(row["raw"] - fx["model_all_truth"][i]))
        print("%-16s all-points: deviation %.2e, bound %.2e" % (name, dev, bound_all[i]))
        worst = max(worst, dev / bound_all[i])
        assert dev <= bound_all[i], (name, dev, bound_all[i])
        assert np.allclose(row["init"], R.to_search(row["raw"], *fx["map%d" % fx["case_map"][i]].shape), rtol=1e-12, atol=1e-12), name
    print("worst ratio to the bound: %.3f" % worst)


def test_ransac_with_the_recorded_draws(fx, device_rows):
    bound, _ = bounds(fx)
    worst = 0.0
    for i, name in enumerate(fx["case_names"]):
        row = device_rows[i]
        print("%-16s device %s reference %s" % (name, row["stats_i"].tolist(), fx["ints"][i].tolist()))
        if not fx["valid"][i]:
            assert row["frame_of"] == -1 and np.all(row["raw"] == -1) and row["stats_i"][0] == fx["ints"][i, 0], name
            continue
        assert row["stats_i"].tolist() == fx["ints"][i].tolist(), name          # N, best iteration, |I|, candidates
        assert row["frame_of"] >= 0 and row["cls"] == fx["case_cls"][i]
        dev = np.max(np.abs(row["raw"] - fx["model_truth"][i]))
        worst = max(worst, dev / bound[i])
        assert dev <= bound[i], (name, dev, bound[i])
        assert abs(row["stats_f"][0] - fx["flt"][i, 0]) <= 1e-9 * fx["flt"][i, 0], name
        assert abs(row["stats_f"][1] - fx["flt"][i, 1]) <= 1e-9 * max(1.0, abs(fx["flt"][i, 1])), name
        H, W = fx["map%d" % fx["case_map"][i]].shape
        assert np.allclose(row["init"], R.to_search(row["raw"], H, W), rtol=1e-12, atol=1e-12), name
    print("worst ratio to the bound: %.3f" % worst)


def test_absent_direct_and_lane_stride_cases(fx, device_rows):
    names = list(fx["case_names"])
    r6 = device_rows[names.index("pts6")]
    assert r6["stats_i"].tolist() == [6, -1, 0, 0] and r6["frame_of"] == -1 and np.all(r6["init"] == -1)
    assert np.isinf(r6["stats_f"]).all()
    for n in (7, 15):
        r = device_rows[names.index("pts%d" % n)]
        assert r["stats_i"].tolist() == [n, -1, n, 1] and r["frame_of"] >= 0          # the direct fit: no iteration runs
    for n in (16, 65, 129):
        r = device_rows[names.index("pts%d" % n)]
        assert r["stats_i"].tolist() == fx["ints"][names.index("pts%d" % n)].tolist()


def test_drawn_ellipses(fx, device_rows):
    """Centre and semi-axes within 1.5 px of the drawn values (the reference's own worst case on these is below 1.07); the angle of
    the search-convention form against the drawn one on the eccentric ones."""
    names = list(fx["case_names"])
    seen = 0
    for f, name in enumerate(fx["frame_names"]):
        if not fx["frame_full"][f]:
            continue
        for r, part in enumerate(("iris", "pupil")):
            row, drawn = device_rows[names.index("%s_%s" % (name, part))], fx["frame_drawn"][f, r]
            assert max(abs(row["raw"][0] - drawn[0]), abs(row["raw"][1] - drawn[1])) <= 1.5
            assert np.max(np.abs(np.sort(row["raw"][2:4]) - np.sort(drawn[2:4]))) <= 1.5
            if abs(drawn[2] - drawn[3]) >= 5:
                t = drawn[4] if drawn[2] >= drawn[3] else drawn[4] + np.pi / 2
                assert abs((row["init"][4] - t + np.pi / 2) % np.pi - np.pi / 2) < 0.1
            seen += 1
    assert seen == 10


# ---- draws ---------------------------------------------------------------------------------------------------------------------------
def _frames(fx, shape):
    return np.stack([fx["map%d" % m].astype(np.int64) for m in fx["frame_map"] if fx["map%d" % m].shape == shape])


def test_table_mode_errors(fx):
    masks = _frames(fx, (70, 130))[:2]
    n = 4
    good = np.stack([R.generated_draws(1, i, 40, 15, 40) for i in range(n)])          # indices below 40: inside every row's list
    assert call(masks, draws=good)["status"][0] == 0
    for what, (row, it, slot, val) in (("repeated", (1, 3, 5, None)), ("out of range", (2, 40, 0, 10 ** 6)), ("negative", (0, 0, 14, -1))):
        bad = good.copy()
        bad[row, it, slot] = bad[row, it, slot - 1] if val is None else val
        res = call(masks, draws=bad)
        assert res["status"][0] & 1, what
        assert res["frame_of"][row] == -1 and np.all(res["init"][row] == -1), what
        others = [i for i in range(n) if i != row]
        assert np.all(res["frame_of"][others] >= 0), what


def test_generated_mode(fx):
    masks = _frames(fx, (70, 130))
    a = call(masks, seed=7)
    b = call(masks, seed=7)
    want = R.ransac_from_mask(masks, seed=7)
    assert a["status"][0] == 0 and want["status"] == 0
    assert np.array_equal(a["draws"], want["draws"])                                  # the generator, integer for integer
    assert np.array_equal(a["stats_i"], want["stats_i"]) and np.array_equal(a["frame_of"], want["frame_of"])
    ok = want["frame_of"] >= 0
    assert ok.sum() >= 8
    # restatement (the reference's operation order) and device each deviate from the rational solve by at most the fixture's bound
    tol = 17 * max(np.max(fx["dev_par"]), np.max(fx["dev_par_all"]))
    print("largest difference to the restatement %.2e, tolerance %.2e" % (np.max(np.abs(a["raw"][ok] - want["raw"][ok])), tol))
    assert np.allclose(a["raw"][ok], want["raw"][ok], rtol=0, atol=tol) and np.allclose(a["init"][ok], want["init"][ok], rtol=0, atol=2 * tol)
    assert np.allclose(a["stats_f"][ok], want["stats_f"][ok], rtol=1e-9, atol=1e-12)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k                                    # a second call repeats every bit
    c = call(masks, seed=8)
    assert not np.array_equal(a["draws"], c["draws"])


def test_generated_draws_that_run_out(fx):
    """n_min = 64 of 65 points: 256 attempts seldom reach 64 distinct indices.  Such an iteration is written as -1 to draws_out,
    sets status bit 0 and makes the row absent; the other iterations hold the generator's indices."""
    names = list(fx["case_names"])
    m = fx["map%d" % fx["case_map"][names.index("pts65")]].astype(np.int64)
    want = R.generated_draws(5, 0, 65, 64, 40, partial=True)
    assert np.any(want[:, 0] < 0) and np.any(want[:, 0] >= 0)
    res = call(m[None], regions=((1 << 3, 1, 0),), n_min=64, n_good=64, seed=5)
    assert res["status"][0] == 1 and res["frame_of"].tolist() == [-1] and np.all(res["init"] == -1)
    assert np.array_equal(res["draws"][0], want)


def test_batch_position(fx, device_rows):
    """A row alone and the same row inside a batch of 66 rows (33 frames at 24x40): identical bits."""
    names = list(fx["case_names"])
    i_iris, i_pup = names.index("small_iris"), names.index("small_pupil")
    small = fx["map%d" % fx["case_map"][i_iris]].astype(np.int64)
    rng = np.random.default_rng(9)
    batch = np.stack([np.roll(small, (int(rng.integers(-2, 3)), int(rng.integers(-3, 4))), axis=(0, 1)) for _ in range(33)])
    batch[20] = small
    # the other rows: indices below 16, inside the list of every row that iterates at all (N > 15)
    draws = np.stack([R.generated_draws(1, k, 16, 15, 40) for k in range(66)])
    draws[40], draws[41] = fx["draws"][i_iris], fx["draws"][i_pup]
    big = call(batch, draws=draws)
    one = call(small[None], draws=draws[40:42])
    assert big["status"][0] == 0 and one["status"][0] == 0
    for k in ("init", "raw", "stats_i", "stats_f", "cls", "points"):
        assert big[k][40:42].tobytes() == one[k].tobytes(), k
    assert big["frame_of"][40:42].tolist() == [20, 20] and one["frame_of"].tolist() == [0, 0]
    assert one["raw"][0].tobytes() == device_rows[i_iris]["raw"].tobytes()


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def _same(got, want):
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


def test_fit_from_mask_with_ransac_seeds(fx):
    from egne_amd.pipeline import WindowedFit
    from egne_amd.utils import ellipse_ransac_from_mask, fit_ellipses, fit_ellipses_from_mask
    masks = _frames(fx, (240, 320))
    empty = np.zeros_like(masks[:1])
    m = torch.from_numpy(np.concatenate([masks[:1], empty, masks[1:]])).to(DEV)
    init, fo, cl = (t.cpu().numpy() for t in ellipse_ransac_from_mask(m))
    assert fo.tolist() == [0, 0, -1, -1, 2, 2] and cl.tolist() == [1, 2] * 3
    fit = fit_ellipses_from_mask(m, seed_kind="ransac")
    assert fit.dtype == torch.float64 and tuple(fit.shape) == (3, 2, 5)
    got = fit.cpu().numpy().reshape(6, 5)
    keep = fo >= 0
    want = fit_ellipses(m, fo[keep], cl[keep], init[keep])
    assert _same(got[keep], want) and np.all(got[~keep] == -1)
    h = WindowedFit(DEV, windowed=False).submit(m, None, seed="ransac")
    h.synchronize()
    assert _same(h.result.cpu().numpy(), fit.cpu().numpy())
    with pytest.raises(TypeError):
        fit_ellipses_from_mask(m, seed=3)
    with pytest.raises(ValueError):
        fit_ellipses_from_mask(m, seed_kind="canny")


def test_video_ransac_seed_same_ellipses_and_frames_through_three_paths(tmp_path, nets):
    """--ellipse_seed ransac on the clip of tests/test_gpu_mask_seed.py: the host path, --device_io 1 and --device_io 1 --low_latency 1
    (the whole estimator inside the captured graph) write the same ellipses; what they write is neither what pred nor what mask
    writes.  The frames handed to both video writers are byte-identical between --device_io 0 and 1 at the same --low_latency, as
    tests/test_gpu_evalio.py has it for pred: the edge network's map itself differs in a few bytes between a batch of the whole clip
    and a frame pair, whatever the seeds are."""
    import video_harness as V
    vid = V.clip(tmp_path)
    flag = ["--ellipse_seed", "ransac"]
    V.run(vid, tmp_path, nets, flag, "warm")
    host = V.run(vid, tmp_path, nets, flag, "host")
    dev = V.run(vid, tmp_path, nets, flag + ["--device_io", "1"], "dev")
    host1 = V.run(vid, tmp_path, nets, flag + ["--low_latency", "1"], "host1")
    live = V.run(vid, tmp_path, nets, flag + ["--device_io", "1", "--low_latency", "1"], "live")
    assert all((j, i) in host.res for j in range(4) for i in range(2))
    V.same_frames(host, dev)
    V.same_frames(host1, live)
    assert set(host.res) == set(live.res)
    for k in host.res:
        for e_a, e_b in zip(host.res[k], live.res[k]):
            assert np.array_equal(e_a, e_b), (k, e_a, e_b)
    for other in ("pred", "mask"):
        res = V.run(vid, tmp_path, nets, ["--ellipse_seed", other], other).res
        assert any(not np.array_equal(host.res[k][0], res[k][0], equal_nan=True) or not np.array_equal(host.res[k][1], res[k][1], equal_nan=True)
                   for k in host.res), other


@pytest.mark.parametrize("model", ["ritnet_v2", "deepvog"])
def test_evaluate_main_ransac_ellipses_come_from_the_class_map(monkeypatch, model):
    """evaluate.py --ellipse_seed ransac [--model deepvog]: the reported ellipses are fit_ellipses_from_mask(class maps,
    seed_kind="ransac") with the model's regions (deepvog: class map {0, 1 = pupil}, no iris row)."""
    from egne_amd import evaluate as E
    from egne_amd.utils import fit_ellipses_from_mask
    seen = []
    real = E.evaluate_ellseg_on_image

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(E, "evaluate_ellseg_on_image", spy)
    pup, iri = E.main(["--synthetic", "2", "--model", model, "--ellipse_seed", "ransac"])
    edge, seg, pup2, iri2 = seen[0]
    assert np.array_equal(pup, pup2, equal_nan=True) and np.array_equal(iri, iri2, equal_nan=True)
    regions = E.RANSAC_REGIONS[model]
    assert (regions is None) == (model == "ritnet_v2")
    want = fit_ellipses_from_mask(torch.from_numpy(np.ascontiguousarray(seg)).to(DEV), regions, seed_kind="ransac").cpu().numpy()
    assert _same(iri, want[:, 0]) and _same(pup, want[:, 1])
    if model == "deepvog":
        assert set(np.unique(seg)) <= {0, 1} and np.array_equal(iri, np.full((2, 5), -1.0))
        # (seeded random weights: the pupil rows may well be absent too -- what the rows were made of is in the statistics)
        st = call(seg, regions=regions)["stats_i"]
        assert st[0::2, 0].tolist() == [0, 0] and st[1::2, 0].tolist() == [len(R.boundary_points(m, 0b010)) for m in seg]
    else:
        assert np.any(pup != -1) and np.any(iri != -1)


# ---- targets and training --------------------------------------------------------------------------------------------------------------
def test_ellipse_targets(fx):
    """dataprep.ellipse_targets against get_ellipse_info / the acceptance rule run by the reference on the fixture's frames.  The
    outputs are float32: 4 float32 ulps of max(1, |value|) -- the float64 deviations behind them (1e-13 px before the 2/W scaling)
    are nine orders below that."""
    from egne_amd import dataprep
    names = list(fx["case_names"])
    for shape in ((240, 320), (70, 130), (24, 40)):
        sel = [f for f in range(len(fx["frame_names"])) if fx["map%d" % fx["frame_map"][f]].shape == shape]
        masks = np.stack([fx["map%d" % fx["frame_map"][f]].astype(np.int64) for f in sel])
        draws = np.maximum(np.stack([fx["draws"][names.index("%s_%s" % (fx["frame_names"][f], p))] for f in sel for p in ("iris", "pupil")]), 0)
        pc, ic, el, cond = (t.cpu().numpy() for t in dataprep.ellipse_targets(torch.from_numpy(masks).to(DEV), draws=draws))
        assert pc.dtype == ic.dtype == el.dtype == cond.dtype == np.float32 and el.shape == (len(sel), 2, 5) and cond.shape == (len(sel), 4)
        assert np.array_equal(cond, fx["tg_cond"][sel].astype(np.float32))
        for got, want in ((pc, fx["tg_pc"][sel]), (ic, fx["tg_ic"][sel]), (el, fx["tg_el"][sel])):
            want = want.astype(np.float32)
            tol = 4 * np.finfo(np.float32).eps * np.maximum(1.0, np.abs(want))
            assert np.all(np.abs(got - want) <= tol), (shape, got, want)
        rpc, ric, rel, rcond = R.ellipse_targets(masks, draws=draws)
        assert np.array_equal(rcond, cond) and np.allclose(rel, el, rtol=0, atol=1e-6)
    speck = list(fx["frame_names"]).index("speck")
    assert fx["tg_cond"][speck].tolist() == [0, 0, 1, 0]          # the centroid fallback: pupil fit rejected, centre kept


def test_ellipse_targets_of_absent_parts(fx):
    """Frames without what the contract needs: all background (no centre, no ellipse: every flag set, -1 everywhere), an iris with
    no pupil pixel (iris kept, pupil centre -1), and a 2 x 3 pupil alone (too few boundary points: centroid for both centres)."""
    from egne_amd import dataprep
    names = list(fx["case_names"])
    full = fx["map%d" % fx["case_map"][names.index("full2_iris")]].astype(np.int64)
    no_pupil = np.where(full == 2, 1, full)
    tiny = np.zeros_like(full)
    tiny[30:32, 60:63] = 2
    masks = np.stack([np.zeros_like(full), no_pupil, tiny, full])
    i_iris, i_pup = names.index("full2_iris"), names.index("full2_pupil")
    draws = np.maximum(np.stack([fx["draws"][i_iris], fx["draws"][i_pup]] * 4), 0)
    assert len(R.boundary_points(no_pupil, 0b110)) == fx["ints"][i_iris, 0]          # same iris outline: the recorded draws fit
    pc, ic, el, cond = (t.cpu().numpy() for t in dataprep.ellipse_targets(torch.from_numpy(masks).to(DEV), draws=draws))
    assert cond.tolist() == [[1, 1, 1, 1], [1, 0, 1, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    assert np.all(pc[0] == -1) and np.all(ic[0] == -1) and np.all(el[0] == -1)
    assert np.all(pc[1] == -1) and np.all(el[1, 1] == -1) and np.all(el[1, 0] != -1) and np.all(ic[1] > 0)
    assert pc[2].tolist() == [61.0, 30.5] and ic[2].tolist() == [61.0, 30.5] and np.all(el[2] == -1)
    rpc, ric, rel, rcond = R.ellipse_targets(masks, draws=draws)
    assert np.array_equal(rcond, cond)
    for got, want in ((pc, rpc), (ic, ric), (el, rel)):
        assert np.all(np.abs(got - want) <= 4 * np.finfo(np.float32).eps * np.maximum(1.0, np.abs(want)))
    assert np.array_equal(el[1, 0], el[3, 0])          # the iris row does not depend on the pupil


def test_train_py_device_prep_3(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from egne_amd import train as TR
    TR.main(["--synthetic", "4", "--batchsize", "2", "--epochs", "1", "--setting", "configs/baseline_edge.yaml", "--device_prep", "3",
             "--expname", "e"])
    ck = torch.load(os.path.join("logs", "ritnet_v2", "e", "weights", "ritnet_v2_0.pkl"), map_location="cpu")
    bad = [k for k, v in ck["state_dict"].items() if torch.is_floating_point(v) and not torch.isfinite(v).all()]
    assert not bad, bad[:5]
