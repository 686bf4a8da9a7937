"""ElliFit + RANSAC (csrc/ellifit.hip), everything that runs without a GPU: the NumPy restatement against the outputs of
the reference itself (tests/golden/ellifit.npz), its boundary rule against scipy, the draw generator, the conditions the fixture
promises, the workspace-size entry point, and the kernels' own arithmetic (csrc/ellifit_core.h) compiled into a stand-alone host
program under -fsanitize=address,undefined.

Float tolerance of the device's Fit (the host program runs the same text, sums in list order): the truth is the exact-rational Phi
and the reference's formulas applied to it in float64; the reference's own deviation from that truth is in the fixture; the code
must stay within 16 times that deviation per case, with the largest deviation of any case as the floor.  Measured here: the host
build's worst ratio to that bound is printed by test_host_fit_within_the_reference_bound (0.24 for Phi, 0.23 for the parameters
when this was written)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ellifit_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "edge-guided-near-eye-image-analysis-for-head-mounted-displays_amd", "csrc")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ellifit.npz"))


def case_points(fx, i):
    return fx["pts%d" % i].astype(np.int64)


def bounds(fx):
    """Per-case tolerances of the float rule: (Phi relative to max|Phi|, parameters absolute) for the best set and the all-points set."""
    ok = fx["valid"]
    phi_floor = max(np.max(fx["flt"][ok, 4]), np.max(fx["flt"][np.isfinite(fx["flt"][:, 5]), 5]))
    par_floor = max(np.max(fx["dev_par"][ok]), np.max(fx["dev_par_all"]))
    return (np.maximum(16 * fx["flt"][:, 4], phi_floor), np.maximum(16 * fx["dev_par"].max(axis=1), par_floor),
            np.maximum(16 * fx["flt"][:, 5], phi_floor), np.maximum(16 * fx["dev_par_all"].max(axis=1), par_floor))


def test_restatement_reproduces_the_reference(fx):
    n_min, iters, thres, n_good = int(fx["params"][0]), int(fx["params"][1]), float(fx["params"][2]), int(fx["params"][3])
    for i, name in enumerate(fx["case_names"]):
        pts = case_points(fx, i)
        m = fx["map%d" % fx["case_map"][i]]
        assert np.array_equal(R.boundary_points(m, int(fx["case_bits"][i]), int(fx["case_excl"][i])), pts), name
        res = R.ransac(pts, fx["draws"][i], n_min, iters, thres, n_good)
        assert (len(pts), res["best_iter"], res["n_inl"], res["n_cand"]) == tuple(fx["ints"][i]), name
        assert res["valid"] == bool(fx["valid"][i]), name
        assert np.array_equal(res["model"], fx["model"][i]), name          # the reference's operations in its order: every bit
        if res["valid"]:
            assert res["error"] == fx["flt"][i, 0], name
            assert np.array_equal(res["inliers"], fx["inl%d" % i]), name
            assert abs(R.verify(res["model"], pts) - fx["flt"][i, 1]) <= 1e-12 * max(1.0, abs(fx["flt"][i, 1])), name
        if len(pts) >= 7:
            Phi, model, _ = R.fit(pts)
            assert np.array_equal(Phi, fx["phi_all_ref"][i]) and np.array_equal(model, fx["model_all_ref"][i]), name


def test_fixture_conditions(fx):
    names = list(fx["case_names"])
    ints, flt = fx["ints"], fx["flt"]
    assert np.all(flt[:, 2] >= 1e-6) and np.all(flt[:, 3] >= 1e-6)
    counts = {n: int(ints[names.index(n), 0]) for n in ("pts6", "pts7", "pts15", "pts16", "pts65", "pts129")}
    assert counts == {"pts6": 6, "pts7": 7, "pts15": 15, "pts16": 16, "pts65": 65, "pts129": 129}
    assert not fx["valid"][names.index("pts6")]
    for n in ("pts7", "pts15"):
        assert ints[names.index(n), 1] == -1 and ints[names.index(n), 3] == 1          # the direct fit
    assert np.all(fx["draws"][names.index("pts15")] == -1) and np.all(fx["draws"][names.index("pts16")] >= 0)
    m = fx["map%d" % fx["case_map"][names.index("alledges")]]
    assert np.all(m[0] == 1) and np.all(m[-1] == 1) and np.all(m[:, 0] == 1) and np.all(m[:, -1] == 1)
    assert os.path.getsize(os.path.join(HERE, "golden", "ellifit.npz")) < 256 * 1024
    # the centroid fallback is exercised: a pupil fit the acceptance rule rejects next to an accepted iris
    assert any(c[2] == 1 and c[3] == 0 for c in fx["tg_cond"])
    # every stored deviation of the reference from the rational solve is tiny next to a wrong term (1e-3 and above)
    assert np.max(flt[fx["valid"], 4]) < 1e-9 and np.max(fx["dev_par"]) < 1e-9


def test_drawn_ellipses_reference_recipe(fx):
    names = list(fx["case_names"])
    for f, name in enumerate(fx["frame_names"]):
        if not fx["frame_full"][f]:
            continue
        for r, part in enumerate(("iris", "pupil")):
            mod, drawn = fx["model"][names.index("%s_%s" % (name, part))], fx["frame_drawn"][f, r]
            assert max(abs(mod[0] - drawn[0]), abs(mod[1] - drawn[1])) <= 1.5
            assert np.max(np.abs(np.sort(mod[2:4]) - np.sort(drawn[2:4]))) <= 1.5


def test_boundary_is_region_minus_its_erosion():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    cross = ndi.generate_binary_structure(2, 1)
    for H, W, p in ((24, 40, 0.5), (24, 40, 0.9), (70, 130, 0.7), (2, 2, 0.5), (3, 65, 0.8)):
        m = (rng.random((H, W)) < p).astype(np.int64) * 2
        m[rng.random((H, W)) < 0.05] = 40          # ids outside 0..31 are never in a region
        m[rng.random((H, W)) < 0.05] = -3
        region = m == 2
        want = region & ~ndi.binary_erosion(region, structure=cross, border_value=1)
        r, c = np.nonzero(want)
        assert np.array_equal(R.boundary_points(m, 0b100), np.stack([c, r], axis=1))
        # exclude bits: no pixel of the 3x3 neighbourhood in an excluded class (here class 0)
        near0 = ndi.binary_dilation(m == 0, structure=np.ones((3, 3), bool))
        r, c = np.nonzero(want & ~near0)
        assert np.array_equal(R.boundary_points(m, 0b100, 0b001), np.stack([c, r], axis=1))
    full = np.ones((5, 7), np.int64)
    assert len(R.boundary_points(full, 0b10)) == 0          # the frame edge contributes no points


def test_generated_draws():
    for seed, row, N, n_min, iters in ((0, 0, 16, 15, 40), (1, 3, 352, 15, 40), (7, 65, 4096, 15, 3), (2, 1, 33, 32, 5)):
        d = R.generated_draws(seed, row, N, n_min, iters)
        assert d.shape == (iters + 1, n_min) and d.min() >= 0 and d.max() < N
        assert all(len(set(r.tolist())) == n_min for r in d)
        assert np.array_equal(d, R.generated_draws(seed, row, N, n_min, iters))
        assert not np.array_equal(d, R.generated_draws(seed + 1, row, N, n_min, iters))
        assert not np.array_equal(d, R.generated_draws(seed, row + 1, N, n_min, iters))
    assert R.generated_draws(0, 0, 8, 15, 2) is None          # 15 distinct indices out of 8: the attempts run out


def test_workspace_bytes_on_the_host():
    from egne_amd import _lib
    L = _lib.lib()
    f = L.egne_ellipse_ransac_workspace_bytes
    assert f(2, 240, 320, 4096) == 2 * (128 + 240 * 5 * 8 + 240 * 5 * 4 + 4096 * 4)
    assert f(1, 2, 2, 2) > 0 and f(1, 1024, 1024, 16384) > 0
    for n, H, W, mp in ((1, 1, 64, 256), (1, 64, 1, 256), (1, 1025, 64, 256), (1, 64, 1025, 256), (0, 64, 64, 256), (1, 64, 64, 0),
                        (1, 64, 64, 16385)):
        assert f(n, H, W, mp) < 0


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the launcher's offset arithmetic is proven by this program")
    d = tmp_path_factory.mktemp("ellifit_host")
    exe = str(d / "ellifit_host")
    # the sanitizer runtimes are linked statically (clang's default; g++ needs the two switches): a stand-alone program with its
    # own main, never code loaded into Python
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC] + static + ["-o", exe, os.path.join(HERE, "ellifit_host.cpp")])
    return exe, d


def run(args):
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    return p.stdout.decode()


def test_host_layout_runs_clean(host_program):
    exe, _ = host_program
    assert "layout ok" in run([exe, "layout"])


def test_host_draws_equal_the_restatement(host_program):
    exe, _ = host_program
    for seed, row, N, n_min, iters in ((0, 0, 16, 15, 40), (5, 129, 4095, 15, 7), (3, 2, 70, 64, 2)):
        lines = run([exe, "draws", str(seed), str(row), str(N), str(n_min), str(iters)]).split("\n")[:iters + 1]
        got = np.array([[int(v) for v in ln.split()] for ln in lines], np.int32)
        assert np.array_equal(got, R.generated_draws(seed, row, N, n_min, iters))


def test_host_fit_within_the_reference_bound(fx, host_program):
    """The device's Fit text (Cholesky of the Gram matrix) on the all-points set and on the best candidate's set of every case."""
    exe, d = host_program
    sets, which = [], []
    for i in range(len(fx["case_names"])):
        pts = case_points(fx, i)
        if len(pts) >= 7:
            sets.append(pts)
            which.append((i, "all"))
        if fx["valid"][i]:
            sets.append(pts[fx["inl%d" % i]])
            which.append((i, "best"))
    with open(str(d / "sets.bin"), "wb") as f:
        f.write(np.int32(len(sets)).tobytes())
        for s in sets:
            f.write(np.int32(len(s)).tobytes() + s.astype(np.int32).tobytes())
    run([exe, "fit", str(d / "sets.bin"), str(d / "out.bin")])
    out = np.fromfile(str(d / "out.bin"), np.float64).reshape(len(sets), 12)
    phi_b, par_b, phi_a, par_a = bounds(fx)
    worst = [0.0, 0.0]
    for (i, kind), o in zip(which, out):
        name = fx["case_names"][i]
        exact, truth = (fx["phi_all_exact"][i], fx["model_all_truth"][i]) if kind == "all" else (fx["phi_best_exact"][i], fx["model_truth"][i])
        pb, qb = (phi_a[i], par_a[i]) if kind == "all" else (phi_b[i], par_b[i])
        dphi = np.max(np.abs(o[:5] - exact)) / np.max(np.abs(exact))
        worst[0] = max(worst[0], dphi / pb)
        assert dphi <= pb, (name, kind, dphi, pb)
        if np.all(truth == -1):
            continue
        assert o[10] == 1.0, (name, kind)
        dpar = np.max(np.abs(o[5:10] - truth))
        worst[1] = max(worst[1], dpar / qb)
        assert dpar <= qb, (name, kind, dpar, qb)
        if kind == "best":
            assert abs(o[11] - fx["flt"][i, 0]) <= 1e-9 * fx["flt"][i, 0], name          # (the error only ranks candidates: gaps >= 1e-6)
    print("worst ratio to the bound: Phi %.3f, parameters %.3f" % tuple(worst))
