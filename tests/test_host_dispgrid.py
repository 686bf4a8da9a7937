"""Prediction overlay grid (csrc/dispgrid.hip), everything that runs without a GPU: the NumPy restatement
(tests/dispgrid_refs.py) against what the reference's generateImageGrid recorded (tests/golden/dispgrid.npz), the kernels' arithmetic
(csrc/dispgrid_core.h) compiled into a stand-alone host program under -fsanitize=address,undefined, and the command-line flag."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dispgrid_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "edge-guided-near-eye-image-analysis-for-head-mounted-displays_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "dispgrid.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(R.FIXTURE_CASES))
def test_restatement_reproduces_the_golden_file(name):
    G = np.load(GOLDEN, allow_pickle=False)
    B, H, W, seed, override, leave = R.FIXTURE_CASES[name]
    inp, override = R.fixture_inputs(name)
    p = name + "_"
    assert str(G[p + "inputs_sha"]) == R.sha(np.concatenate([inp[k].astype(np.float64).ravel() for k in ("img", "mask", "el", "el_gt", "cond")]))
    n = min(4, B)
    # pinned by the reference: the uint8 arrays handed to equalizeHist, the integers and the orientation handed to ellipse_perimeter
    assert np.array_equal(np.stack([R.frame_u8(inp["img"][i])[0] for i in range(n)]), G[p + "u8"])
    calls = []
    for i in range(n):
        if override or inp["cond"][i, 1] == 0:
            for e in (inp["el_gt"][i, 0], inp["el_gt"][i, 1], inp["el"][i, 0], inp["el"][i, 1]):        # utils.py:316-343: the call order
                px = R.pixel_ellipse(e, H, W)
                calls.append(R.ints_of(px) + (float(px[4]),))
    got, want = np.array(calls, np.float64).reshape(-1, 5), G[p + "perimeter_args"]
    assert np.array_equal(got[:, :4], want[:, :4])
    assert np.allclose(got[:, 4], want[:, 4], rtol=0, atol=1e-12)        # (np.linalg.inv of the reference against the oracle's: last places)
    grid, u8, status = R.image_grid(inp["img"], inp["mask"], inp["el"], inp["cond"], inp["el_gt"], override=override)
    assert not status.any()
    assert R.sha(grid) == str(G[p + "grid_sha"])
    assert np.array_equal(u8, G[p + "grid_u8"])
    if name in R.HASHED:
        assert p + "grid" not in G.files
    else:
        assert np.array_equal(_bits(grid), _bits(G[p + "grid"]))
    if name == "cond":          # frames whose cond[:,1] is set stay grey
        assert any(inp["cond"][:n, 1] != 0) and any(inp["cond"][:n, 1] == 0)
        for i in range(n):
            r0, c0 = R.grid_origin(i, n, 4, H, W)
            tile = grid[:, r0:r0 + H, c0:c0 + W]
            assert (tile.max() <= 1) == (inp["cond"][i, 1] != 0)


def test_golden_file_holds_data_only():
    G = np.load(GOLDEN, allow_pickle=False)          # (a pickled object would raise here)
    assert "pixels_from" in G.files and "pinned_by_reference" in G.files
    for k in G.files:
        assert G[k].dtype.kind in "uifU", (k, G[k].dtype)
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_the_general_table_and_the_clip():
    # OpenCV's rule on histograms the frames cannot produce, and the two forms of the grey table
    rng = np.random.RandomState(5)
    one = np.zeros(256, np.int64); one[77] = 1234
    assert np.array_equal(R.equalize_lut(one), np.full(256, 77, np.uint8)) and not R.grey_table(one)[1].any()
    two = np.zeros(256, np.int64); two[[3, 200]] = (10, 30)
    lut = R.equalize_lut(two)
    assert lut[3] == 0 and lut[200] == 255 and lut[199] == 0
    tie = np.zeros(256, np.int64); tie[[0, 1, 2]] = (5, 1, 1)         # 1 * 127.5: the tie goes to the even 128
    assert list(R.equalize_lut(tie)[:3]) == [0, 128, 255]
    for _ in range(50):
        h = np.where(rng.rand(256) < rng.uniform(0.02, 1), rng.randint(0, 500, 256), 0)
        h[rng.randint(256)] += 1
        u = np.repeat(np.arange(256, dtype=np.uint8), h)
        lut, table = R.grey_table(h)
        assert np.array_equal(_bits(table[u]), _bits(R.grey(R.equalize(u))))
    # ndarray.clip(6, n - 6) taken literally, also where n - 6 < 6
    rr, cc = R.clip_rows_cols(np.array([-5, 0, 6, 7, 100]), np.array([-5, 0, 6, 7, 100]), 8, 13)
    assert list(rr) == [2, 2, 2, 2, 2] and list(cc) == [6, 6, 6, 7, 7]
    assert R.grid_shape(1, 4, 48, 64) == (48, 64) and R.grid_shape(5, 4, 48, 64) == (102, 266) and R.grid_shape(2, 4, 33, 47) == (37, 100)
    assert R.grid_origin(5, 6, 4, 48, 64) == (52, 68)


SPECIAL_ELLIPSES = (
    (float("nan"), 10., 5., 4., 0.1), (20., 10., 0.99, 4., 0.1), (20., 10., 5., float("inf"), 0.2), (1e300, -1e300, 1e299, 3., 1.0),
    (-40.5, 200.25, 7.5, 3.5, -0.7), (20.5, 10.5, 1.0, 1.0, 0.0), (3e9, 3e9, 5.5, 4.5, 0.3))


def special_frames(H, W):
    rng = np.random.RandomState(H * 100 + W)
    base = rng.randn(H, W).astype(np.float32)
    nan = base.copy(); nan[H // 2, W // 3] = np.nan
    inf = base.copy(); inf[0, 0] = np.inf; inf[1, 1] = -np.inf
    two = np.where(rng.rand(H, W) < 0.3, np.float32(-1.25), np.float32(0.5)).astype(np.float32)
    negzero = np.abs(base); negzero[2, 3] = -0.0; negzero[4, 5] = 0.0
    with np.errstate(over="ignore"):
        huge = (base * np.float32(3e38)).astype(np.float32)
    tiny = (base * np.float32(1e-42)).astype(np.float32)         # subnormal span
    return {"constant": np.full((H, W), np.float32(-0.75)), "nan": nan, "inf": inf, "two_levels": two, "negative_zero": negzero, "huge": huge,
            "subnormal": tiny}


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the kernels' arithmetic is proven by this program")
    d = tmp_path_factory.mktemp("dispgrid_host")
    exe = str(d / "dispgrid_host")
    # the sanitizer runtimes are linked statically (clang's default; g++ needs the two switches): a stand-alone program with its own
    # main, never code loaded into Python
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC] + static + ["-o", exe, os.path.join(HERE, "dispgrid_host.cpp")])
    return exe, d


def test_host_program_equals_the_restatement(host_program):
    exe, d = host_program
    t = np.linspace(0, 2 * np.pi, 720, endpoint=False)
    rng = np.random.RandomState(9)
    gv = np.concatenate([np.arange(256) / np.float64(255), [255., 102., -1., -0., 0.5, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1e-45, 0.999999],
                         rng.rand(200)]).astype(np.float32)
    hists = []
    for k in range(40):
        h = np.where(rng.rand(256) < rng.uniform(0.01, 1), rng.randint(0, 2000, 256), 0)
        h[rng.randint(256)] += 1 + (k % 3 == 0) * 100000
        hists.append(h.astype(np.int32))
    one = np.zeros(256, np.int32); one[200] = 7
    hists.append(one)
    blob = [np.cos(t).tobytes(), np.sin(t).tobytes(), np.int32(len(gv)).tobytes(), gv.tobytes(), np.int32(len(hists)).tobytes()]
    blob += [h.tobytes() for h in hists]
    cases = []
    for name in ("five", "odd", "clip"):
        B, H, W = R.FIXTURE_CASES[name][:3]
        inp, _ = R.fixture_inputs(name)
        ells = [R.pixel_ellipse(e, H, W) for e in np.concatenate([inp["el"].reshape(-1, 5), inp["el_gt"].reshape(-1, 5)])]
        cases.append((name, H, W, list(inp["img"]), 4, ells))
    for H, W in ((13, 17), (6, 6), (8, 40)):
        cases.append(("special_%dx%d" % (H, W), H, W, list(special_frames(H, W).values()), 3, [np.array(e) for e in SPECIAL_ELLIPSES]))
    blob.append(np.int32(len(cases)).tobytes())
    for name, H, W, frames, nrow, ells in cases:
        blob.append(np.array([H, W, len(frames), nrow, len(ells)], np.int32).tobytes())
        blob += [np.ascontiguousarray(f, np.float32).tobytes() for f in frames]
        blob += [np.concatenate([e[:5], [np.cos(e[4]), np.sin(e[4])]]).astype(np.float64).tobytes() for e in ells]
    with open(str(d / "in.bin"), "wb") as f:
        f.write(b"".join(blob))
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    raw = open(str(d / "out.bin"), "rb").read()
    at = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, at[0])
        at[0] += a.nbytes
        return a
    assert np.array_equal(take(np.uint8, len(gv)), np.rint(np.float32(255) * np.clip(gv, np.float32(0), np.float32(1))).astype(np.uint8))
    for h in hists:
        lut, table = R.grey_table(h)
        assert np.array_equal(take(np.uint8, 256), lut)
        assert np.array_equal(take(np.uint32, 256), _bits(table))
    for name, H, W, frames, nrow, ells in cases:
        for i, f in enumerate(frames):
            what = "%s frame %d" % (name, i)
            mn, dd = take(np.float32, 1)[0], take(np.float32, 1)[0]
            fin = np.isfinite(f)
            with np.errstate(all="ignore"):
                assert mn == f[fin].min() and _bits(dd) == _bits(np.float32(f[fin].max() - f[fin].min())), what
            u, st = R.frame_u8(f)
            assert np.array_equal(take(np.uint8, H * W).reshape(H, W), u), what
            lut, table = R.grey_table(np.bincount(u.ravel(), minlength=256))
            assert np.array_equal(take(np.uint8, 256), lut), what
            assert np.array_equal(take(np.uint32, 256), _bits(table)), what
            if not st:
                assert lut[u].min() == 0 and lut[u].max() == 255, what          # (what the kernel's comment states)
                assert np.array_equal(_bits(table[u]), _bits(R.grey(R.equalize(u)))), what
        n = len(frames)
        assert tuple(take(np.int32, 2)) == R.grid_shape(n, nrow, H, W), name
        for i in range(n):
            assert tuple(take(np.int32, 2)) == R.grid_origin(i, n, nrow, H, W), name
        for k, e in enumerate(ells):
            drawn, rows, cols = take(np.int32, 1)[0], take(np.int32, 720), take(np.int32, 720)
            want = R.outline(e, H, W)
            assert bool(drawn) == (want is not None), (name, k)
            if want is not None:
                assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1]), (name, k)
                assert rows.min() >= 0 and rows.max() < H and cols.min() >= 0 and cols.max() < W
                if np.all(np.abs(e[:4]) < 1e9):          # the integer form of the clip, where an int64 holds the coordinates
                    rr, cc = R.clip_rows_cols(*R.perimeter(*R.ints_of(e), e[4]), H, W)
                    assert np.array_equal(rows, rr) and np.array_equal(cols, cc), (name, k)
    assert at[0] == len(raw)


def test_disp_flag():
    from egne_amd import args as A
    p = A.build_parser()
    assert p.parse_args([]).disp == 0 and p.parse_args(["--disp", "1"]).disp == 1
    text = " ".join(p.format_help().split())
    assert "img/<curObj or 'synthetic'>_<method>_disp/batch_%05d.jpg" in text
    assert "logs/<model>/<expname>/disp/epoch_%03d.jpg" in text
    assert "Nothing is drawn per training batch" in text
