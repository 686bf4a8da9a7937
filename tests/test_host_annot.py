"""Label maps from TEyeD annotations (csrc/annot.hip), everything that runs without a GPU: the host functions of
egne_amd.dataprep and the NumPy restatement (tests/annot_refs.py) against what the reference's Extract_TEyeD_NvGaze_AR_histo.py
recorded (tests/golden/annot.npz), the kernel's rules (csrc/annot_core.h) compiled into a stand-alone host program under
-fsanitize=address,undefined, exact properties of the rules, and a sanity check of the polygon rule against PIL."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import annot_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "edge-guided-near-eye-image-analysis-for-head-mounted-displays_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "annot.npz")


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN, allow_pickle=False))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def test_golden_file_holds_data_only(G):
    assert "pixels_from" in G and "pinned_by_reference" in G and len(G["supplied"]) == 2
    for k, v in G.items():
        assert v.dtype.kind in "uifU", (k, v.dtype)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert len(G["kept"]) >= 12 and len(G["ann_ball"]) - len(G["kept"]) >= 3
    ang = np.concatenate([G["ann_iris"][G["kept"], 0], G["ann_pupil"][G["kept"], 0]])
    assert (ang < 90).any() and (ang > 90).any()
    lid = G["ann_lid"][G["kept"]]
    assert (lid < 0).any() and (lid[..., 0] > 640).any()


def test_keep_and_fits_reproduce_the_reference(G):
    from egne_amd import dataprep
    keep = dataprep.annotation_keep(G["ann_ball"], G["ann_iris"], G["ann_pupil"])
    assert np.array_equal(np.nonzero(keep)[0], G["kept"])
    # the scripts' counter: candidates are every interval-th frame of the 1-based running count
    assert np.array_equal(G["frame_rows"][G["kept"]], np.array([int(s) for s in G["info"]]))
    k = G["kept"]
    loc, fp, fi = dataprep.annotation_fits(G["ann_iris"][k], G["ann_pupil"][k])
    assert np.array_equal(loc, G["pupil_loc"]) and np.array_equal(loc, G["keydict_pupil_loc"])
    assert np.array_equal(fp, G["Fits_pupil"]) and np.array_equal(fi, G["Fits_iris"])
    b = G["ann_ball"][k]
    assert np.array_equal(np.stack([b[:, 1], b[:, 2], b[:, 0], b[:, 0], np.zeros(len(b))], 1), G["Fits_ball"])
    assert np.array_equal(G["resolution"], np.tile([480, 640], (len(k), 1)))


def test_pack_reproduces_every_recorded_cv2_argument(G):
    from egne_amd import dataprep
    k = G["kept"]
    rec = dataprep.pack_annotations(G["ann_ball"][k], G["ann_iris"][k], G["ann_pupil"][k], G["ann_lid"][k])
    assert rec.dtype == np.int32 and rec.shape == (len(k), R.RECORD_WORDS)
    assert list(G["call_order"]) == ["circle", "ellipse", "ellipse", "fillPoly"] * len(k)
    d = rec.view(np.float64)
    assert np.array_equal(rec[:, 0], np.full(len(k), 15)) and np.array_equal(rec[:, 1], np.full(len(k), 34))
    assert np.array_equal(rec[:, 2:5], G["circle_args"][:, :3])
    assert np.array_equal(G["circle_args"][:, 3:], np.tile([1, -1], (len(k), 1)))
    for j, (word, colour, src) in enumerate(((6, 2, "ann_iris"), (14, 3, "ann_pupil"))):
        args = G["ellipse_args"][j::2]
        assert np.array_equal(rec[:, word:word + 4], args[:, :4])
        assert np.array_equal(args[:, 4], G[src][k, 0])                # the angle goes in unmodified
        t = np.radians(args[:, 4])
        assert np.array_equal(d[:, word // 2 + 2], np.cos(t)) and np.array_equal(d[:, word // 2 + 3], np.sin(t))
        assert np.array_equal(args[:, 5:], np.tile([0, 360, colour, -1], (len(k), 1)))
    assert np.array_equal(rec[:, 22:22 + 68].reshape(len(k), 34, 2), G["fillpoly_pts"])
    assert np.array_equal(rec, R.pack(G["ann_ball"][k], G["ann_iris"][k], G["ann_pupil"][k], G["ann_lid"][k]))


def test_restatement_reproduces_the_masks(G):
    from egne_amd import dataprep
    k = G["kept"]
    rec = dataprep.pack_annotations(G["ann_ball"][k], G["ann_iris"][k], G["ann_pupil"][k], G["ann_lid"][k])
    noskin, skin, status = R.paint(rec, 480, 640)
    assert not status.any()
    assert R.sha(skin) == str(G["Masks_sha"]) and R.sha(noskin) == str(G["Masks_noSkin_sha"])
    assert np.array_equal(skin[G["full"]], G["Masks_full"]) and np.array_equal(noskin[G["full"]], G["Masks_noSkin_full"])
    assert set(np.unique(noskin)) == {0, 1, 2, 3} and (skin != noskin).any() and ((skin == noskin) | (skin == 0)).all()


def test_pack_limits_and_absent_shapes():
    from egne_amd import dataprep
    ball, iris, pupil, lid = R.seeded_annotations(3, 11, 96, 128)
    rec = dataprep.pack_annotations(ball, iris, pupil, lid, present=[(1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0)])
    assert list(rec[:, 0]) == [15, 10, 5] and list(rec[:, 1]) == [34, 34, 0]
    assert np.array_equal(rec, R.pack(ball, iris, pupil, lid, present=[(1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0)]))
    assert list(dataprep.pack_annotations(None, iris, None, None)[:, 0]) == [2, 2, 2]
    assert dataprep.pack_annotations(ball, iris, pupil, np.full((3, 34, 2), -0.5))[:, 22:90].any() == False          # noqa: E712  int(-0.5) == 0
    for field, at, v in (("ball", (1, 0), 2.0 ** 20 + 1), ("iris", (0, 1), -2.0 ** 20 - 1), ("pupil", (2, 3), 2.0 ** 21 + 4), ("lid", (1, 5, 1), 1e9),
                         ("iris", (1, 2), float("nan")), ("pupil", (0, 0), float("inf"))):
        a = {"ball": ball.copy(), "iris": iris.copy(), "pupil": pupil.copy(), "lid": lid.copy()}
        a[field][at] = v
        with pytest.raises(ValueError):
            dataprep.pack_annotations(a["ball"], a["iris"], a["pupil"], a["lid"])
    dataprep.pack_annotations(np.array([[2.0 ** 20, 0, 0]]), None, None, None)          # the limit itself is accepted
    with pytest.raises(ValueError):
        dataprep.pack_annotations(ball, iris, pupil, np.zeros((3, 65, 2)))


# ---- the host program ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the kernel's rules are proven by this program")
    d = tmp_path_factory.mktemp("annot_host")
    exe = str(d / "annot_host")
    # the sanitizer runtimes are linked statically (clang's default; g++ needs the two switches): a stand-alone program with its own
    # main, never code loaded into Python
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC] + static + ["-o", exe, os.path.join(HERE, "annot_host.cpp")])
    return exe, d


HOST_CASES = ((5, 7, 3, False), (37, 53, 5, True), (64, 64, 5, False), (65, 129, 5, True), (240, 320, 18, False), (48, 64, 18, True))


def test_host_program_equals_the_restatement(host_program):
    exe, d = host_program
    blob, cases = [np.int32(len(HOST_CASES)).tobytes()], []
    for i, (r, c, B, ragged) in enumerate(HOST_CASES):
        names, rec = R.case_records(r, c, B, first=5 * i)
        hw = R.ragged_hw(r, c, B) if ragged else None
        cases.append((r, c, B, hw, rec))
        blob += [np.array([B, r, c, int(ragged), 1], np.int32).tobytes(), rec.tobytes()] + ([hw.tobytes()] if ragged else [])
    with open(str(d / "in.bin"), "wb") as f:
        f.write(b"".join(blob))
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    raw, at = open(str(d / "out.bin"), "rb").read(), 0
    seen = 0
    for r, c, B, hw, rec in cases:
        noskin, skin, status = R.paint(rec, r, c, hw)
        n = B * r * c
        assert np.array_equal(np.frombuffer(raw, np.int8, n, at).reshape(B, r, c), noskin), (r, c)
        assert np.array_equal(np.frombuffer(raw, np.int8, n, at + n).reshape(B, r, c), skin), (r, c)
        assert np.array_equal(np.frombuffer(raw, np.int32, B, at + 2 * n), status), (r, c)
        at += 2 * n + 4 * B
        seen |= int(np.bitwise_or.reduce(status))
    assert at == len(raw) and seen == 7           # every status bit occurs


# ---- exact properties of the rules ----------------------------------------------------------------------------------------------------------
def _cs(deg):
    t = np.radians(np.float64(deg))
    return np.cos(t), np.sin(t)


def test_circle_and_ellipse_are_point_symmetric():
    R_, C_ = 61, 81          # odd: the centre pixel (30, 40) is the centre of the canvas
    for br in (0, 1, 7, 29, 100):
        m = R.circle_map(R_, C_, 40, 30, br)
        assert np.array_equal(m, m[::-1, ::-1]) and m[30, 40]
    assert R.circle_map(R_, C_, 40, 30, 0).sum() == 1
    for A, B, deg in ((20, 9, 0), (20, 9, 37.5), (7, 25, 137.25), (1, 1, 12), (30, 30, 90), (25, 3, -61)):
        m = R.ellipse_map(R_, C_, 40, 30, A, B, *_cs(deg))
        assert m.any() and np.array_equal(m, m[::-1, ::-1]), (A, B, deg)


def test_ellipse_containment_and_half_turn():
    R_, C_ = 70, 90
    for deg in (0, 90, 37.5, 137.25, -20):
        for A, B in ((1, 1), (5, 12), (20, 7), (30, 30)):
            small, big = R.ellipse_map(R_, C_, 44, 33, A, B, *_cs(deg)), R.ellipse_map(R_, C_, 44, 33, A + 1, B + 1, *_cs(deg))
            assert not (small & ~big).any() and big.sum() > small.sum(), (A, B, deg)
    for deg in (0, 90, 37.5):
        for A, B in ((20, 7), (5, 12)):
            assert np.array_equal(R.ellipse_map(R_, C_, 44, 33, A, B, *_cs(deg)), R.ellipse_map(R_, C_, 44, 33, A, B, *_cs(deg + 180))), (A, B, deg)
    assert not R.ellipse_map(R_, C_, 44, 33, 0, 9, *_cs(10)).any() and not R.ellipse_map(R_, C_, 44, 33, 9, 0, *_cs(10)).any()


def _segment_pixels(R_, C_, a, b):
    """The integer points of the canvas that lie on the segment a-b exactly."""
    x, y = np.arange(C_)[None, :], np.arange(R_)[:, None]
    cross = (x - a[0]) * (b[1] - a[1]) - (b[0] - a[0]) * (y - a[1])
    return (cross == 0) & (x >= min(a[0], b[0])) & (x <= max(a[0], b[0])) & (y >= min(a[1], b[1])) & (y <= max(a[1], b[1]))


def test_degenerate_polygons_are_their_boundary():
    R_, C_ = 40, 50
    for pts in ([(3, 4), (33, 24)], [(3, 4), (33, 24), (18, 14)], [(5, 7), (45, 7), (20, 7)], [(9, 2), (9, 30)], [(12, 12)],
                [(3, 4), (3, 4), (33, 24), (33, 24), (3, 4)], [(-10, -5), (60, 45)]):
        want = np.zeros((R_, C_), bool)
        for i in range(len(pts)):
            want |= _segment_pixels(R_, C_, pts[i], pts[(i + 1) % len(pts)])
        assert np.array_equal(R.polygon_map(R_, C_, pts), want), pts
    # repeated vertices in a polygon with area: the same map as without them
    sq = [(5, 5), (30, 5), (30, 25), (5, 25)]
    rep = [sq[0], sq[0], sq[1], sq[2], sq[2], sq[2], sq[3]]
    m = R.polygon_map(R_, C_, sq)
    assert np.array_equal(m, R.polygon_map(R_, C_, rep)) and m.sum() == 26 * 21


def test_polygon_against_pil():
    """Sanity, no gate on pixel counts: where the rule and ImageDraw.polygon(fill=1, outline=1) differ, the pixel lies within one pixel
    of the polygon's outline."""
    from PIL import Image, ImageDraw
    R_, C_ = 96, 128
    rng = np.random.RandomState(300)
    worst, differing = 0.0, 0
    for k in range(300):
        pts = R.eyelid(rng, R_, C_, jitter=rng.uniform(0, 3), cross=k % 4 == 0, reach=0.2 * (k % 3 == 0))
        pts = np.trunc(pts).astype(np.int64)
        im = Image.new("L", (C_, R_), 0)
        ImageDraw.Draw(im).polygon([tuple(int(v) for v in p) for p in pts], fill=1, outline=1)
        diff = R.polygon_map(R_, C_, pts) != (np.asarray(im) != 0)
        if diff.any():
            differing += 1
            yy, xx = np.nonzero(diff)
            worst = max(worst, float(R.distance_to_edges(xx, yy, pts).max()))
    print("polygons that differ from PIL somewhere: %d of 300; largest distance of a differing pixel to the outline: %.3f" % (differing, worst))
    assert worst < 1.0


def test_loader_flags_and_archive_choice(tmp_path):
    from egne_amd import args as A
    p = A.build_parser()
    ns = p.parse_args([])
    assert ns.loader_size == "240x320" and ns.loader_scale == 0.0 and A.loader_geometry(ns) == ((240, 320), False)
    assert A.loader_geometry(p.parse_args(["--loader_size", "480x640", "--loader_scale", "0.5"])) == ((480, 640), 0.5)
    with pytest.raises(SystemExit):
        A.loader_geometry(p.parse_args(["--loader_size", "480"]))
    from egne_amd import loader
    ball, iris, pupil, lid = R.seeded_annotations(3, 5, 24, 32)
    img = np.random.RandomState(0).randint(0, 256, (3, 24, 32)).astype(np.uint8)
    a, r = str(tmp_path / "a.npz"), str(tmp_path / "r.npz")
    np.savez(a, Images=img, ann_ball=ball, ann_iris=iris, ann_pupil=pupil, ann_lid=lid)
    np.savez(r, Images=img, Masks_noSkin=np.zeros((3, 24, 32), np.int8), pupil_loc=np.zeros((3, 2)), Fits_pupil=np.ones((3, 5)), Fits_iris=np.ones((3, 5)))
    A_, R__ = loader.open_archive(a), loader.open_archive(r)
    assert isinstance(A_, loader.AnnotationArchive) and isinstance(R__, loader.RawArchive)
    assert loader.collate_for(A_) is loader.collate_annotated and loader.collate_for(R__) is loader.collate_raw
    b = loader.collate_annotated([A_[0], A_[2]])
    assert isinstance(b, loader.AnnotBatch) and b.records.shape == (2, 150) and b.records.dtype == np.int32 and not b.cond.any()
    assert np.array_equal(b.records, R.pack(ball, iris, pupil, lid)[[0, 2]])
    assert all(isinstance(s, loader.AnnotationArchive) for s in loader.split_archive(a))


def test_make_archive_reads_annotation_files(tmp_path):
    from egne_amd import make_archive as M
    ball, iris, pupil, lid = R.seeded_annotations(4, 6, 24, 32)
    rows = np.zeros((4, 70)); rows[:, 0] = np.arange(4)
    for k, i in enumerate(M.LID_FIELDS):
        rows[:, i], rows[:, i + 1] = lid[:, k, 0], lid[:, k, 1]
    pre = str(tmp_path / "v.avi")
    for name, t in (("eye_ball", ball), ("iris_eli", iris), ("pupil_eli", pupil)):
        with open(pre + name + ".txt", "w") as f:
            f.write("FRAME;A;B;\n" + "".join("%d;" % j + ";".join(repr(float(v)) for v in row) + ";\n" for j, row in enumerate(t)))
    with open(pre + "lid_lm_2D.txt", "w") as f:          # (no trailing separator here)
        f.write("FRAME;...\n" + "".join(";".join(repr(float(v)) for v in row) + "\n" for row in rows))
    got = M.read_annotations(pre)
    for g, w in zip(got, (ball, iris, pupil, lid)):
        assert np.array_equal(g, w)
    bad = tmp_path / "clip.avi"
    bad.write_bytes(b"RIFF\0\0\0\0AVI LIST\0\0\0\0hdrlstrh\0\0\0\0vidsH264" + b"\0" * 64)
    with pytest.raises(SystemExit, match="not a Motion-JPEG"):
        list(M.iter_frames(str(bad)))
