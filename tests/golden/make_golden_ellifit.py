#!/usr/bin/env python3
"""Record what the REFERENCE's ElliFit + RANSAC give on the boundary points of small class maps.

    python tests/golden/make_golden_ellifit.py        # writes tests/golden/ellifit.npz

CPU only.  Runs helperfunctions.ElliFit, ransac(pts, ElliFit, 15, 40, 5e-3, 15).loop(), my_ellipse.verify and get_ellipse_info of
the reference (through _ref_shim; none of these needs OpenCV) with np.random.choice wrapped to record the draws, on the point lists
that tests/ellifit_refs.boundary_points extracts from drawn class maps.  Stored per row case: the points, the draws, the
reference's Phi / model / error / best iteration / inlier count, the exact-rational Phi (fractions) of the all-points set and of the
best candidate's set with the reference's own deviation from it, and the decision gaps.  A case is refused (assert) when a residual
comes within 1e-6 relative of the threshold, when the two best errors are closer than 1e-6 relative, when a valid candidate does
not beat every invalid one in the reference's own numbers, or when the order-free restatement disagrees with the reference's loop.
Runs only where the reference is present; holds none of its text.
"""
import io
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_shim  # noqa: E402
import ellifit_refs as R  # noqa: E402

N_MIN, ITERS, THRES, N_GOOD = 15, 40, 5e-3, 15


def draw_frame(H, W, iris, pupil, lid=None, speck=None):
    """uint8 class map: 1 inside the iris ellipse, 2 inside the pupil ellipse; (cx, cy, a, b, t) with a along (cos t, sin t)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    lab = np.zeros((H, W), np.uint8)
    for cls, (cx, cy, a, b, t) in ((1, iris), (2, pupil)):
        dx, dy = xx - cx, yy - cy
        u, v = dx * np.cos(t) + dy * np.sin(t), dy * np.cos(t) - dx * np.sin(t)
        lab[(u / a) ** 2 + (v / b) ** 2 <= 1.0] = cls
    if lid is not None:
        lab[:lid] = 0
    if speck is not None:
        lab[speck[1]:speck[1] + 2, speck[0]:speck[0] + 2] = 2
    return lab


def draw_points(H, W, k, ell):
    """k isolated pixels of class 3 on an ellipse: a region whose boundary has exactly k points."""
    cx, cy, a, b, t = ell
    lab = np.zeros((H, W), np.uint8)
    got = set()
    M = 8 * k
    for j in list(range(0, M, 8)) + list(range(M)):      # evenly spaced first, then whatever is still free
        if len(got) == k:
            break
        th = 2 * np.pi * j / M
        x = int(round(cx + a * np.cos(th) * np.cos(t) - b * np.sin(th) * np.sin(t)))
        y = int(round(cy + a * np.cos(th) * np.sin(t) + b * np.sin(th) * np.cos(t)))
        assert 0 <= x < W and 0 <= y < H
        got.add((x, y))
    assert len(got) == k, (k, len(got))
    for x, y in got:
        lab[y, x] = 3
    return lab


def main():
    hf = _ref_shim.reference_modules()["hf"]
    maps, cases = [], []          # cases: (name, map index, class_bits, search_cls, exclude_bits, np.random seed)
    frames = []                   # (name, map index, drawn iris, drawn pupil, fully visible)

    def add_frame(name, lab, iris, pupil, full):
        maps.append(lab)
        m = len(maps) - 1
        frames.append((name, m, iris, pupil, full))
        for r, (cb, sc, eb) in enumerate(R.DEFAULT_REGIONS):
            cases.append(("%s_%s" % (name, ("iris", "pupil")[r]), m, cb, sc, eb, r))

    fulls = [("full0", 240, 320, (160, 120, 70, 55, 0.3), (165, 118, 28, 22, -0.2)),
             ("full1", 240, 320, (150, 125, 80, 60, -0.5), (140, 130, 20, 25, 0.8)),
             ("full2", 70, 130, (65, 35, 40, 25, 0.2), (63, 36, 12, 9, 0.0)),
             ("full3", 70, 130, (60, 34, 35, 28, 1.0), (62, 33, 10, 8, -0.6)),
             ("full4", 70, 130, (70, 36, 45, 22, -0.15), (72, 35, 11, 11, 0.0))]
    for name, H, W, iris, pupil in fulls:
        add_frame(name, draw_frame(H, W, iris, pupil), iris, pupil, True)
    add_frame("lidcut", draw_frame(70, 130, fulls[2][3], fulls[2][4], lid=22), fulls[2][3], fulls[2][4], False)
    add_frame("framecut", draw_frame(70, 130, (105, 50, 40, 25, 0.2), (103, 51, 12, 9, 0.0)), (105, 50, 40, 25, 0.2), (103, 51, 12, 9, 0.0), False)
    add_frame("speck", draw_frame(70, 130, fulls[2][3], fulls[2][4], speck=(79, 36)), fulls[2][3], fulls[2][4], False)
    add_frame("small", draw_frame(24, 40, (20, 12, 15, 9.5, 0.1), (20, 12, 5, 4.2, 0.0)), (20, 12, 15, 9.5, 0.1), (20, 12, 5, 4.2, 0.0), False)
    for k, (H, W, ell) in ((6, (24, 40, (20, 12, 14, 8, 0.2))), (7, (24, 40, (20, 12, 14, 8, 0.2))), (15, (24, 40, (20, 12, 14, 8, 0.2))),
                           (16, (24, 40, (20, 12, 14, 8, 0.2))), (65, (70, 130, (65, 35, 50, 28, 0.2))),
                           (129, (70, 130, (65, 35, 55, 30, -0.1)))):
        maps.append(draw_points(H, W, k, ell))
        cases.append(("pts%d" % k, len(maps) - 1, 1 << 3, 1, 0, 0))
    lab = np.ones((24, 40), np.uint8)                    # a region that touches all four frame edges: only the hole has a boundary
    lab[draw_frame(24, 40, (19, 11, 12, 7, -0.3), (0, 0, 0.1, 0.1, 0)) == 1] = 0
    maps.append(lab)
    cases.append(("alledges", len(maps) - 1, 0b10, 1, 0, 0))

    out = {"n_maps": len(maps), "case_names": np.array([c[0] for c in cases]),
           "case_map": np.array([c[1] for c in cases], np.int32), "case_bits": np.array([c[2] for c in cases], np.int64),
           "case_cls": np.array([c[3] for c in cases], np.int32), "case_excl": np.array([c[4] for c in cases], np.int64),
           "params": np.array([N_MIN, ITERS, THRES, N_GOOD], np.float64)}
    for i, m in enumerate(maps):
        out["map%d" % i] = m
    K1 = ITERS + 1
    n = len(cases)
    draws = -np.ones((n, K1, N_MIN), np.int32)
    keys = ("model", "phi_all_ref", "phi_all_exact", "phi_best_ref", "phi_best_exact", "model_all_ref", "model_all_truth", "model_truth")
    arr = {k: -np.ones((n, 5)) for k in keys}
    ints = np.zeros((n, 4), np.int32)                     # N, best iteration, |I|, candidates including -1
    flt = np.full((n, 6), np.inf)                         # error, verify, gap_T, gap_best, dev_phi (ref vs exact, best set), dev_phi_all
    dev_par = np.zeros((n, 5))                            # |reference model - truth|, best set
    dev_par_all = np.zeros((n, 5))
    valid = np.zeros(n, bool)

    for i, (name, m, cb, sc, eb, seed) in enumerate(cases):
        pts = R.boundary_points(maps[m], cb, eb)
        out["pts%d" % i] = pts.astype(np.int16)
        N = len(pts)
        rec = []
        orig = np.random.choice

        def choice(a, size=None, replace=True, p=None):
            r = orig(a, size, replace, p)
            rec.append(np.array(r))
            return r

        np.random.seed(seed)
        np.random.choice = choice
        try:
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                if N > 0:
                    rs = hf.ransac(pts, hf.ElliFit, N_MIN, ITERS, THRES, N_GOOD)
                    allfit = hf.ElliFit(**{"data": pts})
                    bestm = rs.loop()
                else:
                    bestm = None
        finally:
            np.random.choice = orig
        if rec:
            assert len(rec) == K1
            draws[i] = np.stack(rec)
        res = R.ransac(pts, draws[i], N_MIN, ITERS, THRES, N_GOOD)
        ints[i] = (N, res["best_iter"], res["n_inl"], res["n_cand"])
        if N < 7:
            assert bestm is None or np.all(np.asarray(bestm.model) == -1)
            print("%-16s N=%d absent" % (name, N))
            continue
        ref_model = np.asarray(bestm.model, dtype=np.float64)
        ref_valid = not np.all(ref_model == -1)
        # the order-free restatement IS the reference's loop on this case
        assert ref_valid == res["valid"], name
        assert np.array_equal(ref_model, res["model"]), (name, ref_model, res["model"])
        if ref_valid:
            assert float(bestm.error) == res["error"], (name, bestm.error, res["error"])
            assert np.size(bestm.data) // 2 == res["n_inl"]
        # decision gaps
        assert res["gap_T"] >= 1e-6 and res["gap_best"] >= 1e-6, (name, res["gap_T"], res["gap_best"])
        valid[i] = ref_valid
        arr["model"][i] = ref_model
        flt[i, 2:4] = (res["gap_T"], res["gap_best"])
        # all-points fit
        arr["phi_all_ref"][i] = np.asarray(allfit.Phi, dtype=np.float64)
        arr["model_all_ref"][i] = np.asarray(allfit.model, dtype=np.float64)
        ex = R.exact_phi(pts)
        if ex is not None:
            arr["phi_all_exact"][i] = ex[0]
            t = R.model_of_phi(ex[0], ex[1], ex[2])
            if t is not None and not np.all(arr["model_all_ref"][i] == -1):
                arr["model_all_truth"][i] = t
                dev_par_all[i] = np.abs(arr["model_all_ref"][i] - t)
            flt[i, 5] = np.max(np.abs(arr["phi_all_ref"][i] - ex[0])) / np.max(np.abs(ex[0]))
        if not ref_valid:
            print("%-16s N=%d invalid" % (name, N))
            continue
        with contextlib.redirect_stdout(io.StringIO()):
            flt[i, 0:2] = (float(bestm.error), float(hf.my_ellipse(ref_model).verify(pts)))
        sel = pts[res["inliers"]]
        arr["phi_best_ref"][i] = np.asarray(bestm.Phi, dtype=np.float64)
        ex = R.exact_phi(sel)
        arr["phi_best_exact"][i] = ex[0]
        arr["model_truth"][i] = R.model_of_phi(ex[0], ex[1], ex[2])
        dev_par[i] = np.abs(ref_model - arr["model_truth"][i])
        flt[i, 4] = np.max(np.abs(arr["phi_best_ref"][i] - ex[0])) / np.max(np.abs(ex[0]))
        out["inl%d" % i] = res["inliers"]
        assert abs(R.verify(ref_model, pts) - flt[i, 1]) <= 1e-9 * max(1.0, abs(flt[i, 1]))
        print("%-16s N=%4d best %3d |I| %4d cand %2d err %.3e verify %+.4f gapT %.1e gapB %.1e devPhi %.1e devPar %.1e"
              % (name, N, res["best_iter"], res["n_inl"], res["n_cand"], flt[i, 0], flt[i, 1], flt[i, 2], flt[i, 3], flt[i, 4], dev_par[i].max()))

    # drawn fully visible ellipses: what the reference recipe recovers, and the search-convention angle against the drawn one
    for name, m, iris, pupil, full in frames:
        if not full:
            continue
        for r, drawn in enumerate((iris, pupil)):
            i = [c[0] for c in cases].index("%s_%s" % (name, ("iris", "pupil")[r]))
            mod = arr["model"][i]
            dc = max(abs(mod[0] - drawn[0]), abs(mod[1] - drawn[1]))
            da = np.max(np.abs(np.sort(mod[2:4]) - np.sort(drawn[2:4])))
            s = R.to_search(mod, *maps[m].shape)
            dth = (s[4] - (drawn[4] if drawn[2] >= drawn[3] else drawn[4] + np.pi / 2) + np.pi / 2) % np.pi - np.pi / 2
            print("drawn %-12s centre off %.2f px, axes off %.2f px, search-convention angle off %+.3f rad" % (cases[i][0], dc, da, dth))
            assert dc <= 1.5 and da <= 1.5
            assert drawn[2] == drawn[3] or abs(dth) < 0.1

    # the batch targets of the frames (CurriculumLib.py:152-165, :189-193 on Extract*.py's acceptance rule)
    F = len(frames)
    tg_pc, tg_ic, tg_el, tg_cond = -np.ones((F, 2)), -np.ones((F, 2)), -np.ones((F, 2, 5)), np.zeros((F, 4))
    names = [c[0] for c in cases]
    for f, (name, m, iris, pupil, full) in enumerate(frames):
        lab = maps[m]
        H, W = lab.shape
        Hn = np.array([[2 / W, 0, -1], [0, 2 / H, -1], [0, 0, 1]])
        ii, ip = names.index(name + "_iris"), names.index(name + "_pupil")
        ok_i = valid[ii] and abs(flt[ii, 1]) < 0.05
        ok_p = valid[ip] and abs(flt[ip, 1]) < 0.05
        r, c = np.where(lab == 2)
        tg_pc[f] = arr["model"][ip][:2] if ok_p else np.stack([np.mean(c), np.mean(r)], axis=0)
        tg_ic[f] = arr["model"][ii][:2] if ok_i else tg_pc[f]
        tg_cond[f] = (0, float(np.all(lab == 0)), float(not ok_p), float(not ok_i))
        for k, (ok, i) in enumerate(((ok_i, ii), (ok_p, ip))):
            with contextlib.redirect_stdout(io.StringIO()):
                tg_el[f, k] = hf.get_ellipse_info(arr["model"][i].copy(), Hn, not ok)[1]
        print("targets %-9s verify iris %+.4f pupil %+.4f cond %s" % (name, flt[ii, 1], flt[ip, 1], tg_cond[f]))
    assert any(c[2] == 1 and c[3] == 0 for c in tg_cond), "no frame exercises the centroid fallback"

    out.update(draws=draws, ints=ints, flt=flt, valid=valid, dev_par=dev_par, dev_par_all=dev_par_all,
               frame_names=np.array([f[0] for f in frames]), frame_map=np.array([f[1] for f in frames], np.int32),
               frame_full=np.array([f[4] for f in frames]), frame_drawn=np.array([[f[2], f[3]] for f in frames], np.float64),
               tg_pc=tg_pc, tg_ic=tg_ic, tg_el=tg_el, tg_cond=tg_cond, **arr)
    path = os.path.join(HERE, "ellifit.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d maps, %d row cases" % (path, os.path.getsize(path), len(maps), n))


if __name__ == "__main__":
    main()
