"""-m gpu: the ellipse-fit kernel (csrc/fit.hip) against the oracle (oracle/fit.py) where its shortcuts can go wrong without moving a
final search result of the 240x320 fixtures: every evaluation's three counts (egne_ellipse_iou_counts, the device functions the search
calls) at shapes with partial mask words, clamped intervals and more rows than a pass; whole searches off the workload's shape with
their evaluation counts; every launch form with partly filled workgroups; the seeds.  Integers and bit patterns: no tolerance except
the seeds' float64 conic algebra (rtol = atol = 1e-11, as tests/test_gpu_batch.py)."""
import numpy as np
import pytest
import torch

import fit_cases as fc
from oracle import fit as ofit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON, GUARD, NG = 0x5A5A5A5A, 0x7E7E7E7E, 64


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _i32(v):
    return int(np.array(v, np.uint32).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# (a) counts of single evaluations
# ---------------------------------------------------------------------------------------------------------------------
def _counts_c_abi(mk, fo, cl, ell, roww):
    """egne_ellipse_iou_counts straight through the C-ABI into a poisoned buffer between guard words: (counts uint32 [n,3], guards)."""
    from egne_amd import _lib
    from egne_amd.utils import _mesh_axes
    L = _lib.lib()
    F, H, W = mk.shape
    n = len(fo)
    buf = torch.full((NG + 3 * n + NG,), _i32(POISON), dtype=torch.int32, device=DEV)
    buf[:NG] = _i32(GUARD)
    buf[NG + 3 * n:] = _i32(GUARD)
    m = torch.from_numpy(mk).to(DEV)
    fo_d, cl_d, el_d = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (fo, cl, ell))
    xs, ys = _mesh_axes(H, W, torch.device(DEV))
    _lib.check(L.egne_ellipse_iou_counts(m.data_ptr(), F, fo_d.data_ptr(), cl_d.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(),
                                         el_d.data_ptr(), buf.data_ptr() + 4 * NG, roww, _lib.stream_ptr()), "ellipse_iou_counts")
    got = buf.cpu().numpy().view(np.uint32)
    return got[NG:NG + 3 * n].reshape(n, 3), np.concatenate([got[:NG], got[NG + 3 * n:]])


@pytest.mark.parametrize("roww", [1, 4])
@pytest.mark.parametrize("H,W", fc.SHAPES)
def test_counts_of_every_evaluation_equal_the_oracle(H, W, roww):
    """Every ellipse of the shape against three class maps and classes 1, 2, 3 in one launch: (nseg, nell, inter) == ell_counts."""
    mk, ell, fo, cl, idx = fc.count_batch(H, W)
    want = fc.oracle_counts(H, W)
    got, guards = _counts_c_abi(mk, fo, cl, ell, roww)
    assert (guards == GUARD).all(), "guard words around counts overwritten (%dx%d, roww %d)" % (H, W, roww)
    assert not (got == POISON).any(), "counts left unwritten (%dx%d, roww %d)" % (H, W, roww)
    bad = np.flatnonzero((got != want).any(axis=1))
    names = fc.ellipses(H, W)[0]
    print("counts %dx%d roww %d: %d evaluations, %d differ" % (H, W, roww, len(want), len(bad)))
    msg = ["%dx%d roww %d frame %d class %d ellipse %s %s: (nseg, nell, inter) device %s oracle %s"
           % (H, W, roww, fo[i], cl[i], names[idx[i]], ell[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:8]]
    assert len(bad) == 0, "%d of %d evaluations differ; first:\n%s" % (len(bad), len(want), "\n".join(msg))


def test_counts_wrapper_and_frames_it_was_not_given():
    """utils.ellipse_iou_counts returns what the C-ABI wrote; rows that name a frame outside the tensor report all ones and leave their
    neighbours alone."""
    from egne_amd.utils import ellipse_iou_counts
    H, W = 61, 83
    mk, ell, fo, cl, _ = fc.count_batch(H, W)
    want = fc.oracle_counts(H, W)
    sel = np.arange(0, len(fo), 11)
    fo2 = fo[sel].copy()
    fo2[[5, 100]] = (-1, 3)
    for roww in (1, 4):
        got = ellipse_iou_counts(torch.from_numpy(mk).to(DEV), fo2, cl[sel], ell[sel], roww)
        assert got.dtype == np.uint32 and got.shape == (len(sel), 3)
        assert (got[[5, 100]] == 0xFFFFFFFF).all()
        keep = np.ones(len(sel), bool)
        keep[[5, 100]] = False
        assert np.array_equal(got[keep], want[sel][keep])
    with pytest.raises(RuntimeError):
        ellipse_iou_counts(torch.from_numpy(mk).to(DEV), fo2, cl[sel], ell[sel], 2)


# ---------------------------------------------------------------------------------------------------------------------
# (b) whole searches, alone: the eight-wave form
# ---------------------------------------------------------------------------------------------------------------------
def _same_row(got, want):
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("name", list(fc.SEARCHES))
def test_single_search_equals_the_oracle(name):
    from egne_amd.utils import fit_ellipses
    want, nev = fc.oracle_search(name)
    mask = torch.from_numpy(fc.search_mask(name).astype(np.int64)[None]).to(DEV)
    out, ev = fit_ellipses(mask, [0], [1], fc.search_init(name)[None], return_evals=True)
    print("search %s: device %s evals %d, oracle %s evals %d" % (name, out[0].tolist(), ev[0], want.tolist(), nev))
    assert np.array_equal(out[0], want), "%s: device %s, oracle %s" % (name, out[0].tolist(), want.tolist())
    assert int(ev[0]) == nev == fc.SEARCHES[name][4], "%s: %d evaluations on the device, %d in the oracle" % (name, ev[0], nev)
    if name == "empty":
        init = fc.search_init(name)
        assert np.array_equal(out[0][:4], init[:4]) and out[0][4] == init[4] * 180. / ofit.PI_REF / 180.0 * ofit.PI_REF


# ---------------------------------------------------------------------------------------------------------------------
# (c) launch forms and partly filled workgroups
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_batch(frames, fo, cl, inits):
    res = []
    with np.errstate(all="ignore"):
        for f, c, ini in zip(fo, cl, inits):
            res.append(ofit.fit_ellipse(frames[f] == c, list(ini), count_evals=True))
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)


@pytest.fixture(scope="module")
def batch_61x83():
    """Base batch at 61x83: the six search cases of that shape on frames of their own, then classes 1, 2, 3 of two shared class maps
    (the second holds no class 3: an empty mask, NaN scores).  (frames, frame_of, cls, inits, oracle results, oracle counts)."""
    H, W = 61, 83
    names = [n for n, c in fc.SEARCHES.items() if c[:2] == (H, W)]
    assert len(names) == 6
    shared = fc.masks(H, W)[[0, 2]]
    frames = np.concatenate([np.stack([fc.search_mask(n) for n in names]).astype(np.int64), shared])
    fo = list(range(6)) + [6, 6, 6, 7, 7, 7]
    cl = [1] * 6 + [1, 2, 3, 1, 2, 3]
    iris = (0.45 * W + 1, 0.5 * H - 1, 0.38 * W - 2, 0.3 * H + 2, 0.3)
    pupil = (0.55 * W - 1, 0.45 * H + 1, 0.2 * W + 2, 0.22 * H - 1, -0.2)
    other = (0.3 * W, 0.6 * H, 0.25 * W + 1.5, 0.35 * H - 2, 1.0)
    inits = np.array([fc.search_init(n) for n in names] + [iris, pupil, iris, other, pupil, other], np.float64)
    want, nev = _oracle_batch(frames, fo, cl, inits)
    return frames, np.array(fo), np.array(cl), inits, want, nev


def _check_rows(out, ev, want, nev, order, what):
    bad = [int(i) for i, c in enumerate(order) if not (_same_row(out[i], want[c]) and ev[i] == nev[c])]
    msg = ["row %d (case %d): device %s evals %d, oracle %s evals %d" % (i, order[i], out[i].tolist(), ev[i], want[order[i]].tolist(),
                                                                        nev[order[i]]) for i in bad[:8]]
    assert not bad, "%s: %d rows differ; first:\n%s" % (what, len(bad), "\n".join(msg))


@pytest.mark.parametrize("n", [3, 15, 16, 17, 63, 64, 65, 67])
def test_every_launch_form_with_partly_filled_workgroups(batch_61x83, n):
    """n < 16: eight waves per search; 16 <= n < 64: two searches per workgroup (n = 17: the last holds one); n >= 64: four per
    workgroup with pair-local synchronisation (n = 65: the last holds one, n = 63 / 67: three)."""
    from egne_amd.utils import fit_ellipses
    frames, fo, cl, inits, want, nev = batch_61x83
    order = np.random.RandomState(n).permutation(np.tile(np.arange(len(fo)), -(-n // len(fo))))[:n]
    out, ev = fit_ellipses(torch.from_numpy(frames).to(DEV), fo[order].tolist(), cl[order].tolist(), inits[order], return_evals=True)
    _check_rows(out, ev, want, nev, order, "61x83, n = %d" % n)


def test_a_frame_it_was_not_given_in_the_middle_of_a_batch(batch_61x83):
    """n = 67 through the C-ABI with row 33 naming frame 99: that row is NaN with no evaluations, every other row the oracle's."""
    from egne_amd import _lib
    from egne_amd.utils import _mesh_axes
    frames, fo, cl, inits, want, nev = batch_61x83
    n, H, W = 67, 61, 83
    order = np.random.RandomState(n).permutation(np.tile(np.arange(len(fo)), -(-n // len(fo))))[:n]
    fo_n = fo[order].astype(np.int32)
    fo_n[33] = 99
    m = torch.from_numpy(frames).to(DEV)
    fo_d = torch.from_numpy(fo_n).to(DEV)
    cl_d = torch.from_numpy(cl[order].astype(np.int32)).to(DEV)
    ini = torch.from_numpy(np.ascontiguousarray(inits[order])).to(DEV)
    out = torch.full((n, 5), 7.0, dtype=torch.float64, device=DEV)
    ev = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    xs, ys = _mesh_axes(H, W, torch.device(DEV))
    _lib.check(_lib.lib().egne_ellipse_fit(m.data_ptr(), len(frames), fo_d.data_ptr(), cl_d.data_ptr(), n, H, W, xs.data_ptr(),
                                           ys.data_ptr(), ini.data_ptr(), out.data_ptr(), ev.data_ptr(), _lib.stream_ptr()), "ellipse_fit")
    out, ev = out.cpu().numpy(), ev.cpu().numpy()
    assert np.isnan(out[33]).all() and ev[33] == 0
    keep = np.arange(n) != 33
    _check_rows(out[keep], ev[keep], want, nev, order[keep], "61x83, n = 67 with a foreign frame in row 33")


@pytest.mark.parametrize("n", [5, 64])
def test_searches_over_more_rows_than_one_pass(n):
    """300x40: an ellipse of 240 rows needs four passes of one wave (n = 64, four searches per workgroup) and, alone (n = 5, eight waves
    per search), the whole frame of the all-class-1 mask a second pass of 256 lanes."""
    from egne_amd.utils import fit_ellipses
    H, W = fc.TALL_SHAPE
    frames = np.concatenate([np.stack([fc.render(H, W, r) for r, _ in fc.TALL_SEARCHES]).astype(np.int64), fc.masks(H, W)[1:2]])
    fo, cl = np.arange(5), np.ones(5, int)
    inits = np.array([i for _, i in fc.TALL_SEARCHES] + [fc.TALL_SEARCHES[0][1]], np.float64)
    want, nev = _oracle_batch(frames, fo, cl, inits)
    order = np.random.RandomState(n).permutation(np.tile(np.arange(5), -(-n // 5)))[:n]
    out, ev = fit_ellipses(torch.from_numpy(frames).to(DEV), fo[order].tolist(), cl[order].tolist(), inits[order], return_evals=True)
    _check_rows(out, ev, want, nev, order, "300x40, n = %d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# (d) seeds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 33, 65])
@pytest.mark.parametrize("H,W", [(240, 320), (61, 83), (300, 40)])
def test_seeds_vs_transform(H, W, F):
    """egne_ellipse_init_from_pred against oracle.fit.transform; 2F = 130 rows need a third, partly filled block of 64 threads.  The
    first frame's ellipses have theta exactly 0 (a < b, a > b): the |b| <= 1e-40 branches, told apart on a non-square frame."""
    from egne_amd.utils import ellipse_seeds_from_pred
    prm = fc.seed_params(F)
    Hm = np.array([[W / 2.0, 0, W / 2.0], [0, H / 2.0, H / 2.0], [0, 0, 1]])
    want = np.stack([ofit.transform(p.astype(np.float64), Hm) for p in prm.reshape(2 * F, 5)])
    init, fo, cl = ellipse_seeds_from_pred(torch.from_numpy(prm).to(DEV), H, W)
    assert fo.cpu().tolist() == [i // 2 for i in range(2 * F)] and cl.cpu().tolist() == [1, 2] * F
    got = init.cpu().numpy()
    print("seeds %dx%d F=%d: max abs diff %.3e" % (H, W, F, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11)
