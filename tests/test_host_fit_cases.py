"""CPU: the oracle's counts (oracle.fit.ell_counts) and the case generators of tests/fit_cases.py that tests/test_gpu_fit.py holds the
fit kernel against -- the generators are deterministic and their population stays where the kernel's shortcuts are exercised."""
import numpy as np
import pytest

import fit_cases as fc
from common import gold
from oracle import fit as ofit


def test_ell_counts_reproduce_the_golden_scores():
    g = gold("fit_cases")
    H, W = 240, 320
    mesh = ofit.mesh_f32(H, W)
    m0 = np.unpackbits(g["masks"][0]).reshape(H, W).astype(bool)
    for i in range(8):
        el = list(g["inits"][i][:4]) + [g["inits"][i][4] * 180. / 3.14159]
        nseg, nell, inter = ofit.ell_counts(m0, el, mesh)
        assert nseg == int(m0.sum()) and 0 <= inter <= min(nseg, nell)
        f = np.float32
        assert float(f(inter) / f(f(f(nseg) + f(nell)) - f(inter))) == g["iou0"][i]
        assert ofit.score_of_counts(nseg, nell, inter) == g["iou0"][i]
        assert ofit.ell_iou(m0, el, mesh) == g["iou0"][i]


def test_generators_are_deterministic():
    for H, W in fc.SHAPES:
        a, b = fc.count_batch(H, W), fc.count_batch(H, W)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
        names, ell = fc.ellipses(H, W)
        assert len(names) == len(ell) == fc.N_RANDOM + 7 + len(fc.NONTAME) and len(set(names)) == len(names)
        assert set(np.unique(a[0])) <= set(fc.VALUES.tolist())
        assert (a[0][1] == 1).all() and not (a[0][2] == 3).any() and ((H, W) == (2, 2) or all((a[0][0] == c).any() for c in (1, 2)))
    for F in (1, 33, 65):
        assert np.array_equal(fc.seed_params(F), fc.seed_params(F)) and fc.seed_params(F).shape == (F, 10)
    for name in fc.SEARCHES:
        assert np.array_equal(fc.search_mask(name), fc.search_mask(name))


@pytest.mark.parametrize("H,W", fc.SHAPES[:-1])
def test_shared_rasterisation_equals_ell_counts(H, W):
    """oracle_counts rasterises an ellipse once for the nine class masks; every 7th row (and all hand-made ones of the first mask) must
    be what ell_counts itself returns."""
    mk, ell, fo, cl, idx = fc.count_batch(H, W)
    want = fc.oracle_counts(H, W)
    mesh = ofit.mesh_f32(H, W)
    rows = sorted(set(range(0, len(idx), 7)) | set(range(fc.N_RANDOM, len(fc.ellipses(H, W)[0]))))
    with np.errstate(all="ignore"):
        for i in rows:
            assert ofit.ell_counts(mk[fo[i]] == cl[i], ell[i], mesh) == tuple(int(v) for v in want[i]), (H, W, i)


@pytest.mark.parametrize("H,W", fc.SHAPES[1:])
def test_population_stays_in_the_hard_region(H, W):
    p = fc.population(H, W)
    print((H, W), p)
    assert p["interior"] >= 0.10 and p["clipped"] >= 0.40 and p["empty"] <= 0.35 and p["mixed_rows"] >= 0.08, p


@pytest.mark.parametrize("H,W", fc.SHAPES)
def test_hand_made_ellipses_are_what_their_names_say(H, W):
    names, _ = fc.ellipses(H, W)
    ins = fc.inside_maps(H, W)
    nell = {n: int(ins[i].sum()) for i, n in enumerate(names)}
    assert nell["cover"] == H * W
    for name, (_, _, kind) in fc.NONTAME.items():
        if (H, W) == (2, 2) and name in ("a=-3", "a=1e6"):
            kind = "empty"            # the exception: a band 0.6 px wide through (1, 1) passes between the four pixels
        assert (nell[name] == 0) == (kind == "empty"), (name, nell[name])
        assert 0 <= nell[name] <= H * W
    if (H, W) != (2, 2):
        for y, x, name in ((0, 0, "corner00"), (0, W - 1, "corner0W"), (H - 1, 0, "cornerH0"), (H - 1, W - 1, "cornerHW")):
            i = names.index(name)
            assert ins[i][y, x] and 0 < nell[name] < H * W
        for name in ("tangent_row0", "tangent_lastcol"):
            i = names.index(name)
            assert nell[name] > 0 and not ins[i][-1].any() and not ins[i][:, 0].any()


def test_search_cases_match_their_recorded_evaluation_counts():
    for name, case in fc.SEARCHES.items():
        out, nev = fc.oracle_search(name)
        assert nev == case[4], (name, nev)
    out, _ = fc.oracle_search("empty")
    init = fc.search_init("empty")
    assert np.array_equal(out[:4], init[:4]) and out[4] == init[4] * 180. / ofit.PI_REF / 180.0 * ofit.PI_REF


def test_tiny_search_scores_an_axis_of_exactly_zero(monkeypatch):
    seen = []
    real = ofit.ell_counts

    def spy(seg, el, mesh):
        seen.append(tuple(float(v) for v in el))
        return real(seg, el, mesh)

    monkeypatch.setattr(ofit, "ell_counts", spy)
    with np.errstate(all="ignore"):
        out, nev = ofit.fit_ellipse(fc.search_mask("tiny"), list(fc.search_init("tiny")), count_evals=True)
    assert nev == len(seen) == fc.SEARCHES["tiny"][4]
    assert any(e[2] == 0.0 or e[3] == 0.0 for e in seen)
    assert out[2] == 1.0
