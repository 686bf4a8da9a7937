"""CPU: the torch restatement of the self-consistency term (tests/selfcorr_refs.py, the reference of tests/test_gpu_selfcorr.py) against
what the reference's own loss.get_selfConsistency gave in float32 (tests/golden/selfcorr.npz part (a), make_golden_selfcorr.py).

Bound (small_op_refs.bound, the project's rule): four times the error of the restatement's own float32 run against its float64 run,
not below 4 fp32 ulps, relative to the output's absolute maximum.  The reference's gradient w.r.t. elPred is NaN in the pupil entries
of most cases (0 * log 0 in kl_div's target gradient); it is compared where the fixture says it is finite, and the float64
restatement must be finite everywhere."""
import os

import numpy as np
import pytest
import torch

import selfcorr_refs as S
import small_op_refs as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selfcorr.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def runs():
    """Per case: inputs, the float64 and the float32 run of the restatement (computed once, shared, never modified)."""
    out = {}
    for shape, okp, es in S.CASES:
        op, el, ok = S.case_inputs(shape, okp, es)
        out[(shape, okp, es)] = (op, el, ok, S.value_and_grads(op.double(), el.double(), ok.double()), S.value_and_grads(op, el, ok))
    return out


def _fixture(gold, case):
    k = "a_" + S.case_key(*case) + "_"
    return (torch.tensor(float(gold[k + "value"])), torch.from_numpy(gold[k + "g_op"]), torch.from_numpy(gold[k + "g_el"]),
            torch.from_numpy(gold[k + "g_el_finite"]))


def _within(name, got, ref64, cpu32):
    bnd, e32 = R.bound(ref64, cpu32)
    err = R.rel_err(got, ref64)
    print("%s: reference differs by %.3e (restatement fp32 %.3e, bound %.3e)" % (name, err, e32, bnd))
    return err <= bnd, err, bnd


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: S.case_key(*c))
def test_restatement_matches_the_reference(gold, runs, case):
    _, _, _, r64, r32 = runs[case]
    val, g_op, g_el, fin = _fixture(gold, case)
    for name, got, a, b in (("value", val, r64[0], r32[0]), ("g_op", g_op, r64[1], r32[1])):
        ok, err, bnd = _within(name, got, a, b)
        assert ok, "%s: %.3e above %.3e" % (name, err, bnd)
    assert fin[:, :5].all(), "the fixture's iris gradient is finite in every case"
    ok, err, bnd = _within("g_elPred (finite entries: %d of %d)" % (int(fin.sum()), fin.numel()),
                           torch.where(fin, g_el.double(), r64[2]), r64[2], r32[2])
    assert ok, "g_elPred: %.3e above %.3e" % (err, bnd)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: S.case_key(*c))
def test_float64_gradient_is_finite_where_the_reference_is_not(gold, runs, case):
    _, _, _, r64, r32 = runs[case]
    for t in r64 + r32:
        assert torch.isfinite(t).all()
    shape, okp, es = case
    if es == "typical" and okp != "none":
        assert not _fixture(gold, case)[3][:, 5:].all(), "the fixture records NaN for the typical pupil ellipse"
    if es == "covering":
        assert _fixture(gold, case)[3].all()


def test_none_ok_is_exactly_zero(runs):
    for case in S.CASES:
        if case[1] == "none":
            for t in runs[case][3] + runs[case][4]:
                assert (t == 0).all()


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_emulated_mistakes_are_caught(gold, runs, mistake):
    """Each mistake moves the weighted term (10 * term, what the models add to the loss) or one of its gradients beyond the bound
    on at least one case."""
    caught = []
    for case in S.CASES:
        op, el, ok, _, _ = runs[case]
        val, g_op, g_el, fin = _fixture(gold, case)
        r64 = S.value_and_grads(op.double(), el.double(), ok.double(), fn=S.weighted)
        r32 = S.value_and_grads(op, el, ok, fn=S.weighted)
        bad = S.value_and_grads(op, el, ok, mistake=mistake, fn=S.weighted)
        refs = (S.WEIGHT * val.double(), S.WEIGHT * g_op.double(), torch.where(fin, S.WEIGHT * g_el.double(), r64[2]))
        for name, got, ref, a, b in zip(("value", "g_op", "g_el"), bad, refs, r64, r32):
            got = torch.where(fin, got.double(), ref) if name == "g_el" else got
            bnd, _ = R.bound(a, b)
            scale = max(a.abs().max().item(), 1e-30)
            err = (got.double() - ref).abs().max().item() / scale
            if err > bnd:
                caught.append((S.case_key(*case), name, err, bnd))
    print("%s: caught %d times, e.g. %s" % (mistake, len(caught), caught[:2]))
    assert caught, "the emulated mistake %r passes every case" % mistake
