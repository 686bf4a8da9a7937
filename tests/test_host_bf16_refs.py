"""tests/bf16_refs.py on the CPU: the conditions that make the exact runs of tests/test_gpu_bf16_sweep.py exact are asserted per row,
not assumed; every row's claimed template instantiation follows from the restated launch rule (and, where the library answers on the
host -- egne_conv2d_wgrad_splits, egne_conv_narrow_bf16_supported, egne_conv1x1_bf16_pack_elems, egne_conv1x1_bf16_multi_supported --
from the library itself, put to a descriptor with the row's sizes and dummy addresses); and the table as a whole claims every
instantiation of bf16_refs.REQUIRED, so that a later edit cannot drop one silently.

The float64 backward reference bf16_refs.train_ref is held against plain torch autograd through the whole graph of a row, so that a
wrong reference cannot vouch for the kernels.

Instantiations the table must claim (test_every_required_instantiation_is_claimed walks bf16_refs.REQUIRED): conv3x3_bf16.hip all 21
<KCH, MB, RM> of the default switches; conv1x1_bf16.hip the six streaming forms and multi <1|2|3|4|6|8>; conv_narrow_bf16.hip all six;
wgrad_bf16.hip pair, quad, the six 1x1 forms and a two-launch layer; backward.hip <bf16, BFM>, <.., FOLD>, wide <true> / <false> and
all-pairs <3, 64, bf16>.  Not claimed, hence not checked here: builds behind EGNE_* switches, the other all-pairs instantiations on bf16
tensors (the docstring of bf16_refs.py lists them per file).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import bf16_refs as S
import conv_refs as R

D = torch.float64


def _ids(rows):
    return [c["id"] for c in rows]


# ---- the rules -------------------------------------------------------------------------------------------------------------------

def _form(case):
    part = case["part"]
    if part == "fwd3":
        return S.b3_form(case)
    if part in ("fwd1", "multi"):
        return S.s1_form(case)
    if part == "narrow":
        return S.narrow_form(case)
    if part == "dgrad3":
        return tuple(f for _, f in S.dgrad3_forms(case))
    if part == "dgrad1":
        return tuple(f for _, f, _ in S.dgrad1_forms(case))
    return S.wgrad_form(case)


@pytest.mark.parametrize("case", S.BF16_SWEEP, ids=S.BF16_IDS)
def test_claimed_instantiation_follows_from_the_rule(case):
    assert _form(case) == case["inst"], (case["id"], _form(case), case["inst"])
    assert case["part"] in ("fwd3", "fwd1", "narrow", "dgrad3", "dgrad1", "multi", "wgrad3", "wgrad1", "wgrad_generic")


def test_every_required_instantiation_is_claimed():
    claimed = set()
    for case in S.BF16_SWEEP:
        claimed |= S.instantiations(case)
    missing = S.REQUIRED - claimed
    assert not missing, "no row reaches %s" % sorted(missing, key=str)
    assert len(set(S.BF16_IDS)) == len(S.BF16_IDS)


def test_forward_rows_of_the_training_rows_are_3x3_rules_too():
    """Single-layer training rows on the bf16 3x3 also pin their forward launch: the rule answers for them."""
    for case in S.TRAIN_ROWS:
        if case["fwd"] == S.B3 and case["layers"] is None:
            f = S.b3_form(case)
            assert f[0] == "b3" and f[3] == 0


def test_walk_arithmetic_of_the_rows_that_are_about_it():
    """The 3x3 forward: one row whose workers walk two tiles, the others with fewer tiles than workers; the weight gradients: per form
    one row with more tiles than splits and one with the split count capped by the tile count."""
    by = {c["id"]: c for c in S.BF16_SWEEP}
    c = by["b3-two-tiles-per-worker"]
    ntiles, nrun, nworkers = S.b3_walk(c["H"], c["W"], c["B"], S.cout_store(c), 2)
    assert (ntiles, nrun, nworkers) == (72, 4, 64) and nworkers < ntiles <= 2 * nworkers
    c = by["b3-k1-mb1"]
    assert S.b3_walk(c["H"], c["W"], c["B"], S.cout_store(c), 1) == (8, 1, 256)
    for id, tiles, cap in (("w3-pair-two-tiles", 72, 64), ("w3-quad-two-tiles", 72, 64), ("w3-pair-32-32", 8, 256), ("w3-quad-64-64", 4, 256)):
        c = by[id]
        t = ((c["W"] + 31) // 32) * ((c["H"] + 7) // 8) * c["B"]
        assert t == tiles and S.wgrad_form(c)[1] == min(tiles, cap)


def _desc(case, ly, gz_stride_pad=16):
    """egne_conv_desc of a layer of a row as the backward plan hands it to egne_conv2d_wgrad, with dummy (aligned, non-null) addresses:
    the host-side rules read sizes, offsets and whether pointers are set."""
    from egne_amd import _lib
    kh, kw = ly["k"]
    d = _lib.ConvDesc()
    d.dtype, d.B, d.H, d.W = 1, case["B"], case["H"], case["W"]
    d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.pad_mode, d.ngroups = kh, kw, ly["stride"], ly["pad"][0], ly["pad"][1], ly["pad_mode"], 1
    d.Ho, d.Wo = (case["H"] + 2 * ly["pad"][0] - kh) // ly["stride"] + 1, (case["W"] + 2 * ly["pad"][1] - kw) // ly["stride"] + 1
    for g in range(_lib.MAXGROUP):
        d.dil[g] = 1
    cps = [S.pad8(S.chans_of(case, s)) for s in ly["src"]]
    d.nseg = len(cps)
    off = 8
    for i, cp in enumerate(cps):
        sg = d.seg[i]
        sg.ptr, sg.pix_stride, sg.ch_off, sg.Cp = 4096, 16 + sum(cps), off, cp
        if i in ly["norm"]:
            sg.scale, sg.shift, sg.act_in = 4096, 4096, 1
        off += cp
    d.Ktot, d.CoutP = sum(cps), S.pad32(ly["Cout"])
    d.Cout_store = S.pad8(ly["Cout"])
    d.out, d.out_pix_stride, d.out_ch_off = 4096, d.Cout_store + gz_stride_pad, 8
    d.w = 4096
    return d


@pytest.mark.parametrize("case", S.TRAIN_ROWS, ids=_ids(S.TRAIN_ROWS))
def test_split_count_of_the_rule_is_the_library_s(case):
    """egne_conv2d_wgrad_splits is host code: the restated rule must give its answer for every layer of every training row."""
    from egne_amd import _lib
    L = _lib.lib()
    for ly in S.layers_of(case):
        want = int(L.egne_conv2d_wgrad_splits(C.byref(_desc(case, ly))))
        assert S.wgrad_form(case, ly)[-1] == want, (case["id"], ly["name"], S.wgrad_form(case, ly), want)


@pytest.mark.parametrize("case", S.NARROW, ids=_ids(S.NARROW))
def test_narrow_rows_pass_the_library_s_predicate(case):
    from egne_amd import _lib
    ly = S.layers_of(case)[0]
    d = _desc(case, ly)
    d.Cout_store = S.cout_store(case)
    assert int(_lib.lib().egne_conv_narrow_bf16_supported(C.byref(d))) == 1 and S.narrow_form(case) is not None
    d.residual = 4096                          # (a descriptor it refuses, for the predicate's sake)
    assert int(_lib.lib().egne_conv_narrow_bf16_supported(C.byref(d))) == 0
    assert S.narrow_form(dict(case, residual=True)) is None and S.narrow_form(dict(case, chans=(96,))) is None


def test_streaming_1x1_rows_fit_the_library_s_lds_budget():
    from egne_amd import _lib
    L = _lib.lib()
    for case in S.FWD1 + S.TRAIN1 + S.DGRAD1:
        for ly in S.layers_of(case):
            d = _desc(case, ly)
            n = int(L.egne_conv1x1_bf16_pack_elems(C.byref(d)))
            assert n == S.s1_steps([S.pad8(c) for c in case["chans"]]) * S.pad32(ly["Cout"]) * 32, case["id"]
        assert case["B"] * case["H"] * case["W"] >= S.S1_MIN_PIX


@pytest.mark.parametrize("case", S.MULTI_ROWS, ids=_ids(S.MULTI_ROWS))
def test_multi_rows_are_accepted_by_the_library_s_predicate(case):
    """Never launch what a predicate refuses: egne_conv1x1_bf16_multi_supported (host code) on the row's sizes."""
    from egne_amd import _lib
    L = _lib.lib()
    Cs, dsts = case["multi"]
    d = _lib.ConvDesc()
    d.dtype, d.B, d.H, d.W, d.Ho, d.Wo, d.nseg, d.Ktot = 1, case["B"], case["H"], case["W"], case["H"], case["W"], 1, S.pad8(Cs)
    d.seg[0].Cp = S.pad8(Cs)
    arr = (_lib.Dst * len(dsts))()
    for q, (Cd, _, _, _) in zip(arr, dsts):
        q.C, q.CoutP = S.pad8(Cd), S.pad32(Cd)
    assert int(L.egne_conv1x1_bf16_multi_supported(C.byref(d), len(dsts), arr)) == 1
    assert S.s1_form(case)[2] == S.s1_steps([S.pad8(Cs)]) <= 8
    assert sum(1 for _, _, _, s in dsts if s) <= 1 and all(S.pad32(Cd) <= 128 for Cd, _, _, s in dsts if s)


# ---- the data ----------------------------------------------------------------------------------------------------------------------

FWD_PLAIN = [c for c in S.FORWARD_ROWS if c["up"] is None]


@pytest.mark.parametrize("case", FWD_PLAIN, ids=_ids(FWD_PLAIN))
def test_forward_rows_are_exact(case):
    """conv_refs.int_conditions per row (asserted inside fwd_case): integers, stored tensors within +-256, power-of-two scales, partial
    sums below 2^24, half of the outputs non-zero."""
    data, want = S.fwd_case(case)
    R.int_conditions(case, data, want)
    if case["part"] == "narrow":
        assert all(x.abs().max().item() == 1 for x in data["xs"])
    if case["stats"]:
        # the statistics partials are fp64 sums of integers and of their squares: exact
        assert (want ** 2).sum((2, 3)).max().item() < 2 ** 53


UP_ROWS = [c for c in S.FWD1 if c["up"] is not None]


@pytest.mark.parametrize("case", UP_ROWS, ids=_ids(UP_ROWS))
def test_up_sampled_addend_is_an_fp32_value_before_the_store(case):
    """conv + bias + up2x(P) on integer data is a multiple of 1/16 below 2^24 / 16: an fp32 value whatever the order of the sum, so
    the stored bf16 bits are those of the float64 value rounded once."""
    data, P, pre = S.up_case(case)
    assert torch.equal(P, P.round()) and P.abs().max().item() <= 4
    assert torch.equal(pre * 16, (pre * 16).round()) and pre.abs().max().item() < 2 ** 24 / 16
    assert torch.equal(pre.float().double(), pre)
    assert R.abs_bound(case, data) + 4 < 2 ** 24 / 16
    # the interpolation itself: weights 9/16, 3/16, 3/16, 1/16 inside the map, edge pixels clamped
    up = F.interpolate(P.double(), scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.equal(up[:, :, 1, 1], (9 * P[:, :, 0, 0] + 3 * P[:, :, 0, 1] + 3 * P[:, :, 1, 0] + P[:, :, 1, 1]).double() / 16)
    assert torch.equal(up[:, :, 0, 0], P[:, :, 0, 0].double())
    assert ((pre.to(torch.bfloat16).double() != pre).double().mean().item()) > 0.05, "the row should exercise the rounding of the store"


@pytest.mark.parametrize("case", S.TRAIN_ROWS, ids=_ids(S.TRAIN_ROWS))
def test_training_rows_are_exact(case):
    data, ref = S.train_case(case)
    S.train_conditions(case, data, ref)
    print("%s: weight density %.4f, |gy| <= %d, max |y| %d, max |gx| %d, max |dW| %d, partial sums below %d"
          % (case["id"], data["density"], data["glim"], max(t.abs().max().item() for t in ref["y"].values()),
             max([0] + [t.abs().max().item() for t in ref["gx"].values()]), max(t.abs().max().item() for t in ref["dW"].values()), ref["bound"]))


@pytest.mark.parametrize("case", S.MULTI_ROWS, ids=_ids(S.MULTI_ROWS))
def test_multi_rows_are_exact(case):
    gz, dsts = S.multi_case(case)
    assert torch.equal(gz, gz.round()) and gz.abs().max().item() <= 4
    for q in dsts:
        t = q["want"]
        assert torch.equal(t, t.round()) and t.abs().max().item() <= 256 and (t[:, q["Cd"]:] == 0).all()
        # the per-wave channel sums are sums of stored integers in fp32: exact below 2^24
        assert t.abs().sum(0).max().item() < 2 ** 24


@pytest.mark.parametrize("id", ["d3-chain-cmid40", "d3-two-slices", "d1-merged-accumulate", "w1-1-128-cp40", "w3-pair-affine-cp40", "wg-4x4-s2-reflect-wide"])
def test_train_ref_is_plain_autograd_through_the_whole_graph(id):
    """train_ref walks the layers by hand (the plan's order of writers, masks from the stored outputs); on exact data that must be what
    torch autograd gives for sum_outputs <y, gy> through the whole graph in one go."""
    case = next(c for c in S.BF16_SWEEP if c["id"] == id)
    data, ref = S.train_case(case)
    xs = [x.double().requires_grad_(True) for x in data["xs"]]
    t = {"x%d" % i: x for i, x in enumerate(xs)}
    ws, bs = {}, {}
    for ly in S.layers_of(case):
        n = ly["name"]
        ws[n], bs[n] = data["w"][n].double().requires_grad_(True), data["b"][n].double().requires_grad_(True)
        ins = []
        for i, s in enumerate(ly["src"]):
            x = t[s]
            if i in ly["norm"]:
                sc, sh = data["affine"][(n, i)]
                x = F.relu(x * sc.double()[:, :, None, None] + sh.double()[:, :, None, None])
            ins.append(x)
        xin = torch.cat(ins, 1)
        ph, pw = ly["pad"]
        if ly["pad_mode"] == 1:
            z = F.conv2d(F.pad(xin, (pw, pw, ph, ph), mode="reflect"), ws[n], bs[n], stride=ly["stride"])
        else:
            z = F.conv2d(xin, ws[n], bs[n], stride=ly["stride"], padding=(ph, pw))
        t[n] = F.relu(z) if ly["act"] else z
        assert torch.equal(t[n].detach(), ref["y"][n])
    loss = sum((t[n] * gy.double()).sum() for n, gy in data["gy"].items())
    loss.backward()
    for ly in S.layers_of(case):
        n = ly["name"]
        assert torch.equal(ws[n].grad, ref["dW"][n]) and torch.equal(bs[n].grad, ref["db"][n]), (id, n)
    for i, x in enumerate(xs):
        if "x%d" % i in ref["gx"]:
            assert torch.equal(x.grad, ref["gx"]["x%d" % i]), (id, i)
