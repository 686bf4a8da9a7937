"""tests/split_refs.py on the CPU: for every row of the split-f16 sweep table and each of its three exact data generators, under the scales
the engine would choose, (1) the conditions that make the run exact hold (split_conditions), (2) the float64 emulation of the kernel's
arithmetic -- hi*hi + hi*lo + lo*hi, or hi*hi alone for rows of plain-f16 plans -- equals the expected value bit for bit, and (3) the data
is sensitive: an emulation that reads a lo half one pixel off, drops the lo halves of the last K chunk (tap), or drops the last channel
group differs from the reference.  (3) stands in for any fault injection on the GPU: it shows what tests/test_gpu_split_f16_sweep.py
would see if a kernel did that."""
import math

import pytest
import torch

import split_refs as S

D = torch.float64


def _a_scale(vmax):      # engine._a_scale_for, restated
    return 16.0 if vmax == 0.0 else 2.0 ** max(-100, min(100, math.floor(math.log2(2048.0 / vmax))))


def _w_scale(ws):        # ConvLayer.ensure_packed, restated
    mx = max(float(w.abs().max()) for w in ws)
    return 2.0 ** math.floor(math.log2(2048.0 / mx)) if mx > 0 else 1.0


def _scales(case, data):
    a = 16.0 if case["norm"] else _a_scale(max(float(x.abs().max()) for x in data["xs"]))
    return a, _w_scale(data["ws"])


def _hi_only(case, data, a, w):
    """Float64 convolution of the f16-rounded operands alone."""
    xt, wt = S.operands(case, data, a, w)
    return S.conv_ref([t.half().double() / a for t in xt], [t.half().double() / w for t in wt], data["bs"], stride=case["stride"], pad=case["pad"],
                      dils=case["dils"], act=data["act"], pad_mode=case["pad_mode"], residual=data["residual"], post=data["post"])


def test_split_restates_the_header():
    """hi = f16(t), lo = f16(t - hi): 2047.5 = 2048 - 0.5, 1234.5 = 1234 + 0.5, integers below 2049 have no lo half."""
    hi, lo = S.split_f16(torch.tensor([2047.5, 1234.5, 1500.0, -3071.5, 0.0]))
    assert hi.tolist() == [2048.0, 1234.0, 1500.0, -3072.0, 0.0] and lo.tolist() == [-0.5, 0.5, 0.0, 0.5, 0.0]
    assert S.a_scale_for(2047.5) == 1.0 and S.a_scale_for(4.0) == 512.0 and S.a_scale_for(2048.5) == 0.5
    assert S.w_scale_for([torch.tensor([2.0, -1.0])]) == 1024.0 and S.w_scale_for([torch.tensor([0.5]), torch.tensor([-2047.5])]) == 1.0


def test_the_table_covers_what_it_is_meant_to():
    ids = S.SPLIT_IDS
    assert len(set(ids)) == len(ids) == 43
    kinds = {c["kind"].split(":")[1] for c in S.SPLIT_SWEEP}
    assert kinds == {"halo", "rs", "rw", "flat", "small", "big", "stream1x1", "gemm1x1", "msdil", "lattice", "first"}
    for c in S.SPLIT_SWEEP:
        assert c["switches"]["SMALL_ENABLED"] == (c["kind"] == "conv_f16x3:small"), c["id"]
        assert c["products"] in (1, 3) and c["runs"] == (2 if c["kind"] == "conv_f16x3:small" else 1)
        assert c["launches"] == (3 if c["kind"] == "conv_f16x3:lattice" else 1)
        assert not (c["norm"] and len(c["chans"]) > 1)
    assert sum(c["products"] == 1 for c in S.SPLIT_SWEEP) == 4 and sum(c["stats"] for c in S.SPLIT_SWEEP) == 6


@pytest.mark.parametrize("case", S.SPLIT_SWEEP, ids=S.SPLIT_IDS)
def test_out_hw_agrees_with_the_layer_arithmetic(case):
    """conv_refs.out_hw against ConvLayer.out_hw's formula and the reference's own shape; normal_case's shapes and dtypes."""
    kh, kw = case["k"]
    d = case["dils"][0]
    ho = (case["H"] + 2 * case["pad"][0] * d - d * (kh - 1) - 1) // case["stride"] + 1
    wo = (case["W"] + 2 * case["pad"][1] * d - d * (kw - 1) - 1) // case["stride"] + 1
    assert S.out_hw(case) == (ho, wo) == (case["H"], case["W"]) or case["id"] == "flat-32taps"
    assert S.out_hw(case) == (ho, wo)
    small = dict(case, B=1)
    data = S.normal_case(torch.Generator().manual_seed(5), small)
    assert [tuple(x.shape) for x in data["xs"]] == [(1, c, case["H"], case["W"]) for c in case["chans"]]
    assert all(tuple(w.shape) == (case["Cout"], sum(case["chans"])) + case["k"] and w.dtype == torch.float32 for w in data["ws"])
    assert len(data["ws"]) == len(data["bs"]) == len(case["dils"]) and all(x.dtype == torch.float32 for x in data["xs"])
    assert (data["residual"] is not None) == case["residual"] and (data["post"] is not None) == case["post"]
    assert data["act"] == case["act"] and set(data["norm"] or {}) == set(case["norm"])
    if case["residual"]:
        assert tuple(data["residual"].shape) == (1, case["Cout"], ho, wo)


@pytest.mark.parametrize("kind", list(S.GENERATORS))
@pytest.mark.parametrize("case", S.SPLIT_SWEEP, ids=S.SPLIT_IDS)
def test_exact_data_is_exact_and_sensitive_for_the_row(case, kind):
    data, want, a, w = S.exact_case(kind, case)
    assert (a, w) == _scales(case, data), "split_refs.scales_for differs from the engine's rule"
    assert a == (16.0 if case["norm"] else {"int": 512.0, "fine_inputs": 1.0, "fine_weights": 512.0}[kind])
    assert w == (1.0 if kind == "fine_weights" else 1024.0)
    units = S.split_conditions(case, data, want, a, w)
    dens = S.lo_density(case, data, a, w) if data["fine"] else 0.0
    print("%s / %s: weight density %.3f, largest partial sum %.3g units, lo density %.1f %%, max |y| %g"
          % (case["id"], kind, data["density"], units, 100 * dens, want.abs().max().item()))
    # the kernel's arithmetic, restated: bit-equal to the reference (three products), or to the convolution of the hi halves (one)
    got = S.emulate(case, data, a, w, case["products"])
    full = got if case["products"] == 3 else S.emulate(case, data, a, w, 3)
    assert torch.equal(full, want), "hi*hi + hi*lo + lo*hi differs from the float64 reference"
    if case["products"] == 1:
        assert torch.equal(got, _hi_only(case, data, a, w))
        assert torch.equal(got, want) == (kind == "int"), "a fine run must tell one product from three"
    # the same value in fp32, in torch's own order of summation
    got32 = S.conv_ref(data["xs"], data["ws"], data["bs"], stride=case["stride"], pad=case["pad"], dils=case["dils"], act=data["act"],
                       pad_mode=case["pad_mode"], norm=data["norm"], residual=data["residual"], post=data["post"], dtype=torch.float32)
    assert torch.equal(got32.to(D), want)
    for wt in data["ws"]:
        assert (wt.abs().sum(dim=0) > 0).all(), "a (channel, tap) pair without any weight"
    if kind == "int":
        assert not torch.equal(S.emulate_last_group_dropped(case, data, a, w), want)
    else:
        hi1 = S.emulate(case, data, a, w, 1)
        frac = (hi1 != want).double().mean().item()
        assert frac > 0.5, "dropping every lo half changes only %.0f %% of the outputs" % (100 * frac)
        assert not torch.equal(S.emulate_lo_shifted(case, data, a, w), want), "a lo half read one pixel off goes unnoticed"
        assert not torch.equal(S.emulate_lo_tail_dropped(case, data, a, w), want), "a dropped lo K tail goes unnoticed"
    if case["norm"]:
        for sc, sh, _ in data["norm"].values():
            assert sc.shape[0] == case["B"] and (sc[0] != sc[1]).any() and (sh[0] != sh[1]).any()


def _row(id):
    return next(c for c in S.SPLIT_SWEEP if c["id"] == id)


def _cdiv(a, b):
    return -(-a // b)


def test_rows_reach_the_edge_they_name():
    """The launchers' own arithmetic, restated for the rows whose purpose is a count: which walk the halo kernel takes and how many tiles
    a workgroup gets (launch_hf / launch_hf_tp of conv_halo_f16.hip: 32x8 tiles, 512 / ny workgroups), the role-split kernels' tiles
    over 256 workgroups (launch_rs: 32 x TH, TH 8 for Ktot 32 and 4 for 64), the flat kernel's tile by pack width and its small-problem
    plan (small_plan of conv_f16x3.hip: target 640 workgroups, at least 6 K steps per split), the deep kernel's ragged last tile."""
    def halo(c):      # (tiles per frame of the plain walk, of the transposed walk)
        return _cdiv(c["W"], 32) * _cdiv(c["H"], 8), _cdiv(c["H"], 32) * _cdiv(c["W"], 8)
    assert halo(_row("halo-n32")) == (4, 5) and _row("halo-n32")["W"] % 32 == 1 and _row("halo-n32")["H"] % 8 == 1
    assert halo(_row("halo-n64-tall")) == (16, 12)
    for id in ("halo-n96", "halo-tail16-n192", "halo-np1", "lattice-123"):
        n, t = halo(_row(id))
        assert n <= t, id                                   # plain walk
    c = _row("halo-second-tile")
    assert halo(c)[0] * c["B"] == 528 and c["dils"] == (2,) and S.pad32(c["Cout"]) == 32      # one N tile: 512 workgroups
    assert S.pad8(_row("halo-tail16-n192")["chans"][0]) % 32 == 8 and _cdiv(_row("halo-tail16-n192")["Cout"], 64) == 3
    for id, ktot, coutp, th in (("rs-1x1x8", 32, 32, 8), ("rs-1x2x8", 32, 64, 8), ("rs-2x1x4", 64, 32, 4), ("rs-2x2x4-affine", 64, 64, 4),
                                ("rs-2x4x4", 64, 128, 4), ("rs-tpo-64-64", 64, 64, 4), ("rs-tpo-64-32-res", 64, 32, 4)):
        c = _row(id)
        cp = S.pad32(c["Cout"])
        assert (S.pad32(S.pad8(c["chans"][0])), cp if cp <= 64 else _cdiv(cp, 64) * 64) == (ktot, coutp), id
        assert c["W"] >= 60 and _cdiv(c["W"], 32) * _cdiv(c["H"], th) * c["B"] <= 256, id
    assert _row("rs-1x1x8")["W"] % 32 == 1 and _row("rs-1x1x8")["H"] % 8 == 1 and _row("rs-2x1x4")["H"] % 4 == 1
    assert _row("rs-2x2x4-affine")["chans"][0] % 32 == 24 and S.pad8(_row("rs-2x4x4")["Cout"]) == 104
    for id in ("rs-tpo-64-64", "rs-tpo-64-32-res"):       # the transposed store needs Cout_store == CoutP and no statistics
        assert _row(id)["Cout"] % 32 == 0 and not _row(id)["stats"] and _row(id)["switches"]["RW_ENABLED"] is False
    c = _row("rs-second-tile")
    assert _cdiv(c["W"], 32) * _cdiv(c["H"], 4) * c["B"] == 272
    c = _row("rw-3of4-second-tile")
    assert _cdiv(c["W"], 32) * _cdiv(c["H"], 8) * c["B"] == 81 and _cdiv(c["Cout"], 32) == 3
    assert _row("rw-streamed")["W"] >= 120 and _row("rw-streamed")["chans"][0] // 32 == 4
    c = _row("rw-streamed-tail")
    assert c["W"] >= 120 and S.pad32(c["chans"][0]) == 96 and c["chans"][0] % 32 == 8 and S.pad8(c["Cout"]) == 24
    for id in ("halo-np1", "rw-np1"):
        assert 30 <= _row(id)["W"] < 60 and _row(id)["products"] == 1
    # ---- flat: the pack is 128 rows wide above 64 outputs, else pad32; M = 270 = 256 + 14
    for id, tile in (("flat-256x32", 32), ("flat-256x64-5x5", 64), ("flat-128x128-dil3", 128), ("flat-32taps", 32), ("flat-grouped", 32), ("flat-1x1-res", 32)):
        c = _row(id)
        G = len(c["dils"])
        coutp = _cdiv(c["Cout"], 128) * 128 if (c["Cout"] > 64 and G == 1) else S.pad32(c["Cout"])
        assert (128 if coutp % 128 == 0 and G == 1 else (64 if coutp % 64 == 0 and G == 1 else 32)) == tile, id
        assert c["W"] < 30, id                              # below the halo kernels' narrowest map
    assert _row("flat-256x32")["B"] * 90 == 270 and _row("flat-32taps")["k"] == (4, 8)
    # ---- small_plan
    def small(c):
        Ho, Wo = S.out_hw(c)
        M, cp = c["B"] * Ho * Wo, S.pad8(c["chans"][0])
        coutp = _cdiv(c["Cout"], 128) * 128 if c["Cout"] > 64 else S.pad32(c["Cout"])
        nsteps = c["k"][0] * c["k"][1] * _cdiv(cp, 32)
        tiles = _cdiv(M, 128) * (coutp // 128) if coutp % 128 == 0 else _cdiv(M, 256) * (coutp // (64 if coutp % 64 == 0 else 32))
        assert tiles < 192
        wide = coutp % 128 == 0 and nsteps >= 48 and tiles * (nsteps // 6) >= 640
        t2 = tiles if wide else (_cdiv(M, 64) * (coutp // 64) if coutp % 64 == 0 else _cdiv(M, 128) * (coutp // 32))
        return ("128x128" if wide else ("64x64" if coutp % 64 == 0 else "128x32")), max(1, min(_cdiv(640, t2), nsteps // 6, 16))
    assert small(_row("small-64x64-z6")) == ("64x64", 6)
    assert small(_row("small-128x32-z3-epilogue")) == ("128x32", 3)
    assert small(_row("small-wide")) == ("128x128", 16)
    # ---- deep trunk kernels: at least 256 * 128 output rows, a ragged last 256-row tile, the four-stage form on an even step count only
    for id in ("big-n256", "big1", "big-np1-n128"):
        c = _row(id)
        M = c["B"] * c["H"] * c["W"]
        assert M >= 256 * 128 and M % 256 and (c["H"] * c["W"]) % 256 and c["Cout"] % 128 == 0 and c["chans"][0] % 32 == 0
        steps = c["chans"][0] // 32 * 9
        assert (steps % 2 == 0) == (id != "big-np1-n128")
    assert _row("big-np1-n128")["Cout"] % 256 != 0 and _row("big-n256")["Cout"] % 256 == 0
    # ---- 1x1: M no multiple of 32, slices with 8- and 16-channel tails, what keeps the staged rows off the streaming kernel
    assert _row("s1x1-two-slices")["B"] * 63 == 189 and [S.pad8(c) % 16 for c in _row("s1x1-ragged-slices")["chans"]] == [8, 0, 8]
    assert S.pad32(_row("ms1x1-n96")["Cout"]) == 96 and sum(_row("ms1x1-k549")["chans"]) == 549
    # ---- dilated groups: the one-launch kernel takes 32 -> 32 with (4, 8, 12); the lattice launches need W // dilation >= 20
    assert _row("msdil-small-map")["H"] < 12 and _row("lattice-4812")["W"] // 12 == 20 and _row("lattice-123")["W"] // 3 == 20
    assert _row("lattice-4812")["chans"] == (64,)           # (64 input channels keep it off the one-launch kernel)
