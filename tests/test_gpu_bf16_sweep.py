"""-m gpu: addressing sweep of the kernels that carry training plans with bf16 activation storage, on data for which they must be
BIT-EQUAL to float64 -- forward outputs and data gradients as stored bf16, weight and bias gradients as fp32, statistics partials and
mask sums as exact integers.

Every row of bf16_refs.BF16_SWEEP runs through a training plan (Plan(train=True, dtype=bfloat16), build_backward()) and is pinned
before anything is compared: the kinds in Plan.meta, the _lib entry of every launch, the descriptor fields the restated launch rule
reads (bf16_refs.b3_form / s1_form / narrow_form / wgrad_form) and, for weight gradients, egne_conv2d_wgrad_splits against the rule's
split count.  The multi-destination 1x1 at a chosen k-step count is driven through its C entry, with descriptors its own predicate
accepts (tests/test_host_bf16_refs.py checks that on the host).  Every row runs twice:

(a) integer data (bf16_refs.fwd_case / train_case / multi_case; the conditions that make it exact are asserted per row on the CPU by
    tests/test_host_bf16_refs.py): torch.equal with the float64 reference, whatever the order of summation.  Up-sampled-addend rows:
    the value before the store is an fp32 value (a multiple of 1/16), so the stored bits are the float64 value rounded once to bf16.
(b) seeded normal data with bf16-representable stored tensors and weights, LeakyReLU where the row has an activation, under the bounds
    the project already holds: EPS = 2^-8 of the largest element (test_gpu_bf16.py) for bf16 tensors; 3e-3 / 2e-5 / 1e-5 for 3x3 weight,
    1x1 weight and bias gradients (test_weight_and_data_gradients_bf16_storage) on every row, the generic weight-gradient rows included;
    the 7x7 and 4x4 weight gradients, which that test has no figure for, 3e-3 (test_style_encoder_layers_bf16_storage).  No tighter bound
    is asserted here; the measured figures are below.
    ONE DEVIATION from "EPS for bf16 tensors", not an imported bound: a gradient slice with two writers is stored twice, and each store
    rounds by up to half an ulp, 2^-8 of the state it stores.  Its bound is EPS x (max |first state| + max |final state|), between EPS and
    2 EPS of the final state (7.3e-3 for d1-merged-accumulate); it holds for that row and for the input slice of every chain row, which
    measure 2.9e-3 .. 4.4e-3.  Two ideal roundings emulated on the CPU give d1-merged-accumulate's measured 4.1e-3 / 4.4e-3 to three
    digits: a single EPS cannot be met by any kernel that stores twice.  (test_gpu_bf16.py holds twice-rounded gradients to 2 EPS.)

Input slices sit behind eight poisoned channels (768) and in front of eight more, outputs and gradient slices between two poisoned
blocks; the padding channels of every stored slice must come back as zeros.  Every plan runs its forward twice and its backward twice
and must repeat its bits.

Template instantiations the rows reach, per kernel file (bf16_refs.REQUIRED; the host test walks the set):
  conv3x3_bf16.hip   forward: <KCH, MB, RM> = <1|2|3|4|streamed, 1, 0>, <1|2|streamed, 2, 0>, <2, 1, 1>, <2, 2, 1>, with ragged tiles in x and y,
                     a 128-channel pack of which 104 are stored, blocks 64 + 64 + 32, Cp 40 under the fused affine + ReLU, 3 outputs stored
                     as 8, a deep-K tiny map, a worker that walks two tiles, statistics partials (ragged and full tiles).  Data gradient
                     (BfDgradLayer, pack_weight_bf16frag_dgrad_k): first writer <.., 0>; second writer <1|2|3|4|streamed, 1, 1> and
                     <1|2|streamed, 2, 1>; last writer with the producer's mask and bias sums <1|2|3|4|streamed, 1, 2> (Cmid 32, 64, padded 40,
                     96, 128, 160); c0 = 0 / 64 of a two-slice layer; 100 -> 38.  That is every <KCH, MB, RM> the launcher's default switches can
                     choose: 15 with MB = 1 and 6 with MB = 2 (MB = 2 has no RM = 2 and no KCH 3 / 4).  Not reached: the RW = 1 builds behind
                     EGNE_B3_RW and the one-block forms behind EGNE_B3_MB (opt-in: out of scope).
  conv1x1_bf16.hip   streaming <NB16, NW, UP> = <2, 4>, <4, 4>, <4, 8> plain and with the up-sampled addend (15x20 -> 30x40, odd half size 13x17);
                     Cp 40, pixel count 4230, 16 k-steps with ragged slice ends, CoutP 96 / 128 / 192, accumulated residual; as a data gradient
                     the merged launch over adjacent slices, first writer and accumulating second writer (d1-merged-accumulate).  Multi-destination
                     <NKS> = 1, 2, 4 (last step 8 channels), 6 (five steps), 8 (seven and eight steps) through the C entry; residual, res_pixels
                     ending mid-group, ReLU mask, per-wave channel sums; four rows through the plan (name.dgrad_multi, k-steps and
                     destinations asserted): <1> with three destinations and with one, <2> with three, <3> with two (w1-4-64-store88).
  conv_narrow_bf16.hip  <7,2> <7,1> <5,2> <5,1> <3,2> <3,1>, Cout 3 (Cout_store 4) and 5 .. 8, pad (0, 1) and valid, ragged tiles, 270 tiles on
                     256 workgroups (0.5 s with its reference).  All six instantiations: none left out.
  wgrad_bf16.hip     pair form (32 -> 32 ragged, Cout 64 over Ktot 32, three input blocks, affine on load with Cp 40, W = 16 and 17, two tiles
                     per workgroup), quad form (one full quad, quads with missing pairs, Cout_store 104, Ktot 40, two tiles per workgroup), 1x1
                     <1,256> <1,128> <2,128> <2,64> <4,64> <8,64> and a two-launch layer (459 -> 153).
  backward.hip       conv_wgrad_kernel<bf16, BFM> (3x3 on W = 13; 1x1 on 600 pixels), <.., FOLD> (7x7 on 3 channels, CoutP 32),
                     conv_wgrad_wide_kernel<true> (7x7, CoutP 64) and <false> (4x4 / stride 2 / reflect, CoutP 128),
                     conv1x1_wgrad_allpairs_kernel<3, 64, bf16>: the 1x1 with nco * nkc = 12 that wgrad1x1_bf16_supported refuses (a slice with
                     an affine on load).  Not reached: the other all-pairs instantiations on bf16 tensors (same code as the fp32 ones of
                     test_gpu_conv_backward_fp32.py), conv_wgrad_kernel<bf16, false> (behind EGNE_IGEMM_BF16_MFMA=0: out of scope).
Out of scope: the fused norm-backward kernels, elementwise bf16 twins, builds behind EGNE_* switches.

Measured on MI355X: all 73 exact runs (16 fwd3, 8 fwd1 of which 3 with the up-sampled addend, 7 narrow, 36 training and 6 multi-destination
rows; a training row compares y, gz, dW and db of every layer and gx of every slice) are bit-equal, the statistics partials and channel
sums exact, and every plan repeats its bits.  Normal data, relative to the largest element: stored bf16 tensors fwd3 1.9e-3 .. 3.4e-3, fwd1
2.1e-3 .. 3.1e-3, narrow 1.9e-3 .. 3.0e-3, multi 1.9e-3 .. 3.2e-3, training rows outputs 1.5e-3 .. 3.6e-3, masked gradients 0 .. 3.1e-3,
once-stored data gradients 1.9e-3 .. 3.4e-3 (bound 3.9e-3: the rounding of the store), twice-stored ones 2.9e-3 .. 4.4e-3 (see (b)); 3x3
weight gradients 8.9e-8 .. 1.6e-7 (bound 3e-3), 1x1 weight gradients 1.2e-7 .. 2.9e-7 (bound 2e-5), 7x7 / 4x4 8.9e-8 .. 2.3e-7 (bound 3e-3),
bias gradients 0 .. 5.8e-8 (bound 1e-5), rstd / shift from the statistics partials 5.7e-8 / 1.2e-7 (bound 2e-6).  The 3x3 weight gradient
sits FOUR orders below its 3e-3 bound once the reference rounds an affined operand to bf16 as the kernel does (2.1e-3 without that, on
the one row with an affine): 1e-6 is the figure a later tightening would start from.  Per row in the docstrings of the three normal-data
tests.  The file's 146 tests take 8.3 s of wall time, float64 references included (the largest, w3-quad-two-tiles, is 2 GFLOP).
"""
import ctypes as C

import pytest
import torch

import bf16_refs as S
import conv_refs as R
from test_gpu_bf16 import EPS
from test_gpu_conv_igemm_sweep import DEV, POISON

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
# The parameter-gradient bounds of test_gpu_bf16.py::test_weight_and_data_gradients_bf16_storage: 3x3 weight, 1x1 weight, bias.  That test
# holds them as literals inside its body, so there is no name to import (EPS above is imported): they are restated here, unchanged.
WGRAD3_BOUND, WGRAD1_BOUND, BIAS_BOUND = 3e-3, 2e-5, 1e-5
# 7x7 and 4x4 weight gradients, for which that test has no figure: the 3e-3 of test_style_encoder_layers_bf16_storage
OTHER_K_W_BOUND = 3e-3
ENTRY = {S.B3: "egne_conv3x3_bf16_fwd", S.S1: "egne_conv1x1_bf16_fwd", S.NA: "egne_conv_narrow_bf16_fwd", S.IG: "egne_conv2d_fwd"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import egne_amd  # noqa: F401
    return True


def _ids(rows):
    return [c["id"] for c in rows]


def _slices(pl, xs, B, H, W):
    """NCHW CPU tensors -> padded slices of one NHWC bf16 buffer, behind eight poisoned channels and in front of eight more."""
    from egne_amd.engine import Piece
    buf = pl.buf(B, H, W, 16 + sum(S.pad8(x.shape[1]) for x in xs))
    buf.fill_(POISON)
    pieces, off = [], 8
    for x in xs:
        c = x.shape[1]
        buf[..., off:off + S.pad8(c)] = 0
        buf[..., off:off + c] = x.permute(0, 2, 3, 1).to(DEV).to(BF)
        pieces.append(Piece(buf, off, c))
        off += S.pad8(c)
    return pieces


def _stored(t, off, C_, Cs, what):
    """The slice [off, off + Cs) of an NHWC tensor between two poisoned blocks, as NCHW float64 on the CPU: poison intact, padding
    channels zero."""
    o = t.float().cpu()
    assert (o[..., :off] == POISON).all() and (o[..., off + Cs:] == POISON).all(), "%s: wrote outside its slice" % what
    if C_ < Cs:
        assert (o[..., off + C_:off + Cs] == 0).all(), "%s: padding channels must be zeros" % what
    return o[..., off:off + C_].permute(0, 3, 1, 2).contiguous().double()


def _launches(pl, name):
    """(kind, function, arguments) of the launches of ``pl`` named exactly ``name``."""
    return [(m[0], c[0], c[1]) for m, c in zip(pl.meta, pl.calls) if c[2] == name]


def _affine(pl, piece, sc, sh, act_in, B):
    scp, shp = torch.zeros(B, piece.Cp, device=DEV), torch.zeros(B, piece.Cp, device=DEV)
    scp[:, :sc.shape[1]], shp[:, :sh.shape[1]] = sc.to(DEV), sh.to(DEV)
    pl.keep += [scp, shp]
    return piece.with_norm(scp, shp, act_in)


def _report(case, got, want, what):
    bad = got != want
    if bad.any():
        idx = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements of %s differ; first at %s: got %r, want %r"
                             % (case["id"], int(bad.sum()), bad.numel(), what, idx, got[tuple(idx)].item(), want[tuple(idx)].item()))
    assert torch.equal(got, want), what


# ---- forward rows ------------------------------------------------------------------------------------------------------------------

def _run_forward(case, data, P=None):
    """One Plan.conv of a forward row on ``data``, pinned to the row's kernel and instantiation; two runs, identical bits.  Returns the
    stored result (NCHW float64), the plan and the launch's descriptor."""
    from egne_amd.engine import ConvLayer, Piece, Plan
    B, H, W, Cout = case["B"], case["H"], case["W"], case["Cout"]
    pl = Plan(torch.device(DEV), train=True, dtype=BF)
    pieces = _slices(pl, data["xs"], B, H, W)
    layer = ConvLayer([torch.nn.Parameter(data["ws"][0].to(DEV))], [torch.nn.Parameter(data["bs"][0].to(DEV))], [(p.C, p.Cp) for p in pieces],
                      pad=case["pad"], act=data["act"], cout_pad=case["cout_pad"])
    for i, (sc, sh, act_in) in (data["norm"] or {}).items():
        pieces[i] = _affine(pl, pieces[i], sc, sh, act_in, B)
    Ho, Wo = layer.out_hw(H, W)
    assert (Ho, Wo) == R.out_hw(case)
    out = pl.buf(B, Ho, Wo, S.pad8(Cout) + 16)
    out.fill_(POISON)
    dst = Piece(out, 8, Cout)
    res = _slices(pl, [data["residual"]], B, Ho, Wo)[0] if data["residual"] is not None else None
    up = None
    if P is not None:
        ph, pw = case["up"]
        Pb = pl.buf(B, ph, pw, S.pad8(Cout))
        Pb[..., :Cout] = P.permute(0, 2, 3, 1).to(DEV).to(BF)
        up = (Piece(Pb, 0, Cout), ph, pw)
        assert pl.bf16_stream1x1_ok(layer, pieces, dst, B, H, W)
    pl.conv(layer, pieces, dst, B, H, W, residual=res, name="sweep", stats=case["stats"], partials=case["stats"], up_add=up)
    # ---- the row is about ONE kernel and ONE instantiation of it
    hits = _launches(pl, "sweep")
    assert [h[0] for h in hits] == [case["fwd"]], "%s: planned as %s" % (case["id"], [h[0] for h in hits])
    assert hits[0][1] is getattr(pl.L, ENTRY[case["fwd"]]), case["id"]
    d = hits[0][2][0]._obj
    cps = [S.pad8(c) for c in case["chans"]]
    assert (d.dtype, d.B, d.H, d.W, d.CoutP, d.Cout_store, d.nseg) == (1, B, H, W, S.pad32(Cout), S.cout_store(case), len(cps))
    assert [d.seg[i].Cp for i in range(d.nseg)] == cps and bool(d.seg[0].scale) == bool(case["norm"])
    assert bool(d.residual) == (case["residual"] or P is not None) and not d.mask_y and bool(d.stats_ws) == case["stats"]
    part = case["part"]
    if part == "fwd3":
        assert d.Ktot == S.pad32(cps[0]) and S._b3(d.seg[0].Cp, d.CoutP, 1 if d.residual else 0) == case["inst"] == S.b3_form(case)
    elif part == "fwd1":
        assert d.Ktot == sum(cps) and (d.Ho, d.Wo) == (case["up"] or (H, W)) and S.s1_form(case) == case["inst"]
    else:
        assert d.Ktot == cps[0] and (d.kh, d.kw) == case["k"] and int(pl.L.egne_conv_narrow_bf16_supported(C.byref(d))) == 1
        assert S.narrow_form(case) == case["inst"]
    first = None
    for _ in range(2):
        pl.run()
        torch.cuda.synchronize()
        got = _stored(out, 8, Cout, int(d.Cout_store), case["id"])
        if first is None:
            first = got
        assert torch.equal(got, first), "%s: a second run of the same plan gives other bits" % case["id"]
    return first, pl, d


FWD_PLAIN = [c for c in S.FORWARD_ROWS if c["up"] is None]
UP_ROWS = [c for c in S.FORWARD_ROWS if c["up"] is not None]


@pytest.mark.parametrize("case", FWD_PLAIN, ids=_ids(FWD_PLAIN))
def test_forward_integer_data_is_bit_equal(gpu, case):
    """(a) forward rows: torch.equal with float64.  Rows with statistics: the partial sums the epilogue leaves in stats_ws, summed over
    the chunks of a frame, are the exact integer sum and sum of squares of the stored output per (frame, channel); last_stats under the
    tolerances of test_statistics_from_the_bf16_3x3_epilogue (2e-6, per (sample, channel))."""
    data, want = S.fwd_case(case)
    got, pl, d = _run_forward(case, data)
    print("%s %s: weight density %.3f, max |y| %d, %d of %d outputs differ" % (case["id"], case["inst"], data["density"], want.abs().max().item(),
                                                                               int((got != want).sum()), want.numel()))
    _report(case, got, want, "the output")
    if case["stats"]:
        ws, nchunk, Cs = pl.last_partials
        assert nchunk == ((case["W"] + 31) // 32) * ((case["H"] + 7) // 8) * 4 and Cs == int(d.Cout_store)
        part = ws.cpu().view(case["B"], nchunk, Cs, 2).sum(1)
        Cout = case["Cout"]
        _report(case, part[:, :Cout, 0], want.sum((2, 3)), "the sums of the statistics partials")
        _report(case, part[:, :Cout, 1], (want ** 2).sum((2, 3)), "the sums of squares of the statistics partials")
        assert (part[:, Cout:] == 0).all()
        sc, sh = pl.last_stats
        m_, v_ = want.mean((2, 3)), want.var((2, 3), unbiased=False)
        want_sc = 1.0 / torch.sqrt(v_ + 1e-5)
        e1 = ((sc.cpu().double()[:, :Cout] - want_sc).abs() / want_sc).max().item()
        e2 = ((sh.cpu().double()[:, :Cout] + m_ * want_sc).abs() / (m_ * want_sc).abs().clamp_min(1e-3)).max().item()
        print("%s: rstd / shift from the epilogue %.2e / %.2e" % (case["id"], e1, e2))
        assert e1 < 2e-6 and e2 < 2e-6


@pytest.mark.parametrize("case", UP_ROWS, ids=_ids(UP_ROWS))
def test_up_sampled_addend_integer_data_is_the_float64_value_rounded_once(gpu, case):
    """(a) conv1x1 + bias + up2x(P): exact before the store (host test), so the stored bf16 bits are determined."""
    data, P, pre = S.up_case(case)
    got, _, _ = _run_forward(case, data, P)
    want = pre.float().to(BF).double()
    print("%s %s: max |value| %g, %d of %d outputs differ, %.0f %% of the values are rounded by the store"
          % (case["id"], case["inst"], pre.abs().max().item(), int((got != want).sum()), want.numel(), 100 * (want != pre).double().mean().item()))
    _report(case, got, want, "the output")


@pytest.mark.parametrize("case", S.FORWARD_ROWS, ids=_ids(S.FORWARD_ROWS))
def test_forward_normal_data_within_the_project_bound(gpu, case):
    """(b) forward rows against float64 on the same stored values and bf16-rounded weights: EPS of the largest output.  Relative error on
    MI355X, per row:
      b3-k1-mb1 2.37e-03; b3-k2-mb1-res 2.74e-03; b3-k2-mb1 1.98e-03; b3-k3-mb1 1.85e-03; b3-k4-mb1 2.53e-03; b3-streamed-mb1 2.01e-03;
      b3-k1-mb2-stats 3.25e-03; b3-k2-mb2-res 2.62e-03; b3-streamed-mb2-180 3.21e-03; b3-104-of-128 2.61e-03; b3-64-64-32 2.57e-03;
      b3-cin38-affine 3.03e-03; b3-cout3 1.99e-03; b3-deep-k-tiny-map 1.95e-03; b3-two-tiles-per-worker 2.80e-03;
      b3-k1-mb1-stats-full-tiles 3.45e-03; s1-nb2 3.12e-03; s1-nb2-cout96-res 2.12e-03; s1-nb4-cp40 3.07e-03; s1-nw8-16-steps 3.03e-03;
      s1-cout180 2.92e-03; s1-up-nb2 2.66e-03; s1-up-nb4-odd-half 2.62e-03; s1-up-nw8 2.51e-03; narrow-7x7-64-cout3 2.13e-03;
      narrow-7x7-32-cout5 1.90e-03; narrow-5x5-64-cout8 2.05e-03; narrow-5x5-32-cout7 2.06e-03; narrow-3x3-64-valid 2.08e-03;
      narrow-3x3-32-pad01 2.11e-03; narrow-5x5-32-second-tile 2.99e-03"""
    data = R.normal_case(torch.Generator().manual_seed(4321), case)
    data["ws"] = [w.to(BF).float() for w in data["ws"]]
    if case["up"] is not None:
        _, P, want = S.up_case(case, data)
        got, _, _ = _run_forward(case, data, P)
    else:
        want = R.ref_of(case, data)
        got, _, _ = _run_forward(case, data)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print("NORMAL %s [%s]: relative error %.2e (bound %.1e)" % (case["id"], case["part"], err, EPS))
    assert err <= EPS, "%s: relative error %.2e" % (case["id"], err)


# ---- training rows -----------------------------------------------------------------------------------------------------------------

def _run_train(case, data):
    """The row's graph as a training plan: forward, then two backward passes that must repeat their bits.  Everything is pinned before
    the first launch.  Returns what the plan stored: y and gz per layer, gx per input slice with a data gradient, dW and db per layer."""
    from egne_amd import _lib
    from egne_amd.engine import ConvLayer, Piece, Plan
    B = case["B"]
    exact = data["exact"]
    pl = Plan(torch.device(DEV), train=True, dtype=BF)
    L = _lib.lib()
    pieces = _slices(pl, data["xs"], B, case["H"], case["W"])
    tensors = {"x%d" % i: (p, case["H"], case["W"]) for i, p in enumerate(pieces)}
    layers, outs, params = S.layers_of(case), {}, {}
    for ly in layers:
        name = ly["name"]
        _, H, W = tensors[ly["src"][0]]
        ins = []
        for i, s in enumerate(ly["src"]):
            p = tensors[s][0]
            p = Piece(p.buf, p.off, p.C, p.Cp)
            if i in ly["norm"]:
                sc, sh = data["affine"][(name, i)]
                p = _affine(pl, p, sc, sh, R.ACT_RELU if exact else R.ACT_LEAKY, B)
            p.nograd = i in ly["nograd"]
            ins.append(p)
        w, b = torch.nn.Parameter(data["w"][name].to(DEV)), torch.nn.Parameter(data["b"][name].to(DEV))
        w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
        act = (R.ACT_RELU if exact else R.ACT_LEAKY) if ly["act"] else R.ACT_NONE
        layer = ConvLayer([w], [b], [(p.C, p.Cp) for p in ins], stride=ly["stride"], pad=ly["pad"], act=act, pad_mode=ly["pad_mode"])
        Ho, Wo = layer.out_hw(H, W)
        Cs = S.pad8(ly["Cout"])
        out = pl.buf(B, Ho, Wo, Cs + 16)
        out.fill_(POISON)
        dst = Piece(out, 8, ly["Cout"])
        pl.conv(layer, ins, dst, B, H, W, name=name)
        tensors[name] = (dst, Ho, Wo)
        outs[name], params[name] = out, (w, b)
        hits = _launches(pl, name)
        assert [h[0] for h in hits] == [case["fwd"]], "%s: layer %s planned as %s" % (case["id"], name, [h[0] for h in hits])
        assert hits[0][1] is getattr(pl.L, ENTRY[case["fwd"]])
    bw = pl.build_backward()
    # ---- the backward plan: weight gradients (entry, descriptor, split count), data gradients (kind, entry, instantiation)
    names = [c[2] for c in bw.calls]
    for ly in layers:
        hits = _launches(bw, ly["name"] + ".wgrad")
        assert len(hits) == 1 and hits[0][0] == "conv_bf16:wgrad" and hits[0][1] is bw.L.egne_conv2d_wgrad, (case["id"], names)
        d = hits[0][2][0]._obj
        cps = [S.pad8(S.chans_of(case, s)) for s in ly["src"]]
        assert (d.dtype, d.B, d.CoutP, d.Ktot, d.Cout_store) == (1, B, S.pad32(ly["Cout"]), sum(cps), S.pad8(ly["Cout"]))
        assert [d.seg[i].Cp for i in range(d.nseg)] == cps and [bool(d.seg[i].scale) for i in range(d.nseg)] == [i in ly["norm"] for i in range(len(cps))]
        assert (d.H, d.W) == tensors[ly["src"][0]][1:] and d.out_pix_stride == S.pad8(ly["Cout"]) + 16 and d.out_ch_off == 8
        form = S.wgrad_form(case, ly)
        assert int(L.egne_conv2d_wgrad_splits(C.byref(d))) == form[-1], (case["id"], ly["name"], form)
    assert S.wgrad_form(case) == case["inst"] or case["part"] in ("dgrad3", "dgrad1")
    dg = {c[2]: (m[0], c[0], c[1]) for m, c in zip(bw.meta, bw.calls) if ".dgrad" in c[2] and m[0].startswith("conv")}
    assert {n: k for n, (k, _, _) in dg.items()} == case["bw"], (case["id"], {n: k for n, (k, _, _) in dg.items()})
    forms3 = dict(S.dgrad3_forms(case))
    forms1 = {n: (f, acc) for n, f, acc in S.dgrad1_forms(case)}
    for n, (kind, fn, args) in dg.items():
        if n.endswith(".dgrad_multi"):
            assert fn is bw.L.egne_conv1x1_bf16_multi_fwd
            assert int(L.egne_conv1x1_bf16_multi_supported(args[0], args[1], args[2])) == 1
            dm = args[0]._obj          # the k-steps of gz decide <NKS>; every raw slice of the layer is a destination
            steps = S.s1_steps([dm.seg[0].Cp])
            form = S.plan_multi_form(case)
            assert (dm.nseg, steps, args[1]) == (1, form[2], form[3]) and form[1] == {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}[steps], (case["id"], steps, form)
            continue
        assert fn is getattr(bw.L, ENTRY[kind]), (case["id"], n)
        d = args[0]._obj
        if kind == S.B3:
            rm = 2 if d.mask_y else (1 if d.residual else 0)
            assert S._b3(d.seg[0].Cp, d.CoutP, rm) == forms3[n], (case["id"], n, S._b3(d.seg[0].Cp, d.CoutP, rm), forms3[n])
            assert bool(d.mask_sums) == (rm == 2)
        elif kind == S.S1 and n in forms1:
            got1 = S._s1([d.seg[i].Cp for i in range(d.nseg)], d.CoutP, False)
            assert (got1, bool(d.residual)) == forms1[n] and (d.Ho, d.Wo) == (d.H, d.W), (case["id"], n, got1, forms1[n])
    if case["part"] == "dgrad3":
        assert tuple(forms3[n] for n, _ in S.dgrad3_forms(case)) == case["inst"]
    if case["part"] == "dgrad1":
        assert tuple(f for _, f, _ in S.dgrad1_forms(case)) == case["inst"] and set(forms1) == set(dg)
    if case["part"] == "dgrad3" and case["layers"] is not None:          # the chains: a's mask and bias sums come out of b's data gradient, no masking pass for a
        assert "a.act_bwd" not in names and "a.bias_sums" in names, names
    final = [ly["name"] for ly in layers if ly["name"] in data["gy"]]
    pl.run()
    torch.cuda.synchronize()
    y1 = {n: outs[n].clone() for n in outs}
    pl.run()
    torch.cuda.synchronize()
    assert all(torch.equal(outs[n], y1[n]) for n in outs), "%s: a second forward run gives other bits" % case["id"]

    def backward_pass():
        for w, b in params.values():
            w.grad.zero_()
            b.grad.zero_()
        pl.zero_grads()
        twins = [pl.gbuf(pieces[0].buf)] + [pl.gbuf(outs[n]) for n in outs]
        for t in twins:
            t[..., :8] = POISON
            t[..., -8:] = POISON
        for n in final:
            g = pl.gbuf(outs[n])
            g[..., 8:-8] = 0
            g[..., 8:8 + data["gy"][n].shape[1]] = data["gy"][n].permute(0, 2, 3, 1).to(DEV).to(BF)
        bw.run()
        torch.cuda.synchronize()
        return [t.clone() for t in twins] + [p.grad.clone() for wb in params.values() for p in wb]
    first = backward_pass()
    second = backward_pass()
    assert all(torch.equal(a, b_) for a, b_ in zip(first, second)), "%s: a second backward pass over the same plan gives other bits" % case["id"]
    res = dict(y={}, gz={}, gx={}, dW={}, db={})
    for ly in layers:
        n = ly["name"]
        res["y"][n] = _stored(outs[n], 8, ly["Cout"], S.pad8(ly["Cout"]), "%s: output of %s" % (case["id"], n))
        res["gz"][n] = _stored(pl.gbuf(outs[n]), 8, ly["Cout"], S.pad8(ly["Cout"]), "%s: output gradient of %s" % (case["id"], n))
        res["dW"][n], res["db"][n] = params[n][0].grad.double().cpu(), params[n][1].grad.double().cpu()
    gin = pl.gbuf(pieces[0].buf).float().cpu()
    assert (gin[..., :8] == POISON).all() and (gin[..., -8:] == POISON).all(), "%s: a data gradient wrote outside its slices" % case["id"]
    with_grad = {s for ly in layers for i, s in enumerate(ly["src"]) if i not in ly["nograd"]}
    for i, p in enumerate(pieces):
        if "x%d" % i in with_grad:
            assert (gin[..., p.off + p.C:p.off + p.Cp] == 0).all(), "%s: padding channels of the gradient of slice %d must be zeros" % (case["id"], i)
            res["gx"]["x%d" % i] = gin[..., p.off:p.off + p.C].permute(0, 3, 1, 2).contiguous().double()
    return res


@pytest.mark.parametrize("case", S.TRAIN_ROWS, ids=_ids(S.TRAIN_ROWS))
def test_training_integer_data_is_bit_equal(gpu, case):
    """(a) training rows: stored outputs, masked output gradients, data gradients (bf16), weight and bias gradients (fp32) torch.equal
    with float64; the bias gradient out of a data gradient's mask sums included (chain rows)."""
    data, ref = S.train_case(case)
    got = _run_train(case, data)
    diff = {k: {n: int((got[k][n] != ref[k][n]).sum()) for n in got[k]} for k in ("y", "gz", "gx", "dW", "db")}
    print("%s %s: weight density %.4f, max |dW| %d; elements that differ: %s" % (case["id"], case["inst"], data["density"],
                                                                               max(t.abs().max().item() for t in ref["dW"].values()), diff))
    for k in ("y", "gz", "gx", "dW", "db"):
        for n in got[k]:
            _report(case, got[k][n], ref[k][n], "%s of %s" % (k, n))


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("case", S.TRAIN_ROWS, ids=_ids(S.TRAIN_ROWS))
def test_training_normal_data_within_the_project_bounds(gpu, case):
    """(b) training rows on normal data.  The reference follows what the plan stored (bf16_refs.train_ref: masks from the stored outputs,
    weight and data gradients from the stored, rounded gz), as test_weight_and_data_gradients_bf16_storage does.  Relative error on MI355X,
    per row (y: stored output, dW / db: weight / bias gradient, gx: data gradient; .name: the layer or input slice):
      w3-pair-32-32: y.c 1.86e-03; dW.c 1.35e-07; db.c 3.71e-08; gz.c 2.17e-05; gx.x0 2.23e-03
      w3-pair-cout64-k32: y.c 3.26e-03; dW.c 8.89e-08; db.c 3.67e-08; gz.c 2.30e-05; gx.x0 2.48e-03
      w3-pair-three-input-blocks: y.c 2.02e-03; dW.c 1.41e-07; db.c 3.28e-08; gz.c 2.66e-05; gx.x0 1.97e-03
      w3-pair-affine-cp40: y.c 2.97e-03; dW.c 1.48e-07; db.c 3.77e-08; gz.c 2.33e-05
      w3-pair-w16: y.c 3.34e-03; dW.c 9.88e-08; db.c 3.01e-08; gz.c 2.57e-05; gx.x0 2.07e-03
      w3-pair-w17: y.c 1.46e-03; dW.c 1.02e-07; db.c 0.00e+00; gz.c 0.00e+00; gx.x0 2.62e-03
      w3-pair-two-tiles: y.c 2.92e-03; dW.c 1.36e-07; db.c 3.35e-08; gz.c 1.96e-05; gx.x0 3.31e-03
      w3-quad-64-64: y.c 1.82e-03; dW.c 1.58e-07; db.c 4.29e-08; gz.c 2.37e-05; gx.x0 1.96e-03
      w3-quad-96-96: y.c 2.01e-03; dW.c 1.22e-07; db.c 2.59e-08; gz.c 2.45e-05; gx.x0 2.20e-03
      w3-quad-128-100: y.c 3.59e-03; dW.c 1.17e-07; db.c 3.80e-08; gz.c 2.19e-05; gx.x0 2.41e-03
      w3-quad-38-64: y.c 2.86e-03; dW.c 1.43e-07; db.c 4.01e-08; gz.c 2.17e-05; gx.x0 2.62e-03
      w3-quad-two-tiles: y.c 2.94e-03; dW.c 1.41e-07; db.c 2.91e-08; gz.c 1.96e-05; gx.x0 3.40e-03
      d3-chain-cmid32: y.a 1.86e-03; dW.a 1.15e-07; db.a 3.69e-08; gz.a 2.11e-03; y.b 2.42e-03; dW.b 1.09e-07; db.b 4.08e-08; gz.b 2.39e-05; y.c 3.13e-03; dW.c 1.46e-07; db.c 4.01e-08; gz.c 2.36e-05; gx.x0 3.16e-03
      d3-chain-cmid64: y.a 2.42e-03; dW.a 1.36e-07; db.a 4.28e-08; gz.a 3.05e-03; y.b 2.30e-03; dW.b 1.28e-07; db.b 4.14e-08; gz.b 2.64e-05; y.c 3.27e-03; dW.c 1.27e-07; db.c 1.56e-08; gz.c 2.34e-05; gx.x0 3.10e-03
      d3-chain-cmid40: y.a 2.32e-03; dW.a 1.06e-07; db.a 3.43e-08; gz.a 2.48e-03; y.b 2.37e-03; dW.b 9.46e-08; db.b 4.36e-08; gz.b 2.55e-05; y.c 2.17e-03; dW.c 9.56e-08; db.c 2.65e-08; gz.c 2.33e-05; gx.x0 2.95e-03
      d3-chain-b64-cmid96: y.a 2.67e-03; dW.a 1.09e-07; db.a 2.96e-08; gz.a 2.59e-03; y.b 2.68e-03; dW.b 1.07e-07; db.b 2.68e-08; gz.b 2.34e-05; y.c 1.99e-03; dW.c 1.31e-07; db.c 3.03e-08; gz.c 2.31e-05; gx.x0 3.29e-03
      d3-chain-b96-cmid128: y.a 1.53e-03; dW.a 1.13e-07; db.a 2.69e-08; gz.a 2.57e-03; y.b 2.34e-03; dW.b 1.14e-07; db.b 3.29e-08; gz.b 2.19e-05; y.c 2.86e-03; dW.c 1.35e-07; db.c 1.74e-08; gz.c 2.33e-05; gx.x0 3.57e-03
      d3-chain-b128-cmid160: y.a 2.36e-03; dW.a 1.15e-07; db.a 3.27e-08; gz.a 2.21e-03; y.b 2.29e-03; dW.b 1.24e-07; db.b 3.97e-08; gz.b 2.01e-05; y.c 3.22e-03; dW.c 1.10e-07; db.c 3.30e-08; gz.c 2.47e-05; gx.x0 3.36e-03
      d3-chain-b160-cmid32: y.a 3.19e-03; dW.a 1.45e-07; db.a 5.84e-08; gz.a 2.21e-03; y.b 2.15e-03; dW.b 1.47e-07; db.b 3.30e-08; gz.b 2.31e-05; y.c 2.03e-03; dW.c 1.05e-07; db.c 1.76e-08; gz.c 2.29e-05; gx.x0 3.24e-03
      d3-chain-x64-cmid96: y.a 3.09e-03; dW.a 1.35e-07; db.a 2.51e-08; gz.a 1.72e-03; y.b 3.62e-03; dW.b 1.13e-07; db.b 2.29e-08; gz.b 2.34e-05; y.c 2.13e-03; dW.c 1.08e-07; db.c 3.20e-08; gz.c 2.21e-05; gx.x0 4.41e-03
      d3-chain-x64-cmid32: y.a 1.91e-03; dW.a 1.26e-07; db.a 3.31e-08; gz.a 2.13e-03; y.b 2.68e-03; dW.b 9.89e-08; db.b 4.09e-08; gz.b 2.66e-05; y.c 2.62e-03; dW.c 9.46e-08; db.c 3.30e-08; gz.c 2.64e-05; gx.x0 3.16e-03
      d3-two-slices: y.c 2.49e-03; dW.c 1.28e-07; db.c 3.13e-08; gz.c 2.37e-05; gx.x0 1.97e-03; gx.x1 1.85e-03
      d3-38-100: y.c 3.40e-03; dW.c 1.34e-07; db.c 3.00e-08; gz.c 2.13e-05; gx.x0 2.88e-03
      d1-merged-accumulate: y.a 3.26e-03; dW.a 2.45e-07; db.a 3.71e-08; gz.a 2.16e-05; y.c 3.23e-03; dW.c 2.85e-07; db.c 2.25e-08; gz.c 1.93e-05; gx.x0 4.14e-03; gx.x1 4.36e-03
      w1-1-256: y.c 3.26e-03; dW.c 2.45e-07; db.c 3.71e-08; gz.c 2.16e-05; gx.x0 2.30e-03; gx.x1 2.28e-03
      w1-1-128-cp40: y.c 2.84e-03; dW.c 2.31e-07; db.c 3.62e-08; gz.c 2.16e-05; gx.x0 3.16e-03; gx.x1 2.89e-03; gx.x2 2.62e-03
      w1-2-128: y.c 3.30e-03; dW.c 2.06e-07; db.c 3.47e-08; gz.c 1.94e-05; gx.x0 2.61e-03; gx.x1 2.46e-03; gx.x2 2.48e-03
      w1-2-64: y.c 2.42e-03; dW.c 1.29e-07; db.c 2.08e-08; gz.c 2.17e-05; gx.x0 2.13e-03
      w1-4-64-store88: y.c 3.07e-03; dW.c 1.63e-07; db.c 2.41e-08; gz.c 1.91e-05; gx.x0 2.56e-03; gx.x1 2.37e-03
      w1-8-64-two-launches: y.c 3.05e-03; dW.c 1.24e-07; db.c 2.81e-08; gz.c 1.95e-05; gx.x0 2.92e-03; gx.x1 2.72e-03; gx.x2 3.45e-03
      wg-3x3-w13: y.c 2.02e-03; dW.c 1.06e-07; db.c 2.80e-08; gz.c 2.57e-05
      wg-1x1-small: y.c 3.31e-03; dW.c 1.28e-07; db.c 3.12e-08; gz.c 2.16e-05
      wg-1x1-allpairs-affine: y.c 3.19e-03; dW.c 2.43e-07; db.c 2.50e-08; gz.c 2.06e-05
      wg-4x4-s2-reflect-wide: y.c 2.98e-03; dW.c 1.10e-07; db.c 4.35e-08; gz.c 2.50e-05
      wg-7x7-c3-cout64: y.c 3.08e-03; dW.c 2.26e-07; db.c 2.52e-08; gz.c 2.37e-05
      wg-7x7-c3-cout32: y.c 3.23e-03; dW.c 8.90e-08; db.c 2.87e-08; gz.c 2.64e-05"""
    data = S.train_normal_case(case)
    data["w"] = {n: w.to(BF).float() for n, w in data["w"].items()}
    got = _run_train(case, data)
    ref = S.train_ref(case, data, y_stored=got["y"], gz_stored=got["gz"])
    consumed = {s for ly in S.layers_of(case) for s in ly["src"]}
    figs = {}
    for ly in S.layers_of(case):
        n = ly["name"]
        figs["y." + n] = (_rel(got["y"][n], ref["yc"][n]), EPS)
        figs["dW." + n] = (_rel(got["dW"][n], ref["dW"][n]), {(3, 3): WGRAD3_BOUND, (1, 1): WGRAD1_BOUND}.get(ly["k"], OTHER_K_W_BOUND))
        # bias: sums of the unrounded masked gradient where a masking pass takes them, of the stored one where a data gradient's epilogue does
        want_b = got["gz"][n].sum((0, 2, 3)) if n in consumed else ref["db"][n]
        figs["db." + n] = (_rel(got["db"][n], want_b), BIAS_BOUND)
        figs["gz." + n] = (_rel(got["gz"][n], ref["gzc"][n]), EPS)
    for s, g in got["gx"].items():
        # a store rounds by at most half an ulp, 2^-8 of the stored value: EPS of the largest element of the state it stores.  A slice with
        # two writers is stored twice (first state, then first + second): EPS x (max |first state| + max |final state|)
        states = [t.abs().max().item() for n, t in ref["states"] if n.startswith(s + " after ")]
        figs["gx." + s] = (_rel(g, ref["gx"][s]), EPS * sum(states) / states[-1])
    print("NORMAL %s [%s]: %s" % (case["id"], case["part"], "; ".join("%s %.2e" % (k, v[0]) for k, v in figs.items())))
    for k, (e, bound) in figs.items():
        assert e <= bound, "%s: %s relative error %.2e (bound %.1e)" % (case["id"], k, e, bound)


# ---- the multi-destination 1x1 through its C entry -----------------------------------------------------------------------------------

def _run_multi(case, exact):
    """egne_conv1x1_bf16_multi_fwd on the row's destinations (as test_conv1x1_bf16_multi_destinations drives it): returns per destination
    the stored slice [M][Cp] and the per-wave channel sums, float64 on the CPU."""
    from egne_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    gzv, dsts = S.multi_case(case, exact)
    Cs = case["multi"][0]
    Csp, M = S.pad8(Cs), gzv.shape[0]
    gz = torch.full((M, Csp + 16), POISON, dtype=BF, device=DEV)
    gz[:, 8:8 + Csp] = 0
    gz[:, 8:8 + Cs] = gzv.to(DEV).to(BF)
    dm = _lib.ConvDesc()
    dm.dtype = 1
    dm.B, dm.H, dm.W, dm.Ho, dm.Wo = case["B"], case["H"], case["W"], case["H"], case["W"]
    dm.kh = dm.kw = dm.stride = dm.ngroups = 1
    for g_ in range(_lib.MAXGROUP):
        dm.dil[g_] = 1
    dm.nseg = 1
    dm.seg[0].ptr, dm.seg[0].pix_stride, dm.seg[0].ch_off, dm.seg[0].Cp = gz.data_ptr(), Csp + 16, 8, Csp
    dm.Ktot = Csp
    arr = (_lib.Dst * len(dsts))()
    keep, outs = [], []
    for j, q_ in enumerate(dsts):
        Cd, Cp, CoutP = q_["Cd"], q_["Cp"], S.pad32(q_["Cd"])
        wflat = torch.zeros(CoutP, Csp)
        wflat[:Cd, :Cs] = q_["w"]
        wflat = wflat.to(DEV)
        dp = _lib.ConvDesc()
        dp.nseg, dp.CoutP, dp.Ktot = 1, CoutP, Csp
        dp.seg[0].Cp = Csp
        n = int(L.egne_conv1x1_bf16_pack_elems(C.byref(dp)))
        assert n > 0
        frag = torch.empty(n, dtype=BF, device=DEV)
        info = torch.tensor([0, Csp], dtype=torch.int32, device=DEV)
        _lib.check(L.egne_pack_conv1x1_bf16(C.byref(dp), wflat.data_ptr(), info.data_ptr(), frag.data_ptr(), st), "pack")
        out = torch.full((M, Cp + 16), POISON, dtype=BF, device=DEV)
        q = arr[j]
        q.out, q.out_pix_stride, q.out_ch_off, q.C, q.CoutP, q.wfrag = out.data_ptr(), Cp + 16, 8, Cp, CoutP, frag.data_ptr()
        if q_["r0"] is not None:
            out[:, 8:8 + Cp] = q_["r0"].to(DEV).to(BF)
            q.residual, q.res_pix_stride, q.res_ch_off = out.data_ptr(), Cp + 16, 8
            q.res_pixels = q_["rp"] if q_["rp"] < M else 0
        yb = None
        if q_["ym"] is not None:
            yb = q_["ym"].to(DEV).to(BF).contiguous()
            q.mask_y, q.mask_pix_stride, q.mask_ch_off, q.act = yb.data_ptr(), Cp, 0, (R.ACT_RELU if exact else R.ACT_LEAKY)
        keep += [wflat, frag, info, yb]
        outs.append([out, None])
    for j, q_ in enumerate(dsts):
        if q_["sums"]:
            nrows = int(L.egne_conv1x1_bf16_multi_waves(C.byref(dm), len(dsts), arr))
            assert nrows > 0
            outs[j][1] = torch.full((nrows, q_["Cp"]), float("nan"), device=DEV)
            arr[j].sums = outs[j][1].data_ptr()
    # never launch what the predicate refuses
    assert int(L.egne_conv1x1_bf16_multi_supported(C.byref(dm), len(dsts), arr)) == 1
    assert S.s1_form(case) == case["inst"] and S.s1_steps([Csp]) == case["inst"][2]
    _lib.check(L.egne_conv1x1_bf16_multi_fwd(C.byref(dm), len(dsts), arr, st), "multi")
    torch.cuda.synchronize()
    assert (gz[:, :8] == POISON).all() and (gz[:, 8 + Csp:] == POISON).all()
    res = []
    for (out, sm), q_ in zip(outs, dsts):
        o = out.float().cpu().double()
        assert (o[:, :8] == POISON).all() and (o[:, 8 + q_["Cp"]:] == POISON).all(), "%s: a destination wrote outside its slice" % case["id"]
        res.append((o[:, 8:8 + q_["Cp"]], sm.double().cpu() if sm is not None else None))
    return dsts, res


@pytest.mark.parametrize("case", S.MULTI_ROWS, ids=_ids(S.MULTI_ROWS))
def test_multi_destination_integer_data_is_bit_equal(gpu, case):
    """(a) every destination torch.equal with float64 (padding channels zero), the per-wave channel sums added up the exact integer sum
    of what was stored."""
    dsts, res = _run_multi(case, True)
    for j, (q_, (o, sm)) in enumerate(zip(dsts, res)):
        print("%s %s destination %d: weight density %.3f, max |value| %d, %d of %d elements differ"
              % (case["id"], case["inst"], j, q_["density"], q_["want"].abs().max().item(), int((o != q_["want"]).sum()), o.numel()))
        _report(case, o, q_["want"], "destination %d" % j)
        if sm is not None:
            assert torch.isfinite(sm).all()
            _report(case, sm.sum(0), q_["want"].sum(0), "the channel sums of destination %d" % j)


@pytest.mark.parametrize("case", S.MULTI_ROWS, ids=_ids(S.MULTI_ROWS))
def test_multi_destination_normal_data_within_the_project_bound(gpu, case):
    """(b) EPS of the largest element per destination; channel sums as test_conv1x1_bf16_multi_destinations holds them (1e-5 of the
    largest sum of magnitudes, against the sums of what was stored).  Relative error on MI355X, per row and destination:
      multi-1-step 3.16e-03, 2.60e-03 (sums 1.2e-09); multi-4-steps-last-8 2.36e-03 (sums 1.3e-09), 2.46e-03; multi-5-on-6 3.12e-03, 2.92e-03;
      multi-7-on-8 2.63e-03 (sums 1.8e-09), 1.97e-03; multi-8-steps 1.86e-03, 2.08e-03; multi-res-pixels-mid-group 2.36e-03 (sums 1.2e-09), 2.62e-03"""
    dsts, res = _run_multi(case, False)
    figs = []
    for j, (q_, (o, sm)) in enumerate(zip(dsts, res)):
        e = _rel(o, q_["want"])
        figs.append("%.2e" % e)
        assert e <= EPS, "%s: destination %d relative error %.2e" % (case["id"], j, e)
        if sm is not None:
            es = (sm.sum(0) - o.sum(0)).abs().max().item() / o.abs().sum(0).max().item()
            figs.append("sums %.1e" % es)
            assert torch.isfinite(sm).all() and es <= 1e-5
    print("NORMAL %s [multi]: %s" % (case["id"], "; ".join(figs)))
