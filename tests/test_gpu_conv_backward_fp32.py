"""-m gpu: backward of ONE convolution of an fp32-storage training plan, off the 3x3 / 1x1 fast paths, against float64 autograd.

What runs here (engine.Plan._bw_conv): the tile-per-workgroup weight gradient conv_wgrad_kernel<float, false> with its reducer
wgrad_reduce_k (backward.hip), the generic data gradients -- DgradLayer on pack_weight_dgrad_k's flipped pack, TransposedLayer with
egne_reflect_pad_bwd for the reflect-padded and stride-2 layers -- and the store-or-accumulate bookkeeping of the gradient twins
(first_touch / mark_stored / _zero_free).  The geometries are the ones the trained models use and that only whole-network
fixtures reached for fp32 storage: the StyleEncoder's reflect-padded 7x7 and 4x4 / stride 2 (RITnet_v2.py:91-107), DeepVOG's
2x2 / stride 2 (models/deepvog_pytorch.py:22), the regression module's 2x3 "valid" convolution over two 153-channel slices and its
Linear(480, 256) as a 3x5 "valid" convolution (utils.py:991-1020), a zero-padded 3x3 over two concatenated slices, a 3x3 on a map
narrower than 16 and a dilated 3x3.

Truth is F.conv2d in float64 on the same fp32 values, through .backward; the activation mask is taken from the STORED fp32 output,
so a pre-activation within rounding of zero is no failure.  Every gradient is measured relative to the largest element of the true
gradient.

Bounds: fp32 MFMA accumulation (weight / bias gradients, and data gradients / outputs of the exact-fp32 kinds conv_igemm and
conv3x3_halo) 2e-5, as test_conv3x3_backward_halo_wgrad holds it; launches of a conv_f16x3:* kind 3e-6, as
test_split_data_gradient_layer holds that arithmetic.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FP32_BOUND = 2e-5        # test_conv3x3_backward_halo_wgrad
F16X3_BOUND = 3e-6       # test_split_data_gradient_layer
EXACT_KINDS = ("conv_igemm", "conv3x3_halo")
SLOPE = {0: 1.0, 1: 0.0, 2: 0.01}      # d act / d z on the non-positive side: none, ReLU, LeakyReLU


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


@pytest.fixture(scope="module")
def G():
    from gpu_util import conv_hip  # noqa: F401  (imports torch.cuda)
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.Generator().manual_seed(4711)


def _act(z, act):
    return F.relu(z) if act == 1 else (F.leaky_relu(z, 0.01) if act == 2 else z)


def _mask(ystored, act):
    """d act / d z, the branch of every pixel taken from the STORED output (float64)."""
    one = torch.ones_like(ystored)
    return torch.where(ystored > 0, one, one * SLOPE[act])


def _bound(kinds, what):
    """Bound of a result by the kinds of the convolution launches that produced it: all exact fp32, or all split-f16 (a result that
    sums contributions of both kinds takes the fp32 bound, the larger one)."""
    assert kinds, "%s: no convolution launch found" % what
    for k in kinds:
        assert k in EXACT_KINDS or k.startswith("conv_f16x3:"), "%s: launch kind %r has no bound here" % (what, k)
    return FP32_BOUND if any(k in EXACT_KINDS for k in kinds) else F16X3_BOUND


def _rel(got, want):
    return (got.double() - want).abs().max().item() / want.abs().max().item()


def _conv_kinds(plan, part):
    """Kinds of the convolution launches of ``plan`` whose name contains ``part``."""
    return [k for (k, _), (_, _, n) in zip(plan.meta, plan.calls) if part in n and k.startswith("conv")]


def _wgrad_entry(bw, name):
    """(descriptor argument, kind) of the weight-gradient launch of layer ``name`` in the backward plan."""
    hits = [(c[1][0], m[0]) for c, m in zip(bw.calls, bw.meta) if c[2] == name + ".wgrad"]
    assert len(hits) == 1, [c[2] for c in bw.calls]
    return hits[0]


def _nchw(t, off, C):
    return t.cpu()[..., off:off + C].permute(0, 3, 1, 2)


def _run_layer(G, chans, Cout, k, H, W, B=2, stride=1, pad=(0, 0), dil=1, act=0, pad_mode=0, flat_weight=False, norm0=False, split=True):
    """One ConvLayer of an fp32 training plan, forward + two backward passes; returns the measurements.  ``split`` = False: the plan
    keeps its 3x3 gradients off the split-f16 kernels, as EGNE_TRAIN_SPLIT=0 does (Plan.dyn_scales)."""
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd import _lib
    from egne_amd.engine import ConvLayer, Piece, Plan, pad8
    kh, kw = k
    Cin = sum(chans)
    xs = [_rand(G, B, c, H, W) for c in chans]
    w = _rand(G, Cout, Cin, kh, kw) / (Cin * kh * kw) ** 0.5
    b = _rand(G, Cout)
    pl = Plan(torch.device(DEV), train=True)
    if not split:
        pl.dyn_scales = False
    raw = to_nhwc_buf(pl, xs, B, H, W)
    pieces = list(raw)
    sc = sh = None
    if norm0:
        # per-sample affine + LeakyReLU on load of slice 0, shifts of order 1: a zero-padded pixel must contribute 0, not leaky(shift)
        sc, sh = 0.5 + _rand(G, B, chans[0]).abs(), 1.0 + _rand(G, B, chans[0])
        scp, shp = torch.zeros(B, raw[0].Cp, device=DEV), torch.zeros(B, raw[0].Cp, device=DEV)
        scp[:, :chans[0]], shp[:, :chans[0]] = sc.to(DEV), sh.to(DEV)
        pl.keep += [scp, shp]
        pieces[0] = raw[0].with_norm(scp, shp, 2)
        pieces[0].nograd = True      # (the normalisation backward needs its statistics; weight path and the raw slice are under test)
    wd = torch.nn.Parameter((w.reshape(Cout, -1) if flat_weight else w).to(DEV))
    bd = torch.nn.Parameter(b.to(DEV))
    wd.grad, bd.grad = torch.zeros_like(wd), torch.zeros_like(bd)
    layer = ConvLayer([wd], [bd], [(p.C, p.Cp) for p in pieces], stride=stride, pad=pad, dils=(dil,), act=act, pad_mode=pad_mode,
                      kernel_hw=(kh, kw) if flat_weight else None)
    Ho, Wo = layer.out_hw(H, W)
    gy = _rand(G, B, Cout, Ho, Wo)
    gyd = gy.permute(0, 2, 3, 1).to(DEV)
    out = pl.buf(B, Ho, Wo, pad8(Cout))
    pl.conv(layer, pieces, Piece(out, 0, Cout), B, H, W, name="c")
    bw = pl.build_backward()
    pl.run()

    def backward_pass():
        wd.grad.zero_()
        bd.grad.zero_()
        pl.zero_grads()
        pl.gbuf(out)[..., :Cout] = gyd
        bw.run()
        torch.cuda.synchronize()
        return wd.grad.clone(), bd.grad.clone(), pl.gbuf(raw[0].buf).clone()
    first = backward_pass()
    second = backward_pass()

    # float64 truth on the same fp32 values
    xd = [x.double().requires_grad_(True) for x in xs]
    xe = list(xd)
    if norm0:
        xe[0] = F.leaky_relu(xd[0] * sc.double()[:, :, None, None] + sh.double()[:, :, None, None], 0.01)
    xin = torch.cat(xe, 1)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    if pad_mode == 1:
        z = F.conv2d(F.pad(xin, (pad[1], pad[1], pad[0], pad[0]), mode="reflect"), w64, b64, stride=stride, dilation=dil)
    else:
        z = F.conv2d(xin, w64, b64, stride=stride, padding=(pad[0] * dil, pad[1] * dil), dilation=dil)
    assert tuple(z.shape[2:]) == (Ho, Wo)
    ystored = _nchw(out, 0, Cout).double()
    e_fwd = _rel(ystored, _act(z.detach(), act))
    z.backward(gy.double() * _mask(ystored, act))
    gw, gb, gtwin = first
    ew = _rel(gw.cpu().reshape(w.shape), w64.grad)
    eb = _rel(gb.cpu(), b64.grad)
    exs = [_rel(_nchw(gtwin, p.off, p.C), x.grad) for q, p, x in zip(pieces, raw, xd) if not q.nograd]
    wdesc, wkind = _wgrad_entry(bw, "c")
    res = dict(ew=ew, eb=eb, ex=max(exs), e_fwd=e_fwd, wkind=wkind, splits=int(_lib.lib().egne_conv2d_wgrad_splits(wdesc)),
               fwd_kinds=_conv_kinds(pl, "c"), dgrad_kinds=_conv_kinds(bw, ".dgrad"),
               same_bits=all(torch.equal(a, b_) for a, b_ in zip(first, second)))
    print("fp32 conv backward %dx%d s%d d%d %s->%d on %dx%d: splits %d, forward %s, backward %s + %s | forward %.2e, weight gradient "
          "%.2e, bias gradient %.2e, data gradient %.2e" % (kh, kw, stride, dil, list(chans), Cout, H, W, res["splits"], res["fwd_kinds"],
                                                          wkind, res["dgrad_kinds"], e_fwd, ew, eb, res["ex"]))
    return res


def _check(res, splits):
    """``splits``: "multi" / "one" pin the case on the multi-split / single-split form of the weight gradient, None only reports."""
    # a later routing change must not quietly move these cases onto the halo / all-pairs weight gradients
    assert res["wkind"] == "conv_wgrad", res["wkind"]
    if splits == "multi":
        assert res["splits"] >= 2, res["splits"]
    elif splits == "one":
        assert res["splits"] == 1, res["splits"]
    assert res["e_fwd"] < _bound(res["fwd_kinds"], "forward"), "forward output: relative error %.2e" % res["e_fwd"]
    assert res["ew"] < FP32_BOUND, "weight gradient: relative error %.2e" % res["ew"]
    assert res["eb"] < FP32_BOUND, "bias gradient: relative error %.2e" % res["eb"]
    assert res["ex"] < _bound(res["dgrad_kinds"], "data gradient"), "data gradient: relative error %.2e (%s)" % (res["ex"], res["dgrad_kinds"])
    # the generic weight gradient needs a zero-filled partial-sum workspace that its reduction clears again (clean = 1 in wgrad_impl)
    assert res["same_bits"], "a second backward pass over the same plan gave other bits"


@pytest.mark.parametrize("H,W,splits", [(23, 37, "multi"),      # M = 1702 output pixels: two pixel splits, ragged last chunk
                                        (9, 11, "one")])        # less than one 128-pixel chunk per frame
def test_reflect_padded_7x7_fp32(G, H, W, splits):
    """(a) StyleEncoder head: ReflectionPad2d(3) + 7x7, 3 -> 64, ReLU; the data gradient w.r.t. the padded input is folded back by
    egne_reflect_pad_bwd.  That gradient is a zero-padded 7x7 with pad 6 on the implicit GEMM: 49 taps, more than the 32-bit word of
    tap bits the kernel kept its zero-padding test in (conv_igemm.hip; relative error 0.8 before the kernel tested the coordinates
    of such layers per step)."""
    _check(_run_layer(G, (3,), 64, (7, 7), H, W, pad=(3, 3), act=1, pad_mode=1), splits)


@pytest.mark.parametrize("H,W", [(9, 11), (23, 37)])
def test_zero_padded_7x7_split_layer_takes_the_implicit_gemm(G, H, W, monkeypatch):
    """A zero-padded 7x7 (pad 3, 32 -> 32) of a frozen net with layer.split = True: 49 taps do not fit the 32-bit tap mask that the
    split-f16 flat / small / big kernels keep per staged row, so the planner and egne_conv2d_auto_kind (compared under
    EGNE_CHECK_DISPATCH) both leave it to conv_igemm, and the split-f16 entry point refuses the descriptor by its tap count.
    Planned as conv_f16x3:flat / :small the output is wrong by a relative error of order 1 (tap 32 + k aliases tap k)."""
    import ctypes as C
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd import _lib, engine
    from egne_amd.engine import ConvLayer, Piece, Plan
    monkeypatch.setattr(engine, "CHECK_DISPATCH", True)
    B, Cn = 2, 32
    x = _rand(G, B, Cn, H, W)
    w, b = _rand(G, Cn, Cn, 7, 7) / (Cn * 49) ** 0.5, _rand(G, Cn)
    truth = F.conv2d(x.double(), w.double(), b.double(), padding=3)
    pl = Plan(torch.device(DEV))
    (px,) = to_nhwc_buf(pl, [x], B, H, W)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cn, Cn)], pad=(3, 3))
    layer.split = True
    out = pl.buf(B, H, W, Cn + 8)
    out.fill_(777.0)
    pl.conv(layer, [px], Piece(out, 8, Cn), B, H, W, name="c7")        # (raises when the two dispatchers disagree)
    assert _conv_kinds(pl, "c7") == ["conv_igemm"], _conv_kinds(pl, "c7")
    assert engine.DISPATCH_LOG[-1] == ("c7", "conv_igemm", "conv_igemm"), engine.DISPATCH_LOG[-1]
    pl.run()
    torch.cuda.synchronize()
    assert (out[..., :8] == 777.0).all(), "conv wrote outside its output slice"
    e = _rel(_nchw(out, 8, Cn), truth)
    print("zero-padded 7x7 with layer.split on %dx%d: %s, relative error %.2e" % (H, W, _conv_kinds(pl, "c7"), e))
    assert e < _bound(_conv_kinds(pl, "c7"), "forward"), "forward output: relative error %.2e" % e
    # the split-f16 entry point on the same descriptor: an error that names the tap count, nothing launched
    L = _lib.lib()
    d = pl.calls[-1][1][0]._obj
    assert (d.kh, d.kw) == (7, 7)
    wdummy = torch.zeros(64, device=DEV)
    before = out.clone()
    rc = L.egne_conv2d_f16x3_fwd(C.byref(d), wdummy.data_ptr(), wdummy.data_ptr(), 1.0, 1.0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"49 taps" in L.egne_last_error(), (rc, L.egne_last_error())
    assert torch.equal(out, before)


@pytest.mark.parametrize("H,W,splits", [(64, 96, "multi"),      # M = 3072
                                        (24, 32, "one")])
def test_reflect_padded_4x4_stride2_fp32(G, H, W, splits):
    """(b) StyleEncoder down-sampling block: ReflectionPad2d(1) + 4x4 / stride 2, 64 -> 128, ReLU; phase-packed data gradient."""
    _check(_run_layer(G, (64,), 128, (4, 4), H, W, stride=2, pad=(1, 1), act=1, pad_mode=1), splits)


def test_stride2_dgrad_refuses_odd_sizes(G):
    """(b) the phase-packed stride-2 data gradient needs even padded sizes: 25x32 is refused when the backward plan is built."""
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd.engine import ConvLayer, Piece, Plan
    B, H, W = 2, 25, 32
    pl = Plan(torch.device(DEV), train=True)
    (px,) = to_nhwc_buf(pl, [_rand(G, B, 64, H, W)], B, H, W)
    wd, bd = torch.nn.Parameter((_rand(G, 128, 64, 4, 4) / 32).to(DEV)), torch.nn.Parameter(_rand(G, 128).to(DEV))
    wd.grad, bd.grad = torch.zeros_like(wd), torch.zeros_like(bd)
    layer = ConvLayer([wd], [bd], [(64, 64)], stride=2, pad=(1, 1), act=1, pad_mode=1)
    Ho, Wo = layer.out_hw(H, W)
    pl.conv(layer, [px], Piece(pl.buf(B, Ho, Wo, 128), 0, 128), B, H, W, name="c")
    with pytest.raises(NotImplementedError, match="stride-2 dgrad needs even input sizes"):
        pl.build_backward()


def test_2x2_stride2_fp32(G):
    """(c) DeepVOG's down-sampling convolution: 2x2 / stride 2, no padding, 32 -> 64 (a 1x1 per phase, un-shuffled by
    egne_reflect_pad_bwd with P = 0)."""
    _check(_run_layer(G, (32,), 64, (2, 2), 48, 64, stride=2), None)


def test_valid_2x3_over_two_slices_fp32(G):
    """(d) regression module c1: 2x3 "valid" over two 153-channel slices (channel tails 153 -> 160 in both), LeakyReLU; the data
    gradient is a 2x3 convolution with pad (1, 2) on the flipped pack."""
    _check(_run_layer(G, (153, 153), 128, (2, 3), 15, 20, act=2), "one")


def test_linear_as_valid_3x5_fp32(G):
    """(e) Linear(480, 256) as a 3x5 "valid" convolution with one output pixel per sample, weight held as [256, 480]."""
    _check(_run_layer(G, (32,), 256, (3, 5), 3, 5, B=4, flat_weight=True), "one")


@pytest.mark.parametrize("H,W,norm0,split,splits", [(24, 32, False, True, None), (40, 56, False, True, "multi"),      # M = 4480
                                                    (24, 32, True, True, None), (24, 32, False, False, None)])
def test_3x3_over_two_slices_fp32(G, H, W, norm0, split, splits):
    """(f) zero-padded 3x3 over the concatenation of a 64- and a 32-channel slice; ``norm0``: slice 0 carries a per-sample affine +
    LeakyReLU on load -- zero padding applies AFTER the transform.  A training plan takes the data gradients of this layer on the
    split-f16 kernels (SplitDgradLayer, weights flipped by torch); the last case keeps them on DgradLayer's flipped pack."""
    res = _run_layer(G, (64, 32), 32, (3, 3), H, W, pad=(1, 1), norm0=norm0, split=split)
    assert split or all(k in EXACT_KINDS for k in res["dgrad_kinds"]), res["dgrad_kinds"]
    _check(res, splits)


def test_3x3_on_a_map_narrower_than_16_fp32(G):
    """(g) 3x3 "same", one slice, 15x10: too narrow for the halo weight gradient."""
    _check(_run_layer(G, (64,), 64, (3, 3), 15, 10, pad=(1, 1), act=2), "one")


def test_3x3_dilation_2_fp32(G):
    """(h) 3x3 "same" with dilation 2, 38 -> 38 (channel tails), LeakyReLU: _bw_conv takes it like any stride-1 zero-padded layer."""
    _check(_run_layer(G, (38,), 38, (3, 3), 30, 40, pad=(1, 1), dil=2, act=2), None)


# ---- fan-out: one buffer read by several layers ----------------------------------------------------------------------------------

FAN_B, FAN_H, FAN_W = 2, 24, 32
FAN_SPECS = {          # name -> (input slices, Cout, kernel, stride, pad, act)
    "1x1": ("ab", 40, 1, 1, 0, 2),      # over [A | B]: ONE data-gradient launch for both slices (DgradLayer span = 2)
    "3x3": ("a", 32, 3, 1, 1, 0),       # zero-padded, A alone
    "2x2": ("b", 64, 2, 2, 0, 0),       # stride 2, B alone: TransposedLayer phase 2 + egne_reflect_pad_bwd
}


@pytest.fixture(scope="module")
def fan_data(G):
    d = dict(xa=_rand(G, FAN_B, 32, FAN_H, FAN_W), xb=_rand(G, FAN_B, 32, FAN_H, FAN_W))
    for n, (src, Cout, k, s, p, _) in FAN_SPECS.items():
        Cin = 32 * len(src)
        ho, wo = (FAN_H + 2 * p - k) // s + 1, (FAN_W + 2 * p - k) // s + 1
        d[n] = (_rand(G, Cout, Cin, k, k) / (Cin * k * k) ** 0.5, _rand(G, Cout), _rand(G, FAN_B, Cout, ho, wo))
    return d


def _run_fan(data, order):
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd import engine
    from egne_amd.engine import ConvLayer, Piece, Plan, pad8
    B, H, W = FAN_B, FAN_H, FAN_W
    pl = Plan(torch.device(DEV), train=True)
    pa, pb = to_nhwc_buf(pl, [data["xa"], data["xb"]], B, H, W)
    par, outs, gyd = {}, {}, {}
    for n in order:
        src, Cout, k, s, p, act = FAN_SPECS[n]
        w, b, gy = data[n]
        wd, bd = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV))
        wd.grad, bd.grad = torch.zeros_like(wd), torch.zeros_like(bd)
        pieces = [dict(a=pa, b=pb)[c] for c in src]
        layer = ConvLayer([wd], [bd], [(q.C, q.Cp) for q in pieces], stride=s, pad=(p, p), act=act)
        outs[n] = pl.buf(B, gy.shape[2], gy.shape[3], pad8(Cout))
        pl.conv(layer, pieces, Piece(outs[n], 0, Cout), B, H, W, name=n)
        par[n], gyd[n] = (wd, bd), gy.permute(0, 2, 3, 1).to(DEV)
    bw = pl.build_backward()
    pl.run()

    def backward_pass():
        for wd, bd in par.values():
            wd.grad.zero_()
            bd.grad.zero_()
        pl.zero_grads()
        for n in order:
            pl.gbuf(outs[n])[..., :FAN_SPECS[n][1]] = gyd[n]
        bw.run()
        torch.cuda.synchronize()
        return [pl.gbuf(pa.buf).clone()] + [t.grad.clone() for n in sorted(par) for t in par[n]]
    first = backward_pass()
    # poisoned run: whatever the twins held must not reach a gradient (a buffer in _zero_free that some launch still accumulates
    # into, or a first writer marked as storing that leaves channels / samples of its slice unwritten, would let it through)
    for t in pl.gtwins.values():
        t.fill_(1e30)
    second = backward_pass()
    # float64 truth: each slice's gradient is the sum of its two readers' contributions
    xa, xb = data["xa"].double().requires_grad_(True), data["xb"].double().requires_grad_(True)
    for n in order:
        src, Cout, k, s, p, act = FAN_SPECS[n]
        w, b, gy = data[n]
        z = F.conv2d(torch.cat([dict(a=xa, b=xb)[c] for c in src], 1), w.double(), b.double(), stride=s, padding=p)
        ystored = _nchw(outs[n], 0, Cout).double()
        (z * gy.double() * _mask(ystored, act)).sum().backward()
    ga, gb = _nchw(first[0], pa.off, 32).double(), _nchw(first[0], pb.off, 32).double()
    kinds = {n: _conv_kinds(bw, n + ".dgrad") for n in order}
    zero_free = id(pa.buf) in pl._zero_free
    print("fan-out %s: data-gradient kinds %s, input twin zero-free %s | gradient of A %.2e, of B %.2e"
          % (order, kinds, zero_free, _rel(ga, xa.grad), _rel(gb, xb.grad)))
    return dict(ga=ga, gb=gb, ta=xa.grad, tb=xb.grad, kinds=kinds, zero_free=zero_free, knobs=engine.ZERO_SKIP and engine.FIRST_WRITER,
                same_bits=all(torch.equal(a, b_) for a, b_ in zip(first, second)))


@pytest.fixture(scope="module")
def fan(fan_data):
    memo = {}

    def get(order):
        if order not in memo:
            memo[order] = _run_fan(fan_data, order)
        return memo[order]
    return get


FAN_ORDERS = [("1x1", "3x3", "2x2"),      # backward: 2x2 accumulates into B, 3x3 is the first writer of A (stores), 1x1 accumulates
              ("2x2", "3x3", "1x1")]      # backward: 1x1 is the first writer of A AND B (stores both), the others accumulate


@pytest.mark.parametrize("order", FAN_ORDERS, ids=["1x1-first-on-tape", "1x1-last-on-tape"])
def test_fan_out_gradients_sum_over_the_readers(fan, order):
    """Slices A and B of one buffer feed a 1x1 over [A | B], a 3x3 over A and a 2x2 / stride 2 over B: each slice's gradient is the
    float64 sum of its two contributions, whichever reader the tape makes the first writer; a second pass over twins filled with
    1e30 (zero_grads skips the buffers in _zero_free) gives the same bits."""
    r = fan(order)
    ba = _bound(r["kinds"]["1x1"] + r["kinds"]["3x3"], "gradient of A")
    bb = _bound(r["kinds"]["1x1"] + r["kinds"]["2x2"], "gradient of B")
    ea, eb = _rel(r["ga"], r["ta"]), _rel(r["gb"], r["tb"])
    assert ea < ba and eb < bb, "gradient of A %.2e (bound %.0e), of B %.2e (bound %.0e)" % (ea, ba, eb, bb)
    if r["knobs"]:
        # every access of the input twin is covered by the first writer's full-batch store only when the 1x1 over both slices comes
        # first in the backward pass; with the 2x2 first, B's slice is accumulated into before anything stored it
        assert r["zero_free"] == (order[-1] == "1x1")
    assert r["same_bits"], "poisoned gradient twins reached a gradient"


def test_fan_out_first_writer_does_not_matter(fan):
    """The two tape orders make different launches the first writer of each slice; their gradients agree to the same bound."""
    r0, r1 = fan(FAN_ORDERS[0]), fan(FAN_ORDERS[1])
    ba = _bound(r0["kinds"]["1x1"] + r0["kinds"]["3x3"] + r1["kinds"]["1x1"] + r1["kinds"]["3x3"], "gradient of A")
    bb = _bound(r0["kinds"]["1x1"] + r0["kinds"]["2x2"] + r1["kinds"]["1x1"] + r1["kinds"]["2x2"], "gradient of B")
    ea, eb = _rel(r1["ga"], r0["ga"]), _rel(r1["gb"], r0["gb"])
    print("fan-out, one tape order against the other: gradient of A %.2e, of B %.2e" % (ea, eb))
    assert ea < ba and eb < bb, (ea, eb)
