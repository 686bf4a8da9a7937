"""-m gpu: ESF-Net's encoder kernels at 60x80 and below -- the 96-wide tile of the split-f16 halo 3x3 (conv_halo_f16.hip) and the
fused Transition_down launch with the next block's InstanceNorm partial sums from its epilogue (conv1x1_f16.hip), each against
float64 (models/RITnet_v2.py:32-44,57-62), plus the shape of the inference plan that uses them.

Bounds: max |diff| / max |truth| < 2e-6 is the bound of tests/test_gpu_ops.py for the three-product split-f16 family (operands
carry 22 bits, fp32 accumulation); the statistics bounds are those of test_conv3x3_role_split (fp64 partial sums of the stored fp32
values, finished in fp64: what is left is the fp32 rounding of scale / shift themselves).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


@pytest.fixture
def _one_kernel_per_test():
    """(kernel-level tests only)  Small shapes address ONE kernel each: the small-problem form of the flat split-f16 kernel stays off, and the halo kernel's
    minimum map width is lifted (the 36x12 map of the transposed walk is narrower than the planner's default of 30)."""
    from egne_amd import engine
    old = engine.SMALL_ENABLED, engine.HALO_F16_MIN_W
    engine.SMALL_ENABLED, engine.HALO_F16_MIN_W = False, 0
    yield
    engine.SMALL_ENABLED, engine.HALO_F16_MIN_W = old


@pytest.fixture(scope="module")
def G():
    from gpu_util import conv_hip  # noqa: F401  (imports torch.cuda)
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.Generator().manual_seed(9600)


def _check_stats(scale, shift, y, C):
    """scale / shift [B][Cp] against the float64 InstanceNorm statistics of the stored output y [B][C][H][W]."""
    rstd = 1.0 / torch.sqrt(y.var((2, 3), unbiased=False) + 1e-5)
    np.testing.assert_allclose(scale.cpu().numpy()[:, :C], rstd.numpy(), rtol=2e-6)
    np.testing.assert_allclose(shift.cpu().numpy()[:, :C], (-y.mean((2, 3)) * rstd).numpy(), rtol=2e-5, atol=2e-6)


@pytest.mark.usefixtures("_one_kernel_per_test")
@pytest.mark.parametrize("mode", ["raw", "norm", "stats"])
@pytest.mark.parametrize("H,W", [(12, 36), (36, 12)])           # 4 against 5 tiles each way: the normal and the transposed walk
@pytest.mark.parametrize("Cin,Cout", [(76, 96), (96, 96)])
def test_halo_96_wide_tile(G, Cin, Cout, H, W, mode):
    """conv3x3_halo_f16_kernel<2, 3, 1, false>: 96 outputs as ONE tile (the 60x80 dense block's 3x3 layers) -- against a float64
    convolution with raw input, with the InstanceNorm affine + LeakyReLU applied while the halo is staged, and with the statistics
    of the stored output from the epilogue; bit for bit against the two 64-wide tiles it replaces (same operands, same order)."""
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd.engine import ConvLayer, Piece, Plan, pad8
    B = 2
    x = _rand(G, B, Cin, H, W) * 2 + 0.5
    w, b = _rand(G, Cout, Cin, 3, 3) / (3 * Cin ** 0.5), _rand(G, Cout)
    xin = x.double()
    if mode == "norm":
        xin = F.leaky_relu(F.instance_norm(x.double()))
    truth = F.leaky_relu(F.conv2d(xin, w.double(), b.double(), padding=1))
    outs = []
    for wide in (96, 128):
        pl = Plan(torch.device(DEV))
        (px,) = to_nhwc_buf(pl, [x], B, H, W)
        layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cin, pad8(Cin))], pad=(1, 1), act=2)
        layer.split = True
        if wide == 128:
            layer.sfrag_coutp = lambda: 128          # the form in front of the 96-wide tile: two 64-wide tiles, 32 padding columns
        if mode == "norm":
            mean, rstd = x.mean((2, 3)), 1 / torch.sqrt(x.var((2, 3), unbiased=False) + 1e-5)
            sc, sh = torch.zeros(B, px.Cp, device=DEV), torch.zeros(B, px.Cp, device=DEV)
            sc[:, :Cin], sh[:, :Cin] = rstd.to(DEV), (-mean * rstd).to(DEV)
            pl.keep += [sc, sh]
            px = px.with_norm(sc, sh, 2)
        out = pl.buf(B, H, W, pad8(Cout) + 8)
        out.fill_(777.0)
        pl.conv(layer, [px], Piece(out, 0, Cout), B, H, W, stats=(mode == "stats"))
        assert [m[0] for m in pl.meta if m[0].startswith("conv")] == ["conv_f16x3:halo"]
        assert int(layer.sfrag_coutp()) == wide
        if mode == "stats":
            assert pl.calls[-1][0] is pl.L.egne_norm_stats_finish           # from the epilogue, not a pass over the output
        for _ in range(2):
            pl.run()
            torch.cuda.synchronize()
            o = out.cpu()
            assert (o[..., pad8(Cout):] == 777.0).all(), "wrote outside the output slice"
            got = o[..., :pad8(Cout)].permute(0, 3, 1, 2).double()
            err = (got[:, :Cout] - truth).abs().max().item() / truth.abs().max().item()
            print("halo %d-wide %s %dx%d %d->%d: rel err %.3e" % (wide, mode, H, W, Cin, Cout, err))
            assert err < 2e-6
            assert (got[:, Cout:] == 0).all()
            if mode == "stats":
                _check_stats(*pl.last_stats, got[:, :Cout], Cout)
        outs.append(out[..., :Cout].clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.usefixtures("_one_kernel_per_test")
def test_64_to_96_keeps_the_role_split_kernel(G):
    """The 96-wide tile is the halo kernel's: a 64 -> 96 layer on a wide map is routed by the 128-row rule as before."""
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd.engine import ConvLayer, Piece, Plan
    B, H, W = 1, 8, 64
    pl = Plan(torch.device(DEV))
    (px,) = to_nhwc_buf(pl, [_rand(G, B, 64, H, W)], B, H, W)
    layer = ConvLayer([torch.nn.Parameter((_rand(G, 96, 64, 3, 3) / 24).to(DEV))], None, [(64, 64)], pad=(1, 1), act=2)
    layer.split = True
    pl.conv(layer, [px], Piece(pl.buf(B, H, W, 96), 0, 96), B, H, W)
    assert [m[0] for m in pl.meta if m[0].startswith("conv")][0] in ("conv_f16x3:rs", "conv_f16x3:rw")
    assert layer.sfrag_coutp() == 128


@pytest.mark.usefixtures("_one_kernel_per_test")
@pytest.mark.parametrize("H,W", [(12, 36), (36, 12)])
def test_halo_96_wide_tile_with_residual(G, H, W):
    """The kernel adds egne_conv_desc.residual behind the activation (the lattice launches of a dilated group accumulate through it;
    the planner itself sends no 96-channel layer with an addend here, so the descriptor of a planned launch is given one): against
    float64 and bit for bit against the two 64-wide tiles; then the same layer object planned 96, 128 and 96 rows wide in turn."""
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd import _lib
    from egne_amd.engine import ConvLayer, Piece, Plan
    B, Cin, Cout = 2, 96, 96
    x, r = _rand(G, B, Cin, H, W) * 2 + 0.5, _rand(G, B, Cout, H, W)
    w, b = _rand(G, Cout, Cin, 3, 3) / (3 * Cin ** 0.5), _rand(G, Cout)
    truth = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)) + r.double()
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cin, Cin)], pad=(1, 1), act=2)
    layer.split = True
    outs = []
    for wide in (96, 128, 96):
        if wide == 128:
            layer.sfrag_coutp = lambda: 128
        else:
            layer.__dict__.pop("sfrag_coutp", None)
        pl = Plan(torch.device(DEV))
        px, pr = to_nhwc_buf(pl, [x, r], B, H, W)
        out = pl.buf(B, H, W, Cout)
        pl.conv(layer, [px], Piece(out, 0, Cout), B, H, W)
        assert [m[0] for m in pl.meta if m[0].startswith("conv")] == ["conv_f16x3:halo"]
        d = [k for k in pl.keep if isinstance(k, _lib.ConvDesc)][-1]
        assert int(d.CoutP) == wide and pl.calls[-1][1][1] == layer._sfrag_packs[wide][0].data_ptr()
        d.residual, d.res_pix_stride, d.res_ch_off = pr.ptr, pr.stride, pr.off
        pl.run()
        torch.cuda.synchronize()
        got = out.cpu().permute(0, 3, 1, 2).double()
        err = (got - truth).abs().max().item() / truth.abs().max().item()
        print("halo %d-wide + residual %dx%d: rel err %.3e" % (wide, H, W, err))
        assert err < 2e-6
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


_TD_CASES = [((32, 32), 38, 3, 24, 40), ((64, 38), 76, 2, 30, 50), ((32, 24), 30, 3, 10, 30)]


def _td_plan(xs, w, b, B, H, W, Cout, stats):
    from gpu_util import DEV, to_nhwc_buf
    from egne_amd.engine import ConvLayer, Piece, Plan, pad8
    pl = Plan(torch.device(DEV))
    pieces = to_nhwc_buf(pl, xs, B, H, W)
    normed = []
    for x, pc in zip(xs, pieces):
        mean, rstd = x.mean((2, 3)), 1 / torch.sqrt(x.var((2, 3), unbiased=False) + 1e-5)
        sc, sh = torch.zeros(B, pc.Cp, device=DEV), torch.zeros(B, pc.Cp, device=DEV)
        sc[:, :pc.C], sh[:, :pc.C] = rstd.to(DEV), (-mean * rstd).to(DEV)
        pl.keep += [sc, sh]
        normed.append(pc.with_norm(sc, sh, 2))
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(p.C, p.Cp) for p in pieces])
    layer.split1 = True
    out = pl.buf(B, H // 2, W // 2, pad8(Cout))
    dst = Piece(out, 0, Cout)
    assert pl.td_pool_fusable(layer, normed, dst)
    pl.conv1x1_pooled(layer, normed, dst, B, H, W, stats=stats)
    return pl, out


@pytest.mark.usefixtures("_one_kernel_per_test")
@pytest.mark.parametrize("stats", [False, True, "runs"])
@pytest.mark.parametrize("chans,Cout,B,H,W", _TD_CASES)
def test_transition_down_with_statistics(G, chans, Cout, B, H, W, stats):
    """models/RITnet_v2.py:32-44 as ONE launch (2x2 average folded in front of the 1x1), without and with the InstanceNorm partial
    sums of the stored output from its epilogue -- output and statistics against float64, and a second run bit for bit equal to
    the first.  The shapes cover blocks spanning two frames (no statistics), partial last blocks of a frame (statistics), an
    8-channel slice tail and one, two and three 32-channel output blocks.  "runs": chunks of several blocks per wave (the
    flagship's split), forced here by a small engine.TDPOOL_STATS_UNITS."""
    from egne_amd import engine
    xs = [_rand(G, B, c, H, W) * 2 + 0.3 for c in chans]
    w, b = _rand(G, Cout, sum(chans), 1, 1) / sum(chans) ** 0.5, _rand(G, Cout)
    xin = torch.cat([F.leaky_relu(F.instance_norm(x.double())) for x in xs], 1)
    truth = F.avg_pool2d(F.conv2d(xin, w.double(), b.double()), 2)
    old = engine.TDPOOL_STATS_UNITS
    if stats == "runs":
        engine.TDPOOL_STATS_UNITS = max(1, B * ((H // 2) * (W // 2) + 31) // 32 // 3)       # three blocks per chunk
    try:
        pl, out = _td_plan(xs, w, b, B, H, W, Cout, bool(stats))
    finally:
        engine.TDPOOL_STATS_UNITS = old
    if stats:
        assert pl.calls[-1][0] is pl.L.egne_norm_stats_finish and pl.calls[-1][2].endswith(".stats")
        nchunk = int(pl.calls[-1][1][3])
        assert (nchunk < ((H // 2) * (W // 2) + 31) // 32) == (stats == "runs")
    else:
        assert len(pl.calls) == 1
    first = None
    for _ in range(2):
        pl.run()
        torch.cuda.synchronize()
        got = out.cpu().permute(0, 3, 1, 2).double()
        err = (got[:, :Cout] - truth).abs().max().item() / truth.abs().max().item()
        print("TD %s -> %d, %dx%dx%d, stats %s: rel err %.3e" % (chans, Cout, B, H, W, stats, err))
        assert err < 2e-6
        assert (got[:, Cout:] == 0).all()
        now = [out.clone()]
        if stats:
            _check_stats(*pl.last_stats, got[:, :Cout], Cout)
            now += [t.clone() for t in pl.last_stats]
        if first is None:
            first = now
        else:
            assert all(torch.equal(a, c) for a, c in zip(first, now))


def test_encoder_plan_takes_statistics_from_the_transition_down():
    """The inference plan of ESF-Net (240x320: the regression head ties the network to it; two frames): the input statistics of
    dense blocks 1 and 2 come from the fused Transition_down launches of blocks 0 and 1, block 3 keeps its pass over memory."""
    from common import batch_args, esf_module
    from gpu_util import DEV
    from egne_amd import synth
    b = synth.make_batch(2, seed=5)
    edge = torch.rand(2, 1, 240, 320, device=DEV)
    m = esf_module("baseline_edge", seed=3).to(DEV).eval()
    with torch.no_grad():
        m(*[a.to(DEV) if torch.is_tensor(a) else a for a in batch_args(b, edge)])
    torch.cuda.synchronize()
    pl = m._last_plan
    calls = list(pl.calls)
    names = [c[2] for c in calls]
    assert "enc.b1.in_x" not in names and "enc.b2.in_x" not in names
    for i in (0, 1):
        k = names.index("enc.b%d.TD" % i)
        assert calls[k][0] is pl.L.egne_conv1x1_pool2_f16x3_fwd
        assert names[k + 1] == "enc.b%d.TD.stats" % i and calls[k + 1][0] is pl.L.egne_norm_stats_finish
    k = names.index("enc.b3.in_x")
    assert calls[k][0] is pl.L.egne_norm_stats
