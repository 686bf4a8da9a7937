"""Channel-order split-pair storage (egne_conv_desc.out_split = 3 / egne_seg.presplit = 3, engine.PRESPLIT_TRUNK) of the edge network's
wide trunk tensors conv3_1 .. conv5_3, pool3, pool4 (vgg16_c.py:72-88) in the calibrated three-product inference plan.

The producers store the (hi, lo) f16 pair of x * s that every reader's staging would derive from the fp32 value; the readers copy it.  Operands
and order of products are those of the fp32-tensor plan, so everything here is compared BIT FOR BIT (``torch.equal``) with the fp32-tensor form."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture()
def G():
    g = torch.Generator()
    g.manual_seed(4321)
    return g


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _split(x, s):
    """(hi, lo) of x * s as every split-f16 staging path derives them (csrc/split_f16.h)."""
    t = x * s
    hi = t.half()
    return hi, (t - hi.float()).half()


def _pack(x_nhwc, s):
    """fp32 NHWC [..., C] (C % 32 == 0) -> the same bytes in channel-order split-pair storage: per 32-channel block 32 hi halves, then 32 lo halves."""
    hi, lo = _split(x_nhwc, s)
    C = x_nhwc.shape[-1]
    lead = x_nhwc.shape[:-1]
    planes = torch.stack([hi.reshape(*lead, C // 32, 32), lo.reshape(*lead, C // 32, 32)], dim=-2)      # [..., block, 2, 32]
    return planes.reshape(*lead, 2 * C).contiguous().view(torch.float32)


def _unpack(buf):
    """split-pair storage [..., C] (as fp32 words) -> (hi, lo) halves [..., C] in channel order."""
    C = buf.shape[-1]
    lead = buf.shape[:-1]
    planes = buf.contiguous().view(torch.float16).reshape(*lead, C // 32, 2, 32)
    return planes[..., 0, :].reshape(*lead, C), planes[..., 1, :].reshape(*lead, C)


@pytest.mark.parametrize("B,Cin,Cout,H,W,d,tail", [
    (47, 256, 512, 23, 31, 1, False),     # ragged last tile (33 511 pixels), two output tiles
    (110, 512, 512, 15, 20, 2, False),    # dilation 2, 144 K steps
    (102, 256, 384, 17, 19, 1, False),    # 128-wide output tiles, ragged last tile
    (40, 256, 512, 30, 40, 1, True),      # the last frames go to the 128 x 128 kernel (engine.BIG_SPLIT_TAIL)
])
def test_deep_trunk_kernel_split_pair_in_and_out(G, B, Cin, Cout, H, W, d, tail):
    """conv_f16x3_big_kernel<.., PS = 3> (and the flat kernel's PS = 3 form behind it): input held as split pairs, activations staged by LDS-DMA like
    the weights, output stored as pairs -- against the fp32-tensor launch of the same layer on the de-split input: the stored planes must be exactly
    hi = f16(o s), lo = f16(o s - hi) of that fp32 result o, s the power of two that puts max o in [1024, 2048); 32 guard channels in front of both
    slices stay untouched."""
    from gpu_util import DEV
    from egne_amd import engine
    from egne_amd.engine import ConvLayer, Piece, Plan, SplitScale
    x0 = F.relu(_rand(G, B, H, W, Cin))
    s_in = engine._a_scale_for(float(x0.max()))
    h0, l0 = _split(x0, s_in)
    x = (h0.float() + l0.float()) / s_in                          # the de-split input: what the stored tensor holds
    hi, lo = _split(x, s_in)
    assert torch.equal((hi.float() + lo.float()) / s_in, x) and engine._a_scale_for(float(x.max())) == s_in
    w, b = _rand(G, Cout, Cin, 3, 3) / (3 * Cin ** 0.5), _rand(G, Cout)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cin, Cin)], pad=(1, 1), dils=(d,), act=1)
    layer.split = True
    # fp32 tensors in and out
    pl0 = Plan(torch.device(DEV))
    xb = pl0.buf(B, H, W, Cin)
    xb.copy_(x.to(DEV))
    o0 = pl0.buf(B, H, W, Cout)
    pl0.conv(layer, [Piece(xb, 0, Cin)], Piece(o0, 0, Cout), B, H, W)
    want_calls = [c[0] for c in pl0.calls]       # (the planner cuts a ragged last round of workgroups off as a frame tail: both plans alike)
    assert want_calls in ([pl0.L.egne_conv2d_f16x3_big_fwd], [pl0.L.egne_conv2d_f16x3_big_fwd, pl0.L.egne_conv2d_f16x3_fwd])
    assert not tail or len(want_calls) == 2, "expected the big + tail launches"
    pl0.run()
    assert pl0.calls[0][1][2] == s_in, "the fp32-tensor launch calibrates to the storage scale"
    # split pairs in and out
    pl1 = Plan(torch.device(DEV))
    xs = pl1.buf(B, H, W, Cin + 32)
    xs.fill_(777.0)
    xs[..., 32:].copy_(_pack(x, s_in).to(DEV))
    pin = Piece(xs, 32, Cin)
    pin.split3 = SplitScale()
    pin.split3.value = s_in
    o1 = pl1.buf(B, H, W, Cout + 32)
    o1.fill_(777.0)
    pout = Piece(o1, 32, Cout)
    pout.split3 = SplitScale()
    pl1.conv(layer, [pin], pout, B, H, W)
    assert [c[0] for c in pl1.calls] == want_calls and len(pl1.post_cal3) == 1
    descs = [dd for _, dd in next(iter(pl1.post_cal3.values()))[0]]
    assert len(descs) == len(want_calls) and all(dd.seg[0].presplit == 3 and dd.out_split == 3 for dd in descs)
    pl1.run()          # calibrating run
    pl1.run()          # replay
    torch.cuda.synchronize()
    assert all(dd.out_split == 3 for dd in descs)
    s_out = pout.split3.value
    assert s_out == engine._a_scale_for(float(o0.max())), (s_out, float(o0.max()))
    assert (o1[..., :32] == 777.0).all(), "stores outside the output slice"
    assert (xs[..., :32] == 777.0).all()
    gh, gl = _unpack(o1[..., 32:])
    m = float((gh.float() + gl.float()).abs().max())
    assert 1024.0 <= m < 2048.0, (m, s_out)
    wh, wl = _split(o0, s_out)
    assert torch.equal(gh, wh), "hi plane differs from f16(fp32 result * scale): %d elements" % (gh != wh).sum().item()
    assert torch.equal(gl, wl), "lo plane differs: %d elements" % (gl != wl).sum().item()
    print("deep trunk kernel, split pairs in / out: %dx%dx%dx%d -> %d, scales %g -> %g, max stored %.1f" % (B, Cin, H, W, Cout, s_in, s_out, m))


def test_deep_trunk_kernel_fp32_in_split_pair_out(G):
    """conv3_1's form (its input pool2 stays fp32): converting input path, split-pair output."""
    from gpu_util import DEV
    from egne_amd import engine
    from egne_amd.engine import ConvLayer, Piece, Plan, SplitScale
    B, Cin, Cout, H, W = 28, 128, 256, 30, 40
    x = F.relu(_rand(G, B, H, W, Cin))
    w, b = _rand(G, Cout, Cin, 3, 3) / (3 * Cin ** 0.5), _rand(G, Cout)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cin, Cin)], pad=(1, 1), act=1)
    layer.split = True
    outs = []
    for on in (False, True):
        pl = Plan(torch.device(DEV))
        xb = pl.buf(B, H, W, Cin)
        xb.copy_(x.to(DEV))
        o = pl.buf(B, H, W, Cout + 32)
        o.fill_(777.0)
        po = Piece(o, 32, Cout)
        if on:
            po.split3 = SplitScale()
        pl.conv(layer, [Piece(xb, 0, Cin)], po, B, H, W)
        assert pl.calls[0][0] == pl.L.egne_conv2d_f16x3_big_fwd
        pl.run()
        pl.run()
        torch.cuda.synchronize()
        assert (o[..., :32] == 777.0).all()
        outs.append((o[..., 32:].clone(), po))
    (o0, _), (o1, po) = outs
    s = po.split3.value
    assert s == engine._a_scale_for(float(o0.max()))
    gh, gl = _unpack(o1)
    wh, wl = _split(o0, s)
    assert torch.equal(gh, wh) and torch.equal(gl, wl)


@pytest.mark.parametrize("B,Cin,H,W", [(11, 256, 60, 80), (41, 512, 30, 40), (70, 256, 23, 31)])
def test_halo_kernel_split_pair_input(G, B, Cin, H, W):
    """MSBlock 3x3 (bdcn_new.py:50) over a trunk tensor held as split pairs: the halo kernel copies the stored halves -- equal to its result
    on the fp32 tensor."""
    from gpu_util import DEV
    from egne_amd import engine
    from egne_amd.engine import ConvLayer, Piece, Plan, SplitScale
    x = F.relu(_rand(G, B, H, W, Cin))
    s_in = engine._a_scale_for(float(x.max()))
    w, b = _rand(G, 32, Cin, 3, 3) / (3 * Cin ** 0.5), _rand(G, 32)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cin, Cin)], pad=(1, 1), act=1)
    layer.split = True
    outs = []
    for on in (False, True):
        pl = Plan(torch.device(DEV))
        xb = pl.buf(B, H, W, Cin + 32)
        xb.fill_(777.0)
        xb[..., 32:].copy_((_pack(x, s_in) if on else x).to(DEV))
        pin = Piece(xb, 32, Cin)
        if on:
            pin.split3 = SplitScale()
            pin.split3.value = s_in
        o = pl.buf(B, H, W, 40)
        o.fill_(777.0)
        pl.conv(layer, [pin], Piece(o, 8, 32), B, H, W)
        assert [c[0] for c in pl.calls] == [pl.L.egne_conv3x3_halo_f16_fwd]
        assert [dd.seg[0].presplit for dd in pl.keep if hasattr(dd, "seg")] == [3 if on else 0]
        pl.run()
        pl.run()
        torch.cuda.synchronize()
        assert pl.calls[0][1][3] == s_in
        assert (o[..., :8] == 777.0).all()
        outs.append(o[..., 8:].clone())
    assert torch.equal(outs[0], outs[1]), "split-pair input: %d elements differ" % (outs[0] != outs[1]).sum().item()


@pytest.mark.parametrize("stride", [1, 2])
def test_maxpool_over_split_pairs_with_ties(G, stride):
    """egne_maxpool2_split against the split of egne_maxpool2's fp32 result, with neighbours whose hi + lo tie: t' = 1025.5 splits into (1026, -0.5)
    (round to even), t = 1025.5 - 2^-13 into (1025, 0.5) (the lo half rounds up to the midpoint): equal sums, different pairs, and the fp32
    pooling keeps t'."""
    from gpu_util import DEV
    from egne_amd.engine import Piece, Plan, SplitScale, maxpool_out
    B, H, W, C = 3, 31, 45, 64
    x = F.relu(_rand(G, B, H, W, C)) * 200.0
    t1 = 1025.5
    t0 = float(torch.tensor(t1) - 2.0 ** -13)
    ha, la = _split(torch.tensor([t0, t1]), 1.0)
    assert float(ha[0]) == 1025.0 and float(la[0]) == 0.5 and float(ha[1]) == 1026.0 and float(la[1]) == -0.5
    n = 0
    for yy in range(1, H - 1, 3):
        for xx in range(1, W - 2, 4):
            a, b_ = (t0, t1) if (n & 1) else (t1, t0)          # both orders inside a window
            if n % 3 == 2:
                x[:, yy, xx, :], x[:, yy + 1, xx, :] = a, b_     # vertical neighbours
            else:
                x[:, yy, xx, :], x[:, yy, xx + 1, :] = a, b_
            n += 1
    Ho, Wo = maxpool_out(H, stride), maxpool_out(W, stride)
    pl = Plan(torch.device(DEV))
    xf = pl.buf(B, H, W, C)
    xf.copy_(x.to(DEV))
    yf = pl.buf(B, Ho, Wo, C)
    pl.maxpool2(Piece(xf, 0, C), Piece(yf, 0, C), B, H, W, stride)
    xs = pl.buf(B, H, W, C + 32)
    xs.fill_(777.0)
    xs[..., 32:].copy_(_pack(x, 1.0).to(DEV))
    ys = pl.buf(B, Ho, Wo, C + 32)
    ys.fill_(777.0)
    ss = SplitScale()
    ss.value = 1.0
    pi, po = Piece(xs, 32, C), Piece(ys, 32, C)
    pi.split3 = po.split3 = ss
    pl.maxpool2(pi, po, B, H, W, stride)
    assert [c[0] for c in pl.calls] == [pl.L.egne_maxpool2, pl.L.egne_maxpool2_split]
    pl.run()
    torch.cuda.synchronize()
    assert torch.equal(yf.cpu(), F.max_pool2d(x.permute(0, 3, 1, 2), 2, stride, ceil_mode=True).permute(0, 2, 3, 1))
    assert (ys[..., :32] == 777.0).all()
    gh, gl = _unpack(ys[..., 32:])
    wh, wl = _split(yf, 1.0)
    ties = int(((wh == 1026.0) & (wl == -0.5)).sum())
    assert ties > 100, ties
    assert torch.equal(gh, wh) and torch.equal(gl, wl), "%d / %d elements differ" % ((gh != wh).sum().item(), (gl != wl).sum().item())


def _edge_plans(B, seed):
    """All 11 outputs of the edge network on B distinct frames with PRESPLIT_TRUNK off and on (calibrating run and replay each)."""
    from common import bdcn_module
    from gpu_util import DEV
    from egne_amd import engine, synth
    x = torch.cat((synth.make_batch(B, seed=seed)["img"],) * 3, 1).float().to(DEV)
    res = []
    old = engine.PRESPLIT_TRUNK
    try:
        for on in (False, True):
            engine.PRESPLIT_TRUNK = on
            bd = bdcn_module().to(DEV)
            first = [o.clone() for o in bd(x)]
            second = [o.clone() for o in bd(x)]
            assert not bd.overflowed()
            for a, b_ in zip(first, second):
                assert torch.equal(a, b_), "calibrating run and replay differ"
            res.append((bd, second))
    finally:
        engine.PRESPLIT_TRUNK = old
    return x, res


def _trunk_paths(pl):
    """(launch name, entry point, presplit of its input, out_split) of the stage 3-5 trunk launches, their MSBlock 3x3 and the poolings."""
    rows = []
    for fn, args, name in pl.calls:
        if not (name.startswith(("vgg.conv3", "vgg.conv4", "vgg.conv5")) or (name.startswith(("ms3", "ms4", "ms5")) and name.endswith(".conv")) or name == "vgg.pool"):
            continue
        if name == "vgg.pool":
            rows.append((name, fn, None, None))
            continue
        dd = args[0]._obj            # (ctypes.byref keeps its object)
        rows.append((name, fn, int(dd.seg[0].presplit), int(dd.out_split)))
    return rows


def test_edge_network_b64_identical_with_and_without_split_pair_trunk():
    """240x320, 64 distinct frames: all 11 outputs bit-identical between engine.PRESPLIT_TRUNK on and off; the on plan really stores conv3_1 ..
    conv5_3 / pool3 / pool4 as pairs and reads them so (deep trunk kernel, frame tails, MSBlock 3x3, pooling), the off plan nowhere.  Then a batch
    64x larger in magnitude than the calibration batch: check_overflow() re-calibrates producers and readers together, outputs again identical."""
    x, ((bd0, out0), (bd1, out1)) = _edge_plans(64, seed=20264)
    for k, (a, b_) in enumerate(zip(out0, out1)):
        assert torch.equal(a, b_), "output %d: %d elements differ (max %.3e)" % (k, (a != b_).sum().item(), (a - b_).abs().max().item())
    pl0, pl1 = bd0._last_plan, bd1._last_plan
    assert pl1.split3_trunk and not pl0.split3_trunk
    L = pl1.L
    r0, r1 = _trunk_paths(pl0), _trunk_paths(pl1)
    assert [r[0] for r in r0] == [r[0] for r in r1] and [r[1] for r in r0 if r[0] != "vgg.pool"] == [r[1] for r in r1 if r[0] != "vgg.pool"]
    assert len(pl0.calls) == len(pl1.calls), "the storage adds no launch"
    names = [r[0] for r in r1]
    assert sum(n.endswith(".tail") for n in names) == 6 and sum(n.startswith("ms") for n in names) == 9 and names.count("vgg.pool") == 2, names
    for name, fn, pin, pout in r0:
        assert fn is not L.egne_maxpool2_split and (pin, pout) in ((0, 0), (None, None)), (name, pin, pout)
    for name, fn, pin, pout in r1:
        if name == "vgg.pool":
            assert fn is L.egne_maxpool2_split, name
        elif name.startswith("ms"):
            assert fn is L.egne_conv3x3_halo_f16_fwd and (pin, pout) == (3, 0), (name, pin, pout)
        else:
            assert fn is (L.egne_conv2d_f16x3_fwd if name.endswith(".tail") else L.egne_conv2d_f16x3_big_fwd), name
            assert (pin, pout) == ((0, 3) if name.startswith("vgg.conv3_1") else (3, 3)), (name, pin, pout)
    # a batch 64x larger than the one the plans were calibrated on leaves the f16 range of the calibrated pre-scales
    big = []
    for bd in (bd0, bd1):
        pl = bd._last_plan
        pl.x_in.copy_(x * 64.0)
        pl.run()
        assert pl.check_overflow(), "the 64x batch must trip the overflow word"
        big.append([pl.outs[k].clone() for k in range(11)])
    for k, (a, b_) in enumerate(zip(*big)):
        assert torch.isfinite(a).all() and torch.equal(a, b_), "after re-calibration, output %d: %d elements differ" % (k, (a != b_).sum().item())


def test_edge_network_b2_identical_with_and_without_split_pair_trunk():
    """240x320, 2 frames: no layer of so small a batch reaches the deep trunk kernel (it starts at 32 768 output pixels), so the plan builder keeps every
    tensor fp32 (BDCN._build tries the storage from 32 768 pixels at stage 4 on, and falls back on engine.NeedsFp32Storage) -- the plans, and with them the outputs, are the same with the switch on and off."""
    _, ((bd0, out0), (bd1, out1)) = _edge_plans(2, seed=31)
    for k, (a, b_) in enumerate(zip(out0, out1)):
        assert torch.equal(a, b_), "output %d differs" % k
    pl0, pl1 = bd0._last_plan, bd1._last_plan
    assert "conv_f16x3:big" not in {k for k, _ in pl1.meta}
    assert not pl1.split3_trunk and not pl1.post_cal3
    assert [(c[0], c[2]) for c in pl0.calls] == [(c[0], c[2]) for c in pl1.calls]
