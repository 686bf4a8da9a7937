"""The float64 references of tests/small_op_refs.py against independent statements (torch.nn.functional, the oracle), so that a wrong
reference cannot vouch for a kernel in tests/test_gpu_small_ops.py.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import small_op_refs as R
from common import bdcn_module

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    scale = max(b.abs().max().item(), 1e-30)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, "max err %.3e vs scale %.3e" % (err, scale)


@pytest.mark.parametrize("B,H,W", [(1, 37, 53), (2, 9, 65)])
def test_tail_reference_reproduces_the_oracle_forward(B, H, W):
    """The score maps of oracle.bdcn.bdcn_forward through R.bdcn_tail give that function's eleven outputs (float64 round-off), with
    the stage sizes of R.bdcn_stage_geometry."""
    from oracle import bdcn as obdcn
    sd = {k: v.to(D) for k, v in bdcn_module(seed=3).state_dict().items()}
    for k in list(sd):                       # seeded heads are tiny: scale the side outputs up so that the sigmoids are not all 0.5
        if k.startswith("score_dsn") or k.startswith("fuse"):
            sd[k] = sd[k] * 30
    x = torch.randn(B, 3, H, W, generator=_g(1), dtype=D)
    with torch.no_grad():
        want = obdcn.bdcn_forward(sd, x)
        s_a, s_b = R.bdcn_scores_of_oracle(sd, x)
        hs, ws, strides, crops = R.bdcn_stage_geometry(H, W)
        assert [tuple(t.shape[-2:]) for t in s_a] == list(zip(hs, ws))
        ups = [None] + [sd[obdcn.UPS[k][0] + ".weight"] for k in "2345"]
        got, _ = R.bdcn_tail(s_a, s_b, ups, strides, crops, sd["fuse.weight"].reshape(10), sd["fuse.bias"], H, W)
        thr, _ = R.bdcn_tail(s_a, s_b, ups, strides, crops, sd["fuse.weight"].reshape(10), sd["fuse.bias"], H, W, edge_thres=1)
    assert len(got) == 11
    assert max(w.std().item() for w in want) > 1e-3, "degenerate fixture"
    for g, w in zip(got, want):
        _close(g, w, 1e-13)
    e = torch.where(want[-1] >= 0.1, torch.ones_like(want[-1]), want[-1])       # utils.calc_edge / oracle.bdcn.calc_edge
    assert (e == 1).any() and (e < 0.1).any(), "the fixture must have pixels on both sides of the switch"
    assert torch.equal(thr[-1], e)
    for g, w in zip(thr[:10], want[:10]):
        _close(g, w, 1e-13)


@pytest.mark.parametrize("B,H,W", [(1, 100, 100), (2, 37, 53), (2, 240, 320), (3, 9, 65)])
def test_tail_threshold_margin_of_seeded_score_maps(B, H, W):
    """Seeded Gaussian score maps of magnitude 3 (the inputs of the device test): hardly any fused value lies near the edge_thres
    switch (sigmoid = 0.1), so excluding the pixels within the kernel's fp32 error of it removes far less than 0.1 % of a frame."""
    import math
    s_a, s_b, ups, strides, crops, fw, fb = R.bdcn_tail_inputs(B, H, W, seed=7)
    _, fuse = R.bdcn_tail([t.to(D) for t in s_a], [t.to(D) for t in s_b], [u if u is None else u.to(D) for u in ups], strides, crops,
                          fw.to(D), fb.to(D), H, W, edge_thres=1)
    near = ((fuse - math.log(0.1 / 0.9)).abs() < 1e-4 * fuse.abs().max()).sum().item()
    assert near < 1e-3 * fuse.numel(), near


def test_stage_scores_reference_is_the_oracle_convs():
    g = _g(2)
    B, h, w = 2, 5, 7
    ms = [torch.randn(B, 32, h, w, generator=g, dtype=D) for _ in range(3)]
    wd, bd = torch.randn(3, 21, 32, generator=g, dtype=D), torch.randn(3, 21, generator=g, dtype=D)
    ws, ws1 = torch.randn(21, generator=g, dtype=D), torch.randn(21, generator=g, dtype=D)
    bs, bs1 = torch.randn(1, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    tot = sum(F.conv2d(m, wd[k].reshape(21, 32, 1, 1), bd[k]) for k, m in enumerate(ms))
    want = F.conv2d(tot, ws.reshape(1, 21, 1, 1), bs), F.conv2d(tot, ws1.reshape(1, 21, 1, 1), bs1)
    got = R.bdcn_stage_scores([m.permute(0, 2, 3, 1).reshape(-1, 32) for m in ms], wd, bd, ws, bs, ws1, bs1)
    for a, b in zip(got, want):
        _close(a.reshape(B, h, w), b[:, 0], 1e-13)


def test_adain_softmax_conf_references():
    g = _g(3)
    B, HW, C = 3, 17, 6
    x = torch.randn(B, HW, C, generator=g, dtype=D) * 2 + 1
    gam, bet = torch.randn(B, C, generator=g, dtype=D), torch.randn(B, C, generator=g, dtype=D)
    # AdaIN == instance norm with the unbiased variance: rescale F.instance_norm's biased one
    xc = x.permute(0, 2, 1)
    mean, var_u = xc.mean(2, keepdim=True), xc.var(2, unbiased=True, keepdim=True)
    want = ((xc - mean) / torch.sqrt(var_u + 1e-5) * gam[:, :, None] + bet[:, :, None]).permute(0, 2, 1)
    _close(R.adain(x, gam, bet), want, 1e-13)
    inorm = F.instance_norm(xc, eps=1e-5 * (HW - 1) / HW) * ((HW - 1) / HW) ** 0.5      # (x - m) / sqrt(var_b + e') rescaled to var_u + e
    _close(R.adain(x, gam, bet), (inorm * gam[:, :, None] + bet[:, :, None]).permute(0, 2, 1), 1e-12)
    # a constant channel: variance 0, std sqrt(eps), output beta
    xk = x.clone()
    xk[:, :, 2] = 0.75
    _close(R.adain(xk, gam, bet)[:, :, 2], bet[:, None, 2].expand(B, HW), 1e-12)
    # softmax3
    l3 = 60 * torch.randn(5, 7, 3, generator=g, dtype=D)
    _close(R.softmax3(l3), F.softmax(l3, dim=-1))
    _close(R.softmax3(l3), torch.exp(l3 - torch.logsumexp(l3, -1, keepdim=True)), 1e-12)
    # conf loss, both flags
    p, gt = torch.randn(6, 4, generator=g, dtype=D), torch.randint(0, 4, (6,), generator=g)
    _close(R.conf_loss(p, gt, 1), (F.softmax(p, 1) - 0.25).abs().sum() / 24)
    _close(R.conf_loss(p, gt, 0), -F.log_softmax(p, 1)[torch.arange(6), gt].mean(), 1e-13)
    t0, t7 = R.conf_terms(p, gt, 1, 2.0, torch.tensor(5.0, dtype=D))
    _close(t0, 5.0 + 2.0 * t7)
    t0, t7 = R.conf_terms(p, gt, 0, 2.0, torch.tensor(5.0, dtype=D))
    assert t0 == t7


def test_head_references():
    g = _g(4)
    x = torch.randn(4, 10, generator=g, dtype=D) * 2
    y = R.ellipse_head_act(x)
    for o in (0, 5):
        _close(y[:, o:o + 2], torch.tanh(x[:, o:o + 2]))
        _close(y[:, o + 2:o + 4], 1 / (1 + torch.exp(-x[:, o + 2:o + 4])), 1e-14)
        assert torch.equal(y[:, o + 4], x[:, o + 4])
    v = torch.linspace(-20, 20, 41, dtype=D)
    a, s = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
    _close(R.selu(v), s * torch.where(v > 0, v, a * torch.expm1(v)), 1e-14)
    m = torch.randn(2, 9, 5, generator=g, dtype=D)
    _close(R.spatial_mean(m), m.sum(1) / 9, 1e-14)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (5, 6), (15, 20)])
def test_resampling_transposes_against_autograd(H, W):
    g = _g(5)
    B, C = 2, 3
    x = torch.randn(B, C, H, W, generator=g, dtype=D, requires_grad=True)
    gy = torch.randn(B, 2 * H, 2 * W, C, generator=g, dtype=D)
    nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
    (want,) = torch.autograd.grad((F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) * nchw(gy)).sum(), x)
    _close(nchw(R.upsample2x_bwd(gy)), want, 1e-13)
    (want,) = torch.autograd.grad((F.interpolate(x, scale_factor=2, mode="nearest") * nchw(gy)).sum(), x)
    _close(nchw(R.upsample2x_nearest_bwd(gy)), want, 1e-13)
    assert torch.equal(nchw(R.upsample2x_nearest(x.detach().permute(0, 2, 3, 1))), F.interpolate(x.detach(), scale_factor=2, mode="nearest"))
    if H >= 2 and W >= 2:
        gq = torch.randn(B, H // 2, W // 2, C, generator=g, dtype=D)
        (want,) = torch.autograd.grad((F.avg_pool2d(x, 2) * nchw(gq)).sum(), x)
        _close(nchw(R.avgpool2_bwd(gq, H, W)), want, 1e-13)


@pytest.mark.parametrize("H,W,P", [(4, 4, 3), (2, 2, 1), (45, 70, 3), (5, 7, 1), (6, 9, 0)])
def test_reflect_pad_transpose_against_autograd(H, W, P):
    g = _g(6)
    B, C = 2, 4
    x = torch.randn(B, C, H, W, generator=g, dtype=D, requires_grad=True)
    gp = torch.randn(B, H + 2 * P, W + 2 * P, C, generator=g, dtype=D)
    (want,) = torch.autograd.grad((F.pad(x, (P, P, P, P), mode="reflect") * gp.permute(0, 3, 1, 2)).sum(), x) if P else (gp.permute(0, 3, 1, 2),)
    _close(R.reflect_pad_bwd(gp, P).permute(0, 3, 1, 2), want, 1e-13)
    if (H + 2 * P) % 2 == 0 and (W + 2 * P) % 2 == 0:
        # the phase-packed layout, element by element: block (py & 1) * 2 + (px & 1) of pixel (py >> 1, px >> 1)
        pk = R.phase_pack(gp)
        assert pk.shape == (B, (H + 2 * P) // 2, (W + 2 * P) // 2, 4 * C)
        for py in range(H + 2 * P):
            for px in range(W + 2 * P):
                blk = (py & 1) * 2 + (px & 1)
                assert torch.equal(pk[:, py >> 1, px >> 1, blk * C:(blk + 1) * C], gp[:, py, px])


def test_loss_backward_reference_routes_the_iris_centre():
    """Without any mask in the batch pred_c's iris row is elOut[:, 5:7] (oracle.losses.all_loss), so its upstream gradient lands in
    g_elOut and not in the logits; with a mask it lands in the logits."""
    g = _g(8)
    B, H, W = 3, 6, 8
    op = torch.randn(B, 3, H, W, generator=g, dtype=D)
    elOut = torch.rand(B, 10, generator=g, dtype=D) * 2 - 1
    tgt = torch.randint(0, 3, (B, H, W), generator=g)
    pc = torch.rand(B, 2, generator=g, dtype=D) * torch.tensor([W, H])
    eln = torch.rand(B, 2, 5, generator=g, dtype=D) * 2 - 1
    sw, dist = torch.rand(B, H, W, generator=g, dtype=D) + 1, torch.randn(B, 3, H, W, generator=g, dtype=D)
    gpc = torch.randn(B, 2, 2, generator=g, dtype=D)
    for absent in (True, False):
        cond = torch.zeros(B, 4, dtype=D)
        if absent:
            cond[:, 1:] = 1
        g0 = R.loss_head_bwd(op, elOut, tgt, pc, eln, sw, dist, cond, 0.3, 0.0)
        assert g0[0].abs().max() == 0 and g0[1].abs().max() == 0
        gl, ge = R.loss_head_bwd(op, elOut, tgt, pc, eln, sw, dist, cond, 0.3, 0.0, g_pred_c=gpc)
        if absent:
            _close(ge[:, 5:7], gpc[:, 0])
            assert gl[:, 0].abs().max() == 0          # channel 0 (the iris soft-argmax) gets nothing
        else:
            assert ge.abs().max() == 0 and gl[:, 0].abs().max() > 0
        assert gl[:, 2].abs().max() > 0 and gl[:, 1].abs().max() == 0


# ---- normalisation, pooling, bilinear up-sampling (tests/test_gpu_norm_pool_ops.py) ------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 4), (3, 8, 6, 7)])
def test_norm_references_against_instance_and_batch_norm(B, H, W, C):
    g = _g(20 + H)
    x = torch.randn(B, H * W, C, generator=g, dtype=D) * 3 + 0.5
    xc = x.permute(0, 2, 1)                                         # [B, C, HW]
    gam, bet = torch.randn(C, generator=g, dtype=D) + 1, torch.randn(C, generator=g, dtype=D)
    # statistics: scale / shift reproduce the normalised tensor, mean / variance are the biased moments
    for ps in (1, 0):
        sc, sh, mean, var = R.norm_stats(x, ps)
        assert sc.shape == ((B, C) if ps else (1, C))
        want = F.instance_norm(xc, eps=1e-5) if ps else F.batch_norm(xc, None, None, training=True, eps=1e-5)
        _close((x * sc[:, None] + sh[:, None]).permute(0, 2, 1), want)
        dims = (2,) if ps else (0, 2)
        _close(mean, xc.mean(dims).reshape(mean.shape))
        _close(var, xc.var(dims, unbiased=False).reshape(var.shape))
        # partial sums of ragged chunks give the same statistics
        cuts = [0, 1, H * W // 2, H * W]
        xs = x if ps else x.reshape(1, B * H * W, C)
        if not ps:
            cuts = [0, 1, H * W + 2, B * H * W]
        parts = torch.stack([torch.stack([xs[:, a:b].sum(1), (xs[:, a:b] ** 2).sum(1)], -1) for a, b in zip(cuts, cuts[1:])], 1)
        for a, b in zip(R.stats_finish(parts, xs.shape[1]), (sc, sh, mean, var)):
            _close(a, b, 1e-11)
    # forward whose vjp is the reference of egne_norm_bwd
    for act_in, fn in ((0, lambda t: t), (1, F.relu), (2, lambda t: F.leaky_relu(t, 0.01))):
        _close(R.norm_fwd(x, None, None, 1, act_in).permute(0, 2, 1), fn(F.instance_norm(xc, eps=1e-5)))
    _close(R.norm_fwd(x, gam, bet, 0, 0).permute(0, 2, 1), F.batch_norm(xc, None, None, gam, bet, training=True, eps=1e-5))
    gy = torch.randn(B, H * W, C, generator=g, dtype=D)
    xa, ga, ba = xc.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    want = torch.autograd.grad((F.batch_norm(xa, None, None, ga, ba, training=True, eps=1e-5) * gy.permute(0, 2, 1)).sum(), (xa, ga, ba))
    got = R.vjp(lambda a, b, c: R.norm_fwd(a, b, c, 0, 0), [x, gam, bet], [gy])
    _close(got[0].permute(0, 2, 1), want[0])
    _close(got[1], want[1])
    _close(got[2], want[2])
    xa = xc.clone().requires_grad_(True)
    (want,) = torch.autograd.grad((F.leaky_relu(F.instance_norm(xa, eps=1e-5), 0.01) * gy.permute(0, 2, 1)).sum(), xa)
    (got,) = R.vjp(lambda a: R.norm_fwd(a, None, None, 1, 2), [x], [gy])
    _close(got.permute(0, 2, 1), want)


def test_norm_stats_reference_takes_a_single_pixel():
    x = torch.tensor([[[3.0, -2.0]]], dtype=D)
    sc, sh, mean, var = R.norm_stats(x, 1)
    assert torch.equal(var, torch.zeros(1, 2, dtype=D)) and torch.equal(mean, x[:, 0])
    _close(sc, torch.full((1, 2), 1e-5, dtype=D).rsqrt())
    assert (x[:, 0] * sc + sh).abs().max().item() < 1e-12


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 3), (1, 2, 2, 4), (2, 6, 4, 5)])
def test_pooling_and_affine_references(B, H, W, C):
    g = _g(30 + H)
    x = torch.randn(B, H, W, C, generator=g, dtype=D)
    _close(_nchw(R.avgpool2(x)), F.avg_pool2d(_nchw(x), 2), 1e-15)
    assert R.avgpool2(x).shape == (B, H // 2, W // 2, C)
    a, b = torch.randn(C, generator=g, dtype=D), torch.randn(C, generator=g, dtype=D)
    assert torch.equal(R.affine(x, a, b), x * a + b)
    assert torch.equal(R.affine_act(x, a, b, kind=2), F.leaky_relu(x * a + b, 0.01))
    assert torch.equal(R.affine_act(x, a, b), F.relu(x * a + b)) and torch.equal(R.affine_act(x, a, b, False), x * a + b)
    sc, sh = torch.rand(B, C, generator=g, dtype=D) + 0.5, torch.randn(B, C, generator=g, dtype=D)
    t = _nchw(x) * sc[:, :, None, None] + sh[:, :, None, None]
    for kind, fn in ((0, lambda v: v), (1, F.relu), (2, lambda v: F.leaky_relu(v, 0.01))):
        _close(_nchw(R.norm_act_pool2(x, sc, sh, kind)), F.avg_pool2d(fn(t), 2), 1e-15)


@pytest.mark.parametrize("H,W", [(2, 2), (25, 13), (7, 2), (6, 8)])
@pytest.mark.parametrize("stride", [1, 2])
def test_maxpool_reference_against_ceil_mode_max_pool2d(H, W, stride):
    g = _g(40 + H)
    for x in (torch.randn(2, H, W, 3, generator=g, dtype=D), -1.0 - torch.rand(2, H, W, 3, generator=g, dtype=D),
              (torch.randn(2, H, W, 3, generator=g, dtype=D) * 2).round() / 2):
        want = F.max_pool2d(_nchw(x), 2, stride, ceil_mode=True)
        assert torch.equal(_nchw(R.maxpool2(x, stride)), want)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (3, 5)])
def test_upsample_reference_against_bilinear_interpolate(H, W):
    x = torch.randn(2, H, W, 3, generator=_g(50 + H + W), dtype=D)
    _close(_nchw(R.upsample2x(x)), F.interpolate(_nchw(x), scale_factor=2, mode="bilinear", align_corners=False), 1e-15)


@pytest.mark.parametrize("shape", [(7, 4), (2, 3, 5, 6)])
def test_act_bwd_bias_reference_against_autograd(shape):
    """The masked gradient is autograd of the activation wherever the output is not 0; at y = 0 the kernel's documented branch is the
    slope (F.leaky_relu's own choice there), for ReLU as well."""
    g = _g(60 + len(shape))
    z = torch.randn(*shape, generator=g, dtype=D)
    z.reshape(-1)[::5] = 0.0
    gy = torch.randn(*shape, generator=g, dtype=D)
    for kind, slope in ((0, 1.0), (1, 0.0), (2, 0.01)):
        za = z.clone().requires_grad_(True)
        y = F.leaky_relu(za, slope)
        (want,) = torch.autograd.grad((y * gy).sum(), za)
        gz, db = R.act_bwd_bias(gy, y.detach(), kind)
        _close(gz, want, 1e-15)
        _close(db, want.reshape(-1, shape[-1]).sum(0), 1e-14)
        assert torch.equal(gz[z == 0], gy[z == 0] * slope)
