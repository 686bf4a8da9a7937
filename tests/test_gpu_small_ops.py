"""-m gpu: the small kernels of csrc/adain.hip, elementwise.hip, backward.hip, loss.hip and bdcn_tail.hip, one C-ABI call at a time,
against the float64 references of tests/small_op_refs.py (pinned by tests/test_host_small_op_refs.py).

Conventions: seeded CPU inputs; every output is a channel slice at a non-zero offset of a wider buffer whose other elements hold
POISON and must come back untouched; accumulating kernels start from a seeded non-zero destination and must leave pre-fill +
gradient, the storing forms overwrite POISON.

Tolerances (small_op_refs.bound): the same operation is done in fp32 by torch on the CPU and its error against float64 measured,
relative to the output's absolute maximum; the kernel may have four times that, not less than 4 fp32 ulps of the output scale.  Both
numbers are printed by every test.  Copies, selections and fixed-association sums are compared bit for bit.  A bf16 twin on
bf16-representable inputs agrees with its fp32 original to one bf16 rounding of the result (EPS of tests/test_gpu_bf16.py)."""
import ctypes as C

import pytest
import torch

import small_op_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 777.0
BF = torch.bfloat16
EPS = 2.0 ** -8          # one bf16 rounding (tests/test_gpu_bf16.py)
D = torch.float64


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from egne_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _q(x):
    """Round to bf16-representable fp32."""
    return x.to(BF).float()


def _buf(x, stride, off, dtype=torch.float32):
    """x [..., C] (CPU) as the slice off:off+C of a POISON-filled [..., stride] device buffer."""
    b = torch.full(tuple(x.shape[:-1]) + (stride,), POISON, dtype=dtype)
    b[..., off:off + x.shape[-1]] = x.to(dtype)
    return b.to(DEV)


def _poison(shape, dtype=torch.float32):
    return torch.full(tuple(shape), POISON, dtype=dtype, device=DEV)


def _slice(buf, before, off, Cn):
    """The slice off:off+Cn of a device buffer as fp32 on the CPU, after asserting that nothing outside it differs from ``before``."""
    a, b = buf.cpu(), before.cpu()
    got = a[..., off:off + Cn].float().clone()
    a[..., off:off + Cn] = 0
    b[..., off:off + Cn] = 0
    assert torch.equal(a, b), "the kernel wrote outside its slice"
    return got


def _check(name, got, ref64, cpu32):
    bnd, e32 = R.bound(ref64, cpu32)
    err = R.rel_err(got, ref64)
    print("%s: err %.3e (fp32 on the CPU %.3e, bound %.3e)" % (name, err, e32, bnd))
    assert err <= bnd, "%s: err %.3e above %.3e (4 x the CPU's fp32 error %.3e, floor 4 ulp)" % (name, err, bnd, e32)


def _twin(name, o16, o32):
    err = (o16.float() - o32.float()).abs().max().item()
    lim = EPS * o32.float().abs().max().item() * 1.01
    print("%s: bf16 twin differs by %.3e (one rounding: %.3e)" % (name, err, lim))
    assert err <= lim, "%s: bf16 twin differs by %.3e > %.3e" % (name, err, lim)


def _sync():
    torch.cuda.synchronize()


def _same32(name, a16, a32):
    """An output that is fp32 in the bf16 twin and in the fp32 kernel (loss terms, parameter sums): 1e-6 of its largest element."""
    scale = max(a32.abs().max().item(), 1e-30)
    err = (a16.double() - a32.double()).abs().max().item() / scale
    print("%s: bf16 twin's fp32 output differs by %.3e (limit 1e-6)" % (name, err))
    assert err <= 1e-6, "%s: the twin's fp32 output differs by %.3e" % (name, err)


# ==== AdaIN fusion path ===============================================================================================================
@pytest.mark.parametrize("mag", [1.0, 60.0])
@pytest.mark.parametrize("Cp_out", [3, 8])
@pytest.mark.parametrize("npix", [1, 300, 2 * 240 * 320, 16 * 240 * 320])
def test_softmax3_and_backward(lib, npix, Cp_out, mag):
    """egne_softmax3 / egne_softmax3_bwd; 16*240*320 pixels are more than 4096 * 256: the grid-stride loop runs.
    MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(11)
    x = mag * torch.randn(npix, 3, generator=g)
    gy = torch.randn(npix, 3, generator=g)
    pre = torch.randn(npix, 3, generator=g)
    xs, xo, ys, yo = 5, 1, Cp_out + 3, 2
    xb, yb = _buf(x, xs, xo), _poison((npix, ys))
    y0 = yb.clone()
    _lib.check(L.egne_softmax3(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, Cp_out, npix, st))
    _sync()
    got = _slice(yb, y0, yo, Cp_out)
    _check("softmax3", got[:, :3], R.softmax3(x.double()), R.softmax3(x))
    assert (got[:, 3:] == 0).all(), "channels 3..Cp_out must be written as zeros"
    # backward on the forward's own output: gx += y * (gy - <gy, y>)
    gyb, gxb = _buf(gy, 4, 1), _buf(pre, 6, 2)
    g0 = gxb.clone()
    _lib.check(L.egne_softmax3_bwd(yb.data_ptr(), ys, yo, gyb.data_ptr(), 4, 1, gxb.data_ptr(), 6, 2, npix, st))
    _sync()
    (r64,) = R.vjp(R.softmax3, [x.double()], [gy.double()])
    (r32,) = R.vjp(R.softmax3, [x], [gy])
    _check("softmax3_bwd", _slice(gxb, g0, 2, 3), pre.double() + r64, pre + r32)


def test_softmax3_bf16_twin(lib):
    _lib, L, st = lib
    g = _g(12)
    npix = 5000
    x, gy, pre = (_q(torch.randn(npix, 3, generator=g) * s) for s in (3.0, 1.0, 1.0))
    outs = []
    for dt, fw, bw in ((torch.float32, L.egne_softmax3, L.egne_softmax3_bwd), (BF, L.egne_softmax3_bf16, L.egne_softmax3_bwd_bf16)):
        xb, yb = _buf(x, 8, 1, dt), _poison((npix, 8), dt)
        _lib.check(fw(xb.data_ptr(), 8, 1, yb.data_ptr(), 8, 2, 3, npix, st))
        _sync()
        y = yb[:, 2:5].clone()
        # the backward of both reads the SAME bf16-representable y
        yin = _buf(_q(outs[0][0].cpu()) if outs else _q(y.float().cpu()), 8, 2, dt)
        gyb, gxb = _buf(gy, 8, 0, dt), _buf(pre, 8, 3, dt)
        _lib.check(bw(yin.data_ptr(), 8, 2, gyb.data_ptr(), 8, 0, gxb.data_ptr(), 8, 3, npix, st))
        _sync()
        outs.append((y.float(), gxb[:, 3:6].float()))
    _twin("softmax3", outs[1][0], outs[0][0])
    _twin("softmax3_bwd", outs[1][1], outs[0][1])


def _adain_inputs(B, HW, Cn, kind, seed):
    g = _g(seed)
    x = torch.randn(B, HW, Cn, generator=g)
    if kind == "mean100":
        x = 100.0 + 0.1 * x
    elif kind == "const":
        x[:, :, 1] = 0.75
        x[0, :, Cn - 1] = -3.0
    gam, bet = torch.randn(B, Cn, generator=g) + 1.0, torch.randn(B, Cn, generator=g)
    gy, pre = torch.randn(B, HW, Cn, generator=g), torch.randn(B, HW, Cn, generator=g)
    pgg, pgb = torch.randn(B, Cn, generator=g), torch.randn(B, Cn, generator=g)
    return x, gam, bet, gy, pre, pgg, pgb


def _run_adain(lib, B, HW, Cn, ins, dt=torch.float32):
    """One forward and one backward call.  gamma / beta are the columns gb_off + c and gb_off + Cn + c of one row buffer (the MLP's
    output row, esf_engine.py:577-585), their gradients go to the same columns of a pre-filled gradient row."""
    _lib, L, st = lib
    x, gam, bet, gy, pre, pgg, pgb = ins
    esz = 4 if dt == torch.float32 else 2
    fw, bw = (L.egne_adain, L.egne_adain_bwd) if dt == torch.float32 else (L.egne_adain_bf16, L.egne_adain_bwd_bf16)
    Cs = (Cn + 7) // 8 * 8
    xs, xo, ys, yo, gb_off, row = Cs + 8, 3, Cs + 16, 5, 2, 2 * Cn + 7
    xb, yb = _buf(x, xs, xo, dt), _poison((B, HW, ys), dt)
    rowb = _buf(torch.cat([gam, bet], 1), row, gb_off, dt)
    y0 = yb.clone()
    _lib.check(fw(xb.data_ptr(), xs, xo, Cn, rowb.data_ptr(), rowb.data_ptr() + esz * Cn, row, gb_off, yb.data_ptr(), ys, yo, B, HW, 1e-5, st))
    _sync()
    y = _slice(yb, y0, yo, Cn)
    gyb, gxb = _buf(gy, Cs + 8, 1, dt), _buf(pre, Cs + 8, 6, dt)
    grow = _buf(torch.cat([pgg, pgb], 1), row, gb_off, dt)
    gx0, gr0 = gxb.clone(), grow.clone()
    _lib.check(bw(xb.data_ptr(), xs, xo, Cn, rowb.data_ptr(), row, gb_off, gyb.data_ptr(), Cs + 8, 1, gxb.data_ptr(), Cs + 8, 6,
                  grow.data_ptr(), grow.data_ptr() + esz * Cn, row, gb_off, B, HW, 1e-5, st))
    _sync()
    gr = _slice(grow, gr0, gb_off, 2 * Cn)
    return y, _slice(gxb, gx0, 6, Cn), gr[:, :Cn], gr[:, Cn:]


def _check_adain(lib, B, HW, Cn, kind, seed):
    ins = _adain_inputs(B, HW, Cn, kind, seed)
    x, gam, bet, gy, pre, pgg, pgb = ins
    y, gx, gg, gb = _run_adain(lib, B, HW, Cn, ins)
    tag = "adain[B%d HW%d C%d %s]" % (B, HW, Cn, kind)
    _check(tag, y, R.adain(x.double(), gam.double(), bet.double()), R.adain(x, gam, bet))
    r64 = R.vjp(R.adain, [x.double(), gam.double(), bet.double()], [gy.double()])
    r32 = R.vjp(R.adain, [x, gam, bet], [gy])
    _check(tag + " gx", gx, pre.double() + r64[0], pre + r32[0])
    _check(tag + " ggamma", gg, pgg.double() + r64[1], pgg + r32[1])
    _check(tag + " gbeta", gb, pgb.double() + r64[2], pgb + r32[2])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [2, 7, 300, 1200])
@pytest.mark.parametrize("Cn", [16, 32, 38, 64])
def test_adain_and_backward(lib, Cn, HW, B):
    """egne_adain / egne_adain_bwd (unbiased variance: HW - 1 inside the gradient; gx, ggamma, gbeta accumulate).  C = 16 and 38 leave
    a partial 32-channel group, HW = 2 is the smallest legal map.  MI355X: not yet recorded."""
    _check_adain(lib, B, HW, Cn, "randn", 100 * Cn + HW + B)


@pytest.mark.parametrize("kind", ["mean100", "const"])
def test_adain_offset_mean_and_constant_channel(lib, kind):
    """Per-channel mean 100 / std 0.1 (the sum of squares must be formed in double) and a constant channel (variance clamps to 0, the
    output is beta as in the model).  MI355X: not yet recorded."""
    _check_adain(lib, 3, 300, 38, kind, 77)


def test_adain_rejects_a_single_pixel(lib):
    _lib, L, st = lib
    z = torch.zeros(64, device=DEV)
    p = z.data_ptr()
    assert L.egne_adain(p, 8, 0, 8, p, p, 8, 0, p, 8, 0, 1, 1, 1e-5, st) != 0
    assert L.egne_adain_bwd(p, 8, 0, 8, p, 8, 0, p, 8, 0, p, 8, 0, p, p, 8, 0, 1, 1, 1e-5, st) != 0
    _sync()
    assert (z == 0).all()


def test_adain_bf16_twin(lib):
    B, HW, Cn = 3, 300, 38
    ins = tuple(_q(t) for t in _adain_inputs(B, HW, Cn, "randn", 5))
    o32 = _run_adain(lib, B, HW, Cn, ins)
    o16 = _run_adain(lib, B, HW, Cn, ins, BF)
    for n, a, b in zip(("adain", "adain_bwd gx", "adain_bwd ggamma", "adain_bwd gbeta"), o16, o32):
        _twin(n, a, b)


@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("Cn", [2, 4])
@pytest.mark.parametrize("B", [1, 6, 300])
def test_conf_loss_and_backward(lib, B, Cn, flag):
    """egne_conf_loss (one block: B = 300 is more samples than threads) / egne_conf_loss_bwd.  MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(31 + B + Cn)
    x = torch.randn(B, Cn, generator=g)
    gt = torch.randint(0, Cn, (B,), generator=g)
    tie = (torch.softmax(x.double(), 1) - 1.0 / Cn).abs().min().item()
    assert tie > 1e-5, "an L1 term sits on its kink (%.2e): choose another seed" % tie
    ld, gld, weight, gscale = Cn + 3, Cn + 2, 2.0, 0.37
    xb = _buf(x, ld, 0)
    terms = _poison((8,))
    terms[0] = 5.0
    gtd = gt.to(DEV)
    _lib.check(L.egne_conf_loss(xb.data_ptr(), ld, gtd.data_ptr(), B, Cn, flag, weight, terms.data_ptr(), st))
    gsc = torch.tensor([gscale], device=DEV)
    gxb = _poison((B, gld))
    g0 = gxb.clone()
    _lib.check(L.egne_conf_loss_bwd(xb.data_ptr(), ld, gtd.data_ptr(), B, Cn, flag, gsc.data_ptr(), gxb.data_ptr(), gld, st))
    _sync()
    t = terms.cpu()
    assert (t[1:7] == POISON).all()
    t0_64, t7_64 = R.conf_terms(x.double(), gt, flag, weight, torch.tensor(5.0, dtype=D))
    t0_32, t7_32 = R.conf_terms(x, gt, flag, weight, torch.tensor(5.0))
    _check("conf_loss terms[7]", t[7:8], t7_64.reshape(1), t7_32.reshape(1))
    _check("conf_loss terms[0] (%s)" % ("accumulated" if flag else "replaced"), t[0:1], t0_64.reshape(1), t0_32.reshape(1))
    f = lambda p: gscale * R.conf_loss(p, gt, flag)  # noqa: E731
    (r64,) = R.vjp(f, [x.double()], [torch.ones((), dtype=D)])
    (r32,) = R.vjp(f, [x], [torch.ones(())])
    _check("conf_loss_bwd", _slice(gxb, g0, 0, Cn), r64, r32)


@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("B,Cn", [(1, 2), (6, 4)])
def test_conf_loss_bf16_twin(lib, B, Cn, flag):
    """egne_conf_loss_bf16 / egne_conf_loss_bwd_bf16 on the inputs of test_conf_loss_and_backward rounded to bf16: the loss terms are
    fp32 in both, the gradient differs by one bf16 rounding."""
    _lib, L, st = lib
    g = _g(31 + B + Cn)
    x = _q(torch.randn(B, Cn, generator=g))
    gt = torch.randint(0, Cn, (B,), generator=g).to(DEV)
    ld, gld = Cn + 3, Cn + 2
    gsc = torch.tensor([0.37], device=DEV)
    outs = []
    for dt, fw, bw in ((torch.float32, L.egne_conf_loss, L.egne_conf_loss_bwd), (BF, L.egne_conf_loss_bf16, L.egne_conf_loss_bwd_bf16)):
        xb, terms, gxb = _buf(x, ld, 0, dt), _poison((8,)), _poison((B, gld), dt)
        terms[0] = 5.0
        g0 = gxb.clone()
        _lib.check(fw(xb.data_ptr(), ld, gt.data_ptr(), B, Cn, flag, 2.0, terms.data_ptr(), st))
        _lib.check(bw(xb.data_ptr(), ld, gt.data_ptr(), B, Cn, flag, gsc.data_ptr(), gxb.data_ptr(), gld, st))
        _sync()
        t = terms.cpu()
        assert (t[1:7] == POISON).all()
        outs.append((t[[0, 7]], _slice(gxb, g0, 0, Cn)))
    _same32("conf_loss terms", outs[1][0], outs[0][0])
    _twin("conf_loss_bwd", outs[1][1], outs[0][1])


@pytest.mark.parametrize("P,phase,B,H,W,Cp", [(3, 0, 2, 4, 4, 8), (3, 0, 2, 45, 70, 8), (1, 0, 2, 2, 2, 4), (1, 0, 1, 45, 70, 12),
                                              (1, 1, 2, 2, 2, 8), (1, 1, 2, 46, 70, 8), (3, 0, 2, 240, 320, 112)])
def test_reflect_pad_backward(lib, P, phase, B, H, W, Cp):
    """egne_reflect_pad_bwd, dense and phase-packed gradient; H = P + 1 is the smallest accepted size; 2 x 240 x 320 x 112 is more than
    16384 * 256 vectors (grid-stride loop).  MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(40 + H + P)
    gp = torch.randn(B, H + 2 * P, W + 2 * P, Cp, generator=g)
    pre = torch.randn(B, H, W, Cp, generator=g)
    src = R.phase_pack(gp) if phase else gp
    gs, go, xs, xo = src.shape[-1] + 8, 4, Cp + 4, 4
    gpb, gxb = _buf(src, gs, go), _buf(pre, xs, xo)
    g0 = gxb.clone()
    _lib.check(L.egne_reflect_pad_bwd(gpb.data_ptr(), gs, go, phase, Cp, gxb.data_ptr(), xs, xo, B, H, W, P, st))
    _sync()
    _check("reflect_pad_bwd", _slice(gxb, g0, xo, Cp), pre.double() + R.reflect_pad_bwd(gp.double(), P), pre + R.reflect_pad_bwd(gp, P))


@pytest.mark.parametrize("P,phase,B,H,W,Cp", [(1, 0, 2, 2, 2, 4), (3, 0, 2, 45, 70, 8), (1, 1, 2, 46, 70, 8)])
def test_reflect_pad_backward_bf16_twin(lib, P, phase, B, H, W, Cp):
    """egne_reflect_pad_bwd_bf16 on the inputs of test_reflect_pad_backward rounded to bf16 (slices at offset 4)."""
    _lib, L, st = lib
    g = _g(40 + H + P)
    gp = _q(torch.randn(B, H + 2 * P, W + 2 * P, Cp, generator=g))
    pre = _q(torch.randn(B, H, W, Cp, generator=g))
    src = R.phase_pack(gp) if phase else gp
    gs, go, xs, xo = src.shape[-1] + 8, 4, Cp + 4, 4
    outs = []
    for dt, fn in ((torch.float32, L.egne_reflect_pad_bwd), (BF, L.egne_reflect_pad_bwd_bf16)):
        gpb, gxb = _buf(src, gs, go, dt), _buf(pre, xs, xo, dt)
        g0 = gxb.clone()
        _lib.check(fn(gpb.data_ptr(), gs, go, phase, Cp, gxb.data_ptr(), xs, xo, B, H, W, P, st))
        _sync()
        outs.append(_slice(gxb, g0, xo, Cp))
    _twin("reflect_pad_bwd", outs[1], outs[0])


# ==== regression head and latent ======================================================================================================
@pytest.mark.parametrize("n", [1, 512, 600001])
def test_selu_and_backward(lib, n):
    """egne_selu_inplace / egne_selu_bwd (which differentiates from the OUTPUT) over [-20, 20] with an exact 0.
    MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(50 + n % 7)
    x = torch.linspace(-20, 20, n)[torch.randperm(n, generator=g)] if n > 1 else torch.zeros(1)
    x[n // 2] = 0.0
    gy = torch.randn(n, generator=g)
    xb = _poison((n + 8,))
    xb[:n] = x.to(DEV)
    gb = _poison((n + 8,))
    gb[:n] = gy.to(DEV)
    _lib.check(L.egne_selu_inplace(xb.data_ptr(), n, st))
    _lib.check(L.egne_selu_bwd(gb.data_ptr(), xb.data_ptr(), n, st))
    _sync()
    assert (xb[n:] == POISON).all() and (gb[n:] == POISON).all()
    _check("selu", xb[:n].cpu(), R.selu(x.double()), R.selu(x))
    (r64,) = R.vjp(R.selu, [x.double()], [gy.double()])
    (r32,) = R.vjp(R.selu, [x], [gy])
    _check("selu_bwd", gb[:n].cpu(), r64, r32)


@pytest.mark.parametrize("B", [1, 30])
def test_ellipse_head_act_and_backward(lib, B):
    """Columns 0-1 / 5-6 tanh, 2-3 / 7-8 sigmoid, 4 / 9 identity, 10..15 of an ld = 16 row untouched.  MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(60 + B)
    x, gy = 2 * torch.randn(B, 10, generator=g), torch.randn(B, 10, generator=g)
    xb, gb = _buf(x, 16, 0), _buf(gy, 16, 0)
    x0, g0 = xb.clone(), gb.clone()
    _lib.check(L.egne_ellipse_head_act(xb.data_ptr(), B, 16, st))
    _lib.check(L.egne_ellipse_head_act_bwd(gb.data_ptr(), xb.data_ptr(), B, 16, st))
    _sync()
    y = _slice(xb, x0, 0, 10)
    _check("ellipse_head_act", y, R.ellipse_head_act(x.double()), R.ellipse_head_act(x))
    assert torch.equal(y[:, 4], x[:, 4]) and torch.equal(y[:, 9], x[:, 9])
    (r64,) = R.vjp(R.ellipse_head_act, [x.double()], [gy.double()])
    (r32,) = R.vjp(R.ellipse_head_act, [x], [gy])
    gx = _slice(gb, g0, 0, 10)
    _check("ellipse_head_act_bwd", gx, r64, r32)
    assert torch.equal(gx[:, 4], gy[:, 4]) and torch.equal(gx[:, 9], gy[:, 9])


@pytest.mark.parametrize("kind", ["randn", "mean100"])
@pytest.mark.parametrize("HW", [1, 7, 300])
@pytest.mark.parametrize("Cn", [8, 38, 264])
def test_spatial_mean_and_backward(lib, Cn, HW, kind):
    """egne_spatial_mean / egne_spatial_mean_bwd; C = 264 is more channels than threads.  MI355X: not yet recorded."""
    _lib, L, st = lib
    B = 2
    g = _g(70 + Cn + HW)
    x = torch.randn(B, HW, Cn, generator=g)
    if kind == "mean100":
        x = 100.0 + 0.1 * x
    gm, pre = torch.randn(B, Cn, generator=g), torch.randn(B, HW, Cn, generator=g)
    xs, xo = Cn + 9, 5
    xb, out = _buf(x, xs, xo), _poison((B * Cn + 8,))
    _lib.check(L.egne_spatial_mean(xb.data_ptr(), xs, xo, Cn, B, HW, out.data_ptr(), st))
    gmb, gxb = _buf(gm, Cn + 3, 0), _buf(pre, xs, xo)
    g0 = gxb.clone()
    _lib.check(L.egne_spatial_mean_bwd(gmb.data_ptr(), Cn + 3, gxb.data_ptr(), xs, xo, Cn, B, HW, st))
    _sync()
    assert (out[B * Cn:] == POISON).all()
    _check("spatial_mean", out[:B * Cn].cpu().reshape(B, Cn), R.spatial_mean(x.double()), R.spatial_mean(x))
    (r64,) = R.vjp(R.spatial_mean, [x.double()], [gm.double()])
    (r32,) = R.vjp(R.spatial_mean, [x], [gm])
    _check("spatial_mean_bwd", _slice(gxb, g0, xo, Cn), pre.double() + r64, pre + r32)


@pytest.mark.parametrize("n", [1, 512])
def test_selu_bf16_twin(lib, n):
    """egne_selu_inplace_bf16 / egne_selu_bwd_bf16 on the inputs of test_selu_and_backward rounded to bf16; both backward kernels read
    the SAME bf16-representable output."""
    _lib, L, st = lib
    g = _g(50 + n % 7)
    x = torch.linspace(-20, 20, n)[torch.randperm(n, generator=g)] if n > 1 else torch.zeros(1)
    x[n // 2] = 0.0
    x, gy = _q(x), _q(torch.randn(n, generator=g))
    outs = []
    for dt, fw, bw in ((torch.float32, L.egne_selu_inplace, L.egne_selu_bwd), (BF, L.egne_selu_inplace_bf16, L.egne_selu_bwd_bf16)):
        xb = _poison((n + 8,), dt)
        xb[:n] = x.to(DEV).to(dt)
        _lib.check(fw(xb.data_ptr(), n, st))
        _sync()
        y = xb[:n].float().cpu()
        yin, gb = _poison((n + 8,), dt), _poison((n + 8,), dt)
        yin[:n] = _q(outs[0][0] if outs else y).to(DEV).to(dt)
        gb[:n] = gy.to(DEV).to(dt)
        _lib.check(bw(gb.data_ptr(), yin.data_ptr(), n, st))
        _sync()
        assert (xb[n:] == POISON).all() and (gb[n:] == POISON).all()
        outs.append((y, gb[:n].float().cpu()))
    _twin("selu", outs[1][0], outs[0][0])
    _twin("selu_bwd", outs[1][1], outs[0][1])


@pytest.mark.parametrize("B", [1, 30])
def test_ellipse_head_act_bf16_twin(lib, B):
    """egne_ellipse_head_act_bf16 / egne_ellipse_head_act_bwd_bf16 on the inputs of test_ellipse_head_act_and_backward rounded to bf16
    (ld = 16: columns 10 .. 15 untouched); both backward kernels read the SAME bf16-representable output."""
    _lib, L, st = lib
    g = _g(60 + B)
    x, gy = _q(2 * torch.randn(B, 10, generator=g)), _q(torch.randn(B, 10, generator=g))
    outs = []
    for dt, fw, bw in ((torch.float32, L.egne_ellipse_head_act, L.egne_ellipse_head_act_bwd),
                       (BF, L.egne_ellipse_head_act_bf16, L.egne_ellipse_head_act_bwd_bf16)):
        xb = _buf(x, 16, 0, dt)
        x0 = xb.clone()
        _lib.check(fw(xb.data_ptr(), B, 16, st))
        _sync()
        y = _slice(xb, x0, 0, 10)
        yin, gb = _buf(_q(outs[0][0] if outs else y), 16, 0, dt), _buf(gy, 16, 0, dt)
        g0 = gb.clone()
        _lib.check(bw(gb.data_ptr(), yin.data_ptr(), B, 16, st))
        _sync()
        outs.append((y, _slice(gb, g0, 0, 10)))
    _twin("ellipse_head_act", outs[1][0], outs[0][0])
    _twin("ellipse_head_act_bwd", outs[1][1], outs[0][1])
    assert torch.equal(outs[1][0][:, 4], x[:, 4]) and torch.equal(outs[1][1][:, 9], gy[:, 9])


@pytest.mark.parametrize("Cn,HW", [(8, 1), (38, 300)])
def test_spatial_mean_bf16_twin(lib, Cn, HW):
    """egne_spatial_mean_bf16 (bf16 in, bf16 out) / egne_spatial_mean_bwd_bf16 on the inputs of test_spatial_mean_and_backward rounded
    to bf16, slices at offset 5."""
    _lib, L, st = lib
    B = 2
    g = _g(70 + Cn + HW)
    x = _q(torch.randn(B, HW, Cn, generator=g))
    gm, pre = _q(torch.randn(B, Cn, generator=g)), _q(torch.randn(B, HW, Cn, generator=g))
    xs, xo = Cn + 9, 5
    outs = []
    for dt, fw, bw in ((torch.float32, L.egne_spatial_mean, L.egne_spatial_mean_bwd), (BF, L.egne_spatial_mean_bf16, L.egne_spatial_mean_bwd_bf16)):
        xb, out = _buf(x, xs, xo, dt), _poison((B * Cn + 8,), dt)
        _lib.check(fw(xb.data_ptr(), xs, xo, Cn, B, HW, out.data_ptr(), st))
        gmb, gxb = _buf(gm, Cn + 3, 0, dt), _buf(pre, xs, xo, dt)
        g0 = gxb.clone()
        _lib.check(bw(gmb.data_ptr(), Cn + 3, gxb.data_ptr(), xs, xo, Cn, B, HW, st))
        _sync()
        assert (out[B * Cn:] == POISON).all()
        outs.append((out[:B * Cn].float().cpu().reshape(B, Cn), _slice(gxb, g0, xo, Cn)))
    _twin("spatial_mean", outs[1][0], outs[0][0])
    _twin("spatial_mean_bwd", outs[1][1], outs[0][1])


# ==== resampling and layout ===========================================================================================================
@pytest.mark.parametrize("B,H,W,Cn", [(1, 1, 1, 8), (3, 15, 20, 40), (2, 120, 160, 64)])
def test_upsample2x_nearest_and_backward(lib, B, H, W, Cn):
    """Forward: exact copies.  Backward: (a + b) + (c + d) in fp32, bit for bit, then the pre-fill; 2 x 120 x 160 x 64 is more than
    2048 * 256 vectors (stride loop).  MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(80 + H)
    x, gy, pre = torch.randn(B, H, W, Cn, generator=g), torch.randn(B, 2 * H, 2 * W, Cn, generator=g), torch.randn(B, H, W, Cn, generator=g)
    xs, xo, ys, yo = Cn + 8, 4, Cn + 12, 8
    xb, yb = _buf(x, xs, xo), _poison((B, 2 * H, 2 * W, ys))
    y0 = yb.clone()
    _lib.check(L.egne_upsample2x_nearest(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, B, H, W, Cn, st))
    gyb, gxb = _buf(gy, ys, yo), _buf(pre, xs, xo)
    g0 = gxb.clone()
    _lib.check(L.egne_upsample2x_nearest_bwd(gyb.data_ptr(), ys, yo, gxb.data_ptr(), xs, xo, B, H, W, Cn, st))
    _sync()
    assert torch.equal(_slice(yb, y0, yo, Cn), R.upsample2x_nearest(x))
    gx = _slice(gxb, g0, xo, Cn)
    same = pre + ((gy[:, 0::2, 0::2] + gy[:, 0::2, 1::2]) + (gy[:, 1::2, 0::2] + gy[:, 1::2, 1::2]))
    assert torch.equal(gx, same), "nearest backward: (a + b) + (c + d), then the destination"
    _check("upsample2x_nearest_bwd", gx, pre.double() + R.upsample2x_nearest_bwd(gy.double()), same)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (15, 20), (120, 160)])
def test_upsample2x_backward_accumulating_and_storing(lib, H, W):
    """Transpose of the bilinear x2 up-sampling (border weights 1.0 at the first / last row and column).  MI355X: not yet recorded."""
    _lib, L, st = lib
    B, Cn = 2, 16
    g = _g(90 + H + W)
    gy, pre = torch.randn(B, 2 * H, 2 * W, Cn, generator=g), torch.randn(B, H, W, Cn, generator=g)
    r64, r32 = R.upsample2x_bwd(gy.double()), R.upsample2x_bwd(gy)
    gyb = _buf(gy, Cn + 8, 4)
    for name, fn, start in (("upsample2x_bwd", L.egne_upsample2x_bwd, pre), ("upsample2x_bwd_store", L.egne_upsample2x_bwd_store, None)):
        gxb = _buf(pre, Cn + 12, 8) if start is not None else _poison((B, H, W, Cn + 12))
        g0 = gxb.clone()
        _lib.check(fn(gyb.data_ptr(), Cn + 8, 4, gxb.data_ptr(), Cn + 12, 8, B, H, W, Cn, st))
        _sync()
        got = _slice(gxb, g0, 8, Cn)
        if start is not None:
            _check(name, got, pre.double() + r64, pre + r32)
        else:
            _check(name, got, r64, r32)


@pytest.mark.parametrize("B,H,W,Cn", [(1, 1, 1, 8), (3, 15, 20, 40)])
def test_upsample2x_nearest_bf16_twin(lib, B, H, W, Cn):
    """egne_upsample2x_nearest_bf16 (exact copies of the bf16 values) / egne_upsample2x_nearest_bwd_bf16 on the inputs of
    test_upsample2x_nearest_and_backward rounded to bf16, slices at offsets 4 and 8."""
    _lib, L, st = lib
    g = _g(80 + H)
    x, gy, pre = (_q(torch.randn(*shp, generator=g)) for shp in ((B, H, W, Cn), (B, 2 * H, 2 * W, Cn), (B, H, W, Cn)))
    xs, xo, ys, yo = Cn + 8, 4, Cn + 12, 8
    outs = []
    for dt, fw, bw in ((torch.float32, L.egne_upsample2x_nearest, L.egne_upsample2x_nearest_bwd),
                       (BF, L.egne_upsample2x_nearest_bf16, L.egne_upsample2x_nearest_bwd_bf16)):
        xb, yb = _buf(x, xs, xo, dt), _poison((B, 2 * H, 2 * W, ys), dt)
        y0 = yb.clone()
        _lib.check(fw(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, B, H, W, Cn, st))
        gyb, gxb = _buf(gy, ys, yo, dt), _buf(pre, xs, xo, dt)
        g0 = gxb.clone()
        _lib.check(bw(gyb.data_ptr(), ys, yo, gxb.data_ptr(), xs, xo, B, H, W, Cn, st))
        _sync()
        assert torch.equal(_slice(yb, y0, yo, Cn), R.upsample2x_nearest(x))
        outs.append(_slice(gxb, g0, xo, Cn))
    _twin("upsample2x_nearest_bwd", outs[1], outs[0])


@pytest.mark.parametrize("H,W", [(1, 1), (15, 20)])
def test_upsample2x_backward_store_bf16_twin(lib, H, W):
    """egne_upsample2x_bwd_store_bf16 on the inputs of test_upsample2x_backward_accumulating_and_storing rounded to bf16: POISON is
    overwritten; slices at offset 8 (the twin moves 16-byte vectors: it refuses the fp32 test's offset 4)."""
    _lib, L, st = lib
    B, Cn = 2, 16
    gy = _q(torch.randn(B, 2 * H, 2 * W, Cn, generator=_g(90 + H + W)))
    outs = []
    for dt, fn in ((torch.float32, L.egne_upsample2x_bwd_store), (BF, L.egne_upsample2x_bwd_store_bf16)):
        gyb, gxb = _buf(gy, Cn + 8, 8, dt), _poison((B, H, W, Cn + 16), dt)
        g0 = gxb.clone()
        if dt == BF:
            assert fn(gyb.data_ptr(), Cn + 8, 4, gxb.data_ptr(), Cn + 16, 8, B, H, W, Cn, st) != 0
        _lib.check(fn(gyb.data_ptr(), Cn + 8, 8, gxb.data_ptr(), Cn + 16, 8, B, H, W, Cn, st))
        _sync()
        outs.append(_slice(gxb, g0, 8, Cn))
    _twin("upsample2x_bwd_store", outs[1], outs[0])


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (30, 40)])
def test_avgpool2_backward(lib, H, W):
    """On odd sizes the last row / column of the destination keeps its pre-fill.  MI355X: not yet recorded."""
    _lib, L, st = lib
    B, Cn = 3, 12
    g = _g(100 + H)
    gq, pre = torch.randn(B, H // 2, W // 2, Cn, generator=g), torch.randn(B, H, W, Cn, generator=g)
    gqb, gxb = _buf(gq, Cn + 4, 4), _buf(pre, Cn + 8, 4)
    g0 = gxb.clone()
    _lib.check(L.egne_avgpool2_bwd(gqb.data_ptr(), Cn + 4, 4, gxb.data_ptr(), Cn + 8, 4, B, H, W, Cn, st))
    _sync()
    got = _slice(gxb, g0, 4, Cn)
    _check("avgpool2_bwd", got, pre.double() + R.avgpool2_bwd(gq.double(), H, W), pre + R.avgpool2_bwd(gq, H, W))
    if H % 2:
        assert torch.equal(got[:, H - 1], pre[:, H - 1])
    if W % 2:
        assert torch.equal(got[:, :, W - 1], pre[:, :, W - 1])


@pytest.mark.parametrize("stride", [2, 1])
@pytest.mark.parametrize("B,H,W,Cn", [(1, 25, 13, 8), (2, 30, 41, 24), (2, 2, 2, 8)])
def test_maxpool2_f16(lib, B, H, W, Cn, stride):
    """Exactly F.max_pool2d(ceil_mode=True) of the same f16 values: clipped windows at odd sizes, deliberate ties."""
    _lib, L, st = lib
    g = _g(110 + H)
    x = (torch.randn(B, H, W, Cn, generator=g) * 2).round() / 2          # few distinct levels: ties in most windows
    x[0, :, :, 0] = 1.5
    want = R.maxpool2(x, stride)
    Ho, Wo = want.shape[1:3]
    xb, yb = _buf(x, Cn + 16, 8, torch.float16), _poison((B, Ho, Wo, Cn + 8), torch.float16)
    y0 = yb.clone()
    _lib.check(L.egne_maxpool2_f16(xb.data_ptr(), Cn + 16, 8, yb.data_ptr(), Cn + 8, 8, B, H, W, Ho, Wo, stride, Cn, st))
    _sync()
    assert torch.equal(_slice(yb, y0, 8, Cn), want)


@pytest.mark.parametrize("yo", [0, 1])
@pytest.mark.parametrize("Cn", [1, 3])
def test_layout_kernels(lib, Cn, yo):
    """egne_nchw_to_nhwc (fp32 and bf16) into Cp = 8 channels at offset yo of a 16-wide buffer with the zero fill of C..Cp, the
    Cp = 1 form (one channel and nothing else, esf_engine.py:236), egne_nhwc_to_nchw back: all exact."""
    _lib, L, st = lib
    B, H, W = 3, 17, 23
    x = torch.randn(B, Cn, H, W, generator=_g(120 + Cn))
    xd = x.to(DEV)
    nhwc = x.permute(0, 2, 3, 1)
    for dt, fn in ((torch.float32, L.egne_nchw_to_nhwc), (BF, L.egne_nchw_to_nhwc_bf16)):
        yb = _poison((B, H, W, 16), dt)
        y0 = yb.clone()
        _lib.check(fn(xd.data_ptr(), B, Cn, H, W, yb.data_ptr(), 16, yo, 8, st))
        _sync()
        got = _slice(yb, y0, yo, 8)
        assert torch.equal(got[..., :Cn], nhwc.to(dt).float()) and (got[..., Cn:] == 0).all()
        if dt == torch.float32:
            back = _poison((B * Cn * H * W + 8,))
            _lib.check(L.egne_nhwc_to_nchw(yb.data_ptr(), 16, yo, B, Cn, H, W, back.data_ptr(), st))
            _sync()
            assert torch.equal(back[:-8].cpu().reshape(B, Cn, H, W), x) and (back[-8:] == POISON).all()
    if Cn == 1:
        yb = _poison((B, H, W, 8))
        y0 = yb.clone()
        _lib.check(L.egne_nchw_to_nhwc(xd.data_ptr(), B, 1, H, W, yb.data_ptr(), 8, 1 + yo, 1, st))
        _sync()
        assert torch.equal(_slice(yb, y0, 1 + yo, 1), nhwc)


@pytest.mark.parametrize("npix,Cn", [(1, 4), (301, 12), (2 * 120 * 160, 64)])
def test_affine_act_and_inplace(lib, npix, Cn):
    """relu(x * a + b) per channel of a padded slice at a channel offset (fp32 rule: torch's fp32 error x 4).
    MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(130 + Cn)
    x = torch.randn(npix, Cn, generator=g)
    a, b = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    xb, yb = _buf(x, Cn + 8, 4), _poison((npix, Cn + 12))
    y0, x0 = yb.clone(), xb.clone()
    _lib.check(L.egne_affine_act(xb.data_ptr(), Cn + 8, 4, yb.data_ptr(), Cn + 12, 8, Cn, npix, ad.data_ptr(), bd.data_ptr(), 1, st))
    _sync()
    _check("affine_act", _slice(yb, y0, 8, Cn), R.affine_act(x.double(), a.double(), b.double()), R.affine_act(x, a, b))
    _lib.check(L.egne_affine_inplace(xb.data_ptr(), Cn + 8, 4, Cn, npix, ad.data_ptr(), bd.data_ptr(), st))
    _sync()
    _check("affine_inplace", _slice(xb, x0, 4, Cn), R.affine_act(x.double(), a.double(), b.double(), False), R.affine_act(x, a, b, False))


# ==== losses ==========================================================================================================================
def _loss_inputs(B, H, W, absent, seed):
    """The inputs of test_loss_head_vs_oracle: sample 1 has no pupil pixel (one class missing), masks absent none / some / all."""
    g = _g(seed)
    op = _q(2 * torch.randn(B, 3, H, W, generator=g))             # bf16-representable logits: the bf16 entry reads the same values
    tgt = torch.randint(0, 3, (B, H, W), generator=g)
    tgt[1][tgt[1] == 2] = 1
    sw = 1 + 20 * (torch.rand(B, H, W, generator=g) > 0.9).float()
    dist = torch.randn(B, 3, H, W, generator=g)
    pc = torch.rand(B, 2, generator=g) * torch.tensor([W, H])
    eln = torch.rand(B, 2, 5, generator=g) * 2 - 1
    elOut = torch.rand(B, 10, generator=g) * 2 - 1
    cond = torch.zeros(B, 4)
    if absent == "some":
        cond[min(2, B - 1), 1:] = 1
        cond[B - 1, 1:] = 1
    elif absent == "all":
        cond[:, 1:] = 1
    ups = (torch.randn(B, 3, H, W, generator=g) * 1e-4, torch.randn(B, 2, 2, generator=g), torch.randn(B, 10, generator=g))
    return dict(op=op, tgt=tgt, sw=sw, dist=dist, pc=pc, eln=eln, elOut=elOut, cond=cond), ups


LOSS_SHAPES = [(5, 48, 64, "none"), (3, 240, 320, "some"), (4, 30, 40, "all")]
LOSS_CASES = [(B, H, W, ab, al, up) for (B, H, W, ab) in LOSS_SHAPES for al in (0.0, 0.3, 1.0) for up in ("none", "all")]
LOSS_CASES += [(B, H, W, "all", al, "pred_c") for (B, H, W, _) in LOSS_SHAPES for al in (0.3,)]
LOSS_CASES += [(5, 48, 64, "some", 0.3, "pred_c"), (4, 30, 40, "none", 0.3, "all"), (4, 30, 40, "some", 1.0, "all")]


@pytest.mark.parametrize("B,H,W,absent,alpha,upstream", LOSS_CASES)
def test_loss_head_backward(lib, B, H, W, absent, alpha, upstream):
    """egne_loss_bwd (fp32 entry, and the bf16 entry as its twin) after egne_loss_fwd with coef set, against autograd of
    gscale * total + <g_op, op> + <g_pred_c, pred_c> + <g_elOut_up, elOut> through oracle.losses.all_loss in float64.
    upstream = "pred_c" with no mask in the batch: the iris row of g_pred_c belongs to elOut[:, 5:7], not to the logits.
    MI355X: not yet recorded."""
    _lib, L, st = lib
    t, ups = _loss_inputs(B, H, W, absent, 7 * B + H)
    gscale = 0.7
    g_op, g_pc, g_el = {"none": (None, None, None), "all": ups, "pred_c": (None, ups[1], None)}[upstream]
    # keep every L1 / sign term away from its kink
    _, pred_c, _ = R.loss_head(t["op"].double(), t["elOut"].double(), t["tgt"], t["pc"].double(), t["eln"].double(), t["sw"].double(),
                               t["dist"].double(), t["cond"].double(), alpha)
    from oracle import losses as olosses
    pcn = olosses.norm_pts(t["pc"].double(), H, W)
    ties = [(pred_c[:, 1] - pcn).abs().min().item(), (t["elOut"] - t["eln"].reshape(B, 10)).abs().min().item(),
            (t["elOut"][:, 5:7].double() - pcn).abs().min().item()]
    if absent != "all":
        ties.append((pred_c[:, 0] - t["eln"][:, 0, :2].double()).abs().min().item())
    assert min(ties) > 1e-5, "an L1 term sits on its kink (%.2e): choose another seed" % min(ties)

    dbl = lambda v: None if v is None else v.double()  # noqa: E731
    r64 = R.loss_head_bwd(t["op"].double(), t["elOut"].double(), t["tgt"], t["pc"].double(), t["eln"].double(), t["sw"].double(),
                          t["dist"].double(), t["cond"].double(), alpha, gscale, dbl(g_op), dbl(g_pc), dbl(g_el))
    r32 = R.loss_head_bwd(t["op"], t["elOut"], t["tgt"], t["pc"], t["eln"], t["sw"], t["dist"], t["cond"], alpha, gscale, g_op, g_pc, g_el)

    dv = {k: v.to(DEV).contiguous() for k, v in t.items()}
    keep = [None if v is None else v.to(DEV).contiguous() for v in (g_op, g_pc, g_el)]
    gx, gy = torch.linspace(-1, 1, W).to(DEV), torch.linspace(-1, 1, H).to(DEV)
    gsc = torch.tensor([gscale], device=DEV)
    outs = {}
    for dt in (torch.float32, BF):
        logits = _buf(t["op"].permute(0, 2, 3, 1), 8, 2, dt)
        part = torch.zeros(int(L.egne_loss_workspace_floats(B, H, W)), device=DEV)
        out_terms, pcd, elp = torch.zeros(8, device=DEV), torch.zeros(B, 2, 2, device=DEV), torch.zeros(B, 10, device=DEV)
        coef = torch.zeros(B, 32, device=DEV)
        d = _lib.LossDesc()
        d.B, d.H, d.W = B, H, W
        d.logits, d.pix_stride, d.ch_off, d.dtype = logits.data_ptr(), 8, 2, (0 if dt == torch.float32 else 1)
        d.target, d.spatWts, d.distMap, d.cond = dv["tgt"].data_ptr(), dv["sw"].data_ptr(), dv["dist"].data_ptr(), dv["cond"].data_ptr()
        d.pupil_center, d.elNorm, d.elOut, d.alpha = dv["pc"].data_ptr(), dv["eln"].data_ptr(), dv["elOut"].data_ptr(), alpha
        d.grid_x, d.grid_y = gx.data_ptr(), gy.data_ptr()
        d.partials, d.out_terms, d.pred_c, d.elPred = part.data_ptr(), out_terms.data_ptr(), pcd.data_ptr(), elp.data_ptr()
        d.coef = coef.data_ptr()
        _lib.check(L.egne_loss_fwd(C.byref(d), st), "loss")
        d.g_op_nchw, d.g_pred_c, d.g_elOut_up = [None if k is None else k.data_ptr() for k in keep]
        bwd = L.egne_loss_bwd if dt == torch.float32 else L.egne_loss_bwd_bf16
        res = []
        for gs, go in ((8, 0), (16, 5)):
            gl, ge = _poison((B, H, W, gs), dt), _poison((B * 10 + 6,))
            gl0 = gl.clone()
            _lib.check(bwd(C.byref(d), gsc.data_ptr(), gl.data_ptr(), gs, go, ge.data_ptr(), st), "loss_bwd")
            _sync()
            assert (ge[B * 10:] == POISON).all()
            res.append((_slice(gl, gl0, go, 3).permute(0, 3, 1, 2), ge[:B * 10].cpu().reshape(B, 10)))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "the gradient must not depend on its slice"
        outs[dt] = res[0]
    tag = "loss_bwd[%dx%dx%d %s alpha %.1f up %s]" % (B, H, W, absent, alpha, upstream)
    _check(tag + " g_logits", outs[torch.float32][0], r64[0], r32[0])
    _check(tag + " g_elOut", outs[torch.float32][1], r64[1], r32[1])
    _twin(tag + " g_logits", outs[BF][0], outs[torch.float32][0])
    assert torch.equal(outs[BF][1], outs[torch.float32][1]), "g_elOut is fp32 in both entries"


@pytest.mark.parametrize("absent", ["none", "some", "all"])
@pytest.mark.parametrize("B,H,W", [(2, 240, 320), (3, 37, 53), (300, 8, 12)])
def test_deepvog_loss_and_backward(lib, B, H, W, absent):
    """egne_deepvog_loss_fwd / _bwd against oracle.deepvog.deepvog_loss and its autograd; B = 300 is more frames than the combining
    block has threads.  MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(200 + B)
    op = 2 * torch.randn(B, 2, H, W, generator=g)
    tgt = torch.randint(0, 3, (B, H, W), generator=g)
    pc = torch.rand(B, 2, generator=g) * torch.tensor([W, H])
    cond = torch.zeros(B, 4)
    if absent == "some":
        cond[::2, 1] = 1
    elif absent == "all":
        cond[:, 1] = 1
    gscale = 1.3
    loss64, pc64, tm64 = R.deepvog_loss(op.double(), tgt, pc.double(), cond.double())
    loss32, pc32, tm32 = R.deepvog_loss(op, tgt, pc, cond)
    from oracle import losses as olosses
    tie = (pc64 - olosses.norm_pts(pc.double(), H, W)).abs().min().item()
    assert tie > 1e-5, "an L1 term sits on its kink (%.2e): choose another seed" % tie
    logits = _buf(op.permute(0, 2, 3, 1), 8, 3)
    tg, pcd, cd = tgt.to(DEV), pc.to(DEV), cond.to(DEV)
    part = torch.zeros(int(L.egne_deepvog_loss_workspace_floats(B, H, W)), device=DEV)
    terms, prd = _poison((8,)), _poison((B * 2 + 4,))
    opn, mask = _poison((B, 2, H, W)), torch.full((B, H, W), 7, dtype=torch.int64, device=DEV)
    _lib.check(L.egne_deepvog_loss_fwd(logits.data_ptr(), 8, 3, tg.data_ptr(), pcd.data_ptr(), cd.data_ptr(), B, H, W, part.data_ptr(),
                                       terms.data_ptr(), prd.data_ptr(), opn.data_ptr(), mask.data_ptr(), st))
    gsc = torch.tensor([gscale], device=DEV)
    gl = _poison((B, H, W, 8))
    gl0 = gl.clone()
    _lib.check(L.egne_deepvog_loss_bwd(logits.data_ptr(), 8, 3, tg.data_ptr(), pcd.data_ptr(), cd.data_ptr(), B, H, W, part.data_ptr(),
                                       prd.data_ptr(), gsc.data_ptr(), gl.data_ptr(), 8, 5, st))
    _sync()
    t = terms.cpu()
    assert (t[3:] == POISON).all() and (prd[B * 2:] == POISON).all()
    as1 = lambda v: torch.as_tensor(v).reshape(1)  # noqa: E731
    _check("deepvog loss", t[0:1], as1(loss64), as1(loss32))
    if absent != "all":
        _check("deepvog l_seg", t[1:2], as1(tm64["l_seg"]), as1(tm32["l_seg"]))
    else:
        assert t[1].item() == 0.0
    _check("deepvog l_pt", t[2:3], as1(tm64["l_pt"]), as1(tm32["l_pt"]))
    _check("deepvog pred_c", prd[:B * 2].cpu().reshape(B, 2), pc64, pc32)
    assert torch.equal(mask.cpu(), op.max(1)[1]), "argmax mask must be identical (first maximum on ties)"
    assert torch.equal(opn.cpu(), op)
    _check("deepvog_loss_bwd", _slice(gl, gl0, 5, 2).permute(0, 3, 1, 2), R.deepvog_loss_bwd(op.double(), tgt, pc.double(), cond.double(), gscale),
           R.deepvog_loss_bwd(op, tgt, pc, cond, gscale))


# ==== BDCN side-output path ===========================================================================================================
@pytest.mark.parametrize("stride", [32, 64])
@pytest.mark.parametrize("npix", [1, 31, 33, 100 * 100])
@pytest.mark.parametrize("nblk", [2, 3])
def test_bdcn_stage_scores(lib, nblk, npix, stride):
    """The 1x1 down convolutions of a stage's MSBlocks summed, then the two score heads.  MI355X: not yet recorded."""
    _lib, L, st = lib
    g = _g(300 + nblk + npix % 5)
    ms = [torch.randn(npix, 32, generator=g) for _ in range(nblk)]
    wd, bd = torch.randn(nblk, 21, 32, generator=g) * 0.2, torch.randn(nblk, 21, generator=g)
    ws, ws1 = torch.randn(21, generator=g) * 0.3, torch.randn(21, generator=g) * 0.3
    bs, bs1 = torch.randn(1, generator=g), torch.randn(1, generator=g)
    mb = [_buf(m, stride, 0) for m in ms]
    arr = (C.c_void_p * nblk)(*[m.data_ptr() for m in mb])
    dev = [v.to(DEV).contiguous() for v in (wd, bd, ws, bs, ws1, bs1)]
    s, s1 = _poison((npix + 8,)), _poison((npix + 8,))
    _lib.check(L.egne_bdcn_stage_scores(arr, nblk, stride, npix, *[v.data_ptr() for v in dev], s.data_ptr(), s1.data_ptr(), st))
    _sync()
    assert (s[npix:] == POISON).all() and (s1[npix:] == POISON).all()
    r64 = R.bdcn_stage_scores([m.double() for m in ms], wd.double(), bd.double(), ws.double(), bs.double(), ws1.double(), bs1.double())
    r32 = R.bdcn_stage_scores(ms, wd, bd, ws, bs, ws1, bs1)
    _check("stage_scores s", s[:npix].cpu(), r64[0], r32[0])
    _check("stage_scores s1", s1[:npix].cpu(), r64[1], r32[1])


@pytest.mark.parametrize("edge_thres", [0, 1])
@pytest.mark.parametrize("B,H,W", [(1, 100, 100), (2, 37, 53), (2, 240, 320), (3, 9, 65)])
def test_bdcn_tail(lib, B, H, W, edge_thres):
    """Transposed-conv sampling, crop, the two cascades, fuse, sigmoid and the edge_thres switch, on seeded score maps of magnitude 3
    at the plan's stage sizes; all eleven outputs, then a call with only out[10].  With edge_thres = 1 the pixels whose float64 fused
    map lies within the bound of 0.1 may land on either side: they are excluded and counted (< 0.1 % of the frame).
    MI355X: not yet recorded."""
    _lib, L, st = lib
    s_a, s_b, ups, strides, crops, fw, fb = R.bdcn_tail_inputs(B, H, W, seed=7)
    dbl = lambda ts: [None if t is None else t.double() for t in ts]  # noqa: E731
    r64, _ = R.bdcn_tail(dbl(s_a), dbl(s_b), dbl(ups), strides, crops, fw.double(), fb.double(), H, W, 0)
    r32, _ = R.bdcn_tail(s_a, s_b, ups, strides, crops, fw, fb, H, W, 0)
    keep = [[t.to(DEV).contiguous() for t in s_a], [t.to(DEV).contiguous() for t in s_b], [None if u is None else u.to(DEV).contiguous() for u in ups],
            fw.to(DEV), fb.to(DEV)]
    for only_fuse in (False, True):
        outs = _poison((11, B * H * W + 8))
        d = _lib.BdcnTailDesc()
        d.B, d.H, d.W = B, H, W
        for k in range(5):
            d.s[k], d.s1[k] = keep[0][k].data_ptr(), keep[1][k].data_ptr()
            d.h[k], d.w[k] = s_a[k].shape[-2:]
            d.stride[k], d.crop[k] = strides[k], crops[k]
            d.up[k] = None if keep[2][k] is None else keep[2][k].data_ptr()
        d.fuse_w, d.fuse_b, d.edge_thres = keep[3].data_ptr(), keep[4].data_ptr(), edge_thres
        for k in range(11):
            d.out[k] = outs[k].data_ptr() if (k == 10 or not only_fuse) else None
        _lib.check(L.egne_bdcn_tail(C.byref(d), st), "tail")
        _sync()
        o = outs.cpu()
        assert (o[:, B * H * W:] == POISON).all()
        if only_fuse:
            assert (o[:10] == POISON).all(), "an output that is not asked for must not be written"
        else:
            for k in range(10):
                _check("bdcn_tail out[%d]" % k, o[k, :B * H * W].reshape(B, 1, H, W), r64[k], r32[k])
        e = o[10, :B * H * W].reshape(B, 1, H, W)
        bnd, e32 = R.bound(r64[10], r32[10])
        if edge_thres == 0:
            _check("bdcn_tail fused", e, r64[10], r32[10])
        else:
            lim = bnd * r64[10].abs().max().item()
            near = (r64[10] - 0.1).abs() <= lim
            n_near = int(near.sum())
            print("bdcn_tail edge_thres: %d of %d pixels within %.2e of the switch" % (n_near, near.numel(), lim))
            assert n_near < 1e-3 * near.numel()
            want = torch.where(r64[10] >= 0.1, torch.ones_like(r64[10]), r64[10])
            err = ((e.double() - want).abs() * (~near)).max().item()
            print("bdcn_tail fused (thresholded): err %.3e (bound %.3e)" % (err / r64[10].abs().max().item(), bnd))
            assert err <= lim
            assert (e[(want == 1) & ~near] == 1).all()
