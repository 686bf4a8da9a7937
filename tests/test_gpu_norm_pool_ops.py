"""-m gpu: the kernels that normalise, pool and resample (csrc/elementwise.hip, csrc/backward.hip), one C-ABI call at a time, against
the float64 references of tests/small_op_refs.py (pinned by tests/test_host_small_op_refs.py).

Conventions as in tests/test_gpu_small_ops.py, whose helpers are used here: seeded CPU inputs; every tensor output is a channel slice
at a non-zero offset of a wider buffer whose other elements hold POISON and must come back untouched (tables such as scale / shift
[B][Cp] have no slice: they are followed by POISON); accumulating forms start from a seeded non-zero destination, storing forms
overwrite POISON.

Tolerances: an fp32 kernel's error against float64 stays within small_op_refs.bound -- four times the error of the same operation
done in fp32 by torch on the CPU, floor 4 ulp, both printed.  Copies and maxima are compared bit for bit.  A bf16 twin on
bf16-representable inputs agrees with the fp32 kernel to one bf16 rounding of a tensor output (_twin) and to 1e-6 of the largest
element of an output that is fp32 on both sides (statistics, bias and parameter sums).

The shapes are the smallest that reach every branch of the index arithmetic: one pixel, one more / one less than a 256-pixel chunk,
a second partial 32-channel group (Cp = 40), chunk counts whose last chunk is ragged or empty (76801 pixels: 300 chunks of 257, the
last one empty; 262147 pixels: the 1024-chunk cap), and one case per kernel above grid_for's 2048-block cap (the grid-stride loop).

Measured errors (MI355X, the largest over a test's cases, relative to the output's largest element) are listed in the docstrings of
the tests; nothing measured here exceeds 0.27 of its bound."""
import pytest
import torch

import small_op_refs as R
from test_gpu_small_ops import BF, DEV, D, POISON, _buf, _check, _g, _poison, _q, _slice, _sync, _twin
from test_gpu_small_ops import _same32 as _same
from test_gpu_small_ops import lib  # noqa: F401  (module-scoped fixture: the loaded library, its ctypes handle, the stream)

pytestmark = pytest.mark.gpu

F32 = torch.float32
ULP32 = R.ULP32
INF_BITS = 0x7F800000


def _ws(nbytes):
    """A 16-byte aligned workspace of at least ``nbytes`` bytes, as doubles."""
    return torch.zeros(int(nbytes) // 8 + 2, dtype=D, device=DEV)


def _table(n):
    """n floats for a table output, followed by 8 that must stay POISON."""
    return _poison((n + 8,))


def _table_out(t, n, shape):
    assert (t[n:] == POISON).all(), "the kernel wrote behind its table"
    return t[:n].cpu().reshape(shape)


def _bits(v):
    """Bit pattern of a non-negative fp32 value."""
    return int(torch.tensor([v], dtype=F32).view(torch.int32).item())


def _word(start):
    return torch.tensor([start], dtype=torch.int32, device=DEV)


def _word_out(w):
    return int(w.cpu().item()) & 0xFFFFFFFF


# ==== statistics ======================================================================================================================
def _stats_input(kind, B, HW, Cn, seed):
    z = torch.randn(B, HW, Cn, generator=_g(seed))
    return {"randn": z * 3 + 0.5, "mean100": 100.0 + z, "const": torch.full_like(z, 3.0), "tight": 60.0 + 1e-3 * z}[kind]


def _run_stats(lib, x, per_sample, dt, off, moments):
    _lib, L, st = lib
    B, HW, Cp = x.shape
    Bn, stride = (B if per_sample else 1), Cp + 16
    xb = _buf(x, stride, off, dt)
    outs = [_table(Bn * Cp) for _ in range(4)]
    ws = _ws(L.egne_norm_stats_workspace_bytes(B, HW, Cp, per_sample))
    fn = L.egne_norm_stats if dt == F32 else L.egne_norm_stats_bf16
    mo = [o.data_ptr() if moments else None for o in outs[2:]]
    _lib.check(fn(xb.data_ptr(), stride, off, Cp, B, HW, per_sample, 1e-5, outs[0].data_ptr(), outs[1].data_ptr(), mo[0], mo[1],
                  ws.data_ptr(), st))
    _sync()
    if not moments:
        assert (outs[2] == POISON).all() and (outs[3] == POISON).all()
    return [_table_out(o, Bn * Cp, (Bn, Cp)) for o in outs[:4 if moments else 2]]


STATS_CASES = [(1, 2, hw, cp) for hw in (1, 2, 255, 257, 1200) for cp in (8, 40, 64)]
STATS_CASES += [(1, 1, 76801, 8),           # 300 chunks of 257 pixels: chunk 298 is ragged, chunk 299 empty
                (1, 1, 262147, 8),          # the 1024-chunk cap: 257 pixels each, chunk 1020 ragged, 1021 .. 1023 empty
                (0, 3, 300, 8), (0, 3, 300, 40), (0, 3, 300, 64)]


@pytest.mark.parametrize("kind", ["randn", "mean100", "const", "tight"])
@pytest.mark.parametrize("per_sample,B,HW,Cp", STATS_CASES)
def test_norm_stats(lib, per_sample, B, HW, Cp, kind):
    """egne_norm_stats and egne_norm_stats_bf16: scale = rstd, shift = -mean rstd (and mean / biased variance of the batch form).
    Inputs: 3 N(0,1) + 0.5, mean 100 / std 1, the constant 3, mean 60 / std 1e-3 (the sum of squares must be formed in double).
    MI355X, largest over the cases: scale 1.4e-7, shift 1.7e-7, mean 4.4e-8, variance 1.3e-6 (mean 60 / std 1e-3, where fp32 torch
    is 5e-5 off); never above 0.22 of the bound.  The twins' statistics are bit-equal to the fp32 kernel's."""
    x = _stats_input(kind, B, HW, Cp, 1000 * per_sample + HW + Cp)
    moments = not per_sample
    got = _run_stats(lib, x, per_sample, F32, 4, moments)
    r64, r32 = R.norm_stats(x.double(), per_sample), R.norm_stats(x, per_sample)
    tag = "norm_stats[ps%d B%d HW%d Cp%d %s]" % (per_sample, B, HW, Cp, kind)
    for k, name in enumerate(("scale", "shift", "mean", "var")[:len(got)]):
        _check("%s %s" % (tag, name), got[k], r64[k], r32[k])
    xq = _q(x)
    g32, g16 = _run_stats(lib, xq, per_sample, F32, 8, moments), _run_stats(lib, xq, per_sample, BF, 8, moments)
    for k, name in enumerate(("scale", "shift", "mean", "var")[:len(g32)]):
        _same("%s %s" % (tag, name), g16[k], g32[k])


def _partials(x, nchunk):
    """[B, HW, Cp] fp32 -> ([B, nchunk, Cp, 2] float64 (sum x, sum x^2) of nchunk runs of pixels, the last one shorter."""
    B, HW, Cp = x.shape
    per = -(-HW // nchunk)
    xd = torch.zeros(B, nchunk * per, Cp, dtype=D)
    xd[:, :HW] = x.double()
    xd = xd.reshape(B, nchunk, per, Cp)
    return torch.stack([xd.sum(2), (xd * xd).sum(2)], -1).contiguous()


def _finish_case(kind, B, nchunk, Cp):
    HW = max(3 * nchunk - 1, 2)
    x = _stats_input(kind, B, HW, Cp, 7 * nchunk + Cp + B)
    return x, HW, _partials(x, nchunk)


@pytest.mark.parametrize("kind", ["randn", "mean100"])
@pytest.mark.parametrize("Cp", [8, 40])
@pytest.mark.parametrize("nchunk", [1, 31, 33])
def test_norm_stats_finish(lib, nchunk, Cp, kind):
    """egne_norm_stats_finish on synthetic float64 partial sums ([B][nchunk][Cp][2]; 32 streams per channel: 31 and 33 chunks leave a
    stream empty / give one a second element).  MI355X: scale 5.1e-8, shift 9.9e-8."""
    _lib, L, st = lib
    B = 2
    x, HW, parts = _finish_case(kind, B, nchunk, Cp)
    ws = parts.to(DEV)
    sc, sh = _table(B * Cp), _table(B * Cp)
    _lib.check(L.egne_norm_stats_finish(ws.data_ptr(), Cp, B, nchunk, HW, 1e-5, sc.data_ptr(), sh.data_ptr(), st))
    _sync()
    assert torch.equal(ws.cpu(), parts), "the ungrouped finish must not write its workspace"
    r64, r32 = R.stats_finish(parts, HW), R.norm_stats(x, 1)
    tag = "norm_stats_finish[nchunk %d Cp%d %s]" % (nchunk, Cp, kind)
    _check(tag + " scale", _table_out(sc, B * Cp, (B, Cp)), r64[0], r32[0])
    _check(tag + " shift", _table_out(sh, B * Cp, (B, Cp)), r64[1], r32[1])


@pytest.mark.parametrize("kind", ["randn", "mean100"])
@pytest.mark.parametrize("Cp", [8, 40])
@pytest.mark.parametrize("B,nchunk", [(2, 1), (2, 31), (2, 33), (2, 1024),      # no grouping
                                      (1, 1025),                                # groups of 256 rows, the fifth holds one row
                                      (2, 1280)])                               # five whole groups per sample
def test_norm_stats_finish_moments(lib, B, nchunk, Cp, kind):
    """egne_norm_stats_finish_moments; above 1024 rows per sample the rows are first summed in groups of 256 IN the workspace (the
    call gets a copy).  MI355X: scale 5.8e-8, shift 1.2e-7, mean 5.1e-8, variance 5.7e-8."""
    _lib, L, st = lib
    x, HW, parts = _finish_case(kind, B, nchunk, Cp)
    ws = parts.to(DEV).clone()
    outs = [_table(B * Cp) for _ in range(4)]
    _lib.check(L.egne_norm_stats_finish_moments(ws.data_ptr(), Cp, B, nchunk, HW, 1e-5, *[o.data_ptr() for o in outs], st))
    _sync()
    r64, r32 = R.stats_finish(parts, HW), R.norm_stats(x, 1)
    tag = "norm_stats_finish_moments[B%d nchunk %d Cp%d %s]" % (B, nchunk, Cp, kind)
    for k, name in enumerate(("scale", "shift", "mean", "var")):
        _check("%s %s" % (tag, name), _table_out(outs[k], B * Cp, (B, Cp)), r64[k], r32[k])


def test_norm_stats_finish_moments_refuses_ragged_groups_of_several_samples(lib):
    """1025 rows per sample and two samples: the grouped rows of sample 1 would not start on a group boundary."""
    _lib, L, st = lib
    ws = torch.zeros(2 * 1025 * 8 * 2, dtype=D, device=DEV)
    outs = [_table(16) for _ in range(4)]
    rc = L.egne_norm_stats_finish_moments(ws.data_ptr(), 8, 2, 1025, 3074, 1e-5, *[o.data_ptr() for o in outs], st)
    _sync()
    assert rc != 0 and b"1025" in L.egne_last_error(), L.egne_last_error()
    assert all((o == POISON).all() for o in outs) and (ws == 0).all()


# ==== affine ==========================================================================================================================
AFFINE_CASES = [(1, 8), (1, 40), (300, 8), (300, 40), (70000, 32)]      # 70000 x 8 vectors > 2048 x 256: the grid-stride loop runs


@pytest.mark.parametrize("form", ["affine", "inplace", "act0", "act1", "act2", "bf16"])
@pytest.mark.parametrize("npix,Cp", AFFINE_CASES)
def test_affine_forms(lib, npix, Cp, form):
    """egne_affine, egne_affine_inplace, egne_affine_act (none / ReLU / leaky) and egne_affine_bf16: y = act(x scale[c] + shift[c]).
    MI355X: 4.1e-8 in every form (fp32 torch 6e-8 .. 8e-8); the twin within 0.72 of one bf16 rounding."""
    _lib, L, st = lib
    g = _g(npix + Cp)
    x = torch.randn(npix, Cp, generator=g) * 2
    a, b = torch.rand(Cp, generator=g) + 0.5, torch.randn(Cp, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    xs, xo, ys, yo = Cp + 8, 4, Cp + 12, 8
    tag = "%s[npix %d Cp%d]" % (form, npix, Cp)
    if form == "bf16":
        x = _q(x)
        outs = []
        for dt, fn in ((F32, L.egne_affine), (BF, L.egne_affine_bf16)):
            xb, yb = _buf(x, xs, xo, dt), _poison((npix, ys), dt)
            y0 = yb.clone()
            _lib.check(fn(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, Cp, npix, ad.data_ptr(), bd.data_ptr(), st))
            _sync()
            outs.append(_slice(yb, y0, yo, Cp))
        _twin(tag, outs[1], outs[0])
        return
    kind = int(form[3]) if form.startswith("act") else 0
    xb = _buf(x, xs, xo)
    if form == "inplace":
        x0 = xb.clone()
        _lib.check(L.egne_affine_inplace(xb.data_ptr(), xs, xo, Cp, npix, ad.data_ptr(), bd.data_ptr(), st))
        _sync()
        got = _slice(xb, x0, xo, Cp)
    else:
        yb = _poison((npix, ys))
        y0 = yb.clone()
        if form == "affine":
            _lib.check(L.egne_affine(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, Cp, npix, ad.data_ptr(), bd.data_ptr(), st))
        else:
            _lib.check(L.egne_affine_act(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, Cp, npix, ad.data_ptr(), bd.data_ptr(), kind, st))
        _sync()
        got = _slice(yb, y0, yo, Cp)
    _check(tag, got, R.affine_act(x.double(), a.double(), b.double(), kind=kind), R.affine_act(x, a, b, kind=kind))


# ==== pooling =========================================================================================================================
POOL_CASES = [(1, 2, 2, 8), (2, 5, 7, 40), (3, 30, 40, 40),
              (2, 240, 320, 64)]            # 2 x 120 x 160 x 16 vectors > 2048 x 256: the grid-stride loop runs


def _run_pool(lib, x, sc, sh, op, dt, xo, yo):
    """op = "avg" or an activation code (egne_norm_act_pool2).  The output buffer is followed by as many POISON elements as a
    ceil-sized output would have on top of the floor-sized one."""
    _lib, L, st = lib
    B, H, W, Cp = x.shape
    Ho, Wo = H // 2, W // 2
    xs, ys = Cp + 16, Cp + 24
    xb = _buf(x, xs, xo, dt)
    n = B * Ho * Wo * ys
    flat = _poison((n + (B * ((H + 1) // 2) * ((W + 1) // 2) * ys - n) + 64,), dt)
    f0 = flat.clone()
    if op == "avg":
        fn = L.egne_avgpool2 if dt == F32 else L.egne_avgpool2_bf16
        _lib.check(fn(xb.data_ptr(), xs, xo, flat.data_ptr(), ys, yo, B, H, W, Cp, st))
    else:
        fn = L.egne_norm_act_pool2 if dt == F32 else L.egne_norm_act_pool2_bf16
        _lib.check(fn(xb.data_ptr(), xs, xo, sc.data_ptr(), sh.data_ptr(), op, flat.data_ptr(), ys, yo, B, H, W, Cp, st))
    _sync()
    assert torch.equal(flat[n:], f0[n:]), "written past the floor-sized output"
    return _slice(flat[:n].reshape(B, Ho, Wo, ys), f0[:n].reshape(B, Ho, Wo, ys), yo, Cp)


@pytest.mark.parametrize("op", ["avg", 0, 1, 2])
@pytest.mark.parametrize("B,H,W,Cp", POOL_CASES)
def test_avgpool2_and_norm_act_pool2(lib, B, H, W, Cp, op):
    """egne_avgpool2 / egne_norm_act_pool2 (none, ReLU, leaky) and their bf16 twins; odd sizes drop the last row / column.
    MI355X: avgpool2 7.9e-8 (as fp32 torch: the same summation order), norm_act_pool2 8.4e-8 or less; twins within 0.94 of one bf16
    rounding."""
    g = _g(B + H + W + Cp)
    x = torch.randn(B, H, W, Cp, generator=g) * 2 + 0.3
    sc, sh = torch.rand(B, Cp, generator=g) + 0.5, torch.randn(B, Cp, generator=g)
    scd, shd = sc.to(DEV), sh.to(DEV)
    tag = "%s[%dx%dx%d Cp%d]" % ("avgpool2" if op == "avg" else "norm_act_pool2 act %d" % op, B, H, W, Cp)
    ref = (lambda t, a, b: R.avgpool2(t)) if op == "avg" else (lambda t, a, b: R.norm_act_pool2(t, a, b, op))
    _check(tag, _run_pool(lib, x, scd, shd, op, F32, 4, 12), ref(x.double(), sc.double(), sh.double()), ref(x, sc, sh))
    xq = _q(x)
    _twin(tag, _run_pool(lib, xq, scd, shd, op, BF, 8, 16), _run_pool(lib, xq, scd, shd, op, F32, 8, 16))


@pytest.mark.parametrize("kind", ["negative", "ties"])
@pytest.mark.parametrize("stride", [2, 1])
@pytest.mark.parametrize("H,W,Cp", [(2, 2, 8), (25, 13, 40), (30, 40, 40), (7, 2, 8)])
def test_maxpool2(lib, H, W, Cp, stride, kind):
    """egne_maxpool2 bit for bit against clipped ceil-mode windows: an all-negative input (a window over the border must not see
    zeros there) and an input of few levels (ties in most windows)."""
    _lib, L, st = lib
    B = 2
    g = _g(H + W + stride)
    x = torch.randn(B, H, W, Cp, generator=g)
    x = -0.5 - x.abs() if kind == "negative" else (x * 2).round() / 2
    want = R.maxpool2(x, stride)
    Ho, Wo = want.shape[1:3]
    xs, xo, ys, yo = Cp + 8, 4, Cp + 12, 8
    xb, yb = _buf(x, xs, xo), _poison((B, Ho, Wo, ys))
    y0 = yb.clone()
    _lib.check(L.egne_maxpool2(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, B, H, W, Ho, Wo, stride, Cp, st))
    _sync()
    assert torch.equal(_slice(yb, y0, yo, Cp), want)


# ==== bilinear up-sampling ============================================================================================================
def _run_up(lib, x, dt, xo, yo):
    _lib, L, st = lib
    B, H, W, Cp = x.shape
    xs, ys = Cp + 16, Cp + 24
    xb, yb = _buf(x, xs, xo, dt), _poison((B, 2 * H, 2 * W, ys), dt)
    y0 = yb.clone()
    fn = L.egne_upsample2x if dt == F32 else L.egne_upsample2x_bf16
    _lib.check(fn(xb.data_ptr(), xs, xo, yb.data_ptr(), ys, yo, B, H, W, Cp, st))
    _sync()
    return _slice(yb, y0, yo, Cp)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (3, 5), (30, 40)])
def test_upsample2x(lib, H, W):
    """egne_upsample2x and its bf16 twin (border rows / columns copy their neighbour; a single row or column has no second tap).
    MI355X: 9.9e-8 (fp32 torch 9.3e-8); the twin within 0.72 of one bf16 rounding."""
    B, Cp = 2, 40
    x = torch.randn(B, H, W, Cp, generator=_g(3 * H + W)) * 2
    tag = "upsample2x[%dx%d]" % (H, W)
    _check(tag, _run_up(lib, x, F32, 4, 12), R.upsample2x(x.double()), R.upsample2x(x))
    xq = _q(x)
    _twin(tag, _run_up(lib, xq, BF, 8, 16), _run_up(lib, xq, F32, 8, 16))


# ==== normalisation backward ==========================================================================================================
def _norm_bwd_inputs(B, HW, Cp, per_sample, act_in, seed):
    """x with every normalised value at least 1e-4 away from the kink of act_in (the kernel takes the branch from its own fp32 xh)."""
    g = _g(seed)
    x = torch.randn(B, HW, Cp, generator=g) * 2 + 0.5
    if HW == 2:
        # two pixels d apart: xh = +-a with 1 - a^2 = eps / (d^2 / 4 + eps), and gx = rstd (g1 - g2) / 2 (1 - a^2) is the difference of
        # O(1) terms that cancel to that factor.  With d = O(1) it is 1e-5 of them, and the fp32 rounding of the scale / shift the test
        # hands in (|mean| rstd 2^-24 in xh) alone puts float64 arithmetic 7e-7 .. 3e-4 off the reference, whatever the kernel does.
        # Keep the statistics a well-conditioned input: d^2 / 4 of the order of eps and a mean below d.
        d = 4e-3 + 6e-3 * torch.rand(B, Cp, generator=g)
        m = 1e-3 * torch.randn(B, Cp, generator=g)
        x = torch.stack([m + d / 2, m - d / 2], 1) * torch.where(x[:, :1] < 0, -1.0, 1.0)
    if act_in:
        for _ in range(3):
            sc, sh, _, _ = R.norm_stats(x.double(), per_sample)
            near = (x.double() * sc[:, None] + sh[:, None]).abs() < 1e-3
            x[near] += 0.05
        sc, sh, _, _ = R.norm_stats(x.double(), per_sample)
        margin = (x.double() * sc[:, None] + sh[:, None]).abs().min().item()
        assert margin > 1e-4, "a normalised value sits on the activation's kink (%.2e): choose another seed" % margin
    gy, pre = torch.randn(B, HW, Cp, generator=g), torch.randn(B, HW, Cp, generator=g)
    gam, bet = torch.rand(Cp, generator=g) + 0.5, torch.randn(Cp, generator=g)
    pdg, pdb = torch.randn(Cp, generator=g), torch.randn(Cp, generator=g)
    return x, gy, pre, gam, bet, pdg, pdb


def _run_norm_bwd(lib, ins, per_sample, act_in, C, store, dt, off):
    """One call.  scale / shift are the float64 statistics of x rounded to fp32.  Returns gx and, for batch statistics, the Cp
    entries of the dgamma / dbeta buffers."""
    _lib, L, st = lib
    x, gy, pre, gam, bet, pdg, pdb = ins
    B, HW, Cp = x.shape
    Bn = B if per_sample else 1
    sc, sh, _, _ = R.norm_stats(x.double(), per_sample)
    scd, shd = sc.float().contiguous().to(DEV), sh.float().contiguous().to(DEV)
    xs, gs, gxs = Cp + 16, Cp + 24, Cp + 32
    xb, gyb = _buf(x, xs, off, dt), _buf(gy, gs, off + 8, dt)
    gxb = _poison((B, HW, gxs), dt) if store else _buf(pre, gxs, off + 16, dt)
    g0 = gxb.clone()
    sums, ws = _table(Bn * Cp * 2), _ws(L.egne_norm_bwd_workspace_bytes(B, HW, Cp, per_sample))
    gamd = None if per_sample else gam.to(DEV)
    dg, db = (None, None) if per_sample else (_table(Cp), _table(Cp))
    if not per_sample:
        dg[:Cp], db[:Cp] = pdg.to(DEV), pdb.to(DEV)
    name = "egne_norm_bwd" + ("_store" if store else "") + ("" if dt == F32 else "_bf16")
    _lib.check(getattr(L, name)(xb.data_ptr(), xs, off, scd.data_ptr(), shd.data_ptr(), None if per_sample else gamd.data_ptr(),
                                gyb.data_ptr(), gs, off + 8, act_in, Cp, B, HW, per_sample, gxb.data_ptr(), gxs, off + 16,
                                sums.data_ptr(), None if per_sample else dg.data_ptr(), None if per_sample else db.data_ptr(), C,
                                ws.data_ptr(), st), name)
    _sync()
    _table_out(sums, Bn * Cp * 2, (Bn, Cp, 2))
    gx = _slice(gxb, g0, off + 16, Cp)
    if per_sample:
        return gx, None, None
    return gx, _table_out(dg, Cp, (Cp,)), _table_out(db, Cp, (Cp,))


def _rounded_stats_error(ins, per_sample, act_in, r64):
    """Error of gx that the fp32 rounding of the scale / shift handed to the kernel causes by itself: the kernel's formula in float64
    arithmetic on the rounded statistics against the float64 reference, relative to the largest element of the gradient."""
    x, gy, _, gam = (t.double() for t in ins[:4])
    sc, sh, _, _ = R.norm_stats(x, per_sample)
    sc, sh = sc.float().double()[:, None], sh.float().double()[:, None]
    xh = x * sc + sh
    g = R.act_bwd_bias(gy, xh, act_in)[0]
    dims = (1,) if per_sample else (0, 1)
    gx = sc * (g - g.mean(dims, keepdim=True) - xh * (g * xh).mean(dims, keepdim=True)) * (1.0 if per_sample else gam)
    return R.rel_err(gx, r64)


def _check_norm_bwd(lib, B, HW, Cp, per_sample, act_in, C, store):
    ins = _norm_bwd_inputs(B, HW, Cp, per_sample, act_in, 31 * HW + Cp + act_in)
    x, gy, pre, gam, bet, pdg, pdb = ins
    tag = "norm_bwd%s[ps%d B%d HW%d Cp%d act %d]" % ("_store" if store else "", per_sample, B, HW, Cp, act_in)
    gx, dg, db = _run_norm_bwd(lib, ins, per_sample, act_in, C, store, F32, 4)
    if per_sample:
        f = lambda a: R.norm_fwd(a, None, None, 1, act_in)  # noqa: E731
        (r64,), (r32,) = R.vjp(f, [x.double()], [gy.double()]), R.vjp(f, [x], [gy])
    else:
        f = lambda a, b, c: R.norm_fwd(a, b, c, 0, act_in)  # noqa: E731
        r64, r32 = R.vjp(f, [x.double(), gam.double(), bet.double()], [gy.double()]), R.vjp(f, [x, gam, bet], [gy])
        _check(tag + " dgamma", dg[:C], pdg.double()[:C] + r64[1][:C], pdg[:C] + r32[1][:C])
        _check(tag + " dbeta", db[:C], pdb.double()[:C] + r64[2][:C], pdb[:C] + r32[2][:C])
        assert torch.equal(dg[C:], pdg[C:]) and torch.equal(db[C:], pdb[C:]), "only C entries of dgamma / dbeta may change"
        r64, r32 = r64[0], r32[0]
    e_in = _rounded_stats_error(ins, per_sample, act_in, r64)
    print("%s: the rounding of the scale / shift handed in accounts for %.3e" % (tag, e_in))
    assert e_in <= ULP32, "the test's own statistics are too ill-conditioned an input (%.2e): choose other inputs" % e_in
    if store:
        _check(tag + " gx", gx, r64, r32)
    else:
        _check(tag + " gx", gx, pre.double() + r64, pre + r32)
    # bf16 twin on bf16-representable inputs
    q = tuple(_q(t) for t in ins[:3]) + ins[3:]
    o32, o16 = _run_norm_bwd(lib, q, per_sample, act_in, C, store, F32, 8), _run_norm_bwd(lib, q, per_sample, act_in, C, store, BF, 8)
    _twin(tag + " gx", o16[0], o32[0])
    if not per_sample:
        _same(tag + " dgamma", o16[1], o32[1])
        _same(tag + " dbeta", o16[2], o32[2])


@pytest.mark.parametrize("store", [0, 1])
@pytest.mark.parametrize("act_in", [0, 1, 2])
@pytest.mark.parametrize("B,HW,Cp", [(2, 2, 40), (2, 257, 40), (2, 1200, 40),
                                     (1, 76801, 8)])          # 300 chunks of 257 pixels, the last one empty
def test_norm_bwd_instance(lib, B, HW, Cp, act_in, store):
    """egne_norm_bwd / egne_norm_bwd_store with per-sample statistics against autograd through act_in(InstanceNorm(x)) in float64
    (the reference differentiates through the statistics), and the bf16 twins.  MI355X, largest over the activations: accumulating gx 1.6e-7 at HW = 2,
    7.0e-8 at 257, 6.7e-8 at 1200, 7.7e-8 at 76801; storing 1.3e-7, 1.1e-7, 1.1e-7, 1.2e-7 (fp32 autograd on the CPU 8e-8 .. 2.1e-7);
    at most 0.27 of the bound; the rounding of the statistics handed in accounts for 5.4e-8 or less; twins within 0.88 of one bf16
    rounding."""
    _check_norm_bwd(lib, B, HW, Cp, 1, act_in, Cp, store)


@pytest.mark.parametrize("store", [0, 1])
@pytest.mark.parametrize("Cp,C", [(40, 38), (64, 64)])
def test_norm_bwd_batch(lib, Cp, C, store):
    """Training-mode BatchNorm (B = 3, HW = 300: one statistics group of 900 pixels): gx, and dgamma / dbeta ACCUMULATED onto seeded
    values in their first C entries only.  MI355X: dgamma 6.3e-8, dbeta 5.9e-8 (fp32 autograd on the CPU 1.5e-7 / 1.9e-7), bit-equal in
    the twins; gx 7.6e-8 accumulating, 1.2e-7 storing."""
    _check_norm_bwd(lib, 3, 300, Cp, 0, 0, C, store)


def test_norm_bwd_grid_stride(lib):
    """70000 pixels x 8 vectors of one sample: more than norm_bwd_apply's 2048 blocks of 256.  MI355X: gx 6.9e-8."""
    _check_norm_bwd(lib, 1, 70000, 32, 1, 2, 32, 0)


# ==== activation backward + bias gradient =============================================================================================
def _act_bwd_inputs(npix, Cp, seed):
    g = _g(seed)
    gz, y = torch.randn(npix, Cp, generator=g), torch.randn(npix, Cp, generator=g)
    y.reshape(-1)[::7] = 0.0                      # y = 0 takes the slope's branch
    return gz, y, torch.randn(Cp, generator=g)


def _run_act_bwd(lib, gz, y, pdb, act, C, acc, dt, off, form):
    """form: "plain", "absmax" (word from 0 when acc = 0, from a larger prior word when acc = 1) or "null" (dbias = NULL)."""
    _lib, L, st = lib
    npix, Cp = gz.shape
    gs, ys = Cp + 16, Cp + 24
    gb = _buf(gz, gs, off, dt)
    yb = _buf(y, ys, off + 8, dt) if act else None
    g0 = gb.clone()
    nbytes = int(L.egne_act_bwd_bias_workspace_bytes(npix, Cp))
    ws = _ws(nbytes)
    dbias = _table(Cp)
    dbias[:Cp] = pdb.to(DEV)
    prior = _bits(1e6) if acc else 0
    word = _word(prior)
    args = (gb.data_ptr(), gs, off, yb.data_ptr() if act else None, ys, off + 8, act, Cp, npix, None if form == "null" else dbias.data_ptr(),
            C, acc, ws.data_ptr())
    if form == "absmax":
        _lib.check(L.egne_act_bwd_bias_absmax(*args, word.data_ptr(), st))
    else:
        _lib.check((L.egne_act_bwd_bias if dt == F32 else L.egne_act_bwd_bias_bf16)(*args, st))
    _sync()
    got = _slice(gb, g0, off, Cp)
    nchunk = nbytes // (8 * Cp)
    return got, _table_out(dbias, Cp, (Cp,)), ws[:nchunk * Cp].cpu().reshape(nchunk, Cp).sum(0), _word_out(word), prior


@pytest.mark.parametrize("form,acc", [("plain", 0), ("plain", 1), ("absmax", 0), ("absmax", 1), ("null", 0), ("bf16", 0), ("bf16", 1)])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("npix,Cp,C", [(n, cp, c) for n in (1, 255, 257, 76801) for cp, c in ((8, 5), (40, 38))])
def test_act_bwd_bias(lib, npix, Cp, C, act, form, acc):
    """egne_act_bwd_bias / egne_act_bwd_bias_absmax / egne_act_bwd_bias_bf16: g <- g act'(y) in place, dbias[c < C] (+)= its sums,
    the chunk sums in the workspace (read by egne_pair_bias_bwd) also when dbias is NULL, and the word that receives the bit pattern
    of max |g act'(y)|.  MI355X: masked g 1.8e-9 (leaky: 0.01f against 0.01; exact otherwise), chunk sums 1.8e-9, dbias 7.5e-8 (fp32
    torch up to 3.4e-7); the twin's dbias is bit-equal to the fp32 kernel's."""
    gz, y, pdb = _act_bwd_inputs(npix, Cp, npix + Cp + act)
    tag = "act_bwd_bias[%s npix %d Cp%d act %d acc %d]" % (form, npix, Cp, act, acc)
    if form == "bf16":
        gz, y = _q(gz), _q(y)
        g32, d32, _, _, _ = _run_act_bwd(lib, gz, y, pdb, act, C, acc, F32, 8, "plain")
        g16, d16, _, _, _ = _run_act_bwd(lib, gz, y, pdb, act, C, acc, BF, 8, "plain")
        _twin(tag + " g", g16, g32)
        _same(tag + " dbias", d16, d32)
        assert torch.equal(d16[C:], pdb[C:])
        return
    got, dbias, cols, word, prior = _run_act_bwd(lib, gz, y, pdb, act, C, acc, F32, 4, form)
    (r64, s64), (r32, s32) = R.act_bwd_bias(gz.double(), y.double(), act), R.act_bwd_bias(gz, y, act)
    _check(tag + " g", got, r64, r32)
    if act == 0:
        assert torch.equal(got, gz), "without an activation g is not rewritten"
    _check(tag + " chunk sums", cols, s64, s32)
    if form == "null":
        assert torch.equal(dbias, pdb), "dbias = NULL"
    else:
        start = pdb if acc else torch.zeros(Cp)
        _check(tag + " dbias", dbias[:C], start.double()[:C] + s64[:C], start[:C] + s32[:C])
        assert torch.equal(dbias[C:], pdb[C:]), "only C entries of dbias may change"
    if form == "absmax":
        mine = _bits(got.abs().max().item())
        assert word == max(prior, mine), "absmax word %#x, max |g act'(y)| %#x, prior %#x" % (word, mine, prior)
    else:
        assert word == prior


# ==== absmax ==========================================================================================================================
@pytest.mark.parametrize("kind", ["zero", "prior", "nan"])
@pytest.mark.parametrize("npix,Cp", [(1, 8), (300, 40), (70000, 32)])      # 70000 x 8 vectors > 2048 x 256
def test_absmax(lib, npix, Cp, kind):
    """egne_absmax: the bit pattern of max |x| over the slice, merged into the word with an integer maximum; POISON around the slice
    (777 > every |x| here) must not be seen; a NaN anywhere gives a pattern above +inf."""
    _lib, L, st = lib
    x = torch.randn(npix, Cp, generator=_g(npix + Cp))
    if kind == "nan":
        x[npix // 2, Cp - 3] = float("nan")
    start = _bits(500.0) if kind == "prior" else 0
    xb, word = _buf(x, Cp + 8, 4), _word(start)
    _lib.check(L.egne_absmax(xb.data_ptr(), Cp + 8, 4, Cp, npix, word.data_ptr(), st))
    _sync()
    got = _word_out(word)
    if kind == "nan":
        assert got > INF_BITS, hex(got)
    else:
        assert got == max(start, _bits(x.abs().max().item())), hex(got)


@pytest.mark.parametrize("kind", ["zero", "prior", "nan"])
@pytest.mark.parametrize("npix,Cp", [(1, 8), (300, 40), (70000, 64)])      # 70000 x 8 vectors > 2048 x 256
def test_absmax_f16(lib, npix, Cp, kind):
    """egne_absmax_f16: the same over a slice of halves; the word holds the maximum's pattern AS A FLOAT."""
    _lib, L, st = lib
    x = torch.randn(npix, Cp, generator=_g(npix + Cp + 1)).half()
    if kind == "nan":
        x[npix // 2, Cp - 3] = float("nan")
    start = _bits(500.0) if kind == "prior" else 0
    xb, word = _buf(x, Cp + 8, 8, torch.float16), _word(start)
    _lib.check(L.egne_absmax_f16(xb.data_ptr(), Cp + 8, 8, Cp, npix, word.data_ptr(), st))
    _sync()
    got = _word_out(word)
    if kind == "nan":
        assert got > INF_BITS, hex(got)
    else:
        assert got == max(start, _bits(x.float().abs().max().item())), hex(got)


# ==== the bf16 twins' vector rule =====================================================================================================
def test_bf16_twins_refuse_slices_off_the_8_channel_grid(lib):
    """The twins that move 16-byte vectors (8 bf16 channels) refuse a slice at offset 4, which the fp32 kernels take: once per kernel.
    Nothing is launched."""
    _lib, L, st = lib
    B, H, W, Cp = 1, 2, 2, 8
    xb, yb = _poison((B, H, W, 16), BF), _poison((B, H, W, 16), BF)
    tab, ws = _table(64), _ws(4096)
    x0, y0, t0 = xb.clone(), yb.clone(), tab.clone()
    p, q, t = xb.data_ptr(), yb.data_ptr(), tab.data_ptr()
    rcs = {
        "norm_stats": L.egne_norm_stats_bf16(p, 16, 4, Cp, B, H * W, 1, 1e-5, t, t, None, None, ws.data_ptr(), st),
        "norm_act_pool2": L.egne_norm_act_pool2_bf16(p, 16, 4, t, t, 2, q, 16, 8, B, H, W, Cp, st),
        "act_bwd_bias": L.egne_act_bwd_bias_bf16(p, 16, 4, q, 16, 8, 2, Cp, B * H * W, t, Cp, 0, ws.data_ptr(), st),
        "norm_bwd": L.egne_norm_bwd_bf16(p, 16, 4, t, t, None, q, 16, 8, 0, Cp, B, H * W, 1, q, 16, 0, t, None, None, Cp, ws.data_ptr(), st),
        "norm_bwd_store": L.egne_norm_bwd_store_bf16(p, 16, 4, t, t, None, q, 16, 8, 0, Cp, B, H * W, 1, q, 16, 0, t, None, None, Cp,
                                                     ws.data_ptr(), st),
    }
    _sync()
    assert all(rc != 0 for rc in rcs.values()), rcs
    assert torch.equal(xb, x0) and torch.equal(yb, y0) and torch.equal(tab, t0)
