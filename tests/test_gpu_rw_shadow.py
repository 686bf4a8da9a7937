"""The resident-weights 3x3 (csrc/conv3x3_rw_f16.hip) in its two consumer loops: the shadow form (default: two accumulator sets that swap
by tile parity, the finished tile's epilogue and stores among the MFMAs of the next tile's first job, tile coordinates advanced without a
division) against the hand-over form it replaces (EGNE_RW_SHADOW=0, read at every launch).  The sweep rows of this kernel
(tests/split_refs.py) give a workgroup at most two tiles and never reach the pooled, split-pair or f16 outputs; the cases here give
workers 0, 1, 3, 4 and more tiles, end on partial tiles, and take every epilogue option of the entry point (the one combination that
stays on the hand-over form is marked in CASES).

Every case asserts twice:
  (a) integer data (inputs in [-4, 4] under a_scale 256, weights in [-2, 2] under w_scale 512: no lo half, every partial sum an
      integer below 2^14, so nothing is rounded anywhere): the default form EQUALS the float64 convolution through the epilogue --
      as fp32 values, as f16(v * s) for f16 storage, as hi = f16(v * s), lo = f16(v * s - hi) for split-pair storage;
  (b) seeded normal data: the two forms write the same bits into every output buffer (poisoned padding included) and the same
      overflow word.
test_overflow_word plants one infinite input under the last tile of a worker.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -777.0
NONE, RELU, LEAKY = 0, 1, 2
A_INT, W_INT = 256.0, 512.0


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import egne_amd  # noqa: F401
    from egne_amd import _lib
    return _lib.lib()


def _pad32(c):
    return (c + 31) // 32 * 32


def _case(id, B, H, W, Cin, Cout, act=NONE, products=3, norm=False, residual=False, post=False, pool=False, out_split=0, f16in=False):
    return dict(id=id, B=B, H=H, W=W, Cin=Cin, Cout=Cout, act=act, products=products, norm=norm, residual=residual, post=post, pool=pool,
                out_split=out_split, f16in=f16in)


# tiles are 32 x 8 pixels; workers = 256 / (blocks of 32 stored channels); 41 x 130: 6 x 5 tiles per frame, the last tile row 1 pixel
# high and the last tile column 2 pixels wide; 41 x 129: the last column 1 pixel wide, odd height and width for the ceil-mode pool
CASES = [
    _case("single-tile", 1, 8, 32, 64, 32),                                          # 1 tile, 255 idle workgroups: flush only
    _case("uneven-64-128", 7, 41, 130, 64, 128, act=RELU),                           # 210 tiles on 64 workers: 3 or 4 each
    _case("one-chunk-32-256", 6, 41, 130, 32, 256),                                  # 180 tiles on 32 workers: 5 or 6 each
    _case("one-chunk-affine", 6, 41, 130, 32, 256, act=LEAKY, norm=True),            # InstanceNorm affine + LeakyReLU on load
    _case("streamed-128-128", 7, 41, 130, 128, 128, act=RELU),                       # four streamed chunks, four output blocks
    _case("streamed-tail-72-24", 26, 41, 130, 72, 24, act=LEAKY),                    # Ktot 96 with a K tail; 24 of 32 channels; 780 tiles on 256
    _case("pool-relu", 13, 41, 129, 64, 64, act=RELU, pool=True),                    # 390 tiles on 128 workers: 3 or 4 each
    _case("pool-leaky", 13, 41, 129, 64, 64, act=LEAKY, pool=True),
    _case("split-pair", 26, 41, 130, 64, 32, act=RELU, out_split=1),                 # both planes
    _case("split-pair-np1", 26, 41, 130, 64, 32, act=RELU, out_split=1, products=1),  # the hi plane alone
    # post affine / residual.  Three products: a form of its own (which of the two is present is read at run time: all three
    # combinations); together with a pooled output the launcher keeps the hand-over form, so "pool-residual" compares that form with
    # itself and checks the fallback only.  One product: the epilogue is read at run time, every combination runs the shadow form.
    _case("residual-post", 13, 41, 130, 64, 64, act=LEAKY, residual=True, post=True),
    _case("residual-only", 13, 41, 130, 32, 64, act=RELU, residual=True),            # one resident chunk
    _case("post-only-streamed", 7, 41, 130, 96, 128, act=LEAKY, post=True),           # three streamed chunks
    _case("pool-residual", 13, 41, 129, 64, 64, act=RELU, pool=True, residual=True),
    _case("residual-post-np1", 13, 41, 130, 64, 64, act=LEAKY, residual=True, post=True, products=1),
    _case("pool-residual-np1", 13, 41, 129, 64, 64, act=RELU, pool=True, residual=True, products=1),
    _case("residual-np1-streamed", 7, 41, 130, 96, 128, act=NONE, residual=True, products=1),
    _case("np1-f16-in-out", 13, 41, 129, 64, 64, act=RELU, products=1, out_split=2, f16in=True, pool=True),
]
IDS = [c["id"] for c in CASES]


def _data(case, exact):
    """Seeded inputs of the case on the CPU (NHWC / OIHW float32): integers for the exact run, normal data otherwise."""
    g = torch.Generator().manual_seed(99 + len(case["id"]) + (1000 if exact else 0))
    B, H, W, Cin, Cout = case["B"], case["H"], case["W"], case["Cin"], case["Cout"]
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()      # noqa: E731
    d = {}
    if exact:
        d["x"] = ri((B, H, W, Cin), 0 if case["norm"] else -4, 4)
        d["w"] = ri((Cout, Cin, 3, 3), -2, 2)
        d["bias"] = ri((Cout,), -3, 3)
        d["a_scale"], d["w_scale"] = A_INT, W_INT
        if case["norm"]:        # x * scale + shift: non-negative integers up to 4 (exact through the LeakyReLU on load)
            d["nscale"] = 2.0 ** -ri((B, Cin), 0, 1)
            d["x"] = d["x"] / d["nscale"][:, None, None, :] * (d["x"] <= 2)
            d["nshift"] = ri((B, Cin), 0, 2)
        if case["residual"]:
            d["res"] = ri((B, H, W, Cout), -8, 8)
        if case["post"]:
            d["ps"], d["pt"] = 2.0 ** ri((Cout,), -1, 1), ri((Cout,), -6, 6)
        d["oss"] = float(torch.tensor(1 / 3, dtype=torch.float32)) if case["out_split"] else 1.0      # storage scale of f16 / split-pair outputs: v * s is ONE fp32 rounding, most lo halves are non-zero
    else:
        import split_refs as S
        d["x"] = torch.randn((B, H, W, Cin), generator=g)
        d["w"] = torch.randn((Cout, Cin, 3, 3), generator=g) / (3 * Cin ** 0.5)
        d["bias"] = torch.randn((Cout,), generator=g)
        if case["norm"]:
            d["nscale"], d["nshift"] = torch.rand((B, Cin), generator=g) + 0.5, torch.randn((B, Cin), generator=g)
            d["a_scale"] = S.F16X3_ASCALE
        else:
            d["a_scale"] = S.a_scale_for(float(d["x"].abs().max()))
        d["w_scale"] = S.w_scale_for([d["w"]])
        if case["residual"]:
            d["res"] = torch.randn((B, H, W, Cout), generator=g)
        if case["post"]:
            d["ps"], d["pt"] = torch.rand((Cout,), generator=g) + 0.5, torch.randn((Cout,), generator=g)
        d["oss"] = 256.0
    return d


def _launch(L, case, d, shadow, monkeypatch):
    """One launch of egne_conv3x3_rw_f16_fwd.  Returns (out, pooled or None, overflow word, (channel offset of the output slice, of the pooled
    slice)): the WHOLE buffers, on the CPU."""
    from egne_amd import _lib
    monkeypatch.setenv("EGNE_RW_SHADOW", "1" if shadow else "0")
    B, H, W, Cin, Cout = case["B"], case["H"], case["W"], case["Cin"], case["Cout"]
    Cp, Cs, CoutP = (Cin + 7) // 8 * 8, (Cout + 7) // 8 * 8, _pad32(Cout)
    Ktot = _pad32(Cp)
    f16o = case["out_split"] == 2
    keep = []

    def dev(t, dtype=torch.float32):
        t = t.to(dtype).to(DEV).contiguous()
        keep.append(t)
        return t
    # input slice at channel offset 8 of a wider buffer
    xs = Cp + 16
    xb = torch.full((B, H, W, xs), POISON)
    xb[..., 8:8 + Cin] = d["x"] * (d["a_scale"] if case["f16in"] else 1.0)
    xb[..., 8 + Cin:8 + Cp] = 0
    xb = dev(xb, torch.float16 if case["f16in"] else torch.float32)
    fhi = torch.zeros(9 * CoutP * Ktot, dtype=torch.float16, device=DEV)
    flo = torch.zeros_like(fhi)
    wd = dev(d["w"])
    _lib.check(L.egne_pack_conv_weight_f16frag(wd.data_ptr(), Cout, Cin, 3, 3, CoutP, Ktot, d["w_scale"], fhi.data_ptr(), flo.data_ptr(),
                                               _lib.stream_ptr()), "pack")
    bias = torch.zeros(CoutP)
    bias[:Cout] = d["bias"]
    bias = dev(bias)
    ooff = 32 if case["out_split"] == 1 else 8
    ostride = ooff + CoutP + 8
    out = dev(torch.full((B, H, W, ostride), POISON), torch.float16 if f16o else torch.float32)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    dd = _lib.ConvDesc()
    dd.B, dd.H, dd.W, dd.Ho, dd.Wo = B, H, W, H, W
    dd.kh = dd.kw = 3
    dd.stride, dd.pad_h, dd.pad_w, dd.pad_mode, dd.ngroups, dd.nseg = 1, 1, 1, 0, 1, 1
    dd.dil[0] = 1
    sg = dd.seg[0]
    sg.ptr, sg.pix_stride, sg.ch_off, sg.Cp, sg.presplit = xb.data_ptr(), xs, 8, Cp, 2 if case["f16in"] else 0
    if case["norm"]:
        sc, sh = torch.zeros(B, Cp), torch.zeros(B, Cp)
        sc[:, :Cin], sh[:, :Cin] = d["nscale"], d["nshift"]
        sc, sh = dev(sc), dev(sh)
        sg.scale, sg.shift, sg.act_in = sc.data_ptr(), sh.data_ptr(), LEAKY
    dd.Ktot, dd.CoutP, dd.bias, dd.act = Ktot, CoutP, bias.data_ptr(), case["act"]
    if case["post"]:
        ps, pt = torch.zeros(CoutP), torch.zeros(CoutP)
        ps[:Cout], pt[:Cout] = d["ps"], d["pt"]
        ps, pt = dev(ps), dev(pt)
        dd.post_scale, dd.post_shift = ps.data_ptr(), pt.data_ptr()
    if case["residual"]:
        rb = torch.full((B, H, W, Cs + 8), POISON)
        rb[..., 4:4 + Cout] = d["res"]
        rb = dev(rb)
        dd.residual, dd.res_pix_stride, dd.res_ch_off = rb.data_ptr(), Cs + 8, 4
    dd.out, dd.out_pix_stride, dd.out_ch_off, dd.Cout_store = out.data_ptr(), ostride, ooff, Cs
    pooled = None
    if case["pool"]:
        pooled = dev(torch.full((B, (H + 1) // 2, (W + 1) // 2, Cs + 8), POISON), torch.float16 if f16o else torch.float32)
        dd.pool_out, dd.pool_pix_stride, dd.pool_ch_off = pooled.data_ptr(), Cs + 8, 8 if f16o else 4
    dd.out_split, dd.out_split_scale, dd.ovf_flag, dd.f16_products = case["out_split"], d["oss"], ovf.data_ptr(), case["products"]
    _lib.check(L.egne_conv3x3_rw_f16_fwd(C.byref(dd), fhi.data_ptr(), flo.data_ptr(), d["a_scale"], d["w_scale"], _lib.stream_ptr()), case["id"])
    torch.cuda.synchronize()
    return out.cpu(), None if pooled is None else pooled.cpu(), int(ovf.item()), (ooff, 8 if f16o else 4)


def _conv64(x, w):
    """float64 3x3 'same' convolution, NHWC x OIHW -> NHWC: nine shifted matrix products."""
    B, H, W, Cin = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x
    y = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].double().t()
    return y


def _act32(t, act):
    """The kernels' activation on fp32: fmaxf(t, t * slope)."""
    if act == NONE:
        return t
    return torch.maximum(t, t * torch.tensor(0.0 if act == RELU else 0.01, dtype=torch.float32))


_WANT = {}


def _want(case, d):
    """fp32 values the epilogue must produce on the integer data (everything before the activation is exact; the LeakyReLU slope is
    one fp32 multiply), NHWC, and their ceil-mode 2x2 maxima.  Computed once per case."""
    if case["id"] not in _WANT:
        x = d["x"].double()
        if case["norm"]:
            x = x * d["nscale"].double()[:, None, None, :] + d["nshift"].double()[:, None, None, :]
            assert (x >= 0).all() and (x == x.round()).all() and x.max() <= 4
        t = _conv64(x, d["w"]) + d["bias"].double()
        assert t.abs().max() < 2 ** 14
        v = _act32(t.float(), case["act"])
        assert case["act"] != LEAKY or (v < 0).any()
        pooled = torch.nn.functional.max_pool2d(v.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1) if case["pool"] else None
        if case["post"]:
            v = (v.double() * d["ps"].double() + d["pt"].double()).float()      # one rounding, as the kernel's fused multiply-add
        if case["residual"]:
            v = v + d["res"]
        _WANT[case["id"]] = (v, pooled)
    return _WANT[case["id"]]


def _plane_channel():
    """Position q of a split-pair plane holds channel 4 (q >> 3) + (q & 3) + 16 ((q >> 2) & 1) of the 32-channel block."""
    q = torch.arange(32)
    return 4 * (q >> 3) + (q & 3) + 16 * ((q >> 2) & 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_data_equals_float64(L, case, monkeypatch):
    d = _data(case, True)
    out, pooled, ovf, (ooff, poff) = _launch(L, case, d, True, monkeypatch)
    v, vp = _want(case, d)
    Cout, s = case["Cout"], torch.tensor(d["oss"], dtype=torch.float32)
    assert ovf == 0
    if case["out_split"] == 1:
        planes = out[..., ooff:ooff + 32].contiguous().view(torch.float16).reshape(*out.shape[:3], 2, 32)
        t = v[..., _plane_channel()] * s
        hi = t.half()
        assert torch.equal(planes[..., 0, :], hi), "hi plane"
        if case["products"] == 3:
            assert torch.equal(planes[..., 1, :], (t - hi.float()).half()), "lo plane"
            assert (t - hi.float()).half().abs().max() > 0
        else:
            assert (out[..., ooff + 16:ooff + 32] == POISON).all(), "a one-product launch leaves the lo plane alone"
    elif case["out_split"] == 2:
        assert torch.equal(out[..., ooff:ooff + Cout], (v * s).half())
        assert torch.equal(pooled[..., poff:poff + Cout], (vp * s).half())
    else:
        got = out[..., ooff:ooff + Cout]
        bad = got != v
        assert not bad.any(), "%s: %d of %d outputs differ, first at %s" % (case["id"], int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
        if case["pool"]:
            assert torch.equal(pooled[..., poff:poff + Cout], vp)
    # nothing outside the slice
    Cs = (Cout + 7) // 8 * 8
    assert (out[..., :ooff] == POISON).all() and (out[..., ooff + _pad32(Cs) if case["out_split"] == 1 else ooff + Cs:] == POISON).all()
    if pooled is not None:
        assert (pooled[..., :poff] == POISON).all() and (pooled[..., poff + Cs:] == POISON).all()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_forms_write_the_same_bits(L, case, monkeypatch):
    d = _data(case, False)
    o0, p0, f0, _ = _launch(L, case, d, False, monkeypatch)
    o1, p1, f1, _ = _launch(L, case, d, True, monkeypatch)
    assert torch.equal(_bits(o0), _bits(o1)), "%s: %d output words differ" % (case["id"], int((_bits(o0) != _bits(o1)).sum()))
    assert (p0 is None) == (p1 is None) and (p0 is None or torch.equal(_bits(p0), _bits(p1))), "pooled output"
    assert f0 == f1 == 0
    assert (o1 != POISON).any() and torch.isfinite(o1.float()).all()


@pytest.mark.parametrize("cid", ["uneven-64-128", "pool-relu", "np1-f16-in-out"])
def test_overflow_word(L, cid, monkeypatch):
    """One infinite input under the last pixel of the last frame: a non-finite result in the LAST tile of its worker (the tile that
    is finished after the loop).  Both forms set the word and store the same bits; the clean runs above leave it clear."""
    case = CASES[IDS.index(cid)]
    d = dict(_data(case, False))
    d["x"] = d["x"].clone()
    d["x"][-1, -1, -1, :] = float("inf")
    o0, p0, f0, _ = _launch(L, case, d, False, monkeypatch)
    o1, p1, f1, _ = _launch(L, case, d, True, monkeypatch)
    assert f0 == 1 and f1 == 1
    assert torch.equal(_bits(o0), _bits(o1)) and (p0 is None or torch.equal(_bits(p0), _bits(p1)))
    assert not torch.isfinite(o1[-1, -1, -1].float()).all()
