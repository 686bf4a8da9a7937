"""-m gpu: geometry sweep of the generic convolution kernel egne_conv2d_fwd (csrc/conv_igemm.hip) -- the kernel that takes every convolution
no specialised kernel claims -- in its fp32, grouped, bf16-storage, bf16-MFMA and folded-tap instantiations and its five tile shapes.

Every row of conv_refs.SWEEP runs twice through Plan.conv, and every run must be a single ``conv_igemm`` launch:

(a) integer-valued data (conv_refs.int_case: every product and partial sum an integer the storage type holds exactly, checked on the
    CPU by tests/test_host_conv_refs.py): the result must be BIT-EQUAL to the float64 reference conv_refs.conv_ref, whatever the order
    of summation.  This is the addressing test: a wrong tap, frame, table row, K tail or tile edge changes integers.
(b) seeded normal data against the same reference under the project's bounds: FP32_BOUND = 2e-5 of the largest output
    (test_gpu_conv_backward_fp32.py) for fp32 tensors, EPS = 2^-8 of the output scale (test_gpu_bf16.py) for bf16 storage, where the
    reference reads the bf16 inputs and, on maps of >= 1024 output pixels (the bf16-MFMA rule of launch()), bf16-rounded weights.

Rows whose shape differs from the plain statement of the property, to stay on this kernel:
  * the <1, 4> tile row pads its 2x2 by 1: 128x128 without padding gives 127x127 outputs, 253 tiles of 128 rows, and the launcher takes
    <1, 4> from 256 on;
  * zero-padded 3x3 / stride-1 rows stay narrower than 30 pixels (the LDS-halo kernel takes wider maps), the 3-output row reads 24
    channels (32..64 go to the vector-ALU kernel), no row has <= 4 input channels with a padded 3x3 (first-layer kernel);
  * bf16 rows of >= 1024 output pixels use B = 3: from 4096 pixels a bf16 1x1 over raw slices goes to the streaming kernel.

Input slices sit behind eight poisoned channels and outputs between two poisoned blocks (768, a bf16 value); the padding channels of
the output slice must come back as zeros.

Measured on MI355X: all 49 integer runs bit-equal; normal data (relative to the largest output) fp32 rows 1.4e-7 .. 9.0e-7, grouped
1.5e-7 .. 2.7e-7 (bound 2e-5), bf16 storage with exact products 1.7e-3 .. 3.0e-3, bf16 MFMA 2.9e-3 .. 3.3e-3, folded taps 2.7e-3 .. 3.1e-3
(bound 3.9e-3: the rounding of the stored output, half a bf16 ulp of a value near the top of its binade); per row in the docstring of
test_normal_data_within_the_project_bound.  absmax word 0x411d4814 = bits of 9.830097, the largest stored value.
"""
import ctypes as C

import pytest
import torch

import conv_refs as R
from test_gpu_bf16 import EPS
from test_gpu_conv_backward_fp32 import FP32_BOUND, _conv_kinds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 768.0


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import egne_amd  # noqa: F401
    return True


def _slices(pl, xs, B, H, W, lead=8):
    """NCHW CPU tensors -> padded slices of one NHWC buffer of the plan's storage type, behind ``lead`` poisoned channels."""
    from egne_amd.engine import Piece
    buf = pl.buf(B, H, W, lead + sum(R.pad8(x.shape[1]) for x in xs))
    buf[..., :lead] = POISON
    pieces, off = [], lead
    for x in xs:
        c = x.shape[1]
        buf[..., off:off + c] = x.permute(0, 2, 3, 1).to(DEV).to(buf.dtype)
        pieces.append(Piece(buf, off, c))
        off += R.pad8(c)
    return pieces


def _run(case, data):
    """One Plan.conv of the row on ``data``; returns the NCHW result (fp32 on the CPU), the plan and the launch's descriptor."""
    from egne_amd.engine import ConvLayer, Piece, Plan
    bf = case["dtype"] == "bf16"
    B, H, W, Cout = case["B"], case["H"], case["W"], case["Cout"]
    pl = Plan(torch.device(DEV), dtype=R.BF if bf else torch.float32)
    pieces = _slices(pl, data["xs"], B, H, W)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV)) for w in data["ws"]], [torch.nn.Parameter(b.to(DEV)) for b in data["bs"]],
                      [(p.C, p.Cp) for p in pieces], stride=case["stride"], pad=case["pad"], dils=case["dils"], act=data["act"],
                      pad_mode=case["pad_mode"])
    for i, (sc, sh, act_in) in (data["norm"] or {}).items():
        scp, shp = torch.zeros(B, pieces[i].Cp, device=DEV), torch.zeros(B, pieces[i].Cp, device=DEV)
        scp[:, :sc.shape[1]], shp[:, :sh.shape[1]] = sc.to(DEV), sh.to(DEV)
        pl.keep += [scp, shp]
        pieces[i] = pieces[i].with_norm(scp, shp, act_in)
    if data["post"] is not None:
        ps, pt = torch.zeros(layer.CoutP, device=DEV), torch.zeros(layer.CoutP, device=DEV)
        ps[:Cout], pt[:Cout] = data["post"][0].to(DEV), data["post"][1].to(DEV)
        layer.post = (ps, pt)
    Ho, Wo = layer.out_hw(H, W)
    assert (Ho, Wo) == R.out_hw(case)
    Cs = R.pad8(Cout)
    out = pl.buf(B, Ho, Wo, Cs + 16)
    out.fill_(POISON)
    res = _slices(pl, [data["residual"]], B, Ho, Wo)[0] if data["residual"] is not None else None
    pl.conv(layer, pieces, Piece(out, 8, Cout), B, H, W, residual=res, name="sweep")
    kinds = _conv_kinds(pl, "sweep")
    assert kinds == ["conv_igemm"], "%s: planned as %s" % (case["id"], kinds)
    d = pl.calls[-1][1][0]._obj
    # the descriptor the launcher's rule (conv_refs.launch_form) is applied to
    assert (d.dtype, d.ngroups, d.CoutP, d.B, d.Ho, d.Wo, d.kh, d.kw) == (int(bf), len(case["dils"]), R.pad32(Cout), B, Ho, Wo) + case["k"]
    assert d.nseg == len(case["chans"]) and d.Ktot == sum(R.pad8(c) for c in case["chans"])
    assert R.launch_form(case) == (case["form"], case["tile"])
    pl.run()
    torch.cuda.synchronize()
    o = out.float().cpu()
    assert (o[..., :8] == POISON).all() and (o[..., 8 + Cs:] == POISON).all(), "conv wrote outside its output slice"
    if Cout < Cs:
        assert (o[..., 8 + Cout:8 + Cs] == 0).all(), "padding channels must be written as zeros"
    return o[..., 8:8 + Cout].permute(0, 3, 1, 2).contiguous(), pl, d


@pytest.mark.parametrize("case", R.SWEEP, ids=R.SWEEP_IDS)
def test_integer_data_is_bit_equal(gpu, case):
    """(a) Exactly representable data: torch.equal with the float64 reference, for every row.  MI355X: all 49 rows bit-equal."""
    data, want = R.int_case(torch.Generator().manual_seed(1234), case)
    got, _, _ = _run(case, data)
    bad = (got.double() != want)
    print("%s [%s <%d,%d>]: weight density %.2f, max |y| %d, %d of %d outputs differ"
          % (case["id"], case["form"], case["tile"][0], case["tile"][1], data["density"], want.abs().max().item(), int(bad.sum()), bad.numel()))
    if bad.any():
        n, c, y, x = [int(v) for v in bad.nonzero()[0]]
        per_frame = [int(v) for v in bad.sum(dim=(1, 2, 3))]
        per_tap_row = [int(v) for v in bad.sum(dim=(0, 1, 3))]
        raise AssertionError("%s: %d of %d outputs differ (per frame %s, per output row %s); first at n %d c %d y %d x %d: got %r, want %r"
                             % (case["id"], int(bad.sum()), bad.numel(), per_frame, per_tap_row, n, c, y, x, got[n, c, y, x].item(), want[n, c, y, x].item()))
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("case", R.SWEEP, ids=R.SWEEP_IDS)
def test_normal_data_within_the_project_bound(gpu, case):
    """(b) Seeded normal data against float64 on the same stored values.  Relative error on MI355X, per row:
      f32-1x1-s2 1.37e-07; f32-1x1-3slices-affine 4.67e-07; f32-3x3-s2-9x12 3.41e-07
      f32-3x3-s2-10x13 3.68e-07; f32-3x3-s3 3.75e-07; f32-3x3-pad01 3.13e-07
      f32-5x3-pad20 4.41e-07; f32-1x7-pad03 3.17e-07; f32-7x1-pad30 2.71e-07
      f32-5x5-dil2-reach-past-map 3.28e-07; f32-3x3-dil2-s2 3.68e-07; f32-5x5-on-2x3 2.14e-07
      f32-6x6-s2-36taps 9.03e-07; f32-6x6-s3-36taps 4.22e-07; f32-reflect-4x4-s2 5.15e-07
      f32-reflect-3x3-dil2 3.71e-07; f32-reflect-7x7-pad-H-1 6.53e-07; f32-cout3 3.49e-07
      f32-cout96 4.38e-07; f32-cout64 4.41e-07; f32-cout100 3.76e-07
      f32-1x1-cout96 1.58e-07; f32-tile-1x4 2.39e-07; f32-cin72 7.00e-07
      f32-cin40 6.20e-07; f32-8-slices 8.65e-07; f32-residual-post-act-cout21 2.47e-07
      f32-affine-padded-3x3 5.03e-07; grouped-dil123-cout32 2.67e-07; grouped-dil123-cout64 2.58e-07
      grouped-dil4812-cout32 1.50e-07; grouped-dil4812-cout64 2.06e-07; bf16-3x3-s2-10x13 2.40e-03
      bf16-3x3-pad01 2.09e-03; bf16-6x6-s2-36taps 2.67e-03; bf16-reflect-4x4-s2 1.68e-03
      bf16-reflect-3x3-dil2 1.88e-03; bf16-reflect-7x7-pad-H-1 1.95e-03; bf16-1x1-3slices-affine 3.00e-03
      bfm-3x3-s2-slices-40-24 2.92e-03; bfm-5x5-dil2 2.96e-03; bfm-6x6-s2-36taps 3.05e-03
      bfm-reflect-4x4-s2 3.04e-03; bfm-1x1-slices-8-24 3.25e-03; fold-2x2 2.96e-03
      fold-3x3-pad0 2.98e-03; fold-5x5-zero-pad2 2.74e-03; fold-7x7-zero-pad3 3.08e-03
      fold-7x7-reflect-s2 2.82e-03"""
    data = R.normal_case(torch.Generator().manual_seed(4321), case)
    weights = [w.to(R.BF).float() for w in data["ws"]] if R.rounds_weights(case) else None
    want = R.ref_of(case, data, weights)
    got, _, _ = _run(case, data)
    scale = want.abs().max().item()
    err = (got.double() - want).abs().max().item() / scale
    bound = EPS if case["dtype"] == "bf16" else FP32_BOUND
    print("%s [%s <%d,%d>]: relative error %.2e (bound %.1e)" % (case["id"], case["form"], case["tile"][0], case["tile"][1], err, bound))
    assert err < bound, "%s: relative error %.2e" % (case["id"], err)


def test_absmax_word_is_the_largest_stored_magnitude(gpu):
    """egne_conv_desc.absmax_out (the word a split-f16 consumer of a training plan derives its pre-scale from): the fp32 bit pattern of
    max |stored value| over the output slice.  B = 3 on 9x10 with 256-row tiles: the last tile has 14 of its 256 rows.  Inputs in
    [0.5, 1], weights negative, bias 10: every stored value lies below 10, and a row past M -- an all-zero operand row -- would
    evaluate to the bias itself, so a kernel that takes the maximum over rows that do not exist publishes 10.0."""
    from egne_amd.engine import ConvLayer, Piece, Plan
    g = torch.Generator().manual_seed(99)
    B, H, W, Cin, Cout = 3, 9, 10, 16, 29
    x = 0.5 + 0.5 * torch.rand(B, Cin, H, W, generator=g)
    w = -(0.1 + torch.rand(Cout, Cin, 3, 3, generator=g)) / (Cin * 9)
    b = torch.full((Cout,), 10.0)
    want = R.conv_ref([x], [w], [b], pad=(1, 1))
    assert 0 < want.min().item() and want.max().item() < 10.0
    pl = Plan(torch.device(DEV))
    pl.dyn_scales = True
    (px,) = _slices(pl, [x], B, H, W)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV))], [torch.nn.Parameter(b.to(DEV))], [(Cin, Cin)], pad=(1, 1))
    out = pl.buf(B, H, W, 8 + R.pad8(Cout))
    pl.conv(layer, [px], Piece(out, 8, Cout), B, H, W, name="amax")
    assert _conv_kinds(pl, "amax") == ["conv_igemm"]
    d = pl.calls[-1][1][0]._obj
    assert d.absmax_out and B * H * W % 256 == 14
    slot = (d.absmax_out - pl.dynbuf.data_ptr()) // 4
    for _ in range(2):           # (the word is cleared at the start of every run)
        pl.run()
        torch.cuda.synchronize()
        stored = out[..., 8:8 + R.pad8(Cout)].float().cpu()
        word = int(pl.dynbuf[slot].item())
        expect = int(stored.abs().max().view(torch.int32).item())
        print("absmax word %#x, max |stored| %#x (%.6f)" % (word, expect, stored.abs().max().item()))
        assert (stored[..., :Cout].permute(0, 3, 1, 2).double() - want).abs().max().item() < FP32_BOUND * 10.0
        assert word == expect, (hex(word), hex(expect))


def test_reflect_reach_beyond_the_map_is_refused(gpu):
    """Reflect padding mirrors once, so its reach pad * dilation must stay below the map size: pad 2 with dilation 2 on a 4x9 map
    (pad < H, reach 4 = H) used to pass validation and read rows of the wrong line.  Refused before any launch, naming the sizes."""
    from egne_amd import _lib
    from egne_amd.engine import ConvLayer, Piece, Plan
    g = torch.Generator().manual_seed(7)
    B, H, W, Cin, Cout = 2, 4, 9, 16, 32
    pl = Plan(torch.device(DEV))
    (px,) = _slices(pl, [torch.randn(B, Cin, H, W, generator=g)], B, H, W)
    layer = ConvLayer([torch.nn.Parameter(torch.randn(Cout, Cin, 3, 3, generator=g).to(DEV))], [torch.nn.Parameter(torch.zeros(Cout, device=DEV))],
                      [(Cin, Cin)], pad=(2, 2), dils=(2,), pad_mode=1)
    Ho, Wo = layer.out_hw(H, W)
    out = pl.buf(B, Ho, Wo, Cout)
    out.fill_(POISON)
    pl.conv(layer, [px], Piece(out, 0, Cout), B, H, W, name="refused")
    assert _conv_kinds(pl, "refused") == ["conv_igemm"]
    d = pl.calls[-1][1][0]._obj
    L = _lib.lib()
    rc = L.egne_conv2d_fwd(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = L.egne_last_error()
    assert rc != 0 and b"reflect" in msg and b"4x9" in msg and b"4x4" in msg, (rc, msg)
    assert (out == POISON).all(), "a refused call must not launch"
