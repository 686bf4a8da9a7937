"""-m gpu: addressing sweep of the split-f16 forward convolution kernels on data for which they must be BIT-EQUAL to float64.

Every row of split_refs.SPLIT_SWEEP is pinned to one kernel -- the list of convolution kinds in Plan.meta and the _lib entry of every
launch are asserted before anything runs -- and goes through Plan.conv four times:

(a) integer data (conv_refs.int_case): every lo half is zero; hi addressing, epilogue, slices;
(b) fine inputs (split_refs.fine_inputs_case): 12 to 13 significant bits in the activations, >= 20 % non-zero lo halves, integer weights;
(c) fine weights (split_refs.fine_weights_case): integer activations, 12-bit weights;
(d) seeded normal data under the project's existing bounds: 2e-6 of the largest output against float64 (test_gpu_ops.py), and for rows
    of plain-f16 plans (f16_products = 1) 4e-6 against float64 on the f16-rounded operands (test_deep_trunk_kernel_plain_f16_four_stage_form).

In (a) .. (c) every product hi*hi, hi*lo, lo*hi and every partial sum is an fp32 value (tests/test_host_split_refs.py proves it per row on
the CPU, under the scales asserted here after the calibrating run), so the result is torch.equal to the reference whatever the order
of summation; rows with f16_products = 1 must equal the convolution of the hi halves alone, which in (b) and (c) differs from the
three-product value in more than half of the outputs: they prove that no lo half is used.  Every plan runs at least twice and must
repeat its bits.  Input slices sit behind eight poisoned channels, the output between two poisoned blocks, the residual in a slice of
its own; the padding channels of the output slice must come back as zeros.

Template builds the rows reach, per kernel file:
  conv_halo_f16.hip      32-, 64- (two and three N tiles) and 96-wide tiles; plain and transposed walk; dilation 1, 2 and the lattice
                         mode; input affine; NP = 1; a second tile per workgroup; accumulation onto the destination (lattice rows).
                         Not reached: the pooled second output, statistics from the epilogue, split-pair (3) input
                         (test_gpu_ops.py: test_conv3x3_halo_pooled_second_output, test_instance_norm_statistics_from_the_conv_epilogue).
  conv3x3_rs_f16.hip     <1,1,8> <1,2,8> <2,1,4> <2,2,4> <2,4,4> with statistics, the two transposed-store builds (64 -> 64, 64 -> 32 with
                         residual), a second tile per workgroup.  Not reached: the pooled second output, dyn_scale (training plans).
  conv3x3_rw_f16.hip     resident weights with one and two chunks, 1 / 2 / 3-of-4 output blocks, streamed weights (with a K tail and an
                         input affine), NP = 1, a second tile per worker.  Not reached: split-pair and f16 storage, pooled output.
  conv_f16x3.hip         flat 256x32, 256x64, 128x128, grouped, 1x1 with residual, 32 taps; small-problem 64x64 and 128x32 with split-K and
                         the 128x128 tile.  Not reached: dyn_scale, the deep kernel's frame tail (test_deep_trunk_kernel_with_frame_tail).
  conv_f16x3_big.hip     the 256-wide N tile with three products, the 128-wide one with one product.  conv_f16_big1.hip: the four-stage
                         form, 256 wide.  Not reached: 128 wide with three products (test_conv_f16x3_split_precision), 256 wide with one
                         product in the two-stage form, the four-stage form 128 wide (test_deep_trunk_kernel_plain_f16_four_stage_form),
                         f16 and split-pair storage of either operand.
  conv1x1_f16.hip        32 and 64 outputs, slices of 24 .. 64 channels in two buffers.  Not reached: the up-sampled addend, pooled input.
  conv1x1_ms_f16.hip     96 and 192 packed outputs, K 172 and 549.
  msblock_dil_f16.hip    the three-product one-launch group on a map smaller than its reach and on several tiles.  Not reached: score
                         fusion, split-pair input, the plain-f16 ring form (msblock_dil1_f16.hip) -- all tested in test_gpu_ops.py.
  conv3x3_c4_f16.hip     3 -> 64 and 1 -> 40 with a post affine.  Not reached: planar input, f16 output.
The pair-fused launches (conv_fused_1x1_3x3_f16.hip: the 1x1 + 3x3 pairs, the up-sampled addend, the convBlock head) have a sweep of
their own, tests/test_gpu_fused_pair_sweep.py.  Out of scope here: the 1x1 with folded pooling (conv1x1_pool_f16x3_kernel: its six builds
are value-checked against float64 by test_transition_down_pool_folded_into_the_1x1 and test_gpu_esf_encoder_tiles.py), builds behind
EGNE_* opt-in switches and debug builds.

Measured on MI355X: all 129 exact runs (43 rows x integer, fine inputs, fine weights) bit-equal on the first run, and every plan repeats its
bits -- which is also the measurement that the f16 MFMAs keep a sum of exact products exact, as the bf16 ones do
(test_gpu_conv_igemm_sweep.py), for rows whose partial sums are bounded by up to 1.2e7 units (small-wide, fine inputs).  No kernel or routing change was needed.
Normal data, relative to the largest output: three-product rows 1.3e-07 .. 7.9e-07 (bound 2e-6), one-product rows 3.2e-07 .. 3.9e-07 against the
f16-rounded operands (bound 4e-6); per row in the docstring of test_normal_data_within_the_project_bound.  The file's 172 tests take 11 s
of wall time, float64 references included (the largest, big-np1-n128, is 22 GFLOP).
"""
import numpy as np
import pytest
import torch

import split_refs as S
from test_gpu_conv_backward_fp32 import _conv_kinds
from test_gpu_conv_igemm_sweep import DEV, POISON, _slices

pytestmark = pytest.mark.gpu
BOUND3, BOUND1 = 2e-6, 4e-6        # test_gpu_ops.py: three products against float64; one product against float64 on the f16-rounded operands


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import egne_amd  # noqa: F401
    return True


@pytest.fixture(autouse=True)
def _row_switches(request):
    """engine.SMALL_ENABLED and the row's other switches hold for the row's test only."""
    from egne_amd import engine
    spec = getattr(request.node, "callspec", None)
    sw = dict(spec.params["case"]["switches"]) if spec is not None and "case" in spec.params else dict(SMALL_ENABLED=False)
    old = {k: getattr(engine, k) for k in sw}
    for k, v in sw.items():
        setattr(engine, k, v)
    yield
    for k, v in old.items():
        setattr(engine, k, v)


def _stored(out, Cout):
    Cs = S.pad8(Cout)
    o = out.float().cpu()
    assert (o[..., :8] == POISON).all() and (o[..., 8 + Cs:] == POISON).all(), "conv wrote outside its output slice"
    if Cout < Cs:
        assert (o[..., 8 + Cout:8 + Cs] == 0).all(), "padding channels must be written as zeros"
    return o[..., 8:8 + Cout].permute(0, 3, 1, 2).contiguous()


def _run(case, data, scales=None):
    """One Plan.conv of the row on ``data``, pinned to the row's kernel; runs the plan 1 + max(1, runs) times and requires identical
    bits.  ``scales``: the (a_scale, w_scale) the host test assumed, asserted after the calibrating run.  Returns the NCHW result (fp32
    on the CPU), the a_scale and w_scale of the launch."""
    from egne_amd.engine import ConvLayer, Piece, Plan
    B, H, W, Cout = case["B"], case["H"], case["W"], case["Cout"]
    pl = Plan(torch.device(DEV))
    if case["products"] == 1:
        pl.f16_products = 1
    xs = data["xs"]
    pieces = (_slices(pl, xs[:-1], B, H, W) + _slices(pl, xs[-1:], B, H, W)) if case["second_buffer"] else _slices(pl, xs, B, H, W)
    layer = ConvLayer([torch.nn.Parameter(w.to(DEV)) for w in data["ws"]], [torch.nn.Parameter(b.to(DEV)) for b in data["bs"]],
                      [(p.C, p.Cp) for p in pieces], pad=case["pad"], dils=case["dils"], act=data["act"])
    if case["one"]:
        layer.split1 = True
    else:
        layer.split = True
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
    assert (Ho, Wo) == S.out_hw(case)
    out = pl.buf(B, Ho, Wo, S.pad8(Cout) + 16)
    out.fill_(POISON)
    res = _slices(pl, [data["residual"]], B, Ho, Wo)[0] if data["residual"] is not None else None
    pl.conv(layer, pieces, Piece(out, 8, Cout), B, H, W, residual=res, name="sweep", stats=case["stats"])
    # ---- the row is about ONE kernel: its kind(s) and the entry of every launch
    kinds = _conv_kinds(pl, "sweep")
    assert kinds == [case["kind"]] * case["launches"], "%s: planned as %s" % (case["id"], kinds)
    idx = [i for i, (m, c) in enumerate(zip(pl.meta, pl.calls)) if "sweep" in c[2] and m[0].startswith("conv")]
    for i in idx:
        assert pl.calls[i][0] is getattr(pl.L, case["entry"]), "%s: launch %d is not %s" % (case["id"], i, case["entry"])
    ai = 2 if case["entry"] in S.DEEP else 3
    first = None
    for _ in range(1 + max(1, case["runs"])):
        pl.run()
        torch.cuda.synchronize()
        got = _stored(out, Cout)
        if first is None:
            first = got
            # ---- after the calibrating run: the scales the host test proved the data exact under
            a_s = {float(pl.calls[i][1][ai]) for i in idx}
            w_s = {float(getattr(ly, attr)) for ci, wi, ly, attr in pl.wscale_refs if ci in idx} | {float(pl.calls[ci][1][wi]) for ci, wi, _, _ in pl.wscale_refs if ci in idx}
            assert len(a_s) == 1 and len(w_s) == 1, (a_s, w_s)
            if scales is not None:
                assert (a_s.pop(), w_s.pop()) == tuple(scales), "%s: the launch's scales differ from the host test's %r" % (case["id"], scales)
                a_s, w_s = {scales[0]}, {scales[1]}
        else:
            assert torch.equal(got, first), "%s: a second run of the same plan gives other bits" % case["id"]
        assert pl.overflowed() is False, case["id"]
        if case["stats"]:
            # InstanceNorm statistics of the STORED output from the epilogue's partial sums (tolerances of test_conv3x3_role_split)
            scale, shift = pl.last_stats
            y = got.double()
            rstd = 1.0 / torch.sqrt(y.var((2, 3), unbiased=False) + 1e-5)
            np.testing.assert_allclose(scale.cpu().numpy()[:, :Cout], rstd.numpy(), rtol=2e-6)
            np.testing.assert_allclose(shift.cpu().numpy()[:, :Cout], (-y.mean((2, 3)) * rstd).numpy(), rtol=2e-5, atol=2e-6)
    return first, a_s.pop(), w_s.pop()


def _bit_equal(case, kind):
    data, want, a, w = S.exact_case(kind, case)
    expected = want if case["products"] == 3 else S.emulate(case, data, a, w, 1)
    got, _, _ = _run(case, data, (a, w))
    bad = (got.double() != expected)
    print("%s [%s, %s]: a_scale %g, w_scale %g, weight density %.3f, max |y| %g, %d of %d outputs differ"
          % (case["id"], case["kind"], kind, a, w, data["density"], expected.abs().max().item(), int(bad.sum()), bad.numel()))
    if bad.any():
        n, c, y, x = [int(v) for v in bad.nonzero()[0]]
        per_frame = [int(v) for v in bad.sum(dim=(1, 2, 3))]
        per_row = [int(v) for v in bad.sum(dim=(0, 1, 3))]
        raise AssertionError("%s: %d of %d outputs differ (per frame %s, per output row %s); first at n %d c %d y %d x %d: got %r, want %r"
                             % (case["id"], int(bad.sum()), bad.numel(), per_frame, per_row, n, c, y, x, got[n, c, y, x].item(), expected[n, c, y, x].item()))
    assert torch.equal(got.double(), expected)


@pytest.mark.parametrize("case", S.SPLIT_SWEEP, ids=S.SPLIT_IDS)
def test_integer_data_is_bit_equal(gpu, case):
    """(a) No lo half anywhere: torch.equal with the float64 reference, for every row."""
    _bit_equal(case, "int")


@pytest.mark.parametrize("case", S.SPLIT_SWEEP, ids=S.SPLIT_IDS)
def test_fine_inputs_are_bit_equal(gpu, case):
    """(b) Non-zero lo halves in the activations; rows with f16_products = 1 expect the convolution of the hi halves."""
    _bit_equal(case, "fine_inputs")


@pytest.mark.parametrize("case", S.SPLIT_SWEEP, ids=S.SPLIT_IDS)
def test_fine_weights_are_bit_equal(gpu, case):
    """(c) Non-zero lo halves in the weight pack."""
    _bit_equal(case, "fine_weights")


@pytest.mark.parametrize("case", S.SPLIT_SWEEP, ids=S.SPLIT_IDS)
def test_normal_data_within_the_project_bound(gpu, case):
    """(d) Seeded normal data (LeakyReLU where the row has it) against float64: 2e-6 of the largest output for three products, 4e-6
    against the f16-rounded operands for one.  Relative error on MI355X, per row:
      halo-n32 3.29e-07; halo-n64-tall 2.69e-07; halo-dil2-affine 4.80e-07; halo-n96 5.69e-07
      halo-tail16-n192 4.07e-07; halo-second-tile 4.17e-07; halo-np1 3.47e-07; rs-1x1x8 2.49e-07
      rs-1x2x8 3.32e-07; rs-2x1x4 3.49e-07; rs-2x2x4-affine 5.54e-07; rs-2x4x4 5.33e-07
      rs-second-tile 6.60e-07; rs-tpo-64-64 4.11e-07; rs-tpo-64-32-res 3.02e-07; rw-k1 3.16e-07
      rw-k2-res-post 3.76e-07; rw-3of4-second-tile 5.64e-07; rw-streamed 5.67e-07; rw-streamed-tail 5.67e-07
      rw-np1 3.17e-07; flat-256x32 2.71e-07; flat-256x64-5x5 7.91e-07; flat-128x128-dil3 3.27e-07
      flat-32taps 4.15e-07; flat-grouped 1.67e-07; flat-1x1-res 1.28e-07; small-64x64-z6 2.19e-07
      small-128x32-z3-epilogue 1.53e-07; small-wide 2.24e-07; big-n256 6.60e-07; big1 3.64e-07
      big-np1-n128 3.92e-07; s1x1-two-slices 1.82e-07; s1x1-ragged-slices 2.30e-07; ms1x1-n96 2.47e-07
      ms1x1-k549 3.71e-07; msdil-small-map 1.86e-07; msdil-tiles 2.06e-07; lattice-123 2.11e-07
      lattice-4812 2.78e-07; first-3-64 1.40e-07; first-1-40-post 1.60e-07"""
    data = S.normal_case(torch.Generator().manual_seed(4321), case)
    got, a, w = _run(case, data)
    want = S.ref_of(case, data) if case["products"] == 3 else S.emulate(case, data, a, w, 1)
    err = (got.double() - want).abs().max().item() / want.abs().max().item()
    bound = BOUND3 if case["products"] == 3 else BOUND1
    print("%s [%s]: relative error %.2e (bound %.0e), a_scale %g, w_scale %g" % (case["id"], case["kind"], err, bound, a, w))
    assert err < bound, "%s: relative error %.2e" % (case["id"], err)
