"""-m gpu: sweep of the pair-fused split-f16 launches (conv_fused_1x1_3x3_f16.hip behind Plan.conv_pair: the 1x1 + 3x3 pairs of ESF-Net's
dense and up blocks, the latter with the folded up-sampled addend, and the convBlock head) on data for which they must be BIT-EQUAL to
float64.

Every row of fused_refs.FUSED_SWEEP is pinned to ONE of the 34 template instantiations <NCH, WN, TH, NB, C4, UPADD, UNI, GL, C1V> the
launchers can choose: before anything runs the plan must hold one convolution launch (plus the statistics launch a row asks for), of the
expected _lib entry and Plan.meta kind, and the launch rule restated in fused_refs.launch_form, applied to the launch's two descriptors,
must name the row's build.  Each row then goes through Plan.conv_pair five times:

(a) int      small integers: no lo half in either stage -- hi addressing of slices, tail groups, far frames, tiles, the epilogue;
(b) fine_x   inputs of 12 to 13 significant bits, integer weights: lo halves in the inputs AND in the intermediate held in LDS;
(c) fine_w1  integer inputs, 12-bit first weights: the lo half of the first pack, lo halves in the intermediate;
(d) fine_w2  tiny integers in front of 12-bit second weights: the lo half of the second pack;
(e) seeded normal data, LeakyReLU where the row has an activation, under the bound the project holds for this kernel: 3e-6 of the largest
    output against float64 (test_gpu_ops.py: test_conv1x1_3x3_fused, test_convblock_pair_fused).

In (a) .. (d) every product and every partial sum of both stages is an fp32 value and t * a2 splits into two normal f16 halves
(tests/test_host_fused_refs.py proves it per row and run on the CPU, under the four scales asserted here after the calibrating run),
so the result is torch.equal to the reference whatever the order of summation, and the InstanceNorm statistics from the epilogue are
those of the reference.  Every plan runs three times and must repeat its bits; Plan.overflowed() stays false.  Every input slice sits
between eight poisoned channels on either side, far slices are Piece.samples(B) of a 2B-sample buffer whose first half is poisoned,
the up-sampled addend P is a slice of a wider half-resolution buffer between poison, the planar input sits between poisoned floats,
the output between two poisoned blocks, the residual in a slice of its own buffer; padding channels of the output slice must come
back as zeros and all poison must be intact.

Builds reached (all 34; fused_refs.REQUIRED):
  32-channel intermediate   UNI straight-line G = 4 / 6 / 8; UNI generic and non-UNI, WN 1 and 2, NB 1, 2, 3 (G up to 12; tail groups of 24-
                            and 40-channel slices; 30-channel intermediate; 30 and 38 outputs: the epilogue's edge path)
  64-channel intermediate   UNI G = 7 / 11 straight-line; UNI generic NB 2, 4, 6; the non-UNI build WN 1 and 2, NB 2, 4, 6 (one row with one
                            buffer and 32 outputs); 62-channel intermediate and output
  UPADD                     UNI G = 4 / 6 straight-line, UNI generic NB 1 and 2, non-UNI NB 1 and 2; maps 2 (13 x 17), 16 x 64, 72 x 320
  convBlock                 C1V on the planar input; the MFMA form on 2, 3, 4 NHWC channels and on the planar input (engine.C1V off)
  Tile dealing: one tile per workgroup by stride (12 tiles), a map smaller than a tile, W = 32 with H = TH, and 270 tiles over 256
  workgroups (8-row and 4-row tiles, UPADD, C1V): the second LDS image, the prefetch wrapping into the next tile, the weight ring.
Not reached: builds behind EGNE_* opt-in switches, egne_fused_debug.

Measured on MI355X: all 152 exact runs (38 rows x int, fine_x, fine_w1, fine_w2) bit-equal on the first run, with partial sums bounded by up
to 1.67e7 units (uni64-g7-gl1-big, fine_w2); statistics equal to those of the reference within the tolerances, every plan repeats its
bits, poison and padding intact.  No kernel or launcher change was needed.  Normal data, relative to the largest output (bound 3e-6):
32-channel intermediate 2.3e-07 .. 4.3e-07, 64-channel intermediate 3.7e-07 .. 5.8e-07, UPADD 3.0e-07 .. 4.0e-07, convBlock 1.2e-07 ..
4.2e-07; per row in the docstring of test_normal_data_within_the_project_bound.  The file's 190 tests take 7 s of wall time, float64
references included.
"""
import numpy as np
import pytest
import torch

import fused_refs as R
from test_gpu_conv_backward_fp32 import _conv_kinds
from test_gpu_conv_igemm_sweep import DEV, POISON

pytestmark = pytest.mark.gpu
BOUND = 3e-6          # test_gpu_ops.py: test_conv1x1_3x3_fused and test_convblock_pair_fused hold this bound as a literal in their bodies
RUNS_PER_PLAN = 3     # the calibrating run and two replays


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import egne_amd  # noqa: F401
    return True


def _in_buffer(pl, xs, B, H, W, far=None):
    """NCHW CPU tensors -> slices of ONE NHWC buffer, each between eight poisoned channels.  ``far``: the slices from that index on are
    Piece.samples(B) of a buffer of 2B samples; what frame b of those channel ranges holds is poison."""
    from egne_amd.engine import Piece
    buf = pl.buf(2 * B if far is not None else B, H, W, 8 + sum(R.pad8(x.shape[1]) + 8 for x in xs))
    buf.fill_(R.IN_POISON)
    pieces, off = [], 8
    for i, x in enumerate(xs):
        c, n0 = x.shape[1], B if far is not None and i >= far else 0
        buf[n0:n0 + B, ..., off:off + R.pad8(c)] = 0
        buf[n0:n0 + B, ..., off:off + c] = x.permute(0, 2, 3, 1).to(DEV)
        pieces.append(Piece(buf, off, c).samples(n0) if n0 else Piece(buf, off, c))
        off += R.pad8(c) + 8
    return buf, pieces


def _intact(buf, pieces, B):
    """Everything of an input buffer outside its slices still holds the poison."""
    keep = torch.ones_like(buf, dtype=torch.bool)
    for p in pieces:
        keep[p.n0:p.n0 + B, ..., p.off:p.off + p.Cp] = False
    return bool((buf[keep] == R.IN_POISON).all())


def _run(row, data, scales=None, want=None):
    """One Plan.conv_pair of the row on ``data``, pinned to the row's build; runs the plan RUNS_PER_PLAN times and requires identical bits,
    intact poison, zero padding channels and no overflow.  ``scales``: the (a1, w_scale1, a2, w_scale) the host test assumed, asserted
    after the calibrating run.  ``want``: the float64 reference the statistics are compared with (the stored tensor otherwise).
    Returns the NCHW result (fp32 on the CPU) and the launch's four scales."""
    from egne_amd import engine
    from egne_amd.engine import ConvLayer, Piece, PlanarPiece, Plan
    B, H, W, C1, C2 = row["B"], row["H"], row["W"], row["C1"], row["C2"]
    c4 = row["kind"] == "c4"
    pl = Plan(torch.device(DEV))
    guards = []            # (buffer, pieces) of the NHWC inputs; the planar input's guard floats
    if c4 and row["planar"]:
        n = B * H * W
        flat = torch.full((n + 32,), R.IN_POISON, device=DEV)
        flat[16:16 + n] = data["xs"][0].reshape(-1).to(DEV)
        pl.keep.append(flat)
        pieces = [PlanarPiece(flat[16:16 + n].view(B, 1, H, W))]
    elif c4:
        buf, pieces = _in_buffer(pl, data["xs"], B, H, W)
        guards.append((buf, pieces))
    else:
        cut = row["split"] if row["split"] is not None else len(data["xs"])
        pieces = []
        for part, far in ((data["xs"][:cut], row["far"]), (data["xs"][cut:], None)):
            if part:
                buf, ps = _in_buffer(pl, part, B, H, W, far)
                guards.append((buf, ps))
                pieces += ps
    par = lambda t: torch.nn.Parameter(t.to(DEV))      # noqa: E731
    l1 = ConvLayer([par(data["w1"])], [par(data["b1"])], [(p.C, p.Cp) for p in pieces], pad=(1, 1) if c4 else (0, 0), act=data["act1"])
    l2 = ConvLayer([par(data["w2"])], [par(data["b2"])], [(C1, R.pad8(C1))], pad=(1, 1), act=data["act"])
    l1.split = l1.split1 = l2.split = True
    if data["post"] is not None:
        ps, pt = torch.zeros(l2.CoutP, device=DEV), torch.zeros(l2.CoutP, device=DEV)
        ps[:C2], pt[:C2] = data["post"][0].to(DEV), data["post"][1].to(DEV)
        l2.post = (ps, pt)
    Cs = R.pad8(C2)
    out = pl.buf(B, H, W, Cs + 16)
    out.fill_(POISON)
    res = None
    if data["residual"] is not None:
        rbuf, (res,) = _in_buffer(pl, [data["residual"]], B, H, W)
        guards.append((rbuf, [res]))
    up = pbuf = None
    if data["P"] is not None:
        pbuf = pl.buf(B, H // 2, W // 2, 48)
        pbuf.fill_(R.IN_POISON)
        pbuf[..., 8:40] = data["P"].permute(0, 2, 3, 1).to(DEV)
        up = (Piece(pbuf, 8, 32), H // 2, W // 2)
    old = engine.FUSE_1X1_MIN_W, engine.C1V
    engine.FUSE_1X1_MIN_W, engine.C1V = 0, row["c1v"]
    try:
        pl.conv_pair(l1, pieces, l2, Piece(out, 8, C2), B, H, W, residual=res, name="sweep", stats=row["stats"], up_add=up)
    finally:
        engine.FUSE_1X1_MIN_W, engine.C1V = old
    # ---- the row is about ONE build: one launch of the entry (+ the statistics launch), its kind, and the launcher's rule on its descriptors
    assert len(pl.calls) == 1 + int(row["stats"]), "%s: %d launches" % (row["id"], len(pl.calls))
    assert pl.calls[0][0] is getattr(pl.L, R.ENTRY[row["kind"]]), row["id"]
    assert not row["stats"] or pl.calls[1][0] is pl.L.egne_norm_stats_finish, row["id"]
    assert _conv_kinds(pl, "sweep") == [R.KIND[row["kind"]]] and pl.meta[0][0] == R.KIND[row["kind"]], pl.meta
    args = pl.calls[0][1]
    d1, d2 = args[0]._obj, args[1]._obj
    facts, dn = R.launch_facts(d1, d2, c4)
    assert R.launch_form(**facts) == row["form"], "%s: the launcher takes %s for %s" % (row["id"], R.launch_form(**facts), facts)
    assert dn == (B if row["far"] is not None else 0), (row["id"], dn)
    if row["stats"]:
        assert int(d2.stats_nchunk) == R.stats_nchunk(row), row["id"]
    first = got_scales = None
    for _ in range(RUNS_PER_PLAN):
        pl.run()
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[..., :8] == POISON).all() and (o[..., 8 + Cs:] == POISON).all(), "%s: stores outside the output slice" % row["id"]
        if C2 < Cs:
            assert (o[..., 8 + C2:8 + Cs] == 0).all(), "%s: padding channels must be written as zeros" % row["id"]
        got = o[..., 8:8 + C2].permute(0, 3, 1, 2).contiguous()
        for buf, ps in guards:
            assert _intact(buf, ps, B), "%s: poison around an input slice was overwritten" % row["id"]
        if pbuf is not None:
            assert (pbuf[..., :8] == R.IN_POISON).all() and (pbuf[..., 40:] == R.IN_POISON).all()
        if c4 and row["planar"]:
            assert (flat[:16] == R.IN_POISON).all() and (flat[-16:] == R.IN_POISON).all()
        if first is None:
            first = got
            # ---- after the calibrating run: the scales the host test proved the data exact under
            args = pl.calls[0][1]
            got_scales = tuple(float(args[i]) for i in (4, 5, 8, 9))
            assert got_scales[1] == float(getattr(l1, "w_scale_c4" if c4 else "w_scale1")) and got_scales[3] == float(l2.w_scale)
            if scales is not None:
                assert got_scales == tuple(scales), "%s: the launch's scales %r differ from the host test's %r" % (row["id"], got_scales, scales)
        else:
            assert torch.equal(got, first), "%s: a second run of the same plan gives other bits" % row["id"]
        assert pl.overflowed() is False, row["id"]
        if row["stats"]:
            # InstanceNorm statistics from the epilogue's fp64 partial sums (tolerances of test_conv3x3_role_split): of the REFERENCE on
            # exact data, which the stored tensor must equal; of the stored tensor on normal data
            scale, shift = pl.last_stats
            rstd, sh = R.stats_of(want if want is not None else got)
            np.testing.assert_allclose(scale.cpu().numpy()[:, :C2], rstd.numpy(), rtol=2e-6)
            np.testing.assert_allclose(shift.cpu().numpy()[:, :C2], sh.numpy(), rtol=2e-5, atol=2e-6)
    return first, got_scales


def _bit_equal(row, run):
    data, want, scales = R.exact_case(row, run)
    got, _ = _run(row, data, scales, want)
    bad = (got.double() != want)
    print("%s %s [%s]: scales %s, weight densities %s, max |y| %g, %d of %d outputs differ"
          % (row["id"], R.form_name(row["form"]), run, scales, data["density"], want.abs().max().item(), int(bad.sum()), bad.numel()))
    if bad.any():
        n, c, y, x = [int(v) for v in bad.nonzero()[0]]
        per_frame = [int(v) for v in bad.sum(dim=(1, 2, 3))]
        per_row = [int(v) for v in bad.sum(dim=(0, 1, 3))]
        raise AssertionError("%s %s: %d of %d outputs differ (per frame %s, per output row %s); first at n %d c %d y %d x %d: got %r, want %r"
                             % (row["id"], run, int(bad.sum()), bad.numel(), per_frame, per_row, n, c, y, x, got[n, c, y, x].item(), want[n, c, y, x].item()))
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("row", R.FUSED_SWEEP, ids=R.FUSED_IDS)
def test_integer_data_is_bit_equal(gpu, row):
    """(a) No lo half anywhere: torch.equal with the float64 reference, for every row."""
    _bit_equal(row, "int")


@pytest.mark.parametrize("row", R.FUSED_SWEEP, ids=R.FUSED_IDS)
def test_fine_inputs_are_bit_equal(gpu, row):
    """(b) Non-zero lo halves in the inputs and in the intermediate."""
    _bit_equal(row, "fine_x")


@pytest.mark.parametrize("row", R.FUSED_SWEEP, ids=R.FUSED_IDS)
def test_fine_first_weights_are_bit_equal(gpu, row):
    """(c) Non-zero lo halves in the first weight pack (the fp32 table of the C1V build) and in the intermediate."""
    _bit_equal(row, "fine_w1")


@pytest.mark.parametrize("row", R.FUSED_SWEEP, ids=R.FUSED_IDS)
def test_fine_second_weights_are_bit_equal(gpu, row):
    """(d) Non-zero lo halves in the second weight pack."""
    _bit_equal(row, "fine_w2")


@pytest.mark.parametrize("row", R.FUSED_SWEEP, ids=R.FUSED_IDS)
def test_normal_data_within_the_project_bound(gpu, row):
    """(e) Seeded normal data (LeakyReLU where the row has an activation) against float64: 3e-6 of the largest output.  Relative error on
    MI355X, per row:
      uni-g4-gl4-big 4.28e-07; uni-g6-gl2-far 3.42e-07; uni-g8-gl4 3.40e-07; uni-1-nb1-tiny 2.28e-07; uni-1-nb2-aligned 3.42e-07
      uni-1-nb3 3.72e-07; uni-2-nb1 3.46e-07; uni-2-nb2 3.79e-07; uni-2-nb3 3.85e-07; sep-1-nb1 3.36e-07; sep-1-nb2 3.18e-07
      sep-1-nb3 3.62e-07; sep-2-nb1 2.97e-07; sep-2-nb2 3.63e-07; sep-2-nb3 4.27e-07; uni64-g7-gl1-big 5.44e-07
      uni64-g11-gl1-far 4.95e-07; uni64-nb2 3.68e-07; uni64-nb4 4.16e-07; uni64-nb6 5.84e-07; n64-1-nb2-one-buffer 4.19e-07
      n64-1-nb4 4.22e-07; n64-1-nb6 4.17e-07; n64-2-nb2 5.28e-07; n64-2-nb4 5.05e-07; n64-2-nb6 5.09e-07; up-g4-gl4 3.11e-07
      up-g6-gl2-aligned 2.99e-07; up-uni-nb1 3.11e-07; up-uni-nb2-big 4.01e-07; up-sep-nb1 3.20e-07; up-sep-nb2-aligned 3.26e-07
      c4-planar-c1v 4.20e-07; c4-planar-c1v-big 4.04e-07; c4-nhwc-2 3.00e-07; c4-nhwc-3 2.85e-07; c4-nhwc-4 1.19e-07
      c4-planar-mfma 2.68e-07"""
    data = R.normal_data(torch.Generator().manual_seed(4321 + R.FUSED_IDS.index(row["id"])), row)
    got, scales = _run(row, data)
    want = R.reference(row, data)
    err = (got.double() - want).abs().max().item() / want.abs().max().item()
    print("%s %s: relative error %.2e (bound %.0e), scales %s" % (row["id"], R.form_name(row["form"]), err, BOUND, scales))
    assert err < BOUND, "%s: relative error %.2e" % (row["id"], err)
