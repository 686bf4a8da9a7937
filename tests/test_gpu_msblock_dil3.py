"""msblock_dil3_f16.hip: the dilated group of an MSBlock (bdcn_new.py:49-55) on split-pair input with three f16 products, every tap read
from a ring of phase-plane rows in LDS.  The yardstick is the strip kernel it replaces (msdil_ps_kernel, EGNE_MSDIL3=0): the two forms
must agree BIT for bit -- block output (a 40-channel buffer, slice at offset 8, poison around it) and fused score maps (pre-filled
s0 / s1, both accumulate values) -- the new form must repeat its own bits, and both stay within the project's three-product bound
against float64 (2e-6 of the largest output: test_gpu_ops.py, test_gpu_split_f16_sweep.py BOUND3).

Shapes, the smallest that reach each path (planes are the 16 residue classes (y mod 4, x mod 4); a work item is 32 plane columns wide
and walks down in steps of 8 plane rows through a ring of 24):
  48x64   B=1    planes 12x16: one column with an empty second pixel block, a partial last step
  50x67   B=2    unequal planes (13x17 next to 12x16): a 17-wide column next to 16-wide ones
  49x140  B=1    plane width 35: a second, narrower plane column
  120x72  B=3    plane height 30: four steps, the ring wraps
  96x128  B=18   288 work items for 256 workgroups
  200x64  B=1    EGNE_MSDIL3_SEGS=2: plane height 50 cut into 32 + 18 rows, the second segment warms up inside the plane
  130x70  B=2    EGNE_MSDIL3_SEGS=3: 16 + 16 + 1 rows
MI355X: both forms equal in every case; against float64 2.2e-07 .. 6.2e-07 of the largest output (bound 2e-6); the file's 23 tests take 3 s."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND3 = 2e-6          # three products against float64, relative to the largest output (test_gpu_split_f16_sweep.py)
CIN = 64
PRE0, PRE1 = 1.5, -0.75

SHAPES = [(1, 48, 64, 0), (2, 50, 67, 0), (1, 49, 140, 0), (3, 120, 72, 0), (18, 96, 128, 0), (1, 200, 64, 2), (2, 130, 70, 3)]
MODES = ["out", "scores", "scores_acc"]


@pytest.fixture(scope="module")
def dev():
    from gpu_util import DEV
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return DEV


_REF = {}


def _case(dev, B, H, W):
    """Inputs and the float64 results of one shape: computed once, shared by the modes, never modified."""
    key = (B, H, W)
    if key not in _REF:
        g = torch.Generator().manual_seed(2031 + 7 * B + 3 * H + W)
        rnd = lambda *s: torch.randn(*s, generator=g)
        x = F.relu(rnd(B, CIN, H, W)) * 2
        w0, b0 = rnd(32, CIN, 3, 3) / (3 * CIN ** 0.5), rnd(32)
        ws = [rnd(32, 32, 3, 3) / 17 for _ in range(3)]
        bs = [rnd(32) for _ in range(3)]
        cw, cc = rnd(2, 32) / 6, torch.tensor([0.7, -1.3])
        o = F.relu(F.conv2d(x.double().to(dev), w0.double().to(dev), b0.double().to(dev), padding=1))
        blk = o.clone()
        for w, b, d in zip(ws, bs, (4, 8, 12)):
            blk = blk + F.relu(F.conv2d(o, w.double().to(dev), b.double().to(dev), padding=d, dilation=d))
        lin = torch.stack([(blk * cw[h].double().to(dev)[None, :, None, None]).sum(1) for h in range(2)], 1)
        pre = torch.tensor([PRE0, PRE1], dtype=torch.float64, device=dev)[None, :, None, None]
        truth = {"out": blk, "scores": lin + cc.double().to(dev)[None, :, None, None], "scores_acc": lin + pre}
        _REF[key] = (x, w0, b0, ws, bs, cw, cc, truth)
    return _REF[key]


def _run_form(dev, monkeypatch, form, segs, B, H, W, mode):
    """One plan (resident-weights 3x3 that writes split-pair o, then the dilated group) under EGNE_MSDIL3 = form: the result of the
    second and of the third run."""
    from gpu_util import to_nhwc_buf
    from egne_amd import engine
    from egne_amd.engine import ConvLayer, Piece, Plan, SplitScale, pad8
    x, w0, b0, ws, bs, cw, cc, _ = _case(dev, B, H, W)
    # (one or two small frames would put the producer on the small-problem form of the flat kernel, which writes no split pairs)
    monkeypatch.setattr(engine, "SMALL_ENABLED", False)
    monkeypatch.setenv("EGNE_MSDIL3", form)
    if segs:
        monkeypatch.setenv("EGNE_MSDIL3_SEGS", str(segs))
    else:
        monkeypatch.delenv("EGNE_MSDIL3_SEGS", raising=False)
    pl = Plan(torch.device(dev))
    (px,) = to_nhwc_buf(pl, [x], B, H, W)
    l0 = ConvLayer([torch.nn.Parameter(w0.to(dev))], [torch.nn.Parameter(b0.to(dev))], [(CIN, pad8(CIN))], pad=(1, 1), act=1)
    lg = ConvLayer([torch.nn.Parameter(w.to(dev)) for w in ws], [torch.nn.Parameter(b.to(dev)) for b in bs], [(32, 32)],
                   pad=(1, 1), dils=(4, 8, 12), act=1)
    l0.split = lg.split = True
    obuf = pl.buf(B, H, W, 32)
    po = Piece(obuf, 0, 32)
    assert pl.msdil_ok(lg, po, H, W)
    po.presplit = SplitScale()
    pl.conv(l0, [px], po, B, H, W)
    assert pl.last_presplit, "the resident-weights 3x3 writes split-pair storage"
    s0 = s1 = out = None
    if mode == "out":
        out = pl.buf(B, H, W, 40)
        pl.conv(lg, [po], Piece(out, 8, 32), B, H, W, residual=po)
    else:
        s0, s1 = pl.vec(B, H, W), pl.vec(B, H, W)
        cwd, ccd = cw.to(dev), cc.to(dev)
        pl.keep += [cwd, ccd]
        pl.conv(lg, [po], po, B, H, W, residual=po, scores=(cwd, ccd, s0, s1, mode == "scores_acc"))
    assert pl.meta[-1][0] == "conv_f16x3:msdil"
    res = []
    for _ in range(3):          # calibrating run, then two replays
        if out is not None:
            out.fill_(777.0)
        else:
            s0.fill_(PRE0); s1.fill_(PRE1)
        pl.run()
        torch.cuda.synchronize()
        if out is not None:
            assert (out[..., :8] == 777.0).all(), "stores outside the output slice"
            res.append(out[..., 8:].permute(0, 3, 1, 2).clone())
        else:
            res.append(torch.stack([s0, s1], 1).clone())
    return res[1], res[2]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,segs", SHAPES)
def test_phase_plane_ring_equals_the_strip_kernel(dev, B, H, W, segs, mode, monkeypatch):
    """EGNE_MSDIL3=1 against EGNE_MSDIL3=0 in one process: equal bits, repeatable bits, both within 2e-6 of float64."""
    truth = _case(dev, B, H, W)[-1][mode]
    ring, ring2 = _run_form(dev, monkeypatch, "1", segs, B, H, W, mode)
    strip, _ = _run_form(dev, monkeypatch, "0", segs, B, H, W, mode)
    scale = truth.abs().max().item()
    errs = [(r.double() - truth).abs().max().item() / scale for r in (ring, strip)]
    print("MSBlock dilated group %dx%dx%d segs %d %s: ring %.2e strip %.2e of the largest output, forms differ by %.3e"
          % (B, H, W, segs, mode, errs[0], errs[1], (ring - strip).abs().max().item()))
    assert torch.equal(ring, strip), "ring and strip forms differ: max %.3e" % (ring - strip).abs().max().item()
    assert torch.equal(ring, ring2), "the ring form does not repeat its own bits"
    assert errs[0] < BOUND3 and errs[1] < BOUND3, errs


@pytest.mark.parametrize("mode", ["out", "scores"])
def test_maps_below_the_floor_stay_on_the_strip_kernel(dev, mode, monkeypatch):
    """30x40 (stage 4 of the edge network at 240x320) is below the 48x64 floor: the switch changes nothing."""
    from egne_amd import engine
    monkeypatch.setattr(engine, "RS_MIN_W", 30)          # a resident-weights producer (split-pair o) on a map this narrow
    a, _ = _run_form(dev, monkeypatch, "1", 0, 2, 30, 40, mode)
    b, _ = _run_form(dev, monkeypatch, "0", 0, 2, 30, 40, mode)
    assert torch.equal(a, b)
    truth = _case(dev, 2, 30, 40)[-1][mode]
    assert (a.double() - truth).abs().max().item() / truth.abs().max().item() < BOUND3
