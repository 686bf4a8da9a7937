"""Rows, exactly representable data, a float64 reference, the restated launch rule and CPU emulations for the pair-fused split-f16
launches: conv_fused_1x1_3x3_f16.hip behind Plan.conv_pair -- 3x3(1x1(cat(slices)) + b1 [+ up(P)]) with the intermediate in LDS only
(egne_conv1x1_3x3_fused_f16_fwd), and the convBlock head 3x3(act(3x3(x))) on <= 4 input channels (egne_conv3x3c4_3x3_fused_f16_fwd).

Both stages are split-f16 products (split_refs.py): stage 1 multiplies x * a1 by w1 * w_scale1, stage 2 multiplies the INTERMEDIATE
t * a2 -- split into f16 halves when it is written to the LDS image -- by w2 * w_scale; each drops its lo*lo product.  (The C1V build
computes stage 1 in fp32 fused multiply-adds instead.)  When in each stage one operand has no lo half at all, every scaled operand
equals hi + lo and every partial sum stays below 2^24 units of the smallest product, nothing is rounded anywhere and the launch must
reproduce ``reference`` BIT FOR BIT.  Four generators make such data per row (``RUNS``):

  int       small integers everywhere: t has at most 11 bits, no lo half in either stage;
  fine_x    inputs of 12 to 13 significant bits against integer weights: lo halves in x and in t;
  fine_w1   integer inputs against 12-bit w1: lo halves in the first weight pack and in t;
  fine_w2   tiny integers in front of 12-bit w2: t has no lo half, the second weight pack has.

a2 comes from a BOUND on t (max |x| * max_co sum |w1| + max |b1| [+ max |P|]), not from max |t|, so the halves of t * a2 sit lower than
those of a measured operand; ``conditions`` asserts that they are still two normal f16 values.  ``fused_form`` restates which of the 34
template instantiations <NCH, WN, TH, NB, C4, UPADD, UNI, GL, C1V> a launch takes (``REQUIRED``), ``emulate`` restates the arithmetic
in float64, ``wrong`` restates seven mistakes a kernel could make (tests/test_host_fused_refs.py shows on the CPU that the data tells
each of them from the reference); ``FUSED_SWEEP`` is the table tests/test_gpu_fused_pair_sweep.py runs.
"""
import math

import torch
import torch.nn.functional as F

from conv_refs import ACT_LEAKY, ACT_NONE, ACT_RELU, D, FP32_EXACT, _ints, _pow2, _weights, act_ref, pad8, pad32
from split_refs import LO_DENSITY, a_scale_for, granule, split_f16, w_scale_for

TW = 32                       # tile width of the fused kernel; the tile height is the TH of the row's build
MAX_GRID = 256                # workgroups of a launch: more tiles than this and workgroups walk several
IN_POISON = 2.0 ** 30         # around every input slice: under any a1 of these rows it leaves the f16 range (see wrong: tail_upper)
RUNS = ("int", "fine_x", "fine_w1", "fine_w2")
ENTRY = {"pair": "egne_conv1x1_3x3_fused_f16_fwd", "c4": "egne_conv3x3c4_3x3_fused_f16_fwd"}
KIND = {"pair": "conv_f16x3:fused1x1", "c4": "conv_f16x3:fused3x3c4"}


# ---- the launch rule ---------------------------------------------------------------------------------------------------------------

def form(nch, wn, th, nb, *flags):
    """<NCH, WN, TH, NB, C4, UPADD, UNI, GL, C1V> from <NCH, WN, TH, NB> and the flags that are set ("GL4": GL = 4)."""
    gl = [int(f[2:]) for f in flags if f.startswith("GL")]
    assert all(f in ("C4", "UPADD", "UNI", "C1V") or f.startswith("GL") for f in flags) and len(gl) <= 1
    return (nch, wn, th, nb, "C4" in flags, "UPADD" in flags, "UNI" in flags, gl[0] if gl else 0, "C1V" in flags)


def form_name(f):
    """'<1,1,8,2 UNI GL4>': the four sizes and the flags that are set."""
    flags = [n for n, on in zip(("C4", "UPADD", "UNI"), f[4:7]) if on] + (["GL%d" % f[7]] if f[7] else []) + (["C1V"] if f[8] else [])
    return "<%d,%d,%d,%d%s>" % (f[:4] + ("".join(" " + n for n in flags),))


def launch_form(G, uni, c1p, c2p, upadd, c4=False, c1v=False):
    """The instantiation the two launchers at the end of conv_fused_1x1_3x3_f16.hip choose.  G: 16-channel groups over all slices;
    uni: every slice is a channel range of seg[0]'s buffer; c1p / c2p: d1.CoutP / d2.CoutP; upadd: d1.residual is set;
    c4: the convBlock entry, c1v: its input is planar and d1.w carries the fp32 weight table."""
    if c4:
        return form(1, 1, 8, 1, "C4", "GL3", *(["C1V"] if c1v else []))
    assert 1 <= G <= 12 and c1p in (32, 64) and c2p in (32, 64)
    u = ["UNI"] if uni else []
    if upadd:
        assert c1p == 32 and c2p == 32 and G <= 8
        if uni and G in (4, 6):
            return form(1, 1, 8, 1, "UPADD", "UNI", "GL4") if G == 4 else form(1, 1, 8, 2, "UPADD", "UNI", "GL2")
        return form(1, 1, 8, 1 if G <= 4 else 2, "UPADD", *u)
    if c1p == 32:
        if uni and c2p == 32 and G in (4, 6, 8):
            return form(1, 1, 8, 1 if G == 4 else 2, "UNI", "GL2" if G == 6 else "GL4")
        return form(1, c2p // 32, 8, (G + 3) // 4, *u)
    nb2 = ((G + 1) // 2 + 1) // 2 * 2
    if uni and c2p == 64:
        return form(2, 2, 4, nb2, "UNI", *(["GL1"] if G in (7, 11) else []))
    return form(2, c2p // 32, 4, nb2)          # the non-UNI build, one buffer with 32 outputs included


REQUIRED = frozenset(
    [form(1, 1, 8, 1, "UNI", "GL4"), form(1, 1, 8, 2, "UNI", "GL2"), form(1, 1, 8, 2, "UNI", "GL4")]
    + [form(1, wn, 8, nb, *u) for wn in (1, 2) for nb in (1, 2, 3) for u in (["UNI"], [])]
    + [form(2, 2, 4, 4, "UNI", "GL1"), form(2, 2, 4, 6, "UNI", "GL1")]
    + [form(2, 2, 4, nb, "UNI") for nb in (2, 4, 6)]
    + [form(2, wn, 4, nb) for wn in (1, 2) for nb in (2, 4, 6)]
    + [form(1, 1, 8, 1, "UPADD", "UNI", "GL4"), form(1, 1, 8, 2, "UPADD", "UNI", "GL2")]
    + [form(1, 1, 8, nb, "UPADD", *u) for nb in (1, 2) for u in (["UNI"], [])]
    + [form(1, 1, 8, 1, "C4", "GL3"), form(1, 1, 8, 1, "C4", "GL3", "C1V")])


def groups_of(chans):
    return sum((pad8(c) + 15) // 16 for c in chans)


def fused_form(row):
    """The instantiation the row's launch takes, from the row alone."""
    if row["kind"] == "c4":
        return launch_form(0, False, 32, 32, False, c4=True, c1v=row["planar"] and row["c1v"])
    return launch_form(groups_of(row["chans"]), row["split"] is None, pad32(row["C1"]), pad32(row["C2"]), row["up"])


def launch_facts(d1, d2, c4):
    """What launch_form needs, read off the two descriptors of an actual launch as the launcher reads it; + ``dn``, the common frame
    distance of the far slices."""
    segs = [d1.seg[s] for s in range(d1.nseg)]
    if c4:
        return dict(G=0, uni=False, c1p=int(d1.CoutP), c2p=int(d2.CoutP), upadd=False, c4=True,
                    c1v=segs[0].pix_stride == 1 and bool(d1.w) and d1.w % 16 == 0), 0
    uni, dn = True, 0
    fbytes = d1.H * d1.W * segs[0].pix_stride * 4
    for g in segs:
        delta = g.ptr - segs[0].ptr
        if g.pix_stride != segs[0].pix_stride or delta < 0 or delta % fbytes != 0:
            uni = False
        elif delta > 0:
            if dn not in (0, delta // fbytes):
                uni = False
            else:
                dn = delta // fbytes
    return dict(G=sum((g.Cp + 15) // 16 for g in segs), uni=uni, c1p=int(d1.CoutP), c2p=int(d2.CoutP), upadd=bool(d1.residual)), dn


def tiles_of(row):
    """(TH, tiles_x, tiles_y, tiles of the launch)."""
    th = row["form"][2]
    tx, ty = (row["W"] + TW - 1) // TW, (row["H"] + th - 1) // th
    return th, tx, ty, tx * ty * row["B"]


def tile_walk(row):
    """Per workgroup the tiles it walks, as (frame, y0, x0): the kernel's tile_at / decode.  A grid that is a multiple of 8 deals runs of
    grid / 8 consecutive tiles to the workgroups of one XCD, any other grid deals by stride."""
    th, tx, ty, n = tiles_of(row)
    grid = min(MAX_GRID, n)
    per, walks = grid >> 3, []
    for b in range(grid):
        mine, i = [], 0
        while True:
            t = b + i * grid if grid & 7 else (i * 8 + (b & 7)) * per + (b >> 3)
            if t >= n:
                break
            mine.append((t // (tx * ty), (t // tx) % ty * th, t % tx * TW))
            i += 1
        walks.append(mine)
    assert sorted(t for w in walks for t in w) == sorted((f, y * th, x * TW) for f in range(row["B"]) for y in range(ty) for x in range(tx))
    return walks


def stats_nchunk(row):
    """The launcher's rule: partial sums per tile -- 2 for 64 -> 64 channels, 4 otherwise."""
    _, tx, ty, _ = tiles_of(row)
    return tx * ty * (2 if (row["kind"] == "pair" and pad32(row["C1"]) == 64 and pad32(row["C2"]) == 64) else 4)


# ---- the table ---------------------------------------------------------------------------------------------------------------------

def _p(id, B, H, W, chans, C1, C2, fm, split=None, far=None, up=False, act=ACT_NONE, post=False, residual=False, stats=False):
    """A 1x1 + 3x3 row.  chans: logical widths of the input slices; ``split``: index of the first slice that lives in a second buffer
    (None: one buffer); ``far``: index of the first slice given as Piece.samples(B) of a 2B-sample buffer; ``up``: an up-sampled
    half-resolution addend; ``fm``: the instantiation the row is about."""
    return dict(id=id, kind="pair", B=B, H=H, W=W, chans=tuple(chans), C1=C1, C2=C2, form=fm, split=split, far=far, up=up, act=act, act1=ACT_NONE,
                post=post, residual=residual, stats=stats, planar=False, c1v=True)


def _c4(id, B, H, W, cin, fm, planar=False, c1v=True, C1=32, C2=32, act=ACT_LEAKY, act1=ACT_LEAKY, post=False, residual=False, stats=False):
    """A convBlock row: 3x3 on ``cin`` <= 4 channels (NHWC slice of Cp 8, or the planar one-channel tensor) in front of the 3x3."""
    return dict(id=id, kind="c4", B=B, H=H, W=W, chans=(cin,), C1=C1, C2=C2, form=fm, split=None, far=None, up=False, act=act, act1=act1,
                post=post, residual=residual, stats=stats, planar=planar, c1v=c1v)


_M8, _M4 = (2, 19, 45), (2, 11, 45)            # default maps, ragged in x and y: 12 tiles each, dealt by stride
_BIG8, _BIG4 = (3, 72, 320), (2, 36, 480)      # 270 tiles over 256 workgroups (a multiple of 8): 14 workgroups walk a second tile
_UP = (2, 26, 34)                              # 2 x (13 x 17): odd half size, ragged

FUSED_SWEEP = [
    # ---- 32-channel intermediate, one buffer, straight-line items
    _p("uni-g4-gl4-big", *_BIG8, (32, 32), 32, 32, form(1, 1, 8, 1, "UNI", "GL4"), act=ACT_RELU, stats=True),
    _p("uni-g6-gl2-far", *_M8, (32, 24, 24), 32, 32, form(1, 1, 8, 2, "UNI", "GL2"), far=1, residual=True, act=ACT_LEAKY),   # 24: one full group + a tail
    _p("uni-g8-gl4", *_M8, (40, 40, 32), 32, 30, form(1, 1, 8, 2, "UNI", "GL4"), post=True),                   # 30 of 32 outputs
    # ---- 32-channel intermediate, one buffer, generic
    _p("uni-1-nb1-tiny", 1, 3, 5, (40,), 30, 30, form(1, 1, 8, 1, "UNI"), act=ACT_RELU),                       # a map smaller than a tile
    _p("uni-1-nb2-aligned", 2, 8, 32, (40, 24), 32, 32, form(1, 1, 8, 2, "UNI"), act=ACT_LEAKY, stats=True),   # W = 32, H = TH
    _p("uni-1-nb3", *_M8, (64, 40, 32, 24), 32, 32, form(1, 1, 8, 3, "UNI"), residual=True),                   # G = 11
    _p("uni-2-nb1", *_M8, (32, 24), 30, 38, form(1, 2, 8, 1, "UNI"), act=ACT_RELU, post=True),                 # 40 of 64 outputs stored
    _p("uni-2-nb2", *_M8, (32, 32, 32), 32, 64, form(1, 2, 8, 2, "UNI"), act=ACT_LEAKY, stats=True),
    _p("uni-2-nb3", *_M8, (64, 48, 32), 32, 64, form(1, 2, 8, 3, "UNI")),                                      # G = 9
    # ---- 32-channel intermediate, the last slice(s) in a second buffer
    _p("sep-1-nb1", *_M8, (32, 24), 32, 32, form(1, 1, 8, 1), split=1, act=ACT_LEAKY),
    _p("sep-1-nb2", *_M8, (32, 40, 32), 32, 32, form(1, 1, 8, 2), split=2, post=True, act=ACT_RELU),           # G = 7
    _p("sep-1-nb3", *_M8, (64, 32, 64), 30, 32, form(1, 1, 8, 3), split=2, stats=True),                        # G = 10
    _p("sep-2-nb1", *_M8, (24, 16), 32, 64, form(1, 2, 8, 1), split=1, residual=True),
    _p("sep-2-nb2", *_M8, (40, 24, 16), 32, 64, form(1, 2, 8, 2), split=1, act=ACT_LEAKY),                     # G = 6
    _p("sep-2-nb3", *_M8, (64, 64, 32, 30), 32, 64, form(1, 2, 8, 3), split=2, act=ACT_RELU),                  # G = 12
    # ---- 64-channel intermediate, one buffer, 64 outputs
    _p("uni64-g7-gl1-big", *_BIG4, (38, 64), 64, 64, form(2, 2, 4, 4, "UNI", "GL1"), act=ACT_LEAKY, stats=True),
    _p("uni64-g11-gl1-far", *_M4, (38, 64, 64), 64, 64, form(2, 2, 4, 6, "UNI", "GL1"), far=1, act=ACT_RELU),
    _p("uni64-nb2", *_M4, (32, 24), 62, 62, form(2, 2, 4, 2, "UNI"), post=True, act=ACT_LEAKY),                # 62-channel intermediate and output
    _p("uni64-nb4", 2, 4, 32, (40, 40), 64, 64, form(2, 2, 4, 4, "UNI"), residual=True, stats=True),           # W = 32, H = TH; G = 6
    _p("uni64-nb6", *_M4, (64, 40, 32), 64, 64, form(2, 2, 4, 6, "UNI"), act=ACT_RELU),                        # G = 9
    # ---- 64-channel intermediate, the non-UNI build
    _p("n64-1-nb2-one-buffer", *_M4, (32, 32), 64, 32, form(2, 1, 4, 2), act=ACT_LEAKY, stats=True),           # one buffer, 32 outputs
    _p("n64-1-nb4", *_M4, (40, 32), 62, 30, form(2, 1, 4, 4), split=1, residual=True),                         # G = 5
    _p("n64-1-nb6", *_M4, (64, 32, 48), 64, 32, form(2, 1, 4, 6), split=2, act=ACT_RELU, post=True),           # G = 9
    _p("n64-2-nb2", *_M4, (16, 24), 64, 64, form(2, 2, 4, 2), split=1, act=ACT_LEAKY),
    _p("n64-2-nb4", *_M4, (38, 64), 64, 64, form(2, 2, 4, 4), split=1, stats=True),                            # G = 7 in two buffers
    _p("n64-2-nb6", *_M4, (62, 32, 32, 38), 64, 62, form(2, 2, 4, 6), split=2, act=ACT_RELU),                  # G = 11 in two buffers
    # ---- the up-sampled addend folded through the 1x1 (32 -> 32)
    _p("up-g4-gl4", *_UP, (32, 32), 32, 32, form(1, 1, 8, 1, "UPADD", "UNI", "GL4"), up=True, act=ACT_LEAKY),
    _p("up-g6-gl2-aligned", 2, 16, 64, (32, 32, 32), 32, 32, form(1, 1, 8, 2, "UPADD", "UNI", "GL2"), up=True, residual=True),
    _p("up-uni-nb1", *_UP, (40,), 30, 30, form(1, 1, 8, 1, "UPADD", "UNI"), up=True, act=ACT_RELU, stats=True),
    _p("up-uni-nb2-big", *_BIG8, (40, 24), 32, 32, form(1, 1, 8, 2, "UPADD", "UNI"), up=True, act=ACT_LEAKY),  # G = 5, several tiles per workgroup
    _p("up-sep-nb1", *_UP, (16, 24), 32, 32, form(1, 1, 8, 1, "UPADD"), up=True, split=1, post=True),
    _p("up-sep-nb2-aligned", 2, 16, 64, (32, 24, 32), 32, 32, form(1, 1, 8, 2, "UPADD"), up=True, split=2, act=ACT_RELU),
    # ---- the convBlock head
    _c4("c4-planar-c1v", 4, 19, 45, 1, form(1, 1, 8, 1, "C4", "GL3", "C1V"), planar=True, post=True, stats=True),
    _c4("c4-planar-c1v-big", *_BIG8, 1, form(1, 1, 8, 1, "C4", "GL3", "C1V"), planar=True, stats=True),
    _c4("c4-nhwc-2", *_M8, 2, form(1, 1, 8, 1, "C4", "GL3"), residual=True),
    _c4("c4-nhwc-3", *_M8, 3, form(1, 1, 8, 1, "C4", "GL3"), C1=30, C2=30, post=True, stats=True),
    _c4("c4-nhwc-4", 1, 3, 5, 4, form(1, 1, 8, 1, "C4", "GL3"), act1=ACT_NONE),
    _c4("c4-planar-mfma", 4, 19, 45, 1, form(1, 1, 8, 1, "C4", "GL3"), planar=True, c1v=False, stats=True),    # engine.C1V off: the planar branch of the MFMA form
]
FUSED_IDS = [r["id"] for r in FUSED_SWEEP]
STRIDED = "uni-1-nb3"         # 12 tiles: fewer than 256 and no multiple of 8, dealt by stride


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------

def upsample2(P, clamp=True, shift=0):
    """Bilinear x2 up-sampling of [B][C][h][w], align_corners False, as ATen states it: source index max(0.5 (d + 0.5) - 0.5, 0), the second
    tap clamped to the last sample.  ``clamp`` False and ``shift`` are the mistakes of ``wrong``: the second tap read one past the border
    (zeros), the samples taken one low-resolution pixel to the left."""
    P = P.to(D)
    if shift:
        P = torch.cat([P[..., :1]] * shift + [P[..., :-shift]], 3)
    h, w = P.shape[2:]
    Pz = F.pad(P, (0, 1, 0, 1))

    def axis(n):
        s = (0.5 * (torch.arange(2 * n, dtype=D) + 0.5) - 0.5).clamp(min=0)
        i0 = s.floor().long()
        i1 = (i0 + 1).clamp(max=n - 1) if clamp else i0 + 1
        return i0, i1, s - i0
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    ly = ly[:, None]
    g = lambda yi, xi: Pz[:, :, yi][:, :, :, xi]      # noqa: E731
    return (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))


def first_stage(row, data, xs=None, addend=None, grow=0):
    """t in float64: the 1x1 over the concatenated slices + b1 (+ the up-sampled addend), or act1(3x3(x) + b1) for a convBlock row.
    ``grow``: evaluated on the map grown by that many pixels, from zero-padded INPUTS (what ``wrong`` 'bias_leak' reads)."""
    x = torch.cat([v.to(D) for v in (data["xs"] if xs is None else xs)], 1)
    if grow:
        x = F.pad(x, (grow,) * 4)
    if row["kind"] == "c4":
        return act_ref(F.conv2d(x, data["w1"].to(D), data["b1"].to(D), padding=1), data["act1"])
    t = F.conv2d(x, data["w1"].to(D), data["b1"].to(D))
    if data["P"] is not None:
        u = (upsample2(data["P"]) if addend is None else addend)[:, :t.shape[1]]
        t = t + (F.pad(u, (grow,) * 4) if grow else u)
    return t


def epilogue(data, z):
    y = act_ref(z, data["act"])
    if data["post"] is not None:
        y = y * data["post"][0].to(D)[None, :, None, None] + data["post"][1].to(D)[None, :, None, None]
    if data["residual"] is not None:
        y = y + data["residual"].to(D)
    return y


def reference(row, data):
    """What the launch computes, in float64: the 3x3's zero padding pads the first stage's OUTPUT."""
    return epilogue(data, F.conv2d(first_stage(row, data), data["w2"].to(D), data["b2"].to(D), padding=1))


def stats_of(y):
    """InstanceNorm (scale, shift) of an NCHW tensor in float64: eps 1e-5, biased variance."""
    y = y.to(D)
    rstd = 1.0 / torch.sqrt(y.var((2, 3), unbiased=False) + 1e-5)
    return rstd, -y.mean((2, 3)) * rstd


# ---- scales and the float64 emulation ----------------------------------------------------------------------------------------------

def t_bound(data):
    """The engine's bound on |t| (Plan._conv_pair_impl / _conv_pair_c4, rescale): max |x| * max_co sum |w1| + max |b1| (+ max |P|)."""
    vmax = max(float(x.abs().max()) for x in data["xs"])
    bound = vmax * float(data["w1"].abs().sum(dim=(1, 2, 3)).max()) + float(data["b1"].abs().max())
    return bound + (float(data["P"].abs().max()) if data["P"] is not None else 0.0)


def scales_for(data):
    """(a1, w_scale1 or w_scale_c4, a2, w_scale) the plan uses on ``data``."""
    return (a_scale_for(max(float(x.abs().max()) for x in data["xs"])), w_scale_for([data["w1"]]), a_scale_for(t_bound(data)), w_scale_for([data["w2"]]))


def _halves(v, s):
    t = v.float() * s
    assert torch.equal(t.double(), v.double() * s), "a scaled operand is not an fp32 value"
    return split_f16(t)


def emulate(row, data, scales, drop_t_lo=False):
    """The launch's arithmetic in float64: per stage hi*hi + hi*lo + lo*hi of the scaled operands, divided by the scales; the intermediate
    zeroed outside the image, scaled by a2 and split.  C1V rows take the first stage as fp32 multiply-adds of the unsplit operands."""
    a1, s1, a2, s2 = scales
    w1h, w1l = _halves(data["w1"], s1)
    k = dict(padding=1) if row["kind"] == "c4" else {}
    if row["kind"] == "c4" and row["planar"] and row["c1v"]:
        acc = F.conv2d(data["xs"][0].to(D), data["w1"].to(D), **k)
    else:
        xs = [_halves(x, a1) for x in data["xs"]]
        xh, xl = torch.cat([h for h, _ in xs], 1), torch.cat([l for _, l in xs], 1)
        acc = F.conv2d(torch.cat([xh, xl], 1), torch.cat([w1h + w1l, w1h], 1), **k) / (a1 * s1)
    t = acc + data["b1"].to(D)[None, :, None, None]
    if data["P"] is not None:
        t = t + upsample2(data["P"])[:, :t.shape[1]]
    t = act_ref(t, data["act1"])
    th, tl = _halves(t, a2)
    if drop_t_lo:
        tl = torch.zeros_like(tl)
    w2h, w2l = _halves(data["w2"], s2)
    z = F.conv2d(torch.cat([th, tl], 1), torch.cat([w2h + w2l, w2h], 1), padding=1) / (a2 * s2) + data["b2"].to(D)[None, :, None, None]
    return epilogue(data, z)


# ---- what a wrong kernel would store -----------------------------------------------------------------------------------------------

MISTAKES = ("bias_leak", "tail_upper", "far_near", "t_lo_dropped", "up_shifted", "up_unclamped", "stale_tile")
MISTAKE_RUNS = {m: ("int",) for m in MISTAKES}
MISTAKE_RUNS["t_lo_dropped"] = ("fine_x", "fine_w1")
# rows in which a mistake must change more than 1 % of the stored outputs
NAMED = dict(bias_leak=("uni-g8-gl4", "uni64-nb6", "c4-nhwc-2", "c4-planar-c1v"), tail_upper=("uni-g6-gl2-far", "sep-2-nb2", "n64-2-nb4"),
             far_near=("uni-g6-gl2-far", "uni64-g11-gl1-far"), t_lo_dropped=("uni-g4-gl4-big", "uni64-g7-gl1-big", "c4-planar-c1v", "up-g4-gl4"),
             up_shifted=("up-g4-gl4", "up-sep-nb2-aligned", "up-uni-nb2-big"), up_unclamped=("up-g4-gl4", "up-uni-nb1"),
             stale_tile=("uni-g4-gl4-big", "uni64-g7-gl1-big", "up-uni-nb2-big", "c4-planar-c1v-big"))


def applies(row, mistake):
    pair = row["kind"] == "pair"
    return {"bias_leak": True, "tail_upper": pair and any(pad8(c) % 16 == 8 for c in row["chans"]), "far_near": row["far"] is not None,
            "t_lo_dropped": True, "up_shifted": row["up"], "up_unclamped": row["up"], "stale_tile": tiles_of(row)[3] > MAX_GRID}[mistake]


def wrong(row, data, scales, mistake):
    """The float64 result of a launch that makes ``mistake``:
      bias_leak      the INPUT is zero padded instead of the first stage's output: b1 (act1(b1)) stands in the 3x3's border;
      tail_upper     the upper eight channels of a tail group (a slice of 16 k + 8 padded channels; 0x8000 in the group table) are read:
                     their weights are zero, but what follows the slice is IN_POISON, which a1 takes out of the f16 range -- inf * 0;
      far_near       the far slices are read from frame b, not b + dn: from the poisoned half of their buffer;
      t_lo_dropped   the lo halves of the intermediate are not used;
      up_shifted     the low-resolution patch is taken one pixel to the left;  up_unclamped: the second tap runs past the border;
      stale_tile     the second tile of a workgroup is computed from the LDS image of its first tile."""
    assert applies(row, mistake)
    w2, b2 = data["w2"].to(D), data["b2"].to(D)
    if mistake == "bias_leak":
        return epilogue(data, F.conv2d(first_stage(row, data, grow=1), w2, b2))
    if mistake == "tail_upper":
        want = reference(row, data)
        return torch.full_like(want, float("nan")) if IN_POISON * scales[0] > 65504.0 else want
    if mistake == "far_near":
        xs = [x if i < row["far"] else torch.full_like(x, IN_POISON) for i, x in enumerate(data["xs"])]
        return epilogue(data, F.conv2d(first_stage(row, data, xs=xs), w2, b2, padding=1))
    if mistake == "t_lo_dropped":
        return emulate(row, data, scales, drop_t_lo=True)
    if mistake in ("up_shifted", "up_unclamped"):
        u = upsample2(data["P"], shift=1) if mistake == "up_shifted" else upsample2(data["P"], clamp=False)
        return epilogue(data, F.conv2d(first_stage(row, data, addend=u), w2, b2, padding=1))
    th, tx, ty, _ = tiles_of(row)
    t = first_stage(row, data)
    z = F.conv2d(t, w2, b2, padding=1)
    tp = F.pad(t, (1, tx * TW - row["W"] + 1, 1, ty * th - row["H"] + 1))
    for walk in tile_walk(row):
        if len(walk) > 1:
            (f0, y0, x0), (f1, y1, x1) = walk[0], walk[1]
            zt = F.conv2d(tp[f0:f0 + 1, :, y0:y0 + th + 2, x0:x0 + TW + 2], w2, b2)
            hh, ww = min(th, row["H"] - y1), min(TW, row["W"] - x1)
            z[f1, :, y1:y1 + hh, x1:x1 + ww] = zt[0, :, :hh, :ww]
    return epilogue(data, z)


# ---- conditions --------------------------------------------------------------------------------------------------------------------

def _is_pow2(v):
    return math.frexp(abs(v))[0] == 0.5


def conditions(row, run, data, want, scales):
    """What makes the run exact on the GPU -- conditions on the data, none a tolerance -- and what makes it a test.  Returns the largest
    partial sum of each stage in units of its smallest product."""
    a1, s1, a2, s2 = scales
    assert all(_is_pow2(s) for s in scales), "scales are powers of two"
    assert data["act"] in (ACT_NONE, ACT_RELU) and data["act1"] in (ACT_NONE, ACT_RELU), "0.01 is not a binary fraction"
    assert (data["b1"] != 0).all(), "b1 must show in the border if it leaks"
    assert IN_POISON * a1 > 65504.0
    c1v = row["kind"] == "c4" and row["planar"] and row["c1v"]
    # ---- stage 1
    xs = [_halves(x, a1) for x in data["xs"]]
    xh, xl = [h for h, _ in xs], [l for _, l in xs]
    w1h, w1l = _halves(data["w1"], s1)
    for x, h, l in zip(data["xs"], xh, xl):
        assert torch.equal(h + l, x.double() * a1) and h.abs().max().item() <= 4096, "an input does not split into two f16 halves"
    assert torch.equal(w1h + w1l, data["w1"].double() * s1) and w1h.abs().max().item() <= 4096
    x_plain, w1_plain = all((l == 0).all() for l in xl), bool((w1l == 0).all())
    assert c1v or x_plain or w1_plain, "both operands of stage 1 carry lo halves"
    epi1 = [data["b1"]] + ([data["P"] / 16] if data["P"] is not None else [])
    if data["P"] is not None:
        assert torch.equal((data["P"] / 16).round() * 16, data["P"]), "P must hold multiples of 16: the interpolation weights are multiples of 1 / 16"
    unit1 = min(granule(data["xs"]) * granule([data["w1"]]) if c1v else granule(xh + xl) * granule([w1h, w1l]) / (a1 * s1), granule(epi1))
    tmax = t_bound(data)
    units1 = tmax / unit1
    assert units1 <= FP32_EXACT, "%s %s: a partial sum of stage 1 may reach %.3g units of %g" % (row["id"], run, units1, unit1)
    # ---- the intermediate
    t = first_stage(row, data)
    assert t.abs().max().item() <= tmax
    th, tl = _halves(t, a2)
    assert torch.equal(th + tl, t * a2) and torch.isfinite(th).all() and th.abs().max().item() < 2048, "t * a2 does not split into two f16 halves"
    assert ((tl == 0) | (tl.abs() >= 2.0 ** -14)).all(), "a lo half of t * a2 is subnormal"
    t_dens = (tl != 0).double().mean().item()
    if run in ("int", "fine_w2"):
        assert t_dens == 0.0, "t must have at most 11 bits"
    else:
        assert t_dens >= LO_DENSITY, "%s %s: only %.1f %% of t has a lo half" % (row["id"], run, 100 * t_dens)
    # ---- stage 2
    w2h, w2l = _halves(data["w2"], s2)
    assert torch.equal(w2h + w2l, data["w2"].double() * s2) and w2h.abs().max().item() <= 4096
    assert t_dens == 0.0 or (w2l == 0).all(), "both operands of stage 2 carry lo halves"
    ps = pt = 1.0
    epi2 = [data["b2"]]
    if data["post"] is not None:
        assert all(_is_pow2(v) and abs(v) >= 1 for v in data["post"][0].tolist()), "post scales are powers of two"
        ps, pt = data["post"][0].abs().max().item(), data["post"][1].abs().max().item()
        epi2.append(data["post"][1])
    else:
        pt = 0.0
    rmax = 0.0
    if data["residual"] is not None:
        epi2.append(data["residual"])
        rmax = data["residual"].abs().max().item()
    unit2 = min(granule([th, tl]) * granule([w2h, w2l]) / (a2 * s2), granule(epi2))
    ymax = (tmax * float(data["w2"].abs().sum(dim=(1, 2, 3)).max()) + data["b2"].abs().max().item()) * ps + pt + rmax
    units2 = ymax / unit2
    assert units2 <= FP32_EXACT, "%s %s: a partial sum of stage 2 may reach %.3g units of %g" % (row["id"], run, units2, unit2)
    # ---- the reference, and the run as a test
    assert torch.equal(want.float().double(), want), "the reference is not an fp32 value"
    nz = (want != 0).double().mean().item()
    assert nz >= 0.3, "only %.0f %% of the outputs are non-zero" % (100 * nz)
    share = lambda ls, ws: sum(int((l != 0).sum()) for l in ls) / max(1, sum(int((w != 0).sum()) for w in ws))      # noqa: E731
    if run == "fine_x":
        assert w1_plain and (w2l == 0).all() and share(xl, [torch.ones_like(l) for l in xl]) >= LO_DENSITY
    elif run == "fine_w1":
        assert x_plain and (w2l == 0).all() and share([w1l], [data["w1"]]) >= LO_DENSITY
    elif run == "fine_w2":
        assert x_plain and w1_plain and share([w2l], [data["w2"]]) >= LO_DENSITY
    else:
        assert x_plain and w1_plain and (w2l == 0).all()
    return units1, units2


# ---- data --------------------------------------------------------------------------------------------------------------------------

def _fine(gen, w):
    """The pattern of integer weights ``w`` with magnitudes r / 2, r in [1, 4095] -- three of five of them above 2048, where every odd r
    has a lo half: a thinned pack has few weights to make the share from -- one of them 2047.5 (the pack's scale is 1)."""
    r = torch.where(torch.rand(w.shape, generator=gen) < 0.6, 2048 + _ints(gen, w.shape, 1, 2047), _ints(gen, w.shape, 1, 4095))
    w = torch.sign(w) * r / 2
    w.view(-1)[int(w.view(-1).nonzero()[0])] = 2047.5
    return w


def exact_data(gen, row, run):
    """Data of generator ``run`` for the row.  The weights are thinned (conv_refs._weights: every (input channel, tap) keeps a weight)
    until the worst-case partial sums of both stages fit: |t| <= max |x| S1 + 3 (+ max |P|) and |y| <= (|t| S2 + 3) * 4 + 6 + 8 with
    S = max_co sum |w|, against 2^24 units (2^22 for t, which must split into two halves; 2047 where t must not have a lo half).
    These are the loop's estimates; fused_refs.conditions is what asserts the run exact."""
    B, H, W, C1, C2 = row["B"], row["H"], row["W"], row["C1"], row["C2"]
    c4 = row["kind"] == "c4"
    k1 = 3 if c4 else 1
    Cin = sum(row["chans"])
    xr = 2 if run == "fine_w2" else 4
    xs = []
    for c in row["chans"]:
        s = (B, c, H, W)
        if run == "fine_x":       # q / 2, |q| <= 4095, four of five above 2048 (13 bits; every odd q there has a lo half), either sign
            q = torch.where(torch.rand(s, generator=gen) < 0.8, 2048 + _ints(gen, s, 0, 2047), _ints(gen, s, 0, 4095))
            xs.append(q * (torch.randint(0, 2, s, generator=gen).float() * 2 - 1) / 2)
        else:
            xs.append(_ints(gen, s, -xr, xr))
    xs[0][0, 0, 0, 0] = 2047.5 if run == "fine_x" else xr        # max |x| is known: a1 = 1, 512 or 1024
    sign = lambda shape: torch.randint(0, 2, shape, generator=gen).float() * 2 - 1      # noqa: E731
    P = None
    if row["up"]:
        pr = 2 if run == "fine_w2" else 8
        P = 16 * _ints(gen, (B, 32, H // 2, W // 2), -pr, pr)
    d1 = d2 = 1.0
    while True:
        w1, w2 = _weights(gen, (C1, Cin, k1, k1), d1), _weights(gen, (C2, C1, 3, 3), d2)
        if run == "fine_w1":
            w1 = _fine(gen, w1)
        elif run == "fine_w2":
            w1, w2 = torch.sign(w1), _fine(gen, w2)
        b1, b2 = _ints(gen, (C1,), 1, 3) * sign((C1,)), _ints(gen, (C2,), 1, 3)
        data = dict(xs=xs, w1=w1, b1=b1, P=P, w2=w2, b2=b2, act=ACT_RELU if row["act"] else ACT_NONE, act1=ACT_RELU if row["act1"] else ACT_NONE,
                    post=(_pow2(gen, (C2,)), _ints(gen, (C2,), -6, 6)) if row["post"] else None,
                    residual=_ints(gen, (B, C2, H, W), -8, 8) if row["residual"] else None)
        unit = (0.5 if run in ("fine_x", "fine_w1") else 1.0)
        tmax = t_bound(data)
        ymax = (tmax * float(w2.abs().sum(dim=(1, 2, 3)).max()) + 3) * (4 if row["post"] else 1) + 14
        t_ok = tmax <= 2047 if run in ("int", "fine_w2") else tmax / unit < 2 ** 22
        y_ok = ymax / (unit * (0.5 if run == "fine_w2" else 1.0)) <= FP32_EXACT
        if t_ok and y_ok:
            break
        # thin the operand whose lo halves the run is not about first: a dense w1 keeps many terms, and so many bits, in t
        if not t_ok or (run == "fine_w2" and d1 > 0.02) or d2 <= 0.02:
            d1 *= 0.5
        else:
            d2 *= 0.5
        assert min(d1, d2) > 1e-4, (row["id"], run)
    data["density"] = (d1, d2)
    return data


def normal_data(gen, row):
    """Seeded normal data in the ranges of test_conv1x1_3x3_fused / test_convblock_pair_fused, LeakyReLU where the row has an activation."""
    B, H, W, C1, C2 = row["B"], row["H"], row["W"], row["C1"], row["C2"]
    k1 = 3 if row["kind"] == "c4" else 1
    Cin = sum(row["chans"])
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    return dict(xs=[rn(B, c, H, W) * 2 for c in row["chans"]], w1=rn(C1, Cin, k1, k1) / (k1 * Cin ** 0.5), b1=rn(C1),
                P=rn(B, 32, H // 2, W // 2) if row["up"] else None, w2=rn(C2, C1, 3, 3) / (3 * C1 ** 0.5), b2=rn(C2),
                act=ACT_LEAKY if row["act"] else ACT_NONE, act1=ACT_LEAKY if row["act1"] else ACT_NONE,
                post=(rn(C2).abs() + 0.5, rn(C2)) if row["post"] else None, residual=rn(B, C2, H, W) if row["residual"] else None, density=(1.0, 1.0))


SEED = 1234
_CACHE = {}


def exact_case(row, run):
    """(data, want, scales) of generator ``run`` for the row, seeded per (row, run), computed once per process and shared (do not modify)."""
    key = (row["id"], run)
    if key not in _CACHE:
        data = exact_data(torch.Generator().manual_seed(SEED + 100 * FUSED_IDS.index(row["id"]) + RUNS.index(run)), row, run)
        _CACHE[key] = (data, reference(row, data), scales_for(data))
    return _CACHE[key]
