"""Sweep table, exactly representable data, float64 references and launcher rules for the kernels that carry training plans with bf16
activation storage (BASELINE.json configs[2..4]): csrc/conv3x3_bf16.hip (forward and data gradient), csrc/conv1x1_bf16.hip (streaming
and multi-destination forms), csrc/conv_narrow_bf16.hip, csrc/wgrad_bf16.hip and the bf16 branches of wgrad_impl in csrc/backward.hip.

Modelled on conv_refs.py / split_refs.py and built on them: ``conv_refs.int_case`` draws the forward data, ``conv_refs.conv_ref`` is the
forward reference.  New here:

* ``BF16_SWEEP``: every row names its ``part`` (fwd3, fwd1, narrow, dgrad3, dgrad1, multi, wgrad3, wgrad1, wgrad_generic) and, in
  ``inst``, the template instantiation it is meant to reach.  ``b3_form`` / ``s1_form`` / ``narrow_form`` / ``wgrad_form`` restate the
  launch rules at the end of the four kernel files and of wgrad_impl in Python, as ``conv_refs.launch_form`` does for the implicit GEMM;
  tests/test_host_bf16_refs.py holds every row's claim against them (and, where the library answers on the host, against the
  library), and walks ``REQUIRED`` so that no instantiation can drop out of the table silently.
* training rows are small graphs of layers (``layers_of``): one layer, two 3x3 in a row with a third reader of the input (first, second
  and last writer of a gradient slice), a 1x1 over several slices.  ``train_ref`` is a float64 statement of Plan._bw_conv: per layer,
  in reverse order, gz = g * [y_stored > 0], bias / weight / data gradients of the plain convolution through autograd, the data gradients
  accumulated in the order the plan writes them -- every intermediate value a kernel stores is returned and checked.
* ``train_case`` draws integer data for which y, every gz, every stored state of every gradient slice stay within the +-256 integers
  bf16 holds and every partial sum -- the weight gradient's sum over all pixels included -- below 2^24, by halving the weight density
  and then narrowing the output gradient.  ``narrow_case`` draws ternary inputs (a 7x7 over 64 channels keeps a weight per (channel,
  tap): with inputs in [-4, 4] it cannot come under 256).  ``multi_case`` / ``up_case`` serve the two forms the planner does not reach
  by a plain layer: the multi-destination 1x1 at a chosen k-step count (through the C entry) and the up-sampled addend.

What the rows claim, per kernel file (``REQUIRED``), and what they leave out:
  conv3x3_bf16.hip      every <KCH, MB, RM> the launcher chooses with its default switches: <1|2|3|4|streamed, 1, 0|1|2> and
                        <1|2|streamed, 2, 0|1> (forward rows: RM 0 and the residual forms <2, 1, 1>, <2, 2, 1>; the other RM 1 / 2 forms as second
                        and last writers of a gradient slice, rows d3-chain-*).  Left out: RW = 1 (EGNE_B3_RW) and the forms EGNE_B3_MB selects.
  conv1x1_bf16.hip      streaming <2, 4> <4, 4> <4, 8> without and with the up-sampled addend; multi-destination <1> <2> <3> <4> <6> <8>
                        (<3> through the plan only, row w1-4-64-store88).  Left out: nothing the launcher can choose (NB16 = 2 runs four waves).
  conv_narrow_bf16.hip  all six <K, NCH>.
  wgrad_bf16.hip        pair and quad form, 1x1 <1,256> <1,128> <2,128> <2,64> <4,64> <8,64>, a two-launch layer.  Left out: nothing.
  backward.hip          bf16 branches of wgrad_impl: conv_wgrad_kernel<bf16, BFM>, <.., FOLD>, conv_wgrad_wide_kernel<true> / <false>,
                        conv1x1_wgrad_allpairs_kernel<3, 64, bf16>.  Left out: the other seven all-pairs instantiations on bf16 tensors (the code
                        of the fp32 ones that tests/test_gpu_conv_backward_fp32.py runs; no bf16 test reaches them), conv_wgrad_kernel<bf16, false>
                        (EGNE_IGEMM_BF16_MFMA=0).
Row sizes: a 3x3 row is 11x37 or close to it unless its comment says otherwise -- two tiles of 8 x 32 per axis, both ragged, the smallest
map on which a tile edge, a second tile and a halo across a tile border all occur; a 1x1 row is 2 x 47 x 45 = 4230 pixels, the smallest
odd-sized map over the 4096 pixels from which the planner takes the streaming kernels; multi-destination rows through the C entry need
no 4096 pixels and run 600 .. 1536 pixels, never a multiple of the 128 pixels of a workgroup's four waves except multi-1-step (full groups).
"""
import functools

import torch
import torch.nn.functional as F

import conv_refs as R
from conv_refs import ACT_NONE, ACT_RELU, BF, BF16_EXACT, D, FP32_EXACT, pad8, pad32

TW, TH = 32, 8                 # output tile of conv3x3_bf16.hip, conv_narrow_bf16.hip and the 3x3 forms of wgrad_bf16.hip
S1_MIN_PIX = 4096              # pixels from which the planner takes the streaming 1x1 kernels (engine.choose_conv, wgrad1x1_bf16_supported)
ACT_LEAKY = R.ACT_LEAKY


# ---- the table -------------------------------------------------------------------------------------------------------------------

def _L(name, src, Cout, k=3, pad=None, act=ACT_RELU, norm=(), nograd=(), stride=1, pad_mode=0, bias=True):
    """One layer of a training row: ``src`` names its input slices (x0, x1, ... of the row's input buffer, or another layer's name)."""
    return dict(name=name, src=tuple(src), Cout=Cout, k=(k, k), pad=(k // 2, k // 2) if pad is None else tuple(pad), act=act, norm=tuple(norm),
                nograd=tuple(nograd), stride=stride, pad_mode=pad_mode, bias=bias)


def _r(id, part, B, H, W, chans, Cout, k=3, pad=None, act=ACT_NONE, norm=(), residual=False, inst=None, fwd=None, **kw):
    """One row.  ``inst``: the instantiation the row is about; ``fwd``: the kind(s) of its forward launch(es) in Plan.meta.  Keys beyond
    those of conv_refs._c: stats (statistics partials from the epilogue), cout_pad (ConvLayer.cout_pad: Cout_store), up (half-resolution
    addend: the map is 2 * up), layers (training graph; None: one layer ``c`` over all slices), nograd (slices without a data gradient),
    bw (expected kinds of the backward plan's convolution launches, by name suffix), multi (the C-entry description), seed."""
    kk = (k, k) if isinstance(k, int) else tuple(k)
    pad = (kk[0] // 2, kk[1] // 2) if pad is None else tuple(pad)
    row = R._c(id, B, H, W, chans, Cout, kk, "bf16", stride=kw.pop("stride", 1), pad=pad, act=act, pad_mode=kw.pop("pad_mode", 0), norm=norm,
               residual=residual, form=part, tile=(0, 0))
    row.update(part=part, inst=inst, fwd=fwd, stats=False, cout_pad=None, up=None, layers=None, nograd=(), bw=None, multi=None, seed=1234)
    row.update(kw)
    return row


B3, S1, NA, IG = "conv_bf16:3x3", "conv_bf16:1x1", "conv_bf16:narrow", "conv_igemm"

FWD3 = [
    # <KCH, MB, RM>.  MB = 1: CoutP 32.  Every row but the last two has ragged tiles in x AND y and two tiles per axis (H = 8 + r, W = 32 + s):
    # the smallest maps with that property; ntiles = 2 * 2 * B stays far below the 256 workers (nworkers = 8 * (32 / nrun)): most workers idle.
    _r("b3-k1-mb1", "fwd3", 2, 11, 37, (32,), 32, act=1, inst=("b3", 1, 1, 0), fwd=B3),
    _r("b3-k2-mb1-res", "fwd3", 1, 13, 35, (64,), 32, residual=True, inst=("b3", 2, 1, 1), fwd=B3),
    _r("b3-k2-mb1", "fwd3", 1, 9, 33, (64,), 20, act=1, inst=("b3", 2, 1, 0), fwd=B3),
    _r("b3-k3-mb1", "fwd3", 1, 9, 33, (96,), 24, act=1, inst=("b3", 3, 1, 0), fwd=B3),
    _r("b3-k4-mb1", "fwd3", 1, 10, 41, (128,), 32, inst=("b3", 4, 1, 0), fwd=B3),
    _r("b3-streamed-mb1", "fwd3", 1, 9, 34, (160,), 20, act=1, inst=("b3", 0, 1, 0), fwd=B3),             # Ktot 160 > 128: weights streamed chunk by chunk
    _r("b3-k1-mb2-stats", "fwd3", 2, 11, 37, (32,), 64, act=1, inst=("b3", 1, 2, 0), fwd=B3, stats=True),  # ragged, statistics partials
    _r("b3-k2-mb2-res", "fwd3", 1, 13, 35, (64,), 64, act=1, residual=True, inst=("b3", 2, 2, 1), fwd=B3),
    _r("b3-streamed-mb2-180", "fwd3", 1, 9, 33, (180,), 180, act=1, inst=("b3", 0, 2, 0), fwd=B3),        # Ktot 192, six output blocks: nrun 3
    _r("b3-104-of-128", "fwd3", 1, 12, 36, (64,), 100, act=1, residual=True, inst=("b3", 2, 2, 1), fwd=B3),   # blocks 64 + 64, the second stores 40 of 64
    _r("b3-64-64-32", "fwd3", 1, 12, 40, (96,), 160, act=1, inst=("b3", 0, 2, 0), fwd=B3),               # Ktot 96 with MB = 2: streamed; the last workgroup has ONE block
    _r("b3-cin38-affine", "fwd3", 2, 11, 37, (38,), 38, act=1, norm=(0,), inst=("b3", 2, 2, 0), fwd=B3),  # Cp 40: half-empty second chunk; zero padding after the affine
    _r("b3-cout3", "fwd3", 3, 9, 33, (32,), 3, inst=("b3", 1, 1, 0), fwd=B3),                             # 3 outputs stored as 8
    _r("b3-deep-k-tiny-map", "fwd3", 1, 9, 11, (256,), 64, act=1, inst=("b3", 0, 2, 0), fwd=B3),          # eight chunks, two tiles (9 rows)
    # a worker walks two tiles: Cout 250 -> Cout_store 256, MB 2, nrun = 256 / 64 = 4, workers per XCD 32 / 4 = 8, nworkers 64;
    # 41x97 has 6 x 4 tiles, B = 3: 72 tiles, workers 0..7 take tiles w and w + 64
    _r("b3-two-tiles-per-worker", "fwd3", 3, 41, 97, (32,), 250, act=1, inst=("b3", 1, 2, 0), fwd=B3),
    _r("b3-k1-mb1-stats-full-tiles", "fwd3", 2, 16, 64, (32,), 32, act=1, inst=("b3", 1, 1, 0), fwd=B3, stats=True),
]

FWD1 = [
    # <NB16, NW, UP>.  2 x 47 x 45 = 4230 pixels: the smallest B * H * W >= 4096 with an odd map that is no multiple of 32 (132 groups + 6 pixels)
    _r("s1-nb2", "fwd1", 2, 47, 45, (32, 32), 32, k=1, inst=("s1", 2, 4, False), fwd=S1),
    _r("s1-nb2-cout96-res", "fwd1", 2, 47, 45, (64,), 96, k=1, residual=True, inst=("s1", 2, 4, False), fwd=S1),     # 6 blocks of 16: pieces of 2, three workgroup columns; accumulated residual
    _r("s1-nb4-cp40", "fwd1", 2, 47, 45, (38, 64, 64), 64, k=1, act=1, inst=("s1", 4, 4, False), fwd=S1),           # Cp 40: a k-step with 8 of 32 channels
    _r("s1-nw8-16-steps", "fwd1", 2, 47, 45, (172, 180, 100), 100, k=1, inst=("s1", 4, 8, False), fwd=S1),          # Cp 176 / 184 / 104: 6 + 6 + 4 steps, ragged ends; CoutP 128: two columns
    _r("s1-cout180", "fwd1", 2, 47, 45, (70, 50), 180, k=1, inst=("s1", 4, 4, False), fwd=S1),                      # CoutP 192: three columns of 64
    # up-sampled addend: the map is 2 * up; 4 x 30 x 40 = 4800, 5 x 26 x 34 = 4420 pixels
    _r("s1-up-nb2", "fwd1", 4, 30, 40, (40,), 32, k=1, inst=("s1", 2, 4, True), fwd=S1, up=(15, 20)),
    _r("s1-up-nb4-odd-half", "fwd1", 5, 26, 34, (168,), 62, k=1, inst=("s1", 4, 4, True), fwd=S1, up=(13, 17)),
    _r("s1-up-nw8", "fwd1", 4, 30, 40, (380,), 64, k=1, inst=("s1", 4, 8, True), fwd=S1, up=(15, 20)),             # 12 k-steps
]

NARROW = [
    # <K, NCH>: ternary inputs.  11x37 / 9x35: two ragged tiles per axis.  "Same" 3x3 go to conv3x3_bf16: the 3x3 rows pad (0, 1) / (0, 0)
    _r("narrow-7x7-64-cout3", "narrow", 1, 11, 37, (64,), 3, k=7, inst=("narrow", 7, 2), fwd=NA, cout_pad=4),       # the StyleEncoder gradient's shape: Cout_store 4
    _r("narrow-7x7-32-cout5", "narrow", 1, 11, 37, (32,), 5, k=7, act=1, inst=("narrow", 7, 1), fwd=NA),
    _r("narrow-5x5-64-cout8", "narrow", 1, 9, 35, (64,), 8, k=5, act=1, inst=("narrow", 5, 2), fwd=NA),
    _r("narrow-5x5-32-cout7", "narrow", 2, 9, 35, (32,), 7, k=5, inst=("narrow", 5, 1), fwd=NA),
    _r("narrow-3x3-64-valid", "narrow", 1, 11, 37, (64,), 8, k=3, pad=(0, 0), inst=("narrow", 3, 2), fwd=NA),      # outputs 9 x 35
    _r("narrow-3x3-32-pad01", "narrow", 2, 11, 35, (32,), 6, k=3, pad=(0, 1), act=1, inst=("narrow", 3, 1), fwd=NA),   # outputs 9 x 35
    # more tiles than the 256 workgroups: 65x317 has 9 x 10 tiles, B = 3: 270 tiles, workgroups 0..13 take a second one
    _r("narrow-5x5-32-second-tile", "narrow", 3, 65, 317, (32,), 8, k=5, act=1, inst=("narrow", 5, 1), fwd=NA),
]

# weight-gradient instantiations: ("pair" | "quad", splits), ("w1", ((PPW, CH) per launch), splits), (generic kernel, splits)
TRAIN3 = [
    # pair form: CoutP 32, or one input block, or an affine on load.  tiles = 2 * 2 * B
    _r("w3-pair-32-32", "wgrad3", 2, 11, 37, (32,), 32, act=1, inst=("pair", 8), fwd=B3, bw={"c.dgrad0": B3}),          # 8 tiles under the cap of 256: one tile per workgroup
    _r("w3-pair-cout64-k32", "wgrad3", 1, 11, 37, (32,), 64, act=1, inst=("pair", 4), fwd=B3, bw={"c.dgrad0": B3}),
    _r("w3-pair-three-input-blocks", "wgrad3", 1, 9, 33, (96,), 32, act=1, inst=("pair", 4), fwd=B3, bw={"c.dgrad0": B3}),
    _r("w3-pair-affine-cp40", "wgrad3", 2, 11, 37, (38,), 64, act=1, norm=(0,), nograd=(0,), inst=("pair", 8), fwd=B3, bw={}),     # Ktot 40 > 32 and CoutP 64, but an affine: the quad form refuses
    _r("w3-pair-w16", "wgrad3", 1, 9, 16, (32,), 32, act=1, inst=("pair", 2), fwd=B3, bw={"c.dgrad0": B3}),
    _r("w3-pair-w17", "wgrad3", 1, 9, 17, (32,), 32, inst=("pair", 2), fwd=B3, bw={"c.dgrad0": B3}),
    # a workgroup walks two tiles: 128 -> 32 has 1 x 4 pairs, cap 256 / 4 = 64 splits; 3 x (6 x 4) = 72 tiles.  Its data gradient is 32 -> 128
    _r("w3-pair-two-tiles", "wgrad3", 3, 41, 97, (128,), 32, act=1, inst=("pair", 64), fwd=B3, bw={"c.dgrad0": B3}),
    # quad form: CoutP >= 64, Ktot > 32, raw input
    _r("w3-quad-64-64", "wgrad3", 1, 9, 33, (64,), 64, act=1, inst=("quad", 4), fwd=B3, bw={"c.dgrad0": B3}),           # one full quad; 4 tiles under the cap of 256
    _r("w3-quad-96-96", "wgrad3", 1, 9, 33, (96,), 96, act=1, inst=("quad", 4), fwd=B3, bw={"c.dgrad0": B3}),           # 2 x 2 quads of 3 x 3 blocks: three of them miss pairs
    _r("w3-quad-128-100", "wgrad3", 1, 9, 33, (128,), 100, act=1, inst=("quad", 4), fwd=B3, bw={"c.dgrad0": B3}),       # Cout_store 104 of CoutP 128
    _r("w3-quad-38-64", "wgrad3", 1, 11, 37, (38,), 64, act=1, inst=("quad", 4), fwd=B3, bw={"c.dgrad0": B3}),          # Ktot 40: the second input block is 8 channels wide; dgrad 64 -> 38
    # a workgroup walks two tiles: 96 -> 96 has 4 quads, cap 64 splits; 72 tiles
    _r("w3-quad-two-tiles", "wgrad3", 3, 41, 97, (96,), 96, act=1, inst=("quad", 64), fwd=B3, bw={"c.dgrad0": B3}),
]

DGRAD3 = [
    # <KCH, MB, RM> of the data-gradient launches.  x -> a -> mid -> b -> out and x -> c -> out2: the backward plan runs c, b, a; c.dgrad0
    # is the FIRST writer of g(x) (RM 0, stores), b.dgrad0 the LAST writer of g(mid): it applies a's mask and leaves a's bias sums
    # (RM 2, mask_sums), a.dgrad0 the SECOND writer of g(x) (RM 1, accumulates).  Cmid 32 / 64 / 40 (padded)
    _r("d3-chain-cmid32", "dgrad3", 2, 11, 37, (32,), 32, act=1, inst=(("b3", 1, 1, 0), ("b3", 1, 1, 2), ("b3", 1, 1, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 32), _L("b", ("a",), 32), _L("c", ("x0",), 32)),
       bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-cmid64", "dgrad3", 1, 11, 37, (64,), 64, act=1, inst=(("b3", 1, 2, 0), ("b3", 1, 1, 2), ("b3", 2, 2, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 64), _L("b", ("a",), 32), _L("c", ("x0",), 32)),
       bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-cmid40", "dgrad3", 1, 11, 37, (32,), 40, act=1, inst=(("b3", 1, 1, 0), ("b3", 1, 1, 2), ("b3", 2, 1, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 40), _L("b", ("a",), 32), _L("c", ("x0",), 32)),
       bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    # the same chain over the other resident / streamed weight forms of a second and of a last writer.  KCH of b.dgrad0 follows b's Cout (the
    # channels of ITS gz), KCH of a.dgrad0 follows Cmid; a mask-on-write launch keeps ONE output block per workgroup (MB 1) whatever CoutP is;
    # a second writer has MB 2 where the slice it writes has 64 channels.  11x37, B = 1: four ragged tiles, the smallest map with two per axis
    _r("d3-chain-b64-cmid96", "dgrad3", 1, 11, 37, (32,), 96, act=1, inst=(("b3", 1, 1, 0), ("b3", 2, 1, 2), ("b3", 3, 1, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 96), _L("b", ("a",), 64), _L("c", ("x0",), 32)), bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-b96-cmid128", "dgrad3", 1, 11, 37, (32,), 128, act=1, inst=(("b3", 1, 1, 0), ("b3", 3, 1, 2), ("b3", 4, 1, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 128), _L("b", ("a",), 96), _L("c", ("x0",), 32)), bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-b128-cmid160", "dgrad3", 1, 11, 37, (32,), 160, act=1, inst=(("b3", 1, 1, 0), ("b3", 4, 1, 2), ("b3", 0, 1, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 160), _L("b", ("a",), 128), _L("c", ("x0",), 32)), bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-b160-cmid32", "dgrad3", 1, 11, 37, (32,), 32, act=1, inst=(("b3", 1, 1, 0), ("b3", 0, 1, 2), ("b3", 1, 1, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 32), _L("b", ("a",), 160), _L("c", ("x0",), 32)), bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-x64-cmid96", "dgrad3", 1, 11, 37, (64,), 96, act=1, inst=(("b3", 1, 2, 0), ("b3", 1, 1, 2), ("b3", 0, 2, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 96), _L("b", ("a",), 32), _L("c", ("x0",), 32)), bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    _r("d3-chain-x64-cmid32", "dgrad3", 1, 11, 37, (64,), 32, act=1, inst=(("b3", 1, 2, 0), ("b3", 1, 1, 2), ("b3", 1, 2, 1)), fwd=B3,
       layers=(_L("a", ("x0",), 32), _L("b", ("a",), 32), _L("c", ("x0",), 32)), bw={"c.dgrad0": B3, "b.dgrad0": B3, "a.dgrad0": B3}),
    # a 3x3 over TWO slices: the forward is the implicit GEMM, its data gradients are bf16 3x3 launches packed with c0 = 0 and c0 = 64
    _r("d3-two-slices", "dgrad3", 1, 11, 37, (64, 32), 32, act=1, inst=(("b3", 1, 2, 0), ("b3", 1, 1, 0)), fwd=IG, bw={"c.dgrad0": B3, "c.dgrad1": B3}),
    # Cin != Cout with padding on both sides: forward 38 -> 100, data gradient 100 (Cp 104, Ktot 128) -> 38 (40 stored of CoutP 64)
    _r("d3-38-100", "dgrad3", 1, 11, 37, (38,), 100, act=1, inst=(("b3", 0, 2, 0),), fwd=B3, bw={"c.dgrad0": B3}),
]

DGRAD1 = [
    # the streaming 1x1 as a data gradient: two 1x1 layers over the same adjacent raw slices (32 + 32 channels of one buffer: ONE merged launch
    # per layer, 64 outputs).  c.dgrad0-1 is the first writer (stores; gz of 64 channels: two k-steps), a.dgrad0-1 accumulates onto the
    # slice through the kernel's residual (gz of 32 channels: one k-step)
    _r("d1-merged-accumulate", "dgrad1", 2, 47, 45, (32, 32), 32, k=1, act=1, inst=(("s1", 4, 8, False), ("s1", 4, 4, False)), fwd=S1,
       layers=(_L("a", ("x0", "x1"), 32, k=1), _L("c", ("x0", "x1"), 64, k=1)), bw={"c.dgrad0-1": S1, "a.dgrad0-1": S1}),
]

TRAIN1 = [
    # 1x1 layers on 4230 pixels.  ("w1", ((PPW, CH), ...), splits): splits = ceil(M / (4 CH))
    _r("w1-1-256", "wgrad1", 2, 47, 45, (32, 32), 32, k=1, act=1, inst=("w1", ((1, 256),), 5), fwd=S1, bw={"c.dgrad0-1": S1}),        # 1 + 2 tiles; M = 4230 is no multiple of 5 x 256; merged data gradient
    _r("w1-1-128-cp40", "wgrad1", 2, 47, 45, (38, 64, 64), 32, k=1, act=1, inst=("w1", ((1, 128),), 9), fwd=S1, bw={"c.dgrad_multi": S1}),   # 1 + 6 tiles, 6 pairs; Cp 40; multi-destination data gradient through the plan
    _r("w1-2-128", "wgrad1", 2, 47, 45, (64, 64, 32), 64, k=1, act=1, inst=("w1", ((2, 128),), 9), fwd=S1, bw={"c.dgrad_multi": S1}),  # 2 + 5 tiles, 10 pairs
    _r("w1-2-64", "wgrad1", 2, 47, 45, (256,), 32, k=1, act=1, inst=("w1", ((2, 64),), 17), fwd=S1, bw={"c.dgrad_multi": S1}),        # 1 + 8 tiles, 8 pairs; one slice: a multi-destination launch of one
    _r("w1-4-64-store88", "wgrad1", 2, 47, 45, (96, 96), 84, k=1, act=1, inst=("w1", ((4, 64),), 17), fwd=S1, bw={"c.dgrad_multi": S1}),     # 3 + 6 tiles, 18 pairs; Cout_store 88 < CoutP 96
    # 459 -> 153: 5 output tiles, 13 + 1 + 1 input tiles; groups of min(64 / 5, 16 - 5) = 11: launches of 55 pairs <8, 64> and 20 pairs <4, 64>
    _r("w1-8-64-two-launches", "wgrad1", 2, 47, 45, (395, 32, 32), 153, k=1, act=1, inst=("w1", ((8, 64), (4, 64)), 17), fwd=S1,
       bw={"c.dgrad0": S1, "c.dgrad1-2": S1}),
]

GENERIC = [
    # off the fast forms: weight and bias gradient only (no slice asks for a data gradient)
    _r("wg-3x3-w13", "wgrad_generic", 2, 9, 13, (32,), 32, act=1, nograd=(0,), inst=("conv_wgrad_kernel<bf16,bfm>", 1), fwd=B3, bw={}),           # W < 16
    _r("wg-1x1-small", "wgrad_generic", 1, 20, 30, (32,), 32, k=1, act=1, nograd=(0,), inst=("conv_wgrad_kernel<bf16,bfm>", 1), fwd=IG, bw={}),    # 600 pixels < 4096
    # a 1x1 with nco * nkc = 3 * 4 = 12 that wgrad1x1_bf16_supported refuses: a slice with an affine on load
    _r("wg-1x1-allpairs-affine", "wgrad_generic", 2, 47, 45, (64, 64), 96, k=1, act=1, norm=(0,), nograd=(0, 1),
       inst=("conv1x1_wgrad_allpairs_kernel<3,64,bf16>", 17), fwd=IG, bw={}),
    _r("wg-4x4-s2-reflect-wide", "wgrad_generic", 2, 10, 12, (16,), 128, k=4, pad=(1, 1), stride=2, pad_mode=1, act=1, nograd=(0,),
       inst=("conv_wgrad_wide_kernel<false>", 1), fwd=IG, bw={}),
    _r("wg-7x7-c3-cout64", "wgrad_generic", 2, 23, 45, (3,), 64, k=7, pad=(3, 3), pad_mode=1, act=1, nograd=(0,),
       inst=("conv_wgrad_wide_kernel<true>", 3), fwd=IG, bw={}),                                     # 2070 pixels: ceil(M / 1024) = 3 splits
    _r("wg-7x7-c3-cout32", "wgrad_generic", 1, 12, 14, (3,), 32, k=7, pad=(3, 3), pad_mode=1, act=1, nograd=(0,),
       inst=("conv_wgrad_kernel<bf16,bfm,fold>", 1), fwd=IG, bw={}),
]

# multi-destination 1x1 through the C entry: multi = (gz channels, ((destination channels, residual, masked, sums), ...)); inst: <NKS> and k-steps
MULTI = [
    _r("multi-1-step", "multi", 2, 24, 32, (32,), 32, k=1, inst=("multi", 1, 1), multi=(32, ((32, False, False, False), (32, True, True, True)))),
    _r("multi-4-steps-last-8", "multi", 1, 30, 40, (104,), 100, k=1, inst=("multi", 4, 4), multi=(104, ((102, True, True, True), (100, False, False, False)))),
    _r("multi-5-on-6", "multi", 2, 15, 20, (160,), 128, k=1, inst=("multi", 6, 5), multi=(160, ((128, False, True, False), (115, False, False, False)))),
    _r("multi-7-on-8", "multi", 2, 15, 20, (200,), 64, k=1, inst=("multi", 8, 7), multi=(200, ((64, True, True, True), (38, False, False, False)))),
    _r("multi-8-steps", "multi", 2, 15, 20, (256,), 32, k=1, inst=("multi", 8, 8), multi=(256, ((32, False, False, False), (32, False, True, False)))),
    # residual over the first 450 of 900 pixels (1.5 frames): ends 2 pixels into a group of 32, odd pixel count (900 = 28 x 32 + 4)
    _r("multi-res-pixels-mid-group", "multi", 3, 15, 20, (64,), 64, k=1, inst=("multi", 2, 2), multi=(64, ((38, "half", True, True), (64, "half", False, False)))),
]

BF16_SWEEP = FWD3 + FWD1 + NARROW + TRAIN3 + DGRAD3 + DGRAD1 + TRAIN1 + GENERIC + MULTI
BF16_IDS = [c["id"] for c in BF16_SWEEP]
FORWARD_ROWS = [c for c in BF16_SWEEP if c["part"] in ("fwd3", "fwd1", "narrow")]
TRAIN_ROWS = [c for c in BF16_SWEEP if c["part"] in ("wgrad3", "dgrad3", "dgrad1", "wgrad1", "wgrad_generic")]
MULTI_ROWS = [c for c in BF16_SWEEP if c["part"] == "multi"]

# every instantiation the sweep must keep reaching (tests/test_host_bf16_refs.py walks this set against what the rules say of the rows)
REQUIRED = (
    # conv3x3_bf16.hip: forward and data gradient
    {("b3", k, 1, 0) for k in (1, 2, 3, 4, 0)} | {("b3", 1, 2, 0), ("b3", 2, 2, 0), ("b3", 0, 2, 0)}
    | {("b3", k, 1, r) for k in (1, 2, 3, 4, 0) for r in (1, 2)} | {("b3", k, 2, 1) for k in (1, 2, 0)}
    # conv1x1_bf16.hip
    | {("s1", 2, 4, False), ("s1", 4, 4, False), ("s1", 4, 8, False), ("s1", 2, 4, True), ("s1", 4, 4, True), ("s1", 4, 8, True)}
    | {("multi", n) for n in (1, 2, 3, 4, 6, 8)}
    # conv_narrow_bf16.hip
    | {("narrow", k, n) for k in (7, 5, 3) for n in (2, 1)}
    # wgrad_bf16.hip
    | {("pair",), ("quad",)} | {("w1", p, c) for p, c in ((1, 256), (1, 128), (2, 128), (2, 64), (4, 64), (8, 64))} | {("w1", "two launches")}
    # backward.hip, bf16 branches of wgrad_impl
    | {("conv_wgrad_kernel<bf16,bfm>",), ("conv_wgrad_kernel<bf16,bfm,fold>",), ("conv_wgrad_wide_kernel<false>",), ("conv_wgrad_wide_kernel<true>",),
       ("conv1x1_wgrad_allpairs_kernel<3,64,bf16>",)})


def layers_of(case):
    """The training graph of a row: its ``layers``, or one layer ``c`` over all input slices."""
    if case["layers"] is not None:
        return case["layers"]
    return (dict(name="c", src=tuple("x%d" % i for i in range(len(case["chans"]))), Cout=case["Cout"], k=case["k"], pad=case["pad"], act=case["act"],
                 norm=case["norm"], nograd=case["nograd"], stride=case["stride"], pad_mode=case["pad_mode"], bias=True),)


def chans_of(case, name):
    """Channels of the tensor ``name`` of a row: an input slice x<i> or a layer's output."""
    if name[0] == "x" and name[1:].isdigit():
        return case["chans"][int(name[1:])]
    return {ly["name"]: ly["Cout"] for ly in layers_of(case)}[name]


def cout_store(case):
    return case["cout_pad"] or pad8(case["Cout"])


def instantiations(case):
    """What the row claims, as members of REQUIRED."""
    inst, part = case["inst"], case["part"]
    if part in ("fwd3", "fwd1", "narrow"):
        return {inst}
    if part in ("dgrad3", "dgrad1"):
        return set(inst)
    if part == "multi":
        return {inst[:2]}
    if part == "wgrad1":
        return ({("w1",) + pc for pc in inst[1]} | ({("w1", "two launches")} if len(inst[1]) > 1 else set())
                | ({plan_multi_form(case)[:2]} if "c.dgrad_multi" in case["bw"] else set()))
    return {inst[:1]}


# ---- launcher rules ----------------------------------------------------------------------------------------------------------------

def _b3(Cp, CoutP, rm):
    """<KCH, MB, RM> of egne_conv3x3_bf16_fwd with its default switches: two 32-channel output blocks per workgroup wherever the pack
    has them and the launch is no mask-on-write; resident weights for Ktot 32 .. 128 with one block, 32 / 64 with two; else streamed."""
    Ktot = pad32(Cp)
    mb = 2 if (CoutP >= 64 and rm < 2) else 1
    kch = ({32: 1, 64: 2} if mb == 2 else {32: 1, 64: 2, 96: 3, 128: 4}).get(Ktot, 0)
    return ("b3", kch, mb, rm)


def b3_walk(H, W, B, Cout_store, mb):
    """(ntiles, nrun, nworkers): 256 workgroups; the nrun = ceil(Cout_store / (32 MB)) blocks of a worker share an XCD, 32 / nrun workers
    on each of the 8 XCDs; worker w takes tiles w, w + nworkers, ..."""
    ntiles = ((W + TW - 1) // TW) * ((H + TH - 1) // TH) * B
    nrun = (Cout_store + 32 * mb - 1) // (32 * mb)
    return ntiles, nrun, (32 // nrun) * 8


def b3_form(case):
    """Forward rows and single-layer training rows: the instantiation of the FORWARD launch."""
    rm = 1 if case["residual"] else 0
    return _b3(pad8(case["chans"][0]), pad32(case["Cout"]), rm)


def dgrad3_forms(case):
    """Data-gradient launches of a training row in the order the backward plan emits them: [(name, <KCH, MB, RM>)].  A data gradient is
    the 3x3 over gz (Cout_store channels) onto the slice's C channels; RM 0 for the first writer of a gradient slice, 1 for a later one,
    2 where it is the last writer of the slice of a layer of the plan (mask on write)."""
    layers = layers_of(case)
    produced = {ly["name"] for ly in layers}
    readers = {}
    for ly in layers:
        for s in ly["src"]:
            readers.setdefault(s, []).append(ly["name"])
    out, seen = [], set()
    for ly in reversed(layers):
        if ly["k"] != (3, 3) or ly["stride"] != 1 or ly["pad_mode"] != 0 or ly["pad"] != (1, 1):
            continue
        for i, s in enumerate(ly["src"]):
            if i in ly["nograd"]:
                continue
            first = s not in seen
            seen.add(s)
            last_of_produced = s in produced and readers[s] == [ly["name"]]
            rm = 2 if last_of_produced else (0 if first else 1)
            out.append(("%s.dgrad%d" % (ly["name"], i), _b3(pad8(ly["Cout"]), pad32(chans_of(case, s)), rm)))
    return out


def _wgs_per_cu(lds):
    return max(1, min(8, 163840 // ((lds + 1023) // 1024 * 1024)))


def _s1_lds(nks, nb, nw=4):
    return nks * nb * 1024 + nw * 32 * (16 * nb + 4) * 4


def s1_steps(cps):
    """k-steps of 32 channels, slice by slice (make_tab): a slice of Cp 40 takes two, the second with 8 channels."""
    return sum((cp + 31) // 32 for cp in cps)


def s1_form(case):
    """<NB16, NW, UP> of egne_conv1x1_bf16_fwd, or ("multi", NKS) of egne_conv1x1_bf16_multi_fwd; (the k-step count: s1_steps).  16-channel
    blocks per workgroup: all up to 4, else pieces of 4 (nb16 % 4 == 0) or 2; eight waves where the resident weights leave room for
    one four-wave workgroup per compute unit only."""
    if case["part"] == "multi":
        nks = s1_steps([pad8(case["multi"][0])])
        return ("multi", {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}[nks], nks)
    return _s1([pad8(c) for c in case["chans"]], pad32(case["Cout"]), case["up"] is not None)


def _s1(cps, CoutP, up):
    """<NB16, NW, UP> of egne_conv1x1_bf16_fwd for input slices of ``cps`` padded channels and a pack of CoutP rows."""
    nks = s1_steps(cps)
    nb16 = CoutP // 16
    nb = nb16 if nb16 <= 4 else (4 if nb16 % 4 == 0 else 2)
    assert _s1_lds(nks, nb) <= 120 * 1024
    nw = 8 if (nb == 4 and 8 * _wgs_per_cu(_s1_lds(nks, nb, 8)) > 4 * _wgs_per_cu(_s1_lds(nks, nb, 4)) and _s1_lds(nks, nb, 8) <= 156 * 1024) else 4
    return ("s1", nb, nw, bool(up))


def dgrad1_forms(case):
    """Data-gradient launches of the 1x1 layers of a training row on the streaming kernel, in the order the backward plan emits them:
    [(name, <NB16, NW, UP>, accumulates)].  Plan._bw_conv merges runs of adjacent un-padded raw slices of one buffer of up to 64 channels
    into one launch (name.dgrad<i>-<j>); the first writer of a slice stores, a later one accumulates through the residual.  (Rows whose
    slices do not merge take the multi-destination kernel: bf16_refs rows name those launches in ``bw``.)"""
    out, seen = [], set()
    for ly in reversed(layers_of(case)):
        if ly["k"] != (1, 1):
            continue
        cs = [chans_of(case, s) for s in ly["src"]]
        i = 0
        while i < len(cs):
            j = i
            ok = lambda q: q not in ly["nograd"] and q not in ly["norm"] and cs[q] % 8 == 0 and ly["src"][q][0] == "x"      # noqa: E731
            while ok(i) and j + 1 < len(cs) and ok(j + 1) and sum(cs[i:j + 2]) <= 64:
                j += 1
            if j > i:
                key = tuple(ly["src"][i:j + 1])
                out.append(("%s.dgrad%d-%d" % (ly["name"], i, j), _s1([pad8(ly["Cout"])], pad32(sum(cs[i:j + 1])), False), key in seen))
                seen.add(key)
            i = j + 1
    return out


def plan_multi_form(case):
    """("multi", NKS, k-steps, destinations) of the name.dgrad_multi launch of a single-layer 1x1 training row: Plan._multi_dgrad hands the
    data gradients of all raw slices to ONE egne_conv1x1_bf16_multi_fwd over gz (Cout_store channels: its k-steps)."""
    nks = s1_steps([pad8(case["Cout"])])
    return ("multi", {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8}[nks], nks, len(case["chans"]))


def narrow_form(case):
    """<K, NCH> of egne_conv_narrow_bf16_fwd, None where egne_conv_narrow_bf16_supported refuses."""
    kh, kw = case["k"]
    cp = pad8(case["chans"][0])
    ok = (kh == kw and kh in (7, 5, 3) and case["stride"] == 1 and case["pad_mode"] == 0 and len(case["chans"]) == 1 and cp in (32, 64)
          and not case["norm"] and cout_store(case) <= 8 and cout_store(case) % 4 == 0 and not case["residual"])
    return ("narrow", kh, cp // 32) if ok else None


def wgrad_form(case, layer=None):
    """The weight-gradient launch of ``layer`` (default: the row's first layer) as wgrad_impl decides it for bf16 tensors, with the split
    count egne_conv2d_wgrad_splits answers: ("pair" | "quad", splits), ("w1", ((PPW, CH) per launch), splits) or (generic kernel, splits)."""
    ly = layer or layers_of(case)[0]
    B, H, W = case["B"], case["H"], case["W"]
    kh, kw = ly["k"]
    cps = [pad8(chans_of(case, s)) for s in ly["src"]]
    Ktot, CoutP, nco = sum(cps), pad32(ly["Cout"]), pad32(ly["Cout"]) // 32
    d = 1
    Ho, Wo = (H + 2 * ly["pad"][0] * d - d * (kh - 1) - 1) // ly["stride"] + 1, (W + 2 * ly["pad"][1] * d - d * (kw - 1) - 1) // ly["stride"] + 1
    M = B * Ho * Wo
    raw = not ly["norm"]
    plain = ly["stride"] == 1 and ly["pad_mode"] == 0
    if (kh, kw) == (3, 3) and plain and ly["pad"] == (1, 1) and len(cps) == 1 and W >= 16:          # wgrad3x3_bf16_supported
        tiles = ((W + TW - 1) // TW) * ((H + TH - 1) // TH) * B
        nkc = (Ktot + 31) // 32
        wide = CoutP >= 64 and Ktot > 32 and raw                                                    # wgrad3x3_wide
        units = ((nco + 1) // 2) * ((nkc + 1) // 2) if wide else nco * nkc
        return ("quad" if wide else "pair", max(1, min(256 // units, tiles)))
    nkc = sum((cp + 31) // 32 for cp in cps)
    if (kh, kw) == (1, 1) and plain and ly["pad"] == (0, 0) and raw and nco <= 12 and M >= S1_MIN_PIX:   # wgrad1x1_bf16_supported
        group = min(64 // nco, 16 - nco, nkc)                                                      # w1_group (W1_MAXT = 16 staged tiles)
        nt = nco + group
        ch = 256 if nt <= 4 else (128 if nt <= 8 else 64)                                          # w1_chunk
        launches = []
        for k0 in range(0, nkc, group):
            ppw = (nco * min(group, nkc - k0) + 7) // 8
            launches.append((1, 256) if ch == 256 else ((1 if ppw <= 1 else 2, 128) if ch == 128 else ((2 if ppw <= 2 else (4 if ppw <= 4 else 8)), 64)))
        return ("w1", tuple(launches), max(1, min(512, (M + ch * 4 - 1) // (ch * 4))))
    if (kh, kw) == (1, 1) and plain and ly["pad"] == (0, 0) and nco + nkc <= 12 and 6 <= nco * nkc <= 32 and M >= S1_MIN_PIX:   # w1_supported (fp32 products)
        ch = 64 if (nco + nkc) * 64 * 36 * 4 <= 78 * 1024 else 32
        ppw = (nco * nkc + 3) // 4
        p = (ppw if ppw <= 4 else 8) if ch == 64 else (2 if ppw <= 2 else (4 if ppw <= 4 else 8))
        return ("conv1x1_wgrad_allpairs_kernel<%d,%d,bf16>" % (p, ch), max(1, min(512, (M + ch * 4 - 1) // (ch * 4))))
    T = kh * kw
    tiles = nco * nkc * T
    fold = len(cps) == 1 and cps[0] == 8 and T >= 4            # (the folded forms take an affine on load; the wide one of them does not)
    if fold and CoutP == 64:
        tiles = 2 * (((T + 3) // 4 + 1) // 2)
    splits = max(1, min(4096 // tiles, (M + 1023) // 1024, 512))
    if fold and CoutP == 64 and raw:
        return ("conv_wgrad_wide_kernel<true>", splits)
    if fold:
        return ("conv_wgrad_kernel<bf16,bfm,fold>", splits)
    if CoutP >= 128 and raw:
        return ("conv_wgrad_wide_kernel<false>", splits)
    return ("conv_wgrad_kernel<bf16,bfm>", splits)


# ---- data: forward rows -------------------------------------------------------------------------------------------------------------

def fwd_case(case):
    """Integer data and float64 reference of a forward row: conv_refs.int_case, ternary inputs for the narrow rows (narrow_case)."""
    gen = torch.Generator().manual_seed(case["seed"])
    return narrow_case(gen, case) if case["part"] == "narrow" else R.int_case(gen, case)


def narrow_case(gen, case):
    """As conv_refs.int_case with inputs in {-1, 0, 1}: every (channel, tap) keeps a weight, so a 7x7 over 64 channels sums 3136 products."""
    B, H, W = case["B"], case["H"], case["W"]
    kh, kw = case["k"]
    Cin, Cout = sum(case["chans"]), case["Cout"]
    density = 1.0
    while True:
        data = dict(xs=[R._ints(gen, (B, c, H, W), -1, 1) for c in case["chans"]], ws=[R._weights(gen, (Cout, Cin, kh, kw), density)],
                    bs=[R._ints(gen, (Cout,), 1, 3)], act=ACT_RELU if case["act"] else ACT_NONE, norm=None, residual=None, post=None)
        if data["act"] == ACT_RELU:
            z = R.ref_of(dict(case, act=0), dict(data, act=ACT_NONE))
            data["bs"] = [data["bs"][0] + float(round(0.5 * z.std().item()))]
        want = R.ref_of(case, data)
        if want.abs().max().item() <= BF16_EXACT and R.abs_bound(case, data) < FP32_EXACT:
            break
        density *= 0.5
        assert density > 1e-3, case["id"]
    data["density"] = density
    R.int_conditions(case, data, want)
    return data, want


def up_case(case, data=None):
    """The half-resolution addend P of an up row (integers in [-4, 4], or seeded normal bf16 values when ``data`` is normal data) and
    the float64 value of conv + bias + up2x(P) BEFORE the store: bilinear, align_corners = False -- weights 1/4 and 3/4 per axis, so on
    integer data a multiple of 1/16."""
    gen = torch.Generator().manual_seed(case["seed"] + 1)
    ph, pw = case["up"]
    exact = data is None
    if exact:
        data, want = R.int_case(torch.Generator().manual_seed(case["seed"]), case)
        P = R._ints(gen, (case["B"], case["Cout"], ph, pw), -4, 4)
    else:
        want = R.ref_of(case, data, [w.to(BF).float() for w in data["ws"]])
        P = torch.randn(case["B"], case["Cout"], ph, pw, generator=gen).to(BF).float()
    pre = want + F.interpolate(P.to(D), scale_factor=2, mode="bilinear", align_corners=False)
    return data, P, pre


# ---- data and reference: training rows --------------------------------------------------------------------------------------------------

def _layer_z(case, ly, tensors, w, b, affine, dtype=D, absolute=False):
    """Pre-activation output of one layer in float64: conv_refs.conv_ref without activation over the layer's (affined) input slices."""
    xs = [tensors[s] for s in ly["src"]]
    norm = None
    if ly["norm"] and not absolute and not ly["_exact"] and ly["k"] == (3, 3):
        # normal data: the bf16 3x3 kernels (forward and pair-form weight gradient) round the affined operand to bf16 (as the reference of
        # test_conv3x3_bf16_kernel does); on integer data it is an integer anyway.  Such slices ask for no data gradient.
        xs = list(xs)
        for i in ly["norm"]:
            sc, sh = affine[(ly["name"], i)]
            xs[i] = F.leaky_relu(xs[i].detach() * sc.to(dtype)[:, :, None, None] + sh.to(dtype)[:, :, None, None], 0.01).to(BF).to(dtype)
    elif ly["norm"]:
        norm = {}
        for i in ly["norm"]:
            sc, sh = affine[(ly["name"], i)]
            norm[i] = (sc.abs(), sh.abs(), ACT_NONE) if absolute else (sc, sh, ACT_RELU if ly["_exact"] else ACT_LEAKY)
    return R.conv_ref(xs, [w], [b] if b is not None else None, stride=ly["stride"], pad=ly["pad"], pad_mode=ly["pad_mode"], norm=norm, dtype=dtype)


def train_ref(case, data, y_stored=None, gz_stored=None):
    """Float64 statement of the forward and backward plan of a training row on ``data`` (train_case / train_normal_case).

    Forward: y = act(conv(x') + b) per layer, in order.  Backward, layers in reverse order (Plan.build_backward): gz = g(y) * act'(y),
    the branch taken from the STORED output; bias gradient = sum of gz over pixels; weight gradient and the data gradient of every slice
    of the plain convolution through autograd; a data gradient is added onto the slice's gradient (the first writer stores).
    ``y_stored`` / ``gz_stored``: per layer, the tensors a GPU run stored (normal data: the reference follows the stored, rounded values,
    as test_weight_and_data_gradients_bf16_storage does); None: this function's own.
    Returns y, yc (the output computed from the inputs as stored), gz, gzc (the masked gradient before its store), dW, db per layer, gx per tensor, ``states``: every value a gradient slice held after each writer, and ``bound``: the
    largest magnitude any partial sum of any launch can reach."""
    layers = layers_of(case)
    exact = data["exact"]
    slope = 0.0 if exact else 0.01
    tensors = {"x%d" % i: x.to(D) for i, x in enumerate(data["xs"])}
    y, yc, bound = {}, {}, 0.0
    for ly in layers:
        ly = dict(ly, _exact=exact)
        w = data["w"][ly["name"]].to(D)
        b = data["b"][ly["name"]].to(D)
        z = _layer_z(case, ly, tensors, w, b, data["affine"])
        act = (F.relu(z) if exact else F.leaky_relu(z, 0.01)) if ly["act"] else z
        yc[ly["name"]] = act                         # (computed from the STORED inputs where y_stored names them)
        y[ly["name"]] = act if y_stored is None else y_stored[ly["name"]].to(D)
        tensors[ly["name"]] = y[ly["name"]]
        if exact:
            ab = {k: v.abs() for k, v in tensors.items()}
            bound = max(bound, _layer_z(case, ly, ab, w.abs(), b.abs(), data["affine"], absolute=True).max().item())
    g = {name: gy.to(D).clone() for name, gy in data["gy"].items()}
    gz, gzc, dW, db, states = {}, {}, {}, {}, []
    for ly in reversed(layers):
        ly = dict(ly, _exact=exact)
        name = ly["name"]
        ys = y[name]
        gzl = g[name] * torch.where(ys > 0, 1.0, slope).to(D) if ly["act"] else g[name]
        db[name] = gzl.sum((0, 2, 3))                     # (of the unrounded masked gradient)
        gzc[name] = gzl
        if gz_stored is not None:
            gzl = gz_stored[name].to(D)
        gz[name] = gzl
        ins = {s: tensors[s].detach().clone().requires_grad_(True) for s in ly["src"]}
        w = data["w"][name].to(D).clone().requires_grad_(True)
        z = _layer_z(case, ly, ins, w, None, data["affine"])
        grads = torch.autograd.grad(z, [w] + [ins[s] for s in ly["src"]], gzl, allow_unused=True)
        dW[name] = grads[0]
        for i, s in enumerate(ly["src"]):
            if i in ly["nograd"]:
                continue
            g[s] = grads[1 + i] if s not in g else g[s] + grads[1 + i]
            states.append(("%s after %s.dgrad%d" % (s, name, i), g[s].clone()))
        if exact:
            # partial sums of the weight gradient (over ALL pixels) and of the data gradient: the same sums over magnitudes
            ab = {s: tensors[s].abs().detach().clone().requires_grad_(True) for s in ly["src"]}
            wa = data["w"][name].to(D).abs().clone().requires_grad_(True)
            za = _layer_z(case, ly, ab, wa, None, data["affine"], absolute=True)
            ga = torch.autograd.grad(za, [wa] + [ab[s] for s in ly["src"]], gzl.abs())
            # ... and of the bias gradient / a data gradient's mask sums: sum |gz| over all pixels of a channel
            bound = max([bound, gzl.abs().sum((0, 2, 3)).max().item()] + [t.max().item() for t in ga])
    gx = {s: g[s] for s in g if s in {q for ly in layers for q in ly["src"]}}
    return dict(y=y, yc=yc, gz=gz, gzc=gzc, dW=dW, db=db, gx=gx, states=states, bound=bound)


def _draw_train(gen, case, density, glim):
    layers = layers_of(case)
    B, H, W = case["B"], case["H"], case["W"]
    data = dict(exact=True, xs=[R._ints(gen, (B, c, H, W), -4, 4) for c in case["chans"]], w={}, b={}, affine={}, gy={}, density=density, glim=glim)
    tensors = {"x%d" % i: x.to(D) for i, x in enumerate(data["xs"])}
    consumed = {s for ly in layers for s in ly["src"]}
    for ly in layers:
        kh, kw = ly["k"]
        name, cin = ly["name"], sum(chans_of(case, s) for s in ly["src"])
        for i in ly["norm"]:
            c = chans_of(case, ly["src"][i])
            data["affine"][(name, i)] = (R._pow2(gen, (B, c)), R._ints(gen, (B, c), -3, 3))
        # (conv_refs._weights fills empty (channel, tap) columns with +1: random signs, or a layer over a ReLU output -- positive mean -- sums them up)
        data["w"][name] = R._weights(gen, (ly["Cout"], cin, kh, kw), density) * (torch.randint(0, 2, (ly["Cout"], cin, kh, kw), generator=gen).float() * 2 - 1)
        b = R._ints(gen, (ly["Cout"],), 1, 3)
        lyx = dict(ly, _exact=True)
        z = _layer_z(case, lyx, tensors, data["w"][name].to(D), b.to(D), data["affine"])
        if ly["act"]:
            b = b + float(round(0.5 * z.std().item()))         # (as conv_refs.int_case: 69 % of the outputs stay positive)
            z = _layer_z(case, lyx, tensors, data["w"][name].to(D), b.to(D), data["affine"])
        data["b"][name] = b
        tensors[name] = F.relu(z) if ly["act"] else z
        if name not in consumed:
            data["gy"][name] = R._ints(gen, tuple(z.shape), -glim, glim)
    return data


def train_conditions(case, data, ref):
    """What makes the exact run of a training row exact -- asserted: integers everywhere; every tensor a kernel stores in bf16 (inputs,
    outputs, masked gradients, every state of every gradient slice) within +-256; weights small integers (bf16 values); power-of-two
    affine scales; every partial sum, the weight gradient's sum over all pixels included, below 2^24; at least half of the outputs, of
    the data-gradient elements and of the weight-gradient elements non-zero."""
    ints = list(data["xs"]) + list(data["w"].values()) + list(data["b"].values()) + list(data["gy"].values())
    ints += list(ref["y"].values()) + list(ref["gz"].values()) + list(ref["dW"].values()) + list(ref["db"].values()) + [s for _, s in ref["states"]]
    for t in ints:
        assert torch.equal(t, t.round()), "integer values only"
    stored = list(data["xs"]) + list(data["w"].values()) + list(data["gy"].values()) + list(ref["y"].values()) + list(ref["gz"].values()) + [s for _, s in ref["states"]]
    for t in stored:
        assert t.abs().max().item() <= BF16_EXACT, "a stored value leaves the integers bf16 holds"
        assert torch.equal(t.to(BF).to(t.dtype), t)
    for sc, sh in data["affine"].values():
        m, _ = torch.frexp(sc.abs())
        assert (m == 0.5).all() and torch.equal(sh, sh.round()), "scales are powers of two, shifts integers"
    assert ref["bound"] < FP32_EXACT, "a partial sum may leave the integers fp32 holds"
    for t in list(ref["dW"].values()) + list(ref["db"].values()):
        assert t.abs().max().item() < FP32_EXACT
    for name, t in ref["gz"].items():
        assert t.abs().sum((0, 2, 3)).max().item() < FP32_EXACT, "a partial sum of the bias gradient (or of the mask sums) of %s may leave the integers fp32 holds" % name
    for what, ts in (("outputs", ref["y"]), ("data-gradient elements", ref["gx"]), ("weight-gradient elements", ref["dW"])):
        for name, t in ts.items():
            nz = (t != 0).double().mean().item()
            assert nz >= 0.5, "%s: only %.0f %% of the %s of %s are non-zero" % (case["id"], 100 * nz, what, name)


def _fits(ref):
    stored = list(ref["y"].values()) + list(ref["gz"].values()) + [s for _, s in ref["states"]]
    return all(t.abs().max().item() <= BF16_EXACT for t in stored) and ref["bound"] < FP32_EXACT


@functools.lru_cache(maxsize=None)
def _train_case(id):
    case = next(c for c in BF16_SWEEP if c["id"] == id)
    gen = torch.Generator().manual_seed(case["seed"])
    density, glim = 1.0, 4
    while True:
        data = _draw_train(gen, case, density, glim)
        ref = train_ref(case, data)
        if _fits(ref):
            break
        density *= 0.5
        if density < 1.0 / 256:
            density, glim = 1.0 / 16, glim // 2
            assert glim >= 1, id
    train_conditions(case, data, ref)
    return data, ref


def train_case(case):
    """Integer data of a training row and its reference (train_ref): inputs and output gradients in [-4, 4], weights in [-2, 2]; the
    weight density is halved, then the output gradient narrowed, until JOINTLY every stored tensor fits +-256 and every partial sum
    2^24.  One draw per row and process (the host test and the GPU tests share it)."""
    return _train_case(case["id"])


def train_normal_case(case):
    """Seeded normal data of a training row: bf16-representable inputs and output gradients, weights scaled by 1 / sqrt(K) and rounded to
    bf16 for the layers whose kernels round them (3x3 and 1x1 on the bf16 MFMAs: every row here but the generic weight-gradient rows'
    forward), LeakyReLU where a layer has an activation."""
    gen = torch.Generator().manual_seed(case["seed"] + 4321)
    layers = layers_of(case)
    B, H, W = case["B"], case["H"], case["W"]

    def q(t):
        return t.to(BF).float()
    data = dict(exact=False, xs=[q(torch.randn(B, c, H, W, generator=gen)) for c in case["chans"]], w={}, b={}, affine={}, gy={})
    consumed = {s for ly in layers for s in ly["src"]}
    shape = {"x%d" % i: (H, W) for i in range(len(case["chans"]))}
    for ly in layers:
        kh, kw = ly["k"]
        name, cin = ly["name"], sum(chans_of(case, s) for s in ly["src"])
        for i in ly["norm"]:
            c = chans_of(case, ly["src"][i])
            data["affine"][(name, i)] = (0.5 + torch.randn(B, c, generator=gen).abs(), torch.randn(B, c, generator=gen))
        data["w"][name] = torch.randn(ly["Cout"], cin, kh, kw, generator=gen) / (cin * kh * kw) ** 0.5
        data["b"][name] = torch.randn(ly["Cout"], generator=gen) * 0.5
        h, w_ = shape[ly["src"][0]]
        shape[name] = ((h + 2 * ly["pad"][0] - kh) // ly["stride"] + 1, (w_ + 2 * ly["pad"][1] - kw) // ly["stride"] + 1)
        if name not in consumed:
            data["gy"][name] = q(torch.randn(B, ly["Cout"], *shape[name], generator=gen) * 1e-2)
    return data


# ---- data: multi-destination 1x1 through the C entry -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _multi_case(id, exact):
    case = next(c for c in BF16_SWEEP if c["id"] == id)
    gen = torch.Generator().manual_seed(case["seed"] + (0 if exact else 4321))
    Cs, dsts = case["multi"]
    M = case["B"] * case["H"] * case["W"]
    gz = R._ints(gen, (M, Cs), -4, 4) if exact else torch.randn(M, Cs, generator=gen).to(BF).float()
    out = []
    for Cd, res, masked, sums in dsts:
        Cp = pad8(Cd)
        rp = M // 2 if res == "half" else M
        density = 1.0
        while True:
            if exact:
                w = R._weights(gen, (Cd, Cs), density)
                r0 = R._ints(gen, (M, Cp), -4, 4)
                r0[:, Cd:] = 0                                  # (the padding channels of a gradient slice hold zeros)
                ym = R._ints(gen, (M, Cp), -1, 4)              # (two thirds positive: more than half of a masked destination stays non-zero)
            else:
                w = (torch.randn(Cd, Cs, generator=gen) / Cs ** 0.5)
                r0 = torch.randn(M, Cp, generator=gen).to(BF).float()
                r0[:, Cd:] = 0
                ym = torch.randn(M, Cp, generator=gen).to(BF).float()
            wd = torch.zeros(Cp, Cs, dtype=D)
            wd[:Cd] = (w if exact else w.to(BF).float()).to(D)
            t = gz.to(D) @ wd.t()
            bound = (gz.to(D).abs() @ wd.abs().t()).max().item() + 4
            if res:
                t[:rp] = t[:rp] + r0.to(D)[:rp]
            if masked:
                t = torch.where(ym.to(D) > 0, t, t * (0.0 if exact else 0.01))
            if not exact or (t.abs().max().item() <= BF16_EXACT and bound < FP32_EXACT):
                break
            density *= 0.5
            assert density > 1e-3, id
        if exact:
            assert torch.equal(t, t.round()) and torch.equal(w, w.round()) and w.abs().max().item() <= 2
            nz = (t[:, :Cd] != 0).double().mean().item()
            assert nz >= 0.5, "%s: only %.0f %% of a destination non-zero" % (id, 100 * nz)
        out.append(dict(Cd=Cd, Cp=Cp, w=w, r0=r0 if res else None, rp=rp, ym=ym if masked else None, sums=sums, want=t, density=density))
    return gz, out


def multi_case(case, exact=True):
    """gz [M][Cs] and, per destination, weights, the accumulated residual (over the first ``rp`` pixels), the tensor whose sign masks the
    result (ReLU in the exact run, LeakyReLU on normal data) and the float64 result ``want`` [M][Cp] (padding channels zero)."""
    return _multi_case(case["id"], exact)
