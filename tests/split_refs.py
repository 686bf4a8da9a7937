"""Exactly representable data, a float64 emulation and the sweep table for the split-f16 forward convolution kernels (halo, role-split,
resident-weights, flat, small-problem, deep trunk, streaming / staged 1x1, dilated MSBlock group, first layer).

A split-f16 kernel multiplies an operand by a power of two (``a_scale`` for activations, ``w_scale`` for the weight pack), splits it
as ``hi = f16(t)``, ``lo = f16(t - hi)`` (csrc/split_f16.h and the pack kernels), accumulates ``hi*hi + hi*lo + lo*hi`` in fp32 (the
``lo*lo`` product is dropped; with ``f16_products = 1`` only ``hi*hi``) and multiplies by ``1 / (a_scale * w_scale)`` in its epilogue.
When every ``t`` equals ``hi + lo``, one operand of every product has ``lo = 0`` and every partial sum is below 2^24 units of the
smallest product, nothing is rounded anywhere: the kernel must reproduce the float64 reference conv_refs.conv_ref BIT FOR BIT,
whatever its order of summation.  Three generators make such data for every row of ``SPLIT_SWEEP``:

  int_case            (conv_refs) integers: every lo half is zero -- hi addressing, the epilogue, the slices;
  fine_inputs_case    inputs of 12 to 13 significant bits (lo != 0 for >= 20 % of them) against integer weights -- the lo halves of the
                      ACTIVATIONS: a lo fragment read from another pixel, a dropped lo K tail, swapped planes change the result;
  fine_weights_case   integer inputs against weights of 12 significant bits -- the lo half of the weight PACK.

``split_conditions`` asserts what makes a run exact, ``emulate`` restates the kernel's arithmetic in float64 (tests/test_host_split_refs.py
proves on the CPU that it equals the reference for every row, and that two wrong emulations do not), ``SPLIT_SWEEP`` is the table that
tests/test_gpu_split_f16_sweep.py runs.
"""
import math

import torch

import conv_refs as R
from conv_refs import ACT_LEAKY, ACT_NONE, ACT_RELU, D, FP32_EXACT, _ints, _pow2, _weights, abs_bound, act_ref, conv_ref, int_case, out_hw, pad8, pad32, ref_of  # noqa: F401

F16X3_ASCALE = 16.0           # engine.F16X3_ASCALE: the pre-scale of slices that carry an input affine
LO_DENSITY = 0.2              # least share of operand elements with a non-zero lo half in the fine runs
DEEP = ("egne_conv2d_f16x3_big_fwd", "egne_conv2d_f16_big1_fwd")      # entries whose a_scale is launch argument 2 (3 elsewhere)


def a_scale_for(vmax):
    """engine._a_scale_for: the power of two that puts max |x| in [1024, 2048)."""
    if vmax == 0.0:
        return F16X3_ASCALE
    return 2.0 ** max(-100, min(100, math.floor(math.log2(2048.0 / vmax))))


def w_scale_for(ws):
    """ConvLayer.ensure_packed: one power of two for all groups that puts max |w| in [1024, 2048)."""
    mx = max(float(w.abs().max()) for w in ws)
    return 2.0 ** math.floor(math.log2(2048.0 / mx)) if mx > 0 else 1.0


def scales_for(case, data):
    """(a_scale, w_scale) the engine chooses for the row on ``data``: calibrated from max |x| over the raw slices, 16 for affined ones."""
    if case["norm"]:
        assert len(case["chans"]) == 1
        a = F16X3_ASCALE
    else:
        a = a_scale_for(max(float(x.abs().max()) for x in data["xs"]))
    return a, w_scale_for(data["ws"])


def split_f16(t):
    """(hi, lo) of an fp32 tensor as float64: hi = f16(t), lo = f16(t - hi)."""
    assert t.dtype == torch.float32
    hi = t.half()
    lo = (t - hi.float()).half()
    return hi.double(), lo.double()


def operands(case, data, a_scale, w_scale):
    """The scaled operands as the kernels see them, fp32: per slice act_in(x * scale + shift) * a_scale, per group w * w_scale."""
    xt = []
    for i, x in enumerate(data["xs"]):
        x = x.float()
        if data["norm"] and i in data["norm"]:
            sc, sh, act_in = data["norm"][i]
            x = act_ref(x * sc.float()[:, :, None, None] + sh.float()[:, :, None, None], act_in)
        xt.append(x * a_scale)
    return xt, [w.float() * w_scale for w in data["ws"]]


def halves(case, data, a_scale, w_scale):
    """(xh, xl, wh, wl): lists of the float64 hi / lo halves of the scaled operands."""
    xt, wt = operands(case, data, a_scale, w_scale)
    xs, ws = [split_f16(t) for t in xt], [split_f16(t) for t in wt]
    return [h for h, _ in xs], [l for _, l in xs], [h for h, _ in ws], [l for _, l in ws]


def emulate_terms(case, data, terms, a_scale, w_scale):
    """Float64 convolution of a sum of operand products through the row's epilogue: ``terms`` lists (x halves per slice, w halves per
    group) pairs in the scaled domain; sum_t conv(x_t, w_t) is ONE convolution over the terms' channels laid side by side."""
    xs = [x / a_scale for xt, _ in terms for x in xt]
    G = len(data["ws"])
    ws = [torch.cat([wt[g] for _, wt in terms], 1) / w_scale for g in range(G)]
    return conv_ref(xs, ws, data["bs"], stride=case["stride"], pad=case["pad"], dils=case["dils"], act=data["act"], pad_mode=case["pad_mode"],
                    residual=data["residual"], post=data["post"])


def emulate(case, data, a_scale, w_scale, products):
    """What a split-f16 kernel computes, in float64: hi*hi + hi*lo + lo*hi (products = 3) or hi*hi (products = 1), divided by the
    scales, through bias, activation, post affine and residual."""
    xh, xl, wh, wl = halves(case, data, a_scale, w_scale)
    terms = [(xh, wh)] if products == 1 else [(xh, [h + l for h, l in zip(wh, wl)]), (xl, wh)]
    assert products in (1, 3)
    return emulate_terms(case, data, terms, a_scale, w_scale)


# ---- wrong emulations (what an addressing error in a lo half looks like) -----------------------------------------------------------

def emulate_lo_shifted(case, data, a_scale, w_scale):
    """The lo half of the fine operand taken one pixel to the left: lo(x) rolled in x, or -- for fine weights -- the hi(x) * lo(w)
    product reading its activations one pixel off."""
    xh, xl, wh, wl = halves(case, data, a_scale, w_scale)
    roll = lambda ts: [torch.roll(t, 1, dims=3) for t in ts]      # noqa: E731
    if data["fine"] == "inputs":
        terms = [(xh, [h + l for h, l in zip(wh, wl)]), (roll(xl), wh)]
    else:
        terms = [(xh, wh), (roll(xh), wl), (xl, wh)]
    return emulate_terms(case, data, terms, a_scale, w_scale)


def emulate_lo_tail_dropped(case, data, a_scale, w_scale):
    """The lo halves of the fine operand zeroed in the last K chunk (the channels of the last slice beyond its last multiple of 32);
    rows of at most 32 input channels drop the lo halves of the last tap instead."""
    xh, xl, wh, wl = halves(case, data, a_scale, w_scale)
    Cin = sum(case["chans"])
    last = case["chans"][-1]
    tail = last - (last - 1) // 32 * 32
    xl, wl, wh_lo = [t.clone() for t in xl], [t.clone() for t in wl], [t.clone() for t in wh]
    if Cin > 32:
        xl[-1][:, last - tail:] = 0
        for t in wl:
            t[:, Cin - tail:] = 0
    else:
        for t in wl + wh_lo:          # wh_lo: the weights lo(x) is multiplied with
            t[:, :, -1, -1] = 0
    if data["fine"] == "inputs":
        terms = [(xh, [h + l for h, l in zip(wh, wl)]), (xl, wh_lo if Cin <= 32 else wh)]
    else:
        terms = [(xh, wh), (xh, wl), (xl, wh)]
    return emulate_terms(case, data, terms, a_scale, w_scale)


def emulate_last_group_dropped(case, data, a_scale, w_scale):
    """The last group of (up to) eight input channels left out."""
    xh, xl, wh, wl = halves(case, data, a_scale, w_scale)
    xh = [t.clone() for t in xh]
    xh[-1][:, -min(8, case["chans"][-1]):] = 0
    return emulate_terms(case, data, [(xh, [h + l for h, l in zip(wh, wl)]), (xl, wh)], a_scale, w_scale)


# ---- conditions --------------------------------------------------------------------------------------------------------------------

def granule(ts):
    """Largest power of two that divides every element of the tensors (2^e, e in [-16, 16])."""
    for e in range(16, -17, -1):
        g = 2.0 ** e
        if all(torch.equal((t.double() / g).round() * g, t.double()) for t in ts):
            return g
    raise AssertionError("finer than 2^-16")


def lo_density(case, data, a_scale, w_scale):
    """Share of the fine operand's elements whose lo half is non-zero: of all input elements, or of the non-zero weights."""
    _, xl, _, wl = halves(case, data, a_scale, w_scale)
    if data["fine"] == "inputs":
        return sum(int((t != 0).sum()) for t in xl) / sum(t.numel() for t in xl)
    return sum(int((t != 0).sum()) for t in wl) / max(1, sum(int((w != 0).sum()) for w in data["ws"]))


def bound_units(case, data, a_scale, w_scale):
    """(largest magnitude a partial sum can reach, in units; the unit).  The unit is what every partial sum is a multiple of: the
    smallest product of two halves in the scaled domain, brought back by 1 / (a_scale * w_scale), or the grid of what the epilogue
    adds, whichever is finer; the magnitude is conv_refs.abs_bound (sum |x'| |w| + |b| through the epilogue)."""
    xh, xl, wh, wl = halves(case, data, a_scale, w_scale)
    epi = list(data["bs"]) + ([data["residual"]] if data["residual"] is not None else []) + ([data["post"][1]] if data["post"] is not None else [])
    unit = min(granule(xh + xl) * granule(wh + wl) / (a_scale * w_scale), granule(epi))
    return abs_bound(case, data) / unit, unit


def split_conditions(case, data, want, a_scale, w_scale):
    """What makes a split-f16 run of ``data`` exact -- conditions on the data, none of them a tolerance: power-of-two scales; every scaled
    operand equals hi + lo; one operand of every product has no lo half at all; every partial sum, through the epilogue, is at most
    2^24 units of the smallest product; the reference is an fp32 value; no LeakyReLU.  And what makes it a test: at least half of the
    outputs non-zero, at least 20 % non-zero lo halves in a fine run."""
    for s in (a_scale, w_scale):
        assert math.frexp(s)[0] == 0.5, "scales are powers of two"
    assert data["act"] in (ACT_NONE, ACT_RELU)
    tables = []
    for sc, sh, act_in in (data["norm"] or {}).values():
        assert act_in in (ACT_NONE, ACT_RELU)
        tables.append(sc)
    if data["post"] is not None:
        tables.append(data["post"][0])
    for sc in tables:
        assert (torch.frexp(sc.abs())[0] == 0.5).all(), "affine scales are powers of two"
    xt, wt = operands(case, data, a_scale, w_scale)
    xh, xl, wh, wl = halves(case, data, a_scale, w_scale)
    for t, h, l in zip(xt + wt, xh + wh, xl + wl):
        assert torch.equal(h + l, t.double()), "an operand does not split into two f16 halves"
        assert torch.isfinite(h).all() and h.abs().max().item() <= 4096
    x_plain, w_plain = all((l == 0).all() for l in xl), all((l == 0).all() for l in wl)
    assert x_plain or w_plain, "both operands carry lo halves: the dropped lo*lo product would show"
    units, unit = bound_units(case, data, a_scale, w_scale)
    assert units <= FP32_EXACT, "%s: a partial sum may reach %.3g units of %g" % (case["id"], units, unit)
    assert torch.equal(want.float().double(), want), "the reference is not an fp32 value"
    nz = (want != 0).double().mean().item()
    assert nz >= 0.5, "only %.0f %% of the outputs are non-zero" % (100 * nz)
    if data["fine"]:
        assert (w_plain if data["fine"] == "inputs" else x_plain)
        dens = lo_density(case, data, a_scale, w_scale)
        assert dens >= LO_DENSITY, "%s: only %.1f %% of the lo halves are non-zero" % (case["id"], 100 * dens)
    else:
        assert x_plain and w_plain
    return units


# ---- data --------------------------------------------------------------------------------------------------------------------------

def _halves_of(gen, shape, lo, hi):
    return _ints(gen, shape, lo, hi) / 2


def _fine_case(gen, case, which):
    """int_case with ONE operand on a finer grid (see fine_inputs_case / fine_weights_case); everything the epilogue adds on
    multiples of 0.5, scales powers of two, LeakyReLU rows with ReLU.  The weight density is halved until split_conditions' bound holds."""
    B, H, W = case["B"], case["H"], case["W"]
    kh, kw = case["k"]
    Cin, Cout, G = sum(case["chans"]), case["Cout"], len(case["dils"])
    Ho, Wo = out_hw(case)
    density = 1.0
    while True:
        norm = {i: (_pow2(gen, (B, case["chans"][i])), _ints(gen, (B, case["chans"][i]), -3, 3), ACT_RELU) for i in case["norm"]} or None
        xs = []
        for i, c in enumerate(case["chans"]):
            if which == "weights":
                x = _ints(gen, (B, c, H, W), -4, 4)
            elif norm and i in norm:
                # the affined value v = x * scale + shift on multiples of 1 / 32 below 128 (16 v: multiples of 0.5 below 2048); three of four
                # positive (the ReLU keeps them), four of five of 12 significant bits: x = (v - shift) / scale, exact in fp32 both ways
                m = torch.where(torch.rand((B, c, H, W), generator=gen) < 0.8, 2048 + _ints(gen, (B, c, H, W), 0, 2047), _ints(gen, (B, c, H, W), 0, 4095))
                m = m * torch.where(torch.rand((B, c, H, W), generator=gen) < 0.75, 1.0, -1.0)
                sc, sh, _ = norm[i]
                x = (m / 32 - sh[:, :, None, None]) / sc[:, :, None, None]
            else:
                x = _halves_of(gen, (B, c, H, W), -4095, 4095)
            xs.append(x)
        if which == "inputs" and not norm:
            xs[0][0, 0, 0, 0] = 2047.5          # max |x| in (1024, 2048]: the calibrated a_scale is 1
        ws = [_weights(gen, (Cout, Cin, kh, kw), density) for _ in range(G)]
        if which == "weights":
            # the pattern of _weights (every (channel, tap) pair keeps a weight), magnitudes r / 2 with r in [1, 4095]
            ws = [torch.sign(w) * _halves_of(gen, w.shape, 1, 4095) for w in ws]
            ws[0].view(-1)[int(ws[0].view(-1).nonzero()[0])] = 2047.5       # max |w| in (1024, 2048]: w_scale is 1
        data = dict(xs=xs, ws=ws, bs=[_ints(gen, (Cout,), 1, 3) for _ in range(G)], act=ACT_RELU if case["act"] else ACT_NONE, norm=norm,
                    residual=_halves_of(gen, (B, Cout, Ho, Wo), -8, 8) if case["residual"] else None,
                    post=(_pow2(gen, (Cout,)), _halves_of(gen, (Cout,), -6, 6)) if case["post"] else None, fine=which)
        if data["act"] == ACT_RELU:      # as int_case: lift the bias by half a standard deviation of the pre-activation
            z = conv_ref(xs, ws, data["bs"], stride=case["stride"], pad=case["pad"], dils=case["dils"], pad_mode=case["pad_mode"], norm=norm)
            lift = float(round(0.5 * z.std().item() / G ** 0.5))
            data["bs"] = [b + lift for b in data["bs"]]
        want = ref_of(case, data)
        if bound_units(case, data, *scales_for(case, data))[0] <= FP32_EXACT:
            break
        density *= 0.5
        assert density > 1e-3, case["id"]
    data["density"] = density
    return data, want


def fine_inputs_case(gen, case):
    """Inputs of 12 to 13 significant bits, integer weights in [-2, 2] (w_scale 1024, no lo half).  Raw slices hold q / 2 with integer
    |q| <= 4095 and one planted 2047.5 (a_scale 1); affined slices (a_scale 16) hold what makes 16 relu(x scale + shift) a multiple of 0.5
    below 2048.  Returns the data and the float64 reference."""
    return _fine_case(gen, case, "inputs")


def fine_weights_case(gen, case):
    """Integer inputs in [-4, 4] (no lo half under any a_scale), weights r / 2 with integer |r| <= 4095, thinned as conv_refs._weights
    thins, one planted 2047.5 (w_scale 1).  Returns the data and the float64 reference."""
    return _fine_case(gen, case, "weights")


def int_case_split(gen, case):
    data, want = int_case(gen, case)
    data["fine"] = None
    return data, want


def normal_case(gen, case):
    data = R.normal_case(gen, case)
    data["fine"] = None
    return data


GENERATORS = {"int": int_case_split, "fine_inputs": fine_inputs_case, "fine_weights": fine_weights_case}
SEED = 1234
_CACHE = {}


def exact_case(kind, case):
    """(data, want, a_scale, w_scale) of generator ``kind`` for the row, computed once per process and shared (do not modify)."""
    key = (kind, case["id"])
    if key not in _CACHE:
        data, want = GENERATORS[kind](torch.Generator().manual_seed(SEED), case)
        _CACHE[key] = (data, want) + scales_for(case, data)
    return _CACHE[key]


# ---- the sweep table ---------------------------------------------------------------------------------------------------------------

def _r(id, B, H, W, chans, Cout, kind, entry, k=(3, 3), pad=(1, 1), dils=(1,), act=ACT_NONE, norm=(), residual=False, post=False, products=3,
       switches=None, stats=False, launches=1, runs=1, one=False, second_buffer=False):
    """One row: conv_refs._c's geometry plus ``kind`` (Plan.meta), ``entry`` (the _lib symbol launched), ``products`` (the plan's
    f16_products: 3 products or 1), ``switches`` (engine attributes for the row only), ``stats`` (InstanceNorm statistics from the
    epilogue), ``launches`` (launches of that kind the layer takes), ``runs`` (extra identical runs on one plan), ``one`` (a 1x1 layer:
    ConvLayer.split1), ``second_buffer`` (the last input slice lives in a buffer of its own)."""
    c = R._c(id, B, H, W, chans if isinstance(chans, tuple) else (chans,), Cout, k, pad=pad, dils=dils, act=act, norm=norm, residual=residual,
             post=post, form=kind, tile=())
    sw = dict(SMALL_ENABLED=False)
    sw.update(switches or {})
    c.update(kind="conv_f16x3:" + kind, entry=entry, products=products, switches=sw, stats=stats, launches=launches, runs=runs, one=one,
             second_buffer=second_buffer)
    return c


_HALO, _RS, _RW = "egne_conv3x3_halo_f16_fwd", "egne_conv3x3_rs_f16_fwd", "egne_conv3x3_rw_f16_fwd"
_FLAT, _SMALL, _BIG, _BIG1 = "egne_conv2d_f16x3_fwd", "egne_conv2d_f16x3_small_fwd", "egne_conv2d_f16x3_big_fwd", "egne_conv2d_f16_big1_fwd"
_S1, _M1, _DIL, _FIRST = "egne_conv1x1_f16x3_fwd", "egne_conv1x1_ms_f16x3_fwd", "egne_msblock_dil_f16_fwd", "egne_conv3x3_smallcin_f16_fwd"
_ONE = dict(k=(1, 1), pad=(0, 0), one=True, switches=dict(S1X1_MIN_PIX=0, MS1X1_MIN_PIX=0))
_GRP = dict(residual=True, act=ACT_RELU)

SPLIT_SWEEP = [
    # ---- conv_halo_f16.hip: 32x8-pixel tiles, the whole K loop in one workgroup
    _r("halo-n32", 3, 9, 33, 32, 32, "halo", _HALO, act=ACT_RELU),              # plain walk (4 tiles against 5 transposed); last tile column 1 pixel wide, last tile row 1 row
    _r("halo-n64-tall", 2, 63, 41, 32, 64, "halo", _HALO, post=True),          # transposed walk (12 against 16 tiles), ragged both ways
    _r("halo-dil2-affine", 2, 11, 35, 64, 32, "halo", _HALO, dils=(2,), norm=(0,), act=ACT_LEAKY),   # zero padding AFTER the affine; halo of 2
    _r("halo-n96", 2, 10, 37, 96, 96, "halo", _HALO),                          # the 96-wide tile; three K chunks
    _r("halo-tail16-n192", 2, 9, 64, 40, 160, "halo", _HALO, act=ACT_LEAKY),   # 33..48 channels at W >= 60: K tail of 8; three 64-wide N tiles, 160 of 192 channels stored
    _r("halo-second-tile", 22, 41, 97, 32, 32, "halo", _HALO, dils=(2,)),      # 528 tiles over 512 workgroups: 16 take a second tile
    _r("halo-np1", 2, 9, 33, 96, 64, "halo", _HALO, products=1),               # the NP = 1 build
    # ---- conv3x3_rs_f16.hip (register ring; reached with statistics, or with the resident-weights form off)
    _r("rs-1x1x8", 3, 9, 65, 32, 32, "rs", _RS, stats=True, act=ACT_LEAKY),    # <1, 1, 8>; 32x8 tiles, last column 1 pixel, last row 1 row
    _r("rs-1x2x8", 2, 9, 61, 32, 64, "rs", _RS, stats=True),                   # <1, 2, 8>
    _r("rs-2x1x4", 2, 5, 65, 64, 32, "rs", _RS, stats=True, act=ACT_RELU),     # TH 4: last tile row of 1
    _r("rs-2x2x4-affine", 2, 5, 61, 56, 64, "rs", _RS, stats=True, norm=(0,), act=ACT_LEAKY),   # K tail 24
    _r("rs-2x4x4", 2, 5, 65, 64, 100, "rs", _RS, stats=True),                  # 104 of 128 channels stored
    _r("rs-second-tile", 17, 13, 97, 64, 32, "rs", _RS, stats=True, act=ACT_RELU),   # 272 tiles over 256 workgroups
    _r("rs-tpo-64-64", 2, 5, 65, 64, 64, "rs", _RS, switches=dict(RW_ENABLED=False), act=ACT_LEAKY),   # transposed-store build
    _r("rs-tpo-64-32-res", 2, 5, 65, 64, 32, "rs", _RS, switches=dict(RW_ENABLED=False), residual=True, act=ACT_RELU),   # transposed-store build + residual
    # ---- conv3x3_rw_f16.hip (resident / streamed weights)
    _r("rw-k1", 3, 9, 65, 32, 32, "rw", _RW, act=ACT_RELU),                    # one resident chunk, one output block
    _r("rw-k2-res-post", 2, 9, 61, 64, 64, "rw", _RW, residual=True, post=True, act=ACT_LEAKY),   # two chunks, two output blocks
    _r("rw-3of4-second-tile", 3, 65, 65, 64, 96, "rw", _RW),                   # three computed blocks of four packed; 80 workers for 81 tiles; two idle workgroups per XCD
    _r("rw-streamed", 2, 9, 121, 128, 32, "rw", _RW, act=ACT_RELU),            # weights streamed, four chunks
    _r("rw-streamed-tail", 2, 9, 121, 72, 24, "rw", _RW, norm=(0,), act=ACT_LEAKY),   # Ktot 96 with a K tail of 8; 24 of 32 channels stored
    _r("rw-np1", 2, 9, 33, 64, 64, "rw", _RW, products=1),                     # NP = 1 build (reached at W >= 30)
    # ---- conv_f16x3.hip, flat: M x N tiles over the B * Ho * Wo rows
    _r("flat-256x32", 3, 9, 10, 32, 32, "flat", _FLAT, act=ACT_RELU),          # M = 270: second tile of 14 rows; frames cross the tile
    _r("flat-256x64-5x5", 3, 9, 10, 64, 64, "flat", _FLAT, k=(5, 5), pad=(2, 2)),   # 256x64 tile, 25 taps
    _r("flat-128x128-dil3", 3, 9, 10, 40, 100, "flat", _FLAT, dils=(3,), act=ACT_LEAKY),   # pack rounded to 128; K tail; reach 3
    _r("flat-32taps", 2, 6, 7, 32, 32, "flat", _FLAT, k=(4, 8), pad=(1, 3)),   # the last bit of the tap mask
    _r("flat-grouped", 3, 9, 10, 32, 32, "flat", _FLAT, dils=(1, 2, 3), **_GRP),   # grouped build
    _r("flat-1x1-res", 3, 9, 10, 96, 32, "flat", _FLAT, k=(1, 1), pad=(0, 0), residual=True),   # 1x1 with residual
    # ---- conv_f16x3.hip, small-problem form (split-K through a workspace; every row runs twice on one plan)
    _r("small-64x64-z6", 1, 9, 10, 128, 64, "small", _SMALL, switches=dict(SMALL_ENABLED=True), runs=2),   # 64x64 tiles, split-K 6
    _r("small-128x32-z3-epilogue", 1, 9, 10, 64, 32, "small", _SMALL, switches=dict(SMALL_ENABLED=True), runs=2, residual=True, post=True,
       act=ACT_LEAKY),                                                         # 128x32 tiles, split-K 3; epilogue in the finish kernel
    _r("small-wide", 2, 20, 30, 512, 512, "small", _SMALL, switches=dict(SMALL_ENABLED=True), runs=2, act=ACT_RELU),   # keeps the 128x128 tile
    # ---- conv_f16x3_big.hip / conv_f16_big1.hip: the deep trunk kernels (M = 32883: ragged last tile, frames cross tiles)
    _r("big-n256", 3, 97, 113, 64, 256, "big", _BIG, act=ACT_RELU),            # two-stage form, three products, one 256-wide N tile; 18 K steps
    _r("big1", 3, 97, 113, 64, 256, "big", _BIG1, products=1, act=ACT_RELU),   # four-stage plain-f16 form (even number of K steps)
    _r("big-np1-n128", 3, 97, 113, 96, 384, "big", _BIG, products=1),          # 27 K steps: the two-stage form with one product, 128-wide N tiles
    # ---- conv1x1_f16.hip (streaming) and conv1x1_ms_f16.hip (LDS-staged) over several raw slices
    _r("s1x1-two-slices", 3, 7, 9, (32, 32), 32, "stream1x1", _S1, **_ONE),    # M = 189
    _r("s1x1-ragged-slices", 2, 11, 13, (38, 64, 24), 64, "stream1x1", _S1, act=ACT_RELU, second_buffer=True, **_ONE),   # the last slice in a second buffer
    _r("ms1x1-n96", 2, 11, 13, (76, 96), 96, "gemm1x1", _M1, **_ONE),
    _r("ms1x1-k549", 1, 9, 10, (306, 128, 115), 180, "gemm1x1", _M1, act=ACT_LEAKY, **_ONE),
    # ---- the dilated group of an MSBlock: one launch (msblock_dil_f16.hip) or three accumulating halo launches
    _r("msdil-small-map", 3, 9, 33, 32, 32, "msdil", _DIL, dils=(4, 8, 12), **_GRP),   # the reach exceeds the map height
    _r("msdil-tiles", 2, 27, 70, 32, 32, "msdil", _DIL, dils=(4, 8, 12), **_GRP),      # several tiles
    _r("lattice-123", 2, 9, 61, 32, 64, "lattice", _HALO, dils=(1, 2, 3), launches=3, **_GRP),   # plain, dilation-2 and lattice mode, accumulated onto the destination
    _r("lattice-4812", 1, 13, 241, 64, 32, "lattice", _HALO, dils=(4, 8, 12), launches=3, **_GRP),
    # ---- conv3x3_c4_f16.hip: the first layer, taps folded into K
    _r("first-3-64", 3, 9, 33, 3, 64, "first", _FIRST, act=ACT_LEAKY),
    _r("first-1-40-post", 2, 10, 37, 1, 40, "first", _FIRST, post=True, act=ACT_RELU),
]
SPLIT_IDS = [c["id"] for c in SPLIT_SWEEP]
