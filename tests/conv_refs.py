"""Float64 reference, exactly representable data and the sweep table for the generic convolution kernel (egne_conv2d_fwd, csrc/conv_igemm.hip).

``conv_ref`` states in plain torch what ONE Plan.conv computes; ``int_case`` draws integer-valued data for which every product and every
partial sum is an integer that the storage type holds exactly, so that the summation order cannot matter and a kernel must reproduce the
reference BIT FOR BIT -- a tolerance says little about addressing (a wrong tap, a wrong frame's table, a dropped K tail), equality does.
``SWEEP`` is the list of cases that tests/test_host_conv_refs.py checks on the CPU and tests/test_gpu_conv_igemm_sweep.py runs on the GPU.
"""
import torch
import torch.nn.functional as F

D = torch.float64
BF = torch.bfloat16
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
FP32_EXACT = 2 ** 24          # integers below this magnitude are fp32 values
BF16_EXACT = 256              # ... bf16 values (8 significant bits)
WIDE_MAP = 1024               # output pixels per frame from which launch() takes bf16 tensors on bf16 MFMAs (weights rounded to bf16)


def pad8(c):
    return (int(c) + 7) // 8 * 8


def pad32(c):
    return (int(c) + 31) // 32 * 32


def act_ref(z, act):
    return F.relu(z) if act == ACT_RELU else (F.leaky_relu(z, 0.01) if act == ACT_LEAKY else z)


def conv_ref(xs, ws, bs, stride=1, pad=(0, 0), dils=(1,), act=ACT_NONE, pad_mode=0, norm=None, residual=None, post=None, dtype=D):
    """Float64 statement of one Plan.conv.  xs: NCHW slices in concat order; ws / bs: one OIHW weight / bias per group; ``pad`` is in
    units of the dilation (padding = pad * dil), zero (pad_mode 0) or reflect (1); norm: {slice: (scale[B, C], shift[B, C], act_in)}, the
    per-(frame, channel) affine + activation applied on load -- padding comes AFTER it; the groups' act(conv_g + bias_g) are summed;
    then ``* post_scale + post_shift + residual`` (post: (scale[Cout], shift[Cout])).  ``dtype``: the type it is evaluated in (float64)."""
    D = dtype
    xe = []
    for i, x in enumerate(xs):
        x = x.to(D)
        if norm and i in norm:
            sc, sh, act_in = norm[i]
            x = act_ref(x * sc.to(D)[:, :, None, None] + sh.to(D)[:, :, None, None], act_in)
        xe.append(x)
    xin = torch.cat(xe, 1)
    y = None
    for g, w in enumerate(ws):
        dil = dils[g]
        ph, pw = pad[0] * dil, pad[1] * dil
        b = bs[g].to(D) if bs is not None and bs[g] is not None else None
        if pad_mode == 1:
            z = F.conv2d(F.pad(xin, (pw, pw, ph, ph), mode="reflect"), w.to(D), b, stride=stride, dilation=dil)
        else:
            z = F.conv2d(xin, w.to(D), b, stride=stride, padding=(ph, pw), dilation=dil)
        z = act_ref(z, act)
        y = z if y is None else y + z
    if post is not None:
        y = y * post[0].to(D)[None, :, None, None] + post[1].to(D)[None, :, None, None]
    if residual is not None:
        y = y + residual.to(D)
    return y


# ---- the sweep table -------------------------------------------------------------------------------------------------------------

def _c(id, B, H, W, chans, Cout, k, dtype="fp32", stride=1, pad=(0, 0), dils=(1,), act=ACT_NONE, pad_mode=0, norm=(), residual=False,
       post=False, form=None, tile=None):
    """One row.  ``norm``: slices that carry an input affine + LeakyReLU (ReLU in the integer run); ``form`` / ``tile``: the instantiation
    (fp32, grouped, bf16, bfm, fold) and the <WM, WN> tile the row is meant to reach (launch_form states the library's rule)."""
    return dict(id=id, B=B, H=H, W=W, chans=tuple(chans), Cout=Cout, k=tuple(k), dtype=dtype, stride=stride, pad=tuple(pad),
                dils=tuple(dils), act=act, pad_mode=pad_mode, norm=tuple(norm), residual=residual, post=post, form=form, tile=tuple(tile))


SWEEP = [
    # ---- fp32, geometry (B = 3..5: every 128- / 256-row tile holds rows of two or more frames)
    _c("f32-1x1-s2", 3, 7, 9, (24,), 40, (1, 1), stride=2, act=2, form="fp32", tile=(1, 2)),                        # M = 60: less than one tile
    _c("f32-1x1-3slices-affine", 3, 11, 13, (5, 20, 38), 64, (1, 1), act=2, norm=(1,), form="fp32", tile=(1, 2)),   # Cp 8 / 24 / 40
    _c("f32-3x3-s2-9x12", 3, 9, 12, (16,), 32, (3, 3), stride=2, pad=(1, 1), act=1, form="fp32", tile=(2, 1)),      # Wo = floor(11 / 2) + 1
    _c("f32-3x3-s2-10x13", 3, 10, 13, (16,), 32, (3, 3), stride=2, pad=(1, 1), form="fp32", tile=(2, 1)),           # Ho = floor(9 / 2) + 1
    _c("f32-3x3-s3", 4, 8, 11, (16,), 32, (3, 3), stride=3, pad=(1, 1), act=2, form="fp32", tile=(2, 1)),
    _c("f32-3x3-pad01", 3, 9, 10, (16,), 32, (3, 3), pad=(0, 1), form="fp32", tile=(2, 1)),
    _c("f32-5x3-pad20", 3, 9, 10, (16,), 32, (5, 3), pad=(2, 0), act=1, form="fp32", tile=(2, 1)),
    _c("f32-1x7-pad03", 3, 6, 11, (16,), 32, (1, 7), pad=(0, 3), form="fp32", tile=(2, 1)),
    _c("f32-7x1-pad30", 3, 11, 6, (16,), 32, (7, 1), pad=(3, 0), act=2, form="fp32", tile=(2, 1)),
    _c("f32-5x5-dil2-reach-past-map", 5, 6, 7, (16,), 32, (5, 5), pad=(2, 2), dils=(2,), form="fp32", tile=(2, 1)),
    _c("f32-3x3-dil2-s2", 3, 11, 14, (16,), 32, (3, 3), stride=2, pad=(1, 1), dils=(2,), act=1, form="fp32", tile=(2, 1)),
    _c("f32-5x5-on-2x3", 5, 2, 3, (16,), 32, (5, 5), pad=(2, 2), form="fp32", tile=(2, 1)),                         # kernel larger than the map
    _c("f32-6x6-s2-36taps", 3, 13, 17, (16,), 32, (6, 6), stride=2, pad=(2, 2), act=2, form="fp32", tile=(2, 1)),   # bounds test per step
    _c("f32-6x6-s3-36taps", 3, 13, 17, (16,), 32, (6, 6), stride=3, pad=(1, 1), form="fp32", tile=(2, 1)),
    _c("f32-reflect-4x4-s2", 3, 9, 11, (16,), 32, (4, 4), stride=2, pad=(1, 1), act=1, pad_mode=1, form="fp32", tile=(2, 1)),
    _c("f32-reflect-3x3-dil2", 3, 7, 9, (16,), 32, (3, 3), pad=(1, 1), dils=(2,), pad_mode=1, form="fp32", tile=(2, 1)),
    _c("f32-reflect-7x7-pad-H-1", 4, 4, 5, (8,), 32, (7, 7), pad=(3, 3), act=1, pad_mode=1, form="fp32", tile=(2, 1)),
    # ---- fp32, tiles and K steps
    _c("f32-cout3", 3, 9, 10, (24,), 3, (3, 3), pad=(1, 1), form="fp32", tile=(2, 1)),
    _c("f32-cout96", 3, 9, 10, (16,), 96, (3, 3), pad=(1, 1), act=2, form="fp32", tile=(2, 1)),                     # three N tiles
    _c("f32-cout64", 3, 9, 10, (16,), 64, (3, 3), pad=(1, 1), form="fp32", tile=(2, 2)),
    _c("f32-cout100", 3, 9, 10, (16,), 100, (3, 3), pad=(1, 1), act=1, form="fp32", tile=(1, 1)),                   # CoutP 128 on a small map
    _c("f32-1x1-cout96", 3, 9, 10, (24,), 96, (1, 1), form="fp32", tile=(1, 1)),
    # <1, 4> needs ceil(M / 128) * CoutP / 128 >= 256: 2x2 over 8 channels (one K step per tap) on 128x128; with NO padding the map gives
    # 127x127 outputs and 253 tiles, so the row pads by 1 (129x129, 261 tiles, a ragged last tile)
    _c("f32-tile-1x4", 2, 128, 128, (8,), 128, (2, 2), pad=(1, 1), act=2, form="fp32", tile=(1, 4)),
    _c("f32-cin72", 3, 9, 10, (72,), 32, (3, 3), pad=(1, 1), form="fp32", tile=(2, 1)),                             # K steps of 32, 32, 8
    _c("f32-cin40", 3, 9, 10, (40,), 32, (3, 3), pad=(1, 1), act=2, form="fp32", tile=(2, 1)),                      # 32, 8
    _c("f32-8-slices", 3, 9, 10, (3, 8, 5, 1, 8, 7, 2, 6), 32, (3, 3), pad=(1, 1), form="fp32", tile=(2, 1)),       # EGNE_MAXSEG slices of Cp 8
    # ---- fp32, epilogue and the fused input affine
    _c("f32-residual-post-act-cout21", 3, 9, 10, (16,), 21, (3, 3), pad=(1, 1), act=2, residual=True, post=True, form="fp32", tile=(2, 1)),
    _c("f32-affine-padded-3x3", 4, 9, 10, (24,), 32, (3, 3), pad=(1, 1), act=1, norm=(0,), form="fp32", tile=(2, 1)),   # M = 360: tile 0 holds frames 0..2
    # ---- grouped (the fused MSBlock form): out = residual + sum_g relu(conv_g + bias_g)
    _c("grouped-dil123-cout32", 5, 5, 6, (24,), 32, (3, 3), pad=(1, 1), dils=(1, 2, 3), act=1, residual=True, form="grouped", tile=(2, 1)),
    _c("grouped-dil123-cout64", 5, 5, 6, (24,), 64, (3, 3), pad=(1, 1), dils=(1, 2, 3), act=1, residual=True, form="grouped", tile=(2, 2)),
    _c("grouped-dil4812-cout32", 3, 9, 10, (24,), 32, (3, 3), pad=(1, 1), dils=(4, 8, 12), act=1, residual=True, form="grouped", tile=(2, 1)),
    _c("grouped-dil4812-cout64", 3, 9, 10, (24,), 64, (3, 3), pad=(1, 1), dils=(4, 8, 12), act=1, residual=True, form="grouped", tile=(2, 2)),
    # ---- bf16 storage, exact fp32 products (fewer than 1024 output pixels per frame)
    _c("bf16-3x3-s2-10x13", 3, 10, 13, (16,), 32, (3, 3), "bf16", stride=2, pad=(1, 1), act=1, form="bf16", tile=(2, 1)),
    _c("bf16-3x3-pad01", 3, 9, 10, (16,), 32, (3, 3), "bf16", pad=(0, 1), form="bf16", tile=(2, 1)),
    _c("bf16-6x6-s2-36taps", 3, 13, 17, (16,), 32, (6, 6), "bf16", stride=2, pad=(2, 2), act=2, residual=True, form="bf16", tile=(2, 1)),
    _c("bf16-reflect-4x4-s2", 3, 9, 11, (16,), 32, (4, 4), "bf16", stride=2, pad=(1, 1), act=1, pad_mode=1, form="bf16", tile=(2, 1)),
    _c("bf16-reflect-3x3-dil2", 3, 7, 9, (16,), 32, (3, 3), "bf16", pad=(1, 1), dils=(2,), pad_mode=1, form="bf16", tile=(2, 1)),
    _c("bf16-reflect-7x7-pad-H-1", 4, 4, 5, (8,), 32, (7, 7), "bf16", pad=(3, 3), act=1, pad_mode=1, form="bf16", tile=(2, 1)),
    _c("bf16-1x1-3slices-affine", 3, 11, 13, (5, 20, 38), 64, (1, 1), "bf16", act=2, norm=(1,), form="bf16", tile=(1, 2)),
    # ---- bf16 MFMA (23x45 = 1035 output pixels per frame; B = 3 keeps the 1x1 under the 4096 pixels of the streaming bf16 1x1 kernel)
    _c("bfm-3x3-s2-slices-40-24", 3, 46, 90, (38, 24), 32, (3, 3), "bf16", stride=2, pad=(1, 1), act=1, form="bfm", tile=(2, 1)),   # K tails of 8 and 24
    _c("bfm-5x5-dil2", 3, 23, 45, (16,), 32, (5, 5), "bf16", pad=(2, 2), dils=(2,), form="bfm", tile=(2, 1)),
    _c("bfm-6x6-s2-36taps", 3, 46, 90, (16,), 32, (6, 6), "bf16", stride=2, pad=(2, 2), act=2, form="bfm", tile=(2, 1)),
    _c("bfm-reflect-4x4-s2", 3, 46, 90, (16,), 64, (4, 4), "bf16", stride=2, pad=(1, 1), act=1, pad_mode=1, form="bfm", tile=(2, 2)),
    _c("bfm-1x1-slices-8-24", 3, 23, 45, (5, 20), 64, (1, 1), "bf16", act=2, form="bfm", tile=(1, 2)),
    # ---- folded taps (one slice of Cp 8, at least 1024 output pixels per frame)
    _c("fold-2x2", 3, 24, 46, (8,), 24, (2, 2), "bf16", act=1, form="fold", tile=(2, 1)),                           # 4 taps: one step
    _c("fold-3x3-pad0", 3, 25, 47, (3,), 24, (3, 3), "bf16", form="fold", tile=(2, 1)),                             # 9 taps: 4 + 4 + 1
    _c("fold-5x5-zero-pad2", 3, 23, 45, (8,), 64, (5, 5), "bf16", pad=(2, 2), act=2, form="fold", tile=(2, 2)),     # 25 taps: the last step holds one
    _c("fold-7x7-zero-pad3", 3, 23, 45, (3,), 24, (7, 7), "bf16", pad=(3, 3), form="fold", tile=(2, 1)),            # 49 taps
    _c("fold-7x7-reflect-s2", 3, 46, 90, (3,), 24, (7, 7), "bf16", stride=2, pad=(3, 3), act=1, pad_mode=1, form="fold", tile=(2, 1)),
]
SWEEP_IDS = [c["id"] for c in SWEEP]


def out_hw(case):
    kh, kw = case["k"]
    d = case["dils"][0]
    return ((case["H"] + 2 * case["pad"][0] * d - d * (kh - 1) - 1) // case["stride"] + 1,
            (case["W"] + 2 * case["pad"][1] * d - d * (kw - 1) - 1) // case["stride"] + 1)


def launch_form(case):
    """(form, (WM, WN)): the instantiation and the tile egne_conv2d_fwd launches for the case with its default switches -- a statement of
    the rule at the end of csrc/conv_igemm.hip, so that the table says which of the 7 x 5 kernels a row is about."""
    Ho, Wo = out_hw(case)
    G, c, one = len(case["dils"]), pad32(case["Cout"]), case["k"] == (1, 1)
    mt = (case["B"] * Ho * Wo + 127) // 128
    if one and G == 1 and c % 128 != 0:
        tile = (1, 2) if c % 64 == 0 else (1, 1)
    elif G == 1 and c % 128 == 0 and mt * (c // 128) < 256:
        tile = (1, 2) if mt * (c // 64) >= 256 else (1, 1)
    elif c % 128 == 0:
        tile = (1, 4)
    else:
        tile = (2, 2) if c % 64 == 0 else (2, 1)
    if case["dtype"] == "bf16":
        cps = [pad8(ch) for ch in case["chans"]]
        fold = len(cps) == 1 and cps[0] == 8 and not case["norm"] and case["k"][0] * case["k"][1] >= 4
        form = "bf16" if Ho * Wo < WIDE_MAP else ("fold" if fold else "bfm")
    else:
        form = "grouped" if G > 1 else "fp32"
    return form, tile


def rounds_weights(case):
    """bf16 tensors on maps of >= 1024 output pixels: the products take bf16-rounded weights."""
    Ho, Wo = out_hw(case)
    return case["dtype"] == "bf16" and Ho * Wo >= WIDE_MAP


# ---- data ------------------------------------------------------------------------------------------------------------------------

def _ints(gen, shape, lo, hi, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if density < 1.0:
        v = torch.where(torch.rand(shape, generator=gen) < density, v, torch.zeros(()))
    return v


def _weights(gen, shape, density):
    """Thinned integer weights in which every (input channel, tap) pair keeps a non-zero weight in some output channel: a dropped tap
    or a dropped K tail changes the result."""
    w = _ints(gen, shape, -2, 2, density)
    co = torch.randint(0, shape[0], shape[1:], generator=gen)
    fill = torch.zeros(shape).scatter_(0, co[None], 1.0)
    return torch.where((w.abs().sum(dim=0, keepdim=True) == 0) & (fill > 0), fill, w)


def _pow2(gen, shape, signed=True):
    v = 2.0 ** torch.randint(0, 3, shape, generator=gen).float()          # 1, 2, 4
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    return v


def ref_of(case, data, weights=None):
    return conv_ref(data["xs"], weights if weights is not None else data["ws"], data["bs"], stride=case["stride"], pad=case["pad"],
                    dils=case["dils"], act=data["act"], pad_mode=case["pad_mode"], norm=data["norm"], residual=data["residual"], post=data["post"])


def abs_bound(case, data):
    """Largest magnitude any partial sum of the case can reach: sum |x'| |w| + |b| over the affined inputs, through the epilogue."""
    xs = []
    for i, x in enumerate(data["xs"]):
        x = x.to(D)
        if data["norm"] and i in data["norm"]:
            sc, sh, _ = data["norm"][i]
            x = x.abs() * sc.to(D).abs()[:, :, None, None] + sh.to(D).abs()[:, :, None, None]
        xs.append(x.abs())
    y = conv_ref(xs, [w.abs() for w in data["ws"]], [b.abs() for b in data["bs"]], stride=case["stride"], pad=case["pad"],
                 dils=case["dils"], pad_mode=case["pad_mode"],
                 residual=data["residual"].abs() if data["residual"] is not None else None,
                 post=(data["post"][0].abs(), data["post"][1].abs()) if data["post"] is not None else None)
    return y.max().item()


def int_conditions(case, data, want):
    """What makes the integer run exact -- asserted, not assumed: integer values everywhere, power-of-two scales, no LeakyReLU, every
    partial sum an fp32 integer, for bf16 storage every stored tensor within +-256 and (everywhere, as the bf16 MFMA rounds them) bf16
    weights; and at least half of the outputs non-zero, or a kernel that stores nothing would pass."""
    bf = case["dtype"] == "bf16"
    tensors = list(data["xs"]) + list(data["ws"]) + list(data["bs"])
    if data["residual"] is not None:
        tensors.append(data["residual"])
    tables = []
    for sc, sh, act_in in (data["norm"] or {}).values():
        assert act_in in (ACT_NONE, ACT_RELU)
        tables += [sc, sh]
        tensors.append(sh)
    if data["post"] is not None:
        tables += list(data["post"])
        tensors.append(data["post"][1])
    assert data["act"] in (ACT_NONE, ACT_RELU)
    for t in tensors:
        assert t.dtype == torch.float32 and torch.equal(t, t.round()), "integer values only"
    for sc in tables[0::2]:
        m, _ = torch.frexp(sc.abs())
        assert (m == 0.5).all(), "scales are powers of two"
    assert torch.equal(want, want.round())
    assert abs_bound(case, data) < FP32_EXACT, "a partial sum may leave the integers fp32 holds"
    if bf:
        stored = list(data["xs"]) + list(data["ws"]) + ([data["residual"]] if data["residual"] is not None else []) + [want]
        for t in stored:
            assert t.abs().max().item() <= BF16_EXACT, "a stored value leaves the integers bf16 holds"
            assert torch.equal(t.to(BF).to(t.dtype), t)
    nz = (want != 0).double().mean().item()
    assert nz >= 0.5, "only %.0f %% of the outputs are non-zero" % (100 * nz)


def int_case(gen, case):
    """Integer-valued data for ``case``: inputs in [-4, 4], weights in [-2, 2], bias in [1, 3] (plus, under a ReLU, half a standard deviation of the pre-activation, so that
    more than half of the outputs stay non-zero), residual in [-4, 4], affine tables with scales +-1, +-2, +-4 and shifts in [-3, 3], distinct per
    (frame, channel); activations are none or ReLU (LeakyReLU rows run with ReLU).  The density of non-zero WEIGHTS is halved until the
    reference fits the storage type (max |y| <= 256 for bf16, every partial sum < 2^24 for fp32); the inputs stay dense, so that a
    wrong address reads another value.  Returns the data and the float64 reference."""
    B, H, W = case["B"], case["H"], case["W"]
    kh, kw = case["k"]
    Cin, Cout, G = sum(case["chans"]), case["Cout"], len(case["dils"])
    Ho, Wo = out_hw(case)
    limit = BF16_EXACT if case["dtype"] == "bf16" else FP32_EXACT - 1
    density = 1.0
    while True:
        data = dict(xs=[_ints(gen, (B, c, H, W), -4, 4) for c in case["chans"]],
                    ws=[_weights(gen, (Cout, Cin, kh, kw), density) for _ in range(G)],
                    bs=[_ints(gen, (Cout,), 1, 3) for _ in range(G)],
                    act=ACT_RELU if case["act"] else ACT_NONE,
                    norm={i: (_pow2(gen, (B, case["chans"][i])), _ints(gen, (B, case["chans"][i]), -3, 3), ACT_RELU) for i in case["norm"]} or None,
                    residual=_ints(gen, (B, Cout, Ho, Wo), -4, 4) if case["residual"] else None,
                    post=(_pow2(gen, (Cout,)), _ints(gen, (Cout,), -3, 3)) if case["post"] else None)
        if data["act"] == ACT_RELU:
            # a ReLU zeroes half of a symmetric sum: lift the bias by half a standard deviation of the pre-activation (69 % stay positive)
            z = conv_ref(data["xs"], data["ws"], data["bs"], stride=case["stride"], pad=case["pad"], dils=case["dils"], pad_mode=case["pad_mode"],
                         norm=data["norm"])
            lift = float(round(0.5 * z.std().item() / G ** 0.5))
            data["bs"] = [b + lift for b in data["bs"]]
        want = ref_of(case, data)
        if want.abs().max().item() <= limit and abs_bound(case, data) < FP32_EXACT:
            break
        density *= 0.5
        assert density > 1e-3, case["id"]
    data["density"] = density
    int_conditions(case, data, want)
    return data, want


def normal_case(gen, case):
    """Seeded normal data: weights scaled by 1 / sqrt(K), affine scales 0.5 + |n|, shifts of order 1, LeakyReLU where the row has it.
    bf16 rows hold bf16-representable inputs and residuals (what a bf16 buffer stores)."""
    B, H, W = case["B"], case["H"], case["W"]
    kh, kw = case["k"]
    Cin, Cout, G = sum(case["chans"]), case["Cout"], len(case["dils"])
    Ho, Wo = out_hw(case)

    def rn(*shape):
        return torch.randn(*shape, generator=gen)

    def q(t):
        return t.to(BF).float() if case["dtype"] == "bf16" else t
    return dict(xs=[q(rn(B, c, H, W)) for c in case["chans"]],
                ws=[rn(Cout, Cin, kh, kw) / (Cin * kh * kw) ** 0.5 for _ in range(G)],
                bs=[rn(Cout) * 0.5 for _ in range(G)],
                act=case["act"],
                norm={i: (0.5 + rn(B, case["chans"][i]).abs(), rn(B, case["chans"][i]), ACT_LEAKY) for i in case["norm"]} or None,
                residual=q(rn(B, Cout, Ho, Wo)) if case["residual"] else None,
                post=(0.5 + torch.rand(Cout, generator=gen), rn(Cout)) if case["post"] else None)
