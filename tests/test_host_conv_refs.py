"""tests/conv_refs.py on the CPU: the float64 reference against independent statements with torch.nn.functional, so that a wrong
reference cannot vouch for the kernel in tests/test_gpu_conv_igemm_sweep.py, and the conditions that make the integer run of every
row of the sweep table exact."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=D)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-30)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, "max err %.3e vs scale %.3e" % (err, scale)


def test_slices_are_a_concatenation():
    """conv_ref over slices = F.conv2d over torch.cat; over slices of the WEIGHT = the sum of the per-slice convolutions."""
    g = _g(1)
    xs = [_rn(g, 2, c, 7, 9) for c in (5, 20, 38)]
    w, b = _rn(g, 11, 63, 3, 3), _rn(g, 11)
    got = R.conv_ref(xs, [w], [b], pad=(1, 1))
    _close(got, F.conv2d(torch.cat(xs, 1), w, b, padding=1))
    parts = F.conv2d(xs[0], w[:, :5], b, padding=1) + F.conv2d(xs[1], w[:, 5:25], None, padding=1) + F.conv2d(xs[2], w[:, 25:], None, padding=1)
    _close(got, parts)


def test_geometry_stride_dilation_and_asymmetric_padding():
    """padding = pad * dilation per axis; the output size is the library's (ConvLayer.out_hw)."""
    g = _g(2)
    x, w, b = _rn(g, 2, 4, 11, 14), _rn(g, 6, 4, 3, 5), _rn(g, 6)
    got = R.conv_ref([x], [w], [b], stride=2, pad=(1, 2), dils=(2,), act=R.ACT_LEAKY)
    _close(got, F.leaky_relu(F.conv2d(x, w, b, stride=2, padding=(2, 4), dilation=2), 0.01))
    case = dict(H=11, W=14, k=(3, 5), dils=(2,), pad=(1, 2), stride=2)
    assert tuple(got.shape[2:]) == R.out_hw(case)
    # against a direct sum at one output pixel: out[oy, ox] = b + sum w[ky, kx] x[oy s + (ky - pad_h) d, ox s + (kx - pad_w) d]
    oy, ox, co, n = 3, 2, 4, 1
    acc = b[co].clone()
    for ky in range(3):
        for kx in range(5):
            iy, ix = oy * 2 + (ky - 1) * 2, ox * 2 + (kx - 2) * 2
            if 0 <= iy < 11 and 0 <= ix < 14:
                acc += (w[co, :, ky, kx] * x[n, :, iy, ix]).sum()
    assert abs(F.leaky_relu(acc, 0.01).item() - got[n, co, oy, ox].item()) < 1e-12


def test_reflect_padding_mirrors_without_repeating_the_edge():
    g = _g(3)
    x, w, b = _rn(g, 2, 3, 4, 5), _rn(g, 5, 3, 7, 7), _rn(g, 5)
    got = R.conv_ref([x], [w], [b], pad=(3, 3), pad_mode=1, act=R.ACT_RELU)          # pad = H - 1
    idx_y = torch.tensor([3, 2, 1, 0, 1, 2, 3, 2, 1, 0])
    idx_x = torch.tensor([3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1])
    xp = x[:, :, idx_y][:, :, :, idx_x]
    _close(got, F.relu(F.conv2d(xp, w, b)))
    # with dilation the mirror reaches pad * dil
    w3 = _rn(g, 5, 3, 3, 3)
    got = R.conv_ref([x], [w3], [b], pad=(1, 1), dils=(2,), pad_mode=1)
    _close(got, F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), w3, b, dilation=2))


def test_grouped_sum_residual_and_post_affine():
    """out = (sum_g act(conv_g + b_g)) * post_scale + post_shift + residual."""
    g = _g(4)
    x = _rn(g, 2, 6, 9, 10)
    ws, bs = [_rn(g, 8, 6, 3, 3) for _ in range(3)], [_rn(g, 8) for _ in range(3)]
    res, ps, pt = _rn(g, 2, 8, 9, 10), _rn(g, 8), _rn(g, 8)
    got = R.conv_ref([x], ws, bs, pad=(1, 1), dils=(4, 8, 12), act=R.ACT_RELU, residual=res, post=(ps, pt))
    want = sum(F.relu(F.conv2d(x, w, b, padding=d, dilation=d)) for w, b, d in zip(ws, bs, (4, 8, 12)))
    _close(got, want * ps[None, :, None, None] + pt[None, :, None, None] + res)
    # dilation 12 on a 9x10 map: only the centre tap is inside
    want0 = sum(F.relu(F.conv2d(x, w, b, padding=d, dilation=d)) for w, b, d in zip(ws[:2], bs[:2], (4, 8))) + F.relu(F.conv2d(x, ws[2][:, :, 1:2, 1:2], bs[2]))
    _close(got, want0 * ps[None, :, None, None] + pt[None, :, None, None] + res)


def test_input_affine_comes_before_the_padding():
    """A padded pixel contributes 0, not act(shift)."""
    g = _g(5)
    x0, x1 = _rn(g, 3, 4, 6, 7), _rn(g, 3, 5, 6, 7)
    sc, sh = 0.5 + _rn(g, 3, 5).abs(), 1.0 + _rn(g, 3, 5)
    w, b = _rn(g, 7, 9, 3, 3), _rn(g, 7)
    got = R.conv_ref([x0, x1], [w], [b], pad=(1, 1), norm={1: (sc, sh, R.ACT_LEAKY)})
    x1n = F.leaky_relu(x1 * sc[:, :, None, None] + sh[:, :, None, None], 0.01)
    _close(got, F.conv2d(torch.cat([x0, x1n], 1), w, b, padding=1))
    # per frame: frame n uses row n of the tables
    one = R.conv_ref([x0[2:], x1[2:]], [w], [b], pad=(1, 1), norm={1: (sc[2:], sh[2:], R.ACT_LEAKY)})
    _close(got[2:], one)
    wrong = F.conv2d(F.pad(torch.cat([x0, x1], 1), (1, 1, 1, 1)), w, b)
    assert (got - wrong).abs().max().item() > 1e-3


def test_the_table_covers_what_it_is_meant_to():
    ids = R.SWEEP_IDS
    assert len(set(ids)) == len(ids)
    forms = {R.launch_form(c) for c in R.SWEEP}
    for tile in ((1, 1), (1, 2), (1, 4), (2, 1), (2, 2)):
        assert ("fp32", tile) in forms, tile
    for form in ("grouped", "bf16", "bfm", "fold"):
        assert any(f == form for f, _ in forms), form
    for c in R.SWEEP:
        if c["id"] != "f32-tile-1x4":
            assert 3 <= c["B"] <= 5 and R.out_hw(c)[0] * R.out_hw(c)[1] <= 1100, c["id"]
        if c["pad_mode"] == 1:
            assert all(c["pad"][0] * d < c["H"] and c["pad"][1] * d < c["W"] for d in c["dils"]), c["id"]
    taps = {c["k"][0] * c["k"][1] for c in R.SWEEP if c["form"] == "fold"}
    assert 4 in taps and any(t % 4 for t in taps) and any(t > 32 for t in taps)


@pytest.mark.parametrize("case", R.SWEEP, ids=R.SWEEP_IDS)
def test_row_reaches_its_launch_form(case):
    """The instantiation and tile the row names are the ones the library's rule gives for its sizes."""
    assert R.launch_form(case) == (case["form"], case["tile"]), R.launch_form(case)
    Ho, Wo = R.out_hw(case)
    assert Ho > 0 and Wo > 0
    if case["form"] in ("bfm", "fold"):
        assert R.rounds_weights(case) and Ho * Wo >= R.WIDE_MAP
    if case["form"] == "bf16":
        assert not R.rounds_weights(case)
    if case["form"] == "fold":
        assert len(case["chans"]) == 1 and case["chans"][0] <= 8


@pytest.mark.parametrize("case", R.SWEEP, ids=R.SWEEP_IDS)
def test_integer_data_is_exact_for_the_row(case):
    """int_case: integers, power-of-two scales, every partial sum below 2^24, bf16 rows within +-256 including the stored output, at
    least half of the outputs non-zero (int_conditions asserts each) -- and the float64 reference survives the storage type unchanged,
    evaluated in another summation order too."""
    data, want = R.int_case(_g(1234), case)
    R.int_conditions(case, data, want)
    store = R.BF if case["dtype"] == "bf16" else torch.float32
    assert torch.equal(want.to(store).to(D), want)
    # fp32 arithmetic in torch's own order gives the same integers
    got32 = R.conv_ref(data["xs"], data["ws"], data["bs"], stride=case["stride"], pad=case["pad"], dils=case["dils"], act=data["act"],
                       pad_mode=case["pad_mode"], norm=data["norm"], residual=data["residual"], post=data["post"], dtype=torch.float32)
    assert got32.dtype == torch.float32 and torch.equal(got32.to(D), want)
    # every tap and every input channel carries weight somewhere: a dropped tap or K tail changes the result
    for w in data["ws"]:
        assert (w.abs().sum(dim=0) > 0).all(), "a (channel, tap) pair without any weight"
    if case["norm"]:
        for sc, sh, _ in data["norm"].values():
            assert sc.shape[0] == case["B"] and (sc[0] != sc[1]).any() and (sh[0] != sh[1]).any()


def test_normal_data_of_bf16_rows_is_bf16_representable():
    case = next(c for c in R.SWEEP if c["id"] == "bf16-6x6-s2-36taps")
    data = R.normal_case(_g(5), case)
    for t in data["xs"] + [data["residual"]]:
        assert torch.equal(t.to(R.BF).float(), t)
    assert not torch.equal(data["ws"][0].to(R.BF).float(), data["ws"][0])
