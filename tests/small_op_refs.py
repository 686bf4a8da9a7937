"""Plain torch references of the small operations (csrc/adain.hip, elementwise.hip, backward.hip, loss.hip, bdcn_tail.hip): the AdaIN
path, heads, resampling, normalisation and pooling, losses, the BDCN tail.

Every function computes in the dtype of its inputs: the tests call it once in float64 (the reference) and once in float32 (the
yardstick a kernel's error is measured against, see ``bound``).  A backward reference is autograd through the forward reference
(``vjp``); the transposes that have no forward here (resampling, reflection padding) are written as explicit index maps and pinned to
autograd of torch.nn.functional in tests/test_host_small_op_refs.py.  Nothing here needs a GPU.

Layouts: images are NHWC ``[B, H, W, C]`` like the plan's buffers unless a docstring says otherwise."""
import torch
import torch.nn.functional as F

from oracle import bdcn as obdcn
from oracle import deepvog as odeepvog
from oracle import losses as olosses

ULP32 = 2.0 ** -23


def vjp(fn, inputs, gouts):
    """Gradients of sum_k <gouts[k], fn(*inputs)[k]> w.r.t. every tensor of ``inputs`` (autograd, dtype of the inputs)."""
    xs = [x.detach().clone().requires_grad_(True) for x in inputs]
    outs = fn(*xs)
    if torch.is_tensor(outs):
        outs = (outs,)
    s = sum((g * o).sum() for g, o in zip(gouts, outs))
    return torch.autograd.grad(s, xs, allow_unused=True)


def rel_err(got, ref):
    """max |got - ref| relative to the absolute maximum of ``ref`` (one output tensor)."""
    ref = ref.double()
    scale = max(ref.abs().max().item(), 1e-30)
    return (got.double() - ref).abs().max().item() / scale


def bound(ref64, cpu32):
    """Bound of an fp32 kernel: four times the error of the same operation done in fp32 by torch on the CPU (a different summation
    order, the device's expf / tanhf), not below 4 fp32 ulps of the output scale.  Returns (bound, measured cpu error), both relative."""
    e = rel_err(cpu32, ref64)
    return max(4.0 * e, 4.0 * ULP32), e


# ---- AdaIN fusion path ------------------------------------------------------------------------------------------------------------
def softmax3(x):
    """nn.Softmax(dim=1) over the three logits of every pixel; x [..., 3]."""
    return torch.softmax(x, dim=-1)


def adain(x, gamma, beta, eps=1e-5):
    """oracle/esfnet.py:158-162 (calc_mean_std: unbiased variance + eps), x [B, HW, C], gamma / beta [B, C].  A constant channel has
    variance 0 and std sqrt(eps): its output is beta, as in the model."""
    flat = x.permute(0, 2, 1)                                      # [B, C, HW], the oracle's xb.flatten(2)
    std = (flat.var(dim=2) + eps).sqrt()[:, :, None]
    mean = flat.mean(dim=2)[:, :, None]
    return ((flat - mean) / std * gamma[:, :, None] + beta[:, :, None]).permute(0, 2, 1)


def conf_loss(pred, gt, flag):
    """oracle.losses.conf_loss (loss.py:139-157)."""
    return olosses.conf_loss(pred, gt, bool(flag))


def conf_terms(pred, gt, flag, weight, terms0):
    """What egne_conf_loss leaves in terms[0] and terms[7] (RITnet_v2.py:345-350: toggle -> loss += weight * conf, else loss = conf)."""
    c = conf_loss(pred, gt, flag)
    return (terms0 + weight * c if flag else c), c


def _reflect_index(n, P):
    i = torch.arange(-P, n + P).abs()
    return torch.where(i > n - 1, 2 * (n - 1) - i, i)


def reflect_pad_bwd(gpad, P):
    """Transpose of ReflectionPad2d(P): gpad [B, H+2P, W+2P, C] -> [B, H, W, C]; every padded position adds into the pixel it mirrors."""
    B, Hp, Wp, C = gpad.shape
    H, W = Hp - 2 * P, Wp - 2 * P
    t = torch.zeros(B, H, Wp, C, dtype=gpad.dtype).index_add_(1, _reflect_index(H, P), gpad)
    return torch.zeros(B, H, W, C, dtype=gpad.dtype).index_add_(2, _reflect_index(W, P), t)


def phase_pack(g):
    """Dense [B, Hp, Wp, Cp] -> the phase-packed layout of the stride-2 transposed conv: [B, Hp/2, Wp/2, 4 Cp], channel block
    (py & 1) * 2 + (px & 1)."""
    B, Hp, Wp, Cp = g.shape
    return g.reshape(B, Hp // 2, 2, Wp // 2, 2, Cp).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp // 2, Wp // 2, 4 * Cp)


# ---- regression head and latent ---------------------------------------------------------------------------------------------------
def selu(x):
    return F.selu(x)


def ellipse_head_act(x):
    """x [B, 10]: per 5-vector (tanh, tanh, sigmoid, sigmoid, identity) (RITnet_v2.py regression head)."""
    parts = []
    for o in (0, 5):
        parts += [torch.tanh(x[:, o:o + 2]), torch.sigmoid(x[:, o + 2:o + 4]), x[:, o + 4:o + 5]]
    return torch.cat(parts, 1)


def spatial_mean(x):
    """x [B, HW, C] -> [B, C]."""
    return x.mean(dim=1)


# ---- resampling and layout --------------------------------------------------------------------------------------------------------
def _bilinear_matrix(n, dtype):
    """[2n, n] matrix of F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) along one axis."""
    U = torch.zeros(2 * n, n, dtype=dtype)
    for o in range(2 * n):
        s = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = int(s)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        U[o, i0] += 1.0 - (s - i0)
        U[o, i1] += s - i0
    return U


def _nearest_matrix(n, dtype):
    U = torch.zeros(2 * n, n, dtype=dtype)
    U[torch.arange(2 * n), torch.arange(2 * n) // 2] = 1
    return U


def _avg_matrix(n, dtype):
    """[n // 2, n] matrix of avg_pool(2) along one axis (an odd last row / column is dropped)."""
    A = torch.zeros(n // 2, n, dtype=dtype)
    o = torch.arange(n // 2)
    A[o, 2 * o] = 0.5
    A[o, 2 * o + 1] = 0.5
    return A


def upsample2x_bwd(gy):
    """Transpose of the bilinear x2 up-sampling: gy [B, 2H, 2W, C] -> [B, H, W, C]."""
    H, W = gy.shape[1] // 2, gy.shape[2] // 2
    return torch.einsum("oh,bopc,pw->bhwc", _bilinear_matrix(H, gy.dtype), gy, _bilinear_matrix(W, gy.dtype))


def upsample2x_nearest(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample2x_nearest_bwd(gy):
    H, W = gy.shape[1] // 2, gy.shape[2] // 2
    return torch.einsum("oh,bopc,pw->bhwc", _nearest_matrix(H, gy.dtype), gy, _nearest_matrix(W, gy.dtype))


def avgpool2_bwd(gy, H, W):
    """Transpose of avg_pool2d(2) of an [B, H, W, C] map: gy [B, H//2, W//2, C] -> [B, H, W, C] (zeros in an odd last row / column)."""
    return torch.einsum("oh,bopc,pw->bhwc", _avg_matrix(H, gy.dtype), gy, _avg_matrix(W, gy.dtype))


def _pool_out(n, stride):
    """Output size of a 2-wide ceil-mode pooling window: the last window must start inside the input."""
    o = -((n - 2) // -stride) + 1
    return o - 1 if (o - 1) * stride >= n else o


def maxpool2(x, stride):
    """nn.MaxPool2d(2, stride, ceil_mode=True) of an NHWC tensor, window by window: a window that hangs over the border is clipped to
    the input (what lies outside does not take part, whatever the sign of the data)."""
    H, W = x.shape[1:3]
    y0, x0 = torch.arange(_pool_out(H, stride)) * stride, torch.arange(_pool_out(W, stride)) * stride
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    rows = torch.maximum(x[:, y0], x[:, y1])
    return torch.maximum(rows[:, :, x0], rows[:, :, x1])


def act(x, kind):
    """The library's activation codes: 0 none, 1 ReLU, 2 LeakyReLU(0.01)."""
    return torch.relu(x) if kind == 1 else (F.leaky_relu(x, 0.01) if kind == 2 else x)


def affine(x, a, b):
    """x [..., C] * a + b with a, b [C] (or anything that broadcasts)."""
    return x * a + b


def affine_act(x, a, b, relu=True, kind=None):
    """act(x * a + b); ``kind`` (an activation code) overrides ``relu``."""
    return act(x * a + b, (1 if relu else 0) if kind is None else kind)


# ---- normalisation, pooling, bilinear up-sampling ------------------------------------------------------------------------------------
def _moments(x, per_sample):
    """x [B, HW, C]: mean and biased variance over HW of each sample ([B, 1, C]) or over (B, HW) ([1, 1, C]), two passes."""
    dims = (1,) if per_sample else (0, 1)
    mean = x.mean(dim=dims, keepdim=True)
    return mean, ((x - mean) ** 2).mean(dim=dims, keepdim=True)


def norm_stats(x, per_sample, eps=1e-5):
    """x [B, HW, C] -> (scale = rstd, shift = -mean * rstd, mean, biased variance), each [B, C] (per_sample) or [1, C]: InstanceNorm /
    training-mode BatchNorm statistics.  One spatial element is legal (variance 0)."""
    mean, var = _moments(x, per_sample)
    rstd = 1.0 / torch.sqrt(var + eps)
    return tuple(t[:, 0] for t in (rstd, -mean * rstd, mean, var))


def stats_finish(partials, npix, eps=1e-5):
    """partials [B, nchunk, Cp, 2]: per chunk (sum x, sum x^2) -> (scale, shift, mean, biased variance), each [B, Cp], for samples of
    npix pixels (a variance that rounds below zero is zero)."""
    s = partials.sum(dim=1)
    mean = s[..., 0] / npix
    var = (s[..., 1] / npix - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return rstd, -mean * rstd, mean, var


def norm_fwd(x, gamma, beta, per_sample, act_in, eps=1e-5):
    """What egne_norm_bwd differentiates (csrc/backward.hip: xh = x * scale + shift, g = gy * act_in'(xh), then gamma): x [B, HW, C];
    per_sample = 1: act_in(InstanceNorm(x)) (gamma = beta = None); per_sample = 0: act_in(xh) * gamma + beta with the batch's
    statistics -- a training-mode BatchNorm2d for act_in = 0, the only activation the plans pair with gamma."""
    mean, var = _moments(x, per_sample)
    y = act((x - mean) / torch.sqrt(var + eps), act_in)
    return y if gamma is None else y * gamma + beta


def avgpool2(x):
    """nn.AvgPool2d(2) of an NHWC tensor (floor sizes: an odd last row / column is ignored), summed in row-major order."""
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    t, b = x[:, 0:2 * Ho:2], x[:, 1:2 * Ho:2]
    return (((t[:, :, 0:2 * Wo:2] + t[:, :, 1:2 * Wo:2]) + b[:, :, 0:2 * Wo:2]) + b[:, :, 1:2 * Wo:2]) * 0.25


def norm_act_pool2(x, scale, shift, kind):
    """avgpool2(act(x * scale[n][c] + shift[n][c])): x [B, H, W, C], scale / shift [B, C]."""
    return avgpool2(act(x * scale[:, None, None, :] + shift[:, None, None, :], kind))


def upsample2x(x):
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) of an NHWC tensor."""
    H, W = x.shape[1:3]
    return torch.einsum("oh,bhwc,pw->bopc", _bilinear_matrix(H, x.dtype), x, _bilinear_matrix(W, x.dtype))


def act_bwd_bias(g, y, kind):
    """g * act'(y) with the branch taken from the stored OUTPUT y (y > 0: 1, else the slope: 0 ReLU, 0.01 leaky, 1 none) and its
    per-channel sums over every leading axis."""
    slope = {0: 1.0, 1: 0.0, 2: 0.01}[kind]
    gz = torch.where(y > 0, g, g * slope)
    return gz, gz.reshape(-1, gz.shape[-1]).sum(dim=0)


# ---- losses -----------------------------------------------------------------------------------------------------------------------
def loss_head(op, elOut, target, pupil_center, elNorm, spatWts, distMap, cond, alpha):
    """oracle.losses.all_loss; op [B,3,H,W] NCHW, elNorm [B,2,5].  Returns (total, pred_c [B,2,2], terms)."""
    return olosses.all_loss(op, elOut, target, pupil_center, elNorm, spatWts, distMap, cond, alpha)


def loss_head_bwd(op, elOut, target, pupil_center, elNorm, spatWts, distMap, cond, alpha, gscale, g_op=None, g_pred_c=None,
                  g_elOut_up=None):
    """Gradient w.r.t. (op, elOut) of  gscale * total + <g_op, op> + <g_pred_c, pred_c> + <g_elOut_up, elOut>.  pred_c is the oracle's:
    without any mask in the batch its iris row is a copy of elOut[:, 5:7] (oracle.losses.all_loss), so g_pred_c's iris row then flows
    into elOut."""
    op = op.detach().clone().requires_grad_(True)
    elOut = elOut.detach().clone().requires_grad_(True)
    total, pred_c, _ = loss_head(op, elOut, target, pupil_center, elNorm, spatWts, distMap, cond, alpha)
    s = gscale * total + 0.0 * op.sum() + 0.0 * elOut.sum()
    if g_op is not None:
        s = s + (g_op * op).sum()
    if g_pred_c is not None:
        s = s + (g_pred_c * pred_c).sum()
    if g_elOut_up is not None:
        s = s + (g_elOut_up * elOut).sum()
    return torch.autograd.grad(s, (op, elOut))


def deepvog_loss(op, target, pupil_center, cond):
    """oracle.deepvog.deepvog_loss; op [B,2,H,W].  Returns (loss, pred_c [B,2], terms)."""
    return odeepvog.deepvog_loss(op, target, pupil_center, cond)


def deepvog_loss_bwd(op, target, pupil_center, cond, gscale):
    op = op.detach().clone().requires_grad_(True)
    loss = deepvog_loss(op, target, pupil_center, cond)[0]
    return torch.autograd.grad(gscale * loss + 0.0 * op.sum(), op)[0]


# ---- BDCN side-output path --------------------------------------------------------------------------------------------------------
def bdcn_stage_scores(ms, wd, bd, ws, bs, ws1, bs1):
    """bdcn_new.py:118-166 behind the MSBlocks of one stage: ms = list of [npix, 32] block outputs, wd [nblk, 21, 32], bd [nblk, 21];
    the 1x1 "down" convolutions summed, then the two 21 -> 1 score heads.  Returns (s, s1), [npix] each."""
    tot = None
    for k, m in enumerate(ms):
        dn = m @ wd[k].T + bd[k]
        tot = dn if tot is None else tot + dn
    return tot @ ws + bs, tot @ ws1 + bs1


def bdcn_stage_geometry(H, W):
    """Sizes of the five stages' score maps for an H x W frame (the ceil-mode poolings of vgg16_c.py: stride 2 three times, stride 1
    once) with the stride and crop of each stage's upsampler (bdcn_new.py:127-164)."""
    def pool(n, s):
        o = -((n - 2) // -s) + 1
        return o - 1 if (o - 1) * s >= n else o
    hs, ws = [H], [W]
    for s in (2, 2, 2, 1):
        hs.append(pool(hs[-1], s))
        ws.append(pool(ws[-1], s))
    strides = [1] + [obdcn.UPS[k][1] for k in "2345"]
    crops = [0] + [obdcn.UPS[k][2] for k in "2345"]
    return hs, ws, strides, crops


def bdcn_tail(s_a, s_b, ups, strides, crops, fuse_w, fuse_b, H, W, edge_thres=0):
    """The tail of bdcn_new.py:127-191 as a function of the ten score maps: s_a / s_b = five [B, 1, h_k, w_k] maps each, ups[k] the
    [1, 1, 2 stride, 2 stride] table of stage k (None for stage 1).  Transposed convolution, crop, the two cascades in the association
    of bdcn_new.py:167-176 (s_k + o_{k-1} + ... + o_1 / s_k1 + o_{k+1,1} + ... + o_51), fuse 1x1, sigmoid, and the edge_thres switch of
    utils.calc_edge on the fused map.  Returns the eleven maps and the fused value before the sigmoid."""
    a, b = [], []
    for k in range(5):
        x, y = s_a[k], s_b[k]
        if ups[k] is not None:
            o = crops[k]
            x = F.conv_transpose2d(x, ups[k], stride=strides[k])[:, :, o:o + H, o:o + W]
            y = F.conv_transpose2d(y, ups[k], stride=strides[k])[:, :, o:o + H, o:o + W]
        a.append(x)
        b.append(y)
    p_a, p_b = [], []
    for k in range(5):
        t = a[k]
        for j in range(k - 1, -1, -1):
            t = t + a[j]
        p_a.append(t)
        t = b[k]
        for j in range(k + 1, 5):
            t = t + b[j]
        p_b.append(t)
    maps = p_a + p_b
    fuse = F.conv2d(torch.cat(maps, 1), fuse_w.reshape(1, 10, 1, 1), fuse_b.reshape(1))
    e = torch.sigmoid(fuse)
    if edge_thres == 1:
        e = torch.where(e >= 0.1, torch.ones_like(e), e)
    return [torch.sigmoid(m) for m in maps] + [e], fuse


def bdcn_scores_of_oracle(sd, x, rate=4):
    """The ten score maps oracle.bdcn.bdcn_forward forms in front of its tail (trunk, MSBlocks, down convs, score heads), for the
    host test that feeds them to ``bdcn_tail``."""
    feats = obdcn.vgg_features(sd, x)
    fi, s_a, s_b = 0, [], []
    for st, blocks in obdcn.STAGES:
        tot = None
        for b in blocks:
            m = obdcn.msblock(sd, "msblock%s." % b, feats[fi], rate)
            fi += 1
            dn = F.conv2d(m, sd["conv%s_down.weight" % b], sd["conv%s_down.bias" % b])
            tot = dn if tot is None else tot + dn
        s_a.append(F.conv2d(tot, sd["score_dsn%s.weight" % st], sd["score_dsn%s.bias" % st]))
        s_b.append(F.conv2d(tot, sd["score_dsn%s_1.weight" % st], sd["score_dsn%s_1.bias" % st]))
    return s_a, s_b


def bdcn_tail_inputs(B, H, W, seed):
    """Seeded inputs of the tail (shared with the device test): ten score maps ~ 3 N(0,1) at the plan's stage sizes, the model's
    bilinear tables, a seeded fuse layer."""
    from egne_amd.bdcn_new import get_upsampling_weight
    g = torch.Generator().manual_seed(seed)
    hs, ws, strides, crops = bdcn_stage_geometry(H, W)
    s_a = [3 * torch.randn(B, 1, h, w, generator=g) for h, w in zip(hs, ws)]
    s_b = [3 * torch.randn(B, 1, h, w, generator=g) for h, w in zip(hs, ws)]
    ups = [None] + [get_upsampling_weight(1, 1, 2 * s) for s in strides[1:]]
    fw = 0.08 + 0.05 * torch.randn(10, generator=g)
    fb = 0.1 * torch.randn(1, generator=g)
    return s_a, s_b, ups, strides, crops, fw, fb
