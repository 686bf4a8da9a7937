"""Plain torch restatement of the self-consistency term (csrc/selfcorr.hip; the reference's loss.py:187-219 get_selfConsistency) and
the seeded cases its tests share.  Runs on the CPU in the dtype of its inputs; nothing here needs a GPU.

The restatement is the STABLE form: kl(t, lp) = t (log t - lp) with t = sigmoid(z) and log t = logsigmoid(z) = -softplus(-z), so
autograd forms d kl / d z = t (1 - t) (log t - lp + 1) without ever taking log of an underflowed t.  The reference computes
kl_div(lp, sigmoid(z)) whose target gradient evaluates 0 * log 0 = NaN wherever sigmoid underflows to exactly 0 (pupil ellipse,
q > about 2.6: every realistic frame); value and logit gradient agree everywhere, the ellipse gradient wherever the reference's is
finite (tests/test_host_selfcorr.py, fixture tests/golden/selfcorr.npz).

The mesh axes are float32 ``torch.linspace(-1, 1, n)`` values (create_meshgrid, utils.py:27-60), widened for a float64 run.
"""
import math

import torch
import torch.nn.functional as F

WEIGHT = 10.0        # loss += 10 * loss_selfCorr (models/RITnet_v2.py:341, RITnet_v1.py:287)
MISTAKES = ("swap_ellipses", "swap_xy", "sum_not_mean", "div_by_B", "no_factor")


def mesh_axes(H, W, dtype):
    return torch.linspace(-1, 1, W).to(dtype), torch.linspace(-1, 1, H).to(dtype)


def _q(el, x, y):
    """(X/a)^2 + (Y/b)^2 of get_mask (loss.py:211-216) for one ellipse ``el`` = (cx, cy, a, b, theta)."""
    c, s = torch.cos(el[4]), torch.sin(el[4])
    X = (x - el[0]) * c + (y - el[1]) * s
    Y = -(x - el[0]) * s + (y - el[1]) * c
    return (X / el[2]) ** 2 + (Y / el[3]) ** 2


def _kl(z, lp):
    return torch.sigmoid(z) * (F.logsigmoid(z) - lp)


def term(op, elPred, ok, mistake=None):
    """get_selfConsistency(op, elPred, ok): op [B,3,H,W] logits, elPred [B,10] = (iris, pupil) x (cx, cy, a, b, theta), ok [B] in
    {0, 1}.  ``mistake``: one of MISTAKES (tests only; "no_factor" acts in ``weighted``)."""
    B, _, H, W = op.shape
    lp = F.log_softmax(op, dim=1)
    gx, gy = mesh_axes(H, W, op.dtype)
    x, y = gx[None, :], gy[:, None]
    if mistake == "swap_xy":
        x, y = y, x
    iris, pupil = elPred[:, :5], elPred[:, 5:]
    if mistake == "swap_ellipses":
        iris, pupil = pupil, iris
    red = torch.sum if mistake == "sum_not_mean" else torch.mean
    total = (op.sum() + elPred.sum()) * 0
    for i in range(B):
        if ok[i] != 0:
            total = total + ok[i] * red(_kl(64 * (1 - _q(pupil[i], x, y)), lp[i, 2]))
            total = total + ok[i] * red(_kl(64 * (_q(iris[i], x, y) - 1), lp[i, 0]))
    n = ok.sum()
    if n == 0:
        return total
    return total / (B if mistake == "div_by_B" else n)


def weighted(op, elPred, ok, mistake=None):
    """What the models add to the loss: 10 * term."""
    return (1.0 if mistake == "no_factor" else WEIGHT) * term(op, elPred, ok, mistake)


def value_and_grads(op, elPred, ok, mistake=None, fn=term):
    """(value, d value / d op, d value / d elPred) by autograd, in the dtype of the inputs."""
    a, e = op.detach().clone().requires_grad_(True), elPred.detach().clone().requires_grad_(True)
    v = fn(a, e, ok, mistake)
    ga, ge = torch.autograd.grad(v, (a, e))
    return v.detach(), ga, ge


# ---- seeded cases -----------------------------------------------------------------------------------------------------------------
SHAPES = ((3, 6, 10), (2, 50, 70))
OKS = ("all", "some", "none")
SETS = ("typical", "covering", "outside", "thin", "negative")
# the small shape takes the whole product; the large one every ellipse set with "some", and the other patterns where they say
# something new (the fixture keeps one [B,3,H,W] gradient per case)
CASES = [((3, 6, 10), ok, es) for ok in OKS for es in SETS]
CASES += [((2, 50, 70), "some", es) for es in SETS]
CASES += [((2, 50, 70), "all", "typical"), ((2, 50, 70), "all", "covering"), ((2, 50, 70), "none", "typical")]


def case_key(shape, ok, es):
    return "%dx%dx%d_%s_%s" % (shape + (ok, es))


def ok_vector(B, pattern):
    ok = torch.ones(B)
    if pattern == "some":
        ok[B - 1] = 0
    elif pattern == "none":
        ok[:] = 0
    return ok


def ellipses(B, es, seed=0):
    """elPred [B,10] float32 of one ellipse set; the centres carry a small seeded jitter so that samples differ."""
    g = torch.Generator().manual_seed(1000 + seed)
    j = 0.02 * torch.randn(B, 10, generator=g)
    iris = torch.tensor([0.05, -0.04, 0.55, 0.45, 0.3])
    pupil = torch.tensor([0.10, 0.02, 0.25, 0.20, 0.2])
    if es == "covering":
        pupil = torch.tensor([0.02, -0.03, 1.30, 1.25, 0.2])
        j[:, 5:] = 0
    elif es == "outside":
        iris[:2], pupil[:2] = 3.0, 3.0
    elif es == "thin":
        iris = torch.tensor([0.05, -0.04, 0.9, 0.02, math.pi / 2 - 0.1])
        pupil = torch.tensor([0.10, 0.02, 0.9, 0.02, math.pi / 2 - 0.1])
        j[:, 2:5], j[:, 7:10] = 0, 0
    elif es == "negative":
        iris[4], pupil[4] = -0.7, -1.2
    else:
        assert es == "typical", es
    return (torch.cat((iris, pupil))[None, :] + j).float()


def case_inputs(shape, ok, es):
    """(op [B,3,H,W], elPred [B,10], ok [B]) float32; the logits are bf16-representable so that a bf16-storage kernel reads the
    same values."""
    B, H, W = shape
    g = torch.Generator().manual_seed(17 * B + H)
    op = (2 * torch.randn(B, 3, H, W, generator=g)).to(torch.bfloat16).float()
    return op, ellipses(B, es, seed=H), ok_vector(B, ok)
