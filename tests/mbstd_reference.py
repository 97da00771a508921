"""The references of the MinibatchStdDev tests (a helper, not a test file).

1. The formulas of include/bgan.h "minibatch standard deviation" in numpy, kernel by kernel, in the dtype they are handed (float64:
   the reference; float32: the yardstick of tests/helpers.py's rule).
2. The layer in differentiable torch operations, and the torch-autograd float64 step reference: tests/ln_reference.py's walker (and
   through it tests/objective_reference.py's step) with an ``mbstd`` branch.  The walker raises on a layer kind it does not know, so
   the branch is put in front of it for the duration of a reference call (``walker()``): the layer list is walked up to the layer,
   the layer is applied, and the walk goes on behind it.  Each application records the smallest s of its non-constant columns."""
import contextlib

import numpy as np
import torch

import ln_reference as LN

DT = torch.float64
# No non-constant column of the reference's x-hat pass may have an s this close to sqrt(epsilon) = 1e-4 (the layer's default): above
# it the column's variance exceeds 2e-12, at G = 2 a difference of 2.8e-6 between the members, some forty float32 quanta of
# activations of size 1 -- a column float32 may see as constant where float64 does not would sit below.  (1 / s^3 itself is bounded
# by epsilon^-1.5; with ~10^2 columns per group the smallest s of a pass is typically 1.0e-4 to 2e-4, see the seeds' minima.)
MIN_S = 1.0001e-4


# ---------------------------------------------------------------------------------------------------- 1. numpy, kernel by kernel
def np_stats(x, G, eps):
    """x [N, P, C] -> (mu [N/G, P, C], s [N/G, P, C], f [N/G]) in x's dtype: two-pass, centred."""
    N, P, C = x.shape
    xg = x.reshape(N // G, G, P, C)
    mu = xg.mean(1, dtype=x.dtype)
    var = ((xg - mu[:, None]) ** 2).mean(1, dtype=x.dtype)
    s = np.sqrt(var + x.dtype.type(eps))
    return mu, s, s.reshape(N // G, -1).mean(1, dtype=x.dtype)


def np_fwd(x, G, eps):
    """(y [N, P, C + 1], mu, rs = 1 / s, f)."""
    N, P, C = x.shape
    mu, s, f = np_stats(x, G, eps)
    y = np.empty((N, P, C + 1), x.dtype)
    y[..., :C] = x
    y[..., C] = np.repeat(f, G)[:, None]
    return y, mu, 1 / s, f


def np_bwd(u, x, G, eps):
    """(dx [N, P, C], q [N/G]) for the gradient u [N, P, C + 1] at y."""
    N, P, C = x.shape
    mu, s, _ = np_stats(x, G, eps)
    q = u[..., C].reshape(N // G, -1).sum(1, dtype=x.dtype)
    k = x.dtype.type(1.0 / (G * P * C))
    xc = x.reshape(N // G, G, P, C) - mu[:, None]
    return u[..., :C] + (q[:, None, None, None] * k * xc / s[:, None]).reshape(N, P, C), q


def np_gp(d, x, q, G, eps):
    """(vout [N, P, C + 1], src [N, P, C], fdot [N/G]) for the tangent d at x and the first-order q."""
    N, P, C = x.shape
    mu, s, _ = np_stats(x, G, eps)
    k = x.dtype.type(1.0 / (G * P * C))
    xc = x.reshape(N // G, G, P, C) - mu[:, None]
    dg = d.reshape(N // G, G, P, C)
    fdot = k * (xc / s[:, None] * dg).reshape(N // G, -1).sum(1, dtype=x.dtype)
    vout = np.empty((N, P, C + 1), x.dtype)
    vout[..., :C] = d
    vout[..., C] = np.repeat(fdot, G)[:, None]
    dbar = dg.mean(1, dtype=x.dtype)
    m = (xc * dg).mean(1, dtype=x.dtype)
    src = q[:, None, None, None] * k * ((dg - dbar[:, None]) / s[:, None] - xc * m[:, None] / s[:, None] ** 3)
    return vout, src.reshape(N, P, C), fdot


# ---------------------------------------------------------------------------------------------------- 2. torch
def torch_mbstd(x, G, eps, record=None):
    """The layer on x [N, H, W, C] (or [N, P, C]) in differentiable torch operations."""
    N, C = x.shape[0], x.shape[-1]
    xg = x.reshape(N // G, G, -1)
    mu = xg.mean(1, keepdim=True)
    var = ((xg - mu) ** 2).mean(1)
    s = torch.sqrt(var + eps)
    if record is not None:
        live = var.detach() > 0
        record.append(float(s.detach()[live].min()) if bool(live.any()) else float("inf"))
    f = s.mean(1)
    extra = f.repeat_interleave(G).view(N, *([1] * (x.dim() - 1))).expand(*x.shape[:-1], 1)
    return torch.cat([x, extra], -1)


class _Part:
    """A stretch of a model's layer list, as the walker reads one."""

    def __init__(self, flat):
        self._flat = flat

    def flat_layers(self):
        return self._flat


MIN_S_SEEN = []         # min s of the non-constant columns, one entry per application of the layer since the last walker() began
_plain_walk = LN.ref_forward


def ref_forward(model, W, x, training, masks=None, pre=None):
    flat = model.flat_layers()
    at = [i for i, (l, _) in enumerate(flat) if l.kind == "mbstd"]
    if not at:
        return _plain_walk(model, W, x, training, masks, pre)
    assert len(at) == 1 and not any(l.kind == "dropout" for l, _ in flat[at[0] + 1:])
    layer = flat[at[0]][0]
    x = _plain_walk(_Part(flat[:at[0]]), W, x, training, masks, pre)
    x = torch_mbstd(x, layer.group_size, layer.epsilon, MIN_S_SEEN)
    return _plain_walk(_Part(flat[at[0] + 1:]), W, x, training, None, pre)


@contextlib.contextmanager
def walker():
    """ln_reference.ref_forward with the ``mbstd`` branch, for every reference built on it (they call it through the module)."""
    del MIN_S_SEEN[:]
    LN.ref_forward = ref_forward
    try:
        yield MIN_S_SEEN
    finally:
        LN.ref_forward = _plain_walk


def ref_step(gen, disc, reals, rnd, gbs, objective=None, penalty_step=True):
    """tests/objective_reference.py's step reference (dict) for a critic with the layer, plus ``min_s``: the smallest s of a
    non-constant column of the x-hat pass (inf on a step without the penalty), and ``min_s_all``: the same over all passes.  The
    reference applies the critic to the fakes, the reals, x-hat (with the penalty) and the generator step's fakes, in this order."""
    import objective_reference as OR
    with walker() as seen:
        ref = OR.ref_step_grads(gen, disc, reals, rnd, gbs, objective, penalty_step=penalty_step)
        assert len(seen) == (4 if penalty_step else 3), seen
        ref["min_s"], ref["min_s_all"] = (seen[2] if penalty_step else float("inf")), min(seen)
    return ref


def check_guards(ref):
    """The assertions on the reference alone that precede every comparison."""
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM or ref["norm"] == float("inf"), ref["norm"]
    assert ref["min_s"] > MIN_S, ref["min_s"]
