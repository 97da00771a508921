"""The references of the PixelNormalization tests (a helper, not a test file).

1. The two formulas of include/bgan.h "pixel normalisation" in numpy, in the dtype they are handed (float64: the reference; float32:
   the yardstick of tests/helpers.py's rule).
2. The layer in differentiable torch operations, and the torch-autograd float64 step reference: tests/ln_reference.py's walker (and
   through it tests/objective_reference.py's step) with a ``pixelnorm`` branch.  The walker raises on a layer kind it does not know,
   so the branch is put in front of it for the duration of a reference call (``walker()``), the way tests/mbstd_reference.py does it:
   the layer list is walked up to each such layer, the layer is applied, and the walk goes on behind it.  Each application records
   the smallest mean(a^2) of its rows."""
import contextlib

import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models
import ln_reference as LN
import mbstd_reference as MR

DT = torch.float64
MIN_MS = 1e-4           # no row of the reference may have a mean(a^2) below: epsilon = 1e-8 is then negligible and r <= 100


# ---------------------------------------------------------------------------------------------------- 1. numpy, kernel by kernel
def np_fwd(x, eps, alpha):
    """x [R, C] -> (y [R, C], r [R]) in x's dtype."""
    dt = x.dtype.type
    a = np.where(x > 0, x, dt(alpha) * x)
    r = dt(1) / np.sqrt((a * a).mean(1, dtype=x.dtype) + dt(eps))
    return a * r[:, None], r


def np_bwd(g, y, r, alpha):
    """dz [R, C] for the gradient g at y: through the normalisation and the LeakyReLU in front of it."""
    dt = g.dtype.type
    m = (g * y).mean(1, dtype=g.dtype)
    return np.where(y > 0, dt(1), dt(alpha)) * (r[:, None] * (g - y * m[:, None]))


# ---------------------------------------------------------------------------------------------------- 2. torch
def torch_pixelnorm(x, eps, record=None):
    ms = (x * x).mean(-1, keepdim=True)
    if record is not None:
        record.append(float(ms.detach().min()))
    return x / torch.sqrt(ms + eps)


class _Part:
    """A stretch of a model's layer list, as the walker reads one."""

    def __init__(self, flat):
        self._flat = flat

    def flat_layers(self):
        return self._flat


MIN_MS_SEEN = []        # min mean(a^2) over the rows, one entry per application of the layer since the last walker() began
_inner = [LN.ref_forward]


def ref_forward(model, W, x, training, masks=None, pre=None):
    flat = model.flat_layers()
    at = [i for i, (l, _) in enumerate(flat) if l.kind == "pixelnorm"]
    if not at:
        return _inner[-1](model, W, x, training, masks, pre)
    assert not any(l.kind == "dropout" for l, _ in flat)
    B, lo = x.shape[0], 0
    for i in at:
        if i > lo:
            x = _inner[-1](_Part(flat[lo:i]), W, x, training, None, pre)
        x = torch_pixelnorm(x, flat[i][0].epsilon, MIN_MS_SEEN)
        lo = i + 1
    assert x.shape[0] == B
    return _inner[-1](_Part(flat[lo:]), W, x, training, None, pre) if lo < len(flat) else x


@contextlib.contextmanager
def walker():
    """ln_reference.ref_forward with the ``pixelnorm`` branch in front of whatever stands there (the plain walker, or
    mbstd_reference.walker()'s), for every reference built on it (they call it through the module)."""
    del MIN_MS_SEEN[:]
    _inner.append(LN.ref_forward)
    LN.ref_forward = ref_forward
    try:
        yield MIN_MS_SEEN
    finally:
        LN.ref_forward = _inner.pop()


def ref_step(gen, disc, reals, rnd, gbs, objective=None, penalty_step=True):
    """tests/objective_reference.py's step reference (dict) for a generator with the layer, plus ``min_ms``: the smallest mean(a^2)
    of any row of any application of the layer in the step, and ``min_s``: mbstd_reference.ref_step's, where the critic has a
    MinibatchStdDev (inf otherwise)."""
    import objective_reference as OR
    with MR.walker() as mb_seen, walker() as seen:
        ref = OR.ref_step_grads(gen, disc, reals, rnd, gbs, objective, penalty_step=penalty_step)
        assert seen, "the generator has no PixelNormalization"
        ref["min_ms"] = min(seen)
        ref["min_s"] = mb_seen[2] if mb_seen and penalty_step else float("inf")
    return ref


def check_guards(ref):
    """The assertions on the reference alone that precede every comparison."""
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM or ref["norm"] == float("inf"), ref["norm"]
    assert ref["min_ms"] > MIN_MS, ref["min_ms"]
    assert ref["min_s"] > MR.MIN_S, ref["min_s"]


def make_gan(arch, B, seed, gen_kw=None, disc_kw=None, objective=None, std=None, gbs=None, device=None, **kw):
    """objective_reference.make_gan with keywords for the generator (``normalization="pixel"`` unless said otherwise) and the
    critic."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch, **dict(dict(normalization="pixel"), **(gen_kw or {})))
    disc = models.DCGANDiscriminator(arch=arch, **(disc_kw or {}))
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    LN.randomize(gen, rng), LN.randomize(disc, rng)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, objective=objective, **kw)
    else:
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = bg.BlurredWGANGP(gen, disc, hp, cfg, objective=objective, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = LN.draw(gan.discriminator, B, gen.latent_size, rng)
    return gan, reals, rnd
