"""The references of the FIR-filtered resampling tests (a helper, not a test file).

1. The operators of include/bgan.h "resampling" (UP_t / DOWN_t, per axis, and their separable 2-D products over an NHWC map) as
   dense matrices: numpy in any dtype (float64: the reference; float32 on exact data: the bit-for-bit yardstick, every product and
   partial sum being exact in any order), and StyleGAN2's upfirdn (zero-insert, pad, convolve, decimate) restated in 1-D, which the
   CPU tests hold the matrices against.
2. The two layers in differentiable torch float64, and the torch-autograd step reference: tests/ln_reference.py's walker (and through
   it tests/objective_reference.py's step) with ``firup`` / ``firdown`` branches.  The walker raises on a layer kind it does not
   know, so the branches are put in front of it for the duration of a reference call (``walker()``), the way
   tests/pixelnorm_reference.py does it: the layer list is walked up to each such layer, the layer is applied, and the walk goes on
   behind it, each stretch with the Dropout masks that are its own.  The same front end multiplies the kernels of
   layers.EqualizedLearningRate layers by their coefficient (a differentiable operation on the leaf, so autograd returns the
   gradient at the stored weight)."""
import contextlib

import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
import ln_reference as LN
import mbstd_reference as MR

DT = torch.float64


# ---------------------------------------------------------------------------------------------------- 1. the operators
def flip(taps):
    return tuple(taps)[::-1]


def normalized(kernel):
    """float32(k / sum(k)), normalised in double: what the layers hand the kernels."""
    k = np.asarray(kernel, np.float64)
    return tuple(float(v) for v in (k / k.sum()).astype(np.float32))


def up_matrix(taps, n, dtype=np.float64):
    """U [2n, n]: U[o, i] = t[o - 2i + T - 1] where that is a tap."""
    T = len(taps) // 2
    U = np.zeros((2 * n, n), dtype)
    for o in range(2 * n):
        for i in range(n):
            j = o - 2 * i + T - 1
            if 0 <= j < 2 * T:
                U[o, i] = taps[j]
    return U


def down_matrix(taps, n, dtype=np.float64):
    """D [n, 2n]: D[m, o] = t[T + 2m - o] where that is a tap."""
    T = len(taps) // 2
    D = np.zeros((n, 2 * n), dtype)
    for m in range(n):
        for o in range(2 * n):
            j = T + 2 * m - o
            if 0 <= j < 2 * T:
                D[m, o] = taps[j]
    return D


def _separable(Mh, Mw, x, scale):
    """scale * (Mh over H, Mw over W) of x [B, H, W, C], as two batched matrix products."""
    B, H, W, C = x.shape
    y = np.matmul(Mh, x.reshape(B, H, W * C)).reshape(B, Mh.shape[0], W, C)
    y = np.matmul(Mw, y)
    assert y.dtype == x.dtype
    return scale * y


def np_up(x, taps, scale=1.0, dtype=np.float64):
    """scale * UP_taps over H and W of x [B, H, W, C] in ``dtype``."""
    x = np.asarray(x, dtype)
    return _separable(up_matrix(taps, x.shape[1], dtype), up_matrix(taps, x.shape[2], dtype), x, dtype(scale))


def np_down(x, taps, scale=1.0, dtype=np.float64):
    """scale * DOWN_taps over H and W of x [B, 2H, 2W, C] in ``dtype``."""
    x = np.asarray(x, dtype)
    return _separable(down_matrix(taps, x.shape[1] // 2, dtype), down_matrix(taps, x.shape[2] // 2, dtype), x, dtype(scale))


def abs_weight_sums(taps, n_h, n_w, up):
    """[P, Q]: per output pixel the sum of |w| over the 2-D weights of its terms, what the rounding bound of that output scales with."""
    M = up_matrix if up else down_matrix
    return np.outer(np.abs(M(taps, n_h)).sum(1), np.abs(M(taps, n_w)).sum(1))


def upfirdn_1d(x, k, up, down, pad0, pad1):
    """StyleGAN2's upfirdn on a vector, float64: zero-insert, pad, correlate with the flipped kernel, decimate."""
    x, k = np.asarray(x, np.float64), np.asarray(k, np.float64)
    z = np.zeros(len(x) * up)
    z[::up] = x
    z = np.concatenate([np.zeros(pad0), z, np.zeros(pad1)])
    full = np.array([np.dot(z[o:o + len(k)], k[::-1]) for o in range(len(z) - len(k) + 1)])
    return full[::down]


def stylegan2_up_1d(x, k):
    """upsample_2d's padding rule in 1-D (factor 2; the gain is left to the caller)."""
    p = len(k) - 2
    return upfirdn_1d(x, k, 2, 1, (p + 1) // 2 + 1, p // 2)


def stylegan2_down_1d(x, k):
    """downsample_2d's padding rule in 1-D (factor 2)."""
    p = len(k) - 2
    return upfirdn_1d(x, k, 1, 2, (p + 1) // 2, p // 2)


# ---------------------------------------------------------------------------------------------------- 2. torch
def _apply(x, Mh, Mw, scale):
    return scale * torch.einsum("ph,qw,bhwc->bpqc", torch.as_tensor(Mh, dtype=DT), torch.as_tensor(Mw, dtype=DT), x)


def torch_firup(x, taps):
    """layers.FilteredUpSampling2D on x [B, H, W, C]: UP_f at gain 4."""
    return _apply(x, up_matrix(taps, x.shape[1]), up_matrix(taps, x.shape[2]), 4.0)


def torch_firdown(x, taps):
    """layers.FilteredDownSampling2D on x [B, 2H, 2W, C]: DOWN_f."""
    return _apply(x, down_matrix(taps, x.shape[1] // 2), down_matrix(taps, x.shape[2] // 2), 1.0)


class _Part:
    """A stretch of a model's layer list, as the walker reads one."""

    def __init__(self, flat):
        self._flat = flat

    def flat_layers(self):
        return self._flat


_inner = [LN.ref_forward]
FIR = ("firup", "firdown")


def _effective(flat, W):
    E = dict(W)
    for l, _ in flat:
        if isinstance(l, layers.EqualizedLearningRate):
            E[(id(l), "kernel")] = float(np.float32(l.coefficient)) * W[(id(l), "kernel")]
    return E


def ref_forward(model, W, x, training, masks=None, pre=None):
    flat = model.flat_layers()
    W = _effective(flat, W)
    at = [i for i, (l, _) in enumerate(flat) if l.kind in FIR]
    B, lo, used = x.shape[0], 0, 0
    for i in at + [len(flat)]:
        if i > lo:
            part = flat[lo:i]
            x = _inner[-1](_Part(part), W, x, training, None if masks is None else masks[used:], pre)
            used += sum(1 for l, _ in part if l.kind == "dropout")
        if i < len(flat):
            l = flat[i][0]
            x = torch_firup(x, l.taps) if l.kind == "firup" else torch_firdown(x, l.taps)
        lo = i + 1
    assert x.shape[0] == B
    return x


@contextlib.contextmanager
def walker():
    """ln_reference.ref_forward with the ``firup`` / ``firdown`` branches (and the equalised-learning-rate coefficients) in front of
    whatever stands there (the plain walker, or mbstd_reference.walker()'s), for every reference built on it."""
    _inner.append(LN.ref_forward)
    LN.ref_forward = ref_forward
    try:
        yield
    finally:
        LN.ref_forward = _inner.pop()


def ref_step(gen, disc, reals, rnd, gbs, objective=None, penalty_step=True):
    """tests/objective_reference.py's step reference (dict) for stacks with filtered stages, plus ``min_s``:
    mbstd_reference.ref_step's, where the critic has a MinibatchStdDev (inf otherwise)."""
    import objective_reference as OR
    with MR.walker() as mb_seen, walker():
        ref = OR.ref_step_grads(gen, disc, reals, rnd, gbs, objective, penalty_step=penalty_step)
        ref["min_s"] = mb_seen[2] if mb_seen and penalty_step else float("inf")
    return ref


def check_guards(ref):
    """The assertions on the reference alone that precede every comparison: the kink guard, the norm guard, and the
    MinibatchStdDev guard where the layer is present (LayerNormalization adds none of its own: tests/ln_reference.py's are these)."""
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM or ref["norm"] == float("inf"), ref["norm"]
    assert ref["min_s"] > MR.MIN_S, ref["min_s"]


def make_gan(arch, B, seed, up="filtered", down="filtered", resample_kernel=(1, 3, 3, 1), gen_kw=None, disc_kw=None, objective=None, std=None,
             gbs=None, score_scale=None, score_bias=None, device=None, **kw):
    """A WGANGP (BlurredWGANGP with ``std``) of models' stacks with the filtered variants, randomised as tests/ln_reference.py does;
    ``score_scale`` / ``score_bias``: objective_reference.scale_scores's (a hinge case needs scores on both sides of the hinges)."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch, upsampling=up, resample_kernel=resample_kernel, **(gen_kw or {}))
    disc = models.DCGANDiscriminator(arch=arch, downsampling=down, resample_kernel=resample_kernel, **(disc_kw or {}))
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    LN.randomize(gen, rng), LN.randomize(disc, rng)
    if score_scale is not None:
        import objective_reference as OR
        OR.scale_scores(disc, score_scale, score_bias)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, objective=objective, **kw)
    else:
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = bg.BlurredWGANGP(gen, disc, hp, cfg, objective=objective, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = LN.draw(gan.discriminator, B, gen.latent_size, rng)
    return gan, reals, rnd
