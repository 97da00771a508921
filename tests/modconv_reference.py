"""The references of the StyleModulation tests (a helper, not a test file).

1. The formulas of include/bgan.h "style modulation" in numpy, in the dtype they are handed (float64: the reference; float32 with
   one rounding per operation: what bg_mod_scale_f32 computes bit for bit).
2. The modulated convolution in differentiable torch operations, in the un-fused form the engine runs (scale the activations,
   convolve, scale the output), the fused form of the StyleGAN2 paper (per-sample weights W'[n] = d[n] * (s[n] * W)) by brute force,
   and the backward formulas of DESIGN.md section 5 "Style modulation" written out (``manual_backward``).
3. The torch-autograd float64 step reference: tests/ln_reference.py's walker with a modulation branch put in front of it
   (``walker(maps)``), under tests/objective_reference.py's step.  The branch sees the whole generator: the style source is the
   network's input vector behind the PixelNormalization that may stand first.  It applies the NoiseInjection layers itself
   (tests/noise_reference.py's walker counts one call per forward and cannot stand behind a walker that cuts the list)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
import firsample_reference as FS
import ln_reference as LN
import mbstd_reference as MR
import pixelnorm_reference as PR
from oracle import torch_ref as TR

DT = torch.float64
MIN_Q = 1e-4            # no demodulation sum q = (s * s) . Q of the reference may be smaller: epsilon = 1e-8 is then negligible, d <= 100
MIN_STYLE_GRAD = 1e-6   # no style gradient tensor of the reference may have a smaller max |value|: a dead path cannot pass


# ---------------------------------------------------------------------------------------------------- 1. numpy, kernel by kernel
def np_scale(x, v, bias=None, alpha=1.0):
    """x [B, P, C], v [B, C] -> act(x * v (+ bias)) in x's dtype, every operation rounded once."""
    dt = x.dtype.type
    o = (x * v[:, None, :]).astype(x.dtype)
    if bias is not None:
        o = (o + bias.astype(x.dtype)).astype(x.dtype)
    return np.where(o > 0, o, dt(alpha) * o).astype(x.dtype)


def np_dot(a, b, old=None, beta=0.0, scale=1.0):
    """float64: beta * old + scale * sum_p a * b, and sum_p |a * b| (what the rounding bound scales with)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = scale * (a * b).sum(1)
    if beta != 0.0:
        s = s + beta * np.asarray(old, np.float64)
    return s, np.abs(a * b).sum(1)


def np_wsq(w, transposed):
    """w [k, k, I, O] (``transposed``: [k, k, O, I]) -> Q [I, O] in float64."""
    q = (np.asarray(w, np.float64) ** 2).sum((0, 1))
    return q.T if transposed else q


def np_demod(s, Q, eps):
    s, Q = np.asarray(s, np.float64), np.asarray(Q, np.float64)
    return 1.0 / np.sqrt((s * s) @ Q + eps)


def np_demod_bwd(d, dd, s, Q, ds):
    """(dq, ds + the demodulation term, sum_o |dq * Q| per (n, i)) in float64."""
    d, dd, s, Q = (np.asarray(t, np.float64) for t in (d, dd, s, Q))
    dq = -0.5 * d ** 3 * dd
    return dq, np.asarray(ds, np.float64) + 2.0 * s * (dq @ Q.T), np.abs(dq) @ np.abs(Q).T


def np_wsq_grad(w, dQ, dw, transposed, scale):
    g = np.asarray(dQ, np.float64)
    g = g.T if transposed else g
    return np.asarray(dw, np.float64) + scale * 2.0 * np.asarray(w, np.float64) * g[None, None]


# ---------------------------------------------------------------------------------------------------- 2. torch, one layer
def _conv(kind, x, Wk, stride, k):
    if kind == "conv" and stride == 1:
        return LN._nhwc(F.conv2d(LN._nchw(x).contiguous(), Wk.permute(3, 2, 0, 1).contiguous(), padding=k // 2))
    if kind == "conv":
        return TR.conv2d(x, Wk, stride)
    return TR.conv2d_transpose(x, Wk, stride)


def wsq(kind, Wk):
    q = (Wk * Wk).sum((0, 1))
    return q.t() if kind == "convT" else q


def torch_modconv(kind, x, w, Wk, A, a, bias, stride, demodulate=True, eps=1e-8, q_seen=None):
    """The un-fused modulated convolution on x [B, H, W, I] with styles from w [B, L]; Wk is the EFFECTIVE kernel."""
    s = w @ A + a
    z = _conv(kind, x * s[:, None, None, :], Wk, stride, Wk.shape[0])
    if demodulate:
        q = (s * s) @ wsq(kind, Wk)
        if q_seen is not None:
            q_seen.append(float(q.detach().min()))
        z = z * (1.0 / torch.sqrt(q + eps))[:, None, None, :]
    return z if bias is None else z + bias


def fused_modconv(kind, x, w, Wk, A, a, bias, stride, demodulate=True, eps=1e-8):
    """StyleGAN2's definition by brute force: sample n is convolved with its own weights W'[n] = d[n] * (s[n] * W)."""
    s = w @ A + a
    out = []
    for n in range(x.shape[0]):
        Wn = Wk * (s[n][None, None, None, :] if kind == "convT" else s[n][None, None, :, None])     # the input-channel axis
        if demodulate:
            d = 1.0 / torch.sqrt((Wn * Wn).sum((0, 1, 3) if kind == "convT" else (0, 1, 2)) + eps)    # over taps and input channels: [O]
            Wn = Wn * (d[None, None, :, None] if kind == "convT" else d[None, None, None, :])
        out.append(_conv(kind, x[n:n + 1], Wn, stride, Wk.shape[0]))
    z = torch.cat(out)
    return z if bias is None else z + bias


def manual_backward(kind, x, w, Wk, A, a, bias, stride, dy, eps=1e-8):
    """The backward of a demodulating stage as the engine runs it, the two conv gradients taken by autograd
    on the plain convolution alone: (dW_eff, dbias, dA, da, dx)."""
    with torch.no_grad():
        s = w @ A + a
        Q = wsq(kind, Wk)
        d = 1.0 / torch.sqrt((s * s) @ Q + eps)
    xs = (x * s[:, None, None, :]).detach().requires_grad_(True)
    Wl = Wk.detach().requires_grad_(True)
    z = _conv(kind, xs, Wl, stride, Wk.shape[0])
    with torch.no_grad():
        dd = (dy * z).sum((1, 2))
        dz = d[:, None, None, :] * dy
    dW, dxs = torch.autograd.grad(z, (Wl, xs), dz)
    with torch.no_grad():
        ds = (x * dxs).sum((1, 2))
        dx = s[:, None, None, :] * dxs
        dq = -0.5 * d ** 3 * dd
        ds = ds + 2.0 * s * (dq @ Q.t())
        dQ = (s * s).t() @ dq
        dW = dW + 2.0 * Wk * (dQ.t() if kind == "convT" else dQ)[None, None]
        return dW, dy.sum((0, 1, 2)), w.t() @ ds, ds.sum(0), dx


# ---------------------------------------------------------------------------------------------------- 3. the walker
class _Part:
    """A stretch of a model's layer list, as the walker reads one."""

    def __init__(self, flat):
        self._flat = flat

    def flat_layers(self):
        return self._flat


_inner = [LN.ref_forward]
_maps = []              # the [B, P] noise arrays of the generator forwards still to come, in the step's order
MIN_Q_SEEN = []         # min q of every demodulation since the last walker() began


def is_mod(l):
    return isinstance(l, layers.StyleModulation)


def noise_pixels(model):
    return sum(int(np.prod(s[:-1])) for l, s in model.flat_layers() if l.kind == "noise")


def effective_kernel(l, W):
    """The kernel leaf of modulated layer ``l`` times the coefficient of the EqualizedLearningRate it may wrap."""
    k = W[(id(l), "kernel")]
    return float(np.float32(l.layer.coefficient)) * k if isinstance(l.layer, layers.EqualizedLearningRate) else k


def ref_forward(model, W, x, training, masks=None, pre=None):
    flat = model.flat_layers()
    at = [i for i, (l, _) in enumerate(flat) if is_mod(l) or l.kind == "noise"]
    if not any(is_mod(l) for l, _ in flat):
        return _inner[-1](model, W, x, training, masks, pre)
    assert not any(l.kind == "dropout" for l, _ in flat)
    noisy = any(l.kind == "noise" for l, _ in flat)
    maps = _maps.pop(0) if noisy else False
    w = PR.torch_pixelnorm(x, flat[0][0].epsilon) if flat[0][0].kind == "pixelnorm" else x      # the style source
    assert w.ndim == 2
    B, lo, o = x.shape[0], 0, 0
    for i in at:
        if i > lo:
            x = _inner[-1](_Part(flat[lo:i]), W, x, training, None, pre)
        l, s = flat[i]
        if l.kind == "noise":
            n = int(np.prod(s[:-1]))
            if maps is not False:
                m = torch.as_tensor(np.asarray(maps)[:, o:o + n]).to(DT).reshape(B, s[0], s[1], 1)
                x = x + W[(id(l), "noise_strength")] * m
            o += n
        else:
            x = torch_modconv(l.kind, x.reshape((B,) + tuple(s)), w, effective_kernel(l, W), W[(id(l), "style_kernel")], W[(id(l), "style_bias")],
                              W[(id(l), "bias")] if l.use_bias else None, l.stride, l.demodulate, l.epsilon, MIN_Q_SEEN)
            if l.activation == "tanh":
                x = torch.tanh(x)
        lo = i + 1
    assert maps is False or o == np.asarray(maps).shape[1]
    return _inner[-1](_Part(flat[lo:]), W, x, training, None, pre) if lo < len(flat) else x


@contextlib.contextmanager
def walker(maps=()):
    """ln_reference.ref_forward with the modulation branch in front of whatever stands there; enter it LAST (it must see the whole
    generator).  ``maps``: one [B, P] noise array (or False: no noise) per forward of a generator with NoiseInjection layers, in the
    order they run."""
    _maps[:] = list(maps)
    del MIN_Q_SEEN[:]
    _inner.append(LN.ref_forward)
    LN.ref_forward = ref_forward
    try:
        yield MIN_Q_SEEN
    finally:
        LN.ref_forward = _inner.pop()
        del _maps[:]


def style_index(model):
    """Positions of the style variables among the model's trainable variables."""
    own = {id(l) for l in model._own_layers()}
    return [i for i, (l, n, _, _, tr) in enumerate([e for e in model.store.entries if e[4] and id(e[0]) in own]) if n.startswith("style_")]


def ref_step(gen, disc, reals, rnd, gbs, objective=None, penalty_step=True):
    """tests/objective_reference.py's step reference (dict) for a generator with modulated stages, plus ``min_q`` (the smallest
    demodulation sum of any forward), ``min_style`` (the smallest max |gradient| of a style variable), pixelnorm_reference's
    ``min_ms`` and ``min_s`` = inf (no MinibatchStdDev here)."""
    import objective_reference as OR
    maps = [rnd["noise_d"], rnd["noise_g"]] if "noise_d" in rnd else []
    with MR.walker(), FS.walker(), PR.walker() as seen, walker(maps) as qs:
        ref = OR.ref_step_grads(gen, disc, reals, rnd, gbs, objective, penalty_step=penalty_step)
        ref["min_ms"] = min(seen) if seen else float("inf")
        ref["min_s"] = float("inf")
        ref["min_q"] = min(qs)
    ref["min_style"] = min(float(np.abs(ref["ggrads"][i]).max()) for i in style_index(gen))
    return ref


def check_guards(ref):
    """The assertions on the reference alone that precede every comparison."""
    PR.check_guards(ref)
    assert ref["min_q"] > MIN_Q, ref["min_q"]
    assert ref["min_style"] > MIN_STYLE_GRAD, ref["min_style"]


def randomize(model, rng, strength=0.5):
    """ln_reference.randomize; the style variables drawn afresh (style_bias starts at ones and a Glorot style_kernel is small: s
    would be nearly constant) and the noise strengths from N(0, strength^2) (they start at zero)."""
    LN.randomize(model, rng)
    own = {id(l) for l in model._own_layers()}
    ws = model.get_weights()
    for i, (l, n, _, shape, _) in enumerate([e for e in model.store.entries if id(e[0]) in own]):
        if n == "style_kernel":
            ws[i] = np.asarray(rng.normal(size=shape) * 0.5, np.float32)
        elif n == "style_bias":
            ws[i] = np.asarray(1.0 + rng.normal(size=shape) * 0.3, np.float32)
        elif n == "noise_strength":
            ws[i] = np.asarray(rng.normal(size=shape) * strength, np.float32)
    model.set_weights(ws)


def mixed_generator(arch="tiny"):
    """A hand-built stack that mixes a modulated and a plain stage: Dense + LeakyReLU + PixelNormalization, a demodulated transposed
    convolution, a PLAIN transposed convolution with bias + LeakyReLU, a demodulated one around an EqualizedLearningRate with a
    NoiseInjection, and a modulated tanh output convolution."""
    base, ch, convt, last = models._G[arch]
    k = models.KSIZE.get(arch, 5)
    m = layers.Sequential()
    m.add(layers.Dense(base * base * ch, input_shape=(models.LATENT[arch],)))
    m.add(layers.Reshape((base, base, ch)))
    m.add(layers.LeakyReLU())
    m.add(layers.PixelNormalization())
    for j, (filters, stride, _) in enumerate(convt):
        conv = layers.Conv2DTranspose(filters, (k, k), strides=(stride, stride), padding="same")
        if j == 1:
            m.add(conv)
        elif j == 2:
            m.add(layers.StyleModulation(layers.EqualizedLearningRate(conv)))
            m.add(layers.NoiseInjection())
        else:
            m.add(layers.StyleModulation(conv))
        m.add(layers.LeakyReLU())
    m.add(layers.StyleModulation(layers.Conv2D(last, (k, k), padding="same", use_bias=False, activation="tanh"), demodulate=False))
    m.latent_size = models.LATENT[arch]
    return m


def make_gan(arch, B, seed, gen_kw=None, disc_kw=None, objective=None, std=None, gbs=None, device=None, gen=None, **kw):
    """pixelnorm_reference.make_gan with ``normalization="style"`` for the generator unless ``gen`` (a callable that returns an
    unbuilt generator) is given, the style variables and strengths randomised, and noise_d / noise_g in the randomness where the
    generator has NoiseInjection layers."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = gen() if gen is not None else models.DCGANGenerator(arch=arch, **dict(dict(normalization="style"), **(gen_kw or {})))
    disc = models.DCGANDiscriminator(arch=arch, **(disc_kw or {}))
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    randomize(gen, rng), LN.randomize(disc, rng)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, objective=objective, **kw)
    else:
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = bg.BlurredWGANGP(gen, disc, hp, cfg, objective=objective, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = LN.draw(gan.discriminator, B, gen.latent_size, rng)
    P = noise_pixels(gen)
    if P:
        rnd = dict(rnd, noise_d=rng.normal(size=(B, P)).astype(np.float32), noise_g=rng.normal(size=(B, P)).astype(np.float32))
    return gan, reals, rnd
