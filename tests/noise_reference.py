"""The references of the NoiseInjection tests (a helper, not a test file).

1. bg_normal_f32 restated in numpy float64: Philox4x32-10 on 64-bit counters (third counter word 2), then Box-Muller inside each
   block exactly as include/bgan.h states it -- words (0, 1) give elements (0, 1), words (2, 3) give elements (2, 3);
   u1 = ((w_a >> 8) + 1) * 2^-24, u2 = (w_b >> 8) * 2^-24, r = sqrt(-2 log u1), the pair r cos(2 pi u2), r sin(2 pi u2).  The
   trigonometric functions are taken of the exact quadrant-reduced argument (what cospi / sinpi compute), not of a rounded 2 pi u2.
2. The two formulas of include/bgan.h "noise inputs" in numpy, in the dtype they are handed.
3. The layer in differentiable torch operations, and the torch-autograd float64 step reference: tests/ln_reference.py's walker with a
   ``noise`` branch put in front of it the way tests/pixelnorm_reference.py puts its branch (``walker(maps)``).  ``maps`` is the list
   of [B, P] noise arrays of the generator's forwards in the order the step runs them (D-step, G-step); a model without the layer
   (the critic) passes through."""
import contextlib

import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
import firsample_reference as FS
import ln_reference as LN
import mbstd_reference as MR
import pixelnorm_reference as PR

DT = torch.float64
MAX_ABS = 5.77          # sqrt(-2 log 2^-24) = sqrt(48 log 2) = 5.768...


# ---------------------------------------------------------------------------------------------------- 1. the draw
def philox4x32_10(ctr, key, c2):
    """Philox4x32-10 (Salmon et al., SC'11) on an array of 64-bit counters: counter words (lo, hi, c2, 0), key (lo, hi) -> [n, 4]."""
    ctr = np.asarray(ctr, np.uint64)
    c = [ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.full_like(ctr, c2), np.zeros_like(ctr)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=1)


def _cospi_sinpi(a):
    """(cos(pi a), sin(pi a)) for a in [0, 2) in float64, from the argument reduced to a quadrant exactly (a is a multiple of
    2^-23: every step below is exact)."""
    q = np.floor(2.0 * a + 0.5)                     # nearest multiple of 1/2
    t = (a - 0.5 * q) * np.pi                       # |t| <= pi / 4
    c, s = np.cos(t), np.sin(t)
    k = q.astype(np.int64) & 3
    return np.choose(k, [c, -s, -c, s]), np.choose(k, [s, c, -s, -c])


def normal_from_words(words):
    """[n, 4] Philox words -> [n, 4] float64 values."""
    w = np.asarray(words, np.uint64)
    out = np.empty(w.shape, np.float64)
    for a, b in ((0, 1), (2, 3)):
        u1 = ((w[:, a] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[:, b] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        c, s = _cospi_sinpi(2.0 * u2)
        out[:, a], out[:, b] = r * c, r * s
    return out


def np_normal(n, seed, offset=0):
    """The n values bg_normal_f32(out, n, seed, offset) draws, in float64."""
    blocks = (n + 3) // 4
    ctr = np.uint64(offset) + np.arange(blocks, dtype=np.uint64)
    return normal_from_words(philox4x32_10(ctr, seed, 2)).reshape(-1)[:n]


def statistics(z):
    """(mean, var, fourth moment, corr(even, odd), max |z|) of a draw."""
    z = np.asarray(z, np.float64)
    m = z.mean()
    return dict(mean=float(m), var=float(z.var()), m4=float((z ** 4).mean()), corr=float(np.corrcoef(z[0::2], z[1::2])[0, 1]),
                max=float(np.abs(z).max()))


def check_statistics(st):
    """The issue's bounds (5 standard errors at n = 2^20)."""
    assert abs(st["mean"]) < 5e-3, st
    assert abs(st["var"] - 1) < 7e-3, st
    assert abs(st["m4"] - 3) < 0.05, st
    assert abs(st["corr"]) < 5e-3, st
    assert st["max"] <= MAX_ABS, st


# ---------------------------------------------------------------------------------------------------- 2. numpy, kernel by kernel
def np_add(x, noise, strength, alpha):
    """x [R, C], noise [R], strength scalar -> y [R, C] in x's dtype: t = s * n rounded once, then x + t, then LeakyReLU."""
    dt = x.dtype.type
    t = (dt(strength) * noise.astype(x.dtype)).astype(x.dtype)
    a = (x + t[:, None]).astype(x.dtype)
    return np.where(a > 0, a, dt(alpha) * a).astype(x.dtype)


def np_grad(dz, noise, old=0.0, beta=0.0, scale=1.0):
    """float64: beta * old + scale * sum_r noise[r] * sum_c dz[r, c]."""
    s = float((np.asarray(noise, np.float64) * np.asarray(dz, np.float64).sum(1)).sum())
    return (beta * old if beta != 0.0 else 0.0) + scale * s


# ---------------------------------------------------------------------------------------------------- 3. torch
class _Part:
    """A stretch of a model's layer list, as the walker reads one."""

    def __init__(self, flat):
        self._flat = flat

    def flat_layers(self):
        return self._flat


_inner = [LN.ref_forward]
_maps = []              # the [B, P] noise arrays of the generator forwards still to come, in the step's order


def noise_pixels(model):
    return sum(int(np.prod(s[:-1])) for l, s in model.flat_layers() if l.kind == "noise")


def ref_forward(model, W, x, training, masks=None, pre=None):
    flat = model.flat_layers()
    at = [i for i, (l, _) in enumerate(flat) if l.kind == "noise"]
    if not at:
        return _inner[-1](model, W, x, training, masks, pre)
    assert not any(l.kind == "dropout" for l, _ in flat)
    assert _maps, "walker(maps): one [B, P] array per forward of a model with the layer"
    maps = _maps.pop(0)
    B, lo, o = x.shape[0], 0, 0
    for i in at:
        x = _inner[-1](_Part(flat[lo:i]), W, x, training, None, pre)
        l, s = flat[i]
        n = int(np.prod(s[:-1]))
        if maps is not False:
            m = torch.as_tensor(np.asarray(maps)[:, o:o + n]).to(DT).reshape(B, s[0], s[1], 1)
            x = x + W[(id(l), "noise_strength")] * m
        o, lo = o + n, i + 1
    assert maps is False or o == np.asarray(maps).shape[1]
    return _inner[-1](_Part(flat[lo:]), W, x, training, None, pre)


@contextlib.contextmanager
def walker(maps):
    """ln_reference.ref_forward with the ``noise`` branch in front of whatever stands there.  ``maps``: see the module docstring; an
    entry False is a forward without noise."""
    _maps[:] = list(maps)
    _inner.append(LN.ref_forward)
    LN.ref_forward = ref_forward
    try:
        yield
    finally:
        LN.ref_forward = _inner.pop()
        del _maps[:]


def ref_step(gen, disc, reals, rnd, gbs, objective=None, penalty_step=True):
    """tests/objective_reference.py's step reference (dict) for a generator with the layer: the D-step's forward reads
    rnd["noise_d"], the G-step's rnd["noise_g"].  Plus pixelnorm_reference's ``min_ms`` (inf without PixelNormalization) and
    ``min_s`` (inf: no MinibatchStdDev here).  The equalised-learning-rate coefficients are firsample_reference's."""
    import objective_reference as OR
    with MR.walker(), FS.walker(), PR.walker() as seen, walker([rnd["noise_d"], rnd["noise_g"]]):
        ref = OR.ref_step_grads(gen, disc, reals, rnd, gbs, objective, penalty_step=penalty_step)
        ref["min_ms"] = min(seen) if seen else float("inf")
        ref["min_s"] = float("inf")
    return ref


check_guards = PR.check_guards


def randomize(model, rng, scale=0.5):
    """ln_reference.randomize, then every noise strength drawn from N(0, scale^2) (they start at zero: nothing would be tested)."""
    LN.randomize(model, rng)
    own = {id(l) for l in model._own_layers()}
    ws = model.get_weights()
    for i, (l, n, _, shape, _) in enumerate([e for e in model.store.entries if id(e[0]) in own]):
        if n == "noise_strength":
            ws[i] = np.asarray(rng.normal(size=shape) * scale, np.float32)
    model.set_weights(ws)


def draw_noise(rnd, gen, B, rng):
    """``rnd`` plus noise_d / noise_g: [B, P] standard normal values in float32 (product and reference see the same numbers)."""
    P = noise_pixels(gen)
    return dict(rnd, noise_d=rng.normal(size=(B, P)).astype(np.float32), noise_g=rng.normal(size=(B, P)).astype(np.float32))


def hand_built_generator(arch="tiny"):
    """A generator with NoiseInjection stages WITHOUT PixelNormalization: the reference Dense + BatchNormalization block, then
    (transposed) convolutions with a bias, each followed by NoiseInjection -> LeakyReLU, then the tanh output layer."""
    base, ch, convt, last = models._G[arch]
    k = models.KSIZE.get(arch, 5)
    m = layers.Sequential()
    m.add(layers.Dense(base * base * ch, use_bias=False, input_shape=(models.LATENT[arch],)))
    m.add(layers.BatchNormalization())
    m.add(layers.LeakyReLU())
    m.add(layers.Reshape((base, base, ch)))
    for filters, stride, act in convt:
        m.add(layers.Conv2DTranspose(filters, (k, k), strides=(stride, stride), padding="same", use_bias=act is None, activation=act))
        if act is None:
            m.add(layers.NoiseInjection())
            m.add(layers.LeakyReLU())
    if last is not None:
        m.add(layers.Conv2D(last, (k, k), padding="same", use_bias=False, activation="tanh"))
    m.latent_size = models.LATENT[arch]
    return m


def make_gan(arch, B, seed, gen_kw=None, disc_kw=None, objective=None, std=None, gbs=None, device=None, gen=None, **kw):
    """pixelnorm_reference.make_gan with ``noise=True`` (and ``normalization="pixel"``) for the generator unless ``gen`` (a callable
    that returns an unbuilt generator) is given, the strengths randomised, and noise_d / noise_g in the randomness."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = gen() if gen is not None else models.DCGANGenerator(arch=arch, **dict(dict(normalization="pixel", noise=True), **(gen_kw or {})))
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
    rnd = draw_noise(LN.draw(gan.discriminator, B, gen.latent_size, rng), gen, B, rng)
    return gan, reals, rnd
