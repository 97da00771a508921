"""The float64 reference of the DiffAugment tests (a helper, not a test file).

Kernel level: numpy formulas of the transform T(x) = L x + k of include/bgan.h "differentiable augmentation", of its linear part
and of the adjoint L^T, evaluated in any dtype -- float64 is the reference, the same code in float32 measures what float32
arithmetic loses, from which the tests' bound comes (tests/sn_reference.py: kernel_case's rule).  The decode of a row of uniforms is
written here a second time, in numpy float32.

Model level: a torch-float64 differentiable T, put behind the blur in front of tests/ln_reference.py's walk over the product
model's own layer list (with tests/sn_reference.py's effective weights where the critic is spectrally normalised); autograd
differentiates the loss of oracle/step.py through it, the penalty with create_graph=True."""
import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models
import ln_reference as LN
import sn_reference as SR
from ln_reference import DT, ref_params
from oracle import torch_ref as TR

F32 = np.float32
FLOOR = SR.FLOOR
HI = float(np.nextafter(F32(1), F32(0)))        # 1 - 2^-24: the largest uniform
OPS = {"color": 1, "translation": 2, "cutout": 4}


def as_cfg(policy, translation_ratio=0.125, cutout_ratio=0.5):
    return policy if isinstance(policy, bg.DiffAugment) else bg.DiffAugment(policy, translation_ratio, cutout_ratio)


# ---------------------------------------------------------------------------------------------------- decode
def half_up(extent, ratio):
    return int(np.floor(F32(extent) * F32(ratio) + F32(0.5)))


def pick(u, n):
    return min(int(np.floor(F32(u) * F32(n))), n - 1)


def decode(u, H, W, cfg):
    """One row of eight uniforms -> dict(b, s, c (float32), ty, tx, y0, x0, cy, cx): the cutout box is rows [y0, y0 + cy) x columns
    [x0, x0 + cx).  Operations absent from the policy take their neutral values."""
    names = cfg.policy.split(",")
    d = dict(b=F32(0), s=F32(1), c=F32(1), ty=0, tx=0, y0=0, x0=0, cy=0, cx=0)
    if "color" in names:
        d.update(b=F32(u[0]) - F32(0.5), s=F32(2) * F32(u[1]), c=F32(u[2]) + F32(0.5))
    if "translation" in names:
        Sy, Sx = half_up(H, cfg.translation_ratio), half_up(W, cfg.translation_ratio)
        d.update(ty=pick(u[3], 2 * Sy + 1) - Sy, tx=pick(u[4], 2 * Sx + 1) - Sx)
    if "cutout" in names:
        cy, cx = half_up(H, cfg.cutout_ratio), half_up(W, cfg.cutout_ratio)
        d.update(cy=cy, cx=cx, y0=pick(u[5], H + 1 - cy % 2) - cy // 2, x0=pick(u[6], W + 1 - cx % 2) - cx // 2)
    return d


def _shift_slices(n, t):
    """(destination, source) index ranges of w(i) = v(i + t) inside [0, n)."""
    lo, hi = max(0, -t), min(n, n - t)
    return (slice(lo, max(lo, hi)), slice(lo + t, max(lo, hi) + t))


def keep_mask(d, H, W):
    """[H, W] bool: False inside the cutout box."""
    i, j = np.arange(H)[:, None], np.arange(W)[None, :]
    return ~((i >= d["y0"]) & (i < d["y0"] + d["cy"]) & (j >= d["x0"]) & (j < d["x0"] + d["cx"]))


# ---------------------------------------------------------------------------------------------------- numpy, any dtype
def np_T(x, params, cfg, linear=False, dtype=np.float64):
    """y = T(x) (``linear``: L x) of x [n, H, W, C] with params [n, 8], evaluated in ``dtype``."""
    x = np.asarray(x, dtype)
    n, H, W, C = x.shape
    color = "color" in cfg.policy.split(",")
    y = np.zeros_like(x)
    for k in range(n):
        d = decode(params[k], H, W, cfg)
        v = x[k]
        if color:
            b, s, c = (dtype(0) if linear else dtype(d["b"])), dtype(d["s"]), dtype(d["c"])
            m, mu = v.mean(axis=-1, keepdims=True, dtype=dtype), v.mean(dtype=dtype)
            v = c * (s * (v - m) + m - mu) + mu + b
        (di, si), (dj, sj) = _shift_slices(H, d["ty"]), _shift_slices(W, d["tx"])
        w = np.zeros_like(v)
        w[di, dj] = v[si, sj]
        y[k] = np.where(keep_mask(d, H, W)[:, :, None], w, dtype(0))
    return y


def np_LT(g, params, cfg, dtype=np.float64):
    """dx = L^T g."""
    g = np.asarray(g, dtype)
    n, H, W, C = g.shape
    color = "color" in cfg.policy.split(",")
    dx = np.zeros_like(g)
    for k in range(n):
        d = decode(params[k], H, W, cfg)
        gm = np.where(keep_mask(d, H, W)[:, :, None], g[k], dtype(0))
        (di, si), (dj, sj) = _shift_slices(H, d["ty"]), _shift_slices(W, d["tx"])
        h = np.zeros_like(gm)
        h[si, sj] = gm[di, dj]              # h(i', j') = g(i' - ty, j' - tx)
        if color:
            s, c = dtype(d["s"]), dtype(d["c"])
            e = c * h + (dtype(1) - c) * h.mean(dtype=dtype)
            h = s * e + (dtype(1) - s) * e.mean(axis=-1, keepdims=True, dtype=dtype)
        dx[k] = h
    return dx


def offset_map(params, shape, cfg, dtype=np.float64):
    """T(x) - L x: b on the pixels that are neither cut nor shifted in from outside the map, 0 elsewhere."""
    return np_T(np.zeros(shape, dtype), params, cfg, dtype=dtype)


SPECIAL_ROWS = 4


def injected_params(n, seed, batches=None):
    """[batches, n, 8] float32: seeded uniforms whose first rows are, spread over as many batches as n asks for, the hard ones --
    both extreme shifts in both axes in all four combinations, each with the cutout offsets 0 / last in the matching combination,
    s = 0 (u1 = 0) and c = 0.5 (u2 = 0)."""
    rng = np.random.default_rng(seed)
    special = np.array([rng.uniform(size=8) for _ in range(SPECIAL_ROWS)], F32)
    for r, (a, b) in enumerate(((0.0, 0.0), (0.0, HI), (HI, 0.0), (HI, HI))):
        special[r, 3], special[r, 4], special[r, 5], special[r, 6] = a, b, a, b
    special[0, 1] = special[3, 1] = 0.0
    special[1, 2] = special[3, 2] = 0.0
    nb = -(-SPECIAL_ROWS // n) if batches is None else batches
    out = rng.uniform(size=(nb, n, 8)).astype(F32)
    out = np.minimum(out, F32(HI))
    flat = out.reshape(-1, 8)
    for r in range(min(SPECIAL_ROWS, nb * n)):
        k, i = divmod(r, n) if n < SPECIAL_ROWS else (0, r)
        out[k, i] = special[r]
    assert flat.min() >= 0 and flat.max() < 1
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def kernel_case(shape, policy, seed, params=None):
    """Inputs (float32) of one kernel-level case, the float64 reference of the three entry points and the bound of each: 4 x the
    error a float32 numpy evaluation of the same formulas shows against the float64 one, never below FLOOR (relative L2, as
    sn_reference.kernel_case).  ``params``: [n, 8], default injected_params(n, seed)[0]."""
    cfg = as_cfg(policy)
    rng = np.random.default_rng(seed)
    x = rng.normal(size=shape).astype(F32)
    g = rng.normal(size=shape).astype(F32)
    if params is None:
        params = injected_params(shape[0], seed)[0]
    out = {}
    for dt in (np.float64, np.float32):
        out[dt] = dict(fwd=np_T(x, params, cfg, dtype=dt), lin=np_T(x, params, cfg, linear=True, dtype=dt), adj=np_LT(g, params, cfg, dtype=dt))
    ref, f32 = out[np.float64], out[np.float32]
    bound = {k: max(4 * rel(f32[k], ref[k]), FLOOR) for k in ref}
    return dict(x=x, g=g, params=params, cfg=cfg, ref=ref, bound=bound)


# ---------------------------------------------------------------------------------------------------- torch, differentiable
def torch_T(x, params, cfg, linear=False):
    """T of a float64 torch batch [n, H, W, C], differentiable with respect to x."""
    n, H, W, C = x.shape
    color = "color" in cfg.policy.split(",")
    rows = []
    for k in range(n):
        d = decode(params[k], H, W, cfg)
        v = x[k]
        if color:
            b, s, c = (0.0 if linear else float(d["b"])), float(d["s"]), float(d["c"])
            m, mu = v.mean(dim=-1, keepdim=True), v.mean()
            v = c * (s * (v - m) + m - mu) + mu + b
        (di, si), (dj, sj) = _shift_slices(H, d["ty"]), _shift_slices(W, d["tx"])
        w = torch.zeros_like(v)
        w[di, dj] = v[si, sj]
        rows.append(w * torch.as_tensor(keep_mask(d, H, W)[:, :, None].astype(np.float64)))
    return torch.stack(rows)


class _BehindTheBlur:
    """The layer list of a critic without its leading blur: what ln_reference.ref_forward walks once blur and T have been applied."""

    def __init__(self, model):
        self._layers = [(l, s) for l, s in model.flat_layers() if l.kind != "blur"]
        self.blur = next((l for l, _ in model.flat_layers() if l.kind == "blur"), None)

    def flat_layers(self):
        return self._layers


def critic_forward(disc, W, x, training, masks, pre, cfg, params):
    """The critic on T(blur(x)); ``cfg`` None: the plain walk."""
    if cfg is None:
        return LN.ref_forward(disc, W, x, training, masks, pre)
    tail = _BehindTheBlur(disc)
    if tail.blur is not None:
        x = TR.blur(x, float(tail.blur.std))
    return LN.ref_forward(tail, W, torch_T(x, params, cfg), training, masks, pre)


def ref_step_grads(gen, disc, reals, rnd, gbs, augment, gp_coef=10.0, e_drift=1e-4):
    """sn_reference.ref_step_grads with every critic pass behind T: rnd["aug_fake" / "aug_real" / "aug_hat" / "aug_g"] are the
    passes' [B, 8] params.  Returns dict(dgrads, ggrads, fakes, kink, norm, signal)."""
    cfg = None if augment is None else as_cfg(augment)
    T = lambda a: torch.as_tensor(np.asarray(a)).to(DT)
    Wg, tg = ref_params(gen)
    Wd, td = ref_params(disc)
    pre = []
    reals, B = T(reals), reals.shape[0]
    Ed, info_d = SR.effective(disc, Wd, iterate=True)
    Eg, _ = SR.effective(gen, Wg, iterate=False)
    with torch.no_grad():
        fakes = LN.ref_forward(gen, Eg, T(rnd["z_d"]), False, pre=pre)
    fs = critic_forward(disc, Ed, fakes, True, rnd["mask_fake"], pre, cfg, rnd.get("aug_fake"))
    rs = critic_forward(disc, Ed, reals, True, rnd["mask_real"], pre, cfg, rnd.get("aug_real"))
    xhat = (reals + T(rnd["alpha"]).view(B, 1, 1, 1) * (fakes - reals)).detach().requires_grad_(True)
    yhat = critic_forward(disc, Ed, xhat, False, None, pre, cfg, rnd.get("aug_hat"))
    g, = torch.autograd.grad(yhat.sum(), xhat, create_graph=True)
    norms = g.reshape(B, -1).norm(dim=1)
    gp = ((norms - 1.0) ** 2).mean()
    loss_vec = (fs - rs).sum() / gbs + gp_coef * gp + e_drift * (fs.abs().view(B) + rs.abs().view(B))
    signal = []
    dgrads = SR._grads_and_signal(loss_vec.sum(), td, disc, Wd, info_d, signal)
    Eg, info_g = SR.effective(gen, Wg, iterate=True)
    Ed, _ = SR.effective(disc, Wd, iterate=False)
    fk = LN.ref_forward(gen, Eg, T(rnd["z_g"]), True, pre=pre)
    sc = critic_forward(disc, Ed, fk, False, None, pre, cfg, rnd.get("aug_g"))
    ggrads = SR._grads_and_signal(-sc.sum() / gbs, tg, gen, Wg, info_g, signal)
    return dict(dgrads=dgrads, ggrads=ggrads, fakes=fakes.numpy(), kink=min(pre), norm=float(norms.detach().min()),
                signal=min(signal) if signal else float("inf"))


def check_conditions(ref):
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM, ref["norm"]
    assert ref["signal"] >= 0.05, ref["signal"]


def draw_aug(rnd, B, seed):
    """Adds the four [B, 8] param blocks of a step to ``rnd`` (seeded; the first rows of aug_hat are the hard ones of
    injected_params: extreme shifts and cutout offsets, s = 0, c = 0.5)."""
    rng = np.random.default_rng(seed + 1000)
    for key in ("aug_fake", "aug_real", "aug_g"):
        rnd[key] = np.minimum(rng.uniform(size=(B, 8)).astype(F32), F32(HI))
    rnd["aug_hat"] = injected_params(B, seed + 2000, batches=1)[0]
    return rnd


def make_gan(arch, B, seed, augment, critic_sn=False, down="stride", normalization=None, std=None, gbs=None, device=None, **kw):
    """sn_reference.make_gan with ``augment=`` and the augmentation's injected draws."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch)
    disc = models.DCGANDiscriminator(arch=arch, downsampling=down, normalization=normalization, spectral_norm=critic_sn)
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    LN.randomize(gen, rng), LN.randomize(disc, rng)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, augment=augment, **kw)
    else:
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = bg.BlurredWGANGP(gen, disc, hp, cfg, augment=augment, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = draw_aug(LN.draw(gan.discriminator, B, gen.latent_size, rng), B, seed)
    return gan, reals, rnd
