"""The float64 reference of the SpectralNormalization tests (a helper, not a test file).

Kernel level: numpy formulas of one power round, the sigma-only refresh, W-bar = W / sigma and the gradient map, evaluated in any
dtype -- float64 is the reference, the same code in float32 measures what float32 arithmetic loses, from which the tests' bound
comes.  Model level: tests/ln_reference.py's walk over the product model's own layer list, with the kernel of every wrapped layer
replaced by W / sigma: at the start of a model's step the round runs in float64 from the product's ``vector_u``, sigma = v^T W u
keeps u and v detached, and autograd differentiates the loss of oracle/step.py down to the raw W (create_graph=True for the penalty)."""
import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
import ln_reference as LN
from ln_reference import DT, ref_forward, ref_params

EPS = 1e-12
FLOOR = 16 * 2.0 ** -24       # a few roundings of a float32 result itself


# ---------------------------------------------------------------------------------------------------- kernel level
def normalize(x):
    return x / max(np.sqrt((x * x).sum(dtype=x.dtype)), x.dtype.type(EPS))


def power_round(W, u):
    """t = W u, v = normalize(t), s = W^T v, u = normalize(s), sigma = v^T W u = s . u; in W's dtype."""
    v = normalize(W @ u)
    s = W.T @ v
    u = normalize(s)
    return u, v, (s * u).sum(dtype=W.dtype)


def sigma_only(W, u, v):
    return (v * (W @ u)).sum(dtype=W.dtype)


def grad_map(g, Wbar, u, v, sigma):
    """dL/dW = (g - <g, W-bar> v u^T) / sigma."""
    return (g - (g * Wbar).sum(dtype=g.dtype) * np.outer(v, u)) / sigma


def kernel_case(K, N, seed, rounds=1, W=None):
    """Inputs (float32) of one kernel-level case, its float64 reference and the bound of every output: 4 x the error a float32 numpy
    evaluation of the same formulas shows against the float64 one, never below FLOOR."""
    rng = np.random.default_rng(seed)
    if W is None:
        W = rng.normal(size=(K, N)).astype(np.float32)
    u0 = normalize(rng.normal(size=N)).astype(np.float32)
    g = rng.normal(size=(K, N)).astype(np.float32)
    out = {}
    for dt in (np.float64, np.float32):
        Wd, u = W.astype(dt), u0.astype(dt)
        for _ in range(rounds):
            u, v, sigma = power_round(Wd, u)
        Wbar = Wd / sigma
        out[dt] = dict(u=u, v=v, sigma=sigma, Wbar=Wbar, grad=grad_map(g.astype(dt), Wbar, u, v, sigma))
    ref, f32 = out[np.float64], out[np.float32]
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64).ravel() - np.asarray(b, np.float64).ravel())
                             / max(np.linalg.norm(np.asarray(b, np.float64).ravel()), 1e-300))
    bound = {k: max(4 * rel(f32[k], ref[k]), FLOOR) for k in ref}
    return dict(W=W, u0=u0, g=g, ref=ref, bound=bound)


# ---------------------------------------------------------------------------------------------------- model level
def wrapped(model):
    return [l for l in model._own_layers() if isinstance(l, layers.SpectralNormalization)]


def effective(model, W, iterate):
    """``W`` (ln_reference.ref_params) with the kernel of every wrapped layer replaced by W / sigma, sigma = v^T W u with u and v
    detached.  ``iterate``: the layer's power rounds first, from the u that ``W`` holds; u and v in ``W`` are replaced by the new
    ones (the state the product keeps).  Returns (the dictionary, {layer id: (W-bar, sigma)})."""
    E, info = dict(W), {}
    for l in wrapped(model):
        raw = W[(id(l), "kernel")]
        Wm = raw.reshape(-1, raw.shape[-1])
        u, v = W[(id(l), "vector_u")].detach(), W[(id(l), "vector_v")].detach()
        if iterate:
            with torch.no_grad():
                for _ in range(l.power_iterations):
                    t = Wm @ u
                    v = t / t.norm().clamp_min(EPS)
                    s = Wm.T @ v
                    u = s / s.norm().clamp_min(EPS)
            W[(id(l), "vector_u")], W[(id(l), "vector_v")] = u, v
        sigma = v @ (Wm @ u)
        W[(id(l), "sigma")] = sigma.detach().reshape(1)
        wbar = raw / sigma
        E[(id(l), "kernel")] = wbar
        info[id(l)] = (wbar, sigma.detach())
    return E, info


def ref_step_grads(gen, disc, reals, rnd, gbs, gp_coef=10.0, e_drift=1e-4):
    """ln_reference.ref_step_grads on the effective weights.  Returns dict(dgrads, ggrads, fakes, kink, norm, signal, state):
    ``signal`` = min over wrapped tensors of max|dL/dW| / (max|dL/dW-bar| / sigma) -- the projection must not have cancelled what
    the tolerance is relative to; ``state`` = {"d" / "g": [(u, v, sigma)] per wrapped layer} after the step."""
    T = lambda a: torch.as_tensor(np.asarray(a)).to(DT)
    Wg, tg = ref_params(gen)
    Wd, td = ref_params(disc)
    pre = []
    reals, B = T(reals), reals.shape[0]
    Ed, info_d = effective(disc, Wd, iterate=True)              # the critic's round: the start of its step
    Eg, _ = effective(gen, Wg, iterate=False)
    with torch.no_grad():
        fakes = ref_forward(gen, Eg, T(rnd["z_d"]), False, pre=pre)
    fs = ref_forward(disc, Ed, fakes, True, rnd["mask_fake"], pre)
    rs = ref_forward(disc, Ed, reals, True, rnd["mask_real"], pre)
    xhat = (reals + T(rnd["alpha"]).view(B, 1, 1, 1) * (fakes - reals)).detach().requires_grad_(True)
    yhat = ref_forward(disc, Ed, xhat, False, pre=pre)
    g, = torch.autograd.grad(yhat.sum(), xhat, create_graph=True)
    norms = g.reshape(B, -1).norm(dim=1)
    gp = ((norms - 1.0) ** 2).mean()
    loss_vec = (fs - rs).sum() / gbs + gp_coef * gp + e_drift * (fs.abs().view(B) + rs.abs().view(B))
    signal = []
    dgrads = _grads_and_signal(loss_vec.sum(), td, disc, Wd, info_d, signal)
    Eg, info_g = effective(gen, Wg, iterate=True)               # the generator's round: the start of its step
    Ed, _ = effective(disc, Wd, iterate=False)
    fk = ref_forward(gen, Eg, T(rnd["z_g"]), True, pre=pre)
    sc = ref_forward(disc, Ed, fk, False, pre=pre)
    ggrads = _grads_and_signal(-sc.sum() / gbs, tg, gen, Wg, info_g, signal)
    state = {k: [tuple(W[(id(l), n)].numpy() for n in ("vector_u", "vector_v", "sigma")) for l in wrapped(m)]
             for k, m, W in (("d", disc, Wd), ("g", gen, Wg))}
    return dict(dgrads=dgrads, ggrads=ggrads, fakes=fakes.numpy(), kink=min(pre), norm=float(norms.detach().min()),
                signal=min(signal) if signal else float("inf"), state=state)


def _grads_and_signal(loss, train, model, W, info, signal):
    ls = wrapped(model)
    wbars = [info[id(l)][0] for l in ls]
    grads = torch.autograd.grad(loss, train + wbars)
    for l, gbar in zip(ls, grads[len(train):]):
        raw = next(t for t, leaf in zip(grads, train) if leaf is W[(id(l), "kernel")])
        signal.append(float(raw.abs().max() / (gbar.abs().max() / info[id(l)][1])))
    return [t.numpy() for t in grads[:len(train)]]


def check_conditions(ref):
    """The assertions on the reference alone that precede every comparison."""
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM, ref["norm"]
    assert ref["signal"] >= 0.05, ref["signal"]


def make_gan(arch, B, seed, critic_sn=True, generator_sn=False, up="transpose", down="stride", normalization=None, std=None, gbs=None,
             device=None, **kw):
    """ln_reference.make_gan with the two ``spectral_norm`` arguments."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch, upsampling=up, spectral_norm=generator_sn)
    disc = models.DCGANDiscriminator(arch=arch, downsampling=down, normalization=normalization, spectral_norm=critic_sn)
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    LN.randomize(gen, rng), LN.randomize(disc, rng)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, **kw)
    else:
        gan = bg.BlurredWGANGP(gen, disc, bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B), cfg, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = LN.draw(gan.discriminator, B, gen.latent_size, rng)
    return gan, reals, rnd
