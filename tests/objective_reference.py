"""The float64 reference of the GAN-objective tests (a helper, not a test file).

Kernel level: numpy formulas of bg_gan_d_loss, bg_gan_g_loss and bg_gp_seed_target_f32 (include/bgan.h "GAN objectives"), evaluated in
any dtype: float64 is the reference; float32 is the formula the hinge and Wasserstein seeds and the seed kernel at t = 0 must equal
bit for bit (every operation of theirs is one IEEE operation on the same operands, and the library is built without contraction).

Model level: tests/diffaug_reference.py's step (tests/ln_reference.py's walk over the product model's own layer list, the effective
weights of tests/sn_reference.py, T behind the blur) with the loss swapped in, alpha forced to 0 or 1 where the objective puts the
penalty on the reals or the fakes, (n - t)^2, and the coefficient times the interval -- or the penalty left out."""
import numpy as np
import torch
import torch.nn.functional as F

import blurred_gan_amd as bg
from blurred_gan_amd import models
import diffaug_reference as DR
import ln_reference as LN
import sn_reference as SR
from ln_reference import DT, ref_params

F32 = np.float32
FLOOR = SR.FLOOR
TINY = 2.0 ** -126          # the smallest normal float32: below it the format keeps no relative precision
LOSS = {"wasserstein": 0, "hinge": 1, "nonsaturating": 2}
HINGE_MARGIN = 1e-3         # no score of a hinge case may lie this close to its hinge


# ---------------------------------------------------------------------------------------------------- numpy, any dtype
def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def np_d_loss(fs, rs, norms, loss, inv_gbs, gp_coef, t, e_drift, vec_scale, dtype=np.float64):
    """dict(dfs, drs, met [6], mag [6]): ``mag`` is, per metric slot, the sum of the absolute values of the terms that enter it."""
    c = lambda v: np.asarray(v, dtype)
    fs, rs, inv, e, t, gc = c(fs), c(rs), c(inv_gbs), c(e_drift), c(t), c(gp_coef)
    w = c(vec_scale) * inv
    B = fs.size
    if loss == "hinge":
        terms = np.maximum(1 + fs, 0) + np.maximum(1 - rs, 0)
        dfs, drs = np.where(fs > -1, w, c(0)), np.where(rs < 1, -w, c(0))
    elif loss == "nonsaturating":
        terms = softplus(fs) + softplus(-rs)
        dfs, drs = w * sigmoid(fs), -w * sigmoid(-rs)
    else:
        terms = fs - rs
        dfs, drs = np.full(B, w, dtype), np.full(B, -w, dtype)
    dfs, drs = dfs + e * np.sign(fs), drs + e * np.sign(rs)
    drift = e * (np.abs(fs) + np.abs(rs))
    sq = np.zeros(B, dtype) if norms is None else (c(norms) - t) ** 2
    gp = sq.sum() / B
    lw = terms.sum() * inv
    met = np.array([fs.sum() / B, rs.sum() / B, lw + gc * gp + drift.sum() / B, gc * gp, drift.sum() / B, gp], dtype)
    a = lambda v: float(np.abs(np.asarray(v, np.float64)).sum())
    lterms = a(fs) + a(rs) if loss == "wasserstein" else a(terms)
    mag = np.array([a(fs) / B, a(rs) / B, lterms * float(inv) + float(gc) * a(sq) / B + a(drift) / B, float(gc) * a(sq) / B, a(drift) / B,
                    a(sq) / B])
    return dict(dfs=dfs.astype(dtype), drs=drs.astype(dtype), met=met, mag=mag)


def np_g_loss(s, loss, inv_gbs, dtype=np.float64):
    s, inv = np.asarray(s, dtype), np.asarray(inv_gbs, dtype)
    B = s.size
    a = lambda v: float(np.abs(np.asarray(v, np.float64)).sum())
    if loss == "nonsaturating":
        terms = softplus(-s)
        return dict(ds=(-inv * sigmoid(-s)).astype(dtype), met=np.array([s.sum() / B, terms.sum() * inv], dtype),
                    mag=np.array([a(s) / B, a(terms) * float(inv)]))
    return dict(ds=np.full(B, -inv, dtype), met=np.array([s.sum() / B, -s.sum() * inv], dtype), mag=np.array([a(s) / B, a(s) * float(inv)]))


def np_gp_seed(g, norms, coef, t, guard, dtype=np.float64):
    """out = coef * ((n - t) / n) * g; t == 0: coef * g; ``guard``: 0 for a sample of zero norm."""
    g, n, coef, t = np.asarray(g, dtype), np.asarray(norms, dtype)[:, None], dtype(coef), dtype(t)
    if t == 0:
        return coef * g
    with np.errstate(divide="ignore", invalid="ignore"):
        out = coef * ((n - t) / n) * g
    return np.where(n == 0, dtype(0), out) if guard else out


# ---------------------------------------------------------------------------------------------------- torch, whole steps
def critic_loss(loss, fs, rs):
    if loss == "hinge":
        return (F.relu(1 + fs) + F.relu(1 - rs)).sum()
    if loss == "nonsaturating":
        return (F.softplus(fs) + F.softplus(-rs)).sum()
    return (fs - rs).sum()


def generator_loss(loss, s):
    return F.softplus(-s).sum() if loss == "nonsaturating" else -s.sum()


def ref_step_grads(gen, disc, reals, rnd, gbs, objective, penalty_step=True, augment=None, gp_coef=10.0, e_drift=1e-4, penalty_class=True):
    """diffaug_reference.ref_step_grads under ``objective``.  ``penalty_step`` False: a step of a lazy objective between two
    penalties (drift term and vector loss stay).  ``penalty_class`` False: the WGAN class -- a scalar loss, no drift, no penalty.
    Returns dict(dgrads, ggrads, fakes, kink, norm, signal, fs, rs, disc_loss, gen_loss, gp_term, norm_term)."""
    obj = bg.objective.as_objective(objective)
    cfg = None if augment is None else DR.as_cfg(augment)
    T = lambda a: torch.as_tensor(np.asarray(a)).to(DT)
    Wg, tg = ref_params(gen)
    Wd, td = ref_params(disc)
    pre = []
    reals, B = T(reals), reals.shape[0]
    Ed, info_d = SR.effective(disc, Wd, iterate=True)
    Eg, _ = SR.effective(gen, Wg, iterate=False)
    with torch.no_grad():
        fakes = LN.ref_forward(gen, Eg, T(rnd["z_d"]), False, pre=pre)
    fs = DR.critic_forward(disc, Ed, fakes, True, rnd["mask_fake"], pre, cfg, rnd.get("aug_fake"))
    rs = DR.critic_forward(disc, Ed, reals, True, rnd["mask_real"], pre, cfg, rnd.get("aug_real"))
    loss = critic_loss(obj.loss, fs, rs) / gbs
    gp_term, min_norm = torch.zeros((), dtype=DT), float("inf")
    if penalty_class and penalty_step:
        alpha = T(rnd["alpha"]) if obj.penalty_alpha is None else torch.full((B,), obj.penalty_alpha, dtype=DT)
        xhat = (reals + alpha.view(B, 1, 1, 1) * (fakes - reals)).detach().requires_grad_(True)
        yhat = DR.critic_forward(disc, Ed, xhat, False, None, pre, cfg, rnd.get("aug_hat"))
        g, = torch.autograd.grad(yhat.sum(), xhat, create_graph=True)
        norms = g.reshape(B, -1).norm(dim=1)
        gp_term = gp_coef * obj.penalty_interval * ((norms - obj.penalty_target) ** 2).mean()
        min_norm = float(norms.detach().min())
    if penalty_class:
        loss_vec = loss + gp_term + e_drift * (fs.abs().view(B) + rs.abs().view(B))
    else:
        loss_vec = loss.view(1)
    signal = []
    dgrads = SR._grads_and_signal(loss_vec.sum(), td, disc, Wd, info_d, signal)
    Eg, info_g = SR.effective(gen, Wg, iterate=True)
    Ed, _ = SR.effective(disc, Wd, iterate=False)
    fk = LN.ref_forward(gen, Eg, T(rnd["z_g"]), True, pre=pre)
    sc = DR.critic_forward(disc, Ed, fk, False, None, pre, cfg, rnd.get("aug_g"))
    gloss = generator_loss(obj.loss, sc) / gbs
    ggrads = SR._grads_and_signal(gloss, tg, gen, Wg, info_g, signal)
    return dict(dgrads=dgrads, ggrads=ggrads, fakes=fakes.numpy(), kink=min(pre), norm=min_norm, signal=min(signal) if signal else float("inf"),
                fs=fs.detach().numpy().ravel(), rs=rs.detach().numpy().ravel(), disc_loss=float(loss_vec.detach().mean()),
                gen_loss=float(gloss.detach()), gp_term=float(gp_term.detach()), loss=obj.loss,
                norm_term=float(e_drift * (fs.abs() + rs.abs()).detach().mean()) if penalty_class else 0.0)


def check_conditions(ref, hinge_sides=True):
    """The assertions on the reference alone that precede every comparison: diffaug_reference's, and for a hinge case a score on
    each side of either hinge with none within HINGE_MARGIN of it (``hinge_sides`` False: only the margin -- the one case whose
    critic cannot reach a hinge, and says so)."""
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM, ref["norm"]
    assert ref["signal"] >= 0.05, ref["signal"]
    if ref["loss"] == "hinge":
        fs, rs = ref["fs"], ref["rs"]
        assert not hinge_sides or fs.min() < -1 < fs.max(), fs
        assert not hinge_sides or rs.min() < 1 < rs.max(), rs
        assert np.abs(fs + 1).min() > HINGE_MARGIN and np.abs(rs - 1).min() > HINGE_MARGIN, (fs, rs)


def scale_scores(disc, score_scale, score_bias=None):
    """Multiplies the last Dense kernel and bias of the critic (the stock tiny critics score within +-0.8: no score would reach a
    hinge or leave the middle of the sigmoid); ``score_bias`` then replaces the bias."""
    ws = disc.get_weights()
    own = {id(l) for l in disc._own_layers()}
    names = [(l.kind, n) for (l, n, _, _, _) in disc.store.entries if id(l) in own]
    ik = max(i for i, kn in enumerate(names) if kn == ("dense", "kernel"))
    ib = max(i for i, kn in enumerate(names) if kn == ("dense", "bias"))
    ws[ik] = (ws[ik] * score_scale).astype(np.float32)
    ws[ib] = (ws[ib] * score_scale if score_bias is None else np.full_like(ws[ib], score_bias)).astype(np.float32)
    disc.set_weights(ws)


def sn_critic_with_plain_head(arch="tiny"):
    """models.DCGANDiscriminator(arch, spectral_norm=True) with the Dense head left unwrapped.  W / sigma would undo any score scale,
    and the fully normalised tiny critic scores within +-0.5 at every seed (seeds 1-8, checked on a CPU): no score would reach a hinge."""
    from blurred_gan_amd import layers as L
    m = L.Sequential()
    for i, c in enumerate(models._D[arch]):
        kw = dict(input_shape=list(models.IMAGE_SHAPE[arch])) if i == 0 else {}
        m.add(L.SpectralNormalization(L.Conv2D(c, models.KSIZE.get(arch, 5), strides=2, padding="same", **kw)))
        m.add(L.LeakyReLU())
        m.add(L.Dropout(0.3))
    m.add(L.Flatten())
    m.add(L.Dense(1, activation="linear"))
    return m


def make_gan(arch, B, seed, objective=None, cls="wgangp", augment=None, critic_sn=False, down="stride", normalization=None, std=None, gbs=None,
             score_scale=None, score_bias=None, device=None, disc=None, **kw):
    """diffaug_reference.make_gan with ``objective=``, the model class (``wgangp`` / ``wgan``, blurred with ``std``) and the critic's
    score scale.  ``disc``: a callable that returns an unbuilt critic, in place of models.DCGANDiscriminator."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch)
    disc = disc() if disc is not None else models.DCGANDiscriminator(arch=arch, downsampling=down, normalization=normalization, spectral_norm=critic_sn)
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    LN.randomize(gen, rng), LN.randomize(disc, rng)
    if score_scale is not None:
        scale_scores(disc, score_scale, score_bias)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    base = {"wgangp": bg.WGANGP, "wgan": bg.WGAN}[cls]
    if std is None:
        gan = base(gen, disc, base.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, augment=augment, objective=objective, **kw)
    else:
        blurred = bg.BlurredVariant(base) if base is bg.WGAN else bg.BlurredWGANGP
        hp = blurred.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = blurred(gen, disc, hp, cfg, augment=augment, objective=objective, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = LN.draw(gan.discriminator, B, gen.latent_size, rng)
    if augment is not None:
        rnd = DR.draw_aug(rnd, B, seed)
    return gan, reals, rnd
