"""The reference of the adaptive-augmentation tests (a helper, not a test file), built on tests/diffaug_reference.py.

Gated decode: a row is twelve uniforms; u8 / u9 / u10 gate colour / translation / cutout, and an operation of the policy fires iff its
gate is below p, compared in float32.  A sample's transform is then diffaug_reference's for the policy ``policy & fired`` on the
row's first eight uniforms -- the numpy T / L^T and the differentiable torch T below do exactly that, sample by sample.

Controller: the rule of include/bgan.h "adaptive augmentation" in numpy float32, one operation per rounding.

Model level: objective_reference.ref_step_grads with every critic pass behind the gated T."""
import numpy as np
import torch

import blurred_gan_amd as bg
import diffaug_reference as DR
import ln_reference as LN
import objective_reference as OR
import sn_reference as SR
from diffaug_reference import OPS
from ln_reference import DT, ref_params
from oracle import torch_ref as TR

F32 = np.float32
HI = DR.HI
GATE_COLUMN = {"color": 8, "translation": 9, "cutout": 10}


# ---------------------------------------------------------------------------------------------------- decode
def policy_of(mask):
    return ",".join(name for name, bit in OPS.items() if mask & bit)


def fired_mask(u, p, cfg):
    """policy & fired of one row of twelve uniforms at probability p (float32 compare)."""
    return sum(bit for name, bit in OPS.items() if name in cfg.policy.split(",") and F32(u[GATE_COLUMN[name]]) < F32(p))


def sample_cfg(u, p, cfg):
    """The DiffAugment one sample goes through: the policy's operations that fired, the policy's ratios."""
    return bg.DiffAugment(policy_of(fired_mask(u, p, cfg)), cfg.translation_ratio, cfg.cutout_ratio)


def decode(u, p, H, W, cfg):
    """diffaug_reference.decode of the fired operations, plus ``fired``."""
    return dict(DR.decode(u[:8], H, W, sample_cfg(u, p, cfg)), fired=fired_mask(u, p, cfg))


def with_gates(params8, masks):
    """[n, 12] float32: ``params8`` with gate columns that make sample i fire exactly ``masks[i]`` at any p in (0, 1): 0 fires, HI not."""
    params8 = np.asarray(params8, F32)
    out = np.zeros((params8.shape[0], 12), F32)
    out[:, :8] = params8
    for i, m in enumerate(masks):
        for name, bit in OPS.items():
            out[i, GATE_COLUMN[name]] = 0.0 if m & bit else HI
    out[:, 11] = 0.5
    return out


# ---------------------------------------------------------------------------------------------------- numpy, any dtype
def np_T(x, params, p, cfg, linear=False, dtype=np.float64):
    x = np.asarray(x, dtype)
    return np.concatenate([DR.np_T(x[k:k + 1], params[k:k + 1, :8], sample_cfg(params[k], p, cfg), linear=linear, dtype=dtype)
                           for k in range(x.shape[0])])


def np_LT(g, params, p, cfg, dtype=np.float64):
    g = np.asarray(g, dtype)
    return np.concatenate([DR.np_LT(g[k:k + 1], params[k:k + 1, :8], sample_cfg(params[k], p, cfg), dtype=dtype) for k in range(g.shape[0])])


# ---------------------------------------------------------------------------------------------------- the controller
def sign_stats(scores):
    """(sum of sign, count): sign(0) = sign(NaN) = 0."""
    s = np.asarray(scores, F32)
    return F32(np.sum(s > 0) - np.sum(s < 0)), F32(s.size)


class Controller:
    """state = {p, acc_sign, acc_count, k, r_last}; step(scores) is one bg_ada_stats_f32 + bg_ada_update_f32."""

    def __init__(self, p, target, interval, speed_images):
        self.p, self.acc_sign, self.acc_count, self.k, self.r_last = F32(p), F32(0), F32(0), F32(0), F32(0)
        self.target, self.interval, self.inv = F32(target), int(interval), F32(1.0 / speed_images)

    def step(self, scores):
        s, c = sign_stats(scores)
        return self.update(s, c)

    def update(self, s, c):
        self.acc_sign, self.acc_count, self.k = F32(self.acc_sign + s), F32(self.acc_count + c), F32(self.k + F32(1))
        if self.k == F32(self.interval):
            r = F32(self.acc_sign / self.acc_count)
            d = F32(1) if r > self.target else (F32(-1) if r < self.target else F32(0))
            step = F32(F32(d * self.acc_count) * self.inv)
            self.p = F32(min(max(F32(self.p + step), F32(0)), F32(1)))
            self.r_last = r
            self.acc_sign = self.acc_count = self.k = F32(0)
        return self.state()

    def state(self):
        return np.array([self.p, self.acc_sign, self.acc_count, self.k, self.r_last, 0, 0, 0], F32)


# ---------------------------------------------------------------------------------------------------- torch, differentiable
def torch_T(x, params, p, cfg):
    return torch.cat([DR.torch_T(x[k:k + 1], params[k:k + 1, :8], sample_cfg(params[k], p, cfg)) for k in range(x.shape[0])])


def critic_forward(disc, W, x, training, masks, pre, cfg, params, p):
    """diffaug_reference.critic_forward with the gated T."""
    tail = DR._BehindTheBlur(disc)
    if tail.blur is not None:
        x = TR.blur(x, float(tail.blur.std))
    return LN.ref_forward(tail, W, torch_T(x, params, p, cfg), training, masks, pre)


def ref_step_grads(gen, disc, reals, rnd, gbs, objective, augment, p, penalty_step=True, gp_coef=10.0, e_drift=1e-4):
    """objective_reference.ref_step_grads (the WGANGP class) with per-sample masks: rnd["aug_*"] are [B, 12], ``p`` the probability
    of every pass of the step.  Returns its dict; ``rs`` are the real scores the controller's statistics are taken of."""
    obj = bg.objective.as_objective(objective)
    T = lambda a: torch.as_tensor(np.asarray(a)).to(DT)
    Wg, tg = ref_params(gen)
    Wd, td = ref_params(disc)
    pre = []
    reals, B = T(reals), reals.shape[0]
    Ed, info_d = SR.effective(disc, Wd, iterate=True)
    Eg, _ = SR.effective(gen, Wg, iterate=False)
    with torch.no_grad():
        fakes = LN.ref_forward(gen, Eg, T(rnd["z_d"]), False, pre=pre)
    fs = critic_forward(disc, Ed, fakes, True, rnd["mask_fake"], pre, augment, rnd["aug_fake"], p)
    rs = critic_forward(disc, Ed, reals, True, rnd["mask_real"], pre, augment, rnd["aug_real"], p)
    loss = OR.critic_loss(obj.loss, fs, rs) / gbs
    gp_term, min_norm = torch.zeros((), dtype=DT), float("inf")
    if penalty_step:
        alpha = T(rnd["alpha"]) if obj.penalty_alpha is None else torch.full((B,), obj.penalty_alpha, dtype=DT)
        xhat = (reals + alpha.view(B, 1, 1, 1) * (fakes - reals)).detach().requires_grad_(True)
        yhat = critic_forward(disc, Ed, xhat, False, None, pre, augment, rnd["aug_hat"], p)
        g, = torch.autograd.grad(yhat.sum(), xhat, create_graph=True)
        norms = g.reshape(B, -1).norm(dim=1)
        gp_term = gp_coef * obj.penalty_interval * ((norms - obj.penalty_target) ** 2).mean()
        min_norm = float(norms.detach().min())
    loss_vec = loss + gp_term + e_drift * (fs.abs().view(B) + rs.abs().view(B))
    signal = []
    dgrads = SR._grads_and_signal(loss_vec.sum(), td, disc, Wd, info_d, signal)
    Eg, info_g = SR.effective(gen, Wg, iterate=True)
    Ed, _ = SR.effective(disc, Wd, iterate=False)
    fk = LN.ref_forward(gen, Eg, T(rnd["z_g"]), True, pre=pre)
    sc = critic_forward(disc, Ed, fk, False, None, pre, augment, rnd["aug_g"], p)
    gloss = OR.generator_loss(obj.loss, sc) / gbs
    ggrads = SR._grads_and_signal(gloss, tg, gen, Wg, info_g, signal)
    return dict(dgrads=dgrads, ggrads=ggrads, fakes=fakes.numpy(), kink=min(pre), norm=min_norm, signal=min(signal) if signal else float("inf"),
                fs=fs.detach().numpy().ravel(), rs=rs.detach().numpy().ravel(), loss=obj.loss)


def add_gates(rnd, B, seed):
    """Widens the four [B, 8] param blocks of a step to [B, 12]: seeded gates behind diffaug_reference.draw_aug's columns."""
    rng = np.random.default_rng(seed + 3000)
    for key in ("aug_fake", "aug_real", "aug_hat", "aug_g"):
        gates = np.minimum(rng.uniform(size=(B, 4)).astype(F32), F32(HI))
        rnd[key] = np.concatenate([rnd[key], gates], axis=1)
    return rnd


def make_gan(arch, B, seed, augment, objective=None, **kw):
    """objective_reference.make_gan (tiny models and batches, as the DiffAugment step tests use them) with an AdaptiveAugment and
    [B, 12] injected draws (``augment`` None: no augmentation draws at all)."""
    gan, reals, rnd = OR.make_gan(arch, B, seed, objective=objective, augment=augment, **kw)
    return gan, reals, (rnd if augment is None else add_gates(rnd, B, seed))
