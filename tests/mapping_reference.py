"""References of the mapping-network tests (layers.MappingNetwork, csrc/mapping.hip).

1. The three formulas of include/bgan.h "mapping network" in numpy, in the dtype they are handed (float64: the reference; on small
   integers every intermediate is exact in float32 as well, so the same functions give the expected bits of the exact tests).
2. A torch float64 walk of a generator with a mapping prefix: the prefix written out here, the synthesis network by
   modconv_reference's walk (imported, not edited), and the guards of ln_reference / modconv_reference with one more: the smallest
   |pre-activation| of the mapping layers (a LeakyReLU kink there flips a branch between float32 and float64)."""
import contextlib

import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
import firsample_reference as FS
import ln_reference as LN
import mbstd_reference as MB
import modconv_reference as MC
import pixelnorm_reference as PR
from ln_reference import ATOL, DT, KINK, RTOL, assert_close  # noqa: F401  (re-exported: the step tests name them through this module)

MIN_STYLE_GRAD, MIN_Q = MC.MIN_STYLE_GRAD, MC.MIN_Q


# ------------------------------------------------------------------ kernel formulas
def np_dense_lrelu(x, W, bias, c=1.0, bias_mul=1.0, alpha=1.0):
    v = c * (x @ W)
    if bias is not None:
        v = v + bias_mul * bias
    return np.where(v > 0, v, alpha * v)


def np_lrelu_bias_bwd(g, y, alpha, old=None, beta=0.0, scale=1.0):
    gp = g * np.where(y > 0, 1.0, alpha).astype(g.dtype)
    db = scale * gp.sum(axis=0)
    if beta != 0.0:
        db = db + beta * old
    return gp, db


def np_truncate(w, w_avg, psi):
    return w_avg[None, :] + psi * (w - w_avg[None, :])


def np_w_avg_update(w_avg, w_batch, beta, global_batch):
    """One G-step's update in float32, one operation per rounding: mean = sum_b w / global batch as bg_colsum_f32 scales its sum,
    then bg_ema_f32's avg -= (1 - beta) * (avg - mean)."""
    mean = (np.float32(1.0 / global_batch) * w_batch.astype(np.float64).sum(axis=0).astype(np.float32)).astype(np.float32)
    wgt = np.float32(1.0 - beta)
    return (w_avg - (wgt * (w_avg - mean).astype(np.float32)).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------ the model walk (torch float64)
def mapping_layer(model):
    from blurred_gan_amd import layers
    return next((l for l, _ in model.flat_layers() if isinstance(l, layers.MappingNetwork)), None)


def torch_mapping(mp, z, params=None):
    """(w, hs, min |pre-activation|) of the prefix ``mp`` on z [B, L] (torch float64); ``params``: {name: tensor} in place of the
    layer's own variables (leaves of an autograd graph)."""
    h, hs, kink = z, [], np.inf
    for l in range(mp.num_layers):
        k = params[f"kernel_{l}"] if params else torch.from_numpy(mp.vars[f"kernel_{l}"].detach().cpu().numpy().astype(np.float64))
        b = params[f"bias_{l}"] if params else torch.from_numpy(mp.vars[f"bias_{l}"].detach().cpu().numpy().astype(np.float64))
        pre = mp.coefficients[l] * (h @ k) + mp.bias_multiplier * b
        kink = min(kink, float(pre.detach().abs().min()))
        h = torch.where(pre > 0, pre, mp.alpha * pre)
        hs.append(h)
    return h, hs, kink


def manual_mapping_backward(mp, z, hs, dw, params):
    """The backward csrc/mapping.hip + bg_gemm_f32 run, written out: returns ({name: gradient}, dL/dz)."""
    grads, g = {}, dw
    for l in range(mp.num_layers - 1, -1, -1):
        hin = z if l == 0 else hs[l - 1]
        gp = g * torch.where(hs[l] > 0, torch.ones_like(g), torch.full_like(g, mp.alpha))
        grads[f"bias_{l}"] = mp.bias_multiplier * gp.sum(0)
        grads[f"kernel_{l}"] = mp.coefficients[l] * (hin.T @ gp)
        g = mp.coefficients[l] * (gp @ params[f"kernel_{l}"].T)
    return grads, g


# ------------------------------------------------------------------ the walker: the prefix in front of modconv_reference's branch
_inner = []
MAP_KINK_SEEN = []      # min |pre-activation| of the mapping layers of every forward since the last walker() began


def split_prefix(flat):
    """(index of the mapping layer or None) of a flattened layer list: first, or second behind a PixelNormalization."""
    for i, (l, _) in enumerate(flat[:2]):
        if isinstance(l, layers.MappingNetwork) and (i == 0 or flat[0][0].kind == "pixelnorm"):
            return i
    return None


def ref_forward(model, W, x, training, masks=None, pre=None):
    flat = model.flat_layers()
    i = split_prefix(flat)
    if i is None:
        return _inner[-1](model, W, x, training, masks, pre)
    if i == 1:
        x = PR.torch_pixelnorm(x, flat[0][0].epsilon)
    mp = flat[i][0]
    w, _, kink = torch_mapping(mp, x, {n: W[(id(mp), n)] for n in mp.vars if n != "w_avg"})
    MAP_KINK_SEEN.append(kink)
    return _inner[-1](MC._Part(flat[i + 1:]), W, w, training, masks, pre)      # behind the prefix w is the input AND the style source


@contextlib.contextmanager
def walker():
    """Enter it LAST, behind modconv_reference.walker: it cuts the prefix off and hands the rest, with w as its input, to that one."""
    del MAP_KINK_SEEN[:]
    _inner.append(LN.ref_forward)
    LN.ref_forward = ref_forward
    try:
        yield MAP_KINK_SEEN
    finally:
        LN.ref_forward = _inner.pop()


def ref_step(gen, disc, reals, rnd, gbs, objective=None):
    """modconv_reference.ref_step for a generator with a mapping prefix, plus ``map_kink``."""
    import objective_reference as OR
    maps = [rnd["noise_d"], rnd["noise_g"]] if "noise_d" in rnd else []
    with MB.walker(), FS.walker(), PR.walker() as seen, MC.walker(maps) as qs, walker() as kinks:
        ref = OR.ref_step_grads(gen, disc, reals, rnd, gbs, objective)
        ref["min_ms"] = min(seen) if seen else float("inf")
        ref["min_s"] = float("inf")
        ref["min_q"] = min(qs)
        ref["map_kink"] = min(kinks)
    ref["min_style"] = min(float(np.abs(ref["ggrads"][i]).max()) for i in MC.style_index(gen))
    return ref


def check_guards(ref):
    MC.check_guards(ref)
    assert ref["map_kink"] > KINK, ref["map_kink"]


def randomize(model, rng):
    """modconv_reference.randomize; the prefix's biases drawn from N(0, 1) / m (they start at zero; m * bias is then N(0, 1) * 0.1)."""
    MC.randomize(model, rng)
    mp = mapping_layer(model)
    if mp is not None:
        for l in range(mp.num_layers):
            b = mp.vars[f"bias_{l}"]
            b.copy_(torch.from_numpy((rng.normal(size=tuple(b.shape)) * 0.1 / mp.bias_multiplier).astype(np.float32)))
        model.store.tr_dirty = True


def make_gan(arch, B, seed, gen_kw, gbs=None, device=None, std=None, **kw):
    """modconv_reference.make_gan with a mapping prefix in the generator (``gen_kw`` carries mapping_layers, ...)."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch, **dict(dict(normalization="style"), **gen_kw))
    disc = models.DCGANDiscriminator(arch=arch)
    if device is not None:
        gen.build(device), disc.build(device)
    randomize(gen, rng), LN.randomize(disc, rng)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B), cfg, **kw)
    else:
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = bg.BlurredWGANGP(gen, disc, hp, cfg, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = LN.draw(gan.discriminator, B, gen.latent_size, rng)
    P = MC.noise_pixels(gen)
    if P:
        rnd = dict(rnd, noise_d=rng.normal(size=(B, P)).astype(np.float32), noise_g=rng.normal(size=(B, P)).astype(np.float32))
    return gan, reals, rnd


def net_reference_pass(model, rng, z, need_dz, device=None):
    """The generator alone in torch float64: (maps, dout, y, parameter gradients, dL/dz or None, guards) for a random dout.  guards =
    (min |LeakyReLU pre-activation|, min mean(a^2), min q, min max |style gradient|, min |mapping pre-activation|)."""
    if device is not None:
        model.build(device)
    randomize(model, rng)
    B = z.shape[0]
    P = MC.noise_pixels(model)
    maps = rng.normal(size=(B, P)).astype(np.float32) if P else None
    dout = rng.normal(size=(B,) + model.output_shape[1:])
    W, train = LN.ref_params(model)
    pre = []
    zt = torch.as_tensor(z).to(DT).requires_grad_(bool(need_dz))
    with FS.walker(), PR.walker() as seen, MC.walker([maps] if P else []) as qs, walker() as kinks:      # FS: the equalised-learning-rate coefficients
        y = LN.ref_forward(model, W, zt, True, None, pre)
        grads = torch.autograd.grad((y * torch.as_tensor(dout)).sum(), train + ([zt] if need_dz else []))
        guards = (min(pre), min(seen) if seen else float("inf"), min(qs), None, min(kinks))
    grads = [g.numpy() for g in grads]
    dz = grads.pop() if need_dz else None
    min_style = min(float(np.abs(grads[i]).max()) for i in MC.style_index(model))
    return maps, dout, y.detach().numpy(), grads, dz, guards[:3] + (min_style, guards[4])


def check_net_guards(guards):
    kink, min_ms, min_q, min_style, map_kink = guards
    assert kink > KINK and min_ms > PR.MIN_MS and min_q > MIN_Q and min_style > MIN_STYLE_GRAD and map_kink > KINK, guards
