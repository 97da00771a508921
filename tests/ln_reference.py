"""The torch CPU float64 reference of the LayerNormalization tests (a helper, not a test file).

It is the reference of tests/test_resample_step_gpu.py -- it walks the product model's own layer list with the weights the
product holds (Keras layout) and the step's injected randomness, and differentiates the loss of oracle/step.py: discriminator_grads
(gradients of the SUM of the [B] loss vector; the penalty through autograd.grad(create_graph=True)) -- with a ``layernorm``
branch (F.layer_norm over the last axis with the layer's epsilon) and the critic's ``normalization=`` argument.  Besides the
smallest |LeakyReLU pre-activation| of all passes it reports the smallest x-hat gradient norm: the penalty divides by it."""
import numpy as np
import torch
import torch.nn.functional as F

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
from helpers import rel_l2
from oracle import torch_ref as TR

RTOL, ATOL = 2e-3, 2e-4
KINK = 5e-6             # no LeakyReLU pre-activation of the reference may lie this close to zero
MIN_NORM = 1e-3         # no x-hat gradient norm of the reference may be smaller
DT = torch.float64


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def ref_params(model):
    """[(layer id, name, float64 leaf)] in the model's variable order + the trainable ones among them."""
    own = {id(l) for l in model._own_layers()}
    W, train = {}, []
    for (l, n, _, _, tr) in model.store.entries:
        if id(l) not in own:
            continue
        t = l.vars[n].detach().cpu().to(DT).clone()
        if tr:
            t.requires_grad_(True)
            train.append(t)
        W[(id(l), n)] = t
    return W, train


def ref_forward(model, W, x, training, masks=None, pre=None):
    """The layer list of ``model`` in torch.  ``pre``: a list that collects min |LeakyReLU pre-activation| of the pass."""
    mi = 0
    B = x.shape[0]
    for l, s in model.flat_layers():
        k = l.kind
        w = lambda n: W[(id(l), n)]
        if k == "blur":
            x = TR.blur(x, float(l.std))
        elif k == "dense":
            x = x @ w("kernel")
            if l.use_bias:
                x = x + w("bias")
        elif k in ("conv", "convT"):
            if k == "conv" and l.stride == 1:
                x = _nhwc(F.conv2d(_nchw(x).contiguous(), w("kernel").permute(3, 2, 0, 1).contiguous(), padding=l.k // 2))
            elif k == "conv":
                x = TR.conv2d(x, w("kernel"), l.stride)
            else:
                x = TR.conv2d_transpose(x, w("kernel"), l.stride)
            if l.use_bias:
                x = x + w("bias")
            if l.activation == "tanh":
                x = torch.tanh(x)
        elif k == "bn":
            if training:
                ax = tuple(range(x.ndim - 1))
                mean = x.mean(ax)
                var = ((x - mean) ** 2).mean(ax)
            else:
                mean, var = w("moving_mean"), w("moving_variance")
            x = w("gamma") * (x - mean) / torch.sqrt(var + l.epsilon) + w("beta")
        elif k == "layernorm":
            x = F.layer_norm(x, x.shape[-1:], w("gamma"), w("beta"), l.epsilon)
        elif k == "lrelu":
            if pre is not None:
                pre.append(float(x.detach().abs().min()))
            x = F.leaky_relu(x, l.alpha)
        elif k == "dropout":
            if training:
                x = x * (1.0 / (1.0 - l.rate)) * torch.as_tensor(np.asarray(masks[mi])).to(DT)
            mi += 1
        elif k == "upsample":
            x = _nhwc(F.interpolate(_nchw(x), scale_factor=2, mode="nearest"))
        elif k == "avgpool":
            x = _nhwc(F.avg_pool2d(_nchw(x), 2))
        elif k == "reshape":
            x = x.reshape((B,) + tuple(l.target_shape))
        elif k == "flatten":
            x = x.reshape(B, -1)
        else:
            raise AssertionError(k)
    return x


def ref_step_grads(gen, disc, reals, rnd, gbs, gp_coef=10.0, e_drift=1e-4):
    """(critic gradients, generator gradients, fakes of the D-step, min |LeakyReLU pre-activation| over all passes, min x-hat
    gradient norm)."""
    T = lambda a: torch.as_tensor(np.asarray(a)).to(DT)
    Wg, tg = ref_params(gen)
    Wd, td = ref_params(disc)
    pre = []
    reals, B = T(reals), reals.shape[0]
    with torch.no_grad():
        fakes = ref_forward(gen, Wg, T(rnd["z_d"]), False, pre=pre)
    fs = ref_forward(disc, Wd, fakes, True, rnd["mask_fake"], pre)
    rs = ref_forward(disc, Wd, reals, True, rnd["mask_real"], pre)
    xhat = (reals + T(rnd["alpha"]).view(B, 1, 1, 1) * (fakes - reals)).detach().requires_grad_(True)
    yhat = ref_forward(disc, Wd, xhat, False, pre=pre)
    g, = torch.autograd.grad(yhat.sum(), xhat, create_graph=True)
    norms = g.reshape(B, -1).norm(dim=1)
    gp = ((norms - 1.0) ** 2).mean()
    loss_vec = (fs - rs).sum() / gbs + gp_coef * gp + e_drift * (fs.abs().view(B) + rs.abs().view(B))
    dgrads = torch.autograd.grad(loss_vec.sum(), td)
    fk = ref_forward(gen, Wg, T(rnd["z_g"]), True, pre=pre)
    sc = ref_forward(disc, Wd, fk, False, pre=pre)
    ggrads = torch.autograd.grad(-sc.sum() / gbs, tg)
    return [t.numpy() for t in dgrads], [t.numpy() for t in ggrads], fakes.numpy(), min(pre), float(norms.detach().min())


def assert_close(got, want, what):
    assert len(got) == len(want) and len(got) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        b = np.asarray(b).reshape(a.shape)
        scale = max(float(np.abs(b).max()), 1e-6)
        err = float(np.abs(a - b).max())
        print(f"[{what}] tensor {i} {a.shape}: max|err| {err:.2e}, max|ref| {scale:.2e}, rel-L2 {rel_l2(a, b):.1e}")
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL * scale, err_msg=f"{what} tensor {i}")


def randomize(model, rng):
    """Glorot kernels as built; non-trivial biases and normalisation parameters / statistics."""
    model.build()
    own = {id(l) for l in model._own_layers()}
    out = []
    for (l, n, _, shape, _), w in zip([e for e in model.store.entries if id(e[0]) in own], model.get_weights()):
        if n in ("bias", "beta", "moving_mean"):
            w = rng.normal(size=shape) * 0.1
        elif n in ("gamma", "moving_variance"):
            w = 1 + 0.2 * rng.uniform(size=shape)
        out.append(np.asarray(w, np.float32))
    model.set_weights(out)


def draw(disc, B, latent, rng):
    shp = [(B,) + tuple(s) for l, s in disc.flat_layers() if l.kind == "dropout"]
    mk = lambda: [(rng.uniform(size=s) >= 0.3).astype(np.uint8) for s in shp]
    u = lambda *sh: rng.uniform(size=sh).astype(np.float32)           # float32 values: product and reference see the same numbers
    return dict(z_d=u(B, latent), z_g=u(B, latent), alpha=u(B), mask_fake=mk(), mask_real=mk())


def make_gan(arch, B, seed, up="transpose", down="stride", normalization="layer", std=None, gbs=None, device=None, disc=None, **kw):
    """``disc``: a ready (unbuilt) critic for ``arch``'s images, or a callable that returns one (tests/ln_critics.py), in place of
    models.DCGANDiscriminator(arch, down, normalization); it is made after the seed is set and the generator exists, as that one is."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch, upsampling=up)
    if disc is None:
        disc = models.DCGANDiscriminator(arch=arch, downsampling=down, normalization=normalization)
    elif callable(disc) and not isinstance(disc, layers.Sequential):
        disc = disc()
    if device is not None:              # reference-only use (seed selection on a host without a GPU)
        gen.build(device), disc.build(device)
    randomize(gen, rng), randomize(disc, rng)
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    if std is None:
        hp = bg.WGANGP.HyperParameters(global_batch_size=gbs or B, batch_size=B)
        gan = bg.WGANGP(gen, disc, hp, cfg, **kw)
    else:
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=std, global_batch_size=gbs or B, batch_size=B)
        gan = bg.BlurredWGANGP(gen, disc, hp, cfg, **kw)
    reals = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch]).astype(np.float32)
    rnd = draw(gan.discriminator, B, gen.latent_size, rng)
    return gan, reals, rnd
