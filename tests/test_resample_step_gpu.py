"""GPU tests of networks with resampling stages (layers.UpSampling2D / AveragePooling2D; models.DCGANGenerator(upsampling="resize"),
models.DCGANDiscriminator(downsampling="pool")) through engine.Net and whole training steps.

The reference is written here, in torch CPU float64 with autograd: it walks the product model's own layer list, takes the
weights the product holds (Keras layout) and the step's injected randomness, and differentiates the loss of
oracle/step.py: discriminator_grads (gradients of the SUM of the [B] loss vector; the penalty through
autograd.grad(create_graph=True)).  Tolerance of every gradient comparison: tests/test_step_gpu.py:
test_gradients_match_oracle's small-batch one, per tensor rtol 2e-3, atol 2e-4 * max|reference|.  Each comparison also asserts,
on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within 5e-6 of zero (the gradient is
discontinuous there and float32 may legitimately sit on the other branch); the seeds below were chosen so."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blurred_gan_amd as bg
from blurred_gan_amd import models
from helpers import product_grads, rel_l2
from oracle import torch_ref as TR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-3, 2e-4
KINK = 5e-6
DT = torch.float64


# ------------------------------------------------------------------ the torch float64 reference
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
    """(critic gradients, generator gradients, fakes of the D-step, min |LeakyReLU pre-activation| over all passes)."""
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
    gp = ((g.reshape(B, -1).norm(dim=1) - 1.0) ** 2).mean()
    loss_vec = (fs - rs).sum() / gbs + gp_coef * gp + e_drift * (fs.abs().view(B) + rs.abs().view(B))
    dgrads = torch.autograd.grad(loss_vec.sum(), td)
    fk = ref_forward(gen, Wg, T(rnd["z_g"]), True, pre=pre)
    sc = ref_forward(disc, Wd, fk, False, pre=pre)
    ggrads = torch.autograd.grad(-sc.sum() / gbs, tg)
    return [t.numpy() for t in dgrads], [t.numpy() for t in ggrads], fakes.numpy(), min(pre)


def assert_close(got, want, what):
    assert len(got) == len(want) and len(got) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        b = np.asarray(b).reshape(a.shape)
        scale = max(float(np.abs(b).max()), 1e-6)
        err = float(np.abs(a - b).max())
        print(f"[{what}] tensor {i} {a.shape}: max|err| {err:.2e}, max|ref| {scale:.2e}, rel-L2 {rel_l2(a, b):.1e}")
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL * scale, err_msg=f"{what} tensor {i}")


# ------------------------------------------------------------------ models, weights, randomness
def randomize(model, rng):
    """Glorot kernels as built; non-trivial biases and BatchNorm parameters / statistics."""
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


def make_gan(arch, B, seed, up="resize", down="pool", std=None, gbs=None, device=None, **kw):
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    gen = models.DCGANGenerator(arch=arch, upsampling=up)
    disc = models.DCGANDiscriminator(arch=arch, downsampling=down)
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


# ------------------------------------------------------------------ 1. net level
NET_SEED = 2        # min |LeakyReLU pre-activation| of the reference: 2.3e-5 / 3.2e-4 (tiny critic / generator), 3.7e-5 / 2.0e-4 (tiny_mnist)


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist"])
@pytest.mark.parametrize("which", ["critic", "generator"])
def test_net_forward_and_backward_match_torch(arch, which):
    """One pooled critic with injected Dropout masks / one resize generator with BatchNorm in training mode: output, parameter
    gradients and input gradient for a random dout."""
    B = 4
    seed = NET_SEED
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    if which == "critic":
        model = models.DCGANDiscriminator(arch=arch, downsampling="pool")
        x = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch])
    else:
        model = models.DCGANGenerator(arch=arch, upsampling="resize")
        x = rng.uniform(size=(B, model.latent_size))
    randomize(model, rng)
    masks = [(rng.uniform(size=(B,) + tuple(s)) >= 0.3).astype(np.uint8) for l, s in model.flat_layers() if l.kind == "dropout"]
    dout = rng.normal(size=(B,) + model.output_shape[1:])
    # reference
    W, train = ref_params(model)
    xt = torch.as_tensor(x).to(DT).requires_grad_(True)
    pre = []
    y = ref_forward(model, W, xt, True, masks, pre)
    grads = torch.autograd.grad((y * torch.as_tensor(dout)).sum(), train + [xt])
    assert min(pre) > KINK, min(pre)
    # product
    net = model.net()
    assert any(st.kind in ("upsample", "avgpool") for st in net.stages)
    ctx = net.context(B, "test")
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    out = net.forward(ctx, dev(x), training=True, masks=[dev(m, torch.uint8) for m in masks] or None)
    got_y = out.cpu().numpy().copy()
    din = net.backward(ctx, dev(dout), need_dx=True, need_dw=True)
    assert_close([got_y], [y.detach().numpy()], f"{arch} {which} output")
    assert_close(product_grads(model), [g.numpy() for g in grads[:-1]], f"{arch} {which} parameter gradients")
    assert_close([din.cpu().numpy().reshape(x.shape)], [grads[-1].numpy()], f"{arch} {which} input gradient")


# ------------------------------------------------------------------ 2. whole steps
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
# seeds by the reference's min |LeakyReLU pre-activation| over all passes of the step (float64, no GPU involved): seeds 1-6 gave
# 2.7e-6, 3.0e-5, 3.6e-6, 8.2e-6, 2.7e-5, 8.5e-6 for the resize + pool pair; the other cases likewise
STEP_SEED = {"plain": 2, "blur": 2, ("transpose", "pool"): 3, ("resize", "stride"): 5}      # 3.0e-5, 1.0e-5, 1.7e-5, 8.0e-5


def _step_case(arch, B, seed, kw, **variant):
    gan, reals, rnd = make_gan(arch, B, seed, gbs=B + 1, **variant, **kw)
    dg, gg, fakes, kink = ref_step_grads(gan.generator, gan.discriminator, reals, rnd, gbs=B + 1)
    assert kink > KINK, kink
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals.astype(np.float32), randomness=rnd)
    assert_close(product_grads(gan.discriminator), dg, "critic gradients")
    assert_close(product_grads(gan.generator), gg, "generator gradients")
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), fakes, rtol=1e-4, atol=1e-5)
    return gan


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_step_gradients_match_torch_in_every_d_step_configuration(config):
    gan = _step_case("tiny", 4, STEP_SEED["plain"], CONFIGS[config])
    assert [st.kind for st in gan.discriminator.net().stages] == ["conv", "avgpool", "conv", "avgpool", "dense"]
    assert [st.kind for st in gan.generator.net().stages].count("upsample") == 2


def test_step_gradients_match_torch_behind_the_blur():
    gan = _step_case("tiny", 4, STEP_SEED["blur"], {}, std=0.9)
    assert gan.discriminator.net().blur is not None


@pytest.mark.parametrize("up,down", [("transpose", "pool"), ("resize", "stride")])
def test_step_gradients_match_torch_for_mixed_pairs(up, down):
    _step_case("tiny", 4, STEP_SEED[(up, down)], {}, up=up, down=down)


# ------------------------------------------------------------------ 3. the three D-step configurations agree
def test_d_step_configurations_give_the_same_critic_gradients():
    """The relation (and tolerance) of test_step_gpu.py: test_merged_penalty_filter_gradients_equal_the_separate_launches."""
    ref = None
    for name in ("merged", "merged_separate_wgrad", "unmerged"):
        gan, reals, rnd = make_gan("tiny", 5, 4, std=1.0, **CONFIGS[name])
        gan.discriminator.optimizer.learning_rate = 0.0
        gan.generator.optimizer.learning_rate = 0.0
        gan.train_on_batch(reals.astype(np.float32), randomness=rnd)
        grads = product_grads(gan.discriminator)
        if ref is None:
            ref = grads
            continue
        for a, b in zip(grads, ref):
            assert rel_l2(a, b) < 2e-6 or not np.any(b), (name, a.shape, rel_l2(a, b))


# ------------------------------------------------------------------ 4. replay
def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "s3", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
        assert ma.optimizer.iterations == mb.optimizer.iterations
        assert ma.net().rng_offset == mb.net().rng_offset
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _mnist_pair_member(replay, seed=21, B=4, **kw):
    bg.set_seed(seed)
    gen = models.DCGANGenerator(arch="mnist", upsampling="resize")
    disc = models.DCGANDiscriminator(arch="mnist", downsampling="pool")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, **kw)


def test_replayed_steps_equal_eager_steps_bit_for_bit():
    B = 4
    eager, prog = _mnist_pair_member(False), _mnist_pair_member(True)
    g = torch.Generator().manual_seed(3)
    for i in range(8):
        reals = (torch.rand(B, 28, 28, 1, generator=g) * 2 - 1).cuda()
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
    assert prog._programs.stats["replayed"] >= 6, prog._programs.stats


# ------------------------------------------------------------------ 5. weight averaging and checkpoints
def test_averaged_twin_of_a_resize_generator_samples():
    gan = _mnist_pair_member(True, generator_ema=0.9)
    kinds = lambda m: [(st.kind, st.in_shape, st.out_shape, st.act, st.bn is not None) for st in m.net().stages]
    assert kinds(gan.generator_ema) == kinds(gan.generator) and ("upsample", (7, 7, 128), (14, 14, 128), None, False) in kinds(gan.generator)
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        gan.train_on_batch((torch.rand(4, 28, 28, 1, generator=g) * 2 - 1).cuda())
    assert gan.generator_ema_updates == 2
    z = torch.rand(3, gan.latent_size, generator=g)
    avg, live = gan.generate_samples(z, ema=True), gan.generate_samples(z)
    assert tuple(avg.shape) == tuple(live.shape) == (3, 28, 28, 1)
    assert bool(torch.isfinite(avg).all()) and not torch.equal(avg, live)
    # the averaged weights through the live structure give the averaged samples: the twin runs the same stages
    twin = models.DCGANGenerator(arch="mnist", upsampling="resize")
    twin.build()
    twin.set_weights(gan.generator_ema.get_weights())
    assert torch.equal(twin(z.cuda()), avg)


def test_checkpoint_resume_is_bit_identical(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand(4, 28, 28, 1, generator=g) * 2 - 1).cuda() for _ in range(4)]
    ref = _mnist_pair_member(True)
    for reals in batches[:2]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path)).save(2)
    for reals in batches[2:]:
        ref.train_on_batch(reals)
    resumed = _mnist_pair_member(True, seed=5)
    assert not torch.equal(resumed.generator.store.theta, ref.generator.store.theta)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
