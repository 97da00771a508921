"""GPU tests of a generator with PixelNormalization (models.DCGANGenerator(normalization="pixel")) through engine.Net and whole
training steps, against the torch CPU float64 reference of tests/pixelnorm_reference.py (tests/ln_reference.py's walker with a
``pixelnorm`` branch, under tests/objective_reference.py's step).

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/test_layernorm_step_gpu.py).  Each
comparison first asserts, on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within KINK = 5e-6
of zero, that no x-hat gradient norm is below MIN_NORM = 1e-3, and that no row of any PixelNormalization has mean(a^2) below
pixelnorm_reference.MIN_MS = 1e-4 (epsilon is then negligible and r <= 100).  The seeds below were chosen so by running the
reference alone on a CPU (case(..., device="cpu")); the (kink, norm, min mean(a^2)) it gave stand beside them."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
from helpers import product_grads
from ln_reference import DT, KINK, assert_close, randomize, ref_params
import objective_reference as OR
import pixelnorm_reference as PR

pytestmark = pytest.mark.gpu

# name -> (arch, seed, generator keywords, critic keywords, make_gan keywords).  The reference alone (float64, no GPU involved),
# seeds 1-5, as (min |LeakyReLU pre-activation|, min x-hat gradient norm, min mean(a^2) of a PixelNormalization row):
#   plain         (4.5e-05, 0.18, 7.7e-03) (4.7e-05, 0.17, 9.5e-03) (8.1e-06, 0.23, 5.6e-03) (4.4e-05, 0.21, 9.5e-03) (1.5e-05, 0.19, 1.1e-02)
#   plain_mnist   (4.0e-05, 0.31, 6.1e-04) (1.4e-05, 0.24, 9.5e-04) (1.3e-06, 0.21, 2.4e-03) (4.2e-05, 0.21, 1.6e-03) (2.0e-04, 0.19, 1.8e-03)
#   latents       (7.4e-06, 0.19, 9.0e-03) (1.9e-05, 0.18, 8.7e-03) (1.8e-05, 0.22, 5.4e-03) (8.7e-07, 0.2, 1.1e-02) (3.3e-05, 0.19, 1.3e-02)
#   latents_mnist (4.3e-05, 0.32, 7.6e-04) (1.4e-05, 0.24, 1.8e-03) (2.2e-05, 0.22, 1.5e-03) (4.5e-05, 0.21, 1.8e-03) (2.2e-04, 0.19, 1.1e-05)
#   resize        (5.5e-05, 0.19, 8.1e-03) (6.0e-05, 0.19, 1.6e-02) (8.1e-06, 0.23, 1.1e-02) (1.0e-05, 0.2, 1.4e-02) (1.6e-05, 0.19, 1.1e-02)
#   spectral      (4.0e-05, 0.17, 4.8e-03) (2.1e-05, 0.18, 9.0e-03) (1.1e-04, 0.2, 1.0e-02) (5.2e-06, 0.2, 1.4e-02) (2.0e-05, 0.17, 6.8e-03)
#   critic        (1.5e-05, 1.4, 1.0e-02) (3.5e-05, 2.2, 7.6e-03) (2.2e-05, 2.1, 4.4e-03) (3.3e-05, 1.9, 1.1e-02) (5.9e-05, 1.5, 7.4e-03)
#                 (its MinibatchStdDev's min s of the x-hat pass: 1.1e-03 1.3e-03 6.8e-04 3.6e-04 1.5e-03; mbstd_reference.MIN_S holds too)
#   hinge         as plain (the same passes); no score within 0.48 of a hinge
#   blur          (3.1e-05, 0.051, 7.7e-03) (5.3e-05, 0.067, 9.5e-03) (8.1e-06, 0.066, 5.6e-03) (4.5e-05, 0.068, 9.5e-03) (4.6e-06, 0.057, 1.1e-02)
VARIANTS = {
    "plain": ("tiny", 1, {}, {}, {}),
    "plain_mnist": ("tiny_mnist", 1, {}, {}, {}),
    "latents": ("tiny", 5, dict(normalize_latents=True), {}, {}),
    "latents_mnist": ("tiny_mnist", 1, dict(normalize_latents=True), {}, {}),
    "resize": ("tiny", 1, dict(upsampling="resize"), {}, {}),
    "spectral": ("tiny", 1, dict(spectral_norm=True), {}, {}),
    "critic": ("tiny", 2, {}, dict(normalization="layer", minibatch_stddev=2), {}),
    "hinge": ("tiny", 1, {}, {}, dict(objective="hinge")),
    "blur": ("tiny", 1, {}, {}, dict(std=0.9)),
}


def case(name, device=None, seed=None, **kw):
    arch, s, gen_kw, disc_kw, mk = VARIANTS[name]
    return PR.make_gan(arch, 4, s if seed is None else seed, gen_kw=gen_kw, disc_kw=disc_kw, gbs=5, device=device, **mk, **kw)


def reference(gan, reals, rnd):
    ref = PR.ref_step(gan.generator, gan.discriminator, reals, rnd, 5, gan.objective)
    PR.check_guards(ref)
    if ref["loss"] == "hinge":      # no score within the margin of its hinge: the seed's branch is the same in float32
        assert np.abs(ref["fs"] + 1).min() > OR.HINGE_MARGIN and np.abs(ref["rs"] - 1).min() > OR.HINGE_MARGIN, (ref["fs"], ref["rs"])
    return ref


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_step_gradients_match_torch(name):
    gan, reals, rnd = case(name)
    ref = reference(gan, reals, rnd)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals, randomness=rnd)
    G = gan.generator.net()
    assert G.has_pn and sum(st.pn is not None for st in G.stages) >= 3 and (G.latent_pn is not None) == name.startswith("latents")
    assert_close(product_grads(gan.discriminator), ref["dgrads"], f"{name}: critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], f"{name}: generator gradients")
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), ref["fakes"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ net level
# (min |LeakyReLU pre-activation|, min mean(a^2)) of the reference, seeds 1-5:
#   tiny        (7.5e-05, 8.4e-03) (1.7e-04, 1.3e-02) (5.2e-05, 9.7e-03) (9.7e-05, 1.8e-02) (2.2e-05, 1.4e-02)
#     + latents (9.3e-06, 8.5e-03) (1.6e-04, 1.2e-02) (1.6e-04, 1.0e-02) (2.2e-06, 1.9e-02) (2.0e-05, 1.9e-02)
#   tiny_mnist  (1.7e-04, 2.8e-03) (1.1e-04, 2.9e-03) (1.8e-04, 2.5e-03) (2.5e-04, 2.4e-03) (1.8e-04, 1.5e-03)
#     + latents (6.2e-05, 1.6e-03) (2.4e-04, 6.2e-03) (7.7e-05, 3.4e-03) (9.8e-04, 1.7e-03) (1.4e-05, 9.7e-04)
NET_SEED = {"tiny": 2, "tiny_mnist": 4}


def net_reference(arch, seed, B=4, **gen_kw):
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = models.DCGANGenerator(arch=arch, normalization="pixel", **gen_kw)
    z = rng.uniform(size=(B, model.latent_size)).astype(np.float32)          # float32 values: product and reference see the same numbers
    return model, rng, z


def net_reference_pass(model, rng, z, training):
    randomize(model, rng)
    dout = rng.normal(size=(z.shape[0],) + model.output_shape[1:])
    W, train = ref_params(model)
    pre = []
    with PR.walker() as seen:
        y = PR.ref_forward(model, W, torch.as_tensor(z).to(DT), training, None, pre)
        grads = torch.autograd.grad((y * torch.as_tensor(dout)).sum(), train)
        min_ms = min(seen)
    return dout, y.detach().numpy(), [g.numpy() for g in grads], min(pre), min_ms


@pytest.mark.parametrize("latents", [False, True])
@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist"])
def test_net_forward_and_backward_match_torch(arch, latents):
    """The generator alone: output and parameter gradients for a random dout; the same output in inference."""
    B = 4
    model, rng, z = net_reference(arch, NET_SEED[arch], normalize_latents=latents)
    dout, y, grads, kink, min_ms = net_reference_pass(model, rng, z, True)
    assert kink > KINK and min_ms > PR.MIN_MS, (kink, min_ms)
    net = model.net()
    assert [st.pn is not None for st in net.stages] == [True] * (len(net.stages) - 1) + [False] and (net.latent_pn is not None) == latents
    ctx = net.context(B, "test")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch.float32)
    got_y = net.forward(ctx, dev(z), training=True).cpu().numpy().copy()
    assert net.backward(ctx, dev(dout), need_dx=False, need_dw=True) is None
    assert_close([got_y], [y], f"{arch} output")
    assert_close(product_grads(model), grads, f"{arch} parameter gradients")
    assert np.array_equal(net.forward(ctx, dev(z), training=False).cpu().numpy(), got_y)        # nothing depends on the flag
    if latents:
        with pytest.raises(NotImplementedError, match="no backward"):
            net.backward(ctx, dev(dout), need_dx=True)


# ------------------------------------------------------------------ replay, averaging, checkpoints
def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "s3", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
        assert ma.optimizer.iterations == mb.optimizer.iterations
        assert ma.net().rng_offset == mb.net().rng_offset
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _pair_member(replay, seed=21, B=4, **kw):
    bg.set_seed(seed)
    gen = models.DCGANGenerator(arch="tiny", normalization="pixel", normalize_latents=True)
    disc = models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, **kw)


def _batches(n, B=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(n)]


@pytest.mark.parametrize("conv_math", ["fp32", "bf16x6"])
def test_replayed_steps_equal_eager_steps_bit_for_bit(conv_math):
    """The first step, the recorded one and replayed ones (the fourth call among them) against the unreplayed path on a second
    model from the same seed."""
    eager, prog = _pair_member(False, conv_math=conv_math), _pair_member(True, conv_math=conv_math)
    for i, reals in enumerate(_batches(4)):
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
    assert prog._programs.last_was_replay and prog._programs.stats["replayed"] >= 2, prog._programs.stats
    assert eager._programs.stats["replayed"] == 0


def test_sampling_from_the_averaged_generator():
    gan = _pair_member(True, generator_ema=0.5)
    z = torch.rand(5, 10, generator=torch.Generator().manual_seed(1)).cuda()
    for reals in _batches(2):
        gan.train_on_batch(reals)
    assert gan.generator_ema_updates == 2 and gan.generator_ema.net().has_pn and gan.generator_ema.net().latent_pn is not None
    got = gan.generate_samples(z, ema=True).clone()
    bg.set_seed(99)
    fresh = models.DCGANGenerator(arch="tiny", normalization="pixel", normalize_latents=True)
    fresh.build()
    fresh.set_weights(gan.generator_ema.get_weights())
    assert torch.equal(got, fresh(z))
    assert not torch.equal(got, gan.generate_samples(z).clone())            # the live generator is elsewhere
    assert not gan.generator_ema.store.n_state                               # no statistics to average


def test_checkpoint_resume_is_bit_identical(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    batches = _batches(4, seed=6)
    ref = _pair_member(True)
    for reals in batches[:2]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path / "pn")).save(2)
    for reals in batches[2:]:
        ref.train_on_batch(reals)
    resumed = _pair_member(True, seed=5)
    assert not torch.equal(resumed.generator.store.theta, ref.generator.store.theta)
    CheckpointManager(resumed, str(tmp_path / "pn")).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)


# ------------------------------------------------------------------ refusals
def _critic_with_the_layer():
    return layers.Sequential([layers.Conv2D(16, 5, strides=2, padding="same", input_shape=[8, 8, 3]), layers.LeakyReLU(),
                              layers.PixelNormalization(), layers.Flatten(), layers.Dense(1)])


def test_a_critic_with_the_layer_is_refused():
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    for cls in (bg.WGAN, bg.WGANGP):
        with pytest.raises(NotImplementedError, match="PixelNormalization in the discriminator"):
            cls(models.DCGANGenerator(arch="tiny"), _critic_with_the_layer(), cls.HyperParameters(batch_size=4, global_batch_size=4), cfg)
    # the engine itself: first-order passes run, the penalty's second order raises
    m = _critic_with_the_layer()
    m.build()
    net = m.net()
    ctx = net.context(4, "test")
    x = torch.rand(4, 8, 8, 3, generator=torch.Generator().manual_seed(1)).cuda()
    net.forward(ctx, x, training=False)
    din = net.backward(ctx, torch.ones(4, 1, device="cuda"), need_dx=True, need_dw=True)
    assert din is not None and torch.isfinite(din).all()
    for call in (lambda: net.gp_second_order(ctx, din), lambda: net.gp_second_order_merged(ctx, 0, 4)):
        with pytest.raises(NotImplementedError, match="PixelNormalization in a critic under the gradient penalty is not built"):
            call()
