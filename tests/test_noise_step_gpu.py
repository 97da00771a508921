"""GPU tests of a generator with NoiseInjection layers (models.DCGANGenerator(normalization="pixel", noise=True), and a hand-built
stack with noise stages without PixelNormalization) through engine.Net and whole training steps, against the torch CPU float64
reference of tests/noise_reference.py (tests/ln_reference.py's walker with a ``noise`` branch, under tests/objective_reference.py's
step), with the noise maps injected and the strengths randomised (they start at zero).

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/test_layernorm_step_gpu.py).  Each
comparison first asserts, on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within KINK = 5e-6 of
zero, that no x-hat gradient norm is below MIN_NORM = 1e-3, and that no row of any PixelNormalization has mean(a^2) below
pixelnorm_reference.MIN_MS = 1e-4.  The seeds below were chosen so by running the reference alone on a CPU
(case(..., device="cpu")); the (kink, norm, min mean(a^2)) it gave stand beside them."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
from helpers import product_grads
from ln_reference import DT, KINK, assert_close, ref_params
import noise_reference as NR
import objective_reference as OR
import pixelnorm_reference as PR

pytestmark = pytest.mark.gpu

# name -> (arch, seed, generator keywords (or a callable that makes the generator), make_gan keywords).  The reference alone (float64,
# no GPU involved), seeds 1-5, as (min |LeakyReLU pre-activation|, min x-hat gradient norm, min mean(a^2) of a PixelNormalization row |
# the smallest |gradient| of a noise strength):
#   blur         (6.1e-05, 0.044, 1.2e-02 | 6e-03) (4.2e-05, 0.063, 1.1e-02 | 3e-03) (4.2e-05, 0.073, 1.2e-02 | 2e-02) (2.4e-06, 0.063, 6.7e-03 | 1e-03) (4.2e-07, 0.061, 7.7e-03 | 8e-03)
#   eqlr         (1.0e-05, 0.18, 1.2e-02 | 3e-03) (1.7e-05, 0.22, 9.4e-03 | 2e-03) (7.2e-06, 0.2, 8.7e-03 | 1e-02) (5.1e-05, 0.21, 1.2e-02 | 8e-03) (3.5e-05, 0.21, 1.6e-02 | 2e-02)
#   hand_built   (2.9e-05, 0.16, inf | 5e-03) (4.8e-05, 0.18, inf | 9e-03) (6.7e-07, 0.21, inf | 9e-04) (7.3e-06, 0.24, inf | 4e-04) (1.8e-05, 0.23, inf | 3e-03)
#   hinge        as plain (the same passes); no score within 0.69, 0.56, 0.58, 0.82, 0.55 of a hinge
#   plain        (1.7e-05, 0.17, 1.2e-02 | 7e-03) (2.3e-05, 0.19, 1.1e-02 | 3e-02) (5.0e-05, 0.22, 1.2e-02 | 2e-02) (2.4e-06, 0.22, 6.7e-03 | 5e-02) (4.2e-07, 0.2, 7.7e-03 | 1e-02)
#   plain_mnist  (7.9e-05, 0.36, 1.4e-03 | 2e-02) (1.8e-05, 0.22, 1.4e-03 | 6e-04) (4.8e-05, 0.22, 3.5e-03 | 1e-01) (2.7e-05, 0.18, 3.1e-03 | 7e-03) (1.9e-06, 0.22, 1.6e-03 | 4e-02)
#   resize       (3.0e-05, 0.16, 1.4e-02 | 1e-02) (1.0e-05, 0.2, 1.3e-02 | 9e-04) (5.7e-05, 0.23, 1.3e-02 | 5e-02) (6.9e-05, 0.21, 2.2e-02 | 1e-02) (2.3e-06, 0.2, 1.3e-02 | 1e-02)
VARIANTS = {
    "plain": ("tiny", 3, {}, {}),
    "plain_mnist": ("tiny_mnist", 1, {}, {}),
    "resize": ("tiny", 4, dict(upsampling="resize"), {}),
    "eqlr": ("tiny", 4, dict(equalized_lr=True), {}),
    "hinge": ("tiny", 3, {}, dict(objective="hinge")),
    "blur": ("tiny", 1, {}, dict(std=0.9)),
    "hand_built": ("tiny", 2, lambda: NR.hand_built_generator("tiny"), {}),
}


def case(name, device=None, seed=None, **kw):
    arch, s, gen_kw, mk = VARIANTS[name]
    gen = dict(gen=gen_kw) if callable(gen_kw) else dict(gen_kw=gen_kw)
    return NR.make_gan(arch, 4, s if seed is None else seed, gbs=5, device=device, **gen, **mk, **kw)


def reference(gan, reals, rnd):
    ref = NR.ref_step(gan.generator, gan.discriminator, reals, rnd, 5, gan.objective)
    NR.check_guards(ref)
    if ref["loss"] == "hinge":      # no score within the margin of its hinge: the seed's branch is the same in float32
        assert np.abs(ref["fs"] + 1).min() > OR.HINGE_MARGIN and np.abs(ref["rs"] - 1).min() > OR.HINGE_MARGIN, (ref["fs"], ref["rs"])
    return ref


def _strength_index(model):
    own = {id(l) for l in model._own_layers()}
    return [i for i, (l, n, _, _, tr) in enumerate([e for e in model.store.entries if e[4] and id(e[0]) in own]) if n == "noise_strength"]


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_step_gradients_match_torch(name):
    gan, reals, rnd = case(name)
    ref = reference(gan, reals, rnd)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals, randomness=rnd)
    G = gan.generator.net()
    ns = [st for st in G.stages if st.noise is not None]
    assert G.has_noise and len(ns) >= 2 and all((st.pn is None) == (name == "hand_built") for st in ns)
    assert_close(product_grads(gan.discriminator), ref["dgrads"], f"{name}: critic gradients")
    got = product_grads(gan.generator)
    assert_close(got, ref["ggrads"], f"{name}: generator gradients")
    idx = _strength_index(gan.generator)
    assert len(idx) == len(ns)
    for i in idx:       # the strengths' gradients on their own: a scalar each, and not a vanishing one
        print(f"{name}: d noise_strength {got[i][0]:+.6e}, reference {float(ref['ggrads'][i].ravel()[0]):+.6e}")
        assert abs(float(ref["ggrads"][i].ravel()[0])) > 1e-6
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), ref["fakes"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ net level
# (min |LeakyReLU pre-activation|, min mean(a^2)) of the reference, seeds 1-5:
#   tiny        (6.6e-05, 7.2e-03) (1.5e-04, 7.2e-03) (8.4e-06, 8.0e-03) (1.1e-05, 9.6e-03) (2.2e-05, 1.1e-02)
#   tiny_mnist  (3.0e-06, 3.0e-03) (4.2e-04, 2.2e-03) (1.8e-04, 2.5e-03) (4.3e-04, 3.0e-03) (2.7e-04, 2.1e-03)
#   hand_built  (2.0e-05, inf) (3.5e-06, inf) (5.8e-05, inf) (1.8e-06, inf) (2.3e-05, inf)      (no PixelNormalization)
NET_SEED = {"tiny": 2, "tiny_mnist": 2, "hand_built": 3}


def net_model(which, seed, B=4):
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = NR.hand_built_generator("tiny") if which == "hand_built" else models.DCGANGenerator(arch=which, normalization="pixel", noise=True)
    z = rng.uniform(size=(B, model.latent_size)).astype(np.float32)          # float32 values: product and reference see the same numbers
    return model, rng, z


def net_reference_pass(model, rng, z, training, device=None):
    if device is not None:
        model.build(device)
    NR.randomize(model, rng)
    B = z.shape[0]
    maps = rng.normal(size=(B, NR.noise_pixels(model))).astype(np.float32)
    dout = rng.normal(size=(B,) + model.output_shape[1:])
    W, train = ref_params(model)
    pre = []
    with PR.walker() as seen, NR.walker([maps]):
        y = NR.ref_forward(model, W, torch.as_tensor(z).to(DT), training, None, pre)
        grads = torch.autograd.grad((y * torch.as_tensor(dout)).sum(), train)
        min_ms = min(seen) if seen else float("inf")
    return maps, dout, y.detach().numpy(), [g.numpy() for g in grads], min(pre), min_ms


@pytest.mark.parametrize("which", ["tiny", "tiny_mnist", "hand_built"])
def test_net_forward_and_backward_match_torch(which):
    """The generator alone, injected noise: output and parameter gradients for a random dout; the same bits in inference with the
    same noise (a pixel-norm generator: nothing depends on the flag); noise=False equals strengths of 0; drawn noise differs from
    call to call and advances the network's counter."""
    B = 4
    model, rng, z = net_model(which, NET_SEED[which])
    maps, dout, y, grads, kink, min_ms = net_reference_pass(model, rng, z, True)
    assert kink > KINK and min_ms > PR.MIN_MS, (kink, min_ms)
    net = model.net()
    ctx = net.context(B, "test")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch.float32)
    got_y = net.forward(ctx, dev(z), training=True, noise=dev(maps)).cpu().numpy().copy()
    assert net.backward(ctx, dev(dout), need_dx=False, need_dw=True) is None
    assert_close([got_y], [y], f"{which} output")
    assert_close(product_grads(model), grads, f"{which} parameter gradients")
    if which != "hand_built":       # (the hand-built stack has a BatchNormalization: inference is another function)
        assert np.array_equal(net.forward(ctx, dev(z), training=False, noise=dev(maps)).cpu().numpy(), got_y)
    # noise=False: the same weights with the strengths set to 0
    off = net.forward(ctx, dev(z), training=False, noise=False).cpu().numpy().copy()
    ws = model.get_weights()
    own = {id(l) for l in model._own_layers()}
    names = [n for (l, n, _, _, _) in model.store.entries if id(l) in own]
    model.set_weights([np.zeros_like(w) if n == "noise_strength" else w for n, w in zip(names, ws)])
    zero = net.forward(ctx, dev(z), training=False, noise=dev(maps)).cpu().numpy().copy()
    assert np.array_equal(off, zero) and not np.array_equal(off, got_y)
    model.set_weights(ws)
    # drawn noise: two calls see different maps, the same seed and offset the same ones
    o0 = net.rng_offset
    a = net.forward(ctx, dev(z), training=False, seed=5).cpu().numpy().copy()
    o1 = net.rng_offset
    b = net.forward(ctx, dev(z), training=False, seed=5).cpu().numpy().copy()
    assert o1 - o0 == (B * net.noise_pixels + 3) // 4 == net.rng_offset - o1 and not np.array_equal(a, b)
    net.rng_offset = o0
    assert np.array_equal(net.forward(ctx, dev(z), training=False, seed=5).cpu().numpy(), a)
    # the drawn maps are the draw's restatement, stage by stage
    flat = ctx.noise_flat.cpu().numpy()
    np.testing.assert_allclose(flat, NR.np_normal(flat.size, 5, o0), rtol=0, atol=1e-5)


# ------------------------------------------------------------------ replay, successive steps, averaging, checkpoints
def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "s3", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
        assert ma.optimizer.iterations == mb.optimizer.iterations
        assert ma.net().rng_offset == mb.net().rng_offset
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _pair_member(replay, seed=21, B=4, gen_kw=None, strengths=0.5, **kw):
    bg.set_seed(seed)
    gen = models.DCGANGenerator(arch="tiny", **dict(dict(normalization="pixel", noise=True), **(gen_kw or {})))
    disc = models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, **kw)
    if strengths:       # they start at zero: the noise would not reach the output
        for st in gen.net().stages:
            if st.noise is not None:
                st.noise.vars["noise_strength"].fill_(strengths)
    return gan


def _batches(n, B=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(n)]


@pytest.mark.parametrize("latents", ["uniform", "normal"])
def test_replayed_steps_equal_eager_steps_bit_for_bit(latents):
    """The first step, the recorded one and replayed ones (the fourth call among them) against the unreplayed path on a second
    model from the same seed: the noise draws' offsets are bound to the generator network's counter, the latents' to the model's."""
    eager, prog = _pair_member(False, latent_distribution=latents), _pair_member(True, latent_distribution=latents)
    for i, reals in enumerate(_batches(4)):
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
        assert torch.equal(eager.images[0], prog.images[0]), i
    assert prog._programs.last_was_replay and prog._programs.stats["replayed"] >= 2, prog._programs.stats
    assert eager._programs.stats["replayed"] == 0
    G = prog.generator.net()
    assert G.rng_offset == 4 * 2 * ((4 * G.noise_pixels + 3) // 4)          # two generator forwards a step
    assert prog._rng_off > 0


def test_successive_steps_see_different_noise():
    for replay in (False, True):
        gan = _pair_member(replay)
        G = gan.generator.net()
        seen = []
        for reals in _batches(4):
            gan.train_on_batch(reals)
            seen.append(G.context(4, "g").noise_flat.clone())
            seen.append(G.context(4, "g_dstep").noise_flat.clone())
        for i in range(len(seen)):
            for j in range(i):
                assert not torch.equal(seen[i], seen[j]), (replay, i, j)
        st = NR.statistics(torch.cat(seen).cpu().numpy())
        assert abs(st["mean"]) < 0.1 and abs(st["var"] - 1) < 0.15, st          # 2688 values: 5 standard errors


def test_latent_distribution_normal_draws_normal_latents():
    gan = _pair_member(False, latent_distribution="normal")
    gan.batch_size = 4
    off = gan._rng_off
    z = gan.latents_batch().cpu().numpy().copy()
    want = NR.np_normal(z.size, gan._rng_seed, off).reshape(z.shape)
    np.testing.assert_allclose(z, want, rtol=0, atol=1e-5)
    assert gan._rng_off == off + (z.size + 3) // 4 and z.min() < 0
    u = _pair_member(False)
    u.batch_size = 4
    zu = u.latents_batch().cpu().numpy()
    assert zu.min() >= 0 and zu.max() < 1


def test_sampling_takes_the_three_noise_values_and_the_averaged_generator_averages_the_strengths():
    gan = _pair_member(True, generator_ema=0.5)
    z = torch.rand(5, 10, generator=torch.Generator().manual_seed(1)).cuda()
    strengths = lambda model: np.array([float(w[0]) for (l, n, _, _, _), w in zip(model.store.entries, model.get_weights()) if n == "noise_strength"],
                                       np.float32)
    avg = strengths(gan.generator_ema)
    assert np.array_equal(avg, np.zeros(3, np.float32))               # a bit-copy at construction: the strengths' initial zeros
    for k, reals in enumerate(_batches(2)):
        gan.train_on_batch(reals)
        live = strengths(gan.generator)
        w = np.float32(gan.generator_ema_config.w_at(k, 4, 1, 1))       # 1 - beta_k of the model's schedule, rounded once
        avg = avg - w * (avg - live)                                   # bg_ema_f32's line in float32
    E = gan.generator_ema.net()
    assert gan.generator_ema_updates == 2 and E.has_noise and E.noise_pixels == gan.generator.net().noise_pixels
    got_avg = strengths(gan.generator_ema)
    assert len(got_avg) == 3 and np.array_equal(got_avg, avg), (got_avg, avg)
    assert not np.any(got_avg == strengths(gan.generator)) and not np.any(got_avg == 0)         # between the start and the live values
    maps = torch.randn(5, E.noise_pixels, generator=torch.Generator().manual_seed(2))
    got = gan.generate_samples(z, ema=True, noise=maps).clone()
    bg.set_seed(99)
    fresh = models.DCGANGenerator(arch="tiny", normalization="pixel", noise=True)
    fresh.build()
    fresh.set_weights(gan.generator_ema.get_weights())
    fnet = fresh.net()
    assert torch.equal(got, fnet.forward(fnet.context(5, "t"), z, noise=maps.cuda()))
    assert not torch.equal(got, gan.generate_samples(z, noise=maps).clone())            # the live generator is elsewhere
    # False: without noise; None: fresh noise every call
    quiet = gan.generate_samples(z, ema=True, noise=False).clone()
    assert torch.equal(quiet, gan.generate_samples(z, ema=True, noise=False)) and not torch.equal(quiet, got)
    a = gan.generate_samples(z, ema=True).clone()
    assert not torch.equal(a, gan.generate_samples(z, ema=True)) and not torch.equal(a, quiet)


def test_checkpoint_resume_is_bit_identical_and_another_variable_list_is_refused(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    batches = _batches(4, seed=6)
    ref = _pair_member(True)
    for reals in batches[:2]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path / "noise")).save(2)
    for reals in batches[2:]:
        ref.train_on_batch(reals)
    resumed = _pair_member(True, seed=5)
    assert not torch.equal(resumed.generator.store.theta, ref.generator.store.theta)
    CheckpointManager(resumed, str(tmp_path / "noise")).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
        assert a.net().rng_offset == b.net().rng_offset
    # a model without the layers has another variable list: its generator takes no checkpoint of this one
    other = _pair_member(True, gen_kw=dict(noise=False), strengths=None)
    theta = other.generator.store.theta.clone()
    with pytest.raises(RuntimeError):          # the flat buffers differ in size: the copy into theta is refused
        CheckpointManager(other, str(tmp_path / "noise")).restore(path)
    assert torch.equal(other.generator.store.theta, theta)


# ------------------------------------------------------------------ refusals
def _critic_with_the_layer():
    return layers.Sequential([layers.Conv2D(16, 5, strides=2, padding="same", input_shape=[8, 8, 3]), layers.NoiseInjection(),
                              layers.LeakyReLU(), layers.Flatten(), layers.Dense(1)])


def test_a_critic_with_the_layer_is_refused():
    cfg = bg.TrainingConfig(log_dir="/tmp/bg_test_logs")
    for cls in (bg.WGAN, bg.WGANGP):
        with pytest.raises(NotImplementedError, match="NoiseInjection in the discriminator"):
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
        with pytest.raises(NotImplementedError, match="NoiseInjection in a critic under the gradient penalty is not built"):
            call()
