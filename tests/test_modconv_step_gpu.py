"""GPU tests of a generator with StyleModulation stages (models.DCGANGenerator(normalization="style"), and a hand-built stack that
mixes modulated and plain stages) through engine.Net and whole training steps, against the torch CPU float64 reference of
tests/modconv_reference.py (tests/ln_reference.py's walker with a modulation branch, under tests/objective_reference.py's step), with
the style variables randomised (the initial style_bias of ones makes s nearly constant) and the noise maps injected.

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/test_noise_step_gpu.py); images rtol
1e-4, atol 1e-5.  Each comparison first asserts, on the reference alone: no LeakyReLU pre-activation within KINK = 5e-6 of zero, no
x-hat gradient norm below MIN_NORM = 1e-3, no PixelNormalization row with mean(a^2) below 1e-4, no demodulation sum q below
MIN_Q = 1e-4, and no style gradient tensor with max |value| below 1e-6.  The seeds below were chosen so by running the reference
alone on a CPU (case(..., device="cpu")); the values it gave stand beside them."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
from helpers import product_grads
from ln_reference import DT, KINK, assert_close, ref_params
import ln_reference as LN
import modconv_reference as MC
import objective_reference as OR
import pixelnorm_reference as PR

pytestmark = pytest.mark.gpu

# name -> (arch, seed, generator keywords (or a callable that makes the generator), make_gan keywords).  The reference alone (float64,
# no GPU involved), seeds 1-5, as (min |LeakyReLU pre-activation|, min x-hat gradient norm, min mean(a^2) | min q, min max|style
# gradient|):
#   blur         (3.1e-06, 0.066, 9.5e-03 | 8.0e-01, 4e-04) (5.3e-06, 0.068, 1.5e-02 | 9.3e-01, 3e-04) (4.5e-06, 0.052, 1.1e-02 | 1.2e+00, 3e-04) (1.2e-05, 0.065, 2.0e-02 | 1.1e+00, 5e-04) (7.6e-06, 0.052, 1.2e-02 | 1.5e+00, 3e-04)
#   eqlr         (2.0e-06, 0.23, 6.7e-02 | 1.3e+00, 1e-03) (1.5e-05, 0.19, 6.6e-02 | 1.7e+00, 5e-04) (4.9e-06, 0.21, 1.6e-01 | 1.9e+00, 1e-03) (3.0e-06, 0.19, 1.5e-01 | 1.9e+00, 1e-03) (1.6e-05, 0.21, 1.5e-01 | 2.2e+00, 9e-04)
#   filtered     (9.1e-07, 0.18, 9.5e-03 | 7.8e-01, 1e-03) (1.9e-06, 0.21, 1.5e-02 | 9.4e-01, 1e-03) (1.4e-05, 0.18, 1.1e-02 | 1.2e+00, 3e-03) (3.2e-06, 0.21, 2.0e-02 | 1.1e+00, 2e-03) (3.3e-07, 0.2, 1.2e-02 | 1.5e+00, 2e-03)
#   hinge        as plain but the style gradients (6e-04, 8e-04, 1e-03, 2e-03, 9e-04); no score within 0.38, 0.72, 0.51, 0.61, 0.73 of a hinge
#   mixed        (5.3e-05, 0.18, 1.6e-02 | 1.1e+00, 1e-03) (1.4e-05, 0.19, 1.5e-02 | 1.4e+00, 1e-03) (3.9e-05, 0.25, 1.6e-02 | 1.9e+00, 2e-03) (1.5e-05, 0.2, 1.3e-02 | 1.1e+00, 8e-04) (4.0e-06, 0.23, 7.8e-03 | 1.3e+00, 2e-03)
#   noise        (1.5e-05, 0.2, 9.7e-03 | 1.0e+00, 1e-03) (2.2e-06, 0.19, 1.2e-02 | 1.1e+00, 8e-04) (1.4e-05, 0.19, 8.7e-03 | 1.2e+00, 6e-04) (1.8e-05, 0.22, 1.5e-02 | 9.6e-01, 9e-04) (2.7e-05, 0.2, 1.0e-02 | 1.7e+00, 8e-04)
#   noise_mnist  (6.9e-06, 0.16, 8.5e-04 | 6.3e-01, 3e-03) (1.5e-04, 0.33, 1.1e-03 | 7.7e-01, 1e-02) (6.1e-05, 0.24, 4.9e-03 | 9.9e-01, 2e-03) (7.4e-05, 0.29, 2.4e-03 | 1.2e+00, 5e-03) (6.3e-05, 0.21, 1.9e-03 | 9.5e-01, 3e-03)
#   plain        (3.1e-06, 0.18, 9.5e-03 | 8.0e-01, 6e-04) (5.3e-06, 0.21, 1.5e-02 | 9.3e-01, 8e-04) (4.5e-06, 0.17, 1.1e-02 | 1.2e+00, 1e-03) (1.2e-05, 0.21, 2.0e-02 | 1.1e+00, 2e-03) (7.6e-06, 0.19, 1.2e-02 | 1.5e+00, 9e-04)
#   plain_mnist  (2.9e-05, 0.18, 1.4e-03 | 6.7e-01, 2e-03) (1.2e-04, 0.25, 1.5e-03 | 9.8e-01, 1e-02) (1.6e-05, 0.22, 6.9e-03 | 8.1e-01, 4e-03) (4.4e-05, 0.3, 3.3e-03 | 1.1e+00, 8e-03) (1.7e-05, 0.21, 3.9e-03 | 1.1e+00, 2e-03)
#   resize       (2.0e-05, 0.17, 9.5e-03 | 7.8e-01, 4e-03) (4.3e-05, 0.21, 1.5e-02 | 9.4e-01, 3e-03) (1.3e-05, 0.18, 1.1e-02 | 1.2e+00, 5e-03) (1.1e-05, 0.21, 2.0e-02 | 1.1e+00, 3e-03) (2.2e-07, 0.19, 1.2e-02 | 1.5e+00, 4e-03)
VARIANTS = {
    "plain": ("tiny", 4, {}, {}),
    "plain_mnist": ("tiny_mnist", 2, {}, {}),
    "noise": ("tiny", 5, dict(noise=True), {}),
    "noise_mnist": ("tiny_mnist", 2, dict(noise=True), {}),
    "eqlr": ("tiny", 5, dict(equalized_lr=True), {}),
    "resize": ("tiny", 2, dict(upsampling="resize"), {}),
    "filtered": ("tiny", 3, dict(upsampling="filtered"), {}),
    "hinge": ("tiny", 4, {}, dict(objective="hinge")),
    "blur": ("tiny", 4, {}, dict(std=0.9)),
    "mixed": ("tiny", 1, lambda: MC.mixed_generator("tiny"), {}),
}


def case(name, device=None, seed=None, **kw):
    arch, s, gen_kw, mk = VARIANTS[name]
    gen = dict(gen=gen_kw) if callable(gen_kw) else dict(gen_kw=gen_kw)
    return MC.make_gan(arch, 4, s if seed is None else seed, gbs=5, device=device, **gen, **mk, **kw)


def reference(gan, reals, rnd):
    ref = MC.ref_step(gan.generator, gan.discriminator, reals, rnd, 5, gan.objective)
    MC.check_guards(ref)
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
    assert G.has_mod and len(G.mod_layers) >= 3
    assert_close(product_grads(gan.discriminator), ref["dgrads"], f"{name}: critic gradients")
    got = product_grads(gan.generator)
    assert_close(got, ref["ggrads"], f"{name}: generator gradients")
    idx = MC.style_index(gan.generator)
    assert len(idx) == 2 * len(G.mod_layers)
    for i in idx:
        print(f"{name}: style gradient {i}: max |got| {np.abs(got[i]).max():.3e}, max |reference| {np.abs(ref['ggrads'][i]).max():.3e}")
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), ref["fakes"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ net level
# (min |LeakyReLU pre-activation|, min mean(a^2), min q, min max|style gradient|) of the reference, seeds 1-5:
#   tiny        (1.5e-05, 1.0e-02, 1.2e+00, 4e-01) (7.2e-06, 1.7e-02, 9.2e-01, 2e-01) (4.4e-05, 1.6e-02, 1.5e+00, 2e-01) (6.2e-05, 3.3e-02, 1.4e+00, 4e-01) (2.2e-05, 1.4e-02, 1.3e+00, 1e-01)
#   tiny_mnist  (9.2e-04, 4.1e-03, 8.2e-01, 3e-01) (2.5e-04, 4.7e-03, 7.6e-01, 1e+00) (1.8e-04, 2.5e-03, 1.5e+00, 3e-01) (7.7e-05, 1.1e-02, 2.4e+00, 6e-01) (6.9e-04, 4.4e-03, 1.4e+00, 5e-01)
#   mixed       (1.3e-05, 1.0e-02, 1.2e+00, 3e-01) (1.4e-05, 1.7e-02, 9.2e-01, 3e-01) (1.3e-04, 1.6e-02, 1.7e+00, 2e-01) (4.0e-05, 3.3e-02, 1.4e+00, 3e-01) (2.2e-05, 1.4e-02, 1.3e+00, 2e-01)
NET_SEED = {"tiny": 4, "tiny_mnist": 1, "mixed": 3}


def net_model(which, seed, B=4):
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = MC.mixed_generator("tiny") if which == "mixed" else models.DCGANGenerator(arch=which, normalization="style")
    z = rng.uniform(size=(B, model.latent_size)).astype(np.float32)          # float32 values: product and reference see the same numbers
    return model, rng, z


def net_reference_pass(model, rng, z, training, device=None):
    if device is not None:
        model.build(device)
    MC.randomize(model, rng)
    B = z.shape[0]
    P = MC.noise_pixels(model)
    maps = rng.normal(size=(B, P)).astype(np.float32) if P else None
    dout = rng.normal(size=(B,) + model.output_shape[1:])
    W, train = ref_params(model)
    pre = []
    with PR.walker() as seen, MC.walker([maps] if P else []) as qs:
        y = LN.ref_forward(model, W, torch.as_tensor(z).to(DT), training, None, pre)
        grads = [g.numpy() for g in torch.autograd.grad((y * torch.as_tensor(dout)).sum(), train)]
        min_ms, min_q = min(seen), min(qs)
    min_style = min(float(np.abs(grads[i]).max()) for i in MC.style_index(model))
    return maps, dout, y.detach().numpy(), grads, (min(pre), min_ms, min_q, min_style)


@pytest.mark.parametrize("which", ["tiny", "tiny_mnist", "mixed"])
def test_net_forward_and_backward_match_torch(which):
    """The generator alone: output and parameter gradients for a random dout in training; the same bits in inference (nothing in a
    style generator depends on the flag); the gradient at the input is refused."""
    B = 4
    model, rng, z = net_model(which, NET_SEED[which])
    maps, dout, y, grads, (kink, min_ms, min_q, min_style) = net_reference_pass(model, rng, z, True)
    assert kink > KINK and min_ms > PR.MIN_MS and min_q > MC.MIN_Q and min_style > MC.MIN_STYLE_GRAD, (kink, min_ms, min_q, min_style)
    net = model.net()
    ctx = net.context(B, "test")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch.float32)
    nz = dict(noise=dev(maps)) if maps is not None else {}
    got_y = net.forward(ctx, dev(z), training=True, **nz).cpu().numpy().copy()
    assert net.backward(ctx, dev(dout), need_dx=False, need_dw=True) is None
    net.eqlr_scale_gradients()          # the step's: dL/dW = c * dL/dW_eff of the equalised layer of the mixed stack
    assert_close([got_y], [y], f"{which} output")
    assert_close(product_grads(model), grads, f"{which} parameter gradients")
    assert np.array_equal(net.forward(ctx, dev(z), training=False, **nz).cpu().numpy(), got_y)
    with pytest.raises(NotImplementedError, match="dL/dw"):
        net.backward(ctx, dev(dout), need_dx=True)
    # accumulation: beta = 1 on top of the gradients just taken doubles them (the demodulation term of dW rides on the pass's scale)
    net.forward(ctx, dev(z), training=True, **nz)
    net.backward(ctx, dev(dout), need_dx=False, need_dw=True)
    first = [g.copy() for g in product_grads(model)]
    net.backward(ctx, dev(dout), need_dx=False, need_dw=True, beta=1.0, scale=1.0)
    for a, b in zip(product_grads(model), first):
        np.testing.assert_allclose(a, 2 * b, rtol=1e-5, atol=1e-6 * max(float(np.abs(b).max()), 1e-6))


# ------------------------------------------------------------------ replay, averaging, checkpoints, sampling
def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "s3", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
        assert ma.optimizer.iterations == mb.optimizer.iterations
        assert ma.net().rng_offset == mb.net().rng_offset
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _style_values(model):
    return np.concatenate([w.ravel() for (l, n, _, _, _), w in zip(model.store.entries, model.get_weights()) if n.startswith("style_")])


def _pair_member(replay, seed=21, B=4, gen_kw=None, **kw):
    bg.set_seed(seed)
    gen = models.DCGANGenerator(arch="tiny", **dict(dict(normalization="style", noise=True), **(gen_kw or {})))
    disc = models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, **kw)
    for st in gen.net().stages:       # the strengths start at zero: the noise would not reach the output
        if st.noise is not None:
            st.noise.vars["noise_strength"].fill_(0.5)
    return gan


def _batches(n, B=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(n)]


@pytest.mark.parametrize("gen_kw", [{}, dict(equalized_lr=True, upsampling="filtered")], ids=["plain", "eqlr_filtered"])
def test_replayed_steps_equal_eager_steps_bit_for_bit(gen_kw):
    eager, prog = _pair_member(False, gen_kw=gen_kw), _pair_member(True, gen_kw=gen_kw)
    start = _style_values(prog.generator).copy()
    for i, reals in enumerate(_batches(4)):
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
        assert torch.equal(eager.images[0], prog.images[0]), i
    assert prog._programs.last_was_replay and prog._programs.stats["replayed"] >= 2, prog._programs.stats
    assert eager._programs.stats["replayed"] == 0
    now = _style_values(prog.generator)
    assert np.isfinite(now).all() and (now != start).mean() > 0.9          # the style variables train


def test_the_averaged_generator_averages_the_style_variables_and_sampling_works():
    gan = _pair_member(True, generator_ema=0.5)
    z = torch.rand(5, 10, generator=torch.Generator().manual_seed(1)).cuda()
    avg = _style_values(gan.generator_ema)
    assert np.array_equal(avg, _style_values(gan.generator))               # a bit-copy at construction
    for k, reals in enumerate(_batches(2)):
        gan.train_on_batch(reals)
        live = _style_values(gan.generator)
        w = np.float32(gan.generator_ema_config.w_at(k, 4, 1, 1))       # 1 - beta_k of the model's schedule, rounded once
        avg = avg - w * (avg - live)                                   # bg_ema_f32's line in float32
    E = gan.generator_ema.net()
    assert gan.generator_ema_updates == 2 and E.has_mod and len(E.mod_layers) == 4
    got = _style_values(gan.generator_ema)
    assert np.array_equal(got, avg) and (got != _style_values(gan.generator)).mean() > 0.9
    maps = torch.randn(5, E.noise_pixels, generator=torch.Generator().manual_seed(2))
    out = gan.generate_samples(z, ema=True, noise=maps).clone()
    bg.set_seed(99)
    fresh = models.DCGANGenerator(arch="tiny", normalization="style", noise=True)
    fresh.build()
    fresh.set_weights(gan.generator_ema.get_weights())
    fnet = fresh.net()
    assert torch.equal(out, fnet.forward(fnet.context(5, "t"), z, noise=maps.cuda()))
    live = gan.generate_samples(z, noise=maps).clone()
    assert tuple(live.shape) == (5, 8, 8, 3) and torch.isfinite(live).all() and float(live.abs().max()) <= 1.0 and not torch.equal(out, live)
    assert torch.equal(live, gan.generate_samples(z, training=True, noise=maps))


def test_checkpoint_resume_is_bit_identical_and_another_variable_list_is_refused(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    batches = _batches(4, seed=6)
    ref = _pair_member(True)
    for reals in batches[:2]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path / "mod")).save(2)
    for reals in batches[2:]:
        ref.train_on_batch(reals)
    resumed = _pair_member(True, seed=5)
    assert not torch.equal(resumed.generator.store.theta, ref.generator.store.theta)
    CheckpointManager(resumed, str(tmp_path / "mod")).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
        assert a.net().rng_offset == b.net().rng_offset
    # a pixel-norm generator has another variable list: it takes no checkpoint of this one
    other = _pair_member(True, gen_kw=dict(normalization="pixel"))
    theta = other.generator.store.theta.clone()
    with pytest.raises(RuntimeError):          # the flat buffers differ in size: the copy into theta is refused
        CheckpointManager(other, str(tmp_path / "mod")).restore(path)
    assert torch.equal(other.generator.store.theta, theta)
