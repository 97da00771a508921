"""GPU tests of a generator with a MappingNetwork prefix (models.DCGANGenerator(normalization="style", mapping_layers=N)) through
engine.Net and whole training steps, against the torch CPU float64 reference of tests/mapping_reference.py (the prefix written out
in front of tests/modconv_reference.py's walker), B = 4.

Tolerance of every gradient comparison: ln_reference.assert_close, per tensor rtol 2e-3, atol 2e-4 * max|reference|; images rtol
1e-4, atol 1e-5.  Each comparison first asserts, on the reference alone, the guards of tests/test_modconv_step_gpu.py and one more:
no pre-activation of a mapping layer within KINK = 5e-6 of zero.  The seeds were chosen so by running the reference alone on a CPU
(case(..., device="cpu") / net_case(..., device="cpu")); the values it gave stand beside them."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models, ops
from helpers import product_grads
import mapping_reference as R

pytestmark = pytest.mark.gpu

B = 4
# name -> (arch, seed, generator keywords).  units once L (None) and once another size that is no multiple of 4; one and two layers;
# with and without equalized_lr, noise and normalize_latents on either architecture.
# The reference alone, as (min |LeakyReLU pre-activation|, min x-hat norm, min mean(a^2), min q, min max|style gradient|, min |mapping
# pre-activation|):
#   tiny_2       seed 8: (9.2e-06, 0.24, 6.6e-03, 1.1e+00, 2e-03, 1.4e-03)   (seeds 1-7 and 9 give a kink of 4.7e-07 ... 6.7e-06)
#   tiny_eq      seed 3: (5.1e-05, 0.16, 5.6e-01, 2.9e+00, 4e-04, 4.4e-02)
#   mnist_eq     seed 3: (2.2e-05, 0.13, 5.0e-03, 2.8e+00, 1e-03, 1.3e-02)
#   mnist_1      seed 2: (7.9e-05, 0.25, 1.9e-03, 1.3e+00, 5e-03, 2.6e-03)
VARIANTS = {
    "tiny_2": ("tiny", 8, dict(mapping_layers=2, mapping_lr_multiplier=1.0)),
    "tiny_eq": ("tiny", 3, dict(mapping_layers=1, mapping_units=7, equalized_lr=True, noise=True, normalize_latents=True)),
    "mnist_eq": ("tiny_mnist", 3, dict(mapping_layers=2, mapping_units=5, equalized_lr=True)),
    "mnist_1": ("tiny_mnist", 2, dict(mapping_layers=1, mapping_lr_multiplier=1.0, noise=True, normalize_latents=True)),
}


def case(name, device=None, seed=None, **kw):
    arch, s, gen_kw = VARIANTS[name]
    return R.make_gan(arch, B, s if seed is None else seed, gen_kw, gbs=5, device=device, **kw)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch.float32)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_step_gradients_match_torch(name):
    gan, reals, rnd = case(name)
    ref = R.ref_step(gan.generator, gan.discriminator, reals, rnd, 5, gan.objective)
    R.check_guards(ref)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals, randomness=rnd)
    G = gan.generator.net()
    assert G.has_mapping and G.has_mod and G.style_dim == (VARIANTS[name][2].get("mapping_units") or gan.generator.latent_size)
    R.assert_close(product_grads(gan.discriminator), ref["dgrads"], f"{name}: critic gradients")
    got = product_grads(gan.generator)
    R.assert_close(got, ref["ggrads"], f"{name}: generator gradients")
    n = 2 * G.mapping.num_layers
    assert all(np.abs(g).max() > 0 for g in got[:n])          # the prefix's variables come first, and every one has a gradient
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), ref["fakes"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ net level
# guards of the reference alone (min |LeakyReLU pre-activation|, min mean(a^2), min q, min max|style gradient|, min |mapping pre-act.|):
#   tiny_2    seed 1: (1.8e-05, 5.5e-03, 1.0e+00, 3e-01, 2.2e-02)
#   tiny_eq   seed 3: (2.5e-04, 2.6e-01, 2.1e+00, 2e-01, 1.3e-01)
#   mnist_eq  seed 3: (3.1e-04, 3.2e-02, 2.0e+00, 4e-01, 2.8e-02)
#   mnist_1   seed 1: (6.7e-04, 1.2e-02, 1.3e+00, 1e+00, 1.2e-01)
NET_SEED = {"tiny_2": 1, "tiny_eq": 3, "mnist_eq": 3, "mnist_1": 1}


def net_case(name, device=None, seed=None):
    arch, _, gen_kw = VARIANTS[name]
    seed = NET_SEED[name] if seed is None else seed
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = models.DCGANGenerator(arch=arch, normalization="style", **gen_kw)
    z = rng.normal(size=(B, model.latent_size)).astype(np.float32)
    need_dz = not gen_kw.get("normalize_latents", False)
    return model, z, need_dz, R.net_reference_pass(model, rng, z, need_dz, device=device)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_net_forward_and_backward_match_torch(name):
    """The generator alone: output, every parameter gradient and (without normalize_latents) dL/dz from need_dx=True for a random dout;
    beta = 1 doubles the gradients; forward(w = the prefix's output) and truncation with psi = 1 give the same bits; psi = 0 without
    noise gives one image per batch."""
    model, z, need_dz, (maps, dout, y, grads, dz, guards) = net_case(name)
    R.check_net_guards(guards)
    net = model.net()
    ctx = net.context(B, "test")
    nz = dict(noise=dev(maps)) if maps is not None else {}
    got_y = net.forward(ctx, dev(z), training=True, **nz).cpu().numpy().copy()
    if need_dz:
        got_dz = net.backward(ctx, dev(dout), need_dx=True, need_dw=True).cpu().numpy().copy()
        R.assert_close([got_dz], [dz], f"{name} dL/dz")
    else:
        assert net.backward(ctx, dev(dout), need_dx=False, need_dw=True) is None
        with pytest.raises(NotImplementedError, match="PixelNormalization"):
            net.backward(ctx, dev(dout), need_dx=True)
    net.eqlr_scale_gradients()
    R.assert_close([got_y], [y], f"{name} output")
    R.assert_close(product_grads(model), grads, f"{name} parameter gradients")
    # accumulation
    net.forward(ctx, dev(z), training=True, **nz)
    net.backward(ctx, dev(dout), need_dx=False, need_dw=True)
    first = [g.copy() for g in product_grads(model)]
    net.backward(ctx, dev(dout), need_dx=False, need_dw=True, beta=1.0, scale=1.0)
    for a, b in zip(product_grads(model), first):
        np.testing.assert_allclose(a, 2 * b, rtol=1e-5, atol=1e-6 * max(float(np.abs(b).max()), 1e-6))
    # the same bits in inference, from w, and under psi = 1
    assert np.array_equal(net.forward(ctx, dev(z), training=False, **nz).cpu().numpy(), got_y)
    w = ctx.map_h[-1].clone()
    assert tuple(w.shape) == (B, net.style_dim)
    c2 = net.context(B, "test2")
    assert np.array_equal(net.forward(c2, None, w=w, **nz).cpu().numpy(), got_y)
    assert np.array_equal(net.forward(c2, dev(z), truncation_psi=1.0, **nz).cpu().numpy(), got_y)
    net.mapping.vars["w_avg"].copy_(w.mean(0))
    same = net.forward(c2, dev(z), truncation_psi=0.0, **(dict(noise=False) if maps is not None else {})).cpu().numpy()
    assert all(np.array_equal(same[0], s) for s in same[1:]) and not np.array_equal(same, got_y)
    half = net.forward(c2, dev(z), truncation_psi=0.5, **nz).cpu().numpy()
    assert not np.array_equal(half, got_y) and not np.array_equal(half[0], half[1])
    with pytest.raises(ValueError, match="not both"):
        net.forward(c2, dev(z), w=w)
    with pytest.raises(ValueError, match="truncation_psi"):
        net.forward(c2, dev(z), training=True, truncation_psi=0.5)
    with pytest.raises(NotImplementedError, match="part of the batch"):
        net.backward(ctx, dev(dout), dw_rows=2)


# ------------------------------------------------------------------ replay, w_avg, averaging, checkpoints, sampling
def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "s3", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
        assert ma.optimizer.iterations == mb.optimizer.iterations
        assert ma.net().rng_offset == mb.net().rng_offset
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)
    assert np.array_equal(a.w_avg, b.w_avg)


def _pair_member(replay, seed=21, gen_kw=None, **kw):
    bg.set_seed(seed)
    base = dict(normalization="style", noise=True, mapping_layers=2, mapping_units=7, equalized_lr=True)
    gen = models.DCGANGenerator(arch="tiny", **dict(base, **(gen_kw or {})))
    disc = models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, **kw)
    for st in gen.net().stages:
        if st.noise is not None:
            st.noise.vars["noise_strength"].fill_(0.5)
    return gan


def _batches(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(n)]


def _mapping_values(model):
    mp = R.mapping_layer(model)
    return np.concatenate([mp.vars[n].detach().cpu().numpy().ravel() for n in mp.vars if n != "w_avg"])


def test_replayed_steps_equal_eager_steps_bit_for_bit_and_w_avg_follows_its_recurrence():
    eager, prog = _pair_member(False), _pair_member(True)
    assert np.array_equal(prog.w_avg, np.zeros(7, np.float32))
    start, avg = _mapping_values(prog.generator).copy(), np.zeros(7, np.float32)
    G = prog.generator.net()
    for i, reals in enumerate(_batches(4)):
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
        assert torch.equal(eager.images[0], prog.images[0]), i
        # the G-step's w, read back: w_avg -= (1 - beta) * (w_avg - mean), bg_ema_f32's line in float32, the batch mean as bg_colsum_f32
        # leaves it (its own tests hold that kernel; here it is run on the same rows) and within float32 rounding of the float64 mean
        w = G.context(B, "g").map_h[-1]
        mean = ops.colsum(w, torch.empty(7, device="cuda"), B, 7, torch.empty(ops.colsum_workspace_bytes(B, 7) // 4 + 4, device="cuda"),
                          scale=1.0 / B).cpu().numpy()
        np.testing.assert_allclose(mean, w.cpu().numpy().astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)
        avg = avg - np.float32(1.0 - G.mapping.w_avg_beta) * (avg - mean)
        assert avg.dtype == np.float32 and np.array_equal(prog.w_avg, avg), i
    assert prog._programs.last_was_replay and prog._programs.stats["replayed"] >= 2, prog._programs.stats
    assert eager._programs.stats["replayed"] == 0
    now = _mapping_values(prog.generator)
    assert np.isfinite(now).all() and (now != start).mean() > 0.9          # the prefix trains
    assert np.abs(prog.w_avg).max() > 0


def test_sampling_from_w_and_truncation_through_the_model():
    gan = _pair_member(True, generator_ema=0.5)
    for reals in _batches(2):
        gan.train_on_batch(reals)
    z = torch.randn(5, 10, generator=torch.Generator().manual_seed(1)).cuda()
    maps = torch.randn(5, gan.generator.net().noise_pixels, generator=torch.Generator().manual_seed(2))
    for ema in (False, True):
        out = gan.generate_samples(z, ema=ema, noise=maps).clone()
        w = gan.map_latents(z, ema=ema)
        assert tuple(w.shape) == (5, 7)
        assert torch.equal(gan.generate_samples(w=w, ema=ema, noise=maps), out)
        assert torch.equal(gan.generate_samples(z, ema=ema, noise=maps, truncation_psi=1.0), out)
        one = gan.generate_samples(z, ema=ema, noise=False, truncation_psi=0.0)
        assert all(torch.equal(one[0], s) for s in one[1:])
        wt = gan.map_latents(z, ema=ema, truncation_psi=0.5)
        assert torch.equal(gan.generate_samples(w=wt, ema=ema, noise=maps), gan.generate_samples(z, ema=ema, noise=maps, truncation_psi=0.5))
    # the averaged model averages the prefix's variables and w_avg (its state buffer is averaged with the weights)
    live, avg = gan.generator, gan.generator_ema
    assert (_mapping_values(avg) != _mapping_values(live)).mean() > 0.9
    a, l = R.mapping_layer(avg).vars["w_avg"].cpu().numpy(), gan.w_avg
    assert np.abs(a).max() > 0 and not np.array_equal(a, l)
    with pytest.raises(ValueError, match="not both"):
        gan.generate_samples(z, w=w)
    plain = bg.WGANGP(models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny"),
                      bg.WGANGP.HyperParameters(global_batch_size=B, batch_size=B), bg.TrainingConfig(log_dir="/tmp/bg_test_logs"))
    assert plain.w_avg is None
    with pytest.raises(ValueError, match="MappingNetwork"):
        plain.map_latents(z)


def test_checkpoint_resume_is_bit_identical_and_another_multiplier_is_refused(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    batches = _batches(4, seed=6)
    ref = _pair_member(True)
    for reals in batches[:2]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path / "map")).save(2)
    for reals in batches[2:]:
        ref.train_on_batch(reals)
    resumed = _pair_member(True, seed=5)
    assert not torch.equal(resumed.generator.store.theta, ref.generator.store.theta)
    CheckpointManager(resumed, str(tmp_path / "map")).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
    assert np.array_equal(ref.w_avg, resumed.w_avg) and np.abs(ref.w_avg).max() > 0
    other = _pair_member(True, gen_kw=dict(mapping_lr_multiplier=0.1))          # the same variable list, other raw kernels
    theta = other.generator.store.theta.clone()
    with pytest.raises(ValueError, match="mapping network"):
        CheckpointManager(other, str(tmp_path / "map")).restore(path)
    assert torch.equal(other.generator.store.theta, theta)
