"""GPU tests of critics with LayerNormalization stages in other places than models.DCGANDiscriminator(normalization="layer") puts
them (tests/ln_critics.py: a plain stage between, above and below LN stages, three LN stages, LN without Dropout, a conv without
bias, the one-float route, a row of more than one chunk) through engine.Net and whole training steps, against the torch CPU
float64 reference of tests/ln_reference.py.

Tolerance of every gradient comparison: ln_reference.assert_close as it stands -- per tensor rtol 2e-3, atol 2e-4 * max|reference|.
Each comparison first asserts, on the reference alone, that no LeakyReLU pre-activation lies within KINK of zero and no x-hat
gradient norm is below MIN_NORM; the seeds (ln_critics.NET_SEED / STEP_SEED, the reference's minima beside them) were chosen so on a
CPU, and tests/test_layernorm_shapes_cpu.py asserts the same conditions without a GPU."""
import functools

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models, ops
from helpers import product_grads, rel_l2
from ln_reference import KINK, MIN_NORM, assert_close
import ln_critics as LC

pytestmark = pytest.mark.gpu
SHAPES = sorted(LC.SHAPES)


# ------------------------------------------------------------------ 1. net level
@pytest.mark.parametrize("name", SHAPES)
def test_net_forward_and_backward_match_torch(name):
    """Injected Dropout masks, a random dout: output, parameter gradients and input gradient of the bare critic."""
    (model, x, masks, dout), (y, grads, kink) = LC.net_case(name, LC.NET_SEED[name])
    assert kink > KINK, kink
    net = model.net()
    LC.assert_claims(name, net)
    B = LC.B
    ctx = net.context(B, "test")
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    out = net.forward(ctx, dev(x), training=True, masks=[dev(m, torch.uint8) for m in masks] or None)
    got_y = out.cpu().numpy().copy()
    din = net.backward(ctx, dev(dout), need_dx=True, need_dw=True)
    assert_close([got_y], [y], f"{name} output")
    assert_close(product_grads(model), grads[:-1], f"{name} parameter gradients")
    assert_close([din.cpu().numpy().reshape(x.shape)], [grads[-1]], f"{name} input gradient")


# ------------------------------------------------------------------ 2. whole steps
_REFERENCE = {}


def _reference(name, std, gan, reals, rnd):
    """The float64 reference of a step case, computed once per (shape, blur) and shared by the D-step configurations: they start
    from the same seed, so from the same weights -- asserted, bit for bit."""
    theta = [m.store.theta.detach().cpu().clone() for m in (gan.generator, gan.discriminator)]
    if (name, std) not in _REFERENCE:
        _REFERENCE[(name, std)] = (theta, LC.step_reference(gan, reals, rnd))
    theta0, ref = _REFERENCE[(name, std)]
    assert all(torch.equal(a, b) for a, b in zip(theta, theta0))
    return ref


@functools.lru_cache(maxsize=None)
def _step(name, config, std=None):
    """One train_on_batch of shape ``name`` in D-step configuration ``config`` with learning rates 0: what the reference says of
    it and the product's (critic gradients, generator gradients, fakes).  Cached: the comparisons with the reference and the
    agreement of the configurations read the same step."""
    seed = LC.STEP_SEED[name] if std is None else LC.BLUR_SEED
    gan, reals, rnd = LC.step_case(name, seed, std=std, **LC.D_STEP_CONFIGS[config])
    D = gan.discriminator.net()
    LC.assert_claims(name, D)
    assert (D.blur is not None) == (std is not None)
    ref = _reference(name, std, gan, reals, rnd)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals.astype(np.float32), randomness=rnd)
    return ref, (product_grads(gan.discriminator), product_grads(gan.generator), gan.images[0].cpu().numpy())


def _compare(name, config, std=None):
    (dg, gg, fakes, kink, norm), (got_d, got_g, got_fakes) = _step(name, config, std)
    assert kink > KINK, kink
    assert norm > MIN_NORM, norm
    assert_close(got_d, dg, f"{name} {config} critic gradients")
    assert_close(got_g, gg, f"{name} {config} generator gradients")
    np.testing.assert_allclose(got_fakes, fakes, rtol=1e-4, atol=1e-5)


STEP_CASES = [(n, c) for n in SHAPES for c in ("merged", "unmerged")] + [(n, "merged_separate_wgrad") for n in LC.ALL_CONFIGS]


@pytest.mark.parametrize("name,config", STEP_CASES)
def test_step_gradients_match_torch(name, config):
    """gbs = B + 1, learning rates 0: the critic's and the generator's gradients and the fakes of one whole step."""
    _compare(name, config)


def test_step_gradients_match_torch_behind_the_blur():
    """ln_plain_ln behind the blur: blur^T of the input gradient goes to ctx.blur_grad(), the blurred x-hat survives for the source
    backward's first filter gradient."""
    _compare("ln_plain_ln", "merged", std=LC.BLUR_STD)


# ------------------------------------------------------------------ 3. the three D-step configurations agree
@pytest.mark.parametrize("name", LC.ALL_CONFIGS)
def test_d_step_configurations_give_the_same_critic_gradients(name):
    """The relation and bound of test_layernorm_step_gpu.py's test of the same name: rel-L2 < 2e-6, or the tensor is all zero."""
    ref = _step(name, "merged")[1][0]
    for config in ("merged_separate_wgrad", "unmerged"):
        for a, b in zip(_step(name, config)[1][0], ref):
            print(name, config, a.shape, rel_l2(a, b))
            assert rel_l2(a, b) < 2e-6 or not np.any(b), (name, config, a.shape, rel_l2(a, b))


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


def _pair_member(name, replay, seed=21):
    bg.set_seed(seed)
    gen, disc = models.DCGANGenerator(arch=LC.ARCH), LC.build(name)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=LC.BLUR_STD, global_batch_size=LC.B, batch_size=LC.B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay)


@pytest.mark.parametrize("name", LC.ALL_CONFIGS)
def test_replayed_steps_equal_eager_steps_bit_for_bit(name):
    """Eight steps with the build's own randomness and Adam at work, replay on against replay off.  The chunked route's extra
    buffers (ctx.gin, the source backward's ctx.zdot) are addresses a step program holds like any other."""
    eager, prog = _pair_member(name, False), _pair_member(name, True)
    LC.assert_claims(name, prog.discriminator.net())
    assert ops.layernorm.route(LC.SHAPES["chunked"][0][0])["chunks"] > 1
    g = torch.Generator().manual_seed(3)
    for i in range(8):
        reals = (torch.rand(LC.B, *LC.IMAGE, generator=g) * 2 - 1).cuda()
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
    assert prog._programs.stats["replayed"] >= 6, prog._programs.stats
