"""GPU tests of a critic with LayerNormalization stages (models.DCGANDiscriminator(normalization="layer")) through engine.Net and
whole training steps, against the torch CPU float64 reference of tests/ln_reference.py.

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/test_resample_step_gpu.py).  Each
comparison first asserts, on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within 5e-6 of zero
(the gradient is discontinuous there and float32 may legitimately sit on the other branch) and that no x-hat gradient norm is
below 1e-3 (the penalty divides by it); the seeds below were chosen so, by running the reference alone on a CPU
(ln_reference.make_gan(..., device="cpu")), and the minima it gave stand beside them."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models
from helpers import product_grads, rel_l2
from ln_reference import DT, KINK, MIN_NORM, assert_close, make_gan, randomize, ref_forward, ref_params, ref_step_grads

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. net level
# min |LeakyReLU pre-activation| of the reference (float64, no GPU involved), seeds 1-5: tiny 4.8e-4, 3.5e-4, 6.0e-4, 4.4e-4, 2.1e-3;
# tiny_mnist 8.8e-4, 3.7e-3, 2.1e-3, 5.0e-4, 8.1e-4
NET_SEED = {"tiny": 5, "tiny_mnist": 2}


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist"])
def test_net_forward_and_backward_match_torch(arch):
    """The LN critic with injected Dropout masks: output, parameter gradients and input gradient for a random dout."""
    B = 4
    seed = NET_SEED[arch]
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = models.DCGANDiscriminator(arch=arch, normalization="layer")
    x = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch])
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
    assert sum(st.ln is not None for st in net.stages) == 2 and all(st.drop for st in net.stages if st.ln is not None)
    ctx = net.context(B, "test")
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    out = net.forward(ctx, dev(x), training=True, masks=[dev(m, torch.uint8) for m in masks] or None)
    got_y = out.cpu().numpy().copy()
    din = net.backward(ctx, dev(dout), need_dx=True, need_dw=True)
    assert_close([got_y], [y.detach().numpy()], f"{arch} output")
    assert_close(product_grads(model), [g.numpy() for g in grads[:-1]], f"{arch} parameter gradients")
    assert_close([din.cpu().numpy().reshape(x.shape)], [grads[-1].numpy()], f"{arch} input gradient")


# ------------------------------------------------------------------ 2. whole steps
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
# the reference alone (float64, no GPU involved): (min |LeakyReLU pre-activation| over all passes of the step, min x-hat gradient
# norm) for seeds 1-5 -- plain (2.8e-5, 2.6), (1.2e-4, 2.1), (2.9e-7, 2.1), (3.2e-6, 1.7), (3.7e-6, 3.1); behind the blur (2.8e-5, 1.1),
# (2.1e-5, 1.0), (2.9e-7, 1.4), (3.2e-6, 1.2), (3.7e-6, 1.5); pooled (2.8e-5, 1.1), (1.2e-4, 0.67), (2.9e-7, 0.86), (3.2e-6, 0.74),
# (3.7e-6, 0.96)
STEP_SEED = {"plain": 2, "blur": 1, "pool": 2}


def _step_case(arch, B, seed, kw, **variant):
    gan, reals, rnd = make_gan(arch, B, seed, gbs=B + 1, **variant, **kw)
    dg, gg, fakes, kink, norm = ref_step_grads(gan.generator, gan.discriminator, reals, rnd, gbs=B + 1)
    assert kink > KINK, kink
    assert norm > MIN_NORM, norm
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
    assert [(st.kind, st.ln is not None) for st in gan.discriminator.net().stages] == [("conv", True), ("conv", True), ("dense", False)]


def test_step_gradients_match_torch_behind_the_blur():
    gan = _step_case("tiny", 4, STEP_SEED["blur"], {}, std=0.9)
    assert gan.discriminator.net().blur is not None


def test_step_gradients_match_torch_with_pooling():
    gan = _step_case("tiny", 4, STEP_SEED["pool"], {}, down="pool")
    assert [st.kind for st in gan.discriminator.net().stages] == ["conv", "avgpool", "conv", "avgpool", "dense"]


# ------------------------------------------------------------------ 3. the three D-step configurations agree
def test_d_step_configurations_give_the_same_critic_gradients():
    """The relation (and tolerance) of test_step_gpu.py: test_merged_penalty_filter_gradients_equal_the_separate_launches.  With LN
    stages the first two configurations enqueue the same launches; the unmerged one runs the x-hat rows as a batch of their own."""
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
            print(name, a.shape, rel_l2(a, b))
            assert rel_l2(a, b) < 2e-6 or not np.any(b), (name, a.shape, rel_l2(a, b))


# ------------------------------------------------------------------ 4. replay and checkpoints
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
    gen = models.DCGANGenerator(arch="mnist")
    disc = models.DCGANDiscriminator(arch="mnist", normalization="layer")
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
    assert not torch.equal(resumed.discriminator.store.theta, ref.discriminator.store.theta)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
