"""GPU tests of a critic with the MinibatchStdDev layer (models.DCGANDiscriminator(minibatch_stddev=G)) through engine.Net and whole
training steps, against the torch CPU float64 reference of tests/mbstd_reference.py (tests/ln_reference.py's walker with an
``mbstd`` branch, under tests/objective_reference.py's step).

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/test_layernorm_step_gpu.py).  Each
comparison first asserts, on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within KINK = 5e-6
of zero, that no x-hat gradient norm is below MIN_NORM = 1e-3, and that no non-constant column of the layer has an s below
mbstd_reference.MIN_S in the x-hat pass (the source divides by s^3).  The seeds below were chosen so by running the reference
alone on a CPU (case(..., device="cpu")); the (kink, norm, min s) it gave stand beside them."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models
from helpers import product_grads, rel_l2
from ln_reference import DT, KINK, assert_close, randomize, ref_params
import mbstd_reference as MR
import objective_reference as OR

pytestmark = pytest.mark.gpu
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
LAZY_R1 = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals", penalty_interval=2)

# name -> (seed, critic keywords, G, make_gan keywords).  The reference alone (float64, no GPU involved), seeds 1-5, as
# (min |LeakyReLU pre-activation|, min x-hat gradient norm, min s of a non-constant column of the x-hat pass):
#   plain      (7.0e-06, 0.14, 1.7e-04) (3.5e-05, 0.19, 1.0e-04) (3.4e-05, 0.19, 1.8e-04) (2.3e-06, 0.26, 1.0e-04) (4.6e-06, 0.2, 1.0e-04)
#   g4         (7.0e-06, 0.14, 3.9e-03) (3.5e-05, 0.19, 4.9e-03) (3.4e-05, 0.19, 4.6e-03) (2.3e-06, 0.26, 3.6e-04) (4.6e-06, 0.2, 8.3e-03)
#   blur       (1.2e-05, 0.039, 1.1e-04) (2.7e-05, 0.053, 2.0e-04) (3.0e-05, 0.051, 1.0e-04) (2.3e-06, 0.088, 1.0e-04) (4.6e-06, 0.06, 1.1e-04)
#   pool       (3.5e-06, 0.03, 1.0447e-04) (8.2e-07, 0.044, 1.0448e-04) (1.7e-05, 0.046, 1.0139e-04) (2.2e-06, 0.07, 1.0000e-04) (4.6e-06, 0.058, 1.0374e-04)
#   layernorm  (2.8e-05, 2.4, 2.5e-04) (1.2e-04, 2, 5.0e-04) (2.9e-07, 1.6, 1.9e-04) (3.2e-06, 1.6, 3.4e-04) (3.7e-06, 3.3, 4.9e-03)
#   lazy       (1.2e-05, 0.041, 1.3e-04) (2.7e-05, 0.056, 1.8e-04) (1.7e-05, 0.058, 1.0e-04) (2.3e-06, 0.086, 1.0e-04) (4.6e-06, 0.06, 1.4e-04)
#              (its step without the penalty: the same kinks, no x-hat pass)
#   two_launch, the "mnist" critic at G = 4 (a group of 4 * 49 * 128 = 25088 floats, which needs the workspace):
#              (2.1e-07, 0.09, 6.0e-04) (2.6e-07, 0.089, 3.0e-04) (4.8e-08, 0.09, 4.2e-04) (2.1e-07, 0.092, 2.7e-04) (2.5e-07, 0.1, 4.4e-04)
#              No seed can pass KINK there: a step of the "mnist" pair has 552 000 LeakyReLU pre-activations (18 816 per sample
#              in the critic's four passes, 31 360 in the generator's two), about 25 of them within 5e-6 of zero on average; none
#              of the seeds 1-60 keeps its nearest further out than that.  The variant therefore takes the smallest critic on
#              "tiny" images whose top leaves the resident route at G = 4 instead (wide_top_critic: 4 * 64 * 64 = 16384 floats
#              per group, 65 536 pre-activations a step), where about one seed in nine passes:
#   two_launch (2.3e-07, 0.24, 1.8e-03) (6.6e-07, 0.25, 9.4e-04) (2.5e-06, 0.24, 7.4e-04) (2.7e-06, 0.25, 2.2e-03) (1.0e-06, 0.27, 1.6e-03)
#              the first seeds that pass: 17 (1.0e-05, 0.26, 1.4e-03), 31 (6.2e-06, 0.27, 6.6e-04), 40 (5.8e-06, 0.26, 9.0e-04)
VARIANTS = {
    "plain": (1, {}, 2, {}),
    "g4": (2, {}, 4, {}),
    "blur": (2, {}, 2, dict(std=0.9)),
    "pool": (3, dict(downsampling="pool"), 2, {}),
    "layernorm": (1, dict(normalization="layer"), 2, {}),
    "lazy": (2, {}, 2, dict(objective=LAZY_R1, std=0.9)),
    "two_launch": (17, None, 4, {}),
}
WIDE_TOP = (8, 8, 64)       # the map in front of two_launch's layer


def wide_top_critic(G):
    """One 5x5 convolution to 64 channels at full size, LeakyReLU, Dropout, the layer, the head: at batch 4 and G = 4 a group holds
    4 * 8 * 8 * 64 = 16384 floats, more than the resident route takes, so forward and penalty call go through the workspace."""
    from blurred_gan_amd import layers as L
    m = L.SpectralSequential()
    for layer in (L.Conv2D(WIDE_TOP[2], 5, strides=1, padding="same", input_shape=list(models.IMAGE_SHAPE["tiny"])), L.LeakyReLU(), L.Dropout(0.3),
                  L.MinibatchStdDev(group_size=G), L.Flatten(), L.Dense(1, activation="linear")):
        m.add(layer)
    return m


def case(name, device=None, seed=None, **kw):
    s, critic, G, mk = VARIANTS[name]
    disc = (lambda: wide_top_critic(G)) if critic is None else (lambda: models.DCGANDiscriminator(arch="tiny", minibatch_stddev=G, **critic))
    return OR.make_gan("tiny", 4, s if seed is None else seed, gbs=5, device=device, disc=disc, **mk, **kw)


def reference(gan, reals, rnd):
    ref = MR.ref_step(gan.generator, gan.discriminator, reals, rnd, 5, gan.objective, penalty_step=gan._penalty_this_step())
    MR.check_guards(ref)
    return ref


def _step_case(name, kw=None, n_batches=0):
    gan, reals, rnd = case(name, **(kw or {}))
    gan.n_batches.assign(n_batches)
    ref = reference(gan, reals, rnd)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals, randomness=rnd)
    assert_close(product_grads(gan.discriminator), ref["dgrads"], f"{name}: critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], f"{name}: generator gradients")
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), ref["fakes"], rtol=1e-4, atol=1e-5)
    return gan, ref


# ------------------------------------------------------------------ 1. net level
# (min |LeakyReLU pre-activation|, min s of a non-constant column) of the reference, seeds 1-5: tiny (1.3e-06, 1.3e-04),
# (1.5e-04, 2.7e-04), (3.8e-04, 3.3e-04), (4.5e-05, 2.8e-04), (2.5e-04, 1.4e-04); tiny_mnist (1.2e-03, 7.8e-04), (4.1e-04, 2.6e-04),
# (6.2e-04, 6.8e-04), (6.8e-04, 1.6e-03), (4.1e-04, 5.0e-04)
NET_SEED = {"tiny": 5, "tiny_mnist": 2}


def net_reference(arch, seed, B=4, G=2):
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = models.DCGANDiscriminator(arch=arch, minibatch_stddev=G)
    x = rng.uniform(-1, 1, size=(B,) + models.IMAGE_SHAPE[arch])
    return model, rng, x


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist"])
def test_net_forward_and_backward_match_torch(arch):
    """The critic with injected Dropout masks: output, parameter gradients and input gradient for a random dout."""
    B = 4
    model, rng, x = net_reference(arch, NET_SEED[arch])
    randomize(model, rng)
    masks = [(rng.uniform(size=(B,) + tuple(s)) >= 0.3).astype(np.uint8) for l, s in model.flat_layers() if l.kind == "dropout"]
    dout = rng.normal(size=(B,) + model.output_shape[1:])
    W, train = ref_params(model)
    xt = torch.as_tensor(x).to(DT).requires_grad_(True)
    pre = []
    with MR.walker() as seen:
        y = MR.ref_forward(model, W, xt, True, masks, pre)
        grads = torch.autograd.grad((y * torch.as_tensor(dout)).sum(), train + [xt])
    assert min(pre) > KINK, min(pre)
    assert min(seen) > MR.MIN_S, seen
    net = model.net()
    assert [st.kind for st in net.stages] == ["conv", "conv", "mbstd", "dense"]
    ctx = net.context(B, "test")
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    out = net.forward(ctx, dev(x), training=True, masks=[dev(m, torch.uint8) for m in masks] or None)
    got_y = out.cpu().numpy().copy()
    din = net.backward(ctx, dev(dout), need_dx=True, need_dw=True)
    assert_close([got_y], [y.detach().numpy()], f"{arch} output")
    assert_close(product_grads(model), [g.numpy() for g in grads[:-1]], f"{arch} parameter gradients")
    assert_close([din.cpu().numpy().reshape(x.shape)], [grads[-1].numpy()], f"{arch} input gradient")


# ------------------------------------------------------------------ 2. whole steps
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_step_gradients_match_torch_in_every_d_step_configuration(config):
    gan, _ = _step_case("plain", CONFIGS[config])
    assert [st.kind for st in gan.discriminator.net().stages] == ["conv", "conv", "mbstd", "dense"]


def test_step_gradients_match_torch_with_one_group_per_slice():
    gan, _ = _step_case("g4")
    assert gan.discriminator.net().mbstd_layers[0].group_size == 4 == gan.batch_size


def test_step_gradients_match_torch_behind_the_blur():
    gan, _ = _step_case("blur")
    assert gan.discriminator.net().blur is not None


def test_step_gradients_match_torch_with_pooling():
    gan, _ = _step_case("pool")
    assert [st.kind for st in gan.discriminator.net().stages] == ["conv", "avgpool", "conv", "avgpool", "mbstd", "dense"]


def test_step_gradients_match_torch_with_layer_normalization():
    """Both kinds of source in one pass: the source backward starts at the MinibatchStdDev stage and picks up the
    LayerNormalization stages' on the way down."""
    gan, _ = _step_case("layernorm")
    net = gan.discriminator.net()
    assert net.has_ln and net._gp_kinds() == ["ln", "ln", "mbstd", "dense"]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_step_gradients_match_torch_on_the_two_launch_route(config):
    """A top too large for the resident route: the engine sizes the workspace and shares it between the forward (all rows of the
    pass) and the penalty call (the x-hat rows); both take two launches."""
    from blurred_gan_amd import ops
    B, G, (H, W, C) = 4, VARIANTS["two_launch"][2], WIDE_TOP
    for rows in (B, 2 * B, 3 * B):
        assert ops.mbstd.workspace_bytes(rows, G, H * W, C) > 0 and not ops.mbstd.plan(rows, G, H * W, C, "gp")["resident"]
    gan, _ = _step_case("two_launch", CONFIGS[config])
    net = gan.discriminator.net()
    assert [st.kind for st in net.stages] == ["conv", "mbstd", "dense"] and gan.batch_size == B
    st = net.stages[1]
    assert (st.lin.group_size, st.ln_pixels, tuple(st.in_shape)) == (G, H * W, WIDE_TOP)


@pytest.mark.parametrize("n_batches", [0, 1])
def test_lazy_r1_steps_with_and_without_the_penalty(n_batches):
    gan, ref = _step_case("lazy", n_batches=n_batches)
    assert gan._objective.penalty_interval == 2
    assert (ref["gp_term"] != 0.0) == (n_batches == 0)


# ------------------------------------------------------------------ 3. the three D-step configurations agree
def test_d_step_configurations_give_the_same_critic_gradients():
    """The relation (and tolerance) of tests/test_layernorm_step_gpu.py's test of the same name."""
    ref = None
    for name in ("merged", "merged_separate_wgrad", "unmerged"):
        gan, reals, rnd = case("blur", **CONFIGS[name])
        gan.discriminator.optimizer.learning_rate = 0.0
        gan.generator.optimizer.learning_rate = 0.0
        gan.train_on_batch(reals, randomness=rnd)
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


def _mnist_pair_member(replay, seed=21, B=4, mb=4, **kw):
    bg.set_seed(seed)
    gen = models.DCGANGenerator(arch="mnist")
    disc = models.DCGANDiscriminator(arch="mnist", minibatch_stddev=mb)
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


def test_checkpoint_resume_is_bit_identical_and_a_plain_critics_checkpoint_is_refused(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand(4, 28, 28, 1, generator=g) * 2 - 1).cuda() for _ in range(4)]
    ref = _mnist_pair_member(True)
    for reals in batches[:2]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path / "mb")).save(2)
    for reals in batches[2:]:
        ref.train_on_batch(reals)
    resumed = _mnist_pair_member(True, seed=5)
    assert not torch.equal(resumed.discriminator.store.theta, ref.discriminator.store.theta)
    CheckpointManager(resumed, str(tmp_path / "mb")).restore(path)
    for reals in batches[2:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
    # the configuration travels in the Dense kernel's shape: a plain critic's checkpoint does not load into one with the layer
    bg.set_seed(21)
    plain = bg.BlurredWGANGP(models.DCGANGenerator(arch="mnist"), models.DCGANDiscriminator(arch="mnist"),
                             bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=4, batch_size=4),
                             bg.TrainingConfig(log_dir="/tmp/bg_test_logs"))
    plain.train_on_batch(batches[0])
    plain_path = CheckpointManager(plain, str(tmp_path / "plain")).save(1)
    before = resumed.discriminator.store.theta.clone()
    with pytest.raises(Exception) as e:
        CheckpointManager(resumed, str(tmp_path / "plain")).restore(plain_path)
    print("refused with:", type(e.value).__name__, e.value)
    assert not isinstance(e.value, (KeyboardInterrupt, SystemExit))
    assert torch.equal(resumed.discriminator.store.theta, before)
