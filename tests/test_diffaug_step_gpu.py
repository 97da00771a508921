"""GPU tests of ``augment=`` through whole training steps, against the float64 reference of tests/diffaug_reference.py, in the pattern
of tests/test_spectral_step_gpu.py.

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/ln_reference.py).  Each comparison
first asserts, on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within 5e-6 of zero and that no
x-hat gradient norm is below 1e-3 (spectrally normalised critic: and the signal ratio of tests/sn_reference.py).  The seeds below were
chosen so by running the reference alone on a CPU (diffaug_reference.make_gan(..., device="cpu")); what it gave for seeds 1-5 stands
beside them."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import blurred_gan_amd as bg
from blurred_gan_amd import models
from helpers import product_grads
from ln_reference import ATOL, RTOL, assert_close
import diffaug_reference as DR

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
# the reference alone, full policy, batch 4, global batch 5: (min |LeakyReLU pre-activation| over all passes of the step, min x-hat gradient
# norm[, min signal ratio]), seeds 1-5
#   tiny             (1.7e-5, 0.046), (2.6e-6, 0.043), (4.8e-5, 0.085), (2.3e-6, 0.059), (4.6e-6, 0.05)
#   tiny, blur       (1.1e-5, 0.013), (1.1e-5, 0.017), (1.5e-5, 0.032), (2.3e-6, 0.024), (4.6e-6, 0.017)
#   tiny_mnist       (1.0e-5, 0.15), (1.5e-5, 0.14), (1.3e-4, 0.098), (6.8e-6, 0.12), (8.2e-5, 0.11)
#   tiny_mnist, blur (2.7e-5, 0.043), (9.4e-5, 0.032), (2.7e-5, 0.023), (1.3e-4, 0.035), (2.3e-5, 0.034)
#   layer, blur      (2.8e-5, 0.31), (1.2e-4, 0.23), (2.9e-7, 0.21), (3.2e-6, 0.36), (3.7e-6, 0.27)
#   spectral, blur   (9.9e-6, 0.024, 1.02), (3.5e-5, 0.0099, 0.90), (4.5e-5, 0.046, 0.80), (2.3e-6, 0.024, 0.86), (4.6e-6, 0.032, 0.79)
#   pool, blur       (6.3e-6, 0.0077), (1.1e-5, 0.01), (1.5e-5, 0.018), (2.3e-6, 0.013), (8.1e-7, 0.0066)
#   tiny, blur, one operation: color (2.0e-5, 0.019), (3.5e-5, 0.02), (2.3e-5, 0.034), (2.3e-6, 0.032), (4.6e-6, 0.017);
#     translation (1.7e-5, 0.041), (2.7e-5, 0.043), (3.6e-5, 0.053), (1.9e-6, 0.055), (4.6e-6, 0.046);
#     cutout (2.0e-5, 0.044), (6.1e-6, 0.044), (3.0e-5, 0.063), (2.3e-6, 0.074), (4.6e-6, 0.055)
#   2 ranks: tiny, blur, global batch 6  (2.0e-6, 0.013), (2.8e-5, 0.015), (1.1e-5, 0.02), (2.4e-5, 0.024), (1.5e-5, 0.017)
SEED = {("tiny", False): 3, ("tiny", True): 3, ("tiny_mnist", False): 3, ("tiny_mnist", True): 4, "layer": 2, "spectral": 3, "pool": 3, "dp": 2}
STD = 0.9


def _step_case(arch, B, seed, kw, augment=FULL, **variant):
    gan, reals, rnd = DR.make_gan(arch, B, seed, augment, gbs=B + 1, **variant, **kw)
    ref = DR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, B + 1, gan.augment)
    DR.check_conditions(ref)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    gan.train_on_batch(reals.astype(np.float32), randomness=rnd)
    assert_close(product_grads(gan.discriminator), ref["dgrads"], "critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], "generator gradients")
    np.testing.assert_allclose(gan.images[0].cpu().numpy(), ref["fakes"], rtol=1e-4, atol=1e-5)      # self.images: un-augmented
    np.testing.assert_array_equal(gan.images[1].cpu().numpy(), reals)
    return gan


# ------------------------------------------------------------------ 1. gradient parity
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("blur", [False, True], ids=["noblur", "blur"])
@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist"])
def test_step_gradients_match_torch(arch, blur, config):
    gan = _step_case(arch, 4, SEED[(arch, blur)], CONFIGS[config], std=STD if blur else None)
    assert (gan.discriminator.net().blur is not None) == blur and gan.augment == bg.DiffAugment()


def test_step_gradients_match_torch_with_layer_normalization():
    gan = _step_case("tiny", 4, SEED["layer"], {}, normalization="layer", std=STD)
    assert gan.discriminator.net().has_ln


def test_step_gradients_match_torch_with_a_spectrally_normalised_critic():
    gan = _step_case("tiny", 4, SEED["spectral"], {}, critic_sn=True, std=STD)
    assert len(gan.discriminator.net().spectral_layers) == 3


def test_step_gradients_match_torch_with_the_pooling_critic():
    gan = _step_case("tiny", 4, SEED["pool"], {}, down="pool", std=STD)
    assert [st.kind for st in gan.discriminator.net().stages] == ["conv", "avgpool", "conv", "avgpool", "dense"]


def test_step_gradients_match_torch_in_split_bf16_conv_math():
    gan = _step_case("tiny", 4, SEED[("tiny", True)], dict(conv_math="bf16x6"), std=STD)
    assert gan.discriminator.net().conv_math == "bf16x6"


@pytest.mark.parametrize("policy", ["color", "translation", "cutout"])
def test_step_gradients_match_torch_for_each_operation_alone(policy):
    _step_case("tiny", 4, SEED[("tiny", True)], {}, augment=policy, std=STD)


def test_step_gradients_match_torch_with_keras_optimizers():
    """The optimizer objects see the same gradients: RMSprop / SGD at learning rate 0 leave the weights alone, gradients as above."""
    gan, reals, rnd = DR.make_gan("tiny", 4, SEED[("tiny", True)], FULL, gbs=5, std=STD)
    ref = DR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, 5, gan.augment)
    DR.check_conditions(ref)
    gan.discriminator.optimizer = bg.optimizers.RMSprop(0.0)
    gan.generator.optimizer = bg.optimizers.SGD(0.0, momentum=0.5)
    before = gan.discriminator.store.theta.clone()
    gan.train_on_batch(reals, randomness=rnd)
    assert torch.equal(before, gan.discriminator.store.theta)
    assert_close(product_grads(gan.discriminator), ref["dgrads"], "critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], "generator gradients")


# ------------------------------------------------------------------ 2. identity and sensitivity
def _one_step(augment, rnd_extra, kw, blur=True):
    gan, reals, rnd = DR.make_gan("tiny", 4, SEED[("tiny", blur)], augment, gbs=5, std=STD if blur else None, **kw)
    rnd.update(rnd_extra)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    metrics = gan.train_on_batch(reals, randomness=rnd)
    return metrics, product_grads(gan.discriminator), product_grads(gan.generator), gan


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("blur", [False, True], ids=["noblur", "blur"])
def test_a_zero_shift_is_the_unaugmented_step_bit_for_bit(config, blur):
    zero = {k: np.full((4, 8), 0.5, np.float32) for k in ("aug_fake", "aug_real", "aug_hat", "aug_g")}
    assert DR.decode(zero["aug_g"][0], 8, 8, bg.DiffAugment("translation"))["ty"] == 0
    m0, d0, g0, plain = _one_step(None, {}, CONFIGS[config], blur)
    m1, d1, g1, aug = _one_step("translation", zero, CONFIGS[config], blur)
    assert plain.augment is None and aug.augment == bg.DiffAugment("translation")
    assert m0 == m1
    for a, b in zip(d0 + g0, d1 + g1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_full_policy_moves_the_critic_gradients_far_beyond_the_parity_bound(config):
    """A transform that is silently skipped must fail: every kernel gradient of the critic (the Dense bias gradient is a sum of
    signs that no input reaches) differs from the unaugmented step's by more than 100 x the parity bound somewhere."""
    _, d0, _, _ = _one_step(None, {}, CONFIGS[config])
    _, d1, _, _ = _one_step(FULL, {}, CONFIGS[config])
    checked = 0
    for a, b in zip(d1, d0):
        if a.ndim < 2:
            continue
        bound = RTOL * np.abs(b) + ATOL * max(float(np.abs(b).max()), 1e-6)
        ratio = float((np.abs(a - b) / bound).max())
        print(f"[sensitivity] {a.shape}: max |difference| / parity bound = {ratio:.0f}")
        assert ratio > 100, (a.shape, ratio)
        checked += 1
    assert checked == 3


# ------------------------------------------------------------------ 3. replay, checkpoints
def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _pair_member(replay, seed=21, B=4, augment=FULL, **kw):
    bg.set_seed(seed)
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, augment=augment, **kw)


def test_replayed_steps_equal_eager_steps_bit_for_bit_with_drawn_params():
    B = 4
    eager, prog, plain = _pair_member(False), _pair_member(True), _pair_member(True, augment=None)
    g = torch.Generator().manual_seed(3)
    drawn = []
    for i in range(4):
        reals = (torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda()
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
        plain.train_on_batch(reals.clone())
        drawn.append(prog._buf("aug_d", (3 * B, 8)).cpu().numpy().copy())
    assert prog._programs.stats["replayed"] >= 2, prog._programs.stats
    # the params are drawn anew every step, from the model's own stream, which therefore moves faster than the plain model's
    assert all(not np.array_equal(drawn[0], d) for d in drawn[1:]) and all((d >= 0).all() and (d < 1).all() for d in drawn)
    assert prog._rng_off > plain._rng_off
    assert not torch.equal(prog.discriminator.store.theta, plain.discriminator.store.theta)
    # the three D-step slices and the G-step's block are different numbers
    d, gblk = drawn[-1], prog._buf("aug_g", (B, 8)).cpu().numpy()
    blocks = [d[:B], d[B:2 * B], d[2 * B:], gblk]
    assert all(not np.array_equal(blocks[i], blocks[j]) for i in range(4) for j in range(i))


def test_checkpoint_resume_is_bit_identical_and_loads_into_another_setting(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand(4, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(6)]
    ref = _pair_member(True)
    for reals in batches[:3]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path)).save(3)
    for reals in batches[3:]:
        ref.train_on_batch(reals)
    resumed = _pair_member(True, seed=5)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    for reals in batches[3:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v)
    assert ref._rng_off == resumed._rng_off
    # the setting is configuration, not state: the checkpoint loads into a model without it, and into one with another policy
    for other in (None, "cutout"):
        m = _pair_member(True, seed=7, augment=other)
        CheckpointManager(m, str(tmp_path)).restore(path)
        assert (m.augment is None) if other is None else (m.augment == bg.DiffAugment("cutout"))
        m.train_on_batch(batches[3])


# ------------------------------------------------------------------ 4. data parallel
WORLD, LOCAL = 2, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build_dp():
    """The case at the global batch: every rank and the single process build the same weights, images and randomness."""
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import diffaug_reference as DRef
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)        # a rank's model is made with the global batch as its batch_size
        n = LOCAL * WORLD
        gan, reals, rnd = DRef.make_gan("tiny", n, SEED["dp"], FULL, gbs=n, std=STD)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    return gan, reals, rnd


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    gan, reals, rnd = _build_dp()
    sh = lambda a: dist.shard(torch.from_numpy(np.asarray(a))).numpy()
    rnd_local = {k: ([sh(m) for m in v] if isinstance(v, list) else sh(v)) for k, v in rnd.items()}
    gan.train_on_batch(sh(reals), randomness=rnd_local)
    for tag, store in (("d", gan.discriminator.store), ("g", gan.generator.store)):
        np.save(os.path.join(out_dir, f"{tag}_grad_{rank}.npy"), store.grad[:store.n_train].cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_match_the_single_process_on_the_union_batch(tmp_path):
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    gan, reals, rnd = _build_dp()
    ref = DR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, LOCAL * WORLD, gan.augment)
    DR.check_conditions(ref)
    for tag, model in (("d", gan.discriminator), ("g", gan.generator)):
        st = model.store
        g0, g1 = np.load(tmp_path / f"{tag}_grad_0.npy"), np.load(tmp_path / f"{tag}_grad_1.npy")
        np.testing.assert_array_equal(g0, g1)
        own = {id(l) for l in model._own_layers()}
        views = [(off, int(np.prod(shape))) for (l, n, off, shape, tr) in st.entries if tr and id(l) in own]
        assert_close([g0[o:o + k] for o, k in views], ref["dgrads" if tag == "d" else "ggrads"], f"{tag} gradients, ranks against torch")
