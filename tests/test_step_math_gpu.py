"""The whole training step in the opt-in split-bf16 conv math (WGAN(conv_math="bf16x6")): against the oracle with the bounds of
tests/test_step_gpu.py (whose tests run here unchanged, on a model built in this mode), the C2 step against the fp32 step from
the same state, and a checkpoint written in fp32 mode restored into a model in this mode."""
import functools

import numpy as np
import pytest
import torch

import test_step_gpu as T
from helpers import product_grads, rel_l2

pytestmark = pytest.mark.gpu


def _x6(monkeypatch):
    monkeypatch.setattr(T, "_make", functools.partial(T._make, conv_math="bf16x6"))


def _ran_x6(gan, step):
    from blurred_gan_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        step()
        torch.cuda.synchronize()
        return [r[0] for r in ops.prof_records()]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


def test_tiny_three_steps_x6_match_oracle(monkeypatch):
    """tiny, B 4: three full steps (D + GP + G + Adam), the first recorded, the others replayed."""
    _x6(monkeypatch)
    T.test_three_training_steps_match_oracle("tiny", 4, 0.9)


def test_celeba64_steps_x6_match_oracle(monkeypatch):
    """celeba64, B 8: three consecutive steps with the real learning rate against the float64 oracle (the G4 / G5 layers run
    the split kernel)."""
    _x6(monkeypatch)
    T.test_real_architecture_training_steps_match_oracle("celeba64", 8, 5.0, 3)


def test_celeba64_eager_step_x6_matches_oracle(monkeypatch):
    """celeba64, B 8, every launch eager (no step program)."""
    monkeypatch.setattr(T, "_make", functools.partial(T._make, conv_math="bf16x6", step_replay=False))
    T.test_real_architecture_training_steps_match_oracle("celeba64", 8, 5.0, 2)


def test_c2_step_x6_against_fp32_step():
    """C2 (celeba64, B 256, sigma 5): one step in each mode from the same state and randomness, GPU against GPU.  Each mode is
    within the C2 test's bounds of the oracle (critic rel-L2 2e-3, generator 2e-2: test_step_gpu._full_batch_step_matches_oracle),
    so the two are within twice those of each other."""
    from oracle import step as S
    grads = {}
    for math in ("fp32", "bf16x6"):
        gan, st, reals, rng = T._make("celeba64", 256, 5.0, seed=11, conv_math=math)
        rnd = S.draw_randomness("celeba64", 256, rng, np.float64)
        gan.discriminator.optimizer.learning_rate = 0.0
        gan.generator.optimizer.learning_rate = 0.0
        names = _ran_x6(gan, lambda: gan.train_on_batch(reals.astype(np.float32), randomness=rnd))
        assert any("x6" in n for n in names) == (math == "bf16x6"), names
        grads[math] = (product_grads(gan.discriminator), product_grads(gan.generator))
        del gan
    dF, gF = grads["fp32"]
    dX, gX = grads["bf16x6"]
    for i, (p, q) in enumerate(zip(dF, dX)):
        assert np.isfinite(q).all()
        if p.size > 1:
            assert rel_l2(q, p) <= 4e-3, ("d", i, rel_l2(q, p))
    for i, (p, q) in enumerate(zip(gF, gX)):
        assert np.isfinite(q).all()
        if p.size > 1:
            assert rel_l2(q, p) <= 4e-2, ("g", i, rel_l2(q, p))


def test_switching_mode_records_a_new_program():
    gan, st, reals, rng = T._make("celeba64", 8, 5.0, seed=12)
    r = reals.astype(np.float32)
    gan.train_on_batch(r)                              # records the fp32 programs
    gan.conv_math = "bf16x6"
    names = _ran_x6(gan, lambda: gan.train_on_batch(r))
    assert any("x6" in n for n in names), names       # a replay of the fp32 program would launch no split kernel
    assert gan.conv_math == "bf16x6" and gan.generator.net().conv_math == "bf16x6"
    gan.conv_math = "fp32"
    names = _ran_x6(gan, lambda: gan.train_on_batch(r))
    assert not any("x6" in n for n in names), names


def test_checkpoint_from_fp32_mode_restores_in_x6_mode(tmp_path):
    import blurred_gan_amd as bg
    from blurred_gan_amd import models
    from blurred_gan_amd.checkpoint import CheckpointManager
    B = 8

    def make(seed, math):
        bg.set_seed(seed)
        gen, disc = models.DCGANGenerator(arch="celeba64"), models.DCGANDiscriminator(arch="celeba64")
        hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=2.0, global_batch_size=B, batch_size=B)
        return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir=str(tmp_path / "log")), conv_math=math)
    g = torch.Generator().manual_seed(1)
    data = [torch.rand(B, 64, 64, 3, generator=g) * 2 - 1 for _ in range(3)]
    first = make(7, "fp32")
    first.fit(data[:2], epochs=1)
    mgr = CheckpointManager(first, str(tmp_path / "ckpt"))
    mgr.save()
    resumed = make(99, "bf16x6")
    CheckpointManager(resumed, str(tmp_path / "ckpt")).restore(mgr.latest_checkpoint)
    assert int(resumed.n_batches) == 2
    for a, b in ((resumed.generator, first.generator), (resumed.discriminator, first.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta)
    names = _ran_x6(resumed, lambda: resumed.fit(data[2:], epochs=1))
    assert any("x6" in n for n in names), names
    assert int(resumed.n_batches) == 3
    for m in (resumed.generator, resumed.discriminator):
        assert torch.isfinite(m.store.theta).all()
    out = resumed.generate_samples(torch.rand(4, resumed.latent_size, device="cuda"))
    assert torch.isfinite(out).all()
