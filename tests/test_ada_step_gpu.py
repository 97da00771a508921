"""GPU tests of ``augment=AdaptiveAugment(...)`` through whole training steps, against the float64 reference of tests/ada_reference.py
(objective_reference.ref_step_grads behind the gated T), in the pattern of tests/test_diffaug_step_gpu.py and with its tolerances
(tests/ln_reference.py: per tensor rtol 2e-3, atol 2e-4 * max|reference|), after the same assertions on the reference alone.

The seeds were chosen by running the reference alone on a CPU (build(..., device="cpu")); what it gave stands beside each case:
(min |LeakyReLU pre-activation|, min penalised gradient norm), and for the adaptive run the smallest |real score| of all its steps.

The adaptive run: the controller reads only the SIGN of the critic's real scores, so the test first asserts -- on the reference alone --
that no real score of any step lies within SIGN_MARGIN of zero (a hundred times the step tolerance taken of the largest score); the
product's signs are then decided, and gan.augment_p must equal the Python rule fed with the reference's scores exactly."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models
from helpers import product_grads
from ln_reference import ATOL, assert_close
import ada_reference as AR
import diffaug_reference as DR
import ln_reference as LN

pytestmark = pytest.mark.gpu

SCALE, STD, B, GBS = 10.0, 0.9, 4, 5
FULL = "color,translation,cutout"
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
R1 = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals")
LAZY = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals", penalty_interval=2)
FIXED_HALF = dict(policy=FULL, p=0.5, target=None)
# the reference alone, seeds 1-6 (r1 and lazy at n_batches 0 alike; lazy at n_batches 1 has no penalty pass: 7.4e-6 at seed 6, else the same):
#   (9.4e-6, 0.47), (3.5e-5, 0.19), (3.1e-5, 0.6), (2.3e-6, 0.6), (4.6e-6, 0.18), (3.4e-6, 0.32)
# adaptive run, p after each of its five steps / smallest |real score|: seed 3: 0.5, 0.75, 0.75, 1, 1 (the upper clamp) / 0.43;
#   seed 5: 0.5, 0.75, 0.75, 0.75, 0.75 (r_t = 0 = target in the second interval: p stays) / 0.035; seed 1: 0.5, 0.25, 0.25, 0, 0 / 0.15;
#   seed 6: a real score of -0.030 is inside the margin at the scores' scale of 2.5
SEED = {"r1": 3, "lazy": 3}
ADAPTIVE_SEEDS = [1, 3, 5]
SIGN_MARGIN = 100 * ATOL


def build(objective, seed, augment, device=None, **kw):
    return AR.make_gan("tiny", B, seed, augment, objective=objective, gbs=GBS, std=STD, score_scale=SCALE, device=device, **kw)


def reference(gan, reals, rnd, p):
    ref = AR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, GBS, gan.objective, gan.augment, p,
                            penalty_step=gan._penalty_this_step(), e_drift=float(gan.hparams.e_drift))
    assert ref["kink"] > LN.KINK, ref["kink"]
    assert ref["norm"] > LN.MIN_NORM, ref["norm"]
    return ref


def _freeze(gan):
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0


def _fired(rnd, p, cfg):
    return {k: [AR.fired_mask(u, p, cfg) for u in rnd[k]] for k in ("aug_fake", "aug_real", "aug_hat", "aug_g")}


# ------------------------------------------------------------------ 1. gradient parity at a fixed p
def _step_case(objective, seed, kw, n_batches=0):
    gan, reals, rnd = build(objective, seed, bg.AdaptiveAugment(**FIXED_HALF), **kw)
    gan.n_batches.assign(n_batches)
    fired = _fired(rnd, 0.5, gan.augment)
    print("[fired masks]", fired)
    assert len({m for v in fired.values() for m in v}) >= 5          # a mix of masks, none of the passes all on or all off
    ref = reference(gan, reals, rnd, 0.5)
    _freeze(gan)
    gan.train_on_batch(reals, randomness=rnd)
    assert_close(product_grads(gan.discriminator), ref["dgrads"], "critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], "generator gradients")
    assert gan.augment_p == 0.5
    return gan


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_step_gradients_match_torch_at_a_fixed_p(config):                 # seed 3: 3.1e-5, 0.6
    gan = _step_case(R1, SEED["r1"], CONFIGS[config])
    assert gan.discriminator.net().blur is not None and gan.augment == bg.AdaptiveAugment(**FIXED_HALF)


@pytest.mark.parametrize("n_batches", [0, 1], ids=["penalty_step", "penalty_free_step"])
def test_step_gradients_match_torch_under_a_lazy_penalty(n_batches):
    gan = _step_case(LAZY, SEED["lazy"], {}, n_batches=n_batches)
    assert gan.objective.penalty_interval == 2


def test_wrong_width_of_injected_randomness_is_refused():
    gan, reals, rnd = build(R1, SEED["r1"], bg.AdaptiveAugment(**FIXED_HALF))
    rnd["aug_real"] = rnd["aug_real"][:, :8]
    with pytest.raises(ValueError, match="12"):
        gan.train_on_batch(reals, randomness=rnd)


# ------------------------------------------------------------------ 2. p = 1 and p = 0 through the step
def _three_steps(augment, narrow, seed=5):
    gan, reals, rnd = build(R1, seed, augment)
    thetas = []
    for i in range(3):
        r = AR.add_gates(DR.draw_aug(LN.draw(gan.discriminator, B, gan.generator.latent_size, np.random.default_rng(seed + 10 * i)), B, seed + i), B,
                         seed + i)
        if narrow:
            r = {k: (v[:, :8] if k.startswith("aug_") else v) for k, v in r.items()}
        gan.train_on_batch(np.roll(reals, i, axis=0), randomness=r)
    for m in (gan.generator, gan.discriminator):
        thetas += [m.store.theta.clone(), m.store.m.clone(), m.store.v.clone()]
    return gan, thetas


def test_p_one_is_diffaugment_bit_for_bit_after_three_steps():
    a, ta = _three_steps(bg.AdaptiveAugment(FULL, p=1.0, target=None), narrow=False)
    d, td = _three_steps(bg.DiffAugment(FULL), narrow=True)
    assert isinstance(a.augment, bg.AdaptiveAugment) and type(d.augment) is bg.DiffAugment
    assert all(torch.equal(x, y) for x, y in zip(ta, td))
    assert not torch.equal(ta[3], _three_steps(None, narrow=True)[1][3])            # and the augmentation did act


def test_p_zero_is_the_unaugmented_model_bit_for_bit_after_three_steps():
    a, ta = _three_steps(bg.AdaptiveAugment(FULL, p=0.0, target=None), narrow=False)
    n, tn = _three_steps(None, narrow=True)
    assert n.augment is None and a.augment_p == 0.0
    assert all(torch.equal(x, y) for x, y in zip(ta, tn))


# ------------------------------------------------------------------ 3. the adaptive run against the Python rule
INTERVAL, SPEED = 2, 32           # an adjustment is 2 * 4 / 32 = 1/4: exact


def _adaptive_case(seed0, device=None):
    cfg = bg.AdaptiveAugment(FULL, p=0.5, target=0.0, interval=INTERVAL, speed_images=SPEED)
    gan, reals, _ = build(R1, seed0, cfg, device=device)
    steps = []
    for i in range(2 * INTERVAL + 1):
        seed = seed0 + 100 * i
        rnd = AR.add_gates(DR.draw_aug(LN.draw(gan.discriminator, B, gan.generator.latent_size, np.random.default_rng(seed)), B, seed), B, seed)
        steps.append((np.roll(reals, i, axis=0) * np.float32(1 if i % 2 == 0 else -1), rnd))
    return gan, steps


def adaptive_reference_run(gan, steps):
    """The reference's real scores of every step at the p the Python rule holds then, and the rule's state after each step."""
    rule = AR.Controller(0.5, 0.0, INTERVAL, SPEED)
    out = []
    for reals, rnd in steps:
        ref = AR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, GBS, gan.objective, gan.augment, float(rule.p),
                                e_drift=float(gan.hparams.e_drift))
        rs = ref["rs"]
        # on the reference alone: the signs are decided
        assert np.abs(rs).min() > SIGN_MARGIN * max(1.0, float(np.abs(rs).max())), rs
        out.append((rs, rule.step(rs.astype(np.float32)).copy()))
    return out


@pytest.mark.parametrize("seed", ADAPTIVE_SEEDS)
def test_adaptive_p_follows_the_python_rule(seed):
    gan, steps = _adaptive_case(seed)
    _freeze(gan)                  # the reference reads the product's weights: they stay what they are
    want = adaptive_reference_run(gan, steps)
    ps = [float(s[0]) for _, s in want]
    print("[adaptive run] reference real scores per step:", [np.round(r, 3).tolist() for r, _ in want], "p:", ps)
    assert len(set(ps)) > 1, ps                                              # p moves
    for i, ((reals, rnd), (rs, state)) in enumerate(zip(steps, want)):
        m = dict(zip(gan.metrics_names, gan.train_on_batch(reals, randomness=rnd)))
        assert gan.augment_p == float(state[0]), (i, gan.augment_p, state)
        assert np.array_equal(gan._ada_state.cpu().numpy(), state), (i, gan._ada_state, state)
        assert m["augment_p"] == float(state[0]) and m["augment_rt"] == float(state[4]), (i, m, state)


# ------------------------------------------------------------------ 4. replay and checkpoints, with drawn randomness
def _member(replay, seed=21, augment=None, **kw):
    bg.set_seed(seed)
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    augment = augment or bg.AdaptiveAugment(FULL, p=0.5, target=0.6, interval=INTERVAL, speed_images=64)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, augment=augment,
                            objective="nonsaturating", **kw)


def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v"):
            assert torch.equal(getattr(ma.store, name), getattr(mb.store, name)), name
    assert torch.equal(a._ada_state, b._ada_state), (a._ada_state, b._ada_state)
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(n)]


def test_replayed_steps_equal_eager_steps_bit_for_bit():
    eager, prog = _member(False), _member(True)
    ps = []
    for i, reals in enumerate(_batches(2 * INTERVAL + 1, 3)):
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
        ps.append(prog.augment_p)
        assert dict(zip(prog.metrics_names, prog._organize_metrics()))["augment_p"] == ps[-1]
    # of a key's runs the first is eager and the second recorded (the first step's keys differ once more: its weights are fresh), so
    # from step 3 on the critic's step is a replay, and the controller's adjustment after step 4 happened inside one
    assert prog._programs.stats["replayed"] >= 4, prog._programs.stats
    assert eager._programs.stats["replayed"] == 0
    assert ps[0] == 0.5 and ps[1] != 0.5 and ps[3] != ps[1], ps                                      # p moved, eagerly and under replay
    assert ("aug_d", (3 * B, 12), torch.float32) in prog._bufs and ("aug_g", (B, 12), torch.float32) in prog._bufs      # ONE draw per pass, 12 wide


def test_checkpoint_resume_mid_interval_is_bit_identical(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    batches = _batches(INTERVAL + 3, 6)
    ref = _member(True)
    for reals in batches[:INTERVAL + 1]:
        ref.train_on_batch(reals)
    assert ref._ada_state[3].item() == 1 and ref._ada_state[2].item() == B               # mid-interval, a non-empty accumulator
    path = CheckpointManager(ref, str(tmp_path)).save(1)
    resumed = _member(True, seed=5)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    for reals in batches[INTERVAL + 1:]:
        ma, mb = (dict(zip(g.metrics_names, g.train_on_batch(r))) for g, r in ((ref, reals), (resumed, reals.clone())))
        # ("std" is left out: a checkpoint stores the blur's sigma as float32, so the restored model reports float32(0.9))
        assert {k: v for k, v in ma.items() if k != "std"} == {k: v for k, v in mb.items() if k != "std"}
        _same_state(ref, resumed)
    other = _member(True, seed=5, augment=bg.AdaptiveAugment(FULL, p=0.5, target=0.6, interval=INTERVAL + 1, speed_images=64))
    with pytest.raises(ValueError, match="adaptive augmentation"):
        CheckpointManager(other, str(tmp_path)).restore(path)
