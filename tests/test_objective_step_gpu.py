"""GPU tests of ``objective=`` through whole training steps, against the float64 reference of tests/objective_reference.py, in the
pattern of tests/test_diffaug_step_gpu.py.  All cases: batch 4, global batch 5, learning rate 0 unless a case says otherwise.

Tolerance of every gradient comparison: per tensor rtol 2e-3, atol 2e-4 * max|reference| (tests/ln_reference.py).  Each comparison
first asserts, on the reference alone, that no LeakyReLU pre-activation of any reference pass lies within 5e-6 of zero, that no
penalty-point gradient norm is below 1e-3 (spectrally normalised critic: and the signal ratio of tests/sn_reference.py) and, for a hinge
case, that among the fake scores there is one on each side of -1, among the real scores one on each side of +1 and none within 1e-3
of its hinge.

Score scale.  The stock tiny critic scores within +-0.4 behind the blur: no score reaches a hinge.  SCALE = 10 multiplies its last
Dense kernel and bias.  Seeds and scale were chosen by running the reference alone on a CPU (objective_reference.make_gan(...,
device="cpu")); it gave, for tiny behind the blur (std 0.9) at scale 10, seeds 1-8, min |pre-activation| and the scores
  1: 1.2e-5  fs [-1.36 0.03 -0.56 -2.14]   rs [-1.40 -0.96 -1.11 0.23]    no real score above +1
  2: 2.7e-5  fs [0.71 -1.29 0.48 0.08]     rs [-0.18 -1.18 0.29 2.01]     taken
  3: 3.0e-5  fs [2.90 2.76 0.52 1.75]      rs [1.79 1.58 3.08 -1.24]      no fake score below -1
  4: 2.3e-6, 5: 4.6e-6, 6: 4.6e-6, 8: 1.2e-7   too close to a LeakyReLU kink;   7: 2.4e-5, every score below -1
and for the critic of case 2 (convolutions spectrally normalised, plain Dense head, WGAN class, no blur) at scale 10
  7: 5.6e-5  fs [-0.97 -2.47 -0.87 -1.54]  rs [2.35 -5.47 0.41 -1.03]     taken (seeds 1-6 and 8 miss a side or lie at a kink)
The figures of every case below, from the same run, stand in CASES."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import models
from helpers import product_grads
from ln_reference import ATOL, RTOL, assert_close
import objective_reference as OR

pytestmark = pytest.mark.gpu

SCALE, STD = 10.0, 0.9
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
R1 = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals")
FULL = "color,translation,cutout"
# name -> (objective, seed, keywords of make_gan): what the reference alone gave stands beside each (min |pre-activation|, min norm[, signal])
CASES = {
    "hinge": (bg.Objective("hinge"), 2, dict(std=STD, score_scale=SCALE)),                                             # 2.7e-5, 0.46
    "nonsaturating": (bg.Objective("nonsaturating"), 2, dict(std=STD, score_scale=SCALE)),                             # 2.7e-5, 0.46
    "hinge_wgan_sn": (bg.Objective("hinge"), 7, dict(cls="wgan", disc=OR.sn_critic_with_plain_head, score_scale=SCALE)),  # 5.6e-5, -, 1.00
    # every layer normalised, the Dense head too: W / sigma undoes any score scale, the scores stay within (-0.6, 0.3)
    "hinge_wgan_sn_all": (bg.Objective("hinge"), 1, dict(cls="wgan", critic_sn=True)),                                 # 2.0e-5, -, 1.00
    # the Wasserstein loss through the new kernels: any penalty but the default takes bg_gan_d_loss<WASSERSTEIN> and bg_gp_seed_target_f32
    "wasserstein_r1": (bg.Objective(penalty_target=0.0, penalty_on="reals"), 2, dict(std=STD, score_scale=SCALE)),     # 2.7e-5, 0.46
    "r1": (R1, 2, dict(std=STD, score_scale=SCALE)),                                                                   # 2.7e-5, 0.46
    # LayerNormalization scores within +-3.3 as it stands (at scale 10 within +-23, the penalty at 1500: a conditioning of its own)
    "r1_layer": (R1, 2, dict(std=STD, normalization="layer")),                                                        # 2.1e-5, 1.1
    "r1_spectral": (R1, 3, dict(std=STD, critic_sn=True)),                                                            # 1.8e-5, 0.072, 0.83
    "r1_pool": (R1, 1, dict(std=STD, score_scale=SCALE, down="pool")),                          # 1.4e-5, 0.23 (seeds 2-5: below 3e-6)
    "r1_augment": (R1, 3, dict(std=STD, score_scale=SCALE, augment=FULL)),                                            # 1.5e-5, 0.32
    "r2": (bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="fakes"), 2, dict(std=STD, score_scale=SCALE)),        # 2.7e-5, 0.45
    "t0_interpolates": (bg.Objective("nonsaturating", penalty_target=0.0), 2, dict(std=STD, score_scale=SCALE)),              # 2.7e-5, 0.46
    # n_batches 0: 2.7e-5, 0.46, gp_term 5.14 (r1's 2.57 twice); n_batches 1: 2.7e-5, no penalty pass
    "lazy": (bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals", penalty_interval=2), 2, dict(std=STD, score_scale=SCALE)),
}


def build(name, device=None, **kw):
    obj, seed, mk = CASES[name]
    return OR.make_gan("tiny", 4, seed, obj, gbs=5, device=device, **mk, **kw)


def reference(gan, reals, rnd, penalty_step=True, hinge_sides=True, e_drift=1e-4):
    ref = OR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, 5, gan.objective, penalty_step=penalty_step, augment=gan.augment,
                            penalty_class=gan.uses_gradient_penalty, e_drift=e_drift)
    OR.check_conditions(ref, hinge_sides)
    return ref


def _freeze(gan):
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0


def _step_case(name, kw=None, n_batches=0, rnd_extra=None, hinge_sides=True, e_drift=None):
    gan, reals, rnd = build(name, **(kw or {}))
    gan.n_batches.assign(n_batches)
    if e_drift is not None:
        gan.hparams.e_drift = e_drift
    ref = reference(gan, reals, rnd, penalty_step=gan._penalty_this_step(), hinge_sides=hinge_sides,
                    e_drift=float(getattr(gan.hparams, "e_drift", 0.0)))
    _freeze(gan)
    rnd.update(rnd_extra or {})
    values = gan.train_on_batch(reals, randomness=rnd)
    assert_close(product_grads(gan.discriminator), ref["dgrads"], "critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], "generator gradients")
    return gan, ref, dict(zip(gan.metrics_names, values))


def _check_losses(m, ref):
    for key in ("disc_loss", "gen_loss") + (("norm_term",) if "norm_term" in m else ()):
        print(f"[{key}] product {m[key]!r} reference {ref[key]!r}")
        np.testing.assert_allclose(m[key], ref[key], rtol=RTOL, atol=ATOL * max(abs(ref[key]), 1e-6), err_msg=key)


# ------------------------------------------------------------------ 1. the two new losses, every critic-step configuration
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("loss", ["hinge", "nonsaturating"])
def test_step_gradients_match_torch(loss, config):
    gan, ref, m = _step_case(loss, CONFIGS[config])
    assert gan.objective == bg.Objective(loss) and gan.discriminator.net().blur is not None
    _check_losses(m, ref)                                   # 9. the metrics follow the loss
    np.testing.assert_allclose(m["gp_term"], ref["gp_term"], rtol=RTOL, atol=ATOL * ref["gp_term"])


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_wasserstein_loss_with_r1_runs_the_new_kernels_and_matches_torch(config):
    gan, ref, m = _step_case("wasserstein_r1", CONFIGS[config])
    assert gan.objective.loss == "wasserstein" and not gan.objective.is_reference
    _check_losses(m, ref)
    np.testing.assert_allclose(m["gp_term"], ref["gp_term"], rtol=RTOL)


# ------------------------------------------------------------------ 2. the SN-GAN set-up
def test_hinge_on_the_wgan_class_with_a_spectrally_normalised_critic():
    gan, ref, m = _step_case("hinge_wgan_sn")
    assert type(gan) is bg.WGAN and len(gan.discriminator.net().spectral_layers) == 2 and "gp_term" not in m
    _check_losses(m, ref)


def test_hinge_on_the_wgan_class_with_every_layer_of_the_critic_spectrally_normalised():
    """models.DCGANDiscriminator(spectral_norm=True) as it stands, the SN-GAN set-up to the letter.  Its scores cannot reach a hinge
    (every hinge term is active), which is why the case above exists beside it: here only the distance to the hinges is asserted."""
    gan, ref, m = _step_case("hinge_wgan_sn_all", hinge_sides=False)
    assert type(gan) is bg.WGAN and len(gan.discriminator.net().spectral_layers) == 3
    assert np.abs(ref["fs"]).max() < 1 and np.abs(ref["rs"]).max() < 1
    _check_losses(m, ref)


# ------------------------------------------------------------------ 3. R1
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_r1_gradients_match_torch_and_an_injected_alpha_is_ignored(config):
    gan, ref, m = _step_case("r1", CONFIGS[config])
    _check_losses(m, ref)
    other, _, m2 = _step_case("r1", CONFIGS[config], rnd_extra=dict(alpha=np.full(4, 0.7, np.float32)))
    assert m == m2
    for a, b in zip(product_grads(gan.discriminator) + product_grads(gan.generator), product_grads(other.discriminator) + product_grads(other.generator)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert torch.equal(gan._buf("alpha", (4,)), torch.zeros(4, device="cuda"))


@pytest.mark.parametrize("name", ["r1_layer", "r1_spectral", "r1_pool", "r1_augment"])
def test_r1_gradients_match_torch_on_the_other_critics(name):
    gan, _, _ = _step_case(name)
    D = gan.discriminator.net()
    assert {"r1_layer": D.has_ln, "r1_spectral": len(D.spectral_layers) == 3, "r1_pool": any(st.kind == "avgpool" for st in D.stages),
            "r1_augment": gan.augment == bg.DiffAugment()}[name]


def test_r1_gradients_match_torch_in_split_bf16_conv_math():
    gan, _, _ = _step_case("r1", dict(conv_math="bf16x6"))
    assert gan.discriminator.net().conv_math == "bf16x6"


# ------------------------------------------------------------------ 4. / 5. the other penalty points and targets
def test_penalty_on_the_fakes():
    gan, _, _ = _step_case("r2")
    assert torch.equal(gan._buf("alpha", (4,)), torch.ones(4, device="cuda"))


def test_target_zero_on_interpolates():
    _step_case("t0_interpolates")


# ------------------------------------------------------------------ 6. lazy penalty
def test_lazy_penalty_step_carries_the_interval_times_the_coefficient():
    gan, ref, m = _step_case("lazy", n_batches=0)
    assert gan._penalty_this_step() is False and int(gan.n_batches) == 1          # the next step is a skipped one
    assert ref["gp_term"] > 0
    np.testing.assert_allclose(m["gp_term"], ref["gp_term"], rtol=RTOL)           # 2 * gp_coefficient * mean(n^2)
    _check_losses(m, ref)


E_DRIFT_VISIBLE = 0.05      # against w = 4 / 5: the default 1e-4 would be a relative 1.25e-4, below the bound of the comparison


def test_lazy_skipped_step_keeps_drift_and_vector_scale_and_runs_no_penalty():
    gan, ref, m = _step_case("lazy", n_batches=1, e_drift=E_DRIFT_VISIBLE)
    assert ref["gp_term"] == 0 and m["gp_term"] == 0.0 and ref["norm"] == float("inf")
    assert ref["norm_term"] > 1e-2
    _check_losses(m, ref)                                   # disc_loss, gen_loss and norm_term
    # the drift term is in those gradients: the reference without it is far outside the bound
    gan0, reals0, rnd0 = build("lazy")
    no_drift = OR.ref_step_grads(gan0.generator, gan0.discriminator, reals0, rnd0, 5, gan0.objective, penalty_step=False, e_drift=0.0)
    ratios = [float(np.abs(a - b.reshape(a.shape)).max() / (RTOL * np.abs(b).max())) for a, b in zip(product_grads(gan.discriminator), no_drift["dgrads"])]
    print("[drift] max |difference| / (rtol * max|reference without drift|) per tensor:", ratios)
    assert max(ratios) > 10, ratios
    # and the vector-loss scale is in those gradients: the scalar-loss reference (the WGAN class's) is far outside the bound
    gan2, reals, rnd = build("lazy")
    plain = OR.ref_step_grads(gan2.generator, gan2.discriminator, reals, rnd, 5, gan2.objective, penalty_class=False)
    got, want = product_grads(gan.discriminator)[0], plain["dgrads"][0].reshape(product_grads(gan.discriminator)[0].shape)
    assert np.abs(got - want).max() > 100 * (RTOL * np.abs(want).max())


# ------------------------------------------------------------------ 7. replay
def _pair_member(replay, objective, seed=21, B=4, **kw):
    bg.set_seed(seed)
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, objective=objective, **kw)


def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def _batches(n, seed, B=4):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(n)]


def test_replayed_lazy_steps_equal_eager_steps_bit_for_bit():
    """Four steps at learning rate 1e-3, replay against eager, bit for bit in weights and metrics -- and five more.  A step-program key
    runs eagerly at its first use, is recorded at its second and replays from its third (program.StepPrograms), and the first critic
    step of a model has a key of its own (both networks' transposed kernels are stale; from the second step on the generator step has
    refreshed the critic's).  Counting from 0: the step without penalty runs eagerly at step 1, is recorded at 3 and replays at 5 and
    7; the step with penalty runs eagerly at 2, is recorded at 4 and replays at 6 and 8.  So nine steps: both kinds of critic step
    -- the constant-alpha fill, both bg_gan_d_loss launches of the merged pass and bg_gp_seed_target_f32 among the launches of the
    one with penalty -- run twice from their programs."""
    lazy = CASES["lazy"][0]
    eager, prog = _pair_member(False, lazy), _pair_member(True, lazy)
    gp, log = [], []
    run = prog._programs.run

    def spy(key, *a, **kw):             # (kind, penalty this step, ran from a recorded program) of every step of the replaying model
        out = run(key, *a, **kw)
        log.append((key[0], next(e[2] for e in key if isinstance(e, tuple) and e and e[0] == "objective"), prog._programs.last_was_replay))
        return out
    prog._programs.run = spy
    for i, reals in enumerate(_batches(9, 3)):
        a, b = eager.train_on_batch(reals), prog.train_on_batch(reals.clone())
        assert a == b, i
        _same_state(eager, prog)
        gp.append(dict(zip(prog.metrics_names, b))["gp_term"])
    assert all(v > 0 for v in gp[0::2]) and all(v == 0.0 for v in gp[1::2]), gp
    from blurred_gan_amd import program
    stats = prog._programs.stats
    print("[replay]", stats)
    # exactly two critic-step programs -- with and without the penalty -- and the generator's one, which does not depend on the phase
    recorded = [k for k, e in prog._programs.entries.items() if isinstance(e, program.Recorder)]
    d_keys = [k for k in recorded if k[0] == "d"]
    assert len(d_keys) == 2 and len(recorded) == 3, recorded
    assert sorted(next(e[2] for e in k if isinstance(e, tuple) and e and e[0] == "objective") for k in d_keys) == [False, True]
    assert stats["recorded"] == 3 and stats["replayed"] == 11 and stats["evicted"] == 0, stats      # critic steps 5-8, generator steps 2-8
    d_log = [(pen, rep) for kind, pen, rep in log if kind == "d"]
    assert d_log == [(True, False), (False, False), (True, False), (False, False), (True, False),
                     (False, True), (True, True), (False, True), (True, True)], d_log
    assert [rep for kind, _, rep in log if kind == "g"] == [False, False] + [True] * 7


# ------------------------------------------------------------------ 8. the default objective, spelled three ways
def test_the_default_objective_spelled_three_ways_is_one_step_bit_for_bit():
    out = []
    for spelling in (None, bg.Objective(), "wasserstein"):
        gan, reals, rnd = OR.make_gan("tiny", 4, 2, spelling, gbs=5, std=STD)
        gan.discriminator.optimizer.learning_rate = gan.generator.optimizer.learning_rate = 1e-3
        if not out:
            ref = reference(gan, reals, rnd)                # of the weights the step starts from.  Reference alone, seed 2 unscaled: 2.7e-5, 0.046
        values = gan.train_on_batch(reals, randomness=rnd)
        assert gan.objective == bg.Objective() and gan.objective.is_reference
        out.append((values, product_grads(gan.discriminator) + product_grads(gan.generator),
                    [gan.discriminator.store.theta.clone(), gan.generator.store.theta.clone()]))
    # and that step is the reference's -- Wasserstein loss, two-sided penalty on interpolates: the critic's part here (its step comes
    # before any update), the whole step once more at learning rate 0 (the generator's step sees the critic its step left behind)
    assert_close(out[0][1][:len(ref["dgrads"])], ref["dgrads"], "critic gradients")
    m = dict(zip(gan.metrics_names, out[0][0]))
    np.testing.assert_allclose(m["disc_loss"], ref["disc_loss"], rtol=RTOL)
    gan, reals, rnd = OR.make_gan("tiny", 4, 2, None, gbs=5, std=STD)
    ref = reference(gan, reals, rnd)
    _freeze(gan)
    m = dict(zip(gan.metrics_names, gan.train_on_batch(reals, randomness=rnd)))
    assert_close(product_grads(gan.discriminator), ref["dgrads"], "critic gradients")
    assert_close(product_grads(gan.generator), ref["ggrads"], "generator gradients")
    _check_losses(m, ref)
    for values, grads, thetas in out[1:]:
        assert values == out[0][0]
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(grads, out[0][1]))
        assert all(torch.equal(a, b) for a, b in zip(thetas, out[0][2]))


# ------------------------------------------------------------------ 10. checkpoints
def test_a_checkpoint_after_an_odd_number_of_batches_resumes_on_the_right_phase(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    lazy = CASES["lazy"][0]
    batches = _batches(5, 6)
    ref = _pair_member(True, lazy)
    for reals in batches[:3]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path)).save(3)
    resumed = _pair_member(True, lazy, seed=5)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    assert int(resumed.n_batches) == 3 and not resumed._penalty_this_step()
    for k, reals in enumerate(batches[3:]):
        a, b = (dict(zip(m.metrics_names, m.train_on_batch(r))) for m, r in ((ref, reals), (resumed, reals.clone())))
        # the blur's std comes back from a checkpoint as the float32 it was saved as: equal to float32, and the blur's taps with it
        assert np.float32(a.pop("std")) == np.float32(b.pop("std"))
        assert a == b and (a["gp_term"] > 0) == (k == 1), (k, a, b)
        for ma, mb in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
            assert torch.equal(ma.store.grad, mb.store.grad) and torch.equal(ma.store.theta, mb.store.theta)
    # the objective is configuration, not state: the checkpoint loads into a model with another one
    other = _pair_member(True, "hinge", seed=7)
    CheckpointManager(other, str(tmp_path)).restore(path)
    assert other.objective == bg.Objective("hinge")
    other.train_on_batch(batches[3])
