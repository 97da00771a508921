"""GPU tests of equalised-learning-rate models (models.DCGAN*(equalized_lr=True)) through whole training steps.

The reference is a PLAIN TWIN: the same architecture without the wrappers, whose weights are the wrapped model's with every wrapped
kernel replaced by float32(c) * W.  The twin runs only code the feature does not touch (the existing suites hold it to torch and the
oracle), the wrapped model's effective weights are the twin's weights bit for bit, and both take the same reals and randomness at
learning rate 0: so metrics and images must be equal, a wrapped kernel's gradient must be float32(c) * the twin's bit for bit, and
every other gradient the twin's.  This rests on the conv and GEMM routes depending on shapes and 16-byte alignment alone, never on
which buffer holds the weights.  Each test first runs the twin twice and asserts that it equals itself."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models, optimizers
from blurred_gan_amd.checkpoint import CheckpointManager
import pixelnorm_reference as PR

pytestmark = pytest.mark.gpu

EQ = layers.EqualizedLearningRate
CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}      # tests/test_spectral_step_gpu.py's


def _entries(model):
    own = {id(l) for l in model._own_layers()}
    return [e for e in model.store.entries if id(e[0]) in own]


def _effective_weights(model):
    """get_weights() with every wrapped kernel replaced by float32(c) * W."""
    out = []
    for (l, n, _, _, _), w in zip(_entries(model), model.get_weights()):
        if isinstance(l, EQ) and n == "kernel":
            w = np.float32(l.coefficient) * w
            assert w.dtype == np.float32
        out.append(w)
    return out


def _make(arch, B, seed, wrapped, gen_kw, disc_kw, **kw):
    g = dict(dict(normalization="batch"), **gen_kw, equalized_lr=wrapped)
    return PR.make_gan(arch, B, seed, gen_kw=g, disc_kw=dict(disc_kw, equalized_lr=wrapped), **kw)


def _run(gan, reals, rnd):
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    metrics = gan.train_on_batch(reals, randomness=rnd)
    grads = {tag: [(l, n, m.store.view_like(m.store.grad, l, n).detach().cpu().numpy().copy()) for (l, n, _, _, tr) in _entries(m) if tr]
             for tag, m in (("g", gan.generator), ("d", gan.discriminator))}
    return metrics, gan.images[0].detach().cpu().numpy().copy(), grads


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _twin_case(arch="tiny", B=4, seed=3, gen_kw=None, disc_kw=None, **kw):
    gen_kw, disc_kw = gen_kw or {}, disc_kw or {}
    eq, reals, rnd = _make(arch, B, seed, True, gen_kw, disc_kw, **kw)
    twins = []
    for _ in range(2):
        twin, _, _ = _make(arch, B, seed, False, gen_kw, disc_kw, **kw)
        twin.generator.set_weights(_effective_weights(eq.generator))
        twin.discriminator.set_weights(_effective_weights(eq.discriminator))
        twins.append(_run(twin, reals, rnd))
    (m0, img0, g0), (m1, img1, g1) = twins
    assert m0 == m1 and np.array_equal(_bits(img0), _bits(img1)), "the plain twin does not repeat itself"
    for tag in ("g", "d"):
        for (_, n, a), (_, _, b) in zip(g0[tag], g1[tag]):
            assert np.array_equal(_bits(a), _bits(b)), f"the plain twin does not repeat itself: {tag} {n}"
    G, D = eq.generator.net(), eq.discriminator.net()
    assert G.eqlr_layers and D.eqlr_layers and not G.plain_conv_layers and not D.plain_conv_layers
    m, img, g = _run(eq, reals, rnd)
    assert m == m0, (m, m0)
    assert np.array_equal(_bits(img), _bits(img0)), "gan.images differ from the twin's"
    seen = 0
    for tag in ("g", "d"):
        assert len(g[tag]) == len(g0[tag])
        for (l, n, got), (_, n0, ref) in zip(g[tag], g0[tag]):
            assert n == n0 and np.isfinite(ref).all() and np.abs(ref).max() > 0, (tag, n)
            if isinstance(l, EQ) and n == "kernel":
                ref = np.float32(l.coefficient) * ref
                seen += 1
            assert np.array_equal(_bits(got), _bits(ref)), (tag, l.kind, n, tuple(ref.shape), float(np.abs(got - ref).max()))
    assert seen == len(G.eqlr_layers) + len(D.eqlr_layers)
    return eq


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_step_equals_the_plain_twin_in_every_d_step_configuration(config):
    gan = _twin_case(**CONFIGS[config])
    assert len(gan.discriminator.net().eqlr_layers) == 3 and len(gan.generator.net().eqlr_layers) == 5


def test_step_equals_the_plain_twin_behind_the_blur():
    assert _twin_case(std=0.9).discriminator.net().blur is not None


def test_step_equals_the_plain_twin_on_the_source_route():
    gan = _twin_case(disc_kw=dict(normalization="layer", minibatch_stddev=2))
    assert gan.discriminator.net().has_ln and gan.discriminator.net().mbstd_layers and gan.discriminator.net().has_source


def test_step_equals_the_plain_twin_in_split_bf16_conv_math():
    assert _twin_case(conv_math="bf16x6").discriminator.net().conv_math == "bf16x6"


def test_step_equals_the_plain_twin_under_the_nonsaturating_loss_with_r1():
    gan = _twin_case(objective=bg.Objective("nonsaturating", penalty_target=0, penalty_on="reals"))
    assert gan._objective.loss == "nonsaturating"


@pytest.mark.parametrize("variant", ["pool", "resize", "pixel"])
def test_step_equals_the_plain_twin_on_the_odd_stack(variant):
    kw = {"pool": dict(disc_kw=dict(downsampling="pool")), "resize": dict(gen_kw=dict(upsampling="resize")), "pixel": dict(gen_kw=dict(normalization="pixel"))}[variant]
    gan = _twin_case(arch="tiny_mnist", **kw)
    assert {l.vars["kernel"].shape[-1] for l in gan.discriminator.net().eqlr_layers} == {4, 8, 1}      # odd channel counts: the scalar routes
    kinds = [st.kind for st in gan.generator.net().stages] + [st.kind for st in gan.discriminator.net().stages]
    assert {"pool": "avgpool" in kinds, "resize": "upsample" in kinds, "pixel": gan.generator.net().has_pn}[variant]


# ------------------------------------------------------------------ after an update
def _assert_effective_weights_are_current(model):
    net, st = model.net(), model.store
    assert net.eqlr_layers
    for l in net.eqlr_layers:
        W = l.vars["kernel"].cpu().numpy()
        want = np.float32(l.coefficient) * W
        eff = st.kernel(l).cpu().numpy()
        assert eff.shape == W.shape and np.array_equal(_bits(eff), _bits(want)), (l.kind, W.shape)
        K, N, taps = layers.SpectralNormalization.matrix_shape(W.shape)
        if l.kind == "dense":
            assert st.kernel(l, transposed=True) is None
        else:
            tr = st.kernel(l, transposed=True).cpu().numpy().reshape(taps, N, K // taps)
            assert np.array_equal(_bits(tr), _bits(want.reshape(taps, K // taps, N).transpose(0, 2, 1)))


def test_after_an_update_the_passes_see_the_new_weights_times_c():
    gan, reals, rnd = _make("tiny", 4, 3, True, {}, {})
    gan.discriminator.optimizer = optimizers.SGD(0.05)
    gan.generator.optimizer = optimizers.SGD(0.0)
    D = gan.discriminator
    before = D.store.theta.clone()
    gan.train_on_batch(reals, randomness=rnd)         # the D-step moves W; the G-step's critic pass refreshes c * W
    assert not torch.equal(before, D.store.theta)
    _assert_effective_weights_are_current(D)
    _assert_effective_weights_are_current(gan.generator)
    # the SGD step took c * dL/dW_eff: theta moved by exactly lr * the gradient buffer
    assert torch.allclose(D.store.theta, before - 0.05 * D.store.grad, rtol=0, atol=2e-6)


# ------------------------------------------------------------------ replay and checkpoints
def _pair_member(replay, seed=21, B=4, **kw):
    bg.set_seed(seed)
    gen = models.DCGANGenerator(arch="tiny", equalized_lr=True)
    disc = models.DCGANDiscriminator(arch="tiny", equalized_lr=True)
    hp = bg.BlurredWGANGP.HyperParameters(initial_blur_std=0.9, global_batch_size=B, batch_size=B)
    return bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"), step_replay=replay, **kw)


def _same_state(a, b):
    for ma, mb in ((a.generator, b.generator), (a.discriminator, b.discriminator)):
        for name in ("theta", "state", "m", "v", "s3", "grad"):
            x, y = getattr(ma.store, name), getattr(mb.store, name)
            assert (x is None) == (y is None), name
            assert x is None or torch.equal(x, y), name
        for la, lb in zip(ma.net().eqlr_layers, mb.net().eqlr_layers):       # the effective weights, through the engine's accessor
            assert torch.equal(ma.store.kernel(la), mb.store.kernel(lb))
            assert la.kind == "dense" or torch.equal(ma.store.kernel(la, transposed=True), mb.store.kernel(lb, transposed=True))
        assert ma.optimizer.iterations == mb.optimizer.iterations
    assert a._rng_off == b._rng_off and int(a.n_batches) == int(b.n_batches)


def test_replayed_steps_equal_eager_steps_bit_for_bit():
    B = 4
    eager, prog = _pair_member(False), _pair_member(True)
    g = torch.Generator().manual_seed(3)
    for i in range(6):
        reals = (torch.rand(B, 8, 8, 3, generator=g) * 2 - 1).cuda()
        assert eager.train_on_batch(reals) == prog.train_on_batch(reals.clone()), i
        _same_state(eager, prog)
    assert prog._programs.stats["replayed"] >= 4, prog._programs.stats
    assert not torch.equal(prog.generator.store.theta, _pair_member(False).generator.store.theta)         # the steps moved the weights


def test_checkpoint_resume_is_bit_identical(tmp_path):
    g = torch.Generator().manual_seed(6)
    batches = [(torch.rand(4, 8, 8, 3, generator=g) * 2 - 1).cuda() for _ in range(6)]
    ref = _pair_member(True)
    for reals in batches[:3]:
        ref.train_on_batch(reals)
    path = CheckpointManager(ref, str(tmp_path)).save(3)
    for reals in batches[3:]:
        ref.train_on_batch(reals)
    resumed = _pair_member(True, seed=5)
    assert not torch.equal(resumed.discriminator.store.theta, ref.discriminator.store.theta)
    CheckpointManager(resumed, str(tmp_path)).restore(path)
    for reals in batches[3:]:
        resumed.train_on_batch(reals)
    for a, b in ((ref.generator, resumed.generator), (ref.discriminator, resumed.discriminator)):
        assert torch.equal(a.store.theta, b.store.theta) and torch.equal(a.store.state, b.store.state)
        assert torch.equal(a.store.m, b.store.m) and torch.equal(a.store.v, b.store.v) and torch.equal(a.store.eff, b.store.eff)
    plain = bg.BlurredWGANGP(models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny"), ref.hparams, bg.TrainingConfig(log_dir="/tmp/bg_test_logs"))
    with pytest.raises(ValueError, match="coefficients"):
        CheckpointManager(plain, str(tmp_path)).restore(path)


# ------------------------------------------------------------------ the averaged generator
def test_generator_ema_averages_raw_weights_and_samples_with_them_times_c():
    gan = _pair_member(True, generator_ema=0.5)
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        gan.train_on_batch((torch.rand(4, 8, 8, 3, generator=g) * 2 - 1).cuda())
    z = torch.rand(4, 10, generator=g)
    avg = gan.generate_samples(z, ema=True).clone()
    live = gan.generate_samples(z).clone()
    assert torch.isfinite(avg).all() and avg.shape == live.shape and not torch.equal(avg, live)
    E, G = gan.generator_ema, gan.generator
    assert len(E.net().eqlr_layers) == 5 and E.store.eff is not G.store.eff and not torch.equal(E.store.theta, G.store.theta)
    for a, b in zip(E.net().eqlr_layers, G.net().eqlr_layers):
        assert a.coefficient == b.coefficient and a.layer.vars is a.vars and a.vars["kernel"].data_ptr() != b.vars["kernel"].data_ptr()
    _assert_effective_weights_are_current(E)          # c * (the average of W) = the average of c * W
    _assert_effective_weights_are_current(G)
    # the averaged model is the plain twin of its own effective weights
    bg.set_seed(1)
    twin = models.DCGANGenerator(arch="tiny")
    twin.set_weights(_effective_weights(E))
    assert torch.equal(twin(z.cuda(), training=False), avg)
