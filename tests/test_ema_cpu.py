"""CPU tests of generator weight averaging (blurred_gan_amd.ema, WGAN(generator_ema=...)): the schedule object, the argument
errors of bg_ema_f32 and its step-program binding (no device work is launched), the ISA of the update kernel, and the host side
of the averaged model (structural copy, no draw from the weight-initialisation RNG, step key, checkpoint keys)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models
from blurred_gan_amd.ema import GeneratorEMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the schedule
def test_exported_from_the_package():
    assert bg.GeneratorEMA is GeneratorEMA and "GeneratorEMA" in bg.__all__


def test_argument_errors():
    for kw in ({}, {"decay": 0.9, "halflife_images": 100.0}, {"decay": 1.0}, {"decay": -0.1}, {"decay": 1.5}, {"decay": "big"},
               {"decay": True}, {"halflife_images": 0}, {"halflife_images": -5.0}):
        with pytest.raises(ValueError):
            GeneratorEMA(**kw)
    GeneratorEMA(decay=0.0)
    GeneratorEMA(halflife_images=1)


def test_w_at_plain_decay():
    e = GeneratorEMA(decay=0.999)
    for k in (0, 1, 7, 10 ** 6):
        assert e.w_at(k, 8, 1, 1) == 1.0 - 0.999
    # formed in double and rounded once: NOT the float32 subtraction
    assert np.float32(e.w_at(0, 8, 1, 1)) != np.float32(1.0) - np.float32(0.999)


def test_w_at_warmup():
    e = GeneratorEMA(decay=0.9, warmup=True)
    assert e.w_at(0, 8, 1, 1) == 0.9
    for k in range(200):
        assert e.w_at(k, 8, 1, 1) == 1.0 - min(0.9, (1.0 + k) / (10.0 + k))
    assert e.w_at(80, 8, 1, 1) == 1.0 - 0.9 and e.w_at(81, 8, 1, 1) == 1.0 - 0.9     # (1 + 80) / (10 + 80) == 0.9: capped from there on
    assert len({e.w_at(k, 8, 1, 1) for k in range(6)}) == 6                           # a different w at each early step


def test_w_at_halflife_rule():
    e = GeneratorEMA(halflife_images=10_000)
    for B in (8, 5):
        assert e.w_at(3, B, 2, 1) == 1.0 - 0.5 ** (B * 2 * 1 / 10_000.0)
        assert e.w_at(3, B, 2, 2) == 1.0 - 0.5 ** (B * 2 * 2 / 10_000.0)
    assert e.w_at(0, 8, 2, 1) != e.w_at(0, 5, 2, 1) and e.w_at(0, 8, 2, 1) != e.w_at(0, 8, 1, 1)
    assert GeneratorEMA(halflife_images=64).w_at(0, 32, 2, 1) == 0.5                  # one half-life per update
    w = GeneratorEMA(halflife_images=100, warmup=True).w_at(0, 4, 1, 1)
    assert w == 1.0 - min(0.5 ** 0.04, 0.1)


@pytest.mark.parametrize("e", [GeneratorEMA(decay=0.99), GeneratorEMA(halflife_images=5000, warmup=True), GeneratorEMA(decay=0.5, warmup=True)])
def test_config_round_trip(e):
    back = GeneratorEMA.from_config(e.get_config())
    assert back.get_config() == e.get_config() and back.static_config() == e.static_config()
    assert [back.w_at(k, 6, 2, 2) for k in range(5)] == [e.w_at(k, 6, 2, 2) for k in range(5)]


# ------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge._load_build_module().build_lib(verbose=False)
    from blurred_gan_amd import _lib
    return _lib.load()


def test_argument_errors_are_statuses_and_launch_nothing(lib):
    from blurred_gan_amd import _lib
    assert "bg_ema_f32" in _lib.SIGNATURES and _lib.BIND_EMA_W == 4
    buf = np.zeros(64, np.float32)
    base = buf.ctypes.data
    base += (-base) % 16                               # a 16-byte aligned host address: never dereferenced by the checks
    a, t, a2, t2 = base, base + 64, base + 128, base + 192
    assert lib.bg_ema_f32(None, None, 4, None, None, 0, 0.1, None) == -6
    assert lib.bg_ema_f32(a, None, 4, None, None, 0, 0.1, None) == -6
    assert lib.bg_ema_f32(a, t, 4, None, None, 2, 0.1, None) == -6             # a second segment needs its pointers
    assert lib.bg_ema_f32(a, t, 4, a2, None, 2, 0.1, None) == -6
    assert b"bg_ema_f32" in lib.bg_last_error()
    assert lib.bg_ema_f32(a, t, 0, None, None, 0, 0.1, None) == -1             # empty
    for w in (1.5, -0.25, float("nan")):
        assert lib.bg_ema_f32(a, t, 4, a2, t2, 4, w, None) == -1               # w outside [0, 1]
    assert lib.bg_ema_f32(a + 4, t, 4, None, None, 0, 0.1, None) == -2
    assert lib.bg_ema_f32(a, t + 8, 4, None, None, 0, 0.1, None) == -2
    assert lib.bg_ema_f32(a, t, 4, a2 + 4, t2, 4, 0.1, None) == -2
    assert lib.bg_ema_f32(a, t, 4, a2, t2 + 12, 4, 0.1, None) == -2
    assert b"aligned" in lib.bg_last_error()
    assert lib.bg_program_bind_next(_lib.BIND_EMA_W, 0) == -3                  # nothing is being recorded
    assert not buf.any()


def test_bind_kind_is_accepted_while_recording(lib):
    from blurred_gan_amd import _lib
    h = C.c_void_p()
    assert lib.bg_program_create(C.byref(h), 4) == 0
    assert lib.bg_program_record_begin(h) == 0
    assert lib.bg_program_bind_next(_lib.BIND_EMA_W, 1) == 0
    assert lib.bg_program_bind_next(5, 1) == -1                                # the kind after the last one
    assert lib.bg_program_record_end(h) == -3                                  # announced, but no launch consumed it
    assert lib.bg_program_destroy(h) == 0
    assert lib.bg_version() == 5                                               # an addition, as bg_sgd_f32 was


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_ema_kernel_does_not_spill_and_moves_float4(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "optim.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "optim.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    names = re.findall(r"\.name:\s+(\S*ema_kernel\S*)\n", isa)
    assert len(names) == 1, names
    meta = re.search(r"\.name:\s+" + re.escape(names[0]) + r"\n(.*?)\.wavefront_size", isa, flags=re.S).group(1)
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        v = re.search(r"\." + key + r":\s+(\d+)", meta)
        assert v and int(v.group(1)) == 0, key
    body = re.search(r"^" + re.escape(names[0]) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
    assert "v_fma_f32" not in body and "v_fmac_f32" not in body                # a - w * (a - t) stays a subtract, a multiply, a subtract


# ------------------------------------------------------------------ the averaged model, host side
def _gan(seed=3, cls=None, **kw):
    bg.set_seed(seed)
    g, d = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    cls = cls or bg.WGANGP
    return cls(g, d, cls.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir="/tmp/bg_ema_logs"), **kw)


def test_keyword_values():
    assert _gan().generator_ema is None and _gan(generator_ema=None).generator_ema is None
    gan = _gan(generator_ema=0.75)
    assert isinstance(gan.generator_ema, bg.Sequential) and gan.generator_ema_config.get_config() == GeneratorEMA(decay=0.75).get_config()
    sched = GeneratorEMA(halflife_images=100)
    assert _gan(generator_ema=sched).generator_ema_config is sched
    assert _gan(cls=bg.BlurredWGANGP, generator_ema=0.5).generator_ema is not None          # every subclass inherits the keyword
    for bad in (1.0, -0.5, "0.9", True):
        with pytest.raises(ValueError):
            _gan(generator_ema=bad)


def test_averaged_model_is_a_structural_copy_in_its_own_store():
    gan = _gan(generator_ema=0.9)
    G, E = gan.generator, gan.generator_ema
    assert E is not G and E.store is not G.store and gan.generator_ema_updates == 0
    assert [type(l) for l in E.layers] == [type(l) for l in G.layers] and all(a is not b for a, b in zip(E.layers, G.layers))
    assert (E.store.n_train, E.store.n_state) == (G.store.n_train, G.store.n_state) and G.store.n_state > 0
    assert np.array_equal(E.store.theta.numpy(), G.store.theta.numpy()) and np.array_equal(E.store.state.numpy(), G.store.state.numpy())
    assert E.store.theta.data_ptr() != G.store.theta.data_ptr() and E.store.state.data_ptr() != G.store.state.data_ptr()
    # the live layers are still bound to the live store, the copies to their own
    lo, hi = G.store.theta.data_ptr(), G.store.theta.data_ptr() + 4 * G.store.theta.numel()
    assert all(lo <= v.data_ptr() < hi for v in G.trainable_variables)
    assert not any(lo <= v.data_ptr() < hi for v in E.trainable_variables)
    assert [tuple(v.shape) for v in E.variables] == [tuple(v.shape) for v in G.variables]
    # no gradient or optimizer slots, no optimizer
    st = E.store
    assert st.grad is None and st.m is None and st.v is None and st.s3 is None and E.optimizer is None
    # writing the copy leaves the live weights alone
    before = G.get_weights()
    E.set_weights([w + 1.0 for w in E.get_weights()])
    assert all(np.array_equal(a, b) for a, b in zip(before, G.get_weights()))
    gan.reset_generator_ema()
    assert all(np.array_equal(a, b) for a, b in zip(before, E.get_weights())) and E.store.tr_dirty


def test_copy_of_a_hand_built_nested_sequential():
    bg.set_seed(5)
    inner = layers.Sequential([layers.Dense(2 * 2 * 8, use_bias=False, input_shape=(6,)), layers.BatchNormalization(), layers.LeakyReLU(),
                               layers.Reshape((2, 2, 8))])
    gen = layers.Sequential([inner, layers.Conv2DTranspose(4, (3, 3), strides=(2, 2), padding="same", use_bias=True),
                             layers.BatchNormalization(), layers.LeakyReLU(),
                             layers.Conv2DTranspose(3, (5, 5), strides=(2, 2), padding="same", use_bias=False, activation="tanh")])
    disc = models.DCGANDiscriminator(arch="tiny")
    gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(), generator_ema=0.5)
    E = gan.generator_ema
    assert isinstance(E.layers[0], layers.Sequential) and E.layers[0] is not inner and E.layers[0]._store is E.store
    assert inner._store is gen.store
    assert all(np.array_equal(a, b) for a, b in zip(E.get_weights(), gen.get_weights())) and len(E.get_weights()) == 12


def test_building_the_average_draws_nothing_from_the_init_rng():
    out = []
    for kw in ({}, {"generator_ema": GeneratorEMA(decay=0.9)}):
        _gan(seed=11, **kw)
        out.append(models.DCGANGenerator(arch="tiny").build().get_weights())
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert any(np.abs(a).max() > 0 and a.ndim > 1 for a in out[0])


def test_step_key_and_exit_state_change_only_with_the_feature():
    import torch
    reals = torch.zeros(2, 8, 8, 3)
    off, on, on2 = _gan(), _gan(generator_ema=0.9), _gan(generator_ema=0.9)
    k_off, k_on, k_on2 = (g._step_key("g", reals) for g in (off, on, on2))
    assert len(k_on) == len(k_off) + 1 and k_on[-1][0] == "generator_ema"
    E = on.generator_ema.store
    assert k_on[-1][1:3] == (E.theta.data_ptr(), E.state.data_ptr()) and k_on[-1] != k_on2[-1]        # other buffers, other program
    on.generator_ema_config = GeneratorEMA(decay=0.9, warmup=True)
    assert on._step_key("g", reals)[-1] != k_on[-1]                                                   # the static configuration
    assert len(off._exit_state()) == 2 and (E, "tr_dirty", True) in on._exit_state()


def test_sampling_from_a_model_without_the_average_is_an_error():
    gan = _gan()
    with pytest.raises(ValueError, match="generator_ema"):
        gan.generate_samples(np.zeros((2, 10), np.float32), ema=True)
    with pytest.raises(ValueError, match="generator_ema"):
        gan.reset_generator_ema()


def test_conv_math_reaches_the_averaged_model():
    gan = _gan(generator_ema=0.9, conv_math="bf16x6")
    assert gan.generator_ema.conv_math == "bf16x6"
    gan.conv_math = "fp32"
    assert gan.generator_ema.conv_math == "fp32" and gan.generator.conv_math == "fp32"


def test_checkpoint_keys_and_the_three_restore_cases(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    import json
    gan = _gan(generator_ema=GeneratorEMA(halflife_images=500, warmup=True))
    gan.generator_ema.set_weights([w + 0.25 for w in gan.generator_ema.get_weights()])
    gan.generator_ema_updates = 7
    path = CheckpointManager(gan, str(tmp_path / "on")).save(1)
    d = np.load(path)
    assert json.loads(str(d["g_ema_config"])) == {"decay": None, "halflife_images": 500.0, "warmup": True} and int(d["g_ema_updates"]) == 7
    assert np.array_equal(d["g_ema_theta"], gan.generator_ema.store.theta.numpy()) and d["g_ema_state"].shape == d["g_state"].shape
    # with the keys -> a model with the feature
    other = _gan(seed=4, generator_ema=0.9)
    other.generator_ema.store.tr_dirty = False
    CheckpointManager(other, str(tmp_path / "on")).restore(path)
    assert other.generator_ema_updates == 7 and other.generator_ema.store.tr_dirty
    for name in ("theta", "state"):
        assert np.array_equal(getattr(other.generator_ema.store, name).numpy(), getattr(gan.generator_ema.store, name).numpy())
        assert np.array_equal(getattr(other.generator.store, name).numpy(), getattr(gan.generator.store, name).numpy())
    # with the keys -> a model without the feature: ignored
    plain = _gan(seed=5)
    CheckpointManager(plain, str(tmp_path / "on")).restore(path)
    assert plain.generator_ema is None and np.array_equal(plain.generator.store.theta.numpy(), gan.generator.store.theta.numpy())
    # without the keys -> a model with the feature: averages <- restored live weights, count 0, a warning
    old = CheckpointManager(plain, str(tmp_path / "off")).save(1)
    assert not any(k.startswith("g_ema") for k in np.load(old).files)
    third = _gan(seed=6, generator_ema=0.9)
    third.generator_ema_updates = 3
    with pytest.warns(RuntimeWarning, match="averaged generator"):
        CheckpointManager(third, str(tmp_path / "off")).restore(old)
    assert third.generator_ema_updates == 0
    assert np.array_equal(third.generator_ema.store.theta.numpy(), plain.generator.store.theta.numpy())
    assert np.array_equal(third.generator_ema.store.state.numpy(), plain.generator.store.state.numpy())


def test_save_weights_writes_the_averaged_generator(tmp_path):
    gan = _gan(generator_ema=0.9)
    gan.save_weights(str(tmp_path / "w"))
    assert sorted(os.listdir(tmp_path)) == ["w_discriminator.npz", "w_generator.npz", "w_generator_ema.npz"]
    _gan().save_weights(str(tmp_path / "p"))
    assert not os.path.exists(tmp_path / "p_generator_ema.npz")


def test_sample_grid_callback_picks_the_averaged_generator(tmp_path):
    from blurred_gan_amd.callbacks import GenerateSampleGridCallback
    calls = []

    class Model:
        generator_ema = object()

        def generate_samples(self, latents, training=False, **kw):
            calls.append(kw)
            raise StopIteration

    for use_ema, has, want in ((None, True, {"ema": True}), (None, False, {}), (False, True, {}), (True, True, {"ema": True})):
        cb = GenerateSampleGridCallback(str(tmp_path), use_ema=use_ema)
        cb.model = Model()
        if not has:
            cb.model.generator_ema = None
        with pytest.raises(StopIteration):
            cb.make_grid()
        assert calls[-1] == want, (use_ema, has)
    assert GenerateSampleGridCallback(str(tmp_path)).use_ema is None
