"""CPU tests of blurred_gan_amd.optimizers: Keras constructor surface, configs, argument errors, the host's per-step scalar
sequence (the value a step program binds), shared instances, the type check of a step, and the ISA of the update kernels."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import blurred_gan_amd as bg
from blurred_gan_amd import callbacks, models
from blurred_gan_amd import optimizers as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reexported_as_bg_optimizers():
    assert bg.optimizers is O and {"SGD", "RMSprop", "Adam"} <= set(dir(bg.optimizers))


def test_constructor_defaults_match_keras():
    s = O.SGD()
    assert (s.learning_rate, s.momentum, s.nesterov, s.decay, s.iterations) == (0.01, 0.0, False, 0.0, 0)
    r = O.RMSprop()
    assert (r.learning_rate, r.rho, r.momentum, r.epsilon, r.centered, r.decay) == (0.001, 0.9, 0.0, 1e-7, False, 0.0)
    a = O.Adam()
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon, a.amsgrad, a.decay) == (0.001, 0.9, 0.999, 1e-7, False, 0.0)
    assert O.Adam(epsilon=None).epsilon == 1e-7 and O.RMSprop(epsilon=0).epsilon == 1e-7      # Keras: `epsilon or backend epsilon`


def test_slot_sets():
    assert O.SGD()._slot_names() == () and O.SGD(momentum=0.9)._slot_names() == ("m",)
    assert O.RMSprop()._slot_names() == ("v",)
    assert set(O.RMSprop(momentum=0.5, centered=True)._slot_names()) == {"m", "v", "s3"}
    assert O.Adam()._slot_names() == ("m", "v") and O.Adam(amsgrad=True)._slot_names() == ("m", "v", "s3")


@pytest.mark.parametrize("opt", [O.SGD(0.05, momentum=0.9, nesterov=True, decay=0.01), O.RMSprop(2e-4, rho=0.8, momentum=0.3, epsilon=1e-6,
                                                                                             centered=True),
                                 O.Adam(1e-4, beta_1=0.0, beta_2=0.9, epsilon=1e-8, amsgrad=True),
                                 O.Adam(callbacks.ExponentialDecay(1e-3, 100, 0.5))])
def test_get_config_from_config_round_trip(opt):
    cfg = opt.get_config()
    assert cfg["name"] == type(opt).__name__ and "learning_rate" in cfg and "decay" in cfg
    back = type(opt).from_config(cfg)
    assert type(back) is type(opt) and back.get_config() == cfg and back.static_config() == opt.static_config()
    for k in range(5):
        assert back.lr_at(k) == opt.lr_at(k)


def test_lr_alias_and_from_config_lr():
    assert O.SGD(lr=0.3).learning_rate == 0.3 and O.Adam(lr=2e-4).learning_rate == 2e-4
    assert O.RMSprop.from_config({"lr": 0.02, "rho": 0.5}).learning_rate == 0.02
    o = O.Adam()
    o.lr = 0.5
    assert o.learning_rate == 0.5


def test_keras_argument_errors():
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            O.SGD(momentum=bad)
    with pytest.raises(ValueError):
        O.Adam(decay=-1.0)
    with pytest.raises(ValueError):
        O.RMSprop(momentum=-0.5)
    with pytest.raises(TypeError):
        O.SGD(weight_decay=0.1)              # not an optimizer_v2 keyword
    with pytest.raises(ValueError):
        O.Adam(learning_rate="fast")
    for cls in (O.SGD, O.RMSprop, O.Adam):
        for k in ("clipnorm", "clipvalue", "global_clipnorm"):
            with pytest.raises(NotImplementedError):
                cls(**{k: 1.0})
            cls(**{k: None})                 # None is Keras' default and accepted


def _seq(opt, n=10):
    return [opt._advance() for _ in range(n)]


def test_scalar_sequence_constant_rate():
    for cls, lr in ((O.SGD, 0.01), (O.RMSprop, 0.001)):
        o = cls()
        assert _seq(o) == [lr] * 10 and o.iterations == 10


def test_scalar_sequence_inverse_time_decay():
    o = O.SGD(0.1, decay=0.05)
    assert _seq(o) == pytest.approx([0.1 / (1 + 0.05 * k) for k in range(10)], rel=1e-15)


def test_scalar_sequence_schedule_and_decay():
    sched = callbacks.ExponentialDecay(1e-3, decay_steps=4, decay_rate=0.5)
    o = O.RMSprop(sched, decay=0.1)
    want = [sched(k) / (1 + 0.1 * k) for k in range(10)]
    assert _seq(o) == pytest.approx(want, rel=1e-15)
    assert want[4] == pytest.approx(0.5e-3 / 1.4, rel=1e-6)        # the schedule sees k = iterations BEFORE the update
    o2 = O.SGD(lambda step: 0.1 * (step + 1))
    assert _seq(o2, 3) == pytest.approx([0.1, 0.2, 0.3])


def test_scalar_sequence_adam_lr_t():
    o = O.Adam(1e-4, beta_1=0.0, beta_2=0.9)
    want = [1e-4 * math.sqrt(1 - 0.9 ** t) / (1 - 0.0 ** t) for t in range(1, 11)]
    assert _seq(o) == pytest.approx(want, rel=1e-15)
    d = O.Adam()                     # default: the expression the constructor's optimizer always used, bit for bit
    assert _seq(d, 3) == [0.001 * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t) for t in (1, 2, 3)]


def test_learning_rate_writable_between_steps():
    o = O.SGD(0.1)
    assert o._advance() == 0.1
    o.learning_rate = 0.02
    assert o._advance() == 0.02


def _gan():
    bg.set_seed(3)
    g, d = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    return bg.WGANGP(g, d, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir="/tmp/bg_opt_logs"))


def test_default_constructor_makes_adam_and_names_other_than_adam_raise():
    gan = _gan()
    for model in (gan.generator, gan.discriminator):
        assert type(model.optimizer) is O.Adam and model.optimizer.get_config() == O.Adam().get_config()
    with pytest.raises(NotImplementedError, match="optimizers"):
        bg.WGAN(models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny"),
                bg.WGAN.HyperParameters(optimizer="rmsprop"), bg.TrainingConfig())


def test_shared_instance_one_counter_slots_per_network():
    """Keras: one optimizer applied to two variable lists keeps one `iterations`, advanced by each apply_gradients, and one set
    of slots per variable.  Here that is one counter advanced twice per batch and one slot set per ParamStore."""
    gan = _gan()
    opt = O.RMSprop(1e-3, momentum=0.5, centered=True)
    gan.generator.optimizer = gan.discriminator.optimizer = opt
    G, D = gan.generator.store, gan.discriminator.store
    for st in (G, D):
        opt.attach(st)
    assert G.slot_owner is opt and D.slot_owner is opt
    assert all(a.data_ptr() != b.data_ptr() for a, b in ((G.m, D.m), (G.v, D.v), (G.s3, D.s3)))
    for _ in range(3):           # one batch: the D-step's apply, then the G-step's, each advances the shared counter
        opt._advance()
        opt._advance()
    assert opt.iterations == 6


def test_optimizer_swapped_in_starts_from_zero_slots_and_swapped_back_keeps_its_own():
    gan = _gan()
    st = gan.generator.store
    first = gan.generator.optimizer
    first.attach(st)
    st.m.fill_(3.0)
    second = O.Adam(amsgrad=True)
    second.attach(st)
    assert float(st.m.abs().max()) == 0.0 and float(st.s3.abs().max()) == 0.0 and second.iterations == 0
    first.attach(st)
    assert float(st.m.min()) == 3.0


def test_non_optimizer_object_raises_type_error_naming_the_classes():
    gan = _gan()
    gan.discriminator.optimizer = "rmsprop"
    with pytest.raises(TypeError, match="SGD.*RMSprop.*Adam"):
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))


def test_checkpoint_records_optimizer_and_rejects_a_mismatch(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    gan = _gan()
    gan.generator.optimizer = O.RMSprop(2e-4, momentum=0.9, centered=True)
    gan.discriminator.optimizer = O.SGD(0.05, momentum=0.5)
    gan.generator.optimizer.attach(gan.generator.store)
    gan.generator.store.s3.fill_(0.5)
    gan.generator.optimizer.iterations = 4
    path = CheckpointManager(gan, str(tmp_path)).save(1)
    d = np.load(path)
    assert str(d["g_opt_class"]) == "RMSprop" and str(d["d_opt_class"]) == "SGD" and float(d["g_opt_lr"]) == 2e-4
    assert "g_s3" in d.files and "d_s3" not in d.files
    other = _gan()
    other.generator.optimizer = O.RMSprop(1e-3, momentum=0.9, centered=True)       # the rate may differ: restored from the file
    other.discriminator.optimizer = O.SGD(0.05, momentum=0.5)
    CheckpointManager(other, str(tmp_path)).restore(path)
    assert other.generator.optimizer.iterations == 4 and other.generator.optimizer.learning_rate == 2e-4
    assert float(other.generator.store.s3.min()) == 0.5
    for wrong in (O.RMSprop(momentum=0.9), O.Adam(), O.RMSprop(momentum=0.9, centered=True, rho=0.5)):
        third = _gan()
        third.generator.optimizer = wrong
        third.discriminator.optimizer = O.SGD(0.05, momentum=0.5)
        with pytest.raises(ValueError, match="RMSprop"):
            CheckpointManager(third, str(tmp_path)).restore(path)


def test_checkpoint_without_optimizer_record_restores_only_into_default_adam(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    gan = _gan()
    mgr = CheckpointManager(gan, str(tmp_path))
    d = dict(mgr.state_dict())
    for tag in ("g", "d"):           # today's format: m / v and the step count, no optimizer record
        for k in ("opt_class", "opt_config", "opt_lr"):
            d.pop(f"{tag}_{k}")
    d["g_m"] = np.full_like(d["g_m"], 0.125)
    d["g_iterations"] = np.int64(9)
    path = str(tmp_path / "ckpt-1.npz")
    np.savez(path, **d)
    other = _gan()
    CheckpointManager(other, str(tmp_path)).restore(path)
    assert other.generator.optimizer.iterations == 9 and float(other.generator.store.m.min()) == 0.125
    other.discriminator.optimizer = O.SGD()
    with pytest.raises(ValueError, match="optimizer record"):
        CheckpointManager(other, str(tmp_path)).restore(path)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_update_kernels_do_not_spill_and_move_float4(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "optim.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "optim.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    names = re.findall(r"\.name:\s+(\S*(?:sgd|rmsprop|adam_amsgrad)_kernel\S*)\n", isa)
    assert len(names) == 8, names              # 3 SGD + 4 RMSprop variants + amsgrad
    for m in re.finditer(r"\.name:\s+(\S*_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S):
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)
    for name in names:
        body = re.search(r"^" + re.escape(name) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
