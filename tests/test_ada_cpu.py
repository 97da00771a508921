"""CPU tests of adaptive augmentation: the AdaptiveAugment surface and the demos' flags, the library's gated decode (on the host)
against the Python decode of tests/ada_reference.py on hand-picked rows, the statuses of the new calls (nothing is launched), the
controller rule in Python on a scripted score sequence, the model's refusals and the checkpoint keys."""
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, models, ops
from blurred_gan_amd.diffaugment import AdaptiveAugment, DiffAugment, as_augment
import ada_reference as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HI = AR.HI


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge._load_build_module().build_lib(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------ 1. the configuration class
def test_exported_and_a_subclass():
    assert bg.AdaptiveAugment is AdaptiveAugment and "AdaptiveAugment" in bg.__all__ and issubclass(AdaptiveAugment, DiffAugment)


def test_defaults_and_canonical_policy():
    a = AdaptiveAugment("cutout,color")
    assert a.get_config() == dict(policy="color,cutout", translation_ratio=0.125, cutout_ratio=0.5, p=0.0, target=0.6, interval=4,
                                  speed_images=500_000.0)
    assert a.ops_mask == 5 and a.adaptive and not AdaptiveAugment(p=0.5, target=None).adaptive
    assert a.kernel_args() == DiffAugment("color,cutout").kernel_args()


@pytest.mark.parametrize("kw", [dict(p=-0.1), dict(p=1.5), dict(p="half"), dict(p=True), dict(target=1.0), dict(target=-1.0), dict(target="0.6"),
                                dict(interval=0), dict(interval=2.5), dict(interval=True), dict(speed_images=0), dict(speed_images=-5.0),
                                dict(speed_images=float("inf")), dict(policy="rotation"), dict(cutout_ratio=2.0)])
def test_bad_values_are_refused(kw):
    with pytest.raises(ValueError):
        AdaptiveAugment(**kw)


def test_edge_values_are_accepted():
    AdaptiveAugment(p=0, target=0.0, interval=1, speed_images=1)
    AdaptiveAugment(p=1.0, target=-0.999, interval=np.int64(3), speed_images=np.float32(64))


def test_config_round_trip_equality_and_hash():
    a = AdaptiveAugment("color,translation", 0.25, 0.75, p=0.25, target=None, interval=2, speed_images=1024)
    b = AdaptiveAugment.from_config(a.get_config())
    assert a == b and hash(a) == hash(b) and a.static_config() == b.static_config() and repr(a) == repr(b)
    assert "AdaptiveAugment(" in repr(a) and "target=None" in repr(a)
    for other in (dict(p=0.5), dict(target=0.6), dict(interval=3), dict(speed_images=2048)):
        c = AdaptiveAugment.from_config(dict(a.get_config(), **other))
        assert a != c and a.static_config() != c.static_config()
    json.dumps(a.get_config())


def test_never_equal_to_a_diffaugment():
    a, d = AdaptiveAugment(), DiffAugment()
    assert a != d and d != a and not (a == d) and not (d == a)
    assert a.static_config() != d.static_config()
    assert set(d.get_config()) == {"policy", "translation_ratio", "cutout_ratio"}          # the base class is untouched


def test_as_augment():
    a = AdaptiveAugment(p=0.5)
    assert as_augment(a) is a
    assert as_augment(AdaptiveAugment("", p=0.5)) is None           # an empty policy still yields None
    with pytest.raises(ValueError):
        as_augment(0.5)


# ------------------------------------------------------------------ 2. demo flags
@pytest.mark.parametrize("demo", ["demo_mnist", "demo_celeba"])
def test_demo_flags(demo):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    mod = __import__(demo)
    parse = lambda *argv: bg.diffaugment.augment_from_args(mod.make_parser().parse_args(list(argv)))
    assert parse() is None and parse("--diffaugment", "color") == "color"
    assert parse("--ada") == AdaptiveAugment()                     # --ada alone: the full policy
    assert parse("--ada", "--diffaugment", "cutout") == AdaptiveAugment("cutout")
    got = parse("--ada", "--ada-target", "none", "--ada-p", "0.5", "--ada-interval", "2", "--ada-speed-images", "1000")
    assert got == AdaptiveAugment(p=0.5, target=None, interval=2, speed_images=1000)
    assert parse("--ada", "--ada-target", "0.3").target == 0.3
    assert parse("--ada-p", "0.5") is None                          # without --ada the other flags select nothing


# ------------------------------------------------------------------ 3. the gated decode
FULL = DiffAugment()


def _row(gates, base=(0.9, 0.25, 0.75, 0.0, HI, 0.5, 0.0, 0.3)):
    return np.array(list(base) + list(gates) + [0.5], F32)


def _same_decode(lib, u, p, H, W, cfg):
    got = ops.diffaug.decode_gated(u, p, H, W, **cfg.kernel_args())
    want = AR.decode(u, p, H, W, cfg)
    assert got["fired"] == want["fired"], (got, want)
    for k in ("ty", "tx", "y0", "x0", "cy", "cx"):
        assert got[k] == want[k], (k, got, want)
    for k in ("b", "s", "c"):
        assert F32(got[k]) == want[k], (k, got, want)
    return got


def test_gate_equal_to_p_does_not_fire(lib):
    p = F32(0.375)
    below = np.nextafter(p, F32(0))
    d = _same_decode(lib, _row((p, p, p)), p, 16, 12, FULL)
    assert d["fired"] == 0 and (d["b"], d["s"], d["c"], d["ty"], d["tx"], d["cy"], d["cx"]) == (0, 1, 1, 0, 0, 0, 0)
    assert _same_decode(lib, _row((below, below, below)), p, 16, 12, FULL)["fired"] == 7
    assert _same_decode(lib, _row((below, p, below)), p, 16, 12, FULL)["fired"] == 5


def test_p_zero_and_p_one(lib):
    for gates in ((0.0, 0.0, 0.0), (HI, HI, HI), (0.0, HI, 0.3)):
        assert _same_decode(lib, _row(gates), 0.0, 9, 7, FULL)["fired"] == 0
        d = _same_decode(lib, _row(gates), 1.0, 9, 7, FULL)
        assert d["fired"] == 7
        plain = ops.diffaug.decode(_row(gates)[:8], 9, 7, **FULL.kernel_args())
        assert all(d[k] == plain[k] for k in plain)             # p = 1 is the ungated decode


@pytest.mark.parametrize("mask", range(8))
@pytest.mark.parametrize("policy", ["color,translation,cutout", "color", "translation,cutout", "cutout"])
def test_each_gate_alone_and_together(lib, mask, policy):
    cfg = DiffAugment(policy, 0.25, 0.5)
    u = AR.with_gates(_row((0, 0, 0))[None, :8], [mask])[0]
    d = _same_decode(lib, u, 0.5, 10, 10, cfg)
    assert d["fired"] == mask & cfg.ops_mask
    plain = ops.diffaug.decode(u[:8], 10, 10, d["fired"], 0.25, 0.5)
    assert all(d[k] == plain[k] for k in ("b", "s", "c", "ty", "tx", "y0", "x0"))
    assert (d["cy"], d["cx"]) == ((5, 5) if d["fired"] & 4 else (0, 0))


def test_decode_gated_refusals(lib):
    u, bsc, geo, f = (C.c_float * 12)(), (C.c_float * 3)(), (C.c_int * 8)(), C.c_int()
    assert lib.bg_diffaug_decode_gated(None, 0.5, 4, 4, 7, 0.125, 0.5, bsc, geo, C.byref(f)) == -6
    assert lib.bg_diffaug_decode_gated(u, 0.5, 4, 4, 7, 0.125, 0.5, bsc, geo, None) == -6
    assert lib.bg_diffaug_decode_gated(u, 0.5, 0, 4, 7, 0.125, 0.5, bsc, geo, C.byref(f)) == -1
    assert lib.bg_diffaug_decode_gated(u, 0.5, 4, 4, 8, 0.125, 0.5, bsc, geo, C.byref(f)) == -3


# ------------------------------------------------------------------ 4. ABI statuses (host memory: a call that launched would fault)
def test_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "bgan.h")).read()
    for name in ("bg_diffaug_gated_f32", "bg_diffaug_gated_adjoint_f32", "bg_diffaug_decode_gated", "bg_ada_stats_f32", "bg_ada_update_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in hdr
    import __graft_entry__ as ge
    assert "ada.hip" in ge._load_build_module().SOURCES


def test_gated_argument_errors_are_statuses(lib):
    buf = (C.c_float * 96)()
    a = C.cast(buf, C.c_void_p).value
    x, y, u, p = a, a + 64, a + 128, a + 256

    def fwd(x=x, y=y, u=u, p=p, n=1, H=2, W=2, Cc=1, mask=7, tr=0.125, cr=0.5):
        return lib.bg_diffaug_gated_f32(x, y, u, p, n, H, W, Cc, mask, tr, cr, 0, None)

    def adj(x=x, y=y, u=u, p=p, n=1, H=2, W=2, Cc=1, mask=7, tr=0.125, cr=0.5):
        return lib.bg_diffaug_gated_adjoint_f32(x, y, u, p, n, H, W, Cc, mask, tr, cr, None)

    for call in (fwd, adj):
        assert call(p=None) == -6                                     # the new refusal: a null p
        assert b"null" in lib.bg_last_error()
        assert call(x=None) == -6 and call(y=None) == -6 and call(u=None) == -6
        assert call(n=0) == -1 and call(H=0) == -1 and call(Cc=0) == -1
        assert call(tr=1.5) == -3 and call(cr=-0.1) == -3             # bad ratios
        assert call(mask=8) == -3 and call(mask=-1) == -3             # unknown mask bits
        assert call(x=x + 2) == -2 and call(p=p + 2) == -2 and call(u=u + 1) == -2        # misalignment
        assert call(y=x) == -3 and call(y=x + 8) == -3                # overlap
        assert b"overlap" in lib.bg_last_error()


def test_controller_argument_errors_are_statuses(lib):
    buf = (C.c_float * 64)()
    a = C.cast(buf, C.c_void_p).value
    assert lib.bg_ada_stats_f32(None, 4, a, None) == -6 and lib.bg_ada_stats_f32(a, 4, None, None) == -6
    assert lib.bg_ada_stats_f32(a, 0, a + 64, None) == -1 and lib.bg_ada_stats_f32(a, 1 << 24, a + 64, None) == -1
    assert lib.bg_ada_stats_f32(a + 2, 4, a + 64, None) == -2
    upd = lambda stats=a, state=a + 64, met=None, target=0.6, interval=4, inv=1e-3: lib.bg_ada_update_f32(stats, state, met, target, interval, inv, None)
    assert upd(stats=None) == -6 and upd(state=None) == -6
    assert upd(interval=0) == -1
    assert upd(target=1.0) == -3 and upd(target=-1.0) == -3 and upd(inv=0.0) == -3 and upd(target=float("nan")) == -3
    assert upd(met=a + 130) == -2


def test_cpu_tensors_are_rejected(lib):
    x = torch.zeros(1, 4, 4, 3)
    with pytest.raises(ops.BgDeviceError):
        ops.diffaug.fwd_gated(x, torch.empty_like(x), torch.zeros(1, 12), torch.zeros(1), 7, 0.125, 0.5)
    with pytest.raises(ops.BgDeviceError):
        ops.ada.stats(torch.zeros(4), torch.zeros(4))


# ------------------------------------------------------------------ 5. the controller rule
def test_sign_statistics():
    s, c = AR.sign_stats([0.0, -0.0, np.nan, np.inf, -np.inf, 3.0, -1e-30, 1e-45])
    assert (s, c) == (1.0, 8.0)


def test_controller_rule_on_a_scripted_sequence():
    """Batch 4, interval 2, speed 32: every adjustment is 8 / 32 = 1/4, so every p is exact."""
    c = AR.Controller(p=0.5, target=0.5, interval=2, speed_images=32)
    up, down, at = [1, 1, 1, 1], [-1, -1, 1, -1], [1, 1, 1, -1]
    seq = [(up, 0.5), (up, 0.75),            # r = 1 > target: +1/4, after the second step only
           (up, 0.75), (up, 1.0),
           (up, 1.0), (up, 1.0),             # clamped at 1
           (at, 1.0), (at, 1.0),             # r = 4 / 8 = target exactly: sgn(0) = 0, nothing moves
           (down, 1.0), (down, 0.75), (down, 0.75), (down, 0.5), (down, 0.5), (down, 0.25), (down, 0.25), (down, 0.0),
           (down, 0.0), (down, 0.0)]         # clamped at 0
    for i, (scores, want) in enumerate(seq):
        st = c.step(np.array(scores, F32))
        assert st[0] == F32(want), (i, st)
        assert st[3] == (i + 1) % 2 and st[2] == 4 * ((i + 1) % 2)
    assert c.r_last == F32(-0.5)
    # zeros and NaN count in the batch and add no sign: r = 2 / 8
    c = AR.Controller(p=0.5, target=0.25, interval=1, speed_images=16)
    assert c.step(np.array([1, 1, 0, np.nan, 1, -1, 0, 0], F32))[0] == 0.5 and c.r_last == F32(0.25)
    assert c.step(np.array([1, 1, 1, np.nan, 1, -1, 0, 0], F32))[0] == 1.0 and c.r_last == F32(0.375)


# ------------------------------------------------------------------ 6. the model surface
def _gan(cls=None, seed=3, hp=None, **kw):
    bg.set_seed(seed)
    g, d = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
    cls = cls or bg.WGANGP
    return cls(g, d, cls.HyperParameters(batch_size=2, global_batch_size=2, **(hp or {})), bg.TrainingConfig(log_dir="/tmp/bg_ada_logs"), **kw)


def test_wasserstein_without_drift_refuses_a_target():
    a = AdaptiveAugment(p=0.25)
    with pytest.raises(ValueError, match="e_drift"):
        _gan(hp=dict(e_drift=0.0), augment=a)
    with pytest.raises(ValueError, match="e_drift"):
        _gan(cls=bg.WGAN, augment=a)                               # the plain WGAN has no drift term at all
    assert _gan(augment=a).augment is a                            # the default e_drift anchors the sign
    assert _gan(hp=dict(e_drift=0.0), augment=a, objective="hinge").augment is a
    assert _gan(cls=bg.WGAN, augment=a, objective="nonsaturating").augment is a
    fixed = AdaptiveAugment(p=0.25, target=None)                   # a fixed p is fine everywhere
    assert _gan(hp=dict(e_drift=0.0), augment=fixed).augment is fixed and _gan(cls=bg.WGAN, augment=fixed).augment is fixed


def test_metrics_p_property_and_setter():
    plain, diff = _gan(), _gan(augment="color")
    for g in (plain, diff):
        assert g.augment_p is None and "augment_p" not in g.metrics_names
        with pytest.raises(ValueError):
            g.set_augment_p(0.5)
    assert plain.metrics_names == ["loss", "real_scores", "fake_scores", "gen_loss", "disc_loss", "gp_term", "norm_term"]
    gan = _gan(cls=bg.BlurredWGANGP, augment=AdaptiveAugment(p=0.25))
    assert gan.metrics_names[-1] == "std" and {"augment_p", "augment_rt"} <= set(gan.metrics_names)
    assert len(gan.metrics_names) == len(_gan(cls=bg.BlurredWGANGP).metrics_names) + 2
    assert gan.augment_p == 0.25
    gan._ada_state[1:4] = torch.tensor([3.0, 8.0, 2.0])
    gan.set_augment_p(0.75)
    assert gan._ada_state.tolist() == [0.75, 0, 0, 0, 0, 0, 0, 0] and gan._metrics_dev()[12:14].tolist() == [0.75, 0.0]
    for bad in (-0.1, 1.5, "x", True):
        with pytest.raises(ValueError):
            gan.set_augment_p(bad)


def test_step_key_holds_the_configuration_not_the_live_p():
    reals = torch.zeros(2, 8, 8, 3)
    part = lambda gan: [k for k in gan._step_key("d", reals) if isinstance(k, tuple) and k and k[0] == "augment"]
    a, b = _gan(augment=AdaptiveAugment(p=0.25)), _gan(augment=AdaptiveAugment(p=0.5))
    for g in (a, b):
        for m in (g.generator, g.discriminator):
            bg.optimizers.get_optimizer(m).attach(m.store)
    before = part(a)
    assert before and before != part(b) and before != part(_gan(augment=DiffAugment()))
    a.set_augment_p(0.9)
    assert part(a) == before


def test_wrong_width_of_injected_params_is_a_value_error():
    gan = _gan(augment=AdaptiveAugment(p=0.5, target=None))
    gan._injected = {"aug_g": np.zeros((2, 8), F32)}
    with pytest.raises(ValueError, match="12"):
        gan._aug_params("aug_g", ("aug_g",), 2)


def test_checkpoint_keys_and_the_restore_cases(tmp_path):
    from blurred_gan_amd.checkpoint import CheckpointManager
    cfg = AdaptiveAugment(p=0.25, interval=3, speed_images=64)
    gan = _gan(augment=cfg)
    gan._ada_state.copy_(torch.tensor([0.375, 2.0, 8.0, 2.0, 0.5, 0, 0, 0]))
    path = CheckpointManager(gan, str(tmp_path / "on")).save(1)
    d = np.load(path)
    assert d["aug_state"].dtype == np.float32 and d["aug_state"].tolist() == [0.375, 2.0, 8.0, 2.0, 0.5, 0, 0, 0]
    assert json.loads(str(d["aug_config"])) == cfg.get_config()
    # into a fresh model of the same configuration: the state, and the metric slots a fixed-p step would report
    fresh = _gan(seed=4, augment=AdaptiveAugment(p=0.25, interval=3, speed_images=64))
    CheckpointManager(fresh, str(tmp_path / "on")).restore(path)
    assert torch.equal(fresh._ada_state.cpu(), gan._ada_state.cpu()) and fresh._metrics_dev()[12:14].tolist() == [0.375, 0.5]
    # another configuration is refused, before anything is overwritten
    other = _gan(seed=4, augment=AdaptiveAugment(p=0.25, interval=4, speed_images=64))
    theta = other.discriminator.store.theta.clone()
    with pytest.raises(ValueError, match="adaptive augmentation"):
        CheckpointManager(other, str(tmp_path / "on")).restore(path)
    assert torch.equal(theta, other.discriminator.store.theta) and other.augment_p == 0.25
    # a model without the feature ignores the keys; a file without them restores into the initial state, with one warning
    plain = _gan(seed=4)
    CheckpointManager(plain, str(tmp_path / "on")).restore(path)
    old = CheckpointManager(plain, str(tmp_path / "off")).save(1)
    assert "aug_state" not in np.load(old).files and "aug_config" not in np.load(old).files
    fresh._ada_state.copy_(torch.tensor([0.9, 1.0, 4.0, 1.0, 0.1, 0, 0, 0]))
    with pytest.warns(RuntimeWarning, match="adaptive-augmentation state"):
        CheckpointManager(fresh, str(tmp_path / "off")).restore(old)
    assert fresh._ada_state.tolist()[:4] == [0.25, 0, 0, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        CheckpointManager(fresh, str(tmp_path / "off")).restore(old)
