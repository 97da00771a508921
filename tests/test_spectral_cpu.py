"""CPU tests of layers.SpectralNormalization: the layer surface, the argument errors of the bg_spectral_* entry points, what a step
of a spectrally normalised critic enqueues and in which order, and the code objects of csrc/spectral.hip."""
import contextlib
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, layers, models, ops

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


# ------------------------------------------------------------------ 1. the layer surface
def _wrapped_stack():
    return layers.Sequential([
        layers.SpectralNormalization(layers.Conv2D(8, 3, strides=2, padding="same", input_shape=[8, 8, 3])),
        layers.LeakyReLU(),
        layers.SpectralNormalization(layers.Conv2DTranspose(4, 5, strides=2, padding="same", use_bias=False), power_iterations=3),
        layers.LeakyReLU(),
        layers.Flatten(),
        layers.SpectralNormalization(layers.Dense(2)),
    ])


def test_wrapper_builds_on_the_three_layer_kinds_and_refuses_others():
    m = _wrapped_stack().build("cpu")
    names = [(n, tuple(sh), tr) for (_, n, _, sh, tr) in m.store.entries]
    assert names == [("kernel", (3, 3, 3, 8), True), ("bias", (8,), True), ("vector_u", (8,), False), ("vector_v", (27,), False), ("sigma", (1,), False),
                     ("kernel", (5, 5, 4, 8), True), ("vector_u", (8,), False), ("vector_v", (100,), False), ("sigma", (1,), False),
                     ("kernel", (256, 2), True), ("bias", (2,), True), ("vector_u", (2,), False), ("vector_v", (256,), False), ("sigma", (1,), False)]
    assert [tuple(v.shape) for v in m.trainable_variables] == [(3, 3, 3, 8), (8,), (5, 5, 4, 8), (256, 2), (2,)]
    assert m.count_params() == 216 + 8 + 800 + 512 + 2 + (8 + 27 + 1) + (8 + 100 + 1) + (2 + 256 + 1)
    assert m.output_shape == (None, 2) and [l.power_iterations for l in m.layers if l.kind in ("conv", "convT", "dense")] == [1, 3, 1]
    w = m.layers[0]
    assert w.kind == "conv" and w.filters == 8 and w.k == 3 and w.stride == 2 and w.layer.vars is w.vars
    for bad in (layers.LeakyReLU(), layers.BatchNormalization(), layers.LayerNormalization(), layers.Flatten(), layers.UpSampling2D()):
        with pytest.raises(NotImplementedError):
            layers.SpectralNormalization(bad)
    for n in (0, -1):
        with pytest.raises(ValueError):
            layers.SpectralNormalization(layers.Dense(3), power_iterations=n)


def test_initial_state_is_a_power_step_from_a_normal_draw():
    bg.set_seed(11)
    m = _wrapped_stack().build("cpu")
    for l in m.layers:
        if not isinstance(l, layers.SpectralNormalization):
            continue
        W = l.vars["kernel"].numpy().astype(np.float64).reshape(-1, l.vars["kernel"].shape[-1])
        u, v, s = (l.vars[n].numpy().astype(np.float64) for n in ("vector_u", "vector_v", "sigma"))
        assert abs(np.linalg.norm(u) - 1) < 1e-6 and abs(np.linalg.norm(v) - 1) < 1e-6
        t = W @ u
        np.testing.assert_allclose(v, t / np.linalg.norm(t), atol=1e-6)
        np.testing.assert_allclose(s[0], v @ W @ u, rtol=1e-6)


def test_get_and_set_weights_round_trip_the_state():
    bg.set_seed(5)
    a = _wrapped_stack().build("cpu")
    bg.set_seed(6)
    b = _wrapped_stack().build("cpu")
    wa = a.get_weights()
    assert len(wa) == 14 and any(not np.array_equal(x, y) for x, y in zip(wa, b.get_weights()))
    b.store.tr_dirty = False
    b.set_weights(wa)
    assert all(np.array_equal(x, y) for x, y in zip(wa, b.get_weights())) and torch.equal(a.store.state, b.store.state)
    assert b.store.tr_dirty and b.store.sn_dirty


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist", "mnist"])
def test_seeded_init_of_a_model_without_wrappers_is_unchanged(arch):
    """Only wrapped layers draw from the seed stream: a plain model built after a wrapped one was CONSTRUCTED (not built) from the
    same seed equals a plain model built alone, and the wrapped model's kernels are the plain model's up to the first wrapper's draw."""
    def build(cls, **kw):
        bg.set_seed(9)
        return cls(arch=arch, **kw).build("cpu")
    for cls in (models.DCGANDiscriminator, models.DCGANGenerator):
        first, second = build(cls), build(cls)
        assert all(np.array_equal(x, y) for x, y in zip(first.get_weights(), second.get_weights()))
        assert first.store.eff is None and first.net().spectral_layers == [] and first.store.n_state == second.store.n_state
        sn = build(cls, spectral_norm=True)
        assert np.array_equal(sn.get_weights()[0], first.get_weights()[0])
        lin = [l for l in sn._own_layers() if l.kind in ("conv", "convT", "dense")]
        assert lin and all(isinstance(l, layers.SpectralNormalization) for l in lin)
        assert [tuple(v.shape) for v in sn.trainable_variables] == [tuple(v.shape) for v in first.trainable_variables]
        assert [st.kind for st in sn.net().stages] == [st.kind for st in first.net().stages]


def test_demos_take_the_flags():
    import demo_celeba
    import demo_mnist
    for demo in (demo_mnist, demo_celeba):
        off = demo.make_parser().parse_args([])
        assert off.critic_spectral_norm is False and off.generator_spectral_norm is False
        on = demo.make_parser().parse_args(["--critic-spectral-norm", "--generator-spectral-norm"])
        assert on.critic_spectral_norm is True and on.generator_spectral_norm is True
        for cls in (demo.DCGANDiscriminator, demo.DCGANGenerator):
            wrapped = lambda m: [isinstance(l, layers.SpectralNormalization) for l in m.layers if l.kind in ("conv", "convT", "dense")]
            assert not any(wrapped(cls())) and all(wrapped(cls(spectral_norm=True))) and wrapped(cls(spectral_norm=True))


def _gan(critic_sn=True, generator_sn=False, arch="tiny", cls=None, **kw):
    cls = cls or bg.WGANGP
    bg.set_seed(3)
    gen, disc = models.DCGANGenerator(arch=arch, spectral_norm=generator_sn), models.DCGANDiscriminator(arch=arch, spectral_norm=critic_sn)
    gen.build("cpu"), disc.build("cpu")
    return cls(gen, disc, cls.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull), step_replay=False, **kw)


def test_the_averaged_generator_is_refused_with_a_spectrally_normalised_generator():
    with pytest.raises(NotImplementedError, match="generator_ema"):
        _gan(generator_sn=True, generator_ema=0.99)
    assert _gan(critic_sn=True, generator_sn=False, generator_ema=0.99).generator_ema is not None


# ------------------------------------------------------------------ 2. argument errors, no device involved
def _table(shapes=((75, 16, 25), (128, 1, 1))):
    rows, off_t, off_s, off_e = [], 0, 0, 0
    pad = lambda n: -(-n // 4) * 4
    for K, N, taps in shapes:
        rows.append(dict(w_off=off_t, u_off=off_s, v_off=off_s + pad(N), sigma_off=off_s + pad(N) + pad(K), eff_off=off_e,
                         tr_off=off_e + pad(K * N) if taps > 1 else -1, K=K, N=N, taps=taps))
        off_t, off_s, off_e = off_t + pad(K * N), off_s + pad(N) + pad(K) + 4, off_e + 2 * pad(K * N)
    return np.ascontiguousarray(ops.spectral.rows(rows), dtype=np.int32)


def test_route_and_workspace_are_host_queries():
    maker.ensure_library(ROOT)
    r = ops.spectral.route(75, 16, 25)
    assert r["vec"] == 4 and r["lanes"] == 4 and r["chunks"] == 1 and r["pass_units"] == 1 and r["tiles"] == 25 and r["ew_units"] == 1
    assert ops.spectral.route(800, 3, 25)["vec"] == 1 and ops.spectral.route(800, 3, 25)["lanes"] == 4
    assert ops.spectral.route(6400, 512, 25)["chunks"] == 2 and ops.spectral.route(100, 8192)["chunks"] == 0 == ops.spectral.route(7, 67)["chunks"]
    assert ops.spectral.route(100, 8192)["pass_units"] == 25 and ops.spectral.route(12800, 512, 25)["ew_units"] == 400
    t = _table()
    assert ops.spectral.workspace_bytes(t) == 4 * sum(ops.spectral.route(K, N, taps)["ws_floats"] for K, N, taps in ((75, 16, 25), (128, 1, 1)))
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (10, 4, 3)):
        with pytest.raises(ValueError, match="BAD_SHAPE|shape"):
            ops.spectral.route(*bad)


def test_bad_arguments_are_refused_and_launch_nothing():
    """Every call made here carries exactly one bad argument for the entry point it goes to, so every one of them must be refused
    before anything is launched; the host buffer that stands in for the device bases stays untouched."""
    maker.ensure_library(ROOT)
    lib = _lib.load()
    good = _table()
    buf = np.full(64 + 4, 7.0, np.float32)          # host memory standing in for the bases: a refused call never dereferences them
    base = buf.ctypes.data
    base += (-base) % 16
    ws_bytes = ops.spectral.workspace_bytes(good)
    assert ws_bytes > 4
    NULL, SHAPE, ALIGN, WS = -6, -1, -2, -5

    # entry point -> (its pointer arguments in order, the call); `table` / `n` / `wsb` are the host rows, their count, the workspace size
    def power(a, table, n, wsb, sigma_only=0):
        return lib.bg_spectral_power_f32(a["theta"], a["state"], a["desc_d"], table, n, sigma_only, a["ws"], wsb, None)

    def sigma(a, table, n, wsb):
        return power(a, table, n, wsb, sigma_only=1)

    def scale(a, table, n, wsb):
        return lib.bg_spectral_scale_f32(a["theta"], a["state"], a["eff"], a["desc_d"], table, n, None)

    def grad(a, table, n, wsb):
        return lib.bg_spectral_grad_f32(a["grad"], a["eff"], a["state"], a["desc_d"], table, n, a["ws"], wsb, None)

    POINTERS = {power: ("theta", "state", "desc_d", "ws"), sigma: ("theta", "state", "desc_d", "ws"), scale: ("theta", "state", "eff", "desc_d"),
                grad: ("grad", "eff", "state", "desc_d", "ws")}

    def call(fn, table=good, n=None, wsb=ws_bytes, **bad):
        assert set(bad) <= set(POINTERS[fn])          # a pointer the entry point does not take would leave the call valid
        a = {k: bad.get(k, base) for k in POINTERS[fn]}
        return fn(a, None if table is None else table.ctypes.data, (len(good) if n is None else n), wsb)

    for fn, names in POINTERS.items():
        for name in names:                                                  # each pointer of each entry point, null and misaligned
            assert call(fn, **{name: None}) == NULL, (fn.__name__, name)
            assert call(fn, **{name: base + 4}) == ALIGN, (fn.__name__, name)
        assert call(fn, table=None) == NULL, fn.__name__
        assert call(fn, n=0) == SHAPE and call(fn, n=-1) == SHAPE, fn.__name__
        for col, val in ((6, 0), (6, -3), (7, 0), (8, 0), (8, 7), (9, 5), (10, 0), (11, 3), (0, -4)):
            t = good.copy()
            t[1, col] = val                           # K, N, taps, the three first units, a negative offset
            assert call(fn, table=t) == SHAPE, (fn.__name__, col, val)
            assert ops.spectral.workspace_bytes(t) == 0
        for col in (0, 1, 2, 4, 5, 12):
            t = good.copy()
            t[0, col] += 2                            # an offset that is no multiple of four floats
            assert call(fn, table=t) == ALIGN, (fn.__name__, col)
    for fn in (power, sigma, grad):                   # the entry points that take a workspace
        assert call(fn, wsb=ws_bytes - 4) == WS and call(fn, wsb=0) == WS, fn.__name__
        assert b"workspace" in lib.bg_last_error()
    with pytest.raises(_lib.BgError, match="workspace"):
        _lib.check(WS, "bg_spectral_grad_f32")
    assert (buf == 7.0).all()


# ------------------------------------------------------------------ 3. what a step enqueues
SN_RETURNS = {"power": None, "scale": "eff", "grad": "grad"}


class _Recorder:
    def __init__(self):
        self.events = []

    def wrap(self, name, real, ret):
        sig = inspect.signature(real)

        def rec(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            if "counter" in args:
                args["offset"] = ops._draw_offset(args["out"], args["offset"], args.pop("counter"))
            self.events.append((name, args))
            return args[ret] if ret else None
        return rec

    def ready(self, lo, hi):
        self.events.append(("ready", (int(lo), int(hi))))

    def finish(self):
        self.events.append(("finish", ()))


@contextlib.contextmanager
def recording(rec):
    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, obj.__dict__[name] if isinstance(obj, type) else getattr(obj, name)))
        setattr(obj, name, new)

    for name, ret in maker.RETURNS.items():
        patch(ops, name, rec.wrap(name, getattr(ops, name), ret))
    for name, ret in SN_RETURNS.items():
        patch(ops.spectral, name, staticmethod(rec.wrap("spectral." + name, getattr(ops.spectral, name), ret)))
    patch(bg.dist, "GradReducer", lambda *a, **k: rec)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


D_STEP_CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
FORWARDS = ("conv2d_fwd", "conv2d_bwd_data", "gemm", "blur_nhwc", "blur3_lerp", "lerp")


def _step_events(config, arch="tiny", **kw):
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _gan(arch=arch, **D_STEP_CONFIGS[config], **kw)
        gan.train_on_batch(np.zeros((2,) + models.IMAGE_SHAPE[arch], np.float32))
    return gan, rec.events


@pytest.mark.parametrize("config", sorted(D_STEP_CONFIGS))
def test_a_critic_step_enqueues_the_spectral_launches_in_order(config):
    gan, events = _step_events(config)
    names = [n for n, _ in events]
    D = gan.discriminator
    d_end = names.index("adam")                                   # the critic's optimizer launch
    d_names = names[:d_end]
    own = lambda a: a["theta"].data_ptr() == D.store.theta.data_ptr() if "theta" in a else a["grad"].data_ptr() == D.store.grad.data_ptr()
    sn = [(k, n, a) for k, (n, a) in enumerate(events[:d_end]) if n.startswith("spectral.") and own(a)]
    assert [n for _, n, _ in sn] == ["spectral.power", "spectral.scale", "spectral.grad"]
    assert sn[0][2]["sigma_only"] is False and sn[0][2]["table"].n == 3
    first_forward = min(k for k, n in enumerate(d_names) if n in FORWARDS)
    assert sn[0][0] < sn[1][0] < first_forward
    last_wgrad = max(k for k, n in enumerate(d_names) if n in ("conv2d_bwd_filter", "colsum"))
    assert last_wgrad < d_names.index("finish") < sn[2][0] == d_end - 1
    # no separate transpose launch for the spectrally normalised critic: the one there is is the plain generator's
    tr = [a for n, a in events if n == "transpose_last2_batched"]
    assert tr and all(a["src_base"].data_ptr() == gan.generator.store.theta.data_ptr() for a in tr)
    # the G-step's critic pass: sigma = v^T W u refreshed, no round; the generator has no such layer
    g_sn = [(n, a) for n, a in events[d_end + 1:] if n.startswith("spectral.")]
    assert [n for n, _ in g_sn] == ["spectral.power", "spectral.scale"] and g_sn[0][1]["sigma_only"] is True
    # the convs and the Dense read the effective buffer, never the raw kernel
    eff, theta = D.store.eff, D.store.theta
    inside = lambda t, buf: t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    for n, a in events:
        if n in ("conv2d_fwd", "conv2d_bwd_data"):
            w = a["wT"] if n == "conv2d_fwd" else a["w"]
            assert not inside(w, theta)
        if n == "gemm" and not a["transA"]:
            assert not inside(a["Bm"], theta)
    assert sum(inside(a["wT"], eff) for n, a in events if n == "conv2d_fwd") >= 2


def test_the_number_of_spectral_launches_does_not_depend_on_the_number_of_layers(monkeypatch):
    count = lambda ev: [n for n, _ in ev if n.startswith("spectral.")]
    two = count(_step_events("merged")[1])
    monkeypatch.setitem(models._D, "tiny", [16, 32, 32])
    gan, ev = _step_events("merged")
    assert len(gan.discriminator.net().spectral_layers) == 4 and count(ev) == two and len(two) == 5


def test_both_models_normalised_and_more_rounds():
    gan, events = _step_events("merged", generator_sn=True)
    G = gan.generator
    names = [n for n, _ in events]
    assert "transpose_last2_batched" not in names
    g_own = [(n, a) for n, a in events if n.startswith("spectral.") and ("theta" in a and a["theta"].data_ptr() == G.store.theta.data_ptr()
                                                                         or "grad" in a and a["grad"].data_ptr() == G.store.grad.data_ptr())]
    # D-step: the generator's weights are new to this pass -> sigma only; G-step: its round, its scale, its projection
    assert [(n, a.get("sigma_only")) for n, a in g_own] == [("spectral.power", True), ("spectral.scale", None), ("spectral.power", False),
                                                            ("spectral.scale", None), ("spectral.grad", None)]
    assert names.index("spectral.grad") < names.index("adam") and names[::-1].index("adam") < names[::-1].index("spectral.grad")
    # power_iterations = 3 on every critic layer: three power launches, still one scale
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _gan()
        for l in gan.discriminator._own_layers():           # before the Net is built: it reads the number of rounds once
            if isinstance(l, layers.SpectralNormalization):
                l.power_iterations = 3
        gan.discriminator_step(np.zeros((2, 8, 8, 3), np.float32))
    sn = [n for n, _ in rec.events if n.startswith("spectral.")]
    assert sn == ["spectral.power"] * 3 + ["spectral.scale", "spectral.grad"]


def test_a_plain_model_enqueues_no_spectral_launch_and_allocates_nothing():
    gan, events = _step_events("merged", critic_sn=False)
    assert not [n for n, _ in events if n.startswith("spectral.")]
    for m in (gan.generator, gan.discriminator):
        assert m.store.eff is None and m.store._sn_table is None and m.net().plain_conv_layers == m.net().conv_layers


# ------------------------------------------------------------------ 4. the code objects
def test_mixed_rounds_are_refused_when_the_net_is_built_and_the_rounds_are_in_the_step_key():
    m = _wrapped_stack().build("cpu")                 # power_iterations 1, 3, 1
    with pytest.raises(NotImplementedError, match="power_iterations"):
        m.net()
    gan = _gan()
    reals = torch.zeros(2, 8, 8, 3)
    key = gan._step_key("d", reals)
    assert gan.discriminator.net().spectral_rounds == 1 and gan.generator.net().spectral_rounds == 0
    gan.discriminator.net().spectral_rounds = 2
    assert gan._step_key("d", reals) != key
    gan.discriminator.net().spectral_rounds = 1
    assert gan._step_key("d", reals) == key
    gan.discriminator.store.sn_dirty = not gan.discriminator.store.sn_dirty       # a round taken by hand between two steps
    assert gan._step_key("d", reals) != key


def test_kernels_do_not_spill_and_use_no_private_memory(tmp_path_factory):
    """The reading of tests/test_build_cpu.py::test_hot_kernels_do_not_spill, on csrc/spectral.hip."""
    from test_build_cpu import HIPCC, _isa, _resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    isa = _isa(tmp_path_factory, "spectral.hip")
    res = _resources(isa, "_kernel")
    assert len(res) == 5 and all(any(k in n for n in res) for k in ("sn_pass", "sn_finish", "sn_scale", "sn_dot", "sn_apply")), list(res)
    assert all(v == (0, 0, 0) for v in res.values()), res
    for name in res:            # every streaming kernel has a float4 route
        body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end", isa, flags=re.S | re.M).group(1)      # early exits end the program too
        if "sn_finish" not in name:
            assert "global_load_dwordx4" in body, name
        if "sn_scale" in name or "sn_apply" in name:
            assert "global_store_dwordx4" in body, name
