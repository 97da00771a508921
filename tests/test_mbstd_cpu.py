"""layers.MinibatchStdDev without a GPU: the formulas of the kernels against torch autograd in float64, what the case list of the
kernel tests reaches according to bg_mbstd_plan, the layer's surface and refusals, what a critic step with the layer enqueues (and
that one without it enqueues nothing new), and the argument errors of the C entry points."""
import contextlib
import ctypes as C
import importlib.util
import inspect
import io
import os
import re

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, engine, layers, models, ops
import mbstd_cases as MC
import mbstd_reference as MR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L = layers
DT = torch.float64

_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


# ------------------------------------------------------------------ 1. the formulas against autograd, float64
@pytest.mark.parametrize("G,groups,P,C", [(2, 1, 1, 1), (2, 3, 4, 5), (3, 2, 9, 8), (4, 2, 4, 6), (5, 1, 2, 3)])
def test_backward_tangent_and_source_equal_autograd(G, groups, P, C):
    eps = 1e-8
    x, u, d = MC.data(G, groups, P, C, seed=G * 100 + P * 10 + C)
    y, mu, rs, f = MR.np_fwd(x, G, eps)
    xt = torch.as_tensor(x).requires_grad_(True)
    ut, dt = torch.as_tensor(u), torch.as_tensor(d).requires_grad_(True)
    layer = lambda t: MR.torch_mbstd(t, G, eps)
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert rel(y, layer(xt).detach().numpy()) < 1e-14
    # backward: the vector-Jacobian product of u
    dx_ref, = torch.autograd.grad((ut * layer(xt)).sum(), xt, create_graph=True)
    dx, q = MR.np_bwd(u, x, G, eps)
    assert rel(dx, dx_ref.detach().numpy()) < 1e-13
    # tangent: the Jacobian-vector product along d
    _, tan = torch.autograd.functional.jvp(layer, xt, dt, create_graph=True)
    vout, src, fdot = MR.np_gp(d, x, q, G, eps)
    assert rel(vout, tan.detach().numpy()) < 1e-13
    # source: the derivative of <d, J(x)^T u> w.r.t. the primal input, d and u held constant
    src_ref, = torch.autograd.grad((dt.detach() * dx_ref).sum(), xt)
    # the two terms of the source nearly cancel at G = 2: the error is measured against the size of one term, which is what
    # autograd's own rounding scales with
    term = float(np.abs(q).max()) / (G * P * C) * float(np.abs(d).max()) * float(rs.max())
    assert float(np.abs(src - src_ref.numpy()).max()) < 1e-13 * term
    # and the same through the tangent: <u, J(x) d> is the same scalar
    src_tan, = torch.autograd.grad((ut * tan).sum(), xt)
    assert float(np.abs(src_ref.numpy() - src_tan.numpy()).max()) < 1e-13 * term


def test_the_source_at_g2_is_the_epsilon_term_alone():
    """At G = 2 the two terms of the source cancel to q k (d - dbar) eps / s^3: the form the kernel evaluates there."""
    eps = 1e-3          # large enough to see the term in float64 beside the cancellation's rounding
    x, u, d = MC.data(2, 3, 4, 5, seed=7)
    _, q = MR.np_bwd(u, x, 2, eps)
    _, src, _ = MR.np_gp(d, x, q, 2, eps)
    mu, s, _ = MR.np_stats(x, 2, eps)
    dg = d.reshape(3, 2, 4, 5)
    want = q[:, None, None, None] / (2 * 4 * 5) * (dg - dg.mean(1, keepdims=True)) * eps / s[:, None] ** 3
    np.testing.assert_allclose(src.reshape(3, 2, 4, 5), want, rtol=1e-9, atol=1e-15)


def test_exact_case_premise_holds_in_float32():
    for k in (1, 2, 3):
        assert np.sqrt(np.float32(k * k) + np.float32(1e-8), dtype=np.float32) == np.float32(k)
    x, k = MC.exact_data(2, 4, 8, seed=1)
    assert np.array_equal(x, np.round(x)) and np.array_equal(MR.np_stats(x.astype(np.float32), 2, 1e-8)[1], k.astype(np.float32))


def test_a_constant_column_adds_exactly_zero():
    x, u, d = MC.data(3, 2, 2, 4, seed=3)
    x[:, :, 1] = x[0, 0, 1]
    d[:, :, 1] = d[0, 0, 1]
    dx, q = MR.np_bwd(u, x, 3, 1e-8)
    vout, src, fdot = MR.np_gp(d, x, q, 3, 1e-8)
    assert np.array_equal(dx[..., 1], u[..., 1]) and not src[..., 1].any() and np.isfinite(src).all() and np.isfinite(vout).all()


# ------------------------------------------------------------------ 2. what the case list reaches, from bg_mbstd_plan alone
@pytest.fixture(scope="module")
def plans():
    maker.ensure_library(ROOT)
    return {(name, call, off): ops.mbstd.plan(G * groups, G, P, Cc, call, off)
            for name, G, groups, P, Cc in MC.CASES for call in ("fwd", "bwd", "gp") for off in MC.OFFSETS}


@pytest.mark.parametrize("call", ["fwd", "bwd", "gp"])
def test_case_list_reaches_every_route_trip_count_and_tail(plans, call):
    mine = {k: p for k, p in plans.items() if k[1] == call}
    assert {p["resident"] for p in mine.values()} == {True, False}
    trips = set()
    for p in mine.values():
        trips |= {min(p["trips_min"], 2), min(p["trips_max"], 2)}
    assert trips == {0, 1, 2}, trips
    ends = {(p["head"] > 0, p["tail"] > 0) for p in mine.values()}
    assert (False, False) in ends and any(h for h, _ in ends) and any(t for _, t in ends), ends
    cuts = {p["grid_y"] for p in mine.values() if not p["resident"]}
    assert (1 in cuts or call == "bwd") and 2 in cuts and any(c >= 3 for c in cuts), cuts
    # a ragged last cut: its float4s are fewer than the other cuts'
    assert any(not p["resident"] and p["grid_y"] > 1 and p["vecs"] % p["grid_y"] for p in mine.values())


def test_plan_geometry(plans):
    for (name, call, off), p in plans.items():
        _, G, groups, P, Cc = MC.case(name)
        assert p["resident"] == (G * P * Cc <= MC.RESIDENT_FLOATS), (name, call)
        assert p["threads"] == 256 and p["grid_x"] == min(groups, MC.MAX_BLOCKS)
        assert p["launches"] == (1 if p["resident"] or call == "bwd" else 2)
        assert p["lds_bytes"] <= 64 * 1024
        if p["resident"]:
            assert p["grid_y"] == p["grid_y_emit"] == 1
            assert (p["lds_bytes"] == 16) == (call == "bwd")
        n = G * P * Cc if call == "bwd" else P * Cc
        assert p["head"] + 4 * p["vecs"] + p["tail"] == n and p["head"] == min((4 - off) % 4, n)
    assert ops.mbstd.workspace_bytes(8, 4, 4, 512) == 0
    assert ops.mbstd.workspace_bytes(8, 4, 4, 1024) == 4 * 2 * plans[("cut_two", "fwd", 0)]["grid_y"]
    assert plans[("celeba_top", "fwd", 0)]["resident"] and plans[("mnist_top", "fwd", 0)]["resident"]


def test_case_list_reaches_a_second_group_per_workgroup_and_the_cap_on_cuts(plans):
    """More groups than workgroups on the resident route (the LDS image is reused), through the G = 2 branch and the general one;
    a group that would be cut more than MAX_CUTS ways, for the columns and for the emit."""
    text = open(os.path.join(ROOT, "blurred-gan_amd", "csrc", "mbstd.hip")).read()
    assert f"kMaxBlocks = {MC.MAX_BLOCKS};" in text and f"constexpr int kCutFloats = {MC.CUT_FLOATS};" in text
    assert f"constexpr int kMaxCuts = {MC.MAX_CUTS};" in text and "p.gx = (unsigned)std::min(N / G, kMaxBlocks);" in text
    for call in ("fwd", "bwd", "gp"):
        second = [(name, G) for name, G, groups, P, Cc in MC.CASES for p in [plans[(name, call, 0)]]
                  if p["resident"] and p["grid_x"] == MC.MAX_BLOCKS < groups and plans[(name, call, 1)]["grid_x"] == MC.MAX_BLOCKS]
        assert [n for n, G in second if G == 2] and [n for n, G in second if G > 2], (call, second)
        capped = []
        for name, G, groups, P, Cc in MC.CASES:
            p = plans[(name, call, 0)]
            cols, emit = (G * P * Cc, G * P * (Cc + 1))
            if not p["resident"] and p["grid_y"] == MC.MAX_CUTS == p["grid_y_emit"] and min(-(-cols // MC.CUT_FLOATS), -(-emit // MC.CUT_FLOATS)) > MC.MAX_CUTS:
                capped.append(name)
                assert p["trips_max"] >= 2 and p["vecs"] % MC.MAX_CUTS, name          # several trips per lane, a ragged last cut
                if call != "bwd":
                    assert ops.mbstd.workspace_bytes(G * groups, G, P, Cc) == 4 * groups * MC.MAX_CUTS
        assert capped, call
    # three workgroups take a second group; the capped group is one cut past the cap
    assert MC.case("second_trip")[2] - MC.MAX_BLOCKS == 3 and MC.case("second_trip_g3")[2] - MC.MAX_BLOCKS == 2
    _, G, _, P, Cc = MC.case("cut_capped")
    assert -(-G * P * Cc // MC.CUT_FLOATS) == MC.MAX_CUTS + 1 == -(-G * P * (Cc + 1) // MC.CUT_FLOATS)


# ------------------------------------------------------------------ 3. the layer
def test_layer_surface():
    l = L.MinibatchStdDev()
    assert (l.kind, l.group_size, l.epsilon, l.num_new_features) == ("mbstd", 4, 1e-8, 1)
    assert l.out_shape((2, 2, 512)) == (2, 2, 513) and l.var_specs((2, 2, 512)) == [] and l.count_params() == 0
    with pytest.raises(NotImplementedError, match="num_new_features"):
        L.MinibatchStdDev(num_new_features=2)
    for g in (1, 0, -3):
        with pytest.raises(ValueError, match="group_size"):
            L.MinibatchStdDev(group_size=g)
    with pytest.raises(NotImplementedError, match=r"\[H, W, C\]"):
        L.Sequential([L.Dense(4, input_shape=(3,)), L.MinibatchStdDev()])
    assert "consecutive" in L.MinibatchStdDev.__doc__.lower() and "strided" in L.MinibatchStdDev.__doc__


def _refused(ls):
    m = L.Sequential(ls)
    m.build("cpu")
    with pytest.raises(NotImplementedError, match="directly before the critic's Flatten"):
        m.net()


def test_placement_rules():
    conv = lambda **kw: L.Conv2D(8, 3, padding="same", **kw)
    first = dict(input_shape=(4, 4, 3))
    head = lambda: [L.Flatten(), L.Dense(1)]
    for below in (lambda: [L.LeakyReLU()], lambda: [L.LeakyReLU(), L.Dropout(0.3)], lambda: [L.LeakyReLU(), L.AveragePooling2D()],
                  lambda: [L.LayerNormalization(), L.LeakyReLU()]):
        m = L.Sequential([conv(**first), *below(), L.MinibatchStdDev(2), *head()])
        m.build("cpu")
        net = m.net()
        assert [st.kind for st in net.stages][-2:] == ["mbstd", "dense"] and net.has_source and net._gp_kinds()[-2:] == ["mbstd", "dense"]
        with pytest.raises(NotImplementedError, match="overwrites activations"):
            net.gp_second_order_merged(None, 0, 2)
    _refused([conv(**first), L.LeakyReLU(), L.MinibatchStdDev(2), conv(), L.LeakyReLU(), *head()])         # in front of a conv
    _refused([conv(**first), L.MinibatchStdDev(2), *head()])                                              # behind a conv without LeakyReLU
    _refused([L.MinibatchStdDev(2, **first), *head()])                                                     # first in the network
    _refused([conv(**first), L.LeakyReLU(), L.MinibatchStdDev(2), L.Flatten(), L.Dense(2)])             # not the critic's head
    _refused([conv(**first), L.LeakyReLU(), L.MinibatchStdDev(2)])
    _refused([L.Dense(48, input_shape=(5,)), L.Reshape((4, 4, 3)), L.MinibatchStdDev(2), *head()])         # behind a Dense
    gen = [L.Dense(48, use_bias=False, input_shape=(5,)), L.BatchNormalization(), L.LeakyReLU(), L.Reshape((4, 4, 3)),
           L.Conv2DTranspose(3, 3, strides=2, padding="same", use_bias=False), L.BatchNormalization(), L.LeakyReLU(), L.MinibatchStdDev(2),
           L.Conv2D(3, 3, padding="same", activation="tanh")]
    _refused(gen)                                                                                        # a generator
    plain = L.Sequential([conv(**first), L.LeakyReLU(), *head()])
    plain.build("cpu")
    assert not plain.net().has_source and not plain.net().mbstd_layers


@pytest.mark.parametrize("arch", ["tiny", "tiny_mnist", "mnist", "celeba64", "celeba128"])
@pytest.mark.parametrize("kw", [{}, dict(downsampling="pool"), dict(normalization="layer"), dict(spectral_norm=True)])
def test_critic_builder(arch, kw):
    plain, mb = models.DCGANDiscriminator(arch=arch, **kw), models.DCGANDiscriminator(arch=arch, minibatch_stddev=4, **kw)
    assert plain.minibatch_stddev is None and mb.minibatch_stddev == 4
    kinds = [l.kind for l, _ in mb.flat_layers()]
    assert kinds[-3:] == ["mbstd", "flatten", "dense"] and "mbstd" not in [l.kind for l, _ in plain.flat_layers()]
    (layer, s), (dense, sd) = mb.flat_layers()[-3], mb.flat_layers()[-1]
    H, W, Cc = s
    assert layer.group_size == 4 and sd == (H * W * (Cc + 1),)
    assert [sh for n, sh, _, _ in dense.var_specs(sd) if n == "kernel"] == [(H * W * (Cc + 1), 1)]       # Keras' shape, (H, W, C + 1) order
    count = lambda m: sum(int(np.prod(sh)) for l, s in m.flat_layers() for _, sh, _, _ in l.var_specs(s))
    extra = H * W + (H * W if kw.get("spectral_norm") else 0)            # the Dense kernel's rows, and its vector_v's
    assert count(mb) == count(plain) + extra
    for bad in (True, 2.5):
        with pytest.raises(ValueError, match="minibatch_stddev"):
            models.DCGANDiscriminator(arch=arch, minibatch_stddev=bad)
    with pytest.raises(ValueError, match="group_size"):
        models.DCGANDiscriminator(arch=arch, minibatch_stddev=1)


def test_summary_weights_and_count_follow_from_the_layer_list():
    m = models.DCGANDiscriminator(arch="tiny", minibatch_stddev=2)
    m.build("cpu")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.summary()
    assert re.search(r"MinibatchStdDev\s+in=\(2, 2, 32\)\s+out=\(2, 2, 33\)\s+params=0\n", buf.getvalue()), buf.getvalue()
    ws = m.get_weights()
    assert ws[-2].shape == (2 * 2 * 33, 1) and m.count_params() == sum(w.size for w in ws)
    m.set_weights(ws)
    plain = models.DCGANDiscriminator(arch="tiny")
    plain.build("cpu")
    with pytest.raises((RuntimeError, ValueError, AssertionError)):      # a plain critic's weights do not fit: the Dense kernel's shape
        m.set_weights(plain.get_weights())


def test_batch_size_must_be_a_multiple_of_the_group():
    maker.ensure_library(ROOT)
    m = models.DCGANDiscriminator(arch="tiny", minibatch_stddev=4)
    m.build("cpu")
    net = m.net()
    net.check_rows(8)
    for rows in (2, 6, 7):
        with pytest.raises(ValueError, match=r"B % group_size == 0") as e:
            net.check_rows(rows)
        assert "not shrunk" in str(e.value) and f"{rows} rows" in str(e.value)
    with pytest.raises(ValueError, match=r"B % group_size == 0"):
        net.context(6)
    # a step: B = 2 with G = 4 is refused before anything is enqueued, although its 2B = 4 rows would hold one (straddling) group
    bg.layers.set_seed(3)
    gen = models.DCGANGenerator(arch="tiny")
    gen.build("cpu")
    gan = bg.WGANGP(gen, m, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull),
                    step_replay=False, merge_critic_passes=False)
    rec = _Recorder()
    with recording(rec):
        with pytest.raises(ValueError, match=r"B % group_size == 0"):
            gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    assert not [n for n, _ in rec.events if n.startswith("mbstd.") or n.startswith("conv2d")]


def test_demos_take_the_switch():
    import demo_celeba
    import demo_mnist
    for demo in (demo_mnist, demo_celeba):
        assert demo.make_parser().parse_args([]).critic_mbstd == 0
        assert demo.make_parser().parse_args(["--critic-mbstd", "4"]).critic_mbstd == 4
        kinds = lambda m: [l.kind for l in m.layers]
        assert "mbstd" not in kinds(demo.DCGANDiscriminator())
        d = demo.DCGANDiscriminator(minibatch_stddev=4, normalization="layer", downsampling="pool", spectral_norm=True)
        assert kinds(d)[-3:] == ["mbstd", "flatten", "dense"] and d.layers[-3].group_size == 4


# ------------------------------------------------------------------ 4. what a critic step enqueues
MB_RETURNS = {"fwd": "y", "bwd": "dx", "gp": "vout"}


class _Recorder:
    """Launches as (name, arguments) and reducer hand-overs as ("ready", (lo, hi)), in the order the step enqueues them."""

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
    for ns, table in (("layernorm", {"fwd": "a", "bwd": "dz", "tangent": "vout", "gp_source": "s"}), ("mbstd", MB_RETURNS)):
        for name, ret in table.items():
            patch(getattr(ops, ns), name, staticmethod(rec.wrap(f"{ns}.{name}", getattr(getattr(ops, ns), name), ret)))
    patch(bg.dist, "GradReducer", lambda *a, **k: rec)
    patch(layers, "default_device", lambda: torch.device("cpu"))
    try:
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def _cpu_gan(mb=2, blur=False, B=2, cls=None, **kw):
    cls = cls or (bg.BlurredWGANGP if blur else bg.WGANGP)
    bg.layers.set_seed(3)
    critic = {k: kw.pop(k) for k in ("downsampling", "normalization") if k in kw}
    gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny", minibatch_stddev=mb, **critic)
    gen.build("cpu"), disc.build("cpu")
    hp = cls.HyperParameters(batch_size=B, global_batch_size=B, **({"initial_blur_std": 0.9} if blur else {}))
    return cls(gen, disc, hp, bg.TrainingConfig(log_dir=os.devnull), step_replay=False, **kw)


def _grad_writes(args, grad):
    out = []
    for v in args.values():
        if isinstance(v, torch.Tensor) and v.numel() and v.untyped_storage().data_ptr() == grad.untyped_storage().data_ptr():
            out.append((v.storage_offset(), v.storage_offset() + v.numel()))
    return out


D_STEP_CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}


@pytest.mark.parametrize("config", sorted(D_STEP_CONFIGS))
@pytest.mark.parametrize("variant", ["plain", "blur", "pool", "layernorm"])
def test_launch_record_of_a_critic_step_with_the_layer(config, variant):
    maker.ensure_library(ROOT)
    B, G = 2, 2
    critic = {"pool": dict(downsampling="pool"), "layernorm": dict(normalization="layer")}.get(variant, {})
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan(mb=G, blur=variant == "blur", B=B, **critic, **D_STEP_CONFIGS[config])
        gan.train_on_batch(np.zeros((B, 8, 8, 3), np.float32))
    D = gan.discriminator.net()
    grad = D.store.grad
    end = [n for n, _ in rec.events].index("finish")
    ev, rest = rec.events[:end + 1], rec.events[end + 1:]
    names = [n for n, _ in ev]
    merged = config != "unmerged"
    # the critic step: one forward and one backward launch per pass that has them, ONE launch for tangent and source together,
    # and never the merged second-order route (no filter gradient over all 3B rows)
    passes = [(3 * B,)] if merged else [(2 * B,), (B,)]
    fwd = [a for n, a in ev if n == "mbstd.fwd"]
    assert sorted(a["x"].shape[0] for a in fwd) == sorted(p[0] for p in passes)
    assert all(tuple(a["y"].shape[1:]) == (2, 2, 33) and tuple(a["x"].shape[1:]) == (2, 2, 32) and a["G"] == G and a["eps"] == 1e-8 for a in fwd)
    assert names.count("mbstd.bwd") == len(passes) and names.count("mbstd.gp") == 1
    gp = next(a for n, a in ev if n == "mbstd.gp")
    assert gp["d"].shape[0] == B and gp["x"].shape[0] == B and tuple(gp["vout"].shape) == (B, 2, 2, 33) and tuple(gp["src"].shape) == (B, 2, 2, 32)
    # q of the x-hat rows' groups: the groups [2B / G, 3B / G) of the merged pass, the 'hat' pass's own otherwise
    assert gp["q"].numel() == B // G and gp["q"].storage_offset() == (2 * B // G if merged else 0)
    bwd = [a for n, a in ev if n == "mbstd.bwd"]
    assert any(a["q"].untyped_storage().data_ptr() == gp["q"].untyped_storage().data_ptr() for a in bwd)
    assert names.index("mbstd.fwd") < names.index("mbstd.bwd") < names.index("mbstd.gp")
    wgrads = [a for n, a in ev if n == "conv2d_bwd_filter"]
    assert wgrads and all(a["x"].shape[0] in (B, 2 * B) for a in wgrads)
    # behind the tangent: the head's column sum, then the source backward -- through the activation of the stage below first
    k = names.index("mbstd.gp")
    tail = [n for n in names[k + 1:] if n not in ("ready", "workspace")]
    assert tail[0] == "colsum"
    assert tail[1] == {"plain": "mul_grad", "blur": "mul_grad", "pool": "upsample2x", "layernorm": "layernorm.bwd"}[variant], tail[:4]
    assert "conv2d_bwd_filter" in tail[2:]
    # no slice goes to the reducer before its last write, and each layer's goes exactly once
    handed = [(j, a) for j, (n, a) in enumerate(ev) if n == "ready"]
    for j, (lo, hi) in handed:
        late = [(names[i], w) for i in range(j + 1, len(ev)) if names[i] not in ("ready", "finish", "adam")
                for w in _grad_writes(ev[i][1], grad) if w[0] < hi and w[1] > lo]
        assert not late, f"[{lo}, {hi}) handed over at event {j}, written again by {late}"
    ranges = [D._train_range(st) for st in D.stages if st.kind not in engine.PARAMETER_FREE]
    assert sorted(a for _, a in handed) == sorted(ranges)
    # the generator step's critic pass: forward and backward, no penalty launch
    g_names = [n for n, _ in rest]
    assert g_names.count("mbstd.fwd") == 1 == g_names.count("mbstd.bwd") and "mbstd.gp" not in g_names
    print(config, variant, "critic-step launches:", len([n for n in names if n not in ("ready", "finish")]))


def test_lazy_penalty_and_plain_wgan_steps_take_the_two_slice_path():
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        gan = _cpu_gan(cls=bg.WGAN)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    assert names.count("mbstd.fwd") == 2 == names.count("mbstd.bwd") and "mbstd.gp" not in names
    assert [a["x"].shape[0] for n, a in rec.events if n == "mbstd.fwd"] == [4, 2]


def test_a_step_without_the_layer_enqueues_what_it_did():
    """No launch of the new kernels, no buffer of theirs, the merged second-order route as before (the engine-trace fixture holds
    the launch list itself, byte for byte)."""
    maker.ensure_library(ROOT)
    rec = _Recorder()
    with recording(rec):
        bg.layers.set_seed(3)
        gen, disc = models.DCGANGenerator(arch="tiny"), models.DCGANDiscriminator(arch="tiny")
        gen.build("cpu"), disc.build("cpu")
        gan = bg.WGANGP(gen, disc, bg.WGANGP.HyperParameters(batch_size=2, global_batch_size=2), bg.TrainingConfig(log_dir=os.devnull), step_replay=False)
        gan.train_on_batch(np.zeros((2, 8, 8, 3), np.float32))
    names = [n for n, _ in rec.events]
    assert not [n for n in names if n.startswith("mbstd.")]
    D = gan.discriminator.net()
    c3 = D.context(6, "fr3", drop_rows=4)
    assert not D.has_source and not [k for k in c3._extra if k[0] == "mbstd"] and "blur_grad" not in c3._extra
    assert max(a["x"].shape[0] for n, a in rec.events if n == "conv2d_bwd_filter") == 6        # one filter gradient over all 3B rows


# ------------------------------------------------------------------ 5. the C entry points
def test_argument_errors_are_statuses():
    maker.ensure_library(ROOT)
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    out = (C.c_int * _lib.MBSTD_PLAN_INTS)()
    bad_shape, null, unsupported = -1, -6, -3
    fwd = lambda N, G, P, Cc, x=p, y=p: lib.bg_mbstd_fwd_f32(x, y, p, p, p, N, G, P, Cc, 1e-8, None, 0, None)
    bwd = lambda N, G, P, Cc, u=p: lib.bg_mbstd_bwd_f32(u, p, p, p, p, p, N, G, P, Cc, None)
    gp = lambda N, G, P, Cc, d=p: lib.bg_mbstd_gp_f32(d, p, p, p, p, p, p, p, N, G, P, Cc, 1e-8, None, 0, None)
    for call in (fwd, bwd, gp):
        assert call(6, 4, 1, 2) == bad_shape and b"no multiple of the group size" in lib.bg_last_error()
        assert call(4, 1, 1, 2) == bad_shape and b"at least 2" in lib.bg_last_error()
        assert call(0, 2, 1, 2) == bad_shape and call(4, 2, 0, 2) == bad_shape and call(4, 2, 1, 0) == bad_shape
        assert call(4, 2, 1, 2, None) == null and b"null pointer" in lib.bg_last_error()
    assert fwd(4, 2, 1, 2, y=None) == null
    assert lib.bg_mbstd_fwd_f32(p, p, p, p, p, 4, 2, 1, 2, 0.0, None, 0, None) == unsupported
    assert lib.bg_mbstd_plan(6, 4, 1, 2, 0, 0, out) == bad_shape and lib.bg_mbstd_plan(4, 2, 1, 2, 3, 0, out) == unsupported
    assert lib.bg_mbstd_plan(4, 2, 1, 2, 0, 4, out) == unsupported and lib.bg_mbstd_plan(4, 2, 1, 2, 0, 0, None) == null
    assert lib.bg_mbstd_workspace_bytes(6, 4, 1, 2) == 0
    # a pointer one byte off
    odd = C.c_void_p(p.value + 1)
    assert fwd(4, 2, 1, 2, odd) == -2
    # the wrappers raise what the statuses stand for, before anything is launched
    with pytest.raises(ops.BgDeviceError):
        t = torch.zeros(4, 1, 2)
        ops.mbstd.fwd(t, torch.zeros(4, 1, 3), torch.zeros(2, 2), torch.zeros(2, 2), torch.zeros(2), 2)


# ------------------------------------------------------------------ 6. the code objects
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_kernels_use_no_private_memory_and_move_float4(tmp_path):
    import subprocess
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "mbstd.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "mbstd.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    kernels = list(re.finditer(r"\.name:\s+(\S*_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S))
    names = [m.group(1) for m in kernels]
    # forward and penalty call: resident, columns, emit; one backward
    assert len(names) == 7 and sum("mbstd_fwd_kernel" in n for n in names) == 3 == sum("mbstd_gp_kernel" in n for n in names), names
    for m in kernels:
        for key in ("vgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)
    for name in names:
        body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end", isa, flags=re.S | re.M).group(1)
        assert "global_store_dwordx4" in body, name
        assert "global_load_dwordx4" in body or "Li2E" in name, name      # the emit kernels gather their pass-through floats one at a time
