"""CPU tests of layers.MappingNetwork and what is built around it: the layer's variables, initialisers and coefficients, every
refusal with its rule, the model arguments, the style source, the reference's manual backward against torch autograd in float64
(tests/mapping_reference.py: the formulas the engine's launch sequence implements), the w_avg and truncation formulas, the demos'
arguments, the checkpoint's configuration record and the ABI declarations."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from blurred_gan_amd import _lib, checkpoint, engine, layers, models
import mapping_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _specs(layer, L):
    return [(n, tuple(sh), tr) for n, sh, tr, _ in layer.var_specs((L,))]


def test_variable_specs_order_and_shapes():
    mp = layers.MappingNetwork(units=7, num_layers=3)
    assert mp.kind == "mapping" and mp.out_shape((10,)) == (7,)
    assert _specs(mp, 10) == [("kernel_0", (10, 7), True), ("kernel_1", (7, 7), True), ("kernel_2", (7, 7), True),
                              ("bias_0", (7,), True), ("bias_1", (7,), True), ("bias_2", (7,), True), ("w_avg", (7,), False)]
    d = layers.MappingNetwork()
    assert d.num_layers == 8 and d.lr_multiplier == 0.01 and d.alpha == 0.2 and d.equalized_lr and d.w_avg_beta == 0.995
    assert d.out_shape((12,)) == (12,) and _specs(d, 12)[0] == ("kernel_0", (12, 12), True) and len(_specs(d, 12)) == 17


def test_coefficients_and_bias_multiplier_are_fp32_values_of_the_double_formula():
    mp = layers.MappingNetwork(units=512, num_layers=3, lr_multiplier=0.01)
    mp.out_shape((100,))
    want = [float(np.float32(math.sqrt(2.0) / math.sqrt(f) * 0.01)) for f in (100, 512, 512)]
    assert mp.coefficients == want and mp.bias_multiplier == float(np.float32(0.01))
    assert all(float(np.float32(c)) == c for c in mp.coefficients)
    plain = layers.MappingNetwork(units=4, num_layers=2, lr_multiplier=1.0, equalized_lr=False)
    plain.out_shape((3,))
    assert plain.coefficients == [1.0, 1.0] and plain.bias_multiplier == 1.0


def test_initialisers():
    rng = np.random.default_rng(0)
    mp = layers.MappingNetwork(units=256, num_layers=2, lr_multiplier=0.01)
    vals = {n: init(rng) for n, _, _, init in mp.var_specs((200,))}
    for n, fan in (("kernel_0", 200), ("kernel_1", 256)):
        k = vals[n].astype(np.float64)
        assert vals[n].dtype == np.float32
        # N(0, 1) / lr_multiplier: standard deviation 100, mean 0 within 5 standard errors
        assert abs(k.std() / 100.0 - 1.0) < 0.02 and abs(k.mean()) < 5 * 100.0 / math.sqrt(k.size)
    assert not vals["bias_0"].any() and not vals["bias_1"].any() and not vals["w_avg"].any()
    g = layers.MappingNetwork(units=256, num_layers=1, lr_multiplier=1.0, equalized_lr=False)
    k = next(init(rng) for n, _, _, init in g.var_specs((200,)) if n == "kernel_0")
    lim = math.sqrt(6.0 / (200 + 256))
    assert np.abs(k).max() <= lim and np.abs(k).max() > 0.99 * lim and abs(k.std() - lim / math.sqrt(3)) < 0.01 * lim


@pytest.mark.parametrize("kw", [dict(num_layers=0), dict(units=0), dict(lr_multiplier=0.0), dict(lr_multiplier=float("inf")), dict(alpha=0.0),
                                dict(w_avg_beta=1.0), dict(lr_multiplier=0.5, equalized_lr=False)])
def test_bad_arguments_are_value_errors(kw):
    with pytest.raises(ValueError, match="MappingNetwork"):
        layers.MappingNetwork(**kw)


def _stack(*front, tail=True):
    m = layers.Sequential()
    for l in front:
        m.add(l)
    if tail:
        m.add(layers.Dense(2 * 2 * 8))
        m.add(layers.Reshape((2, 2, 8)))
        m.add(layers.LeakyReLU())
        m.add(layers.PixelNormalization())
        m.add(layers.StyleModulation(layers.Conv2DTranspose(3, (3, 3), strides=(2, 2), padding="same", use_bias=False, activation="tanh"),
                                     demodulate=False))
    return m


def test_placement():
    ok = _stack(layers.MappingNetwork(units=5, num_layers=2, input_shape=(6,)))
    ok.build(CPU)
    net = ok.net()
    assert net.has_mapping and net.mapping is ok.layers[0] and net.style_dim == 5 and net.in_shape == (6,) and net.stages[0].in_shape == (5,)
    assert ok.layers[-1].style_dim == 5 and tuple(ok.layers[-1].vars["style_kernel"].shape) == (5, 8)
    behind_pn = _stack(layers.PixelNormalization(input_shape=(6,)), layers.MappingNetwork(num_layers=1))
    behind_pn.build(CPU)
    assert behind_pn.net().has_mapping and behind_pn.net().latent_pn is not None and behind_pn.net().style_dim == 6
    assert engine.Net.MAPPING_RULE is layers.MAPPING_RULE and "first layer" in layers.MAPPING_RULE
    rule = re.escape(layers.MAPPING_RULE[:40])
    # behind a stage
    bad = layers.Sequential([layers.Dense(6, input_shape=(6,)), layers.MappingNetwork(num_layers=1), layers.Dense(4)])
    bad.build(CPU)
    with pytest.raises(NotImplementedError, match=rule):
        bad.net()
    # two of them
    two = _stack(layers.MappingNetwork(num_layers=1, input_shape=(6,)), layers.MappingNetwork(num_layers=1))
    two.build(CPU)
    with pytest.raises(NotImplementedError, match=rule):
        two.net()
    # a critic: an image input
    with pytest.raises(NotImplementedError, match=rule):
        layers.Sequential([layers.MappingNetwork(input_shape=(8, 8, 3))])
    with pytest.raises(NotImplementedError, match=rule):
        layers.Sequential([layers.Conv2D(4, 3, padding="same", input_shape=(8, 8, 3)), layers.MappingNetwork()])


def test_the_ordinary_dense_refusal_and_the_prefix_free_dLdw_refusal_stay():
    m = layers.Sequential([layers.Dense(4, input_shape=(6,)), layers.LeakyReLU(), layers.Dense(2)])
    m.build(CPU)
    with pytest.raises(NotImplementedError, match="Dense \\+ activation without BatchNormalization"):
        m.net()
    g = models.DCGANGenerator(arch="tiny", normalization="style")
    g.build(CPU)
    net = g.net()
    assert not net.has_mapping and net.mapping is None and net.style_dim == 10
    with pytest.raises(NotImplementedError, match="dL/dw"):
        net.backward(None, None, need_dx=True)


def _names(model):
    return [(type(l).__name__, n, tuple(sh), tr) for (l, n, _, sh, tr) in model.store.entries]


@pytest.mark.parametrize("kw", [dict(), dict(normalization="pixel", noise=True), dict(normalization="style", noise=True, equalized_lr=True),
                                dict(normalization="style", normalize_latents=True)])
def test_generator_defaults_build_the_same_variable_lists(kw):
    a = models.DCGANGenerator(arch="tiny", **kw)
    b = models.DCGANGenerator(arch="tiny", mapping_layers=0, mapping_units=None, mapping_lr_multiplier=0.01, **kw)
    a.build(CPU), b.build(CPU)
    assert _names(a) == _names(b) and not any(isinstance(l, layers.MappingNetwork) for l, _ in a.flat_layers())
    assert [type(l).__name__ for l, _ in a.flat_layers()] == [type(l).__name__ for l, _ in b.flat_layers()]


def test_generator_with_a_mapping_network():
    g = models.DCGANGenerator(arch="tiny", normalization="style", normalize_latents=True, equalized_lr=True, mapping_layers=3, mapping_units=7)
    g.build(CPU)
    plain = models.DCGANGenerator(arch="tiny", normalization="style", normalize_latents=True, equalized_lr=True)
    plain.build(CPU)
    names = _names(g)
    assert [n for _, n, _, _ in names[:7]] == ["kernel_0", "kernel_1", "kernel_2", "bias_0", "bias_1", "bias_2", "w_avg"]
    assert names[0][2] == (10, 7) and names[7] == ("EqualizedLearningRate", "kernel", (7, 128), True)
    rest = [(t, n, sh if n not in ("kernel", "style_kernel") or sh[0] != 10 else (7,) + sh[1:], tr) for t, n, sh, tr in _names(plain)]
    assert names[7:] == rest            # the synthesis network's list, with w's size where the latent size stood
    net = g.net()
    assert net.style_dim == 7 and all(l.style_dim == 7 for l in net.mod_layers) and net.mapping.equalized_lr and net.mapping.lr_multiplier == 0.01
    assert not g.store.state[:7].any()            # w_avg lives in the state buffer, zeros at the start
    with pytest.raises(ValueError, match="normalization='style'"):
        models.DCGANGenerator(arch="tiny", normalization="pixel", mapping_layers=2)
    with pytest.raises(ValueError, match="must be 1"):
        models.DCGANGenerator(arch="tiny", normalization="style", mapping_layers=2)          # equalized_lr=False, multiplier 0.01
    assert models.DCGANGenerator(arch="tiny", normalization="style", mapping_layers=2, mapping_lr_multiplier=1.0).output_shape == (None, 8, 8, 3)
    assert "mapping_layers" in models.__doc__


@pytest.mark.parametrize("eq,L,U,n", [(True, 6, 6, 1), (True, 10, 7, 3), (False, 5, 9, 2)])
def test_manual_backward_equals_autograd(eq, L, U, n):
    """The formulas of the engine's launch sequence (lrelu_bias_bwd with scale m, the transA gemm with scale c_l, the transB gemm with
    scale c_l, dL/dz at the bottom) against torch autograd, float64."""
    rng = np.random.default_rng(3)
    mp = layers.MappingNetwork(units=U, num_layers=n, lr_multiplier=0.01 if eq else 1.0, equalized_lr=eq)
    mp.out_shape((L,))
    T = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    params = {f"kernel_{l}": T(rng.normal(size=(L if l == 0 else U, U)) / mp.lr_multiplier) for l in range(n)}
    params.update({f"bias_{l}": T(rng.normal(size=U) / mp.lr_multiplier) for l in range(n)})
    z, dw = T(rng.normal(size=(4, L))), torch.tensor(rng.normal(size=(4, U)))
    w, hs, kink = R.torch_mapping(mp, z, params)
    assert kink > R.KINK
    names = sorted(params)
    auto = torch.autograd.grad((w * dw).sum(), [params[k] for k in names] + [z])
    with torch.no_grad():
        manual, dz = R.manual_mapping_backward(mp, z, hs, dw, params)
    for k, a in zip(names, auto[:-1]):
        np.testing.assert_allclose(manual[k].numpy(), a.numpy(), rtol=1e-12, atol=1e-12 * float(a.abs().max()), err_msg=k)
    np.testing.assert_allclose(dz.numpy(), auto[-1].numpy(), rtol=1e-12, atol=1e-14)


def test_w_avg_and_truncation_formulas():
    rng = np.random.default_rng(5)
    w, avg = rng.normal(size=(8, 7)).astype(np.float32), rng.normal(size=7).astype(np.float32)
    new = R.np_w_avg_update(avg, w, 0.995, 8)
    np.testing.assert_allclose(new, 0.995 * avg.astype(np.float64) + 0.005 * w.astype(np.float64).mean(0), rtol=1e-6, atol=1e-7)
    assert new.dtype == np.float32
    # two ranks' halves, each scaled by 1 / global batch and summed, give the global mean
    halves = sum(np.float64(1.0 / 8) * w[r * 4:(r + 1) * 4].astype(np.float64).sum(0) for r in range(2))
    np.testing.assert_allclose(halves, w.astype(np.float64).mean(0), rtol=1e-14)
    w64, a64 = w.astype(np.float64), avg.astype(np.float64)
    assert np.array_equal(R.np_truncate(w64, a64, 0.0), np.tile(a64, (8, 1)))
    np.testing.assert_allclose(R.np_truncate(w64, a64, 1.0), w64, rtol=1e-15)
    np.testing.assert_allclose(R.np_truncate(w64, a64, 0.5), 0.5 * (w64 + a64), rtol=1e-15)


def test_kernel_formulas_of_the_reference():
    rng = np.random.default_rng(6)
    x, W, b = rng.normal(size=(3, 4)), rng.normal(size=(4, 5)), rng.normal(size=5)
    y = R.np_dense_lrelu(x, W, b, c=0.5, bias_mul=0.25, alpha=0.2)
    pre = 0.5 * (x @ W) + 0.25 * b
    assert np.array_equal(y, np.where(pre > 0, pre, 0.2 * pre)) and np.array_equal(R.np_dense_lrelu(x, W, None), x @ W)
    g = rng.normal(size=(3, 5))
    gp, db = R.np_lrelu_bias_bwd(g, y, 0.2, old=np.ones(5), beta=1.0, scale=2.0)
    assert np.array_equal(gp, g * np.where(pre > 0, 1.0, 0.2)) and np.allclose(db, 1.0 + 2.0 * gp.sum(0))


@pytest.mark.parametrize("demo", ["demo_celeba", "demo_mnist"])
def test_demo_arguments(demo):
    import importlib
    parser = importlib.import_module(demo).make_parser()
    d = parser.parse_args([])
    assert (d.mapping_layers, d.mapping_units, d.mapping_lr_multiplier, d.truncation_psi) == (0, None, 0.01, None)
    a = parser.parse_args(["--generator-norm", "style", "--mapping-layers", "8", "--mapping-units", "512", "--mapping-lr-multiplier", "0.1",
                           "--truncation-psi", "0.7"])
    assert (a.mapping_layers, a.mapping_units, a.mapping_lr_multiplier, a.truncation_psi) == (8, 512, 0.1, 0.7)
    src = open(os.path.join(ROOT, demo + ".py")).read()
    assert "mapping_layers=args.mapping_layers" in src and "truncation_psi=args.truncation_psi" in src


def test_sample_grid_callback_takes_the_truncation():
    from blurred_gan_amd import callbacks
    cb = callbacks.GenerateSampleGridCallback(log_dir="/tmp/bg_test_logs", truncation_psi=0.7)
    assert cb.truncation_psi == 0.7 and callbacks.GenerateSampleGridCallback(log_dir="/tmp/bg_test_logs").truncation_psi is None


def test_checkpoint_configuration_record():
    g = models.DCGANGenerator(arch="tiny", normalization="style", equalized_lr=True, mapping_layers=2, mapping_units=7, mapping_lr_multiplier=0.1)
    g.build(CPU)
    assert json.loads(checkpoint._mapping_signature(g)) == dict(num_layers=2, units=7, lr_multiplier=0.1, equalized_lr=True)
    p = models.DCGANGenerator(arch="tiny")
    p.build(CPU)
    assert json.loads(checkpoint._mapping_signature(p)) is None


def test_abi_declares_and_binds_the_mapping_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bgan.h")).read()
    lib = _lib.load()
    for name in ("bg_dense_lrelu_plan", "bg_dense_lrelu_f32", "bg_lrelu_bias_bwd_workspace_bytes", "bg_lrelu_bias_bwd_f32", "bg_truncate_f32"):
        m = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert name in _lib.SIGNATURES and hasattr(lib, name) and len(args) == len(_lib.SIGNATURES[name][1]), name
    assert lib.bg_version() == 5 and _lib.ABI_VERSION == 5               # additions: the ABI version stays
    assert "mapping network" in hdr and _lib.DENSE_LRELU_PLAN_INTS == 4 and "BG_DENSE_LRELU_PLAN_INTS 4" in hdr
    from blurred_gan_amd import ops
    assert ops.mapping.plan(256, 512, 512) == dict(tile_m=32, tile_n=32, tile_k=64, workgroups=128)
    assert ops.mapping.plan(256, 100, 100)["workgroups"] == 32 and ops.mapping.workspace_bytes(256, 512) > 0
    csrc = open(os.path.join(ROOT, "blurred-gan_amd", "csrc", "mapping.hip")).read()
    assert "atomic" not in csrc.replace("No atomics", "").replace("no atomics", "") and "asm" not in csrc
