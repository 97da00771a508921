"""CPU tests of DiffAugment: the configuration class, the decode of a row of uniforms (the library's own, on the host, and the
reference's) against integers worked out by hand, the float64 reference itself (L^T is the adjoint of L and equals autograd through
the torch T), the boundary (symbols, refusals) and -- under the engine-trace recorders -- where the engine and the step enqueue the
two launches and which buffers they read and write."""
import ctypes as C
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import _lib, ops
import diffaug_reference as DR

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)


@pytest.fixture(scope="module")
def lib():
    maker.ensure_library(os.path.dirname(HERE))
    return _lib.load()


# ------------------------------------------------------------------ 1. configuration
def test_policy_parsing_and_canonical_order():
    a = bg.DiffAugment("cutout, color")
    assert a.policy == "color,cutout" and a.ops_mask == 5 and a.active
    assert bg.DiffAugment().policy == "color,translation,cutout" and bg.DiffAugment().ops_mask == 7
    assert bg.DiffAugment("translation").ops_mask == 2
    assert bg.DiffAugment().translation_ratio == 0.125 and bg.DiffAugment().cutout_ratio == 0.5
    for names in (("color",), ("cutout", "translation"), ("translation", "color", "cutout")):
        assert set(bg.DiffAugment(",".join(names)).policy.split(",")) == set(names)
    assert not bg.DiffAugment("").active and bg.DiffAugment("").ops_mask == 0


@pytest.mark.parametrize("bad", ["colour", "color,rotate", "color;cutout", "color,color"])
def test_unknown_names_are_refused(bad):
    with pytest.raises(ValueError):
        bg.DiffAugment(bad)


def test_bad_ratios_and_types_are_refused():
    for kw in (dict(translation_ratio=-0.1), dict(cutout_ratio=1.5), dict(translation_ratio="x"), dict(policy=3)):
        with pytest.raises(ValueError):
            bg.DiffAugment(**kw)
    with pytest.raises(ValueError):
        bg.diffaugment.as_augment(7)


def test_config_round_trip():
    a = bg.DiffAugment("cutout,translation", translation_ratio=0.25, cutout_ratio=0.3)
    b = bg.DiffAugment.from_config(a.get_config())
    assert a == b and b.get_config() == {"policy": "translation,cutout", "translation_ratio": 0.25, "cutout_ratio": 0.3}
    assert a != bg.DiffAugment("cutout,translation")


def test_as_augment_normalises():
    assert bg.diffaugment.as_augment(None) is None and bg.diffaugment.as_augment("") is None
    assert bg.diffaugment.as_augment("color") == bg.DiffAugment("color")
    a = bg.DiffAugment("cutout")
    assert bg.diffaugment.as_augment(a) is a


# ------------------------------------------------------------------ 2. decode
def _by_hand(u, n):
    """min(floor(fl32(u * n)), n - 1) with the product rounded to float32 once: u * n is exact in a Fraction."""
    prod = Fraction(float(np.float32(u))) * n
    return min(int(np.floor(np.float32(float(prod)))), n - 1)       # float(prod) is exact (24 + 5 bits), float32() rounds once


def _boundary_values(n):
    vals = [0.0, DR.HI]
    for k in range(1, n):
        b = np.float32(k / n)
        vals += [float(np.nextafter(b, np.float32(0))), float(b), float(np.nextafter(b, np.float32(1)))]
    return vals


@pytest.mark.parametrize("H,W", [(8, 8), (28, 28), (5, 7), (64, 64), (2, 2)])
def test_decode_at_the_boundaries_matches_hand_computed_integers(lib, H, W):
    cfg = bg.DiffAugment()
    Sy, Sx = int(np.floor(H * 0.125 + 0.5)), int(np.floor(W * 0.125 + 0.5))
    cy, cx = int(np.floor(H * 0.5 + 0.5)), int(np.floor(W * 0.5 + 0.5))
    ny, nx = H + 1 - cy % 2, W + 1 - cx % 2
    for u in sorted(set(_boundary_values(2 * Sy + 1) + _boundary_values(2 * Sx + 1) + _boundary_values(ny) + _boundary_values(nx))):
        row = np.full(8, u, np.float32)
        want = dict(ty=_by_hand(u, 2 * Sy + 1) - Sy, tx=_by_hand(u, 2 * Sx + 1) - Sx, y0=_by_hand(u, ny) - cy // 2,
                    x0=_by_hand(u, nx) - cx // 2, cy=cy, cx=cx)
        got, ref = ops.diffaug.decode(row, H, W), DR.decode(row, H, W, cfg)
        for k, v in want.items():
            assert got[k] == v == ref[k], (u, k, got[k], ref[k], v)
        for k, v in (("b", np.float32(u) - np.float32(0.5)), ("s", np.float32(2) * np.float32(u)), ("c", np.float32(u) + np.float32(0.5))):
            assert np.float32(got[k]) == v == ref[k], (u, k)
        assert -Sy <= got["ty"] <= Sy and -Sx <= got["tx"] <= Sx


def test_decode_hand_computed_cases(lib):
    # 8 x 8: S = 1, shifts out of 3 values; cutout 4 x 4, offsets out of 9 values, box from offset - 2
    d = ops.diffaug.decode([0.0] * 8, 8, 8)
    assert (d["ty"], d["tx"], d["y0"], d["x0"], d["cy"], d["cx"], d["Sy"], d["Sx"]) == (-1, -1, -2, -2, 4, 4, 1, 1)
    assert (d["b"], d["s"], d["c"]) == (-0.5, 0.0, 0.5)
    d = ops.diffaug.decode([DR.HI] * 8, 8, 8)
    assert (d["ty"], d["tx"], d["y0"], d["x0"]) == (1, 1, 6, 6) and d["c"] == 1.5
    # float32(1/3) lies above 1/3: the middle third starts there; one step below still falls in the lower third
    third = np.float32(1 / 3)
    assert ops.diffaug.decode([0, 0, 0, third, np.nextafter(third, np.float32(0)), 0, 0, 0], 8, 8)["ty"] == 0
    assert ops.diffaug.decode([0, 0, 0, third, np.nextafter(third, np.float32(0)), 0, 0, 0], 8, 8)["tx"] == -1
    # 2 x 2: cutout size 1 (odd): offsets out of 2 values, box from the offset itself; 5 x 7: sizes round half up to 3 and 4
    d = ops.diffaug.decode([0.6] * 8, 2, 2)
    assert (d["cy"], d["cx"], d["y0"], d["x0"], d["Sy"], d["ty"]) == (1, 1, 1, 1, 0, 0)
    d = ops.diffaug.decode([0.5] * 8, 5, 7)
    assert (d["cy"], d["cx"], d["Sy"], d["Sx"], d["ty"], d["tx"], d["y0"], d["x0"]) == (3, 4, 1, 1, 0, 0, 2 - 1, 4 - 2)


def test_absent_operations_decode_to_their_neutral_values(lib):
    u = [0.9] * 8
    d = ops.diffaug.decode(u, 8, 8, ops_mask=4)
    assert (d["b"], d["s"], d["c"], d["ty"], d["tx"]) == (0.0, 1.0, 1.0, 0, 0)
    d = ops.diffaug.decode(u, 8, 8, ops_mask=1)
    assert (d["ty"], d["tx"]) == (0, 0) and d["s"] == np.float32(1.8)
    assert DR.decode(u, 8, 8, bg.DiffAugment("translation"))["cy"] == 0


# ------------------------------------------------------------------ 3. the reference itself
SHAPES = [(1, 2, 2, 1), (3, 5, 7, 3), (2, 8, 8, 3), (5, 16, 12, 4)]
POLICIES = ["color", "translation", "cutout", "translation,cutout", "color,translation,cutout"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("policy", POLICIES)
def test_reference_adjoint_is_the_adjoint_of_the_linear_part(shape, policy):
    cfg = bg.DiffAugment(policy)
    rng = np.random.default_rng(3)
    for params in DR.injected_params(shape[0], 5):
        x, g = rng.normal(size=shape), rng.normal(size=shape)
        lhs = (DR.np_T(x, params, cfg, linear=True) * g).reshape(shape[0], -1).sum(1)
        rhs = (x * DR.np_LT(g, params, cfg)).reshape(shape[0], -1).sum(1)
        assert np.all(np.abs(lhs - rhs) <= 1e-12 * np.maximum(1.0, np.abs(lhs))), (lhs, rhs)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("policy", POLICIES)
def test_reference_equals_autograd_through_the_torch_transform(shape, policy):
    cfg = bg.DiffAugment(policy)
    rng = np.random.default_rng(4)
    for params in DR.injected_params(shape[0], 6):
        x, g = rng.normal(size=shape), rng.normal(size=shape)
        xt = torch.as_tensor(x).requires_grad_(True)
        y = DR.torch_T(xt, params, cfg)
        np.testing.assert_allclose(y.detach().numpy(), DR.np_T(x, params, cfg), rtol=0, atol=1e-12)
        np.testing.assert_allclose(DR.torch_T(xt, params, cfg, linear=True).detach().numpy(), DR.np_T(x, params, cfg, linear=True), rtol=0, atol=1e-12)
        gx, = torch.autograd.grad((y * torch.as_tensor(g)).sum(), xt)
        np.testing.assert_allclose(gx.numpy(), DR.np_LT(g, params, cfg), rtol=0, atol=1e-12)


def test_reference_offset_is_b_on_live_pixels():
    cfg, shape = bg.DiffAugment(), (4, 8, 8, 3)
    params = DR.injected_params(4, 9)[0]
    x = np.random.default_rng(1).normal(size=shape)
    off = DR.np_T(x, params, cfg) - DR.np_T(x, params, cfg, linear=True)
    np.testing.assert_allclose(off, DR.offset_map(params, shape, cfg), rtol=0, atol=1e-12)
    for k in range(4):
        vals = set(np.round(off[k].ravel(), 9))
        assert vals <= {0.0, round(float(DR.decode(params[k], 8, 8, cfg)["b"]), 9)}


def test_injected_params_hold_the_hard_rows():
    cfg = bg.DiffAugment()
    for n in (1, 2, 3, 5, 70):
        p = DR.injected_params(n, 2).reshape(-1, 8)
        d = [DR.decode(r, 16, 12, cfg) for r in p[:4]]
        assert {(x["ty"], x["tx"]) for x in d} == {(-2, -2), (-2, 2), (2, -2), (2, 2)}
        assert {(x["y0"], x["x0"]) for x in d} == {(-4, -3), (-4, 9), (12, -3), (12, 9)}
        assert any(x["s"] == 0 for x in d) and any(x["c"] == 0.5 for x in d)
        assert p.min() >= 0 and p.max() < 1


# ------------------------------------------------------------------ 4. boundary
def test_symbols_are_exported_and_bound(lib):
    for name in ("bg_diffaug_f32", "bg_diffaug_adjoint_f32", "bg_diffaug_route", "bg_diffaug_decode"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "DiffAugment" in bg.__all__ and bg.DiffAugment is bg.diffaugment.DiffAugment
    assert lib.bg_version() == 5


def test_route_query(lib):
    r = ops.diffaug.route(64, 64, 3)
    assert r["resident"] and r["resident_floats"] >= 64 * 64 * 3
    assert not ops.diffaug.route(128, 128, 3)["resident"]
    cap = r["resident_floats"]
    assert ops.diffaug.route(1, cap, 1)["resident"] and not ops.diffaug.route(1, cap + 1, 1)["resident"]
    with pytest.raises(ValueError):
        ops.diffaug.route(0, 4, 3)


def test_argument_errors_are_statuses(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    ok = dict(n=1, H=2, W=2, Cc=1)
    call = lambda x, y, u, n=1, H=2, W=2, Cc=1, mask=7, tr=0.125, cr=0.5: lib.bg_diffaug_f32(x, y, u, n, H, W, Cc, mask, tr, cr, 0, None)
    assert call(None, p, p) == -6 and call(p, None, p) == -6 and call(p, p + 64, None) == -6
    assert call(p, p + 64, p + 128, n=0) == -1 and call(p, p + 64, p + 128, H=0) == -1 and call(p, p + 64, p + 128, Cc=0) == -1
    assert call(p, p, p + 128) == -3                                  # y aliases x
    assert call(p, p + 8, p + 128) == -3                              # overlaps x
    assert b"overlap" in lib.bg_last_error()
    assert call(p, p + 64, p + 128, mask=8) == -3 and call(p, p + 64, p + 128, tr=1.5) == -3 and call(p, p + 64, p + 128, cr=-0.1) == -3
    assert call(p + 2, p + 64, p + 128) == -2
    assert lib.bg_diffaug_adjoint_f32(p, p, p + 128, 1, 2, 2, 1, 7, 0.125, 0.5, None) == -3
    assert lib.bg_diffaug_adjoint_f32(None, p, p + 128, 1, 2, 2, 1, 7, 0.125, 0.5, None) == -6
    assert ok


def test_cpu_tensors_are_rejected(lib):
    x = torch.zeros(1, 4, 4, 3)
    with pytest.raises(ops.BgDeviceError):
        ops.diffaug.fwd(x, torch.empty_like(x), torch.zeros(1, 8), 7, 0.125, 0.5)


# ------------------------------------------------------------------ 5. model surface
def _gan(cls=None, **kw):
    return maker._gan(bg, cls or bg.BlurredWGANGP, **kw)


def test_augment_argument_on_every_model_class():
    for cls, blur in ((bg.WGAN, False), (bg.WGANGP, False), (bg.BlurredWGANGP, True), (bg.BlurredWGAN, True)):
        assert _gan(cls, blur=blur).augment is None
        assert _gan(cls, blur=blur, augment="").augment is None
        assert _gan(cls, blur=blur, augment="cutout,color").augment == bg.DiffAugment("color,cutout")
        a = bg.DiffAugment("translation", translation_ratio=0.25)
        assert _gan(cls, blur=blur, augment=a).augment is a
    with pytest.raises(ValueError):
        _gan(augment="rotation")


def test_step_key_differs_between_policies_and_is_unchanged_without():
    reals = torch.zeros(2, 8, 8, 3)
    keys = {}
    for name, aug in (("none", None), ("empty", ""), ("color", "color"), ("full", bg.DiffAugment()), ("ratio", bg.DiffAugment(cutout_ratio=0.25))):
        gan = _gan(augment=aug)
        for m in (gan.generator, gan.discriminator):
            bg.optimizers.get_optimizer(m).attach(m.store)
        # the addresses in the key belong to each model's own buffers: compare the parts that do not
        keys[name] = tuple(k for k in gan._step_key("d", reals) if isinstance(k, tuple) and k and k[0] == "augment")
        base = [k for k in gan._step_key("d", reals) if not (isinstance(k, tuple) and k and k[0] == "augment")]
        assert len(base) == len(_gan()._step_key("d", reals))
    assert keys["none"] == keys["empty"] == ()
    assert len({keys["color"], keys["full"], keys["ratio"]}) == 3 and all(keys[k] for k in ("color", "full", "ratio"))


# ------------------------------------------------------------------ 6. what the engine and the step enqueue
class _Recorder:
    """Stands in for ops.diffaug under the engine-trace recorders."""

    def __init__(self, tr):
        self.tr = tr

    def _add(self, name, **kw):
        self.tr.add(name, kw)

    def fwd(self, x, y, params, ops_mask, translation_ratio, cutout_ratio, linear=False):
        self._add("diffaug.fwd", x=x, y=y, params=params, ops_mask=ops_mask, linear=bool(linear))
        return y

    def adjoint(self, dy, dx, params, ops_mask, translation_ratio, cutout_ratio):
        self._add("diffaug.adjoint", dy=dy, dx=dx, params=params, ops_mask=ops_mask)
        return dx


def _trace(run, **kw):
    tr = maker.Trace()
    torch.manual_seed(0)
    bg.layers.set_seed(3)
    with maker.tracing(bg, tr, **kw):
        saved = bg.ops.diffaug
        bg.ops.diffaug = _Recorder(tr)
        try:
            run(tr)
        finally:
            bg.ops.diffaug = saved
    return tr.calls


def _names(calls):
    return [c.split("(")[0] for c in calls]


def _arg(call, name):
    return call.split(name + "=")[1].split(",")[0].split(")")[0]


def _aug_rnd(B=2):
    rnd = maker._randomness(bg)
    for k in ("aug_fake", "aug_real", "aug_hat", "aug_g"):
        rnd[k] = np.full((B, 8), 0.5, np.float32)
    return rnd


@pytest.mark.parametrize("kw", [{}, dict(merge_gp_filter_gradients=False), dict(merge_critic_passes=False)], ids=["merged", "separate", "unmerged"])
@pytest.mark.parametrize("blur", [True, False], ids=["blur", "noblur"])
def test_the_step_enqueues_the_transform_around_every_critic_pass(lib, kw, blur):
    cls = bg.BlurredWGANGP if blur else bg.WGANGP
    calls = _trace(lambda tr: maker._train(_gan(cls, blur=blur, augment="color,translation,cutout", **kw)))
    plain = _trace(lambda tr: maker._train(_gan(cls, blur=blur, **kw)))
    names = _names(calls)
    unmerged = "merge_critic_passes" in kw
    fwd = [c for c in calls if c.startswith("diffaug.fwd") and "linear=False" in c]
    lin = [c for c in calls if c.startswith("diffaug.fwd") and "linear=True" in c]
    adj = [c for c in calls if c.startswith("diffaug.adjoint")]
    # D-step: one transform per critic forward (one 3B pass, or 2B + B), one L^T for the x-hat rows, one L for the seed; G-step: one each way
    assert len(fwd) == (3 if unmerged else 2) and len(lin) == 1 and len(adj) == 2
    rows = sorted(int(_arg(c, "x").split(":")[1].split("x")[0]) for c in fwd)
    assert rows == ([2, 2, 4] if unmerged else [2, 6])
    assert all(int(_arg(c, "dy").split(":")[1].split("x")[0]) == 2 for c in adj)
    # one draw of [3B, 8] in the D-step and one of [B, 8] in the G-step
    draws = [c for c in calls if c.startswith("uniform(") and ("x8:" in c)]
    assert [_arg(c, "out").split(":")[1] for c in draws] == ["6x8", "2x8"]
    # every transform reads one buffer and writes another, and the conv that follows reads what it wrote
    for c in fwd:
        i = calls.index(c)
        assert _arg(c, "x").split("+")[0] != _arg(c, "y").split("+")[0]
        nxt = next(k for k in calls[i + 1:] if k.startswith("conv2d_fwd"))
        assert _arg(nxt, "x").split(":")[0] == _arg(c, "y").split(":")[0]
    for c in adj:
        assert _arg(c, "dy").split("+")[0] != _arg(c, "dx").split("+")[0]
        if blur:                        # blur^T follows L^T and reads its output
            nxt = calls[calls.index(c) + 1]
            assert nxt.startswith("blur_nhwc") and _arg(nxt, "x") == _arg(c, "dx")
    if blur:                            # the seed: blur, then L
        i = calls.index(lin[0])
        assert calls[i - 1].startswith("blur_nhwc") and _arg(calls[i - 1], "y") == _arg(lin[0], "x")
    if kw == {}:                        # merged filter gradients: the seed lands in the x-hat rows of the augmented batch
        big = next(c for c in fwd if _arg(c, "x").split(":")[1].startswith("6x"))
        assert _arg(lin[0], "y").split("+")[0] == _arg(big, "y").split("+")[0] and _arg(lin[0], "y").split("+")[1].startswith(str(4 * 8 * 8 * 3))
    # without the augmentation's own calls the launch list is the plain step's, name for name
    rest = [n for c, n in zip(calls, names) if not n.startswith("diffaug") and not (n == "uniform" and "x8:" in c)]
    assert rest == _names(plain)


def test_injected_params_reach_the_launches_and_draw_nothing(lib):
    calls = _trace(lambda tr: maker._train(_gan(augment="cutout"), randomness=_aug_rnd()))
    assert not [c for c in calls if c.startswith("uniform(") and "x8:" in c]
    assert len([c for c in calls if c.startswith("diffaug")]) == 5
    assert all("ops_mask=4" in c for c in calls if c.startswith("diffaug"))
    with pytest.raises(ValueError, match="all or none"):
        rnd = _aug_rnd()
        del rnd["aug_hat"]
        _trace(lambda tr: maker._train(_gan(augment="cutout"), randomness=rnd))


def test_plain_wgan_draws_two_blocks(lib):
    calls = _trace(lambda tr: maker._train(_gan(bg.WGAN, blur=False, augment="translation")))
    draws = [c for c in calls if c.startswith("uniform(") and "x8:" in c]
    assert [_arg(c, "out").split(":")[1] for c in draws] == ["4x8", "2x8"]
    assert len([c for c in calls if c.startswith("diffaug.adjoint")]) == 1          # the G-step's only: the D-step wants no input gradient


def test_layer_normalization_critic_keeps_the_augmented_batch_for_the_source_backward(lib):
    def run(tr):
        bg.layers.set_seed(3)
        gen, disc = bg.models.DCGANGenerator(arch="tiny"), bg.models.DCGANDiscriminator(arch="tiny", normalization="layer")
        for m in (gen, disc):
            m.build("cpu")
        hp = bg.BlurredWGANGP.HyperParameters(batch_size=2, global_batch_size=2, initial_blur_std=0.9)
        gan = bg.BlurredWGANGP(gen, disc, hp, bg.TrainingConfig(log_dir=os.devnull), step_replay=False, augment="color")
        saved = bg.ops.layernorm
        bg.ops.layernorm = _LnStub()
        try:
            maker._train(gan)
        finally:
            bg.ops.layernorm = saved
    calls = _trace(run)
    big = next(c for c in calls if c.startswith("diffaug.fwd") and _arg(c, "x").split(":")[1].startswith("6x"))
    label = _arg(big, "y").split("+")[0]
    after = calls[calls.index(big) + 1:]
    writers = ("y=", "dx=", "out=", "dst=", "dw=")
    for c in after:
        if c.startswith("uniform("):          # the G-step begins
            break
        for w in writers:
            if w in c and not c.startswith("diffaug.fwd"):
                assert _arg(c, w[:-1]).split("+")[0] != label, c
    # the last filter gradient of the D-step (the source backward's layer 1) reads the x-hat rows of the augmented batch
    wg = [c for c in after if c.startswith("conv2d_bwd_filter") and _arg(c, "x").split("+")[0] == label]
    assert any(_arg(c, "x").split("+")[1].startswith(str(4 * 8 * 8 * 3)) for c in wg)


class _LnStub:
    """ops.layernorm on CPU tensors: returns the output operand, answers the host queries."""

    route = staticmethod(ops.layernorm.route)
    workspace_bytes = staticmethod(lambda R, Cc: 0)
    fwd = staticmethod(lambda z, a, **k: a)
    bwd = staticmethod(lambda g, z, dz, **k: dz)
    tangent = staticmethod(lambda zdot, z, vout, **k: vout)
    gp_source = staticmethod(lambda u, zdot, z, s, **k: s)


# ------------------------------------------------------------------ 7. the code objects
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_kernels_use_no_private_memory_fit_eight_waves_and_move_float4(tmp_path):
    """Two 1024-thread workgroups per compute unit (the resident route's plan) need at most 64 vector registers and no scratch.
    (Scalar registers: the eight-waves request caps them, and the compiler parks a few uniform values in vector-register LANES --
    sgpr_spill_count is not zero; nothing goes to memory, which is what private_segment_fixed_size == 0 says.)"""
    import re
    import subprocess
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "diffaug.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(os.path.dirname(HERE), "blurred-gan_amd", "csrc", "diffaug.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    kernels = list(re.finditer(r"\.name:\s+(\S*diffaug_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S))
    names = [m.group(1) for m in kernels]
    assert len(names) == 4, names           # forward / adjoint x resident / two-sweep
    for m in kernels:
        for key in ("vgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)
        v = re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        assert v and int(v.group(1)) <= 64, (m.group(1), v and v.group(1))
    for name in names:
        body = re.search(r"^" + re.escape(name) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
