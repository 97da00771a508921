"""GPU tests of the DiffAugment kernels (bg_diffaug_f32, bg_diffaug_adjoint_f32) against the float64 numpy reference of
tests/diffaug_reference.py.

Every launch writes into a NaN-filled output between guard bands and reads inputs that must stay bit-unchanged.  Without ``color``
the transform is a gather and a mask: forward, linear part and adjoint are array_equal to the reference.  With ``color`` each is
held, in relative L2 over the launch's output, to max(4 x the deviation of the same formulas in float32 numpy from float64,
16 * 2^-24) -- tests/sn_reference.py: kernel_case's rule; every case prints error / bound.

Shapes: the issue's table, and the smallest square three-channel map the route query sends to the two-sweep route."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg  # noqa: F401
from blurred_gan_amd import ops
import diffaug_reference as DR
from helpers import Guarded, rel_l2

pytestmark = pytest.mark.gpu


def _smallest_two_sweep():
    h = 1
    while ops.diffaug.route(h, h, 3)["resident"]:
        h += 1
    return (1, h, h, 3)


SHAPES = [(1, 2, 2, 1), (3, 5, 7, 3), (2, 8, 8, 3), (5, 16, 12, 4), (2, 28, 28, 1), (70, 4, 4, 3), (3, 64, 64, 3), "two_sweep"]
GATHER_POLICIES = ["translation", "cutout", "translation,cutout"]
COLOR_POLICIES = ["color", "color,translation,cutout"]


def _shape(s):
    return _smallest_two_sweep() if s == "two_sweep" else s


def _ids(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


def _run(entry, src, params, cfg, offset=0, linear=False):
    """One guarded launch: returns the output array; asserts the guards, the inputs and that every output element was written."""
    shape = src.shape
    n = int(np.prod(shape))
    gin, gpar, gout = Guarded(n, init=src, offset=offset), Guarded(params.size, init=params), Guarded(n, offset=offset)
    a, p, o = gin.t(*shape), gpar.t(shape[0], 8), gout.t(*shape)
    if entry == "adj":
        ops.diffaug.adjoint(a, o, p, **cfg.kernel_args())
    else:
        ops.diffaug.fwd(a, o, p, **cfg.kernel_args(), linear=linear)
    torch.cuda.synchronize()
    assert gin.guards_intact() and gout.guards_intact() and gpar.guards_intact()
    assert gin.unchanged() and gpar.unchanged()
    return gout.get(*shape)


def _three(case, params, offset=0):
    cfg = case["cfg"]
    return dict(fwd=_run("fwd", case["x"], params, cfg, offset), lin=_run("fwd", case["x"], params, cfg, offset, linear=True),
                adj=_run("adj", case["g"], params, cfg, offset))


def test_routes():
    assert ops.diffaug.route(64, 64, 3)["resident"]
    n, h, w, c = _smallest_two_sweep()
    assert not ops.diffaug.route(h, w, c)["resident"] and ops.diffaug.route(h - 1, w - 1, c)["resident"]
    for s in SHAPES[:-1]:
        assert ops.diffaug.route(*s[1:])["resident"], s


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("policy", GATHER_POLICIES)
def test_translation_and_cutout_are_exact(shape, policy):
    shape = _shape(shape)
    for params in DR.injected_params(shape[0], 11):
        case = DR.kernel_case(shape, policy, 12, params)
        got = _three(case, params)
        for k in ("fwd", "lin", "adj"):
            assert not np.isnan(got[k]).any(), k
            assert np.array_equal(got[k], case["ref"][k].astype(np.float32)), (k, shape, policy)
        assert np.array_equal(got["fwd"], got["lin"])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("policy", COLOR_POLICIES)
def test_colour_matches_the_float64_reference(shape, policy):
    shape = _shape(shape)
    for params in DR.injected_params(shape[0], 21):
        case = DR.kernel_case(shape, policy, 22, params)
        got = _three(case, params)
        for k in ("fwd", "lin", "adj"):
            assert not np.isnan(got[k]).any(), k
            err, bound = rel_l2(got[k], case["ref"][k]), case["bound"][k]
            print(f"[diffaug {k}] {shape} {policy}: rel-L2 {err:.2e} / bound {bound:.2e} = {err / bound:.2f}")
            assert err <= bound, (k, shape, policy, err, bound)
        # the constant offset: forward - linear is b on live pixels, 0 elsewhere, within the forward's bound (of the output's scale)
        off = DR.offset_map(params, shape, case["cfg"])
        scale = float(np.linalg.norm(case["ref"]["fwd"]))
        d = float(np.linalg.norm((got["fwd"].astype(np.float64) - got["lin"]) - off))
        print(f"[diffaug offset] {shape} {policy}: {d / scale:.2e} / bound {case['bound']['fwd']:.2e}")
        assert d <= case["bound"]["fwd"] * scale
        assert not np.any((got["fwd"] != got["lin"]) & (off == 0))


@pytest.mark.parametrize("shape", [(3, 5, 7, 3), (2, 28, 28, 1), "two_sweep"], ids=_ids)
def test_misaligned_views_take_the_scalar_heads_and_tails(shape):
    """A view one float past a 16-byte boundary (and, with an odd sample size, samples at every alignment)."""
    shape = _shape(shape)
    params = DR.injected_params(shape[0], 31)[0]
    exact = DR.kernel_case(shape, "translation,cutout", 32, params)
    got = _three(exact, params, offset=1)
    for k in ("fwd", "lin", "adj"):
        assert np.array_equal(got[k], exact["ref"][k].astype(np.float32)), k
    case = DR.kernel_case(shape, "color,translation,cutout", 33, params)
    got = _three(case, params, offset=1)
    for k in ("fwd", "lin", "adj"):
        assert rel_l2(got[k], case["ref"][k]) <= case["bound"][k], k


@pytest.mark.parametrize("shape", [(5, 16, 12, 4), (70, 4, 4, 3), (3, 64, 64, 3)], ids=_ids)
def test_a_nan_sample_leaves_the_others_alone(shape):
    params = DR.injected_params(shape[0], 41)[0]
    case = DR.kernel_case(shape, "color,translation,cutout", 42, params)
    clean = _three(case, params)
    bad = dict(case, x=case["x"].copy(), g=case["g"].copy())
    bad["x"][1], bad["g"][1] = np.nan, np.nan
    got = _three(bad, params)
    keep = [i for i in range(shape[0]) if i != 1]
    for k in ("fwd", "lin", "adj"):
        assert np.array_equal(got[k][keep], clean[k][keep]), k
        assert np.isnan(got[k][1]).any(), k


@pytest.mark.parametrize("shape", [(70, 4, 4, 3), (3, 64, 64, 3), "two_sweep"], ids=_ids)
def test_two_runs_give_the_same_bits(shape):
    shape = _shape(shape)
    params = DR.injected_params(shape[0], 51)[0]
    case = DR.kernel_case(shape, "color,translation,cutout", 52, params)
    a, b = _three(case, params), _three(case, params)
    for k in ("fwd", "lin", "adj"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_neutral_policy_pieces_copy_bit_for_bit():
    """Without ``color`` values are moved, never computed with: a zero shift without cutout is the identity, bit for bit."""
    shape = (3, 8, 8, 3)
    x = np.random.default_rng(5).normal(size=shape).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    x[1, 2, 3, 1] = np.float32(1e-42)           # a denormal survives
    params = np.full((3, 8), 0.5, np.float32)   # decodes to a zero shift
    cfg = bg.DiffAugment("translation")
    assert DR.decode(params[0], 8, 8, cfg)["ty"] == 0 == DR.decode(params[0], 8, 8, cfg)["tx"]
    for entry in ("fwd", "adj"):
        assert np.array_equal(_run(entry, x, params, cfg).view(np.uint32), x.view(np.uint32)), entry


def test_overlapping_output_is_refused():
    x = torch.zeros(2, 4, 4, 3, device="cuda")
    p = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        ops.diffaug.fwd(x, x, p, 7, 0.125, 0.5)
    with pytest.raises(ValueError, match="overlap"):
        ops.diffaug.adjoint(x, x, p, 7, 0.125, 0.5)
