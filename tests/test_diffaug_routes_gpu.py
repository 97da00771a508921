"""GPU: the DiffAugment kernels on the case table of tests/diffaug_cases.py -- the launches of csrc/diffaug.hip that the shapes of
tests/test_diffaug_gpu.py do not reach (tests/test_diffaug_cases_cpu.py holds each case to its claim through bg_diffaug_plan).

Every launch runs through guarded buffers as in tests/test_diffaug_gpu.py: a NaN-filled output between guard bands, inputs that must
stay bit-unchanged, at every view offset the case lists.  Gather policies are array_equal to the reference.  Colour policies are held
PER SAMPLE to max(4 x the float32-numpy error of that sample, 16 * 2^-24), relative to the sample's own norm, so one wrong sample
among a thousand is not diluted; on the two power-of-two cases they run on data where every intermediate is a float32 number and
must be array_equal to the float64 reference."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg  # noqa: F401
from blurred_gan_amd import ops
import diffaug_cases as DC
import diffaug_reference as DR
from helpers import Guarded

pytestmark = pytest.mark.gpu

KEYS = ("fwd", "lin", "adj")


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
    out = gout.get(*shape)
    assert not np.isnan(out).any(), (entry, shape, offset, "output elements left unwritten", int(np.isnan(out).sum()))
    return out


def _three(x, g, params, cfg, offset=0):
    return dict(fwd=_run("fwd", x, params, cfg, offset), lin=_run("fwd", x, params, cfg, offset, linear=True), adj=_run("adj", g, params, cfg, offset))


def _special_at(case):
    return (1024,) if case["second_sample_trip"] else ()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
@pytest.mark.parametrize("policy", DC.GATHER_POLICIES)
def test_gather_policies_are_exact(case, policy):
    shape, cfg = case["shape"], DR.as_cfg(policy)
    rng = np.random.default_rng(12)
    x, g = rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32)
    for params in DC.params_for(case, 11, _special_at(case)):
        want = dict(fwd=DR.np_T(x, params, cfg), lin=DR.np_T(x, params, cfg, linear=True), adj=DR.np_LT(g, params, cfg))
        for offset in case["offsets"]:
            got = _three(x, g, params, cfg, offset)
            for k in KEYS:
                assert np.array_equal(got[k], want[k].astype(np.float32)), (k, shape, policy, offset)


@pytest.mark.parametrize("case", DC.WITH_COLOR, ids=[DC.case_id(c) for c in DC.WITH_COLOR])
@pytest.mark.parametrize("policy", DC.COLOR_POLICIES)
def test_colour_matches_float64_sample_by_sample(case, policy):
    shape = case["shape"]
    worst = dict.fromkeys(KEYS, 0.0)
    failed = []
    for params in DC.params_for(case, 21, _special_at(case)):
        ref = DC.per_sample_case(shape, policy, 22, params)
        for offset in case["offsets"]:
            got = _three(ref["x"], ref["g"], params, ref["cfg"], offset)
            for k in KEYS:
                ratio = DC.sample_errors(got[k], ref["ref"][k]) / ref["bound"][k]
                i = int(np.argmax(ratio))
                worst[k] = max(worst[k], float(ratio[i]))
                if not ratio[i] <= 1:
                    failed.append((k, offset, i, float(ratio[i]) * float(ref["bound"][k][i]), float(ref["bound"][k][i])))
    print(f"[diffaug routes] {DC.case_id(case)} {policy}: worst error / bound per sample: " + ", ".join(f"{k} {worst[k]:.2f}" for k in KEYS))
    assert not failed, (shape, policy, "(entry, offset, sample, error, bound)", failed[:8])


@pytest.mark.parametrize("case", DC.EXACT, ids=[DC.case_id(c) for c in DC.EXACT])
@pytest.mark.parametrize("policy", DC.COLOR_POLICIES)
def test_colour_is_exact_on_integer_data(case, policy):
    ex = DC.exact_case(case["shape"], policy, seed=61)
    got = _three(ex["x"], ex["g"], ex["params"], ex["cfg"])
    for k in KEYS:
        want = ex["ref"][k].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ex["ref"][k])
        bad = np.argwhere(got[k] != want)
        assert not len(bad), (k, case["shape"], policy, f"{len(bad)} of {want.size} differ; first at {tuple(bad[0])}: got {got[k][tuple(bad[0])]!r}, "
                              f"want {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("case", DC.REPEAT, ids=[DC.case_id(c) for c in DC.REPEAT])
def test_repeat_runs_give_the_same_bits(case):
    """Every workgroup of a sample recomputes the mean, and a workgroup that takes a second sample reuses its LDS: a sample's output
    must not depend on which workgroup wrote it, or when."""
    shape = case["shape"]
    params = DC.params_for(case, 51, _special_at(case))[0]
    ref = DC.per_sample_case(shape, "color,translation,cutout", 52, params) if shape[0] <= 8 else None
    rng = np.random.default_rng(52)
    x, g = (ref["x"], ref["g"]) if ref else (rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32))
    cfg = DR.as_cfg("color,translation,cutout")
    for offset in case["offsets"]:
        a, b = _three(x, g, params, cfg, offset), _three(x, g, params, cfg, offset)
        for k in KEYS:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, shape, offset)
    if case["second_sample_trip"]:
        # the second trip's samples, run as a batch of their own (first trip of their workgroups), give the same bits: grid_x * E is
        # a multiple of 4 floats, so they keep their alignment and with it the order of their sums
        lo = ops.diffaug.plan(*shape, 7)["grid_x"]
        assert lo * int(np.prod(shape[1:])) % 4 == 0
        sub = _three(x[lo:], g[lo:], params[lo:], cfg)
        for k in KEYS:
            assert np.array_equal(_bits(a[k][lo:]), _bits(sub[k])), k


def test_first_size_past_the_resident_cap_takes_two_sweeps():
    """The first E behind resident_floats, found through the query, at view offsets 0 and 3."""
    rf = ops.diffaug.route(1, 1, 1)["resident_floats"]
    shape = (1, 1, rf + 1, 1)
    assert ops.diffaug.plan(1, 1, rf, 1, 1)["resident"] and not ops.diffaug.plan(*shape, 1)["resident"]
    params = DR.injected_params(1, 71)[3]
    ref = DC.per_sample_case(shape, "color,translation,cutout", 72, params)
    for offset in (0, 3):
        got = _three(ref["x"], ref["g"], params, ref["cfg"], offset)
        for k in KEYS:
            err = DC.sample_errors(got[k], ref["ref"][k])
            assert (err <= ref["bound"][k]).all(), (k, offset, err, ref["bound"][k])
