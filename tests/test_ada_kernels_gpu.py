"""GPU tests of the gated DiffAugment kernels (bg_diffaug_gated_f32, bg_diffaug_gated_adjoint_f32) and of the controller kernels
(bg_ada_stats_f32, bg_ada_update_f32).

The gated kernels are held to the ungated ones and to numpy, bit for bit: at p = 1 they ARE the ungated calls on params[:, :8]; at
p = 0 they copy; with mixed gates a sample whose colour did not fire is the numpy gather of tests/ada_reference.py and one whose
colour fired is the ungated call on that sample alone with ops_mask = policy & fired.  (A sample's sum order depends on the
workgroup size, the route and the sample's 16-byte alignment; the first two follow from the policy's colour bit and the sample
size, and the batch of one is placed at the alignment the sample has inside its batch, so it adds in the same order: the comparison
is exact, and no tolerance is used anywhere in this file.)  Shapes: the route cases of
tests/diffaug_cases.py -- both routes, both workgroup sizes, a cut output, the sample loop's second trip, a float4 across a pixel
boundary -- two of them at view offsets 1-3.  Every launch writes into a NaN-filled output between guard bands.

Adjointness is held to the bound of the one existing DiffAugment adjointness test (tests/test_diffaug_cpu.py: |lhs - rhs| <= 1e-12 *
max(1, |lhs|) per sample, in float64).  That bound is a float64 rounding bound, so it is asked where the fp32 outputs carry no
rounding of their own: under the gather policies on any data (values are moved, never computed with) and under the colour policies
on the exact integer data of diffaug_cases.exact_case (its two power-of-two cases), where every intermediate is a float32 number.

The controller runs on exact data: counts times a power-of-two 1 / speed_images, so every p is exact and the state must equal the
Python rule of tests/ada_reference.py bit for bit at every step."""
import numpy as np
import pytest
import torch

import blurred_gan_amd as bg  # noqa: F401
from blurred_gan_amd import ops
import ada_reference as AR
import diffaug_cases as DC
import diffaug_reference as DR
from helpers import Guarded

pytestmark = pytest.mark.gpu

F32 = np.float32
FULL, GATHER = "color,translation,cutout", "translation,cutout"
ROUTE_SHAPES = [(3, 32, 32, 4), (3, 35, 37, 3), (2, 71, 71, 3), (2, 64, 64, 4), (2, 91, 91, 3), (1030, 3, 3, 3), (2, 6, 5, 5)]
ROUTE_CASES = [c for c in DC.CASES if c["shape"] in ROUTE_SHAPES]
ROUTE_IDS = [DC.case_id(c) for c in ROUTE_CASES]
assert len(ROUTE_CASES) == len(ROUTE_SHAPES)
OFFSET_SHAPES = {(3, 35, 37, 3), (2, 6, 5, 5)}           # run at view offsets 0-3 (an odd sample size: every sample alignment)
ADJOINT_BOUND = 1e-12                                    # tests/test_diffaug_cpu.py test_reference_adjoint_is_the_adjoint_of_the_linear_part


def _offsets(case):
    return (0, 1, 2, 3) if case["shape"] in OFFSET_SHAPES else (0,)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _dev_p(p):
    return torch.full((1,), float(p), dtype=torch.float32, device="cuda")


def _run(entry, src, params, cfg, p=None, offset=0, linear=False):
    """One guarded launch of the gated (``p`` a device float) or ungated (``p`` None) entry point."""
    shape = src.shape
    n = int(np.prod(shape))
    gin, gpar, gout = Guarded(n, init=src, offset=offset), Guarded(params.size, init=params), Guarded(n, offset=offset)
    a, u, o = gin.t(*shape), gpar.t(*params.shape), gout.t(*shape)
    if p is None:
        assert params.shape[1] == 8
        if entry == "adj":
            ops.diffaug.adjoint(a, o, u, **cfg.kernel_args())
        else:
            ops.diffaug.fwd(a, o, u, **cfg.kernel_args(), linear=linear)
    else:
        assert params.shape[1] == 12
        if entry == "adj":
            ops.diffaug.adjoint_gated(a, o, u, p, **cfg.kernel_args())
        else:
            ops.diffaug.fwd_gated(a, o, u, p, **cfg.kernel_args(), linear=linear)
    torch.cuda.synchronize()
    assert gin.guards_intact() and gout.guards_intact() and gpar.guards_intact()
    assert gin.unchanged() and gpar.unchanged()
    out = gout.get(*shape)
    assert not np.isnan(out).any(), (entry, shape, offset, "output elements left unwritten", int(np.isnan(out).sum()))
    return out


ENTRIES = (("fwd", "x", False), ("lin", "x", True), ("adj", "g", False))


def _three(data, params, cfg, p=None, offset=0):
    return {k: _run("adj" if k == "adj" else "fwd", data[src], params, cfg, p, offset, linear) for k, src, linear in ENTRIES}


def _data(shape, seed):
    rng = np.random.default_rng(seed)
    d = dict(x=rng.normal(size=shape).astype(F32), g=rng.normal(size=shape).astype(F32))
    d["x"].flat[0], d["g"].flat[0] = -0.0, F32(1e-42)            # a negative zero and a denormal survive a copy
    return d


def _params12(case, seed, masks=None):
    """[n, 12]: the hard rows of diffaug_reference.injected_params (repeated in the sample loop's second trip), seeded gates or the
    gates of ``masks``."""
    n = case["shape"][0]
    p8 = DC.params_for(case, seed, special_at=(1024,) if case["second_sample_trip"] else ())[0]
    if masks is not None:
        return AR.with_gates(p8, masks)
    gates = np.minimum(np.random.default_rng(seed + 1).uniform(size=(n, 4)).astype(F32), F32(DR.HI))
    return np.concatenate([p8, gates], axis=1)


# ------------------------------------------------------------------ 1. p = 1 and p = 0
@pytest.mark.parametrize("case", ROUTE_CASES, ids=ROUTE_IDS)
@pytest.mark.parametrize("policy", [FULL, "color", GATHER])
def test_p_one_is_the_ungated_call_bit_for_bit(case, policy):
    shape, cfg = case["shape"], DR.as_cfg(policy)
    data, params = _data(shape, 71), _params12(case, 72)
    one = _dev_p(1.0)
    for offset in _offsets(case):
        got, want = _three(data, params, cfg, one, offset), _three(data, np.ascontiguousarray(params[:, :8]), cfg, None, offset)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, shape, policy, offset)


@pytest.mark.parametrize("case", ROUTE_CASES, ids=ROUTE_IDS)
def test_p_zero_copies_bit_for_bit(case):
    shape, cfg = case["shape"], DR.as_cfg(FULL)
    data, params = _data(shape, 73), _params12(case, 74)
    params[0, 8:11] = 0.0                                        # the smallest gate there is: 0 < 0 does not hold
    zero = _dev_p(0.0)
    for offset in _offsets(case):
        got = _three(data, params, cfg, zero, offset)
        assert np.array_equal(_bits(got["fwd"]), _bits(data["x"])) and np.array_equal(_bits(got["lin"]), _bits(data["x"]))
        assert np.array_equal(_bits(got["adj"]), _bits(data["g"]))


# ------------------------------------------------------------------ 2. mixed gates
def _mask_batches(n):
    """Lists of per-sample fired masks.  n >= 8: all eight masks in one batch, from the first sample on and on the last eight (so
    in the sample loop's second trip too), once more shifted.  Smaller batches: eight of them, batch b = masks b, b + 1, ...: every
    mask on the first and on the last sample."""
    if n >= 8:
        cyc = [[(i + r) % 8 for i in range(n)] for r in (0, 3)]
        for m in cyc:
            m[-8:] = [(7 - i) % 8 for i in range(8)]
        return cyc
    return [[(b + i) % 8 for i in range(n)] for b in range(8)]


@pytest.mark.parametrize("case", ROUTE_CASES, ids=ROUTE_IDS)
def test_mixed_gates_sample_by_sample(case):
    shape, cfg = case["shape"], DR.as_cfg(FULL)
    n = shape[0]
    data = _data(shape, 75)
    half = _dev_p(0.5)
    seen_first, seen_last = set(), set()
    for b, masks in enumerate(_mask_batches(n)):
        params = _params12(case, 76 + b, masks)
        assert [AR.fired_mask(params[i], 0.5, cfg) for i in range(n)] == masks
        seen_first.add(masks[0]), seen_last.add(masks[-1])
        if n >= 8:
            assert set(masks) == set(range(8)) and set(masks[1024:]) >= {1, 0} and len(set(masks[1024:])) >= 6
        offset = _offsets(case)[b % len(_offsets(case))]
        got = _three(data, params, cfg, half, offset)
        # colour off: the numpy gather, bit for bit (float32 numpy moves values and computes nothing)
        off = [i for i in range(n) if not masks[i] & 1]
        ref = {k: (AR.np_LT(data["g"][off], params[off], 0.5, cfg, dtype=F32) if k == "adj" else
                   AR.np_T(data["x"][off], params[off], 0.5, cfg, dtype=F32)) for k in got}
        for k in got:
            assert np.array_equal(_bits(got[k][off]), _bits(ref[k])), (k, shape, b, "colour off")
        # colour on: the ungated call on the sample alone with ops_mask = policy & fired, at the sample's own alignment in the batch
        # (an odd sample size: the scalar head, and with it the order of the sample's sum, follows the address).  Every sample of a
        # small batch; of a large one the first of each mask, the last and the first of the second trip
        on = [i for i in range(n) if masks[i] & 1]
        alone = on if n < 8 else sorted({min(i for i in on if masks[i] == m) for m in (1, 3, 5, 7)} | {on[-1], min(i for i in on if i >= 1024)})
        E = int(np.prod(shape[1:]))
        for i in alone:
            sub = DR.as_cfg(AR.policy_of(masks[i]))
            one = {k: data[k][i:i + 1] for k in data}
            want = _three(one, np.ascontiguousarray(params[i:i + 1, :8]), sub, None, (offset + i * E) % 4)
            for k in got:
                assert np.array_equal(_bits(got[k][i:i + 1]), _bits(want[k])), (k, shape, b, i, masks[i], "colour on, alone")
    assert seen_first == set(range(8)) == seen_last or n >= 8


@pytest.mark.parametrize("case", [c for c in ROUTE_CASES if c["shape"] in ((3, 35, 37, 3), (2, 91, 91, 3), (1030, 3, 3, 3))], ids=DC.case_id)
def test_mixed_gates_of_a_policy_without_colour_are_the_numpy_gather(case):
    shape, cfg = case["shape"], DR.as_cfg(GATHER)
    data, params = _data(shape, 81), _params12(case, 82)
    got = _three(data, params, cfg, _dev_p(0.5))
    fired = {AR.fired_mask(u, 0.5, cfg) for u in params}
    assert fired == ({0, 2, 4, 6} if shape[0] >= 8 else fired) and not any(f & 1 for f in fired)
    assert np.array_equal(_bits(got["fwd"]), _bits(AR.np_T(data["x"], params, 0.5, cfg, dtype=F32)))
    assert np.array_equal(_bits(got["lin"]), _bits(got["fwd"]))
    assert np.array_equal(_bits(got["adj"]), _bits(AR.np_LT(data["g"], params, 0.5, cfg, dtype=F32)))


# ------------------------------------------------------------------ 3. adjointness
def _adjoint_gap(x, g, lin, adj):
    n = x.shape[0]
    lhs = (lin.astype(np.float64) * g).reshape(n, -1).sum(1)
    rhs = (x.astype(np.float64) * adj).reshape(n, -1).sum(1)
    return lhs, rhs


@pytest.mark.parametrize("case", ROUTE_CASES, ids=ROUTE_IDS)
def test_adjointness_of_the_gather(case):
    shape, cfg = case["shape"], DR.as_cfg(GATHER)
    data, params = _data(shape, 83), _params12(case, 84)
    half = _dev_p(0.5)
    lin, adj = _run("fwd", data["x"], params, cfg, half, linear=True), _run("adj", data["g"], params, cfg, half)
    lhs, rhs = _adjoint_gap(data["x"], data["g"], lin, adj)
    print(f"[ada adjointness, gather] {shape}: max gap {np.abs(lhs - rhs).max():.2e}")
    assert np.all(np.abs(lhs - rhs) <= ADJOINT_BOUND * np.maximum(1.0, np.abs(lhs))), (lhs, rhs)


@pytest.mark.parametrize("case", [c for c in DC.EXACT if c["shape"] in ROUTE_SHAPES], ids=DC.case_id)
@pytest.mark.parametrize("policy", DC.COLOR_POLICIES)
def test_adjointness_with_colour_on_exact_data(case, policy):
    shape = case["shape"]
    ex = DC.exact_case(shape, policy, seed=85)
    gate_rows = [(3 * i + 1) % 8 for i in range(shape[0])]
    for masks in (gate_rows, [7] * shape[0], [1] * shape[0]):
        params = AR.with_gates(ex["params"], masks)
        half = _dev_p(0.5)
        lin, adj = _run("fwd", ex["x"], params, ex["cfg"], half, linear=True), _run("adj", ex["g"], params, ex["cfg"], half)
        assert np.array_equal(lin, AR.np_T(ex["x"], params, 0.5, ex["cfg"], linear=True).astype(F32))
        assert np.array_equal(adj, AR.np_LT(ex["g"], params, 0.5, ex["cfg"]).astype(F32))
        lhs, rhs = _adjoint_gap(ex["x"], ex["g"], lin, adj)
        print(f"[ada adjointness, colour, exact data] {shape} {policy} {masks}: max gap {np.abs(lhs - rhs).max():.2e}")
        assert np.all(np.abs(lhs - rhs) <= ADJOINT_BOUND * np.maximum(1.0, np.abs(lhs))), (lhs, rhs)


# ------------------------------------------------------------------ 4. p is read when the kernel runs
@pytest.mark.parametrize("shape", [(3, 35, 37, 3), (2, 91, 91, 3)], ids=lambda s: "x".join(map(str, s)))
def test_p_is_read_at_launch_time(shape):
    """The property step replay rests on: the same call, with the same arguments, follows the device float."""
    case = next(c for c in ROUTE_CASES if c["shape"] == shape)
    cfg = DR.as_cfg(FULL)
    data, params = _data(shape, 86), _params12(case, 87)
    x, g, u = (torch.from_numpy(a).cuda() for a in (data["x"], data["g"], params))
    p = _dev_p(0.0)
    outs = {}
    for value in (0.0, 1.0):
        p.fill_(value)
        y, dx = torch.full_like(x, float("nan")), torch.full_like(g, float("nan"))
        ops.diffaug.fwd_gated(x, y, u, p, **cfg.kernel_args())
        ops.diffaug.adjoint_gated(g, dx, u, p, **cfg.kernel_args())
        torch.cuda.synchronize()
        outs[value] = (y.cpu().numpy(), dx.cpu().numpy())
    assert np.array_equal(_bits(outs[0.0][0]), _bits(data["x"])) and np.array_equal(_bits(outs[0.0][1]), _bits(data["g"]))
    p8 = np.ascontiguousarray(params[:, :8])
    assert np.array_equal(_bits(outs[1.0][0]), _bits(_run("fwd", data["x"], p8, cfg)))
    assert np.array_equal(_bits(outs[1.0][1]), _bits(_run("adj", data["g"], p8, cfg)))
    assert not np.array_equal(outs[0.0][0], outs[1.0][0]) and not np.array_equal(outs[0.0][1], outs[1.0][1])


def test_overlap_and_null_p_are_refused():
    x, u, p = torch.zeros(2, 4, 4, 3, device="cuda"), torch.zeros(2, 12, device="cuda"), _dev_p(0.5)
    with pytest.raises(ValueError, match="overlap"):
        ops.diffaug.fwd_gated(x, x, u, p, 7, 0.125, 0.5)
    with pytest.raises(ValueError, match="overlap"):
        ops.diffaug.adjoint_gated(x, x, u, p, 7, 0.125, 0.5)


# ------------------------------------------------------------------ 5. the controller
def _scores(kind, n, rng):
    """A score vector of n entries whose sign sum is > 0 (up), < 0 (down) or exactly 0 (level), with zeros, NaN and +-inf among
    them wherever n has room."""
    s = rng.uniform(0.5, 2.0, size=n).astype(F32)
    if kind == "down":
        s = -s
    if kind == "level":
        s[:n // 2] *= -1
        if n % 2:
            s[-1] = 0.0 if n > 1 else np.nan
        if n >= 8:
            s[0], s[-2 - n % 2] = -np.inf, np.inf
            s[1], s[-3 - n % 2] = np.nan, -0.0              # one from either side: the sum stays 0
    elif n >= 8:
        big = np.inf if kind == "up" else -np.inf
        s[0], s[1], s[2], s[3] = big, np.nan, 0.0, -big
    elif n == 1:
        s[0] = np.inf if kind == "up" else -np.inf
    return s


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_controller_equals_the_python_rule_bit_for_bit(n, interval):
    speed = float(2 ** int(np.ceil(np.log2(4 * n * interval))))          # an adjustment is n * interval / speed in (1/8, 1/4], exact
    target = 0.0
    ref = AR.Controller(0.5, target, interval, speed)
    rng = np.random.default_rng(n + interval)
    script = ["up"] * (5 * interval) + ["level"] * interval + ["down"] * (10 * interval) + ["level"] * interval + ["up"] * (interval + interval // 2)
    g_scores, g_stats, g_state, g_met = Guarded(n, init=np.zeros(n, F32), offset=1), Guarded(4), Guarded(8, init=ref.state()), Guarded(2)
    ps = []
    for i, kind in enumerate(script):
        s = _scores(kind, n, rng)
        g_scores.view.copy_(torch.from_numpy(s))
        ops.ada.stats(g_scores.t(n), g_stats.t(4))
        ops.ada.update(g_stats.t(4), g_state.t(8), g_met.t(2), target, interval, 1.0 / speed)
        torch.cuda.synchronize()
        want_stats = AR.sign_stats(s)
        want = ref.step(s)
        assert np.array_equal(_bits(g_stats.get()), _bits(np.array([*want_stats, 0, 0], F32))), (i, kind, g_stats.get(), want_stats)
        assert np.array_equal(_bits(g_state.get()), _bits(want)), (i, kind, g_state.get(), want)
        assert np.array_equal(_bits(g_met.get()), _bits(want[[0, 4]])), (i, kind, g_met.get(), want)
        ps.append(float(want[0]))
    assert all(g.guards_intact() for g in (g_scores, g_stats, g_state, g_met))
    assert max(ps) == 1.0 and min(ps) == 0.0 and ps[-1] > 0.0            # both clamps were reached, and p left the lower one again
    level_at = 5 * interval
    assert ps[level_at - 1] == ps[level_at + interval - 1] == 1.0         # r == target: nothing moved, at either clamp
    assert ps[16 * interval - 1] == ps[17 * interval - 1] == 0.0
    assert ref.state()[3] == interval // 2                                # the script ends mid-interval (interval 3)


def test_update_without_a_metrics_pointer():
    stats = torch.tensor([4.0, 4.0, 0.0, 0.0], device="cuda")
    state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], device="cuda")
    ops.ada.update(stats, state, None, 0.5, 1, 1.0 / 16)
    assert state.tolist() == [0.75, 0, 0, 0, 1.0, 0, 0, 0]
