"""The case table of the DiffAugment kernels' route tests (csrc/diffaug.hip): tests/test_diffaug_cases_cpu.py holds it to its claims on
the CPU through ops.diffaug.plan -- what the two entry points launch -- and tests/test_diffaug_routes_gpu.py runs it on the GPU.

A case is a batch shape (n, H, W, C) with the launch it was chosen for, under the colour policies (``color``: mask 1) and under the
gather policies (``gather``: mask 6; without colour the resident kernel is never launched):
    resident, threads, grid_y     from the plan
    trips                         trips of sweep_read's loop for an aligned sample: ceil((E / 4) / (kBatch * threads)), kBatch = 3
    partial                       the last trip does not fill every lane's batch
    second_sample_trip            n > grid_x: a workgroup takes a second sample
``offsets``: the view offsets, in floats past a 16-byte boundary, the GPU tests run the case at.  ``exact``: the colour transform is
run on data where every intermediate is a float32 number exactly (exact_case)."""
import numpy as np

import diffaug_reference as DR

K_BATCH = 3               # diffaug.hip kBatch
COLOR, GATHER = 1, 6      # ops masks: colour alone decides the launch; translation | cutout stand for "no colour"
GATHER_POLICIES = ["translation", "cutout", "translation,cutout"]
COLOR_POLICIES = ["color", "color,translation,cutout"]


def cdiv(a, b):
    return -(-a // b)


def _c(shape, why, color=None, gather=None, offsets=(0,), exact=False, second_sample_trip=False, policies=("gather", "color")):
    return dict(shape=shape, why=why, color=color, gather=gather, offsets=offsets, exact=exact, second_sample_trip=second_sample_trip,
                policies=policies)


def _l(resident, threads, grid_y, trips=None, partial=None):
    return dict(resident=resident, threads=threads, grid_y=grid_y, trips=trips, partial=partial)


_G1 = _l(False, 256, 1)       # the gather launch of a small sample: no sweep 1, so no read trips to claim

CASES = [
    _c((3, 32, 32, 4), "resident, 256 threads, two read trips; E and C powers of two", color=_l(True, 256, 1, 2, True), gather=_l(False, 256, 2),
       exact=True),
    _c((3, 35, 37, 3), "resident, 256 threads, partial second read trip; E odd: every sample alignment", color=_l(True, 256, 1, 2, True), gather=_G1),
    _c((2, 71, 71, 3), "resident, 1024 threads, partial second read trip; E odd", color=_l(True, 1024, 1, 2, True), gather=_l(False, 256, 7)),
    _c((1, 349, 11, 4), "E = resident_floats: the LDS image and its pad at the cap", color=_l(True, 1024, 1, 2, True), gather=_l(False, 256, 7),
       offsets=(0, 1, 2, 3)),
    _c((1030, 3, 3, 3), "n > kMaxBlocks: the sample loop's second trip", color=_l(True, 256, 1, 1, True), gather=_G1, second_sample_trip=True),
    # (at E = 27 one wave does all of a sample's work; here all four fill and read the LDS image, so the barriers between samples count)
    _c((1030, 16, 16, 4), "n > kMaxBlocks with every wave at work: the LDS image reused between samples", color=_l(True, 256, 1, 1, True), gather=_G1,
       second_sample_trip=True),
    _c((2, 64, 64, 4), "colour, two sweeps, grid_y 2, 1024 threads; E and C powers of two", color=_l(False, 1024, 2, 2, True),
       gather=_l(False, 256, 8), exact=True),
    _c((2, 91, 91, 3), "colour, two sweeps, grid_y 3, E odd", color=_l(False, 1024, 3, 3, True), gather=_l(False, 256, 12), offsets=(0, 1)),
    _c((1, 210, 210, 3), "no colour, grid_y at its cap of 64", gather=_l(False, 256, 64), policies=("gather",)),
    _c((2, 6, 5, 5), "C = 5: a float4 inside one pixel or across one boundary", color=_l(True, 256, 1, 1, True), gather=_G1),
    _c((2, 4, 4, 8), "C = 8: a float4 never crosses a pixel", color=_l(True, 256, 1, 1, True), gather=_G1),
    _c((2, 1, 9, 3), "H = 1: no vertical shift, the cutout covers the axis", color=_l(True, 256, 1, 1, True), gather=_G1),
    _c((2, 9, 1, 3), "W = 1", color=_l(True, 256, 1, 1, True), gather=_G1),
]


def case_id(c):
    return "x".join(map(str, c["shape"]))


IDS = [case_id(c) for c in CASES]
WITH_COLOR = [c for c in CASES if "color" in c["policies"]]
EXACT = [c for c in CASES if c["exact"]]
CUT_COLOR = [c for c in WITH_COLOR if c["color"]["grid_y"] > 1]           # colour with a sample's output cut across workgroups
REPEAT = CUT_COLOR + [c for c in CASES if c["second_sample_trip"]]


def describe(shape, plan, color):
    """The claims of one launch from ``plan`` = ops.diffaug.plan(*shape, mask)."""
    E = int(np.prod(shape[1:]))
    d = dict(resident=plan["resident"], threads=plan["threads"], grid_y=plan["grid_y"], trips=None, partial=None)
    if color:             # sweep 1 exists only with colour
        per = K_BATCH * plan["threads"]
        d["trips"], d["partial"] = cdiv(E // 4, per), (E // 4) % per != 0
    return d


# ------------------------------------------------------------------ data
def params_for(c, seed, special_at=()):
    """DR.injected_params (every batch), the four special rows repeated from each index of ``special_at`` on."""
    n = c["shape"][0]
    batches = DR.injected_params(n, seed)
    for at in special_at:
        batches[0, at:at + DR.SPECIAL_ROWS] = batches[0, :DR.SPECIAL_ROWS]
    return batches


def per_sample_case(shape, policy, seed, params):
    """DR.kernel_case with its rule taken PER SAMPLE: bound[k][i] = max(4 x the float32-numpy error of sample i relative to sample
    i's own norm, FLOOR).  Returns dict(x, g, params, cfg, ref, bound)."""
    cfg = DR.as_cfg(policy)
    rng = np.random.default_rng(seed)
    x = rng.normal(size=shape).astype(DR.F32)
    g = rng.normal(size=shape).astype(DR.F32)
    out = {dt: dict(fwd=DR.np_T(x, params, cfg, dtype=dt), lin=DR.np_T(x, params, cfg, linear=True, dtype=dt), adj=DR.np_LT(g, params, cfg, dtype=dt))
           for dt in (np.float64, np.float32)}
    ref, f32 = out[np.float64], out[np.float32]
    bound = {k: np.maximum(4 * sample_errors(f32[k], ref[k]), DR.FLOOR) for k in ref}
    return dict(x=x, g=g, params=params, cfg=cfg, ref=ref, bound=bound)


def sample_errors(a, b):
    """[n]: ||a_i - b_i|| / ||b_i|| per sample, in float64 (a sample whose reference is all zero must be matched exactly)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = a.shape[0]
    num = np.linalg.norm((a - b).reshape(n, -1), axis=1)
    return num / np.maximum(np.linalg.norm(b.reshape(n, -1), axis=1), 1e-300)


def exact_case(shape, policy, seed):
    """x and g integers in {-4 ... 4}, the three colour uniforms multiples of 1/4 (b, s, c multiples of 1/4 too), the rest of the row
    from DR.injected_params.  With E and C powers of two every mean, product and sum of both directions is a float32 number exactly
    (tests/test_diffaug_cases_cpu.py asserts that the float32 and float64 numpy evaluations agree bit for bit), so the GPU result must be
    array_equal to the float64 reference, whatever the order of its sums."""
    cfg = DR.as_cfg(policy)
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=shape).astype(DR.F32)
    g = rng.integers(-4, 5, size=shape).astype(DR.F32)
    params = DR.injected_params(shape[0], seed, batches=1)[0]
    params[:, :3] = rng.integers(0, 4, size=(shape[0], 3)).astype(DR.F32) / DR.F32(4)
    params[0, 1] = 0.0            # s = 0 and c = 0.5 stay among the draws
    params[-1, 2] = 0.0
    out = {dt: dict(fwd=DR.np_T(x, params, cfg, dtype=dt), lin=DR.np_T(x, params, cfg, linear=True, dtype=dt), adj=DR.np_LT(g, params, cfg, dtype=dt))
           for dt in (np.float64, np.float32)}
    return dict(x=x, g=g, params=params, cfg=cfg, ref=out[np.float64], f32=out[np.float32])
