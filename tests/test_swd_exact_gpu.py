"""GPU: every route, loop trip and misaligned view of the SWD kernels of csrc/swd.hip on exact data (tests/swd_cases.py;
tests/test_swd_cases_cpu.py proves on the CPU that every case is on its claimed cell and every recipe exact).

Every comparison is array_equal, or equality of launch-name lists.  Every tensor a kernel reads or writes is a view inside a larger
buffer (helpers.Guarded) whose bands hold a finite sentinel and must stay bit-unchanged; the view starts on a 16-byte boundary or one
float past it, as the case says.  Outputs start as NaN (the in-place sort and standardize start as their input), so an element a
grid-stride loop skipped shows; inputs must be bit-unchanged; the workspaces of standardize and abs_diff_mean are exactly as long as
their queries report.  The launch names the profiler records must be the restated ones: for the sort the whole ordered list of
sort_rows_chunk / sort_rows_global / sort_rows_tail of swd_cases.sort_plan.  A wrong ingest or gather output prints the element it holds.
"""
import numpy as np
import pytest
import torch

import swd_cases as SC
from helpers import Guarded

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
IDS = [SC.case_id(c) for c in SC.ALL]


def launches(fn):
    from blurred_gan_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.prof_records()]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


def call(fn, profile):
    if profile:
        return launches(fn)
    fn()
    torch.cuda.synchronize()
    return None


def settle(ins, outs, others=()):
    """After a call: guard bands bit-unchanged, inputs bit-unchanged."""
    for name, g in list(ins.items()) + list(outs.items()) + list(others):
        assert g.guards_intact(), f"a guard band of {name} was written"
    for name, g in ins.items():
        assert g.unchanged(), f"the input {name} was written"


def off(case, name):
    return case["off"].get("off_" + name, 0)


# ------------------------------------------------------------------ one runner per entry point: data -> {output name: numpy}, launch names
def run_ingest(case, data, profile=True):
    from blurred_gan_amd import ops
    B, H, W = case["B"], case["H"], case["W"]
    src = data["src"]
    gs, gd = Guarded(src.size, src, offset=off(case, "src")), Guarded(B * 3 * H * W, offset=off(case, "dst"))
    names = call(lambda: ops.swd_ingest(gs.t(*src.shape), gd.t(B, 3, H, W), case["nhwc"], SC.SCALE, SC.SHIFT), profile)
    settle({"src": gs}, {"dst": gd})
    return {"dst": gd.get(B, 3, H, W)}, names


def run_down(case, data, profile=True):
    from blurred_gan_amd import ops
    p, H, W = case["planes"], case["H"], case["W"]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    gx, gy = Guarded(p * H * W, data["x"], offset=off(case, "x")), Guarded(p * Ho * Wo, offset=off(case, "y"))
    names = call(lambda: ops.pyr_down(gx.t(1, p, H, W), gy.t(1, p, Ho, Wo)), profile)
    settle({"x": gx}, {"y": gy})
    return {"y": gy.get(1, p, Ho, Wo)}, names


def run_up(case, data, profile=True, way="fused"):
    from blurred_gan_amd import ops
    p, h, w = case["planes"], case["h"], case["w"]
    n = 4 * p * h * w
    gl = Guarded(p * h * w, data["low"])
    ins = {"low": gl}
    if way == "plain":
        go = Guarded(n, offset=off(case, "out"))
        fn = lambda: ops.pyr_up(gl.t(1, p, h, w), go.t(1, p, 2 * h, 2 * w))
    elif way == "fused":
        go, gm = Guarded(n, offset=off(case, "out")), Guarded(n, data["minuend"], offset=off(case, "min"))
        ins["minuend"] = gm
        fn = lambda: ops.pyr_up(gl.t(1, p, h, w), go.t(1, p, 2 * h, 2 * w), minuend=gm.t(1, p, 2 * h, 2 * w))
    else:
        go = Guarded(n, data["minuend"], offset=off(case, "out"))
        fn = lambda: ops.pyr_up(gl.t(1, p, h, w), go.t(1, p, 2 * h, 2 * w), minuend=go.t(1, p, 2 * h, 2 * w))
    names = call(fn, profile)
    settle(ins, {"out": go})
    return {"out": go.get(1, p, 2 * h, 2 * w)}, names


def run_gather(case, data, profile=True):
    from blurred_gan_amd import ops
    B, H, W, n, pi = case["B"], case["H"], case["W"], case["nhood"], case["per_image"]
    total = B * pi
    gl = Guarded(B * 3 * H * W, data["level"])
    gcx, gcy = Guarded(total, data["cx"], dtype=torch.int32), Guarded(total, data["cy"], dtype=torch.int32)
    gd = Guarded(total * 3 * n * n, offset=off(case, "desc"))
    names = call(lambda: ops.swd_gather(gl.t(B, 3, H, W), gcx.view, gcy.view, gd.t(total, 3, n, n), n, pi), profile)
    settle({"level": gl, "cx": gcx, "cy": gcy}, {"desc": gd})
    return {"desc": gd.get(total, 3, n, n)}, names


def run_std(case, data, profile=True):
    from blurred_gan_amd import ops
    rows, n = case["rows"], case["nhood"]
    nbytes = ops.swd_standardize_workspace_bytes(rows, n)
    assert nbytes == SC.standardize_workspace_bytes(rows, n) and nbytes % 8 == 0
    gd = Guarded(rows * 3 * n * n, data["x"], offset=off(case, "desc"))
    gw, gs = Guarded(nbytes // 8, dtype=torch.float64), Guarded(6, dtype=torch.float64)
    names = call(lambda: ops.swd_standardize(gd.t(rows, 3, n, n), rows, n, gw.view, gs.view), profile)
    settle({}, {"desc": gd, "stats": gs}, [("the workspace", gw)])
    return {"desc": gd.get(rows, 3, n, n), "stats": gs.get()}, names


def run_sort(case, data, profile=True):
    from blurred_gan_amd import ops
    rows, n = case["rows"], case["n"]
    gx = Guarded(rows * n, data["x"], offset=off(case, "x"))
    names = call(lambda: ops.sort_rows(gx.t(rows, n), rows, n), profile)
    settle({}, {"x": gx})
    return {"x": gx.get(rows, n)}, names


def run_absdiff(case, data, profile=True):
    from blurred_gan_amd import ops
    seg, nseg = case["seg"], case["nseg"]
    nbytes = ops.abs_diff_mean_workspace_bytes(seg, nseg)
    assert nbytes == SC.abs_diff_workspace_bytes(seg, nseg)
    ga, gb = Guarded(seg * nseg, data["a"], offset=off(case, "a")), Guarded(seg * nseg, data["b"], offset=off(case, "b"))
    go, gw = Guarded(nseg, dtype=torch.float64), Guarded(nbytes // 8, dtype=torch.float64)
    names = call(lambda: ops.abs_diff_mean(ga.view, gb.view, seg, nseg, go.view, gw.view), profile)
    settle({"a": ga, "b": gb}, {"out": go}, [("the workspace", gw)])
    return {"out": go.get()}, names


RUN = {"ingest": run_ingest, "down": run_down, "up": run_up, "gather": run_gather, "std": run_std, "sort": run_sort, "absdiff": run_absdiff}


# ------------------------------------------------------------------ data and references per entry: (inputs, {output name: wanted})
def make(case, salt=0, recipe="int", kind="perm", way="fused"):
    from blurred_gan_amd import sliced_wasserstein as sw
    e = case["entry"]
    if e == "ingest":
        src, _, want = SC.ingest_data(case)
        return {"src": src}, {"dst": want}
    if e == "down":
        x = SC.down_data(case, recipe, salt)
        return {"x": x}, {"y": sw.pyr_down(x)}                     # float64 in, float64 out; float32 in, the host's float32
    if e == "up":
        low, x = SC.up_data(case, recipe, salt)
        up = sw.pyr_up(low)
        return {"low": low, "minuend": x}, {"out": up if way == "plain" else x - up}
    if e == "gather":
        level = SC.gather_level(case)
        cx, cy = SC.gather_centres(case, salt)
        return {"level": level, "cx": cx, "cy": cy}, {"desc": SC.gather_ref(level, cx, cy, case["nhood"], case["per_image"])}
    if e == "std":
        x, d = SC.std_data(case, salt)
        return {"x": x}, {"desc": d, "stats": SC.std_stats()}
    if e == "sort":
        x = SC.sort_data(case, kind, salt)
        return {"x": x}, {"x": np.sort(x, axis=1)}
    a, b, want = SC.absdiff_data(case, salt)
    return {"a": a, "b": b}, {"out": want}


def same(got, want):
    """Bit for bit against a float32 host result, by value against a float64 reference."""
    if want.dtype == F32:
        return got.dtype == F32 and np.array_equal(got, want)
    return np.array_equal(got.astype(F64), want)


def explain(case, name, got, want):
    if case["entry"] == "ingest":
        detail = SC.decode_ingest(case, got, want)
    elif case["entry"] == "gather":
        detail = SC.decode_level(case, got, want)
    else:
        bad = np.argwhere(got.astype(F64) != want.astype(F64))
        at = tuple(bad[0])
        detail = f"{len(bad)} of {want.size} wrong, first at {[int(v) for v in at]}: got {got[at]}, want {want[at]}"
    return f"{SC.case_id(case)} [{name}]: {int(np.isnan(got).sum())} outputs never written (or NaN); {detail}"


def check(case, outs, want, names, label=""):
    d = SC.describe(case)
    assert names == d["names"], (label, names, d["names"])
    for name, w in want.items():
        if not same(outs[name], w):
            pytest.fail(label + " " + explain(case, name, outs[name], w))


@pytest.mark.parametrize("case", SC.ALL, ids=IDS)
def test_exact_on_its_cell(case):
    e = case["entry"]
    if e == "down":
        for recipe in SC.pyr_recipes(case):
            ins, want = make(case, recipe=recipe)
            outs, names = run_down(case, ins)
            check(case, outs, want, names, recipe)
    elif e == "up":
        for recipe in SC.pyr_recipes(case):
            ins, want = make(case, recipe=recipe, way="plain")        # one reference for the three ways
            for way in ("plain", "fused", "inplace"):
                outs, names = run_up(case, ins, way=way)
                check(case, outs, want if way == "plain" else {"out": ins["minuend"] - want["out"]}, names, f"{recipe} {way}")
    elif e == "sort":
        for kind in SC.sort_kinds(case):
            ins, want = make(case, kind=kind)
            outs, names = run_sort(case, ins)
            check(case, outs, want, names, kind)
    else:
        ins, want = make(case)
        outs, names = RUN[e](case, ins)
        check(case, outs, want, names)


# ------------------------------------------------------------------ one case per entry point: isolation, determinism
PER_ENTRY = [SC.TABLES[e][i] for e, i in SC.PER_ENTRY]
PER_IDS = [SC.case_id(c) for c in PER_ENTRY]
# the input that gets a NaN unit, and how input and outputs are cut into units: image, plane, plane, image, channel, row, segment
UNIT_IN = {"ingest": ("src", lambda c, a: a), "down": ("x", lambda c, a: a[0]), "up": ("low", lambda c, a: a[0]),
           "gather": ("level", lambda c, a: a), "std": ("x", lambda c, a: a.transpose(1, 0, 2, 3)), "sort": ("x", lambda c, a: a),
           "absdiff": ("a", lambda c, a: a.reshape(c["nseg"], c["seg"]))}
UNIT_OUT = {"ingest": lambda c, a: a, "down": lambda c, a: a[0], "up": lambda c, a: a[0], "gather": lambda c, a: a.reshape(c["B"], -1),
            "std": lambda c, a: a.transpose(1, 0, 2, 3) if a.ndim == 4 else a.reshape(3, 2), "sort": lambda c, a: a, "absdiff": lambda c, a: a}


@pytest.mark.parametrize("case", PER_ENTRY, ids=PER_IDS)
def test_a_nan_unit_stays_inside_itself(case):
    """One image (ingest, gather), plane (pyramid), channel (standardize), row (sort) or segment (abs_diff) is NaN throughout: every
    other one equals its reference, and the NaN one comes out NaN everywhere -- for the sort, the NaN row is left as it is."""
    e = case["entry"]
    ins, want = make(case, salt=1)
    key, cut = UNIT_IN[e]
    ins = {k: np.array(v, copy=True) for k, v in ins.items()}
    units = cut(case, ins[key])
    k = len(units) // 2
    assert len(units) >= 2
    units[k] = np.nan                                              # a view: writes through to ins[key]
    assert np.isnan(ins[key]).sum() == units[k].size
    outs, _ = RUN[e](case, ins, profile=False)
    for name, w in want.items():
        g, w = UNIT_OUT[e](case, outs[name]), UNIT_OUT[e](case, np.asarray(w))
        assert len(g) == len(units)
        for u in range(len(units)):
            if u == k:
                assert np.isnan(g[u]).all(), f"{name}: {int((~np.isnan(g[u])).sum())} outputs of the NaN unit are numbers"
            else:
                assert same(np.ascontiguousarray(g[u]), np.ascontiguousarray(w[u])), f"{name}: unit {u} (the NaN unit is {k}) is wrong"


@pytest.mark.parametrize("case", PER_ENTRY, ids=PER_IDS)
def test_two_runs_are_bit_identical(case):
    recipe = "frac" if case["entry"] in ("down", "up") else "int"
    ins, want = make(case, salt=2, recipe=recipe, kind="special")
    o1, _ = RUN[case["entry"]](case, ins, profile=False)
    o2, _ = RUN[case["entry"]](case, ins, profile=False)
    bits = lambda a: a.view(np.uint32 if a.dtype == F32 else np.uint64)
    for name, w in want.items():
        assert np.array_equal(bits(o1[name]), bits(o2[name])), name
        assert same(o1[name], w), name


def test_the_per_entry_cases_have_more_than_one_block_and_unit():
    for c in PER_ENTRY:
        d = SC.describe(c)
        assert d.get("grid", d.get("cgrid", d.get("nb"))) > 1, SC.case_id(c)


def test_laplacian_pyramid_in_place_shares_the_inputs_storage():
    """Two levels on the integer recipe: level 0 is written over the input and both levels equal the float64 evaluation."""
    from blurred_gan_amd import sliced_wasserstein as sw, swd_native as sn
    x = SC.int_image((2, 3, 24, 32), np.random.default_rng(11))
    low = sw.pyr_down(x)
    want = [x - sw.pyr_up(low), low]
    assert all(w.dtype == F64 for w in want)
    gx = Guarded(x.size, x)
    t = gx.t(*x.shape)
    got = []
    names = launches(lambda: got.extend(sn.generate_laplacian_pyramid(t, 2, in_place=True)))
    assert names == ["pyr_down", "pyr_up"], names
    assert len(got) == 2 and got[0].data_ptr() == t.data_ptr() and got[0] is t and got[1].data_ptr() != t.data_ptr()
    assert gx.guards_intact()
    assert same(gx.get(*x.shape), want[0]) and same(got[1].cpu().numpy(), want[1])
    # not in place: the same levels, the input untouched
    gy = Guarded(x.size, x)
    other = sn.generate_laplacian_pyramid(gy.t(*x.shape), 2)
    torch.cuda.synchronize()
    assert gy.unchanged() and gy.guards_intact() and other[0].data_ptr() != gy.view.data_ptr()
    assert same(other[0].cpu().numpy(), want[0]) and same(other[1].cpu().numpy(), want[1])
