"""CPU: bg_diffaug_plan, and the case table of tests/diffaug_cases.py held to its claims through it -- the launch each case was chosen
for is the launch the library reports -- and the precondition of the exact colour test: on its data float32 numpy equals float64
numpy bit for bit."""
import numpy as np
import pytest

from blurred_gan_amd import ops
import diffaug_cases as DC
import diffaug_reference as DR


def test_plan_restates_the_launch_rules():
    """The plan against the rules of csrc/diffaug.hip, written out once more: a seeded sweep over sizes around every threshold."""
    rf = ops.diffaug.route(1, 1, 1)["resident_floats"]
    rng = np.random.default_rng(7)
    sizes = [1, 2047, 2048, 2049, 8191, 8192, 8193, rf - 1, rf, rf + 1, 16383, 16384, 3 * 8192 - 1, 3 * 8192, 131071, 131072, 1 << 20]
    seen = set()
    for E in sizes + [int(v) for v in rng.integers(1, 1 << 19, size=40)]:
        for n in (1, 2, 7, 8, 9, 300, 1024, 1025, 5000):
            for mask in range(8):
                p = ops.diffaug.plan(n, 1, E, 1, mask)
                color = bool(mask & 1)
                assert p["grid_x"] == min(n, 1024)
                assert p["threads"] == (1024 if color and E >= 8192 else 256)
                assert p["resident"] == (color and E <= rf)
                if p["resident"]:
                    assert p["grid_y"] == 1 and p["lds_bytes"] == 64 + (E + 6) // 4 * 16
                    assert p["lds_bytes"] >= 64 + 4 * (E + 3) and p["lds_bytes"] <= 64 * 1024      # the image behind the largest pad fits
                else:
                    want = max(1, min(E // (8192 if color else 2048), 64))
                    assert p["grid_y"] == min(want, max(1, (512 if color else 2048) // p["grid_x"])) and p["lds_bytes"] == 64
                seen.add((p["resident"], p["threads"], min(p["grid_y"], 2), n > p["grid_x"]))
    # (resident, threads, cut, second sample trip): every launch kind there is was reached -- a colour launch of more than 1024
    # samples is never cut (512 / 1024 workgroups), a gather launch of that many still is (2048 / 1024)
    yes, no = True, False
    assert seen == {(yes, 256, 1, no), (yes, 256, 1, yes), (yes, 1024, 1, no), (yes, 1024, 1, yes),
                    (no, 256, 1, no), (no, 256, 2, no), (no, 256, 1, yes), (no, 256, 2, yes),
                    (no, 1024, 1, no), (no, 1024, 2, no), (no, 1024, 1, yes)}
    # the same answer whatever the factorisation of E, and route() keeps answering by E alone
    assert ops.diffaug.plan(2, 64, 64, 3, 7) == ops.diffaug.plan(2, 1, 64 * 64 * 3, 1, 1) == ops.diffaug.plan(2, 3, 64, 64, 5)
    assert ops.diffaug.route(8, 8, 3)["resident"] and not ops.diffaug.plan(4, 8, 8, 3, 6)["resident"]
    for bad in ((0, 4, 4, 3, 7), (1, 0, 4, 3, 7), (1, 4, 4, 3, 8), (1, 4, 4, 3, -1), (1, 1 << 11, 1 << 11, 1 << 10, 7)):
        with pytest.raises(ValueError):
            ops.diffaug.plan(*bad)


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_case_launches_what_it_claims(case):
    shape = case["shape"]
    n = shape[0]
    assert set(case["policies"]) <= {"gather", "color"} and "gather" in case["policies"]
    for kind, mask in (("gather", DC.GATHER), ("color", DC.COLOR)):
        if kind not in case["policies"]:
            assert case[kind] is None
            continue
        for m in ((mask, mask | DC.GATHER) if kind == "color" else (2, 4, 6)):          # every policy of the kind launches the same
            plan = ops.diffaug.plan(*shape, m)
            assert DC.describe(shape, plan, kind == "color") == case[kind], (DC.case_id(case), kind, m, plan)
            assert (n > plan["grid_x"]) == case["second_sample_trip"]


def test_the_table_covers_what_it_was_written_for():
    rf = ops.diffaug.route(1, 1, 1)["resident_floats"]
    E = lambda c: int(np.prod(c["shape"][1:]))
    col = [c for c in DC.WITH_COLOR]
    # resident route: a second read trip at either workgroup size, the cap, a second sample per workgroup
    assert {c["color"]["threads"] for c in col if c["color"]["resident"] and c["color"]["trips"] >= 2} == {256, 1024}
    cap = [c for c in col if E(c) == rf]
    assert len(cap) == 1 and cap[0]["offsets"] == (0, 1, 2, 3) and cap[0]["color"]["resident"]
    assert not ops.diffaug.plan(1, 1, rf + 1, 1, DC.COLOR)["resident"] and ops.diffaug.plan(1, 1, rf + 1, 1, DC.COLOR)["grid_y"] == 1
    assert any(c["second_sample_trip"] and c["color"]["resident"] for c in col)
    assert any(E(c) % 2 == 1 and c["shape"][0] >= 3 and c["color"]["resident"] for c in col)         # samples at every alignment
    # two-sweep colour: the output cut 2 and 3 ways, one of them with odd E and a misaligned view
    assert sorted(c["color"]["grid_y"] for c in DC.CUT_COLOR) == [2, 3] and all(not c["color"]["resident"] for c in DC.CUT_COLOR)
    assert any(E(c) % 2 == 1 and 1 in c["offsets"] for c in DC.CUT_COLOR)
    assert max(c["gather"]["grid_y"] for c in DC.CASES) == 64
    assert {c["shape"][3] for c in DC.CASES} >= {3, 4, 5, 8} and any(c["shape"][1] == 1 for c in DC.CASES) and any(c["shape"][2] == 1 for c in DC.CASES)
    assert len(DC.REPEAT) == 4 and [DC.case_id(c) for c in DC.EXACT] == ["3x32x32x4", "2x64x64x4"]
    # what the issue found missing in tests/test_diffaug_gpu.py's shapes: no resident shape there takes a second read trip
    for s in ((1, 2, 2, 1), (3, 5, 7, 3), (2, 8, 8, 3), (5, 16, 12, 4), (2, 28, 28, 1), (70, 4, 4, 3), (3, 64, 64, 3)):
        assert DC.describe(s, ops.diffaug.plan(*s, DC.COLOR), True)["trips"] == 1 and s[0] <= 1024


def test_special_rows_reach_the_second_sample_trip():
    c = next(c for c in DC.CASES if c["second_sample_trip"])
    p = DC.params_for(c, 5, special_at=(1024,))
    assert p.shape == (1, 1030, 8) and np.array_equal(p[0, 1024:1028], p[0, :4])
    assert (p[0, 1024:1028, 3:7] == np.array([[0, 0, 0, 0], [0, DR.HI, 0, DR.HI], [DR.HI, 0, DR.HI, 0], [DR.HI] * 4], np.float32)).all()
    assert ops.diffaug.plan(*c["shape"], 7)["grid_x"] == 1024


@pytest.mark.parametrize("case", DC.EXACT + [dict(shape=(2, 4, 4, 2)), dict(shape=(3, 8, 2, 4))], ids=lambda c: DC.case_id(c))
@pytest.mark.parametrize("policy", DC.COLOR_POLICIES)
def test_exact_recipe_float32_equals_float64(case, policy):
    """The precondition of the exact colour test: every intermediate is a float32 number, so numpy in float32 and in float64 agree
    bit for bit, forward, linear and adjoint."""
    shape = case["shape"]
    E, C = int(np.prod(shape[1:])), shape[3]
    assert E & (E - 1) == 0 and C & (C - 1) == 0
    ex = DC.exact_case(shape, policy, seed=61)
    for a in (ex["x"], ex["g"]):
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and a.min() == -4 and a.max() == 4
    assert np.array_equal(ex["params"][:, :3] * 4, np.round(ex["params"][:, :3] * 4)) and ex["params"].min() >= 0 and ex["params"].max() < 1
    assert ex["params"][0, 1] == 0 and ex["params"][-1, 2] == 0
    for k in ("fwd", "lin", "adj"):
        assert ex["f32"][k].dtype == np.float32 and ex["ref"][k].dtype == np.float64
        assert np.array_equal(ex["f32"][k].astype(np.float64), ex["ref"][k]), k
        assert np.abs(ex["ref"][k]).max() > 0
    assert not np.array_equal(ex["ref"]["fwd"], ex["ref"]["lin"])                  # b != 0 somewhere
