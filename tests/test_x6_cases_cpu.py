"""CPU: tests/x6_cases.py held to its claims.  Per case and recipe: split3 returns the intended pieces and they sum back to the
element exactly; the kept terms accumulated in float32, in the kernel's issue order and reversed, equal the float64 oracle bit for
bit; the "pieces" expectation is RNE(float64 product); every mutant of the six-term sum (a kept term dropped or doubled, the planes
of an asymmetric term swapped, mid.mid replaced by mid.lo / lo.mid) stays at least 8 ulps away on an output of every (tap, K chunk,
k-slice) the case claims; the float64 emulation WITH lifted zeros passes the comparison the GPU tests use.  The table equals its
declared cell set, and x6_can_run with the dispatch table agrees with the library's bg_conv2d_math_taken."""
import os

import numpy as np
import pytest

import conv_cases as CC
import x6_cases as X

ALL = X.ROUTE_CASES + [c + (set(),) for c in X.TABLE_CASES]
IDS = [X.case_id(c) for c in ALL]


def test_case_ids_are_unique_and_small():
    assert len(set(IDS)) == len(IDS)
    for c in ALL + X.MUST_NOT_RUN + X.EPI_CASES + X.STATS_CASES + X.PRECISION_CASES + X.SCALING_CASES:
        assert int(np.prod(X.out_shape(c[0], c[1]))) <= 200_000
    routes = {c[:3] for c in X.ROUTE_CASES}
    assert set(X.EPI_CASES) <= routes and set(X.STATS_CASES) <= routes
    assert {f"{'dgrad' if b else 'fwd'}:bn{X.launch(b, s, k)['BN']}" for b, s, k in X.EPI_CASES} == {c for c in X.X6_CELLS if ":" in c}
    assert {X.launch(b, s, k)["K"] for b, s, k in X.PRECISION_CASES} >= {32, 288, 800}
    assert {b for b, _, _ in X.PRECISION_CASES} == {b for b, _, _ in X.SCALING_CASES} == {0, 1}
    assert any(X.launch(b, s, k)["empty_tiles"] for b, s, k in X.STATS_CASES)


def test_the_table_hits_every_cell():
    for bwd, shape, k, claimed in X.ROUTE_CASES:
        assert X.x6_can_run(bwd, *shape[:5], k, shape[5]), (bwd, shape, k)
        assert claimed <= X.cells(bwd, shape, k), (X.case_id((bwd, shape, k)), claimed - X.cells(bwd, shape, k))
    assert set().union(*[c[3] for c in X.ROUTE_CASES]) == X.X6_CELLS, set().union(*[c[3] for c in X.ROUTE_CASES]) ^ X.X6_CELLS
    for bwd, shape, k in X.MUST_NOT_RUN:                   # 16 positions: one short of the rule, everything else in order
        p = CC.gather_params(bwd, *shape[:5], k, shape[5])
        assert max(g["Ha"] * g["Wa"] for g in p["ph"]) == 16 and p["Ck"] % 32 == 0 and p["N"] % 32 == 0
        assert not X.x6_can_run(bwd, *shape[:5], k, shape[5])
        for recipe in X.RECIPES:
            act, w = X.make(bwd, shape, k, recipe, cover=False)
            assert X.expected(bwd, shape, act, w).any() and np.array_equal(act, act.astype(np.float32))
    for bwd, shape, k in X.TABLE_CASES:
        assert X.in_table(bwd, *shape[1:5], k, shape[5]) and X.x6_can_run(bwd, *shape[:5], k, shape[5]) and shape[0] == 1


def test_split3_restates_the_kernel_on_hard_values():
    x = np.array([0.0, -0.0, 1.0, -1.0, 3.0, 257.0, -65537.0, 1 + 2.0 ** -23, np.pi, -np.e * 1e-30, 3.4e38, 2.0 ** -126, 2.0 ** -140,
                  np.inf, -np.inf, np.nan], np.float32)
    hi, mid, lo = X.split3(x, lift=False)
    fin = np.isfinite(x)
    big = fin & ((np.abs(x) >= 2.0 ** -100) | (x == 0))         # exact while the low piece is a normal bfloat16 (bf16 ends at 2^-133)
    assert np.array_equal(hi[big].astype(np.float64) + mid[big] + lo[big], x[big].astype(np.float64)) and big.sum() == 11
    assert (np.abs(hi[fin].astype(np.float64) + mid[fin] + lo[fin] - x[fin]) <= 2.0 ** -134).all()
    for p in (hi, mid, lo):                                     # every piece is a bfloat16 number
        assert not (p.view(np.uint32) & 0xffff).any()
    assert np.array_equal(hi[~fin].view(np.uint32), np.array([0x7f800000, 0xff800000, 0x7fc00000], np.uint32))
    assert not mid[~fin].any() and not lo[~fin].any()           # Inf / NaN: mid = lo = 0, not a NaN made by inf - inf
    assert (np.abs(hi[fin]) <= np.abs(x[fin])).all()            # a bit mask, not a rounding
    assert mid[5] == 1.0 and hi[5] == 256.0 and hi[6] == -65536.0 and mid[6] == -1.0
    _, midl, lol = X.split3(x)
    for raw, lifted in ((mid, midl), (lo, lol)):
        small = np.abs(raw) < 2.0 ** -126
        assert np.array_equal(np.abs(lifted[small]), np.full(int(small.sum()), X.LIFT, np.float32))
        assert np.array_equal(lifted[~small], raw[~small])
        assert np.array_equal(np.signbit(lifted), np.signbit(hi))                                          # the element's sign
    assert np.signbit(midl[1]) and not np.signbit(midl[0]) and small.sum() >= 8


def test_a_lifted_zero_stays_under_the_bound():
    """A zero element times any finite operand: the six kept terms hold at most 5 x 2^-126 x |operand| (K = 1)."""
    rng = np.random.default_rng(3)
    w = (rng.uniform(-1, 1, 4000) * 10.0 ** rng.uniform(-30, 30, 4000)).astype(np.float32)
    w[:8] = [0, 1, -1, 65536 + 64 + 1 / 16, 3.0e38, -3.0e38, 2.0 ** -126, 255]
    for zero in (0.0, -0.0):
        a = [p.astype(np.float64) for p in X.split3(np.full(w.shape, zero, np.float32))]
        b = [p.astype(np.float64) for p in X.split3(w)]
        assert a[0].max() == 0 and np.abs(a[1]).max() == X.LIFT == np.abs(a[2]).max()
        for order in (X.KEPT_TERMS, X.KEPT_TERMS[::-1]):
            got = np.zeros(w.shape, np.float32)
            for i, j in order:
                got = got + (a[i] * b[j]).astype(np.float32)
            assert (np.abs(got) <= 5 * X.LIFT * np.maximum(np.abs(w), 1.0)).all()
    assert np.float32(X.LIFT) * np.float32(X.LIFT) == 0                                                     # lifted x lifted underflows


@pytest.mark.parametrize("case", ALL, ids=IDS)
@pytest.mark.parametrize("recipe", X.RECIPES)
def test_recipes_are_exact_in_float32_in_either_order(case, recipe):
    bwd, shape, k = case[:3]
    act, w = X.make(bwd, shape, k, recipe)
    assert act.shape == X.act_shape(bwd, shape) and w.shape == (k, k, shape[3], shape[4])
    assert np.array_equal(act, act.astype(np.float32)) and np.array_equal(w, w.astype(np.float32))
    full = X.conv(bwd, shape, act, w)
    ref = X.expected(bwd, shape, act, w)
    assert ref.shape == X.out_shape(bwd, shape) and ref.any()
    for arr in (act, w):                                        # the pieces sum back to the element exactly
        hi, mid, lo = X.split3(arr, lift=False)
        assert np.array_equal(hi.astype(np.float64) + mid + lo, arr)
        if recipe == "pieces":                                  # ... and are the intended ones
            nz = arr != 0
            assert set(np.abs(hi[nz])) == {65536.0} and set(np.abs(mid[nz])) == {64.0, 128.0, 192.0} and set(np.abs(lo[nz])) == {1 / 16, 2 / 16, 3 / 16}
            assert np.array_equal(np.sign(mid[nz]), np.sign(arr[nz])) and np.array_equal(np.sign(lo[nz]), np.sign(arr[nz]))
    if recipe == "pieces":
        assert w.all() and ((act != 0).sum(-1) <= 1).all()
        assert np.abs(full - ref).max() <= 72 + 9 / 256 < 256                    # the omitted terms, below half an ulp of 2^32
    else:
        assert np.array_equal(full, ref) and np.abs(ref).max() < CC.TWO24        # integers: the oracle itself is a float32 number
    P64 = X.piece_convs(bwd, shape, act, w)
    P32 = X.piece_convs(bwd, shape, act, w, dtype=np.float32)
    assert np.array_equal(X.combine(P64, X.kept_coef()), ref)                    # the kept sum IS RNE(float64 product)
    for order in (X.KEPT_TERMS, X.KEPT_TERMS[::-1]):
        acc = np.zeros(ref.shape, np.float32)
        for i, j in order:
            assert P32[i][j].dtype == np.float32
            acc = acc + P32[i][j]
        assert np.array_equal(acc.astype(np.float64), ref)
    # what the kernel stores, lifted zeros included (float64 emulation), passes the GPU tests' comparison; a shifted copy does not
    K = X.launch(bwd, shape, k)["K"]
    lifted = X.combine(X.piece_convs(bwd, shape, act, w, lift=True), X.kept_coef()).astype(np.float32).astype(np.float64)
    amax, wmax = np.abs(act).max(), np.abs(w).max()
    assert X.compare(lifted, ref, K, amax, wmax) is None
    if (ref == 0).any() and "phase_without_taps" not in X.cells(bwd, shape, k):      # (such a phase stores exact zeros)
        assert 0 < np.abs(lifted[ref == 0]).max() <= X.lifted_zero_bound(K, amax, wmax) < 1e-28
    res = X.compare(np.roll(lifted, 1, axis=-1), ref, K, amax, wmax)
    assert res is not None and "first at" in X.describe_wrong(bwd, shape, k, recipe, act, w, np.roll(lifted, 1, axis=-1), ref, res)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_mutant_moves_every_claimed_slice_by_8_ulps(case):
    bwd, shape, k = case[:3]
    act, w = X.make(bwd, shape, k, "pieces")
    ref = X.expected(bwd, shape, act, w)
    tags = X.slice_tags(bwd, shape, k, act)
    assert set(np.unique(tags)) - {0.0} == X.claimed_tags(bwd, shape, k), "an output window holds two impulses, or a (tap, k-slice) has none"
    assert np.array_equal(tags != 0, (ref != 0).any(-1)) and np.array_equal(tags != 0, (ref != 0).all(-1))
    P = X.piece_convs(bwd, shape, act, w)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    muts = X.mutants()
    assert len(muts) == 6 + 6 + 4 + 2
    for name, coef in muts.items():
        away = (np.abs(X.combine(P, coef) - ref) >= 8 * ulp) & (ref != 0)
        hit = np.bincount(tags.astype(np.int64).ravel(), weights=away.any(-1).ravel())                    # outputs 8 ulps away per (tap, k-slice)
        assert all(hit[int(t)] > 0 for t in X.claimed_tags(bwd, shape, k)), f"{name}: a (tap, k-slice) on which no output moves by 8 ulps"
        got = X.combine(P, coef).astype(np.float32).astype(np.float64)
        res = X.compare(got, ref, X.launch(bwd, shape, k)["K"], np.abs(act).max(), np.abs(w).max())
        assert res is not None
        if name.startswith(("drop", "double")):                # a term lost or doubled shows in EVERY product
            assert away[tags != 0].all() and res["n"] == int((ref != 0).sum())
        assert "WRONG" in X.describe_wrong(bwd, shape, k, "pieces", act, w, got, ref, res)


def test_a_wrong_piece_output_names_its_terms():
    bwd, shape, k = X.ROUTE_CASES[0][:3]
    act, w = X.make(bwd, shape, k, "pieces")
    ref = X.expected(bwd, shape, act, w)
    coef = X.mutants()["drop mid.mid"]
    got = X.combine(X.piece_convs(bwd, shape, act, w), coef)
    res = X.compare(got, ref, 800, 1.0, 1.0)
    msg = X.describe_wrong(bwd, shape, k, "pieces", act, w, got, ref, res)
    i = tuple(int(v) for v in np.argwhere(res["mask"])[0])
    kh, kw, c = X.locate(bwd, shape, k, act, i[:3])
    assert f"(kh, kw, ci, co)=({kh}, {kw}, {c}, {i[3]})" in msg and msg.count("WRONG") == 1 and "m_a m_b" in msg.split("WRONG")[0].split(",")[-1], msg
    assert abs(act[i[0]].sum()) > 0 and w[kh, kw, c, i[3]] * act[i[0]][act[i[0]] != 0][0] != 0


def test_x6_can_run_and_the_table_agree_with_the_library():
    from blurred_gan_amd import _lib
    from test_conv_cases_cpu import _sweep
    assert "BG_CONV_X6_FORCE" not in os.environ
    lib = _lib.load()
    geo = [(b, s, k) for b, s, k, _ in X.ROUTE_CASES] + X.MUST_NOT_RUN + X.TABLE_CASES
    geo += [(bwd, (B, H, W, Ci, Co, s), 5) for (bwd, H, W, Ci, Co, s) in CC.X6_TABLE for B in (1, 8, 256)]
    geo += [(1 - bwd, (8, H, W, Ci, Co, s), 5) for (bwd, H, W, Ci, Co, s) in CC.X6_TABLE]                  # the other direction
    geo += [(0, (256, 32, 32, 64, 128, 1), 5), (0, (256, 64, 64, 64, 32, 2), 5), (0, (8, 8, 8, 64, 128, 2), 5), (0, (8, 32, 32, 64, 128, 2), 3)]
    rng = np.random.default_rng(20261019)
    geo += [(int(rng.integers(0, 2)), c, int(rng.choice([1, 3, 5]))) for c in _sweep(1500, 11)]
    taken = 0
    for bwd, (B, H, W, Ci, Co, s), k in geo:
        want = X.x6_can_run(bwd, B, H, W, Ci, Co, k, s) and X.in_table(bwd, H, W, Ci, Co, k, s)
        assert bool(lib.bg_conv2d_math_taken(bwd, B, H, W, Ci, Co, k, s, 1)) == want, (bwd, B, H, W, Ci, Co, k, s)
        if k == 5:
            assert want == CC.math_taken(bwd, B, H, W, Ci, Co, k, s)
        taken += want
    assert taken >= 8
    assert sum(X.x6_can_run(b, *c[:5], k, c[5]) for b, c, k in geo) > 100                                   # the sweep reaches runnable geometries
