"""CPU: the SWD case tables of tests/swd_cases.py held to their claims -- every case on the cell it is listed under, the cells hit
equal to a written-out set, every second-trip case at two trips (and the edge cases at one with one row, plane or image fewer),
every recipe exact for the reason it gives -- and the restated stats_blocks / abs_diff_blocks held to the library's two host-only
workspace queries.  The V = 4 / V = 1 rules of the entry points and the sort plan have no such hook: the rules are restated by
reading csrc/swd.hip only, and the plan is pinned by the launch-name lists tests/test_swd_exact_gpu.py records (here it is only
shown to be a sorting network, by running it in numpy)."""
import numpy as np
import pytest

import swd_cases as SC

IDS = [SC.case_id(c) for c in SC.ALL]
F32, F64 = np.float32, np.float64


def bits_equal(a32, b64):
    return a32.dtype == F32 and b64.dtype == F64 and np.array_equal(a32.astype(F64), b64)


@pytest.fixture(scope="module")
def lib():
    from blurred_gan_amd import _lib
    return _lib.load()


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", SC.ALL, ids=IDS)
def test_case_is_on_its_claimed_cell(case):
    d = SC.describe(case)
    assert d["cell"] == case["cell"], f"claimed {case['cell']!r}, restated {d['cell']!r}"
    assert set(case["off"].values()) <= {0, 1}
    if case["entry"] != "sort":
        assert d["names"] == SC.NAMES[case["entry"]]
    else:
        assert d["names"][:1] == ["sort_rows_chunk"] and d["names"].count("sort_rows_global") == d["n_global"]
        assert d["names"].count("sort_rows_tail") == max(0, d["N"].bit_length() - 13)        # one per merge width above the chunk


def test_the_tables_hit_every_cell_and_no_other():
    assert SC.missing_and_extra() == ([], [])
    assert len(SC.CELLS) == 91
    # the check can fail: without the misaligned cases exactly their cells are reported
    fewer = [c for c in SC.ALL if not c["off"]]
    missing, extra = SC.missing_and_extra(fewer)
    assert extra == [] and missing == sorted(c for c in SC.CELLS if ":" in c) and len(missing) == 15
    assert [SC.TABLES[e][i]["entry"] for e, i in SC.PER_ENTRY] == list(SC.TABLES)


def test_second_trip_cases_take_two_trips_and_the_edge_cases_one_with_one_fewer():
    second = [c for c in SC.ALL if c["edge"] is not None]
    assert len(second) == 17
    for c in second:
        assert SC.loop_trips(c) == 2, (SC.case_id(c), SC.loop_trips(c))
        f = SC.one_fewer(c)
        df, dc = SC.describe(f), SC.describe(c)
        if c["edge"]:
            assert SC.loop_trips(f) == 1, (SC.case_id(c), "one fewer still takes", SC.loop_trips(f))
            assert df.get("V", df.get("vec")) == dc.get("V", dc.get("vec")), SC.case_id(c)       # the same kernel, one trip
        else:
            assert SC.loop_trips(f) == 2, SC.case_id(c)                                          # why it is not the edge case
    kernel = lambda c: (c["entry"], SC.describe(c).get("V", SC.describe(c).get("vec")), c.get("loop"))
    for c in second:                                              # a case that is not on the edge stands beside one of the same kernel that is
        assert c["edge"] or any(e["edge"] and kernel(e) == kernel(c) for e in second), f"no edge case beside {SC.case_id(c)}"
    assert len(SC.SECOND_TRIP_CELLS) == 15 and len({kernel(c) for c in second}) == 13
    # standardize: 3570 is the smallest even row count, no multiple of 4, whose apply kernel takes a second trip at nhood 7
    two = [r for r in range(2, 4000, 4) if SC.standardize_launch(r, 7)["trips"] == 2]
    assert two[0] == 3570 and SC.standardize_launch(3570, 7)["V"] == 1 and SC.standardize_launch(3570, 7)["total"] % 4 == 2
    # the sort's tail kernel shares the chunk grid, so (2049, 4100) gives it a second trip too, and its last chunk holds 4 floats
    p = SC.sort_plan(2049, 4100)
    assert (p["N"], p["n_chunks"], p["cgrid"], p["last_chunk"], p["names"]) == (8192, 4098, 4096, 4, ["sort_rows_chunk", "sort_rows_global", "sort_rows_tail"])
    # abs_diff and the statistics passes stride over a capped grid: many trips at the cap
    assert SC.abs_diff_launch(1048580, 2)["trips"] == 5 and SC.abs_diff_launch(1048579, 2)["trips"] == 17


def test_pyr_down_thread_kinds():
    """Interior threads (four 16-byte loads) exist from W = 24 on; at W = 8 and 16 every thread of a row is a border thread."""
    kinds = lambda W: ["I" if ox >= 2 and 2 * ox + 11 < W else "B" for ox in range(0, (W + 1) // 2, 4)]
    assert kinds(8) == ["B"] and kinds(16) == ["B", "B"] and kinds(24) == ["B", "I", "B"] and kinds(32) == ["B", "I", "I", "B"]
    assert kinds(64) == ["B"] + ["I"] * 6 + ["B"]
    for W in (7, 15, 23):
        d = SC.pyr_down_launch(2, 6, W)
        assert (d["V"], d["vec_in"], d["threads"]) == (4, 0, "S")
        # the 11 columns of the last thread of a row reach two past the right edge: refl's "at most two outside"
        assert 2 * (d["Wo"] - 4) - 2 + 10 == W + 1


def test_sort_plan_examples_and_the_plan_is_a_sorting_network():
    assert SC.sort_plan(3, 1)["names"] == []
    assert SC.sort_plan(3, 4096)["names"] == ["sort_rows_chunk"]
    p = SC.sort_plan(2, 8196)
    assert p["launches"] == [("sort_rows_chunk", None, None), ("sort_rows_global", 4096, 8191), ("sort_rows_tail", None, None),
                             ("sort_rows_global", 8192, 16383), ("sort_rows_global", 4096, 0), ("sort_rows_tail", None, None)]
    assert (p["wpr"], SC.sort_plan(2, 8196, aligned=False)["wpr"]) == (2048, 8192)
    assert SC.sort_plan(512, 1 << 20)["n_chunks"] == 131072 and SC.sort_plan(512, 1 << 20)["chunk_trips"] == 32      # the metric's own size

    def run(plan, row):
        n, span = len(row), plan["span"]
        x = np.concatenate([row.astype(F64), np.full(plan["N"] - n, np.inf)])
        idx = np.arange(plan["N"])

        def stage(j, partner):
            lo = idx[(idx & j) == 0] if partner is None else idx[idx < partner(idx)]
            hi = lo + j if partner is None else partner(lo)
            a, b = np.minimum(x[lo], x[hi]), np.maximum(x[lo], x[hi])
            x[lo], x[hi] = a, b
        for name, j, mirror in plan["launches"]:
            if name == "sort_rows_chunk":
                x[:] = np.sort(x.reshape(-1, span), axis=1).reshape(-1)
            elif name == "sort_rows_global":
                stage(j, (lambda i, m=mirror: i ^ m) if mirror else None)
            else:
                j = span >> 1
                while j >= 1:
                    stage(j, None)
                    j >>= 1
        return x[:n]
    rng = np.random.default_rng(5)
    for n in sorted({c["n"] for c in SC.SORT}):
        row = rng.permutation(n)
        assert np.array_equal(run(SC.sort_plan(1, n), row), np.sort(row)), n


# ------------------------------------------------------------------ the library's host-only hooks
def test_block_counts_match_the_library(lib):
    """bg_swd_standardize_workspace_bytes = (6 stats_blocks + 6) doubles and bg_abs_diff_mean_workspace_bytes = nseg abs_diff_blocks
    doubles: on the tables and on a seeded sweep of 2000 (rows, nhood) and (seg, nseg) pairs that reaches 1, several and the cap."""
    for c in SC.STD:
        assert lib.bg_swd_standardize_workspace_bytes(c["rows"], c["nhood"]) == SC.standardize_workspace_bytes(c["rows"], c["nhood"]), SC.case_id(c)
    for c in SC.ABSDIFF:
        assert lib.bg_abs_diff_mean_workspace_bytes(c["seg"], c["nseg"]) == SC.abs_diff_workspace_bytes(c["seg"], c["nseg"]), SC.case_id(c)
    rng = np.random.default_rng(20261019)
    seen_s, seen_a = set(), set()
    for _ in range(2000):
        nhood = int(rng.choice([1, 3, 5, 7, 9, 11]))
        total = int(rng.choice([rng.integers(1, 5000), rng.integers(1, 1 << 21), SC.PARTIAL_SPAN * int(rng.integers(1, 300)) + int(rng.integers(-2, 3))]))
        rows = max(1, total // (3 * nhood * nhood) + int(rng.integers(0, 2)))
        nb = SC.stats_blocks(rows * 3 * nhood * nhood)
        seen_s.add(SC._nb_tag(nb))
        assert lib.bg_swd_standardize_workspace_bytes(rows, nhood) == (6 * nb + 6) * 8, (rows, nhood)
        seg = max(1, int(rng.choice([rng.integers(1, 5000), rng.integers(1, 1 << 21), SC.PARTIAL_SPAN * int(rng.integers(1, 300)) + int(rng.integers(-2, 3))])))
        nseg = int(rng.integers(1, 9))
        seen_a.add(SC._nb_tag(SC.abs_diff_blocks(seg)))
        assert lib.bg_abs_diff_mean_workspace_bytes(seg, nseg) == nseg * SC.abs_diff_blocks(seg) * 8, (seg, nseg)
    assert seen_s == seen_a == {"nb1", "nbN", "nbcap"}
    assert lib.bg_swd_standardize_workspace_bytes(0, 7) == 0 == lib.bg_abs_diff_mean_workspace_bytes(0, 3)
    assert SC.stats_blocks(255 * 4096) == 255 and SC.stats_blocks(255 * 4096 + 1) == 256 == SC.stats_blocks(1 << 30)


# ------------------------------------------------------------------ the recipes are exact
@pytest.mark.parametrize("case", SC.INGEST, ids=[SC.case_id(c) for c in SC.INGEST])
def test_ingest_recipe_names_its_source(case):
    src, planar, want = SC.ingest_data(case)
    assert len(np.unique(src)) == src.size and src.min() == 1 and np.abs(want).max() < 1 << 24
    s32 = src.astype(F32)
    assert np.array_equal(s32.astype(F64), src)
    p32 = np.transpose(s32, (0, 3, 1, 2)) if case["nhwc"] else s32
    got = p32 * F32(SC.SCALE) + F32(SC.SHIFT)                     # two float32 roundings, as the kernel
    got = np.repeat(got, 3, axis=1) if case["C"] == 1 else got
    assert bits_equal(got, want) and want.shape == (case["B"], 3, case["H"], case["W"])
    assert SC.decode_ingest(case, got, want) == "equal"
    if src.size < 1 << 16:
        wrong = got.copy()
        wrong[-1, 2, -1, -1] = got[0, 0, 0, 0]
        assert "it holds: image 0" in SC.decode_ingest(case, wrong, want)


@pytest.mark.parametrize("case", SC.DOWN, ids=[SC.case_id(c) for c in SC.DOWN])
def test_pyr_down_integer_recipe_is_exact(case):
    """float32 pyr_down equals its float64 evaluation bit for bit, and so does pyr_down of the result where it is large enough."""
    from blurred_gan_amd import sliced_wasserstein as sw
    x = SC.down_data(case, "int")
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 255 and x.min() < 0 < x.max()
    d64, d32 = sw.pyr_down(x), sw.pyr_down(x.astype(F32))
    assert bits_equal(d32, d64)
    if min(d64.shape[2:]) >= 3:
        assert bits_equal(sw.pyr_down(d32), sw.pyr_down(d64))
    if "frac" in SC.pyr_recipes(case):
        f = SC.down_data(case, "frac")
        assert f.dtype == F32 and f.min() < 0 < f.max() and not np.array_equal(f, np.round(f))
    else:
        assert case["edge"] is not None                           # only the second-trip shapes go without the fractional recipe


@pytest.mark.parametrize("case", SC.UP, ids=[SC.case_id(c) for c in SC.UP])
def test_pyr_up_integer_recipe_is_exact(case):
    """low = pyr_down(integer image): pyr_up(low) and image - pyr_up(low), level 0 of a two-level Laplacian pyramid, are float32
    numbers exactly."""
    from blurred_gan_amd import sliced_wasserstein as sw
    low, x = SC.up_data(case, "int")
    assert low.dtype == F64 and low.shape == (1, case["planes"], case["h"], case["w"]) and np.array_equal(x, np.round(x))
    low32 = low.astype(F32)
    assert np.array_equal(low32.astype(F64), low) and low.min() < 0 < low.max()
    u64, u32 = sw.pyr_up(low), sw.pyr_up(low32)
    assert bits_equal(u32, u64) and bits_equal(x.astype(F32) - u32, x - u64)
    pyr32 = sw.generate_laplacian_pyramid(x.astype(F32), 2)        # the host path (float32 throughout) against the float64 evaluation
    assert pyr32[0].dtype == F32 and np.array_equal(pyr32[0].astype(F64), x - u64) and np.array_equal(pyr32[1].astype(F64), low)
    assert (x - u64).min() < 0 < (x - u64).max()                  # signed residuals


def test_a_third_pyramid_level_is_not_exact():
    """Why the exact multi-level cases stop at two levels: the middle level of a three-level pyramid rounds in float32."""
    from blurred_gan_amd import sliced_wasserstein as sw
    x = SC.int_image((2, 3, 32, 32), np.random.default_rng(7))
    p32 = sw.generate_laplacian_pyramid(x.astype(F32), 3)
    d1 = sw.pyr_down(x)
    d2 = sw.pyr_down(d1)
    p64 = [x - sw.pyr_up(d1), d1 - sw.pyr_up(d2), d2]
    assert all(p.dtype == F64 for p in p64) and all(p.dtype == F32 for p in p32)
    assert np.array_equal(p32[0].astype(F64), p64[0]) and np.array_equal(p32[2].astype(F64), p64[2])
    assert not np.array_equal(p32[1].astype(F64), p64[1])


@pytest.mark.parametrize("case", SC.GATHER, ids=[SC.case_id(c) for c in SC.GATHER])
def test_gather_recipe_names_its_source(case):
    level = SC.gather_level(case)
    assert level.max() < 1 << 24 and len(np.unique(level)) == level.size
    cx, cy = SC.gather_centres(case)
    n, half, pi = case["nhood"], case["nhood"] // 2, case["per_image"]
    assert cx.dtype == np.int32 and len(cx) == len(cy) == case["B"] * pi
    assert cx.min() >= half and cx.max() < case["W"] - half and cy.min() >= half and cy.max() < case["H"] - half
    assert (cx[0], cy[0]) == (half, half) and (cx[-1], cy[-1]) == (case["W"] - half - 1, case["H"] - half - 1)
    want = SC.gather_ref(level, cx, cy, n, pi)
    assert want.shape == (len(cx), 3, n, n)
    for t in sorted({0, len(cx) // 2, len(cx) - 1}):              # the formula, spelled out
        for c, a, b in ((0, 0, 0), (1, n - 1, 0), (2, 0, n - 1), (2, n - 1, n - 1)):
            assert want[t, c, a, b] == level[t // pi, c, cy[t] + b - half, cx[t] + a - half]
    if n * n * 3 * len(cx) < 1 << 16:                             # the host function with the same centres agrees
        from blurred_gan_amd import sliced_wasserstein as sw

        class Fixed:
            def __init__(self):
                self.q = [cx, cy]

            def randint(self, lo, hi, size):
                return self.q.pop(0).reshape(size).astype(np.int64)
        assert np.array_equal(sw.get_descriptors_for_minibatch(level, n, pi, Fixed()), want)
    wrong = want.copy()
    wrong[-1, 2, n - 1, n - 1] = level[0, 1, 2, 3]
    assert "got 33.0 = (image 0, channel 1, y 2, x 3)".replace("33.0", str(float(level[0, 1, 2, 3]))) in SC.decode_level(case, wrong, want)
    if case["cell"] == "gather n1 V4 pi1 t1":                     # every quad crosses b, a, c, t and an image boundary
        assert 3 * n * n == 3 and pi == 1 and SC.describe(case)["total"] // 4 == 3


@pytest.mark.parametrize("case", SC.STD, ids=[SC.case_id(c) for c in SC.STD])
def test_standardize_recipe_is_exact(case):
    """float64 numpy returns exactly (m_c, 2^k_c); the float32 casts, the difference and the quotient are exact: the output is d."""
    x, d = SC.std_data(case)
    assert set(np.unique(d)) == {-1.0, 1.0} and (d.sum(axis=(0, 2, 3)) == 0).all()
    assert (np.square(d).sum(axis=(0, 2, 3)) == case["rows"] * case["nhood"] ** 2).all()
    x32 = x.astype(F32)
    assert np.array_equal(x32.astype(F64), x)
    mean = x.sum(axis=(0, 2, 3)) / (case["rows"] * case["nhood"] ** 2)
    var = np.square(x - mean.reshape(1, 3, 1, 1)).sum(axis=(0, 2, 3)) / (case["rows"] * case["nhood"] ** 2)
    want = SC.std_stats().reshape(3, 2)
    assert np.array_equal(mean, want[:, 0]) and np.array_equal(np.sqrt(var), want[:, 1])
    assert np.array_equal(x.mean(axis=(0, 2, 3)), want[:, 0]) and np.array_equal(x.std(axis=(0, 2, 3)), want[:, 1])
    m32, s32 = want[:, 0].astype(F32).reshape(1, 3, 1, 1), want[:, 1].astype(F32).reshape(1, 3, 1, 1)
    assert bits_equal((x32 - m32) / s32, d)
    assert len(set(zip(SC.STD_M, SC.STD_K))) == 3
    for c in range(3):                                            # another channel's statistics are far from +-1
        for o in range(3):
            if o != c:
                off = (x32[:, c] - m32[0, o]) / s32[0, o]
                assert np.abs(np.abs(off) - 1).min() >= 0.25


@pytest.mark.parametrize("case", SC.SORT, ids=[SC.case_id(c) for c in SC.SORT])
def test_sort_recipes(case):
    kinds = SC.sort_kinds(case)
    assert "perm" in kinds and (set(kinds) == set(SC.KINDS) or case["rows"] * case["n"] > 1 << 20)
    x = SC.sort_data(case, "perm")
    assert x.dtype == F32 and x.shape == (case["rows"], case["n"]) and np.abs(x).max() < 1 << 24
    rows = np.sort(x, axis=1)
    assert (np.diff(rows, axis=1) == 1).all() and (rows[:, 0] == -(case["n"] // 2)).all()        # each row: distinct consecutive integers
    assert case["rows"] == 1 or not np.array_equal(x[0], x[1])
    if "special" in kinds and case["n"] >= 16:
        s = SC.sort_data(case, "special")
        assert np.isinf(s).any() and (s == 0).any() and not np.isnan(s).any()
    if "duplicates" in kinds and case["n"] >= 16:
        assert len(np.unique(SC.sort_data(case, "duplicates"))) <= 8


@pytest.mark.parametrize("case", SC.ABSDIFF, ids=[SC.case_id(c) for c in SC.ABSDIFF])
def test_abs_diff_recipe_is_exact_in_any_order(case):
    a, b, want = SC.absdiff_data(case)
    seg, nseg = case["seg"], case["nseg"]
    diff32 = np.abs(a.astype(F32) - b.astype(F32))
    assert diff32.dtype == F32 and np.array_equal(diff32.astype(F64), np.abs(a - b)) and 255 * seg < 1 << 53
    d = diff32.astype(F64).reshape(nseg, seg)
    assert np.array_equal(d.sum(axis=1) / seg, want) and np.array_equal(d[:, ::-1].cumsum(axis=1)[:, -1] / seg, want)
    assert len(set(want)) == nseg or seg < 16                     # the segments differ: a swapped segment shows
