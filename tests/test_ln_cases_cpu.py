"""No GPU: what tests/ln_cases.py claims of its cases, before tests/test_layernorm_exact_gpu.py relies on it.

Exactness: every output the GPU test compares with ``array_equal`` is, evaluated in float32 with the sums taken from the front and
from the back, the float64 value bit for bit -- and every sum's magnitudes add up to fewer than 2^24 of their common quantum, so any
other order (the kernels' shuffle trees, the four waves through LDS, ln_finish_kernel's strided lanes) gives the same float32 too.
Route: each case lands where it says; the table's cells are the set written out below; the restated route and workspace formulas are
the library's.  Edges: both sides of the kink and the kink itself, every keep byte in every byte lane.  Hard inputs: the float32
yardstick that sets their bound stays within reach of the old bound."""
import numpy as np
import pytest

from blurred_gan_amd import ops
import ln_cases as LC

F32, F64 = np.float32, np.float64
LIMIT = 2.0 ** 24


class Recording(LC.Eval):
    """float64 Eval that keeps the largest sum of magnitudes, in quanta, over the sums it takes."""

    def __init__(self, d):
        self.worst = {}
        super().__init__(d)

    def _sum(self, x, axis):
        k = "row" if axis == 1 else "column"
        self.worst[k] = max(self.worst.get(k, 0.0), LC.magnitude_quanta(x, axis))
        return super()._sum(x, axis)


def _same(a, b, what):
    for k in a:
        if k == "u" and "s" in a:
            continue
        x, y = np.asarray(a[k], F64), np.asarray(b[k], F64)
        assert x.shape == y.shape and np.array_equal(x, y), (what, k, np.argwhere(x != y)[:3], x[x != y][:3], y[x != y][:3])


@pytest.mark.parametrize("i", range(len(LC.CASES)), ids=LC.IDS)
def test_float32_in_two_orders_equals_float64_and_every_sum_stays_below_2_to_24_quanta(i):
    case = LC.CASES[i]
    d = LC.exact_data(case)
    for k in ("z", "gamma", "beta", "g", "zdot", "addend", "old"):
        assert np.array_equal(d[k].astype(F32).astype(F64), d[k]), k
    ref, fwd32, rev32 = Recording(d), LC.Eval(d, F32), LC.Eval(d, F32, rev=True)
    _same(dict(mu=ref.mu, r=ref.r), dict(mu=fwd32.mu, r=fwd32.r), "statistics")
    _same(dict(mu=ref.mu, r=ref.r), dict(mu=rev32.mu, r=rev32.r), "statistics, reversed")
    if case["kind"] == "exact" and case["C"] >= 3:
        assert np.array_equal(ref.mu[:, 0], np.round(ref.mu[:, 0])) and np.abs(ref.mu).max() <= 3
        assert np.array_equal(ref.r[:, 0], np.where(np.arange(case["R"]) % 2 == 0, 0.5, 0.25))
    else:
        assert set(np.unique(ref.r)) == ({0.5} if case["C"] == 2 and case["kind"] == "exact" else {2.0})
    for name, op, args in LC.variants(case):
        if op not in case["ops"]:
            continue
        want = getattr(ref, op)(*args)
        for e, order in ((fwd32, "front"), (rev32, "back")):
            got = getattr(e, op)(*args)
            assert all(v.dtype == F32 for v in got.values()), name
            _same(want, got, f"{name}, sums from the {order}")
    print(f"[ln exact] {LC.case_id(case)}: largest sum of magnitudes, in quanta: {ref.worst}")
    assert max(ref.worst.values()) < LIMIT, ref.worst


@pytest.mark.parametrize("i", range(len(LC.CASES)), ids=LC.IDS)
def test_case_lands_on_the_route_it_claims(i):
    case = LC.CASES[i]
    C, R = case["C"], case["R"]
    t, w = LC.route_for(C), LC.rows_per_workgroup(C)
    lib = ops.layernorm.route(C)
    assert lib == dict(t, rows_per_workgroup=w)
    for cell in case["cells"]:
        if cell[0] == "C":
            want = {4: (4, 1, 1, 1), 8: (4, 2, 1, 1), 12: (4, 4, 1, 1), 16: (4, 4, 1, 1), 20: (4, 8, 1, 1), 32: (4, 8, 1, 1), 64: (4, 16, 1, 1),
                    128: (4, 32, 1, 1), 252: (4, 64, 1, 1), 256: (4, 64, 1, 1), 260: (4, 64, 2, 1), 512: (4, 64, 2, 1), 516: (4, 64, 4, 1),
                    1024: (4, 64, 4, 1), 1028: (4, 64, 1, 5), 1280: (4, 64, 1, 5), 1: (1, 1, 1, 1), 2: (1, 2, 1, 1), 3: (1, 4, 1, 1),
                    5: (1, 8, 1, 1), 7: (1, 8, 1, 1), 17: (1, 32, 1, 1), 33: (1, 64, 1, 1), 63: (1, 64, 1, 1), 65: (1, 64, 2, 1),
                    127: (1, 64, 2, 1), 129: (1, 64, 4, 1), 255: (1, 64, 4, 1), 257: (1, 64, 1, 5), 319: (1, 64, 1, 5)}[C]
            assert (t["vec"], t["lanes"], t["regs"], t["chunks"]) == want
        elif cell[0] == "R":
            assert R == {"1": 1, "w-1": max(w - 1, 1), "w": w, "w+1": w + 1, "2w+3": 2 * w + 3}[cell[1]]
        elif cell[0] == "grid stride":
            assert LC.route_class(C) == cell[1] and R == 1025 * w + 5 and LC.grid_for(R, C)[0] == 1024 and -(-R // w) == 1025 + -(-5 // w)
        elif cell[0] == "nblk":
            assert C == 4 and w == 256 and LC.grid_for(R, C) == (cell[1], 1) and R * C <= 1 << 20
            assert case["dw_rows"] == R, "a workgroup past dw_rows writes a partial row of zeros: dropping it would not show"
            u = LC.exact_data(case)["g"].reshape(cell[1], w, C)
            assert (np.abs(u).sum(1) > 0).all(), "every workgroup adds something to every channel"
        elif cell[0] == "window":
            rpw = w // 4
            end = {"keep": case["keep_rows"], "dw": case["dw_rows"], "u": case["u_hi"]}[cell[1]]
            if cell[2] == "inside a wave":
                assert rpw > 1 and end % rpw != 0
            elif cell[2] == "wave seam":
                assert end % rpw == 0 and end % w != 0
            elif cell[2] == "workgroup seam":
                assert end % w == 0 and 0 < end < R
            elif cell[2] == "one row, row0 > 0":
                assert case["u_hi"] - case["u_lo"] == 1 and case["u_lo"] > 0
            else:
                assert case["u_hi"] == R and case["u_lo"] > 0
        elif cell[0] in ("gamma 0", "offset 1", "constant rows"):
            assert LC.route_class(C) == cell[1]
            assert cell[0] != "offset 1" or (case["offset"] == 1 and t["vec"] == 1)
            assert cell[0] != "constant rows" or case["kind"] == "const"
        else:
            raise AssertionError(cell)
    assert 0 <= case["keep_rows"] <= R and 0 < case["dw_rows"] <= R and 0 <= case["u_lo"] < case["u_hi"] <= R
    assert case["offset"] == 0 or t["vec"] == 1
    if not any(c[0] == "grid stride" for c in case["cells"]):
        assert R * C <= (1 << 20) + (1 << 16), "the largest case stays near a million elements"


def test_the_sparse_rows_sit_on_the_seams_of_their_route():
    for C, must in ((257, {0, 63, 64, 127, 128, 191, 192, 255, 256}), (1028, {0, 3, 252, 255, 256, 259, 1020, 1023, 1024, 1027}),
                    (319, {0, 63, 64, 255, 256, 257, 300, 318}), (260, {0, 3, 252, 255, 256, 259}), (129, {0, 63, 64, 127, 128}),
                    (1024, {0, 255, 256, 511, 512, 767, 768, 1023})):
        seams = set(LC.seam_channels(C).tolist())
        assert must <= seams and max(seams) == C - 1, (C, sorted(must - seams))
    case = next(c for c in LC.CASES if c["C"] == 257 and c["R"] > 8)
    d = LC.exact_data(case)
    for k in ("g", "zdot"):
        nz = d[k] != 0
        assert (nz.sum(1) == 3).all() and set(np.flatnonzero(nz.any(0)).tolist()) <= set(LC.seam_channels(257).tolist())
        assert len({tuple(np.flatnonzero(r)) for r in nz}) > 1, "another set per row"


def test_the_tables_cells_are_the_set_written_out_here():
    cells = set()
    for C in (4, 8, 12, 16, 20, 32, 64, 128, 252, 256, 260, 512, 516, 1024, 1028, 1280, 1, 2, 3, 5, 7, 17, 33, 63, 65, 127, 129, 255, 257, 319):
        cells.add(("C", C))
    for k in ("1", "w-1", "w", "w+1", "2w+3"):
        cells.add(("R", k))
    for k in ("float4 subwave", "float4 regs4", "float4 chunked", "scalar subwave", "scalar chunked"):
        cells |= {("grid stride", k), ("constant rows", k)}
    for n in (1, 63, 64, 65, 448, 449, 511, 512, 513, 1024):
        cells |= {("nblk", n, "bwd"), ("nblk", n, "source")}
    for wn in ("keep", "dw", "u"):
        cells |= {("window", wn, s) for s in ("inside a wave", "wave seam", "workgroup seam")}
    cells |= {("window", "u", "one row, row0 > 0"), ("window", "u", "ends at R")}
    cells |= {("gamma 0", k) for k in ("float4 subwave", "float4 chunked", "scalar subwave", "scalar chunked")} | {("offset 1", "scalar regs4")}
    got = {tuple(x) for c in LC.CASES for x in c["cells"]}
    assert got == cells == LC.CELLS, (sorted(map(str, got - cells)), sorted(map(str, cells - got)))
    # every row-count cell on one C per route class, and the misaligned view on every kind of scalar route
    for C in LC.ALL_R_C:
        assert {x[1] for c in LC.CASES if c["C"] == C for x in c["cells"] if x[0] == "R"} == set(LC.R_KINDS), C
    assert {LC.route_class(c["C"]) for c in LC.CASES if c["offset"]} == {"scalar subwave", "scalar regs4", "scalar chunked"}
    assert {LC.route_class(C) for C in LC.CLASS_C} == set(LC.STRIDE_C) and [c["C"] for c in LC.HARD_CASES] == list(LC.CLASS_C)


def test_finish_trip_counts():
    """ln_finish_kernel: lane l's main loop runs while l + 448 < nblk in steps of 512 rows; the tail runs when a row is left."""
    want = {1: (0, 0, 1), 63: (0, 0, 63), 64: (0, 0, 64), 65: (0, 0, 64), 448: (0, 0, 64), 449: (1, 0, 63), 511: (1, 0, 1),
            512: (1, 1, 0), 513: (1, 1, 1), 1024: (2, 2, 0)}          # trips of lane 0, of lane 63, lanes whose tail runs
    assert set(want) == set(LC.NBLK)
    for n, (first, last, tails) in want.items():
        main, tail = LC.finish_trips(n)
        assert (main[0], main[63], sum(tail)) == (first, last, tails), (n, main[0], main[63], sum(tail))
        left = [len(range(lane + 512 * main[lane], n, 64)) for lane in range(64)]          # rows a lane's tail adds
        assert sum(8 * m for m in main) + sum(left) == n and max(left) <= 8 and [x > 0 for x in left] == tail, n


def test_restated_routes_are_the_librarys():
    for C in range(1, 2101):
        assert ops.layernorm.route(C) == dict(LC.route_for(C), rows_per_workgroup=LC.rows_per_workgroup(C)), C
    for c in LC.CASES + LC.HARD_CASES:
        assert ops.layernorm.workspace_bytes(c["R"], c["C"]) == LC.workspace_bytes(c["R"], c["C"]), (c["R"], c["C"])
    rng = np.random.default_rng(20261020)
    for R, C in zip(rng.integers(1, 300000, size=2000).tolist(), rng.integers(1, 2101, size=2000).tolist()):
        assert ops.layernorm.workspace_bytes(R, C) == LC.workspace_bytes(R, C), (R, C)
    assert ops.layernorm.workspace_bytes(0, 4) == 0 == LC.workspace_bytes(0, 4) and ops.layernorm.workspace_bytes(4, 0) == 0 == LC.workspace_bytes(4, -1)


def test_every_case_holds_the_kink_both_its_sides_and_every_keep_byte_in_every_lane():
    """C = 1 is exempt one case at a time (its one pre-activation per row is beta) and holds the three sides over its cases; a
    mask of fewer than 20 bytes cannot hold 5 values in 4 lanes and holds the first of them in order."""
    sides_c1 = set()
    for case in LC.CASES:
        d = LC.exact_data(case)
        n = LC.Eval(d).n
        sides = {int(s) for s in np.unique(np.sign(n))}
        if case["C"] == 1:
            sides_c1 |= sides
        else:
            assert sides == {-1, 0, 1}, (LC.case_id(case), sides)
        for rows in {case["R"], case["keep_rows"]} - {0}:
            k = d["keep"][:rows].ravel()
            seen = {(int(v), i % 4) for i, v in enumerate(k[:4096])}
            if k.size >= 20:
                assert seen == {(v, l) for v in LC.KEEP_BYTES for l in range(4)}, LC.case_id(case)
            else:
                assert len(seen) == k.size
        if case.get("gamma0"):
            assert (d["gamma"] == 0).sum() == 2
    assert sides_c1 == {-1, 0, 1}


# ------------------------------------------------------------------ hard inputs
@pytest.mark.parametrize("case", LC.HARD_CASES, ids=[f"C{c['C']}" for c in LC.HARD_CASES])
def test_hard_inputs_leave_a_margin(case):
    ref = LC.hard_reference(case)
    d = ref["data"]
    assert np.abs(ref["eval"].n).min() > 0.5, "a pre-activation near the kink"
    assert set(d["row_kind"].tolist()) == {0, 1, 2}
    for k, (want, bound, old, dev3, scale) in ref["out"].items():
        print(f"[ln hard] C={case['C']} {k}: 3 x float32 deviation / old bound at the rows' scale {float((dev3 / old).max()):.2f}, "
              f"/ the rows' scale {float((dev3 / scale).max()):.1e}")
        assert (dev3 <= 10 * old).all(), (k, float((dev3 / old).max()))
        assert (dev3 <= 1e-2 * scale).all(), (k, float((dev3 / scale).max()))
