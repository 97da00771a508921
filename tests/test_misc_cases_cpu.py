"""CPU checks of tests/misc_cases.py, the case tables of tests/test_misc_edges_gpu.py:

1. every "exact" case meets the exactness condition: its reference formula evaluated in numpy float32 in two different summation
   orders equals the float64 evaluation bit for bit, and the largest sum of magnitudes stays below 2^24 quanta (so no partial sum
   of ANY order rounds) -- a case that fails this is ill-chosen and is replaced, never given a tolerance;
2. every case lands on the route and loop shape it is in the table for: the host predicates and the kernels' loop bounds, restated
   in misc_cases.py from csrc/misc.hip, must agree with the facts the case carries.
"""
import os

import numpy as np
import pytest

import misc_cases as MC

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blurred-gan_amd", "csrc", "misc.hip")


def _exact(ref, keys=None):
    """ref(dtype, order, budget) -> array or dict of arrays."""
    budget = MC.Budget()
    want = ref(np.float64, "pairwise", budget)
    assert budget.worst < MC.TWO24, f"partial sums reach {budget.worst:g} quanta"
    for order in MC.ORDERS32:
        got = ref(np.float32, order, None)
        for k in (keys or (want.keys() if isinstance(want, dict) else [None])):
            g, w = (got[k], want[k]) if k is not None else (got, want)
            assert g.dtype == np.float32 and w.dtype == np.float64
            assert np.array_equal(g.astype(np.float64), w), (k, order)


def _holds(shape, facts):
    for k, v in facts.items():
        assert shape[k] == v, (k, shape[k], v, shape)


def test_predicates_restate_the_source():
    """The lines of misc.hip the predicates are restated from are still there, letter for letter; the grid cap and the fold of
    partial rows that it shares with other files, in the headers it takes them from (misc.hip calls them with its own kT)."""
    src = open(SRC).read()
    csrc = os.path.dirname(SRC)
    assert "std::min<size_t>(cdiv(n, (size_t)threads * per_thread), 256 * 8)" in open(os.path.join(csrc, "common.h")).read()
    assert "for (; b + 7 * 64 < nblk; b += 8 * 64, p += 8 * step) {" in open(os.path.join(csrc, "reduce.h")).read()
    for line in ["inline unsigned grid_for(size_t n, int per_thread = 1) { return bg::grid_cap(n, kT, per_thread); }",
                 "float s = bg::lane_sum_partials(partial, nblk, NQ, q, C, c);", "constexpr int kT = 256;",
                 "return C >= 4 && C <= 1024 && (C & (C - 1)) == 0 && M >= 64;", "std::min<size_t>({cap, total4 / (kT * 8), (size_t)M})",
                 "(size_t)atoi(getenv(\"BG_FLAT_BLOCKS\")) : 512;", "std::max(1, std::min(kColBlocks, M / 16))", "constexpr int kColBlocks = 256;",
                 "if (N == 1 && !transA && K >= 64) {", "if (N == 1 && transA && K >= 64) {", "if ((size_t)M * N >= 4096 && K >= 8) {",
                 "for (; q4 + (size_t)(U - 1) * kT < total4; q4 += (size_t)U * kT) {",
                 "for (; q + stride < total4; q += 2 * stride) {", "if ((stride * 4u) % (unsigned)C == 0u) {", "flat_reduce<1, 8>(",
                 "flat_reduce<2, 8>(", "flat_reduce<2, 4>(", "dim3(grid_for(n, vec ? 4 : 1))"]:
        assert line in src, line
    assert "BG_FLAT_BLOCKS" not in os.environ


# ------------------------------------------------------------------ column reductions
@pytest.mark.parametrize("shape,tag,facts", MC.RED_SHAPES, ids=[f"{s[0]}x{s[1]}" for s, _, _ in MC.RED_SHAPES])
def test_reduction_case(shape, tag, facts):
    M, C = shape
    d = MC.red_inputs(M, C)
    assert np.abs(d["x"]).max() <= 5
    _exact(lambda dt, order, b: MC.red_ref(d, dt, order, b))
    _holds(MC.reduction_shape(M, C, True), facts)
    off = MC.reduction_shape(M, C, False)                      # the same shape from a pointer offset by one float
    assert off["kernel"] == "col" and off["nblk"] == MC.red_blocks(M, C)
    if MC.flat_ok(M, C):
        assert off["nblk"] == MC.flat_blocks(M, C) and off["flat_grid"]          # column kernel on the flat grid
    bwd = MC.reduction_shape(M, C, True, U=4)
    if shape == (8192, 512):
        assert bwd["main"] == 2 and bwd["tail"] == 0
    # the workspace the library asks for holds the partials of either kernel on either grid
    assert max(MC.col_blocks(M), 512) >= off["nblk"]


def test_reduction_table_reaches_every_listed_shape():
    shapes = {s: MC.reduction_shape(s[0], s[1], True) for s, _, _ in MC.RED_SHAPES}
    flat = [v for v in shapes.values() if v["kernel"] == "flat"]
    assert any(v["main"] and v["tail"] for v in flat) and any(v["main"] and not v["tail"] for v in flat) and any(not v["main"] for v in flat)
    assert any(v["empty_blocks"] for v in flat) and any(v["ragged_last"] for v in flat)
    col = [v for v in shapes.values() if v["kernel"] == "col"]
    assert any(v["empty_blocks"] for v in col) and any(v["ragged_group"] and v["col_groups"] > 1 for v in col)
    nblks = {v["nblk"] for v in shapes.values()}
    assert 450 in nblks and 512 in nblks                           # wave_sum_partials: mixed lanes, and the 8-deep loop for all
    _holds(MC.wave_sum_shape(450), dict(mixed=True, main_lanes=2, tail_lanes=62))
    _holds(MC.wave_sum_shape(512), dict(mixed=False, main_lanes=64, tail_lanes=0))


# ------------------------------------------------------------------ partial rows
@pytest.mark.parametrize("nrows", MC.PARTIAL_NROWS)
def test_partial_rows_case(nrows):
    _holds(MC.wave_sum_shape(nrows), MC.PARTIAL_TAGS[nrows])
    assert MC.is_pow2(MC.PARTIAL_M)
    for C in MC.PARTIAL_C:
        d = MC.partial_inputs(nrows, C)
        _exact(lambda dt, order, b: MC.partial_ref(d, dt, order, b))


# ------------------------------------------------------------------ BatchNorm apply family
@pytest.mark.parametrize("case", MC.APPLY_CASES, ids=[f"{c[0]}x{c[1]}-x{c[2]}-p{c[3]}" for c in MC.APPLY_CASES])
def test_apply_case(case):
    M, C, x_off, p_off, m_totals, tag, facts = case
    _holds(MC.apply_shape(M, C, x_off == 0, p_off == 0), facts)
    d = MC.apply_inputs(M, C)
    # distinct parameter sets per channel (below 105 channels): a wrong channel is a wrong number
    assert len({(a, b, c, e) for a, b, c, e in zip(d["mean"], d["inv"], d["beta"], d["gamma"])}) == C
    for Mt in m_totals:
        assert Mt >= M and MC.is_pow2(Mt)
        _exact(lambda dt, order, b: MC.apply_ref(d, dt, Mt, b))
    if M == 180000:                                                # the second iteration of a thread meets other channels
        stride4 = MC.grid_for(M * C) * MC.KT * 4
        assert stride4 % C != 0


def test_apply_table_reaches_every_listed_shape():
    shapes = [MC.apply_shape(c[0], c[1], c[2] == 0, c[3] == 0) for c in MC.APPLY_CASES]
    assert {s["path"] for s in shapes} == {"fixed", "periter", "scalar"}
    assert any(s["path"] == "fixed" and s["paired"] and s["epilogue"] for s in shapes)
    assert any(s["path"] == "fixed" and s["paired_twice"] for s in shapes)
    assert any(s["path"] == "fixed" and not s["pa"] for s in shapes)
    assert any(s["path"] == "periter" and s["iters"] > 1 for s in shapes)
    assert any(len(c[4]) == 3 and c[4][1] == 2 * c[4][0] and c[4][2] == 4 * c[4][0] == 4 * c[0] for c in MC.APPLY_CASES)


# ------------------------------------------------------------------ Dense
def _gemm_ids(cases):
    return ["-".join(str(int(v)) for v in c) for c in cases]


@pytest.mark.parametrize("M,K,full", MC.GEMV_T_CASES, ids=_gemm_ids(MC.GEMV_T_CASES))
def test_gemv_t_case(M, K, full):
    assert MC.gemm_route(M, 1, K, True, False) == "dense_gemv_t"
    d = MC.gemm_inputs(M, 1, K)
    _exact(lambda dt, order, b: MC.gemm_ref(d, dt, order, full, b))


@pytest.mark.parametrize("M,K,a_off,w_off,path,iters", MC.ROWDOT_CASES, ids=_gemm_ids([c[:4] for c in MC.ROWDOT_CASES]))
def test_rowdot_case(M, K, a_off, w_off, path, iters):
    assert MC.gemm_route(M, 1, K, False, False) == "dense_rowdot"
    _holds(MC.rowdot_shape(K, a_off == 0 and w_off == 0), dict(path=path, iters=iters))
    d = MC.gemm_inputs(M, 1, K)
    _exact(lambda dt, order, b: MC.gemm_ref(d, dt, order, True, b))


@pytest.mark.parametrize("route,case", [("dense_gemm_tiled", c) for c in MC.TILED_CASES] + [("dense_gemm", c) for c in MC.NAIVE_CASES],
                         ids=_gemm_ids(MC.TILED_CASES + MC.NAIVE_CASES))
def test_gemm_case(route, case):
    M, N, K, tA, tB = case
    assert MC.gemm_route(M, N, K, tA, tB) == route
    d = MC.gemm_inputs(M, N, K)
    _exact(lambda dt, order, b: MC.gemm_ref(d, dt, order, True, b))


def test_gemm_thresholds_are_straddled():
    assert MC.gemm_route(64, 1, 63, False, False) == "dense_gemm" and MC.gemm_route(64, 1, 64, False, False) == "dense_rowdot"
    assert MC.gemm_route(64, 1, 63, True, False) == "dense_gemm" and MC.gemm_route(64, 1, 64, True, False) == "dense_gemv_t"
    assert MC.gemm_route(65, 64, 8, False, False) == "dense_gemm_tiled" and MC.gemm_route(33, 64, 9, False, False) == "dense_gemm"


# ------------------------------------------------------------------ pointwise and small kernels
@pytest.mark.parametrize("total", sorted(MC.POINT_TOTALS))
def test_pointwise_case(total):
    B, n_per = MC.POINT_TOTALS[total]
    assert B * n_per == total
    threads = MC.GRID_CAP * MC.KT
    assert threads == 524288 and MC.pointwise_shape(total)["passes"] == (1 if total <= threads else -(-total // threads))
    if total > threads:
        assert threads % n_per != 0 and n_per % 2 == 1             # e / n_per crosses a row inside a grid-stride pass
    d = MC.point_inputs(total)
    for op in MC.POINT_OPS:
        _exact(lambda dt, order, b: MC.point_ref(op, d, dt, b))
    assert {1, 255, 256, 257, 524288, 524289, 1200003} == set(MC.POINT_TOTALS)
    assert MC.pointwise_shape(1200003)["passes"] == 3 and MC.pointwise_shape(524289)["passes"] == 2


def test_copy_cases():
    for n, do, so in MC.COPY_CASES:
        vec = do == 0 and so == 0
        s = MC.pointwise_shape(n, 4 if vec else 1)
        if n >= 2097152:
            assert s["grid"] == MC.GRID_CAP and (s["passes"] == 1 if vec and n == 2097152 else s["passes"] >= 1)
            assert vec or s["passes"] == 5 - (n == 2097152)
    assert {n % 4 for n in MC.COPY_N if n > 2000000} == {0, 1, 2, 3}       # every length of the scalar tail after a full float4 body


@pytest.mark.parametrize("n_per,off", MC.ROW_NORM_CASES)
def test_row_norm_case(n_per, off):
    s = MC.row_norm_shape(n_per, off)
    want = {(1, 0): ("scalar", 1), (3, 0): ("scalar", 1), (4, 0): ("float4", 1), (6, 0): ("scalar", 1), (4096, 0): ("float4", 1),
            (4100, 0): ("float4", 2), (12288, 0): ("float4", 3), (4, 1): ("scalar", 1), (4096, 1): ("scalar", 4), (6, 1): ("scalar", 1)}
    assert (s["path"], s["iters"]) == want[(n_per, off)]
    for b in range(MC.ROW_NORM_B):
        row, k = MC.row_norm_inputs(n_per, b)
        assert row.size == n_per and np.all(row != 0) and float((row * row).sum()) == k * k < MC.TWO24
        for order in MC.ORDERS32:
            r32 = row.astype(np.float32)[:, None]
            assert np.sqrt(MC.sum0(r32 * r32, order))[0] == np.float32(k)


@pytest.mark.parametrize("B", MC.LOSS_B)
def test_loss_case(B):
    d = MC.loss_inputs(B)
    assert np.signbit(d["rs"][0]) and d["rs"][0] == 0 and not np.signbit(d["fs"][0]) and d["fs"][0] == 0
    for with_norm in (True, False):
        keys = ["sums", "dfs", "drs", "ds"] + (["met", "gmet"] if MC.is_pow2(B) else [])    # dividing by B rounds otherwise
        _exact(lambda dt, order, b: MC.loss_ref(d, dt, order, with_norm, b), keys)
    assert {B > 256 for B in MC.LOSS_B} == {True, False} and min(MC.LOSS_B) < 64


def test_parity_bound_is_fixed_by_the_references():
    ref = np.array([1.0, -2.0, 0.0])
    err, bound, ratio = MC.parity(ref + [0, 1e-3, 0], ref, ref + 1e-7, 1e-5, 1e-6)
    assert err == pytest.approx(1e-3) and bound == pytest.approx(2.1e-5) and ratio > 1
    assert MC.parity(ref, ref, ref, 1e-5, 1e-6)[2] == 0
    assert MC.parity(ref + 2.9e-4, ref, ref + 1e-4, 1e-5, 1e-6)[2] < 1 < MC.parity(ref + 3.1e-4, ref, ref + 1e-4, 1e-5, 1e-6)[2]
    assert MC.parity([np.nan, 0, 0], ref, ref, 1e-5, 1e-6)[2] == np.inf
