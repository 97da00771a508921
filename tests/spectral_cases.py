"""The case table of the spectral normalisation kernels' route tests (csrc/spectral.hip): tests/test_spectral_cases_cpu.py holds it to
its claims on the CPU through ops.spectral.route, tests/test_spectral_routes_gpu.py runs it on the GPU.

A case is (K, N, taps) and the properties it was chosen for, one per kernel family.  describe() derives the same properties from what
bg_spectral_route reports (vec, lanes, chunks, strip_rows, pass_units, ew_units, tiles) and from the constants of the kernels that no
query reports, restated here with the line they restate: a retuning of sn_route moves a case off its claim and the CPU test fails,
where the GPU test would silently go on running some other branch.

Exact data: W in {-3 ... 3}, u and v in {-2 ... 2}, float32.  Every product and every partial sum of v^T W u is an integer below
12 K N < 2^24, so the sigma-only pass gives float(int64 reference) in any order of summation, and a row or a column that a route
drops or takes twice moves the integer."""
import numpy as np

EW_ELEMS = 16384          # spectral.hip kEwElems: elements of one dot / apply unit
WIDE_STRIP = 4            # spectral.hip kWideStrip
FINISH_THREADS = 1024     # spectral.hip kFinishThreads
TILE = 64                 # the scale kernel's tile edge


def cdiv(a, b):
    return -(-a // b)


def _c(K, N, taps, **claims):
    return dict(K=K, N=N, taps=taps, claims=claims)


# Claims (all checked by describe()):
#   route      packed / packed2 (chunks == 2) / wide
#   lanes, strip, units, last         the pass kernel: lanes of a row, rows of a unit, units, rows of the last unit
#   live_lanes                        packed: lanes of a row that hold a live vector in the first chunk
#   chunk2_live                       packed2: lanes whose second vector is live
#   wide                              (vec, lane trips of a row, live lanes of the last trip, trips of the second sweep)
#   ew, tail                          units of the dot / apply kernels, elements of the last one
#   scalar_tail                       elements of the last unit behind its last whole float4
#   midrow                            unit 1 starts inside a row (with N % 4 != 0 its float4s cross row ends)
#   scale                             "float4" / "scalar", "+T" with the transposed copy; grid = (row tiles, column tiles) per tap;
#                                     part = (rows, columns) of the last tile where it is partial, 0 where it is whole
#   finish                            the finish kernel's loops that take a second trip: subset of {"K", "N", "P"}; p8 = P % 8
CASES = [
    _c(4100, 1, 1, route="packed", lanes=1, live_lanes=1, strip=4096, units=2, last=4, ew=1, tail=4100, scalar_tail=0, scale="scalar",
       grid=(65, 1), part=(4, 1), finish={"K"}, p8=2),
    _c(8200, 2, 1, route="packed", lanes=2, live_lanes=2, strip=2048, units=5, last=8, ew=2, tail=16, scalar_tail=0, midrow=False, scale="scalar",
       grid=(129, 1), part=(8, 2), finish={"K"}, p8=5),
    _c(1100, 3, 25, route="packed", lanes=4, live_lanes=3, strip=1024, units=2, last=76, ew=1, tail=3300, scalar_tail=0, scale="scalar+T",
       grid=(1, 1), part=(44, 3), finish={"K"}, p8=2),
    _c(5470, 3, 1, route="packed", lanes=4, live_lanes=3, strip=1024, units=6, last=350, ew=2, tail=26, scalar_tail=2, midrow=True, scale="scalar",
       grid=(86, 1), part=(30, 3), finish={"K"}, p8=6),
    _c(520, 32, 1, route="packed", lanes=8, live_lanes=8, strip=512, units=2, last=8, ew=2, tail=256, scalar_tail=0, midrow=False, scale="float4",
       grid=(9, 1), part=(8, 32), finish=set(), p8=2),
    _c(272, 64, 4, route="packed", lanes=16, live_lanes=16, strip=256, units=2, last=16, ew=2, tail=1024, scalar_tail=0, midrow=False,
       scale="float4+T", grid=(2, 1), part=(4, 0), finish=set(), p8=2),
    _c(130, 128, 1, route="packed", lanes=32, live_lanes=32, strip=128, units=2, last=2, ew=2, tail=256, scalar_tail=0, midrow=False, scale="scalar",
       grid=(3, 2), part=(2, 0), finish=set(), p8=2),
    _c(204, 132, 3, route="packed", lanes=64, live_lanes=33, strip=64, units=4, last=12, ew=2, tail=10544, scalar_tail=0, midrow=True,
       scale="float4+T", grid=(2, 3), part=(4, 4), finish=set(), p8=4),
    _c(150, 260, 1, route="packed2", lanes=64, live_lanes=64, chunk2_live=1, strip=64, units=3, last=22, ew=3, tail=6232, scalar_tail=0, midrow=True,
       scale="scalar", grid=(3, 5), part=(22, 4), finish=set(), p8=3),
    _c(41, 400, 1, route="packed2", lanes=64, live_lanes=64, chunk2_live=36, strip=64, units=1, last=41, ew=2, tail=16, scalar_tail=0, midrow=True,
       scale="scalar", grid=(1, 7), part=(41, 16), finish=set(), p8=1),
    _c(210, 67, 3, route="wide", wide=(1, 2, 3, 1), strip=4, units=53, last=2, ew=1, tail=14070, scalar_tail=2, scale="scalar+T", grid=(2, 2),
       part=(6, 3), finish=set(), p8=5),
    _c(9, 1028, 1, route="wide", wide=(4, 5, 1, 2), strip=4, units=3, last=1, ew=1, tail=9252, scalar_tail=0, scale="scalar", grid=(1, 17),
       part=(9, 4), finish={"N"}, p8=3),
    _c(4100, 67, 1, route="wide", wide=(1, 2, 3, 1), strip=4, units=1025, last=4, ew=17, tail=12556, scalar_tail=0, midrow=True, scale="scalar",
       grid=(65, 2), part=(4, 3), finish={"K", "P"}, p8=1),
]

# What the table as a whole has to cover (the CPU test compares with what describe() finds, by set equality where a set is given)
COVER = dict(
    packed_lanes_multi_unit_partial={1, 2, 4, 8, 16, 32, 64},      # packed, chunks 1, more than one unit, a partial last strip
    packed2_multi_unit_partial=True, packed2_one_live_lane=True, packed2_short_single_unit=True,
    idle_lanes=True,                                               # a packed row with lanes that hold nothing
    wide_vecs={1, 4}, wide_partial_second_sweep=True, wide_last_strip_one_row=True,
    ew_multi_unit_tail={"float4", "scalar"},                       # a partial last unit that is not unit 0, with / without scalar elements
    ew_midrow=True,
    scale_T={("float4", "partial both"), ("scalar", "multi tile")},
    finish={"K", "N", "P"}, finish_p8_nonzero=True,
)


def case_id(c):
    return f"{c['K']}x{c['N']}t{c['taps']}"


IDS = [case_id(c) for c in CASES]


def describe(c, route):
    """The claims of case c, derived from ``route`` = ops.spectral.route(K, N, taps)."""
    K, N, taps = c["K"], c["N"], c["taps"]
    vec, lanes, chunks, strip, P, ew = (route[k] for k in ("vec", "lanes", "chunks", "strip_rows", "pass_units", "ew_units"))
    cols = N // vec
    d = dict(route="wide" if chunks == 0 else "packed2" if chunks == 2 else "packed", strip=strip, units=P, last=K - (P - 1) * strip)
    if chunks == 0:
        trips = cdiv(cols, 64)
        d["wide"] = (vec, trips, cols - 64 * (trips - 1), cdiv(cols, 256))
    else:
        d["lanes"], d["live_lanes"] = lanes, min(cols, lanes)
        if chunks == 2:
            d["chunk2_live"] = cols - 64
    total = K * N
    d["ew"], d["tail"] = ew, total - (ew - 1) * EW_ELEMS
    d["scalar_tail"] = total % 4
    if ew > 1:
        d["midrow"] = EW_ELEMS % N != 0
    R = K // taps
    d["scale"] = ("float4" if (R | N) % 4 == 0 else "scalar") + ("+T" if taps > 1 else "")
    d["grid"] = (cdiv(R, TILE), cdiv(N, TILE))
    d["part"] = (R % TILE, N % TILE)
    assert route["tiles"] == taps * d["grid"][0] * d["grid"][1]
    d["finish"] = {n for n, v in (("K", K), ("N", N), ("P", P)) if v > FINISH_THREADS}
    d["p8"] = P % 8
    return d


def coverage(described):
    """COVER's keys from [(case, describe(case))]."""
    cov = dict(packed_lanes_multi_unit_partial=set(), packed2_multi_unit_partial=False, packed2_one_live_lane=False,
               packed2_short_single_unit=False, idle_lanes=False, wide_vecs=set(), wide_partial_second_sweep=False,
               wide_last_strip_one_row=False, ew_multi_unit_tail=set(), ew_midrow=False, scale_T=set(), finish=set(), finish_p8_nonzero=False)
    for c, d in described:
        partial = d["units"] > 1 and d["last"] < d["strip"]
        if d["route"] == "packed":
            if partial:
                cov["packed_lanes_multi_unit_partial"].add(d["lanes"])
            cov["idle_lanes"] |= d["live_lanes"] < d["lanes"]
        elif d["route"] == "packed2":
            cov["packed2_multi_unit_partial"] |= partial
            cov["packed2_one_live_lane"] |= d["chunk2_live"] == 1
            cov["packed2_short_single_unit"] |= d["units"] == 1 and d["last"] < d["strip"]
        else:
            vec, trips, last_lanes, sweep2 = d["wide"]
            cov["wide_vecs"].add(vec)
            cov["wide_partial_second_sweep"] |= sweep2 > 1 and (c["N"] // vec) % 256 != 0
            cov["wide_last_strip_one_row"] |= d["last"] == 1
        if d["ew"] > 1 and d["tail"] < EW_ELEMS:
            cov["ew_multi_unit_tail"].add("scalar" if d["scalar_tail"] else "float4")
            cov["ew_midrow"] |= d["midrow"] and c["N"] % 4 != 0
        if d["scale"] == "float4+T" and d["part"][0] and d["part"][1] and min(d["grid"]) > 1:
            cov["scale_T"].add(("float4", "partial both"))
        if d["scale"] == "scalar+T" and d["grid"][0] * d["grid"][1] > 1:
            cov["scale_T"].add(("scalar", "multi tile"))
        cov["finish"] |= d["finish"]
        cov["finish_p8_nonzero"] |= d["p8"] != 0 and d["units"] > 8
    return cov


def exact_data(c):
    """W [K, N], u [N], v [K] of small integers as float32, and v^T W u as a Python int (int64 arithmetic)."""
    K, N = c["K"], c["N"]
    rng = np.random.default_rng([K, N, c["taps"]])
    W = rng.integers(-3, 4, size=(K, N))
    u = rng.integers(-2, 3, size=N)
    v = rng.integers(-2, 3, size=K)
    # every row must count, and none may cancel another: W[r] . u != 0 and v_r takes its sign, so every row adds a positive integer
    # and a route that drops rows -- one per unit, say -- lowers the sum whichever rows they are
    u[0] = u[0] or 1
    dead = (W @ u) == 0
    W[dead, 0] += np.where(W[dead, 0] < 3, 1, -1)
    t = W @ u
    v = np.where(v == 0, 1, np.abs(v)) * np.sign(t)
    assert (v * t > 0).all() and np.abs(W).max() <= 3 and np.abs(v).max() <= 2
    return W.astype(np.float32), u.astype(np.float32), v.astype(np.float32), int(v @ (W @ u))
