"""Case tables, integer-data generators, float64 references and restated host predicates for the support kernels of
csrc/misc.hip (tests/test_misc_cases_cpu.py checks the tables on the CPU, tests/test_misc_edges_gpu.py runs them on the GPU).

The method: a sum of small integers (times a power of two) is exact in float32 in ANY order while every partial sum stays below
2^24 quanta, so on such data a correct kernel equals the float64 reference bit for bit whatever its blocking, unrolling or
reduction tree, and a dropped, doubled or mis-indexed element moves the result by at least one quantum.  Every reference below is
written once, for a dtype and a summation order: float64 is the reference, float32 in two other orders is the exactness proof.

The predicates (grid_for, flat_ok, flat_blocks, col_blocks, gemm_route, ...) restate the host code of misc.hip; the shape functions
(reduction_shape, wave_sum_shape, apply_shape, ...) restate the loops of its kernels, so that each case can carry the route and
loop shape it is in the table for and the CPU test can hold the table to it.
"""
import math

import numpy as np

KT = 256                      # threads per workgroup of the grid-stride kernels (misc.hip kT)
GRID_CAP = 256 * 8            # grid_for's cap on workgroups
TWO24 = float(1 << 24)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ host predicates of misc.hip, restated
def grid_for(n, per_thread=1):
    return max(1, min(cdiv(n, KT * per_thread), GRID_CAP))


def flat_ok(M, C):
    return 4 <= C <= 1024 and (C & (C - 1)) == 0 and M >= 64


def flat_blocks(M, C):
    return max(1, min(512, (M * C // 4) // (KT * 8), M))      # the cap is 512 unless BG_FLAT_BLOCKS is set (it is not)


def col_blocks(M):
    return max(1, min(256, M // 16))


def red_blocks(M, C):
    return flat_blocks(M, C) if flat_ok(M, C) else col_blocks(M)


def gemm_route(M, N, K, tA, tB):
    if N == 1 and not tA and K >= 64:
        return "dense_rowdot"
    if N == 1 and tA and K >= 64:
        return "dense_gemv_t"
    if M * N >= 4096 and K >= 8:
        return "dense_gemm_tiled"
    return "dense_gemm"


# ------------------------------------------------------------------ loop shapes of the kernels, restated
def reduction_shape(M, C, aligned, U=8):
    """Partial pass of bg_colsum_f32 / bg_bn_stats_f32 (U = 8) / bg_bn_bwd_stats_f32 (U = 4).  kernel: 'flat' (flat_reduce) or
    'col' (col_reduce); the grid's x size is red_blocks either way, so an unaligned flat_ok shape runs col_reduce on the flat
    grid.  main / tail: iterations of flat_reduce's unrolled loop and of its tail loop for thread 0 of a FULL block."""
    nblk = red_blocks(M, C)
    rows_per = cdiv(M, nblk)
    used = cdiv(M, rows_per)
    s = dict(kernel="flat" if flat_ok(M, C) and aligned else "col", flat_grid=flat_ok(M, C), nblk=nblk, rows_per=rows_per,
             empty_blocks=nblk - used, ragged_last=M - (used - 1) * rows_per != rows_per, col_groups=cdiv(C, 64),
             ragged_group=C % 64 != 0)
    if s["kernel"] == "flat":
        total4 = rows_per * (C // 4)
        q4 = main = 0
        while q4 + (U - 1) * KT < total4:
            q4, main = q4 + U * KT, main + 1
        s.update(G=C // 4, total4=total4, main=main, tail=len(range(q4, total4, KT)))
    return s


def wave_sum_shape(nblk):
    """wave_sum_partials: lane b0 runs the 8-deep loop while b0 + 512 k + 448 < nblk, then the predicated last batch if rows are
    left.  main_lanes / tail_lanes: how many of the 64 lanes enter each; mixed: lanes of one wave take different loops."""
    main_iters, tail = [], []
    for b0 in range(64):
        b = b0
        it = 0
        while b + 7 * 64 < nblk:
            b, it = b + 8 * 64, it + 1
        main_iters.append(it)
        tail.append(b < nblk)
    ml, tl = sum(1 for i in main_iters if i), sum(tail)
    return dict(main_lanes=ml, tail_lanes=tl, main_iters=max(main_iters), mixed=0 < ml < 64 or (ml == 64 and 0 < tl < 64))


def apply_shape(M, C, act_aligned=True, par_aligned=True):
    """bn_apply_kernel / bn_bwd_apply_kernel.  path: 'scalar', 'fixed' (a thread keeps its four channels: parameters read once,
    two quads in flight) or 'periter' (parameters per iteration).  paired: most entries of the two-in-flight loop by any thread;
    paired_twice: threads that enter it at least twice; epilogue: threads that run the single-quad epilogue; iters: iterations
    of thread 0 in the other two loops."""
    total = M * C
    grid = grid_for(total)
    stride = grid * KT
    if C % 4 or not act_aligned:
        return dict(path="scalar", grid=grid, iters=len(range(0, total, stride)))
    total4 = total // 4
    if (stride * 4) % C == 0:
        q, paired = np.arange(stride, dtype=np.int64), np.zeros(stride, np.int64)
        while True:
            m = q + stride < total4
            if not m.any():
                break
            paired += m
            q += 2 * stride * m
        return dict(path="fixed", pa=par_aligned, grid=grid, paired=int(paired.max()), paired_twice=int((paired >= 2).sum()),
                    epilogue=int((q < total4).sum()))
    return dict(path="periter", pa=par_aligned, grid=grid, iters=len(range(0, total4, stride)))


def pointwise_shape(total, per_thread=1):
    grid = grid_for(total, per_thread)
    return dict(grid=grid, passes=cdiv(cdiv(total, per_thread), grid * KT))


def rowdot_shape(K, aligned):
    vec = K % 4 == 0 and aligned
    return dict(path="float4" if vec else "scalar", iters=len(range(0, K // 4 if vec else K, KT)))


def row_norm_shape(n_per, base_off):
    """row_norm_kernel (1024 threads per row): the float4 branch needs n_per % 4 == 0 AND a 16-byte aligned row.  With
    n_per % 4 == 0 every row has the base's alignment; rows of alternating alignment exist only for n_per % 4 == 2, and those
    take the scalar branch for the first reason already."""
    vec = n_per % 4 == 0 and base_off % 4 == 0
    return dict(path="float4" if vec else "scalar", iters=len(range(0, n_per // 4 if vec else n_per, 1024)),
                alternating=n_per % 4 == 2)


# ------------------------------------------------------------------ exactness bookkeeping
class Budget:
    """Collects, for every reduction (or rounding-free expression) of a reference, the largest sum of magnitudes in units of
    the data's quantum.  Any partial sum in any order is a multiple of the quantum no larger than that, so below 2^24 it is a
    float32 number."""

    def __init__(self):
        self.worst = 0.0

    def note(self, terms, quantum, axis=None):
        t = np.asarray(terms, np.float64) / quantum
        assert np.array_equal(t, np.round(t)), "terms are not multiples of the stated quantum"
        self.worst = max(self.worst, float(np.abs(t).sum(axis).max()) if axis is not None else float(np.abs(t).max()))


def sum0(a, order):
    """Sum over axis 0 in a's own dtype: 'pairwise' (numpy's), 'sequential' (a running sum), 'blocked' (37-row blocks summed
    from the bottom up, then the block sums)."""
    if order == "pairwise":
        return a.sum(0, dtype=a.dtype)
    if order == "sequential":
        return np.cumsum(a, axis=0, dtype=a.dtype)[-1]
    assert order == "blocked"
    blocks = [np.cumsum(a[i:i + 37][::-1], axis=0, dtype=a.dtype)[-1] for i in range(0, a.shape[0], 37)]
    return np.cumsum(np.stack(blocks[::-1]), axis=0, dtype=a.dtype)[-1]


def matmul(a, b, order):
    """a @ b in the operands' dtype: BLAS order, or with the k axis reversed / split in two halves."""
    if order == "pairwise":
        return a @ b
    if order == "sequential":
        return a[:, ::-1] @ b[::-1]
    h = a.shape[1] // 2
    return (a[:, h:] @ b[h:] + a[:, :h] @ b[:h]) if h else a @ b


ORDERS32 = ("sequential", "blocked")


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def col_skew(C, period, lo):
    return (np.arange(C) % period + lo).astype(np.float64)


def lrelu(v, alpha):
    return np.where(v > 0, v, v.dtype.type(alpha) * v)


def mask(v, alpha):
    return np.where(v > 0, v.dtype.type(1), v.dtype.type(alpha))


def cast(d, dt):
    return {k: (v.astype(dt) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in d.items()}


# ------------------------------------------------------------------ column reductions
# (M, C), what the case is in the table for, and the facts of reduction_shape that make it so (x aligned)
RED_SHAPES = [
    ((64, 4), "flat, 1 block, fewer quads than threads", dict(kernel="flat", nblk=1, total4=64, main=0, tail=1)),
    ((63, 64), "just under the flat threshold", dict(kernel="col", flat_grid=False, nblk=3)),
    ((100, 256), "flat, 3 blocks, ragged last block", dict(kernel="flat", nblk=3, rows_per=34, ragged_last=True, main=1, tail=1)),
    ((128, 1024), "flat, G = 256", dict(kernel="flat", G=256, nblk=16, main=1, tail=0)),
    ((1001, 1024), "flat, 125 blocks with rows_per 9, trailing blocks empty",
     dict(kernel="flat", nblk=125, rows_per=9, empty_blocks=13, ragged_last=True, main=1, tail=1)),
    ((8192, 512), "flat, 512 blocks, unrolled main loop", dict(kernel="flat", nblk=512, rows_per=16, main=1, tail=0)),
    ((7200, 512), "nblk = 450: the mixed case of wave_sum_partials", dict(kernel="flat", nblk=450, empty_blocks=0)),
    ((5, 3), "column kernel, one block", dict(kernel="col", nblk=1, col_groups=1)),
    ((16, 1), "column kernel, one column", dict(kernel="col", nblk=1, col_groups=1)),
    ((4097, 70), "column kernel, empty trailing blocks, two column groups, the second ragged",
     dict(kernel="col", nblk=256, rows_per=17, empty_blocks=15, col_groups=2, ragged_group=True)),
    ((300, 2048), "column kernel, C above the flat range", dict(kernel="col", flat_grid=False, nblk=18, col_groups=32)),
    ((1000, 12), "column kernel, C no power of two", dict(kernel="col", flat_grid=False, nblk=62, ragged_last=True)),
]
RED_CASES = [(shape, off) for shape, _, _ in RED_SHAPES for off in (0, 1)]      # off: x (dy, y) start `off` floats past 16 bytes
RED_ALPHA, RED_BETA, RED_SCALE = 0.5, 2.0, 0.5


def red_inputs(M, C):
    rng = np.random.default_rng(1000 * M + C)
    d = dict(x=ints(rng, (M, C), -3, 3) + col_skew(C, 5, -2), dy=ints(rng, (M, C), -3, 3), out0=ints(rng, (C,), -9, 9),
             mean=col_skew(C, 3, -1), inv=np.full(C, 0.5), gamma=np.full(C, 2.0), beta=col_skew(C, 2, 0))
    d["y"] = lrelu(d["gamma"] * ((d["x"] - d["mean"]) * d["inv"]) + d["beta"], RED_ALPHA)
    return d


def red_ref(d, dt, order, budget=None):
    d = cast(d, dt)
    x, dy = d["x"], d["dy"]
    dz = dy * mask(d["gamma"] * ((x - d["mean"]) * d["inv"]) + d["beta"], RED_ALPHA)
    xh = (x - d["mean"]) * d["inv"]
    if budget:
        budget.note(x, 1, 0), budget.note(x * x, 1, 0), budget.note(dz, 0.5, 0), budget.note(dz * xh, 0.25, 0)
        budget.note(dt(RED_BETA) * d["out0"] + dt(RED_SCALE) * np.abs(x).sum(0), 0.5)
    sx, sxx = sum0(x, order), sum0(x * x, order)
    return dict(colsum=dt(RED_BETA) * d["out0"] + dt(RED_SCALE) * sx, colsq=sxx, stats=np.concatenate([sx, sxx]),
                bwd=np.concatenate([sum0(dz, order), sum0(dz * xh, order)]))


# ------------------------------------------------------------------ wave_sum_partials through the partial-row entry points
PARTIAL_NROWS = [1, 2, 63, 64, 65, 447, 448, 449, 511, 512, 513, 1061, 2048]
PARTIAL_C = [1, 3, 64, 130]
PARTIAL_TAGS = {        # nrows -> facts of wave_sum_shape
    1: dict(main_lanes=0, tail_lanes=1), 2: dict(main_lanes=0, tail_lanes=2), 63: dict(main_lanes=0, tail_lanes=63),
    64: dict(main_lanes=0, tail_lanes=64), 65: dict(main_lanes=0, tail_lanes=64), 447: dict(main_lanes=0, tail_lanes=64, mixed=False),
    448: dict(main_lanes=0, tail_lanes=64, mixed=False), 449: dict(main_lanes=1, tail_lanes=63, mixed=True),
    511: dict(main_lanes=63, tail_lanes=1, mixed=True), 512: dict(main_lanes=64, tail_lanes=0, mixed=False),
    513: dict(main_lanes=64, tail_lanes=1, mixed=True), 1061: dict(main_lanes=64, tail_lanes=37, main_iters=2, mixed=True),
    2048: dict(main_lanes=64, tail_lanes=0, main_iters=4, mixed=False),
}
PARTIAL_M, PARTIAL_MOMENTUM = 64, 0.5


def partial_inputs(nrows, C):
    rng = np.random.default_rng(77 * nrows + C)
    p = ints(rng, (nrows, 2, C), -6, 6)
    p[:, 0] += col_skew(C, 3, -1)
    p[:, 1] += col_skew(C, 4, 0)
    return dict(partial=p, mm=ints(rng, (C,), -8, 8))


def partial_ref(d, dt, order, budget=None):
    d = cast(d, dt)
    p = d["partial"]
    if budget:
        budget.note(p, 1, 0)
    s = np.concatenate([sum0(p[:, 0], order), sum0(p[:, 1], order)])
    C = p.shape[2]
    mean = s[:C] / dt(PARTIAL_M)
    return dict(sums=s, save_mean=mean, moving_mean=d["mm"] * dt(PARTIAL_MOMENTUM) + mean * (dt(1) - dt(PARTIAL_MOMENTUM)))


# ------------------------------------------------------------------ BatchNorm apply family
# (M, C, x_off, par_off, M_totals of the backward apply, tag, facts of apply_shape)
APPLY_CASES = [
    (83000, 64, 0, 0, (131072,), "two-in-flight loop entered once (two quads per thread), epilogue for part of the grid",
     dict(path="fixed", pa=True, grid=2048, paired=1, epilogue=279424)),
    (100000, 64, 0, 0, (131072,), "two-in-flight loop entered a second time by part of the grid, epilogue for the rest",
     dict(path="fixed", pa=True, grid=2048, paired=2, paired_twice=27136, epilogue=497152)),
    (64, 12, 0, 0, (64, 128, 256), "C % 4 == 0 with fixed channels", dict(path="fixed", pa=True, paired=0, epilogue=192)),
    (100, 12, 0, 0, (128,), "per-iteration parameters", dict(path="periter", pa=True, iters=1)),
    (200, 20, 0, 0, (256,), "per-iteration parameters", dict(path="periter", pa=True, iters=1)),
    (180000, 12, 0, 0, (262144,), "per-iteration parameters, a second iteration at other channels",
     dict(path="periter", pa=True, grid=2048, iters=2)),
    (50, 7, 0, 0, (64,), "scalar path (C % 4 != 0)", dict(path="scalar", iters=1)),
    (4096, 64, 1, 0, (4096,), "scalar path (x offset by one float)", dict(path="scalar", iters=1)),
    (4096, 64, 0, 1, (4096, 8192, 16384), "parameters as slices at offsets 1, 2, 3 of a flat buffer: pa == false",
     dict(path="fixed", pa=False, paired=0)),
]
APPLY_ALPHA = 0.5


def apply_inputs(M, C):
    rng = np.random.default_rng(31 * M + C)
    c = np.arange(C)
    return dict(x=ints(rng, (M, C), -5, 5), dy=ints(rng, (M, C), -3, 3), mean=col_skew(C, 7, -3), beta=col_skew(C, 5, -2),
                inv=np.array([1.0, 0.5, 0.25])[c % 3], gamma=np.array([1.0, 2.0, 4.0])[(c // 3) % 3],
                db=0.5 * ints(rng, (C,), -32, 32), dg=0.25 * ints(rng, (C,), -32, 32))


def apply_ref(d, dt, M_total=None, budget=None):
    """y of bg_bn_apply_f32, and dx of bg_bn_bwd_apply_f32 when M_total is given, in misc.hip's own association."""
    d = cast(d, dt)
    xh = (d["x"] - d["mean"]) * d["inv"]
    v = d["gamma"] * xh + d["beta"]
    out = dict(y=lrelu(v, APPLY_ALPHA))
    if budget:
        budget.note(v, 0.25)
    if M_total is not None:
        dz = d["dy"] * mask(v, APPLY_ALPHA)
        inner = dt(M_total) * dz - d["db"] - xh * d["dg"]
        out["dx"] = d["gamma"] * d["inv"] * (dt(1) / dt(M_total)) * inner
        if budget:
            budget.note(np.abs(float(M_total) * dz) + np.abs(d["db"]) + np.abs(xh * d["dg"]), 1 / 16)
    return out


PARAM_GRADS_C = [1, 255, 256, 257]


# ------------------------------------------------------------------ Dense
GEMV_T_CASES = [(M, K, full) for M in (1, 63, 64, 65, 2048) for K in (64, 65, 256, 271) for full in (True, False)]
# (M, K, a_off, w_off, path, iterations of thread 0)
ROWDOT_CASES = [(M, K, 0, 0, "float4", it) for M in (1, 5) for K, it in ((64, 1), (1024, 1), (1028, 2), (6272, 7))] + \
               [(M, 67, 0, 0, "scalar", 1) for M in (1, 5)] + \
               [(M, 1024, a, w, "scalar", 4) for M in (1, 5) for a, w in ((1, 0), (0, 1))]
TRANSPOSES = [(False, False), (True, False), (False, True), (True, True)]
TILED_CASES = [(M, N, K, tA, tB) for (M, N, K) in ((65, 64, 8), (64, 65, 31), (130, 70, 32), (70, 130, 33)) for tA, tB in TRANSPOSES] + \
              [(1, 4096, 100, False, False), (4096, 1, 16, False, False), (256, 512, 100, False, False)]
NAIVE_CASES = [(M, N, K, tA, tB) for (M, N, K) in ((33, 64, 9), (7, 33, 10), (64, 1, 63)) for tA, tB in TRANSPOSES]
GEMM_SCALE, GEMM_BETA = 2.0, 0.5


def gemm_inputs(M, N, K):
    rng = np.random.default_rng(M * 131 + N * 17 + K)
    return dict(A=ints(rng, (M, K), -4, 4), B=ints(rng, (K, N), -4, 4), bias=ints(rng, (N,), -7, 7), C0=2 * ints(rng, (M, N), -5, 5))


def gemm_ref(d, dt, order, full=True, budget=None):
    d = cast(d, dt)
    acc = matmul(d["A"], d["B"], order)
    out = dt(GEMM_SCALE) * acc
    if full:
        out = out + d["bias"] + dt(GEMM_BETA) * d["C0"]
    if budget:
        budget.note(GEMM_SCALE * (np.abs(d["A"]) @ np.abs(d["B"])) + np.abs(d["bias"]) + GEMM_BETA * np.abs(d["C0"]), 1)
    return out


# ------------------------------------------------------------------ pointwise and small kernels
# total -> (B, n_per): n_per odd (no divisor of the grid's thread count) wherever the total has an odd factor
POINT_TOTALS = {1: (1, 1), 255: (3, 85), 256: (4, 64), 257: (1, 257), 524288: (128, 4096), 524289: (3, 174763), 1200003: (3, 400001)}
POINT_OPS = ["lerp", "outer", "mul_grad", "mul_grad_keep", "tanh_bwd", "fill", "scale"]
POINT_ALPHA, POINT_SCALE = 0.5, 2.0


def point_inputs(total):
    B, n_per = POINT_TOTALS[total]
    rng = np.random.default_rng(total)
    return dict(r=ints(rng, (B, n_per), -9, 9), f=ints(rng, (B, n_per), -9, 9), a=rng.choice([0.0, 0.25, 0.5, 1.0], size=B),
                s=ints(rng, (B,), -9, 9) + 10, w=ints(rng, (n_per,), -9, 9), keep=rng.integers(0, 2, size=(B, n_per)).astype(np.uint8),
                y=rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], size=(B, n_per)))


def point_ref(op, d, dt, budget=None):
    d = cast(d, dt)
    r, f = d["r"], d["f"]
    if budget:
        budget.note(np.abs(r) + np.abs(f - r), 0.25), budget.note(np.abs(d["s"]).max() * np.abs(d["w"]), 1)
    if op == "lerp":
        return r + d["a"][:, None] * (f - r)
    if op == "outer":
        return d["s"][:, None] * d["w"][None, :]
    if op == "mul_grad":
        return r * mask(f, POINT_ALPHA)
    if op == "mul_grad_keep":
        return r * np.where(d["keep"] != 0, mask(f, POINT_ALPHA) * dt(POINT_SCALE), dt(0))
    if op == "tanh_bwd":
        return f * (dt(1) - d["y"] * d["y"])
    if op == "fill":
        return np.full_like(r, dt(-2.5))
    assert op == "scale"
    return r * dt(0.25)


COPY_N = [1, 3, 4, 5, 1027, 2097152, 2097153, 2097154, 2097155]
COPY_CASES = [(n, do, so) for n in COPY_N for do in (0, 1) for so in (0, 1)]

ROW_NORM_N = [1, 3, 4, 6, 4096, 4100, 12288]
ROW_NORM_CASES = [(n, 0) for n in ROW_NORM_N] + [(4, 1), (4096, 1), (6, 1)]     # (n_per, base offset in floats)
ROW_NORM_B = 3


def row_norm_inputs(n_per, b):
    """Row b: entries +-1, +-2, +-3 whose squares sum to a perfect square k^2 (n + 3 a + 8 b' = k^2: a entries become 2, b' become 3)."""
    rng = np.random.default_rng(n_per * 7 + b)
    if n_per == 1:
        return np.array([-3.0 - b]), 3.0 + b
    k = math.isqrt(n_per - 1) + 1
    while True:
        assert k * k <= 9 * n_per
        sol = [(a, bb) for bb in range(0, 3) for a in [(k * k - n_per - 8 * bb) // 3]
               if k * k - n_per - 8 * bb >= 0 and (k * k - n_per - 8 * bb) % 3 == 0 and a + bb <= n_per]
        if sol:
            break
        k += 1
    a, bb = sol[0]
    row = np.ones(n_per)
    row[:a], row[a:a + bb] = 2.0, 3.0
    rng.shuffle(row)
    return row * rng.choice([-1.0, 1.0], size=n_per), float(k)


LOSS_B = [1, 63, 64, 255, 256, 257, 700]
LOSS = dict(inv_gbs=1 / 32, gp_coef=8.0, e_drift=2.0 ** -10, vec_scale=4.0)


def loss_inputs(B):
    rng = np.random.default_rng(500 + B)
    fs, rs = 0.5 * ints(rng, (B,), -8, 8), 0.5 * ints(rng, (B,), -8, 8)
    fs[0] = 0.0
    rs[0] = -0.0
    if B > 2:
        fs[2], rs[1] = -0.0, 0.0
    return dict(fs=fs, rs=rs, norm=1.0 + 0.5 * ints(rng, (B,), -2, 6))


def sgn(v):
    return np.sign(v)


def loss_ref(d, dt, order, with_norm=True, budget=None):
    """The six metric slots of bg_wgangp_d_loss, dfs, drs; the two of bg_wgan_g_loss and ds.  The sums are exact for every B;
    the divisions by B round unless B is a power of two."""
    d = cast(d, dt)
    fs, rs, B = d["fs"], d["rs"], d["fs"].size
    L = {k: dt(v) for k, v in LOSS.items()}
    dn = d["norm"] - dt(1)
    sn_terms = L["e_drift"] * (np.abs(fs) + np.abs(rs))
    if budget:
        budget.note(fs[:, None], 0.5, 0), budget.note(rs[:, None], 0.5, 0), budget.note(sn_terms[:, None], 2.0 ** -11, 0)
        budget.note((dn * dn)[:, None], 0.25, 0)
    sf, sr, sn = sum0(fs, order), sum0(rs, order), sum0(sn_terms, order)
    sg = sum0(dn * dn, order) if with_norm else dt(0)
    gp = sg / dt(B)
    met = np.array([sf / dt(B), sr / dt(B), (sf - sr) * L["inv_gbs"] + L["gp_coef"] * gp + sn / dt(B), L["gp_coef"] * gp, sn / dt(B), gp], dt)
    return dict(sums=np.array([sf, sr, sn, sg], dt), met=met, dfs=L["vec_scale"] * L["inv_gbs"] + L["e_drift"] * sgn(fs),
                drs=-L["vec_scale"] * L["inv_gbs"] + L["e_drift"] * sgn(rs),
                gmet=np.array([sf / dt(B), -sf * L["inv_gbs"]], dt), ds=np.full(B, -L["inv_gbs"], dt))


def is_pow2(n):
    return n & (n - 1) == 0


ADAM_N = [1, 257, 524289]


# ------------------------------------------------------------------ real-valued group: the bound of an output that rounds
def parity(got, ref64, ref32, rtol, atol, yardstick=3.0):
    """(max error, bound there, worst error / bound): the bound of an element is the larger of the bound tests/test_misc_gpu.py
    uses for the op (atol + rtol |ref|) and `yardstick` x the largest deviation of the same formula evaluated in numpy float32
    from its float64 evaluation (the YARDSTICK rule of tests/helpers.py).  The kernel's output does not enter the bound."""
    got, ref64 = np.asarray(got, np.float64).ravel(), np.asarray(ref64, np.float64).ravel()
    dev32 = float(np.abs(np.asarray(ref32, np.float64).ravel() - ref64).max())
    bound = np.maximum(np.maximum(atol + rtol * np.abs(ref64), yardstick * dev32), 1e-300)
    err = np.abs(got - ref64)
    err = np.where(np.isfinite(err), err, np.inf)
    i = int(np.argmax(err / bound))
    return float(err[i]), float(bound[i]), float(err[i] / bound[i])


BN_REAL_ALPHA = 0.3          # the LeakyReLU slope of the real-valued BatchNorm cases, passed to the kernel and to the reference alike


def bn_fwd_ref(sums, M_total, x, gamma, beta, mm, mv, dt, eps=1e-3, momentum=0.99, unbiased=True, alpha=BN_REAL_ALPHA):
    """bn_stats_final_kernel / bn_finalize_sums_kernel + bn_apply_kernel in dtype dt (misc.hip's expressions)."""
    C = gamma.size
    sums, x, gamma, beta, mm, mv = (np.asarray(a).astype(dt) for a in (sums, x, gamma, beta, mm, mv))
    mean = sums[:C] / dt(M_total)
    var = np.maximum(sums[C:] / dt(M_total) - mean * mean, dt(0))
    inv = dt(1) / np.sqrt(var + dt(eps))
    vu = var * (dt(M_total) / dt(max(M_total - 1, 1))) if unbiased else var
    y = lrelu(gamma * ((x - mean) * inv) + beta, alpha)
    return dict(y=y, save_mean=mean, save_inv=inv, moving_mean=mm * dt(momentum) + mean * (dt(1) - dt(momentum)),
                moving_var=mv * dt(momentum) + vu * (dt(1) - dt(momentum)))


# bounds of tests/test_misc_gpu.py (test_batchnorm_lrelu_fwd_bwd); save_inv has none of its own there: y is linear in it, so it
# takes the relative part of y's bound
BN_BOUNDS = dict(y=(1e-4, 2e-5), save_mean=(1e-5, 1e-6), moving_mean=(1e-5, 1e-6), moving_var=(1e-4, 1e-5), save_inv=(1e-4, 0.0))
