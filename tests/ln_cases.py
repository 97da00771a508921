"""Cases of the layer normalisation kernels (csrc/layernorm.hip) for tests/test_layernorm_exact_gpu.py: the routes restated, data on
which every output is exact in float32 whatever the order of the sums, hard inputs with a bound measured from the reference, and the
case table.  tests/test_ln_cases_cpu.py holds every claim made here without a GPU.

Exact recipe (eps = 2).  A row is m + pattern: m an integer in [-3, 3] per row, pattern a shuffled, sign-flipped concatenation of
blocks that each sum to 0 and have mean square v -- v = 2: (1, 1, -2), (2, -2, 0, 0), (2, -2, 1, -1, 0); v = 14: (1, 4, -5),
(6, -4, -2, 0), (7, -4, -2, -1, 0); every C >= 3 is 3a + 4b + 5c.  So mu = m, var = v, r = 1/2 or 1/4 and xh is a multiple of 1/4;
v alternates between neighbouring rows (a lane that takes its neighbour's mu or r is wrong by a factor).  g = 8 C * small integers
and zdot = C * small integers make every row mean an integer quotient; gamma in {+-1/2, +-1, +-2} (or 0), beta in {0, +-1/2, +-1}
(some pre-activations are exactly 0), alpha = 1/4, keep_scale = 2, keep bytes in {0, 1, 2, 0x80, 0xFF}.  Above C = 64 g and zdot
hold three nonzeros per row, at the seams of the route (mean(pc * qc) outgrows 24 bits otherwise); the centring makes the vectors
the kernels work on dense all the same.  C = 1 has variance 0 (eps = 1/4, r = 2); C = 2 takes (a, -a), a = +-1, eps = 3, r = 1/2;
rows of constants run in cases of their own with eps = 1/4."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
ALPHA, KEEP_SCALE = 0.25, 2.0
KEEP_BYTES = (0, 1, 2, 0x80, 0xFF)
K_T, K_WAVES, K_MAX_BLOCKS, K_CHUNK_UNITS = 256, 4, 1024, 64          # rowwise.h: kT, kWaves, kMaxBlocks, kChunkUnits


# ------------------------------------------------------------------ the routes, restated
def route_for(C):
    """rowwise.h route_for with aligned = true (the lines from ``t.vec = C % 4 == 0 && aligned ? 4 : 1`` to ``if (t.chunks > 1) t.nv = 1``)."""
    vec = 4 if C % 4 == 0 else 1
    U = C // vec
    lg = 0
    while (1 << lg) < U and lg < 6:
        lg += 1
    per = (U + 63) // 64
    nv = 1 if per <= 1 else 2 if per <= 2 else 4
    chunks = 1 if per <= 4 else (U + K_CHUNK_UNITS - 1) // K_CHUNK_UNITS
    if chunks > 1:
        nv = 1
    return dict(vec=vec, lanes=1 << lg, regs=nv, chunks=chunks)


def rows_per_workgroup(C):
    """grid_for's ``rows_wg = kWaves * (64 >> t.lg)`` (ROWWISE_POS_SETUP's rpw * kWaves)."""
    return K_WAVES * (64 // route_for(C)["lanes"])


def grid_for(R, C):
    """grid_for: (min(row groups, kMaxBlocks), chunks)."""
    w = rows_per_workgroup(C)
    return min(-(-R // w), K_MAX_BLOCKS), route_for(C)["chunks"]


def workspace_bytes(R, C):
    """bg_ln_workspace_bytes: ``grid_for(R, route_for(C)).x * 2 * C * sizeof(float)``; 0 for R or C <= 0."""
    return 0 if R <= 0 or C <= 0 else grid_for(R, C)[0] * 2 * C * 4


def finish_trips(nblk):
    """ln_finish_kernel for ``nblk`` partial rows -> (main-loop trips of lane 0 ... 63, whether each lane's tail runs): the loop
    ``for (; b + 7 * 64 < nblk; b += 8 * 64)`` from b = lane, then ``if (b < nblk)``."""
    main, tail = [], []
    for lane in range(64):
        b, n = lane, 0
        while b + 7 * 64 < nblk:
            b, n = b + 8 * 64, n + 1
        main.append(n)
        tail.append(b < nblk)
    return main, tail


def route_class(C):
    t = route_for(C)
    kind = "chunked" if t["chunks"] > 1 else "regs%d" % t["regs"] if t["regs"] > 1 else "subwave" if t["lanes"] < 64 else "wave"
    return ("float4" if t["vec"] == 4 else "scalar") + " " + kind


def position(C, row, c):
    """Where element (row, c) lives: dict(workgroup-visit, wave, lane, j = register, chunk)."""
    t = route_for(C)
    u = c // t["vec"]
    L = 64 if t["chunks"] > 1 else t["lanes"]
    rpw = 64 // t["lanes"]
    chunk, j = (u // 64, 0) if t["chunks"] > 1 else (0, u // L)
    return dict(visit=row // (rpw * K_WAVES), wave=(row // rpw) % K_WAVES, lane=(row % rpw) * t["lanes"] + u % L, j=j, chunk=chunk)


def seam_channels(C):
    """Channels at the seams of C's route: the first and last unit, both sides of every lane-register stride j * L and of every
    64-unit chunk, and the whole of a short last chunk."""
    t = route_for(C)
    vec, U = t["vec"], C // t["vec"]
    units = {0, U - 1}
    stride = 64 if t["chunks"] > 1 else t["lanes"]
    for k in range(stride, U, stride):
        units |= {k - 1, k}
    if t["chunks"] > 1 and U % 64:
        units |= set(range(U - U % 64, U))
    return np.array(sorted(u * vec + e for u in units for e in range(vec) if 0 <= u < U), np.int64)


# ------------------------------------------------------------------ exact data
_BLOCKS = {2: {3: (1, 1, -2), 4: (2, -2, 0, 0), 5: (2, -2, 1, -1, 0)}, 14: {3: (1, 4, -5), 4: (6, -4, -2, 0), 5: (7, -4, -2, -1, 0)}}


def _split(C):
    """C = 3a + 4b + 5c with the fewest blocks of 4 and 5."""
    for c5 in range(3):
        for b4 in range(3):
            rem = C - 4 * b4 - 5 * c5
            if rem >= 0 and rem % 3 == 0:
                return rem // 3, b4, c5
    raise ValueError(f"no blocks for C={C}")


def _patterns(R, C, rng):
    """[R, C]: row i a shuffled, sign-flipped concatenation of blocks with mean square 2 (i even) or 14 (i odd)."""
    a3, b4, c5 = _split(C)
    lens = np.array([3] * a3 + [4] * b4 + [5] * c5)
    base = {v: np.concatenate([_BLOCKS[v][k] for k in lens]).astype(F64) for v in (2, 14)}
    out = np.where((np.arange(R) % 2 == 0)[:, None], base[2][None, :], base[14][None, :])
    out = out * np.repeat(rng.choice([-1.0, 1.0], size=(R, lens.size)), lens, axis=1)
    return rng.permuted(out, axis=1)


def _sparse_pair(R, C, rng, gvals, qvals):
    """Two [R, C] arrays with three nonzeros per row each, at seam channels of the route, another set per row; the two sets of a row
    are disjoint wherever the route has six seam channels (a shared channel puts 16 C * 2 C quanta into mean(pc * qc): past 2^24 from
    C = 725 on)."""
    seams = seam_channels(C)
    pick = rng.permuted(np.tile(seams, (R, 1)), axis=1)
    second = pick[:, 3:6] if seams.size >= 6 else rng.permuted(np.tile(seams, (R, 1)), axis=1)[:, :3]
    out = np.zeros((2, R, C))
    out[0][np.arange(R)[:, None], pick[:, :3]] = rng.choice(gvals, size=(R, 3))
    out[1][np.arange(R)[:, None], second] = rng.choice(qvals, size=(R, 3))
    return out


def exact_data(case):
    """Inputs of an exact case, float64 arrays holding float32 values: z, gamma, beta, g, zdot, addend, keep (uint8), old [2, C]."""
    R, C = case["R"], case["C"]
    rng = np.random.default_rng(case["seed"])
    m = rng.integers(-3, 4, size=(R, 1)).astype(F64)
    if case["kind"] == "const" or C == 1:
        z, eps = m + np.zeros((R, C)), 0.25
    elif C == 2:
        z, eps = m + rng.choice([-1.0, 1.0], size=(R, 1)) * np.array([[1.0, -1.0]]), 3.0
    else:
        z, eps = m + _patterns(R, C, rng), 2.0
    gamma = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=C)
    beta = rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], size=C)
    forced = ()
    if "beta_all" in case:                              # C = 1: the one pre-activation is beta
        beta[:] = case["beta_all"]
    elif C >= 3 and case["kind"] == "exact":
        # row 0 (v = 2, xh in {0, +-1/2, +-1}) holds a pre-activation of exactly 0, one above and one below, whatever was drawn
        xh0 = (z[0] - m[0]) * 0.5
        forced = c0, c1, c2 = rng.permutation(C)[:3]
        gamma[c0] = rng.choice([-1.0, 1.0])
        beta[c0] = -gamma[c0] * xh0[c0] + 0.0
        gamma[c1], beta[c1] = (2.0 if xh0[c1] >= 0 else -2.0), 0.5
        gamma[c2], beta[c2] = (-2.0 if xh0[c2] >= 0 else 2.0), -0.5
    elif C == 2:
        gamma[:], beta[:] = (1.0, 2.0), (-0.5, 0.5)
    elif case["kind"] == "const":
        beta[:3] = (0.0, 0.5, -1.0)
    if case.get("gamma0"):                              # the last channel that the kink's three do not hold, and the first
        free = [c for c in range(C) if c not in forced]
        gamma[[free[0], free[-1]]] = 0.0
    gmax, ints = case.get("gmax", 2), lambda lo, hi: rng.integers(lo, hi + 1, size=(R, C)).astype(F64)
    if C > 64:
        g, zdot = _sparse_pair(R, C, rng, [-2.0, -1.0, 1.0, 2.0][2 - gmax:2 + gmax], [-2.0, -1.0, 1.0, 2.0])
        g, zdot = 8 * C * g * (rng.uniform(size=(R, 1)) < case.get("density", 1.0)), C * zdot      # density: the rows that carry a g at all
    else:
        live = rng.uniform(size=(R, C)) < case.get("density", 1.0)
        g = 8 * C * ints(-gmax, gmax) * live
        zdot = C * ints(-2, 2) * (rng.uniform(size=(R, C)) < case.get("density", 1.0))
    keep = rng.choice(np.array(KEEP_BYTES, np.uint8), size=R * C)
    i = np.arange(min(20, R * C))
    keep[i] = np.array(KEEP_BYTES, np.uint8)[(i // 4 + i % 4) % 5]      # each value in each byte lane of a uint32, from the start
    return dict(z=z, gamma=gamma, beta=beta, g=g, zdot=zdot, addend=ints(-4, 4), keep=keep.reshape(R, C), eps=eps,
                old=rng.integers(-8, 9, size=(2, C)).astype(F64))


# ------------------------------------------------------------------ hard inputs (bounded, not exact)
HARD_EPS, HARD_ALPHA, HARD_SCALE = 1e-3, 0.3, 1.0 / 0.7
HARD_KINDS = ("offset", "wide", "spike")


def hard_data(case):
    """Rows by turns offset + N(0, 1), 1e4 * N(0, 1) and (once) all zero but a single 1e4.  |beta| = 8 keeps every pre-activation
    away from the kink (asserted by the CPU test), so float32 and float64 take the same LeakyReLU branch."""
    R, C = case["R"], case["C"]
    rng = np.random.default_rng(case["seed"])
    f32 = lambda a: np.asarray(a).astype(F32).astype(F64)
    kind = np.arange(R) % 2
    z = np.where((kind == 0)[:, None], case["offset"] + rng.normal(size=(R, C)), 1e4 * rng.normal(size=(R, C)))
    if R >= 3:
        kind[R // 2] = 2
        z[R // 2] = 0.0
        z[R // 2, rng.integers(C)] = 1e4
    return dict(z=f32(z), gamma=f32(1 + 0.2 * rng.uniform(size=C)), beta=f32(rng.choice([-8.0, 8.0], size=C)),
                g=f32(rng.normal(size=(R, C))), zdot=f32(rng.normal(size=(R, C))), addend=f32(rng.normal(size=(R, C))),
                keep=(rng.uniform(size=(R, C)) >= 0.3).astype(np.uint8), old=f32(rng.normal(size=(2, C))), eps=HARD_EPS, row_kind=kind)


# ------------------------------------------------------------------ the formulas, in one number format
class Eval:
    """The four entry points' formulas on inputs ``d``, every operation in ``dt``; float32 sums run sequentially (np.cumsum), from
    the front or (``rev``) from the back; ``pairwise`` takes numpy's own float32 sum instead (the hard inputs' yardstick)."""

    def __init__(self, d, dt=F64, rev=False, pairwise=False):
        self.d, self.dt, self.rev, self.pairwise = d, dt, rev, pairwise
        c = lambda k: d[k].astype(dt)
        self.z, self.gamma, self.beta, self.g, self.zdot = c("z"), c("gamma"), c("beta"), c("g"), c("zdot")
        self.Cf = dt(self.z.shape[1])
        self.mu = self.rows(self.z) / self.Cf
        dz = self.z - self.mu
        self.r = dt(1) / np.sqrt(self.rows(dz * dz) / self.Cf + dt(d["eps"]))
        self.xh = dz * self.r
        self.n = self.gamma * self.xh + self.beta

    def _sum(self, x, axis):
        if self.dt is F64 or self.pairwise:
            return x.sum(axis, keepdims=True, dtype=self.dt)
        x = np.flip(x, axis) if self.rev else x
        return np.take(np.cumsum(x, axis=axis, dtype=F32), [-1], axis=axis)

    def rows(self, x):
        return self._sum(x, 1)

    def cols(self, x):
        return self._sum(x, 0)[0] if x.shape[0] else np.zeros(x.shape[1], self.dt)

    def factor(self, alpha, keep_rows):
        dt = self.dt
        f = np.where(self.n > 0, dt(1), dt(alpha)).astype(dt)
        if keep_rows:
            k = self.d["keep"][:keep_rows] != 0
            f[:keep_rows] = np.where(k, f[:keep_rows] * dt(self.d.get("scale", KEEP_SCALE)), dt(0))
        return f

    def M(self, y):
        yc = y - self.rows(y) / self.Cf
        return self.r * (yc - self.xh * (self.rows(yc * self.xh) / self.Cf))

    def fwd(self, alpha, keep_rows):
        dt = self.dt
        y = np.where(self.n > 0, self.n, dt(alpha) * self.n)
        if keep_rows:
            k = self.d["keep"][:keep_rows] != 0
            y[:keep_rows] = np.where(k, y[:keep_rows] * dt(self.d.get("scale", KEEP_SCALE)), dt(0))
        return dict(a=y, mu=self.mu[:, 0], r=self.r[:, 0])

    def bwd(self, alpha, keep_rows, addend=False, dw_rows=0, acc_beta=0.0, acc_scale=1.0):
        dt = self.dt
        u = self.g * self.factor(alpha, keep_rows)
        dz = self.M(self.gamma * u)
        if addend:
            dz = dz + self.d["addend"].astype(dt)
        dw = dw_rows or u.shape[0]
        old = self.d["old"].astype(dt)
        first = lambda k: dt(acc_beta) * old[k] if acc_beta else dt(0)
        return dict(dz=dz, u=u, dgamma=first(0) + dt(acc_scale) * self.cols((u * self.xh)[:dw]), dbeta=first(1) + dt(acc_scale) * self.cols(u[:dw]))

    def tangent(self, alpha):
        return dict(v=(self.factor(alpha, 0) * self.gamma) * self.M(self.zdot))

    def source(self, alpha, acc_beta=0.0, acc_scale=1.0):
        dt = self.dt
        u = self.g * self.factor(alpha, 0)
        p = self.gamma * u
        pc, qc = p - self.rows(p) / self.Cf, self.zdot - self.rows(self.zdot) / self.Cf
        A, Bq, D = (self.rows(x) / self.Cf for x in (pc * self.xh, qc * self.xh, pc * qc))
        s = -(self.r * self.r) * (pc * Bq + qc * A + self.xh * (D - dt(3) * A * Bq))
        col = self.cols(u * (self.r * (qc - self.xh * Bq)))
        old = self.d["old"].astype(dt)
        return dict(s=s, u=u, dgamma=(dt(acc_beta) * old[0] if acc_beta else dt(0)) + dt(acc_scale) * col)


def variants(case):
    """What the GPU test runs of a case and compares exactly: (name, Eval method, arguments)."""
    R, kr, dw = case["R"], case["keep_rows"], case["dw_rows"]
    return [("fwd no mask", "fwd", (ALPHA, 0)), ("fwd full mask", "fwd", (ALPHA, R)), ("fwd mask on first rows", "fwd", (ALPHA, kr)),
            ("fwd alpha 0", "fwd", (0.0, kr)), ("fwd alpha 1", "fwd", (1.0, kr)),
            ("bwd no sums", "bwd", (1.0, 0)), ("bwd sums into NaN", "bwd", (ALPHA, kr, True, dw, 0.0, 1.0)),
            ("bwd sums onto integers", "bwd", (ALPHA, kr, True, dw, 1.0, 0.5)), ("bwd dz over addend", "bwd", (0.0, R, True)),
            ("tangent", "tangent", (ALPHA,)), ("tangent in place", "tangent", (0.0,)),
            ("source into NaN", "source", (ALPHA, 0.0, 1.0)), ("source onto integers", "source", (ALPHA, 1.0, 1.0))]


def magnitude_quanta(terms, axis):
    """Sum of |terms| along ``axis`` in units of the terms' common quantum (the largest power of two dividing them all): below
    2^24 every partial sum, in ANY order, is a float32, so the sum is exact whatever tree adds it."""
    t = np.abs(np.asarray(terms, F64))
    nz = t[t != 0]
    if not nz.size:
        return 0.0
    q = 2.0 ** np.floor(np.log2(nz.min()))
    while not np.array_equal(np.round(nz / q), nz / q):
        q /= 2
    return float((t / q).sum(axis).max())


# ------------------------------------------------------------------ the case table
FLOAT4_C = (4, 8, 12, 16, 20, 32, 64, 128, 252, 256, 260, 512, 516, 1024, 1028, 1280)
SCALAR_C = (1, 2, 3, 5, 7, 17, 33, 63, 65, 127, 129, 255, 257, 319)
R_KINDS = ("1", "w-1", "w", "w+1", "2w+3")
STRIDE_C = {"float4 subwave": 16, "float4 regs4": 1024, "float4 chunked": 1028, "scalar subwave": 5, "scalar chunked": 257}
ALL_R_C = (20, 1024, 1028, 5, 255, 257)             # every row-count cell on one C per route class (and both 4-register routes)
NBLK = (1, 63, 64, 65, 448, 449, 511, 512, 513, 1024)
NBLK_C = 4
SEAMS = ("inside a wave", "wave seam", "workgroup seam")


def _r_of(kind, w):
    return {"1": 1, "w-1": max(w - 1, 1), "w": w, "w+1": w + 1, "2w+3": 2 * w + 3}[kind]


def _case(C, R, cells, kind="exact", **kw):
    c = dict(C=C, R=R, kind=kind, seed=100003 * C + R + (7 if kind == "const" else 0), cells=list(cells), ops=("fwd", "bwd", "tangent", "source"),
             keep_rows=max(R // 2, 1), dw_rows=max(R - R // 3, 1), u_lo=R // 4, u_hi=R, offset=0)
    c.update(kw)
    return c


def _table():
    out = []
    for i, C in enumerate(FLOAT4_C + SCALAR_C):
        w = rows_per_workgroup(C)
        kinds = R_KINDS if C in ALL_R_C else (R_KINDS[i % 5],)
        if C == 2:
            kinds = ("2w+3",)                       # both signs of a, so the kink has both sides
        for k in kinds:
            extra = {}
            if C == 1:
                extra["beta_all"] = 0.5
            out.append(_case(C, _r_of(k, w), [("C", C), ("R", k)], **extra))
    # C = 1: n = beta on every row, so the three sides of the kink take three cases
    out.append(_case(1, 3, [("C", 1)], beta_all=0.0))
    out.append(_case(1, 5, [("C", 1)], beta_all=-1.0))
    # gamma = 0 on two channels (the last one among them), and the misaligned views of the scalar routes
    for C in (16, 1028, 5, 257):
        out.append(_case(C, rows_per_workgroup(C) + 2, [("gamma 0", route_class(C))], gamma0=True, offset=0 if C % 4 == 0 else 1))
    out.append(_case(255, 7, [("offset 1", route_class(255))], offset=1))
    # rows of constants, one per route class
    for C in sorted(STRIDE_C.values()):
        out.append(_case(C, rows_per_workgroup(C) + 1, [("constant rows", route_class(C))], kind="const"))
    # more row groups than the grid holds workgroups
    for cls, C in STRIDE_C.items():
        out.append(_case(C, 1025 * rows_per_workgroup(C) + 5, [("grid stride", cls)], gmax=1, density=0.25 if C <= 64 else 0.1))
    # ln_finish_kernel's loop shapes, through bwd (NQ = 2) and gp_source (NQ = 1)
    for n in NBLK:
        out.append(_case(NBLK_C, n * rows_per_workgroup(NBLK_C), [("nblk", n, "bwd"), ("nblk", n, "source")], ops=("bwd", "source"), gmax=1,
                         density=0.25, keep_rows=0, dw_rows=n * rows_per_workgroup(NBLK_C)))      # every partial row holds a sum
    # the three windows, each ending inside a wave's rows, at a wave seam and at a workgroup seam, chosen independently
    for C in (16, 5):
        w = rows_per_workgroup(C)
        rpw, R = w // 4, 2 * w + 3
        ends = {"inside a wave": w + rpw + 3, "wave seam": w + 2 * rpw, "workgroup seam": w}
        for shift in range(3):
            ks, ds, us = SEAMS[shift], SEAMS[(shift + 1) % 3], SEAMS[(shift + 2) % 3]
            out.append(_case(C, R, [("window", "keep", ks), ("window", "dw", ds), ("window", "u", us)], keep_rows=ends[ks], dw_rows=ends[ds],
                             u_lo=3, u_hi=ends[us], seed=31 * C + shift, ops=("fwd", "bwd")))
        out.append(_case(C, R, [("window", "u", "one row, row0 > 0")], u_lo=w + 1, u_hi=w + 2, ops=("bwd",)))
        out.append(_case(C, R, [("window", "u", "ends at R")], u_lo=R - 2, u_hi=R, ops=("bwd",)))
    return out


CASES = _table()


def case_id(c):
    extra = "".join(f" {k}" for k in ("gamma0",) if c.get(k)) + (" off1" if c["offset"] else "") + (" const" if c["kind"] == "const" else "")
    win = f" k{c['keep_rows']} d{c['dw_rows']} u{c['u_lo']}-{c['u_hi']}" if any(x[0] == "window" for x in c["cells"]) else ""
    beta = f" beta{c['beta_all']:g}" if "beta_all" in c else ""
    return f"C{c['C']} R{c['R']}{extra}{win}{beta}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)

CELLS = ({("C", C) for C in FLOAT4_C + SCALAR_C} | {("R", k) for k in R_KINDS} | {("grid stride", k) for k in STRIDE_C}
         | {("nblk", n, op) for n in NBLK for op in ("bwd", "source")} | {("window", wn, s) for wn in ("keep", "dw", "u") for s in SEAMS}
         | {("window", "u", "one row, row0 > 0"), ("window", "u", "ends at R")}
         | {("gamma 0", route_class(C)) for C in (16, 1028, 5, 257)} | {("offset 1", route_class(255))}
         | {("constant rows", k) for k in STRIDE_C})

# one C per route class: a NaN row, two runs into different buffers, the hard inputs
CLASS_C = tuple(sorted(STRIDE_C.values()))
HARD_OFFSET = 4096.0
HARD_CASES = [dict(C=C, R=2 * rows_per_workgroup(C) + 3, seed=977 * C, offset=HARD_OFFSET, keep_rows=rows_per_workgroup(C) + 1,
                   dw_rows=2 * rows_per_workgroup(C)) for C in CLASS_C]


def hard_runs(case):
    """What the GPU test runs of a hard case: {name: (Eval method, arguments)}."""
    kr, dw = case["keep_rows"], case["dw_rows"]
    return {"fwd": ("fwd", (HARD_ALPHA, kr)), "bwd": ("bwd", (HARD_ALPHA, kr, True, dw, 1.0, 0.5)), "tangent": ("tangent", (HARD_ALPHA,)),
            "source": ("source", (HARD_ALPHA, 1.0, 1.0))}


_OLD_BOUND = {"a": (1e-4, "2e-5"), "mu": (1e-4, "2e-5"), "r": (1e-4, "2e-5"), "u": (1e-4, "2e-5"), "dz": (2e-4, "wide"), "v": (2e-4, "wide"),
              "s": (2e-4, "wide"), "dgamma": (2e-4, "sums"), "dbeta": (2e-4, "sums")}


@functools.lru_cache(maxsize=None)
def _hard(C, R, seed, offset, keep_rows, dw_rows):
    case = dict(C=C, R=R, seed=seed, offset=offset, keep_rows=keep_rows, dw_rows=dw_rows)
    d = dict(hard_data(case), scale=HARD_SCALE)
    e64, e32 = Eval(d), Eval(d, F32, pairwise=True)
    kind, out = d["row_kind"], {}
    for name, (op, args) in hard_runs(case).items():
        want, got = getattr(e64, op)(*args), getattr(e32, op)(*args)
        for k, w in want.items():
            if name == "source" and k == "u":
                continue
            rtol, how = _OLD_BOUND[k]
            atol = {"2e-5": 2e-5, "wide": 2e-5 * max(1.0, float(np.abs(w).max())), "sums": 2e-4 * np.sqrt(R)}[how]
            dev = np.abs(got[k].astype(F64) - w)
            if how == "sums":                       # a column sum mixes the kinds of rows: one deviation and one scale per output
                dev3, scale = np.full(w.shape, 3 * dev.max()), np.full(w.shape, np.abs(w).max())
            else:
                rows = dev.reshape(R, -1).max(1), np.abs(w).reshape(R, -1).max(1)
                per = [np.zeros(R), np.zeros(R)]
                for kd in range(3):
                    for p, x in zip(per, rows):
                        p[kind == kd] = x[kind == kd].max()
                dev3, scale = (np.broadcast_to(p.reshape((R,) + (1,) * (w.ndim - 1)), w.shape) for p in (3 * per[0], per[1]))
            out[f"{name} {k}"] = (w, np.maximum(atol + rtol * np.abs(w), dev3), atol + rtol * scale, dev3, scale)
    return dict(data=d, eval=e64, out=out)


def hard_reference(case):
    """data, the float64 Eval and {"<run> <output>": (float64 reference, elementwise bound, the old bound at the scale of the rows'
    kind, 3 x the float32 deviation of the rows' kind, that scale)}.  The bound is max(atol + rtol |ref| of tests/test_layernorm_gpu.py,
    3 x the deviation from float64 of a float32 numpy two-pass evaluation): measured from the reference, never from the kernel."""
    return _hard(*(case[k] for k in ("C", "R", "seed", "offset", "keep_rows", "dw_rows")))


@functools.lru_cache(maxsize=2)
def _cached(i):
    c = CASES[i]
    d = exact_data(c)
    return d, Eval(d)


def reference(i):
    """(inputs, float64 Eval) of CASES[i]; the last two stay in memory."""
    return _cached(i)
