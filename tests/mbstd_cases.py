"""The case list of the MinibatchStdDev kernel tests (a helper, not a test file): shapes, groups and data.

A case is (name, G, groups, P, C): N = G * groups samples of P pixels and C channels.  tests/test_mbstd_cpu.py checks, from
bg_mbstd_plan alone, that the list reaches every route, lane trip count and head / tail combination of each of the three calls;
tests/test_mbstd_gpu.py runs every case, once with all views 16-byte aligned and once with all of them one float off."""
import numpy as np

EPS = 1e-8
OFFSETS = (0, 1)            # floats past a 16-byte boundary of every view of a run
RESIDENT_FLOATS = 15356     # include/bgan.h: the largest group that waits in LDS

CASES = [
    # the tops of the stock critics
    ("tiny_mnist_top", 2, 2, 9, 8),         # stride 9
    ("tiny_top", 2, 3, 4, 32),
    ("tiny_top_g4", 4, 1, 4, 32),
    ("celeba_top", 4, 2, 4, 512),
    ("mnist_top", 2, 1, 49, 128),
    ("mnist_top_g3", 3, 2, 49, 128),        # 18816 floats: the largest stock top at G = 3 leaves the resident route
    # the smallest maps
    ("one", 2, 3, 1, 1),
    ("one_g3", 3, 1, 1, 1),
    ("five", 4, 2, 1, 5),
    ("five_g3", 3, 3, 1, 5),
    # the last resident group size and the first that is not (G * P * C = 15356, 15360)
    ("resident_last", 2, 2, 11, 698),
    ("resident_first_out", 2, 2, 10, 768),
    # the two-launch route: one column cut (fewer than two float4s of columns), two even cuts, three ragged ones
    ("cut_one", 2200, 1, 1, 7),
    ("cut_two", 4, 2, 4, 1024),
    ("cut_ragged", 3, 2, 7, 911),
    # more groups than the MAX_BLOCKS workgroups of a grid: three workgroups take a second group and reuse their LDS image (resident
    # route); through the G = 2 branch with scalar columns (groups of 24 bytes: every other one's image sits 8 bytes into its LDS
    # slot), and through the general one with float4 columns
    ("second_trip", 2, 1027, 1, 3),
    ("second_trip_g3", 3, 1026, 1, 8),
    # GE = 524320 floats: ceil(GE / CUT_FLOATS) = 65, so the cap of MAX_CUTS holds for the columns; Ly = 524328 does the same for the emit
    ("cut_capped", 2, 1, 4, 65540),
]
MAX_BLOCKS, CUT_FLOATS, MAX_CUTS = 1024, 8192, 64      # csrc/mbstd.hip: kMaxBlocks, kCutFloats, kMaxCuts


def case(name):
    return next(c for c in CASES if c[0] == name)


def data(G, groups, P, C, seed):
    """x [N, P, C], u [N, P, C + 1], d [N, P, C] in float64, exactly representable in float32.  Every column of x is a per-column
    mean plus a zero-mean pattern over the group's members scaled to a standard deviation in [0.5, 2]: conditioning is not in
    question."""
    rng = np.random.default_rng(seed)
    N, E = G * groups, P * C
    pat = rng.normal(size=(groups, G, E))
    pat -= pat.mean(1, keepdims=True)
    pat /= np.sqrt((pat ** 2).mean(1, keepdims=True))
    mean = rng.uniform(-2, 2, size=(groups, 1, E))
    sd = rng.uniform(0.5, 2.0, size=(groups, 1, E))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = f32((mean + sd * pat).reshape(N, P, C))
    return x, f32(rng.normal(size=(N, P, C + 1))), f32(rng.normal(size=(N, P, C)))


def exact_data(groups, P, C, seed):
    """G = 2, integer data a +- k with k in {1, 2, 3}: mu = a and s = k exactly in float32 (sqrt(float32(k^2) + 1e-8) == k), f_g a
    sum of small integers over a power of two."""
    assert (P * C) & (P * C - 1) == 0
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, size=(groups, 1, P * C)).astype(np.float64)
    k = rng.integers(1, 4, size=(groups, 1, P * C)).astype(np.float64)
    sign = np.where(rng.integers(0, 2, size=(groups, 1, P * C)) > 0, 1.0, -1.0)
    x = np.concatenate([a + sign * k, a - sign * k], 1).reshape(2 * groups, P, C)
    return x, k.reshape(groups, P, C)
