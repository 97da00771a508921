"""The case list of the NoiseInjection kernel tests (a helper, not a test file): (name, R, C), chosen where the kernels of
csrc/noise.hip can go wrong, not by the workload.  tests/test_noise_cpu.py proves from bg_noise_route alone what the list reaches;
tests/test_noise_gpu.py runs every case with the matrices 16-byte aligned and one float off, y aliasing x and not, alpha 1 and 0.2.

Routes (csrc/rowwise.h): units of one float4 (C % 4 == 0, aligned views) or one float; up to 64 units a power of two of lanes shares
a row with one unit each, up to 128 / 256 units a wave holds a row with 2 / 4 units per lane, beyond that a row is cut into chunks of
64 units along the grid's second axis.  A workgroup visits 4 * 64 / lanes rows at a time, in a grid-stride loop over at most 1024
workgroups."""
import numpy as np

OFFSETS = (0, 1)            # floats past a 16-byte boundary
ALPHAS = (1.0, 0.2)
MAX_BLOCKS = 1024

CASES = [
    # the issue's channel counts at its row counts
    ("c1_r1", 1, 1), ("c1_r7", 7, 1), ("c3_r1", 1, 3), ("c3_r7", 7, 3), ("c4_r1", 1, 4), ("c4_r7", 7, 4), ("c8_r1", 1, 8), ("c8_r7", 7, 8),
    ("c64_r1", 1, 64), ("c64_r7", 7, 64),
    # one more than a workgroup's rows per visit: 256 at C = 1 and C = 4 (64 by single floats), 128 at C = 8, 16 at C = 64, 64 at C = 3
    ("c1_r257", 257, 1), ("c3_r65", 65, 3), ("c4_r257", 257, 4), ("c4_r65", 65, 4), ("c8_r129", 129, 8), ("c64_r17", 17, 64),
    # the stock generator's maps at batch 4 ("tiny": 2x2x32, 4x4x16, 8x8x16) and a celeba64 map
    ("tiny_32", 16, 32), ("tiny_16", 256, 16), ("celeba_512", 64, 512),
    # float4 units: two per lane (512), four (1024), chunked (1028: a ragged fifth chunk; 2048: whole chunks)
    ("c512_r5", 5, 512), ("c1024_r5", 5, 1024), ("c1028_r3", 3, 1028), ("c2048_r2", 2, 2048),
    # single floats: two per lane (100), four (250), chunked (258: a ragged fifth chunk)
    ("c100_r5", 5, 100), ("c250_r5", 5, 250), ("c258_r3", 3, 258),
    # the grid-stride loop's second trip at C = 4 (on either width)
    ("second_trip", MAX_BLOCKS * 256 + 1, 4),
]


def case(name):
    return next(c for c in CASES if c[0] == name)


def integer_data(R, C, seed):
    """(x or dz [R, C], noise [R]) float64 holding integers in [-3, 3]: every product and every partial sum of the gradient is exact
    in float32 whatever the order (|sum| <= 9 * R * C < 2^24 for every case of the list)."""
    rng = np.random.default_rng(seed)
    assert 9 * R * C < 1 << 24
    return rng.integers(-3, 4, size=(R, C)).astype(np.float64), rng.integers(-3, 4, size=R).astype(np.float64)


def normal_data(R, C, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(R, C)), rng.normal(size=R)
