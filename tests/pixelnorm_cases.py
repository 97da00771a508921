"""The case list of the PixelNormalization kernel tests (a helper, not a test file): (name, R, C, lrelu_alpha), chosen where the
kernels of csrc/pixelnorm.hip can go wrong, not by the workload.  tests/test_pixelnorm_cpu.py proves from bg_pixelnorm_route alone
what the list reaches; tests/test_pixelnorm_gpu.py runs every case with all views 16-byte aligned and one float off.

Routes (csrc/pixelnorm.hip): units of one float4 (C % 4 == 0, aligned views) or one float; up to 64 units a power of two of lanes
shares a row with one unit each, up to 128 / 256 units a wave holds a row with 2 / 4 units per lane, beyond that the row is swept in
chunks of 64 units.  A workgroup visits 4 * 64 / lanes rows at a time, in a grid-stride loop over at most 1024 workgroups."""
import numpy as np

EPS = 1e-8
OFFSETS = (0, 1)            # floats past a 16-byte boundary
MAX_BLOCKS, WAVES = 1024, 4

CASES = [
    # the stock generators' shapes at batch 4: latents (100, 10, 6), maps
    ("latent_100", 4, 100, 1.0), ("latent_10", 4, 10, 1.0), ("latent_6", 5, 6, 1.0),
    ("map_32", 16, 32, 0.3), ("map_16", 64, 16, 0.3), ("map_512", 64, 512, 0.3), ("map_64", 8, 64, 0.3), ("map_8", 8, 8, 0.3),
    # small channel counts
    ("c1", 7, 1, 0.2), ("c2", 7, 2, 1.0), ("c3", 7, 3, 0.0), ("c4", 7, 4, 0.2), ("c5", 7, 5, 1.0),
    # float4 units: the first and the last C of one unit per lane (4, 256), of two (260, 512), of four (516, 1024), the first chunked
    ("c252", 5, 252, 0.2), ("c256", 5, 256, 1.0), ("c260", 5, 260, 0.0), ("c512", 5, 512, 0.2), ("c516", 5, 516, 1.0),
    ("c1024", 5, 1024, 0.2), ("c1028", 5, 1028, 0.0), ("c1284", 3, 1284, 0.2), ("c2048", 2, 2048, 1.0),
    # single floats: the last C of one unit per lane (63), two (65, 127), four (129, 255), chunked (257 ...), ragged last chunks
    ("c63", 5, 63, 0.0), ("c65", 5, 65, 0.2), ("c127", 5, 127, 1.0), ("c129", 5, 129, 0.2), ("c255", 5, 255, 0.0),
    ("c257", 3, 257, 0.2), ("c911", 3, 911, 1.0), ("c2050", 2, 2050, 0.0),
    # rows: one, one short of and one past a workgroup's rows per visit (32 at C = 32, 256 at C = 4), a second grid-stride trip
    ("r1", 1, 32, 0.2), ("r31", 31, 32, 0.2), ("r33", 33, 32, 0.0), ("r255", 255, 4, 1.0), ("r257", 257, 4, 0.2),
    ("second_trip", MAX_BLOCKS * 256 + 257, 4, 0.2),
]


def case(name):
    return next(c for c in CASES if c[0] == name)


def data(R, C, seed):
    """(x, g) [R, C] float64 holding multiples of 1 / 16 in [-2, 2] without zeros: exactly representable in float32."""
    rng = np.random.default_rng(seed)
    draw = lambda: rng.integers(1, 33, size=(R, C)) * rng.choice([-1.0, 1.0], size=(R, C)) / 16.0
    return draw(), draw()


def zero_rows(alpha=0.25):
    """The exact case of the branch rule at 0: rows with zeros (of either sign) whose mean(a^2) = 4 exactly, so that r = 0.5 (the
    epsilon vanishes in float32: 4 + 1e-8 == 4) and every product of either formula is exact.  (x, g, y, r, dz) in float64."""
    x = np.array([[0.0, 4.0, -0.0, 0.0], [-4.0 / alpha, 0.0, 0.0, -0.0], [2.0, 2.0, -2.0 / alpha, 2.0]])
    g = np.array([[3.0, -2.0, 5.0, 1.0], [4.0, 6.0, -8.0, 2.0], [1.0, 2.0, 3.0, 4.0]])
    a = np.where(x > 0, x, alpha * x)
    assert ((a * a).mean(1) == 4.0).all()
    y = a * 0.5
    m = (g * y).mean(1)
    dz = np.where(y > 0, 1.0, alpha) * (0.5 * (g - y * m[:, None]))
    return x, g, y, np.full(3, 0.5), dz
