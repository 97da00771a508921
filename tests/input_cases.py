"""The case list of the uint8 input pipeline's kernel tests (a helper, not a test file): geometries, index vectors and mirror flags
chosen where the kernels of csrc/input.hip and the dense u8_normalize_resize_kernel of csrc/misc.hip can go wrong, not by the workload.

A case is (name, N, B, (Hs, Ws), (Hd, Wd), C, idx, flip): N source images of Hs x Ws x C bytes, B output samples of Hd x Wd x C floats,
sample b the image idx[b], mirrored left-right where flip[b] != 0.  tests/test_input_cases_cpu.py proves from arithmetic on the list
alone what it reaches; tests/test_input_routes_gpu.py runs every case in guarded buffers against the float64 oracle.

The launch (csrc/input.hip): THREADS lanes per workgroup, at most MAX_BLOCKS workgroups in a grid-stride loop.  For C = 1, 3, 4 a lane
takes a GROUP of four consecutive pixels of the batch's flat sequence q = (b * Hd + y) * Wd + x, stepping from pixel to pixel (over
row ends and sample ends), and the n_pix % 4 pixels left over are a scalar tail; for any other C a lane takes one pixel.  The dense
kernel takes one output float per lane under the same cap."""
import numpy as np

THREADS = 256               # csrc/input.hip and csrc/misc.hip: constexpr int kT = 256
MAX_BLOCKS = 2048           # grid_for of either file: 256 * 8
VEC_C = (1, 3, 4)           # channel counts of the four-pixels-per-thread kernel
CAPACITY = THREADS * MAX_BLOCKS         # units (groups, pixels, floats) one trip of the grid-stride loop covers: 524288
YARDSTICK_CAP = 2e-6        # tests/test_misc_gpu.py's atol of the dense kernel: no geometry here may need a wider yardstick

# one set per channel count of the four-pixel kernel: (suffix, N, B, source, output, idx, flip)
_PER_C = [
    # 9/5 and 11/7: a non-dyadic downscale; 105 pixels (tail 1), P = 35: group 8 ends in sample 1 (image 3 mirrored | image 0 not)
    ("down", 4, 3, (9, 11), (5, 7), [3, 0, 3], [1, 0, 1]),
    # 5/7 and 4/10: an upscale whose first row / column lies at a negative position and whose last has its upper tap clamped;
    # 350 pixels (tail 2), P = 70, B > N, a repeated index next to a different one
    ("up", 3, 5, (5, 4), (7, 10), [2, 0, 0, 1, 2], [1, 0, 1, 1, 0]),
    # 75 pixels (tail 3), P = 15
    ("tail3", 2, 5, (6, 6), (3, 5), [1, 0, 0, 1, 1], [0, 1, 0, 0, 1]),
    # rows up, columns down; 108 pixels (no tail), P = 27: the groups still cross rows and samples
    ("tail0", 3, 4, (4, 7), (9, 3), [0, 2, 1, 2], [1, 0, 0, 1]),
]
# fewer than four pixels in the whole batch: no group, the tail alone (three samples of one pixel; one sample of three; two of one)
_FEW = {1: (2, 3, (3, 3), (1, 1), [1, 0, 1], [1, 0, 1]), 3: (2, 1, (2, 2), (1, 3), [1], [1]), 4: (2, 2, (2, 3), (1, 1), [1, 0], [0, 1])}

_TRIP_IDX = [2, 0, 0, 1, 2, 1, 1, 0, 2, 0, 1]       # all six (image, flag) pairs with the flags below
_TRIP_FLIP = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0]

CASES = (
    [(f"c{C}_{s}", N, B, src, dst, C, idx, flip) for C in VEC_C for s, N, B, src, dst, idx, flip in _PER_C]
    + [(f"c{C}_few", *_FEW[C][:4], C, *_FEW[C][4:]) for C in VEC_C]
    + [
        # the one-pixel-per-lane kernel
        ("c2_down", 4, 3, (9, 11), (5, 7), 2, [3, 0, 3], [1, 0, 1]),
        ("c5_up", 3, 5, (5, 4), (7, 10), 5, [2, 0, 0, 1, 2], [1, 0, 1, 1, 0]),
        # degenerate taps: a source of one row (both row taps 0), of one column; an output of one row, of one column (its mirror is
        # the identity: Wd - 1 - x = x)
        ("src_h1", 2, 2, (1, 5), (3, 7), 3, [1, 0], [0, 1]),
        ("src_w1", 2, 2, (5, 1), (4, 3), 1, [1, 0], [1, 0]),
        ("out_h1", 2, 2, (6, 4), (1, 9), 1, [1, 0], [0, 1]),
        ("out_w1", 2, 3, (4, 6), (5, 1), 4, [1, 1, 0], [1, 0, 1]),
        ("c2_src_1x1", 2, 2, (1, 1), (2, 3), 2, [1, 0], [1, 0]),
        # a second trip of the grid-stride loop with a ragged end.  Four-pixel kernel: 33 * 65535 = 2162655 pixels, 540663 groups, a
        # tail of 3; the 33rd sample begins at group 524280, still on the first trip, so the second trip starts mid-sample and stays
        # in it.  With one sample more the boundary 33 * 65535 lies inside group 540663, on the second trip (tail 2).
        ("c1_second_trip", 3, 33, (16, 16), (255, 257), 1, _TRIP_IDX * 3, _TRIP_FLIP * 3),
        ("c1_second_trip_crossing", 3, 34, (16, 16), (255, 257), 1, _TRIP_IDX * 3 + [0], _TRIP_FLIP * 3 + [1]),
        # one-pixel kernel: 9 * 65535 = 589815 pixels
        ("c2_second_trip", 3, 9, (16, 16), (255, 257), 2, _TRIP_IDX[:9], _TRIP_FLIP[:9]),
    ]
)

# the dense kernel past its grid's capacity: (name, B, (Hs, Ws), (Hd, Wd), C): 5 * 187 * 189 * 3 = 530145 floats, 5857 on the second trip
DENSE_CASE = ("dense_second_trip", 5, (6, 7), (187, 189), 3)


def case(name):
    return next(c for c in CASES if c[0] == name)


# The 16 -> 255 / 257 upscales have inexact float32 scales and positions up to 15.5: with full-range bytes the float32 oracle itself
# strays 2e-6 from the float64 one (a lerp weight off by 1e-6 times a step of up to 2), which would take a yardstick of 6e-6.  Their
# bytes are drawn from a band of 48 levels (steps of at most 0.37), where it strays 4e-7: the geometry stays, a wrong tap or a wrong
# sample still shows at 1e-2 and more.
BANDS = {"c1_second_trip": (104, 152), "c1_second_trip_crossing": (104, 152), "c2_second_trip": (104, 152)}


def data(name, N, Hs, Ws, C):
    """N source images of random bytes for case ``name``: the whole range with 0 and 255 among them, or the case's band."""
    lo, hi = BANDS.get(name, (0, 256))
    src = np.random.default_rng(sum(name.encode()) % 1000).integers(lo, hi, size=(N, Hs, Ws, C), dtype=np.uint8)
    if name not in BANDS:
        src.reshape(-1)[0], src.reshape(-1)[-1] = 0, 255
    return src


def constant_images(N, Hs, Ws, C):
    """Image n holds the single byte v_n everywhere (distinct bytes, 0 and 255 first): the exact-value case."""
    v = np.array([0, 255, 100, 37, 201, 128, 127, 64][:N], dtype=np.uint8)
    assert len(v) == N
    return np.broadcast_to(v[:, None, None, None], (N, Hs, Ws, C)).copy(), v


def references(src, dst_hw):
    """The oracle of every image of ``src`` (unmirrored) in float64, and in float32 (the yardstick), both as float64 arrays."""
    from oracle import np_ops as O
    ref = O.normalize_resize_bilinear(src, dst_hw, dtype=np.float64)
    return ref, O.normalize_resize_bilinear(src, dst_hw, dtype=np.float32).astype(np.float64)


def tolerance(ref, ref32):
    """The rule of tests/test_mbstd_gpu.py: (rule, per-element bound, the float32 oracle's largest deviation)."""
    from helpers import POINT_ATOL, POINT_RTOL, YARDSTICK
    tol = POINT_RTOL * np.abs(ref) + POINT_ATOL * float(np.abs(ref).max())
    dev32 = np.abs(ref32 - ref)
    if (dev32 <= tol).all():
        return "point", tol, float(dev32.max())
    return "yardstick", np.full_like(tol, YARDSTICK * float(dev32.max())), float(dev32.max())


def case_references(name):
    """(src, {image: float64 oracle}, {image: per-element bound}, rule, float32 oracle's deviation) over the images case ``name`` gathers."""
    _, N, B, src_hw, dst_hw, C, idx, flip = case(name)
    src = data(name, N, *src_hw, C)
    used = sorted(set(idx))
    ref, ref32 = references(src[used], dst_hw)
    rule, tol, dev32 = tolerance(ref, ref32)
    return src, dict(zip(used, ref)), dict(zip(used, tol)), rule, dev32


def taps(n_out, n_in):
    """(position, lower tap, upper tap) of every output index, in exact-enough float64: what the kernels' tap_of decides."""
    pos = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    return pos, np.maximum(np.floor(pos), 0).astype(int), np.minimum(np.ceil(pos), n_in - 1).astype(int)
