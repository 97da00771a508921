"""Case tables, exact data, references and restated host predicates for the SWD kernels of csrc/swd.hip (tests/test_swd_cases_cpu.py
checks the tables on the CPU, tests/test_swd_exact_gpu.py runs them on the GPU).

The method is the one of tests/misc_cases.py and tests/blur_cases.py: data on which a correct kernel equals a float64 (or purely
combinatorial) reference bit for bit, so every comparison is array_equal, and a table whose every case names the cell -- kernel
instantiation, number of grid-stride trips, interior / border threads -- it is there for.  The predicates below restate the host code
of the seven entry points; each cites the lines it restates.  The V = 4 / V = 1 rules depend on pointer alignment, which no host-only
entry point reports: they are restated by reading only.  stats_blocks and abs_diff_blocks are pinned to the library through the two
workspace queries; the sort plan is pinned by the launch-name lists the GPU test records.

Recipes:
  ingest       the source holds 1 + its flat index (< 2^22), scale 2, shift -3: every output is an odd integer < 2^24 that names the
               (image, channel, y, x) it was read from (decode_ingest).
  pyramid      integer: pixels are integers in [-255, 255]; the taps are k/16, so pyr_down of the image (8 fraction bits), pyr_down of that
               (16), pyr_up of the first (14) and a TWO-level Laplacian pyramid are float32 numbers exactly, all below 2^9; the
               reference is the float64 evaluation of sliced_wasserstein.pyr_down / pyr_up.  Any order of accumulation passes: it tests
               geometry (reflection, seams, trips).  A third level (pyr_up of the second pyr_down: 22 fraction bits) is not exact and is not used.
               fractional: integers + uniform[0, 1), signed; compared with the float32 host functions, whose order of operations the
               kernels promise.  Small cells only.
  gather       the level holds its own flat index: an output names the (image, channel, y, x) it was read from (decode_level).
  standardize  channel c holds m_c + 2^k_c d with d = +-1 in equal numbers, shuffled: mean m_c, variance 4^k_c, the float32 casts and
               the quotient are exact, the output is d and stats_out is (m_c, 2^k_c); another channel's statistics move an element to
               a value that is not +-1.  Needs rows * nhood^2 even.
  sort         rows of distinct integers (a seeded permutation per row), small integers with many duplicates, and normal draws
               salted with +-0, +-inf and 1; the reference is np.sort.
  abs_diff     integers in [0, 256): every partial sum is below 2^53, exact in any order.

Not reachable at test sizes, and therefore not in the tables: the 2^31-element guards of every entry point (kMaxElems, swd.hip:584)
and a sort with n near 2^24 (swd.hip:717: 12 merge widths beyond the LDS chunk, 78 global launches).
"""
import numpy as np

KT = 256                      # swd.hip:20 kT
GRID_CAP = 256 * 8            # swd.hip:23 grid_for's cap, in blocks
SORT_T, SORT_CHUNK = 512, 4096            # swd.hip:449-450 kSortT, kSortChunk
SORT_CHUNK_GRID_CAP = 256 * 16            # swd.hip:726
PARTIAL_SPAN = KT * 16                    # swd.hip:440, :582: elements per block of the two-stage sums
SCALE, SHIFT = 2.0, -3.0                  # the ingest recipe


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ host predicates, restated
def grid_for(n):
    """swd.hip:23: blocks of kT threads for n work items, at most 2048."""
    return max(1, min(cdiv(n, KT), GRID_CAP))


def trips(n_items, grid_threads):
    """Iterations of `for (g = tid; g < n_items; g += grid_threads)` for the thread that makes the most (thread 0)."""
    return cdiv(n_items, grid_threads)


def stats_blocks(total):
    """swd.hip:440."""
    return max(1, min(cdiv(total, PARTIAL_SPAN), KT))


def abs_diff_blocks(seg):
    """swd.hip:582."""
    return max(1, min(cdiv(seg, PARTIAL_SPAN), KT))


def standardize_workspace_bytes(rows, nhood):
    """swd.hip:667-670."""
    return 0 if rows <= 0 or nhood <= 0 else (6 * stats_blocks(rows * 3 * nhood * nhood) + 6) * 8


def abs_diff_workspace_bytes(seg, nseg):
    """swd.hip:756-759."""
    return 0 if seg == 0 or nseg <= 0 else nseg * abs_diff_blocks(seg) * 8


def _launch(n_grp):
    g = grid_for(n_grp)
    return dict(n_grp=n_grp, grid=g, trips=trips(n_grp, g * KT))


def ingest_launch(B, H, W, C, nhwc, src_al=True, dst_al=True):
    """swd.hip:596-601."""
    HW = H * W
    vec = HW % 4 == 0 and src_al and dst_al
    gpi = HW // 4 if vec else HW
    why = "" if HW % 4 else ":".join([""] + [n for n, al in (("src", src_al), ("dst", dst_al)) if not al])
    return dict(_launch(gpi * B), V=4 if vec else 1, layout=0 if C == 1 else 2 if nhwc else 1, why=why)


def pyr_down_launch(planes, H, W, x_al=True, y_al=True):
    """swd.hip:619-627, and the interior condition of swd.hip:118 per thread of an output row."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    vec = Wo % 4 == 0 and y_al
    vec_in = int(vec and W % 4 == 0 and x_al)              # the V = 1 launch passes 0
    gpr = Wo // 4 if vec else Wo
    if vec and vec_in:
        threads = "".join(sorted({"I" if ox >= 2 and 2 * ox + 11 < W else "B" for ox in range(0, Wo, 4)}))
    else:
        threads = "S"                                      # every column through refl, one by one
    why = (":y" if not vec and Wo % 4 == 0 else "") if not vec else (":x" if not vec_in and W % 4 == 0 else "")
    return dict(_launch(planes * Ho * gpr), V=4 if vec else 1, vec_in=vec_in, threads=threads, why=why, Ho=Ho, Wo=Wo)


def pyr_up_launch(planes, h, w, out_al=True, min_al=True):
    """swd.hip:637-643 (a null minuend counts as aligned)."""
    vec = w % 2 == 0 and out_al and min_al
    gpr = 2 * w // 4 if vec else 2 * w
    return dict(_launch(planes * 2 * h * gpr), V=4 if vec else 1)


def gather_launch(B, nhood, per_image, desc_al=True):
    """swd.hip:653-661."""
    total = B * per_image * 3 * nhood * nhood
    vec = total % 4 == 0 and desc_al
    return dict(_launch(total // 4 if vec else total), V=4 if vec else 1, total=total, why="" if total % 4 else ("" if desc_al else ":desc"))


def standardize_launch(rows, nhood, desc_al=True):
    """swd.hip:681-683, :709: nb blocks for the two statistics passes, grid_for for the apply kernel."""
    total = rows * 3 * nhood * nhood
    vec = total % 4 == 0 and desc_al
    V = 4 if vec else 1
    nb = stats_blocks(total)
    return dict(_launch(total // 4 if vec else total), V=V, total=total, nb=nb, stats_trips=trips(cdiv(total, V), nb * KT),
                why="" if total % 4 else ("" if desc_al else ":desc"))


def abs_diff_launch(seg, nseg, a_al=True, b_al=True):
    """swd.hip:767-772: grid (nb, nseg)."""
    vec = seg % 4 == 0 and a_al and b_al
    V = 4 if vec else 1
    nb = abs_diff_blocks(seg)
    why = "" if seg % 4 else ":".join([""] + [n for n, al in (("a", a_al), ("b", b_al)) if not al])
    return dict(V=V, nb=nb, trips=trips(cdiv(seg, V), nb * KT), why=why)


def sort_plan(rows, n, aligned=True):
    """swd.hip:720-752: N, span, chunks per row, the chunk grid, work per row and grid of a global stage, and the ordered launches
    (name, j, mirror) -- j and mirror are None for the two LDS kernels."""
    if n == 1:
        return dict(N=1, vec=False, launches=[], names=[], chunk_trips=0, global_trips=0, n_global=0)
    N = 2
    while N < n:
        N <<= 1
    vec = n % 4 == 0 and aligned
    span = min(N, SORT_CHUNK)
    cpr = cdiv(n, span)
    n_chunks = rows * cpr
    cgrid = min(n_chunks, SORT_CHUNK_GRID_CAP)
    wpr = N // 8 if vec else N // 2
    n_work = rows * wpr
    ggrid = grid_for(n_work)
    launches = [("sort_rows_chunk", None, None)]
    k = 2 * SORT_CHUNK
    while k <= N:
        j = k >> 1
        while j >= SORT_CHUNK:
            launches.append(("sort_rows_global", j, k - 1 if j == k >> 1 else 0))
            j >>= 1
        launches.append(("sort_rows_tail", None, None))
        k <<= 1
    n_global = sum(1 for l in launches if l[0] == "sort_rows_global")
    return dict(N=N, vec=vec, span=span, cpr=cpr, n_chunks=n_chunks, cgrid=cgrid, wpr=wpr, n_work=n_work, ggrid=ggrid, launches=launches,
                names=[l[0] for l in launches], chunk_trips=trips(n_chunks, cgrid), n_global=n_global,
                global_trips=trips(n_work, ggrid * KT) if n_global else 0, last_chunk=n - (cpr - 1) * span,
                why=":x" if n % 4 == 0 and not aligned else "")


NAMES = {"ingest": ["swd_ingest"], "down": ["pyr_down"], "up": ["pyr_up"], "gather": ["swd_gather"],
         "std": ["swd_stats_sum", "swd_stats_dev", "swd_stats_final", "swd_standardize"], "absdiff": ["abs_diff_partial", "abs_diff_mean"]}


# ------------------------------------------------------------------ the case tables
# A case: entry, the arguments of the entry point, the offset in floats (0 aligned, 1 misaligned) of each buffer that has a say in the
# route, the cell it is in the table for, and for a second-trip case whether one row / plane / image fewer is back to one trip.
def _c(entry, cell, edge=None, **kw):
    off = {k: kw.pop(k) for k in list(kw) if k.startswith("off_")}
    return dict(entry=entry, cell=cell, edge=edge, off=off, **kw)


INGEST = [
    _c("ingest", "ingest L0 V4 t1", B=2, H=4, W=6, C=1, nhwc=False),
    _c("ingest", "ingest L0 V1 t1", B=2, H=5, W=7, C=1, nhwc=True),
    _c("ingest", "ingest L1 V4 t1", B=2, H=6, W=6, C=3, nhwc=False),
    _c("ingest", "ingest L1 V1 t1", B=2, H=5, W=7, C=3, nhwc=False),
    _c("ingest", "ingest L2 V4 t1", B=2, H=4, W=6, C=3, nhwc=True),
    _c("ingest", "ingest L2 V4 t1", B=3, H=30, W=36, C=3, nhwc=True),                    # four blocks
    _c("ingest", "ingest L2 V1 t1", B=3, H=5, W=7, C=3, nhwc=True),
    _c("ingest", "ingest L2 V1 t1", B=5, H=9, W=13, C=3, nhwc=True),                     # three blocks
    _c("ingest", "ingest L0 V1:src t1", B=2, H=8, W=8, C=1, nhwc=False, off_src=1),
    _c("ingest", "ingest L2 V1:src t1", B=2, H=4, W=6, C=3, nhwc=True, off_src=1),
    _c("ingest", "ingest L1 V1:dst t1", B=2, H=4, W=6, C=3, nhwc=False, off_dst=1),
    _c("ingest", "ingest L0 V4 t2", B=9, H=484, W=484, C=1, nhwc=True, edge=True),
    _c("ingest", "ingest L0 V1 t2", B=3, H=419, W=419, C=1, nhwc=False, edge=True),
]

DOWN = [
    _c("down", "down V4 in1 BI t1", planes=2, H=6, W=24),
    _c("down", "down V4 in1 BI t1", planes=3, H=10, W=32),
    _c("down", "down V4 in1 BI t1", planes=6, H=17, W=64),                               # two blocks
    _c("down", "down V4 in1 B t1", planes=2, H=7, W=8),
    _c("down", "down V4 in1 B t1", planes=3, H=16, W=16),
    _c("down", "down V4 in0 S t1", planes=2, H=9, W=7),
    _c("down", "down V4 in0 S t1", planes=2, H=6, W=15),
    _c("down", "down V4 in0 S t1", planes=1, H=8, W=23),
    _c("down", "down V4 in0:x S t1", planes=2, H=6, W=16, off_x=1),
    _c("down", "down V1 S t1", planes=2, H=6, W=5),
    _c("down", "down V1 S t1", planes=3, H=17, W=19),
    _c("down", "down V1 S t1", planes=5, H=33, W=34),                                    # six blocks
    _c("down", "down V1:y S t1", planes=2, H=6, W=16, off_y=1),
    _c("down", "down V4 in1 B H3 t1", planes=2, H=3, W=8),
    _c("down", "down V1 S H3 t1", planes=1, H=3, W=3),
    _c("down", "down V4 in0 S H4 t1", planes=2, H=4, W=15),
    _c("down", "down V4 in1 BI H5 t1", planes=2, H=5, W=24),
    _c("down", "down V1 S H5 t1", planes=2, H=5, W=5),
    _c("down", "down V4 in1 BI t2", planes=6, H=1184, W=1184, edge=True),
    _c("down", "down V1 S t2", planes=3, H=837, W=837, edge=True),
]

# pyr_up runs three ways per case -- plain, fused with a separate minuend, in place -- and the V of each is part of the cell
UP = [
    _c("up", "up V444 h2 t1", planes=2, h=2, w=2),
    _c("up", "up V444 hodd t1", planes=3, h=3, w=4),
    _c("up", "up V444 t1", planes=3, h=8, w=8),
    _c("up", "up V444 t1", planes=2, h=32, w=32),                                        # eight blocks
    _c("up", "up V444 hodd t1", planes=6, h=9, w=10),
    _c("up", "up V111 h2 t1", planes=2, h=2, w=3),
    _c("up", "up V111 hodd t1", planes=2, h=5, w=5),
    _c("up", "up V111 t1", planes=2, h=4, w=7),
    _c("up", "up V111 hodd t1", planes=3, h=13, w=15),                                   # five blocks
    _c("up", "up V111:out t1", planes=2, h=4, w=6, off_out=1),
    _c("up", "up V414:min t1", planes=2, h=4, w=6, off_min=1),
    _c("up", "up V444 t2", planes=3, h=420, w=418, edge=True),
    _c("up", "up V111 hodd t2", planes=1, h=363, w=363, edge=False),                     # 362 rows still take two trips
    _c("up", "up V111 t2", planes=1, h=362, w=363, edge=True),
]

GATHER = [
    _c("gather", "gather n1 V4 pi1 t1", B=4, H=5, W=6, nhood=1, per_image=1),           # every quad crosses b, a, c, t and an image
    _c("gather", "gather n1 V1 pi%4 t1", B=3, H=5, W=6, nhood=1, per_image=5),
    _c("gather", "gather n3 V4 pi%4 t1", B=2, H=5, W=6, nhood=3, per_image=6),
    _c("gather", "gather n3 V1 pi1 t1", B=3, H=5, W=6, nhood=3, per_image=1),
    _c("gather", "gather n5 V4 pi4k t1", B=2, H=7, W=9, nhood=5, per_image=8),
    _c("gather", "gather n5 V1 pi%4 t1", B=1, H=7, W=9, nhood=5, per_image=7),
    _c("gather", "gather n7 V4 pi%4 t1", B=4, H=9, W=8, nhood=7, per_image=3),
    _c("gather", "gather n7 V1 pi%4 t1", B=3, H=9, W=8, nhood=7, per_image=5),
    _c("gather", "gather n7 V4 pi4k t1", B=2, H=16, W=24, nhood=7, per_image=128),      # 37 blocks
    _c("gather", "gather n9 V4 pi%4 t1", B=2, H=11, W=13, nhood=9, per_image=2),
    _c("gather", "gather n9 V1 pi%4 t1", B=1, H=11, W=13, nhood=9, per_image=3),
    _c("gather", "gather n7 V1:desc pi4k t1", B=2, H=9, W=8, nhood=7, per_image=4, off_desc=1),
    _c("gather", "gather n1 V1:desc pi4k t1", B=2, H=5, W=6, nhood=1, per_image=4, off_desc=1),
    _c("gather", "gather n7 V4 pi4k t2", B=2, H=16, W=16, nhood=7, per_image=7200, edge=True),
    _c("gather", "gather n7 V1 pi%4 t2", B=1, H=16, W=16, nhood=7, per_image=3567, edge=True),
]

# standardize: V = 1 rows are even (the recipe needs rows * nhood^2 even) and no multiple of 4
STD = [
    _c("std", "std n1 V4 nb1 t1", rows=4, nhood=1),
    _c("std", "std n1 V1 nb1 t1", rows=6, nhood=1),
    _c("std", "std n3 V4 nb1 t1", rows=8, nhood=3),
    _c("std", "std n3 V1 nb1 t1", rows=2, nhood=3),
    _c("std", "std n5 V4 nb1 t1", rows=4, nhood=5),
    _c("std", "std n5 V1 nb1 t1", rows=6, nhood=5),
    _c("std", "std n7 V4 nb1 t1", rows=8, nhood=7),
    _c("std", "std n7 V1 nb1 t1", rows=2, nhood=7),
    _c("std", "std n9 V4 nb1 t1", rows=4, nhood=9),
    _c("std", "std n9 V1 nb1 t1", rows=6, nhood=9),
    _c("std", "std n7 V1:desc nb1 t1", rows=8, nhood=7, off_desc=1),
    _c("std", "std n3 V1:desc nbN t1", rows=640, nhood=3, off_desc=1),
    _c("std", "std n7 V4 nbN t1", rows=640, nhood=7),
    _c("std", "std n5 V1 nbN t1", rows=250, nhood=5),
    _c("std", "std n9 V4 nbcap t1", rows=4300, nhood=9),
    _c("std", "std n7 V1 nbcap t2", rows=7106, nhood=7),
    _c("std", "std n7 V1 nbN t2", rows=3570, nhood=7, edge=True),                       # the smallest even, V = 1 row count with a second trip
]

# sort: kinds are all three of KINDS unless the case names fewer
SORT = [
    _c("sort", "sort scalar span2 c1 g0", rows=3, n=2),
    _c("sort", "sort scalar span8 c1 g0", rows=3, n=5),
    _c("sort", "sort vec span64 c1 g0", rows=2, n=64),
    _c("sort", "sort scalar span1024 c1 g0", rows=3, n=1023),
    _c("sort", "sort vec span4096 c1 g0", rows=2, n=4096),
    _c("sort", "sort scalar span4096 c1 g1x1", rows=3, n=4097),
    _c("sort", "sort vec span4096 c1 g1x1", rows=2, n=4100),
    _c("sort", "sort vec span4096 c1 g3x1", rows=2, n=8196),
    _c("sort", "sort scalar span4096 c1 g6x1", rows=2, n=16385),
    _c("sort", "sort scalar:x span4096 c1 g0", rows=3, n=4096, off_x=1),
    _c("sort", "sort scalar:x span4096 c1 g3x1", rows=3, n=8196, off_x=1),
    _c("sort", "sort vec span32 c2 g0", rows=4100, n=24, edge=False),                   # 4099 rows still take two trips
    _c("sort", "sort scalar span32 c2 g0", rows=4100, n=23, edge=False),
    _c("sort", "sort vec span32 c2 g0", rows=4097, n=24, edge=True),
    _c("sort", "sort scalar span32 c2 g0", rows=4097, n=23, edge=True),
    _c("sort", "sort vec span4096 c2 g1x5", rows=2049, n=4100, edge=True, kinds=("perm", "special")),
    _c("sort", "sort scalar span4096 c1 g3x2", rows=65, n=8193, edge=True, loop="global"),
    _c("sort", "sort vec span4096 c1 g3x2", rows=257, n=8196, edge=True, loop="global", kinds=("perm", "special")),
]
KINDS = ("perm", "duplicates", "special")

ABSDIFF = [
    _c("absdiff", "absdiff V4 nb1 nseg1", seg=8, nseg=1),
    _c("absdiff", "absdiff V1 nb1 nseg5", seg=7, nseg=5),
    _c("absdiff", "absdiff V4 nbN nseg5", seg=12292, nseg=5),
    _c("absdiff", "absdiff V1 nbN nseg1", seg=12291, nseg=1),
    _c("absdiff", "absdiff V1:a nb1 nseg2", seg=8, nseg=2, off_a=1),
    _c("absdiff", "absdiff V1:b nbN nseg2", seg=4100, nseg=2, off_b=1),
    _c("absdiff", "absdiff V4 nbcap nseg2", seg=1048580, nseg=2),
    _c("absdiff", "absdiff V1 nbcap nseg2", seg=1048579, nseg=2),
]

TABLES = {"ingest": INGEST, "down": DOWN, "up": UP, "gather": GATHER, "std": STD, "sort": SORT, "absdiff": ABSDIFF}
ALL = [c for t in TABLES.values() for c in t]

# Every cell the tables have to hit, written out: the CPU test compares by set equality
CELLS = {
    "ingest L0 V4 t1", "ingest L0 V1 t1", "ingest L1 V4 t1", "ingest L1 V1 t1", "ingest L2 V4 t1", "ingest L2 V1 t1",
    "ingest L0 V1:src t1", "ingest L2 V1:src t1", "ingest L1 V1:dst t1", "ingest L0 V4 t2", "ingest L0 V1 t2",
    "down V4 in1 BI t1", "down V4 in1 B t1", "down V4 in0 S t1", "down V4 in0:x S t1", "down V1 S t1", "down V1:y S t1",
    "down V4 in1 B H3 t1", "down V1 S H3 t1", "down V4 in0 S H4 t1", "down V4 in1 BI H5 t1", "down V1 S H5 t1",
    "down V4 in1 BI t2", "down V1 S t2",
    "up V444 h2 t1", "up V444 hodd t1", "up V444 t1", "up V111 h2 t1", "up V111 hodd t1", "up V111 t1", "up V111:out t1", "up V414:min t1",
    "up V444 t2", "up V111 hodd t2", "up V111 t2",
    "gather n1 V4 pi1 t1", "gather n1 V1 pi%4 t1", "gather n3 V4 pi%4 t1", "gather n3 V1 pi1 t1", "gather n5 V4 pi4k t1",
    "gather n5 V1 pi%4 t1", "gather n7 V4 pi%4 t1", "gather n7 V1 pi%4 t1", "gather n7 V4 pi4k t1", "gather n9 V4 pi%4 t1",
    "gather n9 V1 pi%4 t1", "gather n7 V1:desc pi4k t1", "gather n1 V1:desc pi4k t1", "gather n7 V4 pi4k t2", "gather n7 V1 pi%4 t2",
    "std n1 V4 nb1 t1", "std n1 V1 nb1 t1", "std n3 V4 nb1 t1", "std n3 V1 nb1 t1", "std n5 V4 nb1 t1", "std n5 V1 nb1 t1",
    "std n7 V4 nb1 t1", "std n7 V1 nb1 t1", "std n9 V4 nb1 t1", "std n9 V1 nb1 t1", "std n7 V1:desc nb1 t1", "std n3 V1:desc nbN t1",
    "std n7 V4 nbN t1", "std n5 V1 nbN t1", "std n9 V4 nbcap t1", "std n7 V1 nbcap t2", "std n7 V1 nbN t2",
    "sort scalar span2 c1 g0", "sort scalar span8 c1 g0", "sort vec span64 c1 g0", "sort scalar span1024 c1 g0", "sort vec span4096 c1 g0",
    "sort scalar span4096 c1 g1x1", "sort vec span4096 c1 g1x1", "sort vec span4096 c1 g3x1", "sort scalar span4096 c1 g6x1",
    "sort scalar:x span4096 c1 g0", "sort scalar:x span4096 c1 g3x1", "sort vec span32 c2 g0", "sort scalar span32 c2 g0",
    "sort vec span4096 c2 g1x5", "sort scalar span4096 c1 g3x2", "sort vec span4096 c1 g3x2",
    "absdiff V4 nb1 nseg1", "absdiff V1 nb1 nseg5", "absdiff V4 nbN nseg5", "absdiff V1 nbN nseg1", "absdiff V1:a nb1 nseg2",
    "absdiff V1:b nbN nseg2", "absdiff V4 nbcap nseg2", "absdiff V1 nbcap nseg2",
}
# the cells whose subject is a second trip of a grid-stride loop: those of the cases that say whether they sit on the edge
SECOND_TRIP_CELLS = {c["cell"] for c in ALL if c["edge"] is not None}

# one case per entry point for the NaN-isolation and run-twice tests: (entry, index into its table)
PER_ENTRY = [("ingest", 5), ("down", 2), ("up", 4), ("gather", 8), ("std", 12), ("sort", 7), ("absdiff", 2)]


def al(case, name):
    return case["off"].get("off_" + name, 0) == 0


def _nb_tag(nb):
    return "nb1" if nb == 1 else "nbcap" if nb == KT else "nbN"


def describe(case):
    """The restated launch of a case and the cell that follows from it."""
    e = case["entry"]
    if e == "ingest":
        d = ingest_launch(case["B"], case["H"], case["W"], case["C"], case["nhwc"], al(case, "src"), al(case, "dst"))
        d["cell"] = f"ingest L{d['layout']} V{d['V']}{d['why']} t{d['trips']}"
    elif e == "down":
        d = pyr_down_launch(case["planes"], case["H"], case["W"], al(case, "x"), al(case, "y"))
        tag = f" in{d['vec_in']}{d['why']}" if d["V"] == 4 else d["why"]
        d["cell"] = f"down V{d['V']}{tag} {d['threads']}" + (f" H{case['H']}" if case["H"] <= 5 else "") + f" t{d['trips']}"
    elif e == "up":
        ways = up_ways(case)
        d = dict(ways["plain"], ways=ways)
        why = "" if case["w"] % 2 else ":out" if not al(case, "out") else ":min" if not al(case, "min") else ""
        h = " h2" if case["h"] == 2 else " hodd" if case["h"] % 2 else ""
        d["cell"] = "up V" + "".join(str(ways[k]["V"]) for k in ("plain", "fused", "inplace")) + why + h + f" t{max(v['trips'] for v in ways.values())}"
    elif e == "gather":
        d = gather_launch(case["B"], case["nhood"], case["per_image"], al(case, "desc"))
        pi = case["per_image"]
        d["cell"] = f"gather n{case['nhood']} V{d['V']}{d['why']} " + ("pi1" if pi == 1 else "pi%4" if pi % 4 else "pi4k") + f" t{d['trips']}"
    elif e == "std":
        d = standardize_launch(case["rows"], case["nhood"], al(case, "desc"))
        d["cell"] = f"std n{case['nhood']} V{d['V']}{d['why']} {_nb_tag(d['nb'])} t{d['trips']}"
    elif e == "sort":
        d = sort_plan(case["rows"], case["n"], al(case, "x"))
        g = f"g{d['n_global']}" + (f"x{d['global_trips']}" if d["n_global"] else "")
        d["cell"] = f"sort {'vec' if d['vec'] else 'scalar'}{d['why']} span{d['span']} c{d['chunk_trips']} {g}"
    else:
        d = abs_diff_launch(case["seg"], case["nseg"], al(case, "a"), al(case, "b"))
        d["cell"] = f"absdiff V{d['V']}{d['why']} {_nb_tag(d['nb'])} nseg{case['nseg']}"
    d["names"] = d["names"] if e == "sort" else NAMES[e]
    return d


def up_ways(case):
    """pyr_up's three calls per case: plain (null minuend), fused (a separate minuend), in place (the minuend is the output)."""
    p, h, w = case["planes"], case["h"], case["w"]
    return {"plain": pyr_up_launch(p, h, w, al(case, "out"), True), "fused": pyr_up_launch(p, h, w, al(case, "out"), al(case, "min")),
            "inplace": pyr_up_launch(p, h, w, al(case, "out"), al(case, "out"))}


def one_fewer(case):
    """The case with one plane / image / row fewer; with a single plane or image, one row of the image (one descriptor) fewer."""
    c = dict(case)
    e = case["entry"]
    if e == "ingest":
        c["B"] -= 1
    elif e in ("down", "up"):
        if c["planes"] > 1:
            c["planes"] -= 1
        else:
            c["H" if e == "down" else "h"] -= 1
    elif e == "gather":
        if c["B"] > 1:
            c["B"] -= 1
        else:
            c["per_image"] -= 1
    elif e == "std":
        c["rows"] -= 4                  # the next smaller row count that keeps the recipe (even) and the V = 1 of the cell (no multiple of 4)
    else:
        c["rows"] -= 1
    return c


def loop_trips(case):
    """The trip count the cell of a second-trip case is about."""
    d = describe(case)
    if case["entry"] == "sort":
        return d["global_trips"] if case.get("loop") == "global" else d["chunk_trips"]
    if case["entry"] == "up":
        return max(v["trips"] for v in d["ways"].values())
    return d["trips"]


def case_id(case):
    skip = ("entry", "cell", "edge", "off", "kinds", "loop")
    return case["entry"] + "-" + "x".join(f"{k}{int(v)}" for k, v in case.items() if k not in skip) + \
        "".join(f"-{k[4:]}+{v}" for k, v in sorted(case["off"].items()))


def missing_and_extra(cases=None):
    hit = {describe(c)["cell"] for c in (ALL if cases is None else cases)}
    return sorted(CELLS - hit), sorted(hit - CELLS)


# ------------------------------------------------------------------ data and references
def _rng(case, salt=0):
    skip = ("entry", "cell", "edge", "off", "kinds", "loop")
    return np.random.default_rng([salt, list(TABLES).index(case["entry"])] + [int(v) for k, v in case.items() if k not in skip])


def ingest_data(case):
    """(src in its own layout, planar [B, C, H, W] view of it, wanted [B, 3, H, W]) as float64."""
    B, H, W, C = case["B"], case["H"], case["W"], case["C"]
    src = 1.0 + np.arange(B * C * H * W, dtype=np.float64)
    assert src[-1] < 1 << 22
    src = src.reshape((B, H, W, C) if case["nhwc"] else (B, C, H, W))
    planar = np.transpose(src, (0, 3, 1, 2)) if case["nhwc"] else src
    want = planar * SCALE + SHIFT
    return src, planar, (np.repeat(want, 3, axis=1) if C == 1 else want)


def decode_ingest(case, got, want):
    """The first wrong output, and the source element (image, y, x, channel) its value names."""
    bad = np.argwhere(np.asarray(got, np.float64) != want)
    if not len(bad):
        return "equal"
    at = tuple(int(v) for v in bad[0])
    g = float(np.asarray(got)[at])
    B, H, W, C = case["B"], case["H"], case["W"], case["C"]
    k = (g - SHIFT) / SCALE - 1.0
    if np.isfinite(g) and k == int(k) and 0 <= k < B * H * W * C:
        src = np.unravel_index(int(k), (B, H, W, C) if case["nhwc"] else (B, C, H, W))
        names = ("image", "y", "x", "channel") if case["nhwc"] else ("image", "channel", "y", "x")
        seen = ", ".join(f"{n} {int(v)}" for n, v in zip(names, src))
    else:
        seen = "no source element"
    return f"{len(bad)} of {want.size} wrong; first at [image {at[0]}, channel {at[1]}, y {at[2]}, x {at[3]}]: got {g}, want {want[at]}; it holds: {seen}"


def int_image(shape, rng):
    return rng.integers(-255, 256, size=shape).astype(np.float64)


def frac_image(shape, rng):
    return (rng.integers(-255, 255, size=shape) + rng.random(size=shape)).astype(np.float32)


def down_data(case, recipe, salt=0):
    shape = (1, case["planes"], case["H"], case["W"])
    rng = _rng(case, salt)
    return int_image(shape, rng) if recipe == "int" else frac_image(shape, rng)


def up_data(case, recipe, salt=0):
    """(low, minuend): integer recipe -- the minuend is an integer image and low its pyr_down (so minuend - pyr_up(low) is level 0 of
    a two-level Laplacian pyramid); fractional -- two independent draws."""
    p, h, w = case["planes"], case["h"], case["w"]
    rng = _rng(case, salt)
    if recipe == "int":
        from blurred_gan_amd import sliced_wasserstein as sw
        x = int_image((1, p, 2 * h, 2 * w), rng)
        return sw.pyr_down(x), x
    return frac_image((1, p, h, w), rng), frac_image((1, p, 2 * h, 2 * w), rng)


def pyr_recipes(case):
    return ("int",) if "t2" in case["cell"] else ("int", "frac")


def gather_level(case):
    B, H, W = case["B"], case["H"], case["W"]
    return np.arange(B * 3 * H * W, dtype=np.float64).reshape(B, 3, H, W)


def gather_centres(case, salt=0):
    """Seeded centres in [half, size - half); every second one (and the first and the last) at one of the four extreme corners."""
    B, H, W, n, pi = case["B"], case["H"], case["W"], case["nhood"], case["per_image"]
    half, total = n // 2, B * pi
    rng = _rng(case, salt)
    cx = rng.integers(half, W - half, size=total).astype(np.int32)
    cy = rng.integers(half, H - half, size=total).astype(np.int32)
    corners = [(half, half), (W - half - 1, half), (half, H - half - 1), (W - half - 1, H - half - 1)]
    for k in range(0, total, 2):
        cx[k], cy[k] = corners[(k // 2) % 4]
    cx[-1], cy[-1] = corners[3]
    return cx, cy


def gather_ref(level, cx, cy, nhood, per_image):
    """include/bgan.h: desc[t, c, a, b] = level[t // per_image, c, cy[t] + b - half, cx[t] + a - half]."""
    total, half = len(cx), nhood // 2
    img = (np.arange(total) // per_image).reshape(total, 1, 1, 1)
    ch = np.arange(3).reshape(1, 3, 1, 1)
    a = np.arange(nhood).reshape(1, 1, nhood, 1)
    b = np.arange(nhood).reshape(1, 1, 1, nhood)
    return level[img, ch, cy.reshape(-1, 1, 1, 1).astype(np.int64) + b - half, cx.reshape(-1, 1, 1, 1).astype(np.int64) + a - half]


def decode_level(case, got, want):
    bad = np.argwhere(np.asarray(got, np.float64) != want)
    if not len(bad):
        return "equal"
    at = tuple(int(v) for v in bad[0])
    g = float(np.asarray(got)[at])
    shape = (case["B"], 3, case["H"], case["W"])

    def name(v):
        if not (np.isfinite(v) and v == int(v) and 0 <= v < np.prod(shape)):
            return "no level element"
        return "(image %d, channel %d, y %d, x %d)" % tuple(int(i) for i in np.unravel_index(int(v), shape))
    return (f"{len(bad)} of {want.size} wrong; first at [t {at[0]}, c {at[1]}, a {at[2]}, b {at[3]}]: got {g} = {name(g)}, "
            f"want {want[at]} = {name(want[at])}")


STD_M, STD_K = (100.0, -37.0, 5.0), (3, 0, -2)


def std_data(case, salt=0):
    """(x [rows, 3, n, n], d) in float64: x = m_c + 2^k_c d, d = +-1 in equal numbers per channel."""
    rows, n = case["rows"], case["nhood"]
    count = rows * n * n
    assert count % 2 == 0, "the recipe needs rows * nhood^2 even"
    rng = _rng(case, salt)
    d = np.empty((rows, 3, n, n), np.float64)
    for c in range(3):
        v = np.repeat([1.0, -1.0], count // 2)
        rng.shuffle(v)
        d[:, c] = v.reshape(rows, n, n)
    m = np.array(STD_M).reshape(1, 3, 1, 1)
    s = np.array([2.0 ** k for k in STD_K]).reshape(1, 3, 1, 1)
    return m + s * d, d


def std_stats():
    return np.array([[m, 2.0 ** k] for m, k in zip(STD_M, STD_K)]).reshape(6)


def sort_data(case, kind, salt=0):
    rows, n = case["rows"], case["n"]
    rng = _rng(case, salt + 10 * KINDS.index(kind))
    if kind == "perm":
        return (rng.permuted(np.tile(np.arange(n, dtype=np.int64), (rows, 1)), axis=1) - n // 2).astype(np.float32)
    if kind == "duplicates":
        return rng.integers(0, 8, size=(rows, n)).astype(np.float32)
    x = rng.standard_normal((rows, n)).astype(np.float32)
    flat = x.reshape(-1)
    flat[::3] = np.resize(np.array([0.0, -0.0, np.inf, -np.inf, 1.0], np.float32), flat[::3].shape)
    return x


def sort_kinds(case):
    return case.get("kinds", KINDS)


def absdiff_data(case, salt=0):
    seg, nseg = case["seg"], case["nseg"]
    rng = _rng(case, salt)
    a = rng.integers(0, 256, size=seg * nseg).astype(np.float64)
    b = rng.integers(0, 256, size=seg * nseg).astype(np.float64)
    assert 255 * seg < 1 << 53
    return a, b, np.abs(a - b).reshape(nseg, seg).sum(axis=1) / seg
