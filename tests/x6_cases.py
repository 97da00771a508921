"""Case table, data recipes and restated arithmetic for the split-bf16 gather-GEMM of csrc/conv_igemm_x6.hip (conv_math="bf16x6").
tests/test_x6_cases_cpu.py holds the table and the recipes to their claims on the CPU; tests/test_conv_x6_exact_gpu.py and
tests/x6_forced_child.py run them on the GPU.

The kernel rebuilds an fp32 product a.b from six bf16 cross terms of a three-piece split of each operand and accumulates them in
fp32.  `split3` restates the split (conv_igemm_x6.hip:46-77), KEPT_TERMS the six MFMAs in the order they are issued (:235-240),
`x6_can_run` what the kernel can run (:324-342).  conv_tol, the bound the kernel's other tests use, is about 1e-4 of the output scale:
a lost SECOND-order term (hi.lo, lo.hi, mid.mid: 2^-16 of the product) stays a factor of ten inside it.  The recipes here do not:

  pieces    every nonzero operand element is +-(2^16 + m 2^6 + l 2^-4), m and l in {1, 2, 3}, sign, m and l seeded per element.
            split3 gives exactly hi = 2^16, mid = m 2^6, lo = l 2^-4, and the six kept terms of a product add up to
                2^12 (2^20 + (m_a + m_b) 2^10 + (l_a + l_b + m_a m_b)):
            one float32 number (21 significant bits) with each order of terms in a 10-bit digit of its own.  The three terms left
            out add up to at most 72 + 9/256, below the half ulp of 256, so the kept sum IS the correctly rounded product and the
            expectation is RNE(float64 product), whatever the kernel keeps.  One kept term dropped or doubled moves the result by at
            least 2^12 = 8 ulps.  The activations are the impulse images of conv_cases.impulses (no window holds two, the seam pixels
            of the case's M tiles included) with the channels dealt round the 16-channel k-slices, so every output is ONE product;
            every weight at every (tap, ci, co) is live in all three pieces, so a stale LDS plane or a wrong plane offset adds a second
            product and shows.  describe_wrong decodes the digits of a wrong output.
  dense, decode   the integer recipes of conv_cases.py, unchanged.  They hold the geometry and the accumulation across K steps,
            taps and k-slices (decode weights above 255 have a live mid piece, above 65 535 a live lo piece).  Under x6 they are
            exact apart from lifted zeros AND one unit in the last place of the matrix pipe's adder (adder_unit: a negative lifted
            residue in the accumulator is floored against large products, 2.4e-7 on sums of products of [-3, 3]; on the MI355X
            about one dense output in 5000, no decode output); a wrong tap, pixel or channel moves an output by at least 1.

Lifted zeros: a zero mid / lo piece of a finite element is stored as +-2^-126 (no_zero_bf16x2), so an output whose reference is 0
holds up to 5 K 2^-126 max(max|a|, max|w|): a lifted piece meets at most the largest piece of the other operand, five of the six
terms can hold one, and lifted x lifted underflows.  Everywhere else the comparison of "pieces" is array_equal (`compare`).
"""
import numpy as np

import conv_cases as CC
from oracle import np_ops as O

PIECES = ("hi", "mid", "lo")
# (activation piece, weight piece) of the six MFMAs in issue order, conv_igemm_x6.hip:235-240 (bw[] is the weight, af[] the activation)
KEPT_TERMS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))
LIFT = 2.0 ** -126
K_BK, K_BM = 32, 128                 # conv_igemm_x6.hip:37 kBK, the BM of every launch_x6 instantiation (:419-421)
X6_NAMES = ("conv_igemm_x6_fwd", "conv_igemm_x6_dgrad")


# ===================================================================================================================================
# the split, restated
# ===================================================================================================================================
def _bf16_rne(v):
    """float32 -> the nearest bfloat16 (ties to even) as float32: v_cvt_pk_bf16_f32; finite inputs."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _lift(piece, hi):
    """no_zero_bf16x2 (:46-51): a magnitude below the smallest normal bf16 becomes 2^-126; the sign is the ELEMENT's (hi's)."""
    mag = np.maximum(piece.view(np.uint32) & 0x7fff0000, 0x00800000)
    return (mag | (hi.view(np.uint32) & 0x80000000)).astype(np.uint32).view(np.float32)


def split3(x, lift=True):
    """split4 (:54-77) per element -> (hi, mid, lo) as float32 arrays of bf16-representable numbers.
    hi = the top 16 bits of x (a bit mask, not a rounding); r = x - hi; mid = the top 16 bits of r; lo = bf16_rne(r - mid).
    A NaN becomes the canonical quiet NaN first (:61); Inf / NaN get mid = lo = 0 (:64); zero (or subnormal) mid / lo pieces are
    then lifted to +-2^-126 with the element's sign (:71-76) unless lift is False (the exact value of the pieces)."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        hb = np.where(np.isnan(x), np.uint32(0x7fc00000), x.view(np.uint32)).astype(np.uint32)
        hi = (hb & np.uint32(0xffff0000)).view(np.float32)
        r = x - hi
        r = np.where(r == r, r, np.float32(0)).astype(np.float32)
        mid = (r.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        lo = _bf16_rne(r - mid)
    if lift:
        mid, lo = _lift(mid, hi), _lift(lo, hi)
    return hi, mid, lo


def lifted_zero_bound(K, amax, wmax):
    return 5.0 * K * LIFT * max(amax, wmax)


# ===================================================================================================================================
# what runs, restated
# ===================================================================================================================================
def x6_can_run(bwd, B, H, W, Ci, Co, k, s):
    """make_params (:336-342) and x6_geometry_ok (:324-334): 32-channel K steps, whole 32-column tiles, more than 16 positions in
    the largest phase, operands below 2 GiB."""
    if min(B, H, W, Ci, Co) <= 0 or k < 1 or not k & 1 or k * k > 25 or s not in (1, 2):
        return False
    p = CC.gather_params(bwd, B, H, W, Ci, Co, k, s)
    if p["Ck"] % K_BK or p["N"] % 32 or max(g["Ha"] * g["Wa"] for g in p["ph"]) <= 16:
        return False
    return B * p["Hs"] * p["Ws"] * p["Ck"] * 4 < 1 << 31 and B * p["Hd"] * p["Wd"] * p["N"] < 1 << 31 and CC._ntap_w(p) * p["N"] * p["Ck"] * 4 < 1 << 31


def in_table(bwd, H, W, Ci, Co, k, s):
    """x6_in_table (:315-320)."""
    return k == 5 and (int(bool(bwd)), H, W, Ci, Co, s) in CC.X6_TABLE


def launch(bwd, shape, k):
    """try_conv_x6 / launch_x6 (:351-421) for a geometry x6_can_run accepts: tile width, tiles, statistics rows, launch name."""
    B, H, W, Ci, Co, s = shape
    p = CC.gather_params(bwd, B, H, W, Ci, Co, k, s)
    N, Ck = p["N"], p["Ck"]
    BN = 128 if N % 128 == 0 else 64 if N % 64 == 0 else 32
    M = [B * g["Ha"] * g["Wa"] for g in p["ph"]]
    mtiles = CC.cdiv(max(M), K_BM)
    return dict(p=p, N=N, Ck=Ck, BN=BN, ntiles=N // BN, mtiles=mtiles, M=M, nphase=len(M), kchunks=Ck // K_BK,
                stats_rows=len(M) * mtiles, empty_tiles=sum(max(0, mtiles - CC.cdiv(m, K_BM)) for m in M),
                name=X6_NAMES[1 if bwd else 0], K=max(len(g["taps"]) for g in p["ph"]) * Ck)


def cells(bwd, shape, k):
    """The cells of X6_CELLS a case covers."""
    d = launch(bwd, shape, k)
    s = shape[5]
    c = {f"n{d['N']}", f"kchunks{min(d['kchunks'], 3)}", f"k{k}", f"s{s}", f"{'dgrad' if bwd else 'fwd'}:bn{d['BN']}"}
    Mmax = max(d["M"])
    c.add("m_below_one_tile" if Mmax < K_BM else "m_one_tile" if Mmax == K_BM else "m_ragged_tiles" if Mmax % K_BM else "m_whole_tiles")
    if len(set(d["M"])) > 1:
        c.add("phases_of_different_extents")
    if d["empty_tiles"]:
        c.add("empty_m_tile")
    if any(not g["taps"] for g in d["p"]["ph"]):
        c.add("phase_without_taps")
    if max(g["Ha"] * g["Wa"] for g in d["p"]["ph"]) == 17:
        c.add("17_positions")
    return c


X6_CELLS = ({"n128", "n64", "n32", "n96", "n192", "kchunks1", "kchunks2", "kchunks3", "k1", "k3", "k5", "s1", "s2", "m_below_one_tile", "m_one_tile", "m_ragged_tiles", "phases_of_different_extents", "empty_m_tile",
             "phase_without_taps", "17_positions"} | {f"{w}:bn{b}" for w in ("fwd", "dgrad") for b in (128, 64, 32)})

# (data gradient?, (B, H, W, Cin, Cout, stride) on the conv's input side, k, the cells the case is in the table for).  All run with
# BG_CONV_X6_FORCE=1.  N is Cout forward and Cin in the data gradient, the contraction runs over the other.
ROUTE_CASES = [
    (0, (5, 8, 8, 32, 32, 1), 5, {"fwd:bn32", "n32", "m_ragged_tiles", "kchunks1", "k5", "s1"}),                  # M = 320: 2.5 tiles
    (1, (5, 8, 8, 32, 32, 1), 5, {"dgrad:bn32", "n32", "m_ragged_tiles", "kchunks1", "k5", "s1"}),
    (0, (2, 8, 8, 64, 128, 1), 3, {"fwd:bn128", "n128", "m_one_tile", "kchunks2", "k3"}),
    (1, (2, 16, 16, 64, 64, 2), 3, {"dgrad:bn64", "n64", "m_one_tile", "kchunks2", "k3", "s2"}),                  # four phases of 8 x 8
    (0, (1, 8, 8, 96, 64, 1), 1, {"fwd:bn64", "n64", "m_below_one_tile", "kchunks3", "k1"}),
    (1, (1, 6, 6, 32, 96, 1), 1, {"dgrad:bn32", "m_below_one_tile", "kchunks3", "k1", "s1"}),
    (0, (3, 20, 20, 32, 96, 2), 5, {"fwd:bn32", "n96", "m_ragged_tiles", "s2"}),                                  # three 32-column tiles
    (1, (3, 8, 8, 96, 32, 1), 3, {"dgrad:bn32", "n96", "m_ragged_tiles"}),
    (0, (2, 8, 8, 32, 192, 1), 3, {"fwd:bn64", "n192", "m_one_tile"}),                                            # three 64-column tiles
    (1, (5, 8, 8, 192, 64, 1), 5, {"dgrad:bn64", "n192", "kchunks2", "m_ragged_tiles"}),
    (1, (6, 9, 9, 128, 32, 2), 5, {"dgrad:bn128", "n128", "phases_of_different_extents", "empty_m_tile", "s2"}),  # phases of 150 / 120 / 120 / 96 rows
    (0, (3, 21, 21, 64, 64, 2), 5, {"fwd:bn64", "m_ragged_tiles", "kchunks2", "s2"}),                              # 11 x 11 outputs of an odd map
    (1, (2, 10, 10, 32, 32, 2), 1, {"dgrad:bn32", "phase_without_taps", "k1", "s2"}),                              # k = 1 at stride 2: three phases store zeros
    (0, (8, 1, 17, 32, 32, 1), 5, {"17_positions", "m_ragged_tiles"}),                                            # just inside the 16-position rule
]
# 16 positions: the kernel must NOT launch, forced or not (the fp32 path runs and is exact on the integer recipes)
MUST_NOT_RUN = [(0, (8, 4, 4, 32, 32, 1), 5), (1, (8, 8, 8, 32, 32, 2), 5)]
# the two table geometries (conv_cases.X6_TABLE) at B = 1, in a process WITHOUT the force
TABLE_CASES = [(0, (1, 32, 32, 64, 128, 2), 5), (0, (1, 64, 64, 32, 64, 2), 5)]

# epilogues per tile width and direction; statistics on both directions, every tile width, phases with empty tiles and without taps
EPI_CASES = [(0, (5, 8, 8, 32, 32, 1), 5), (1, (5, 8, 8, 32, 32, 1), 5), (0, (2, 8, 8, 64, 128, 1), 3), (1, (6, 9, 9, 128, 32, 2), 5),
             (0, (1, 8, 8, 96, 64, 1), 1), (1, (2, 16, 16, 64, 64, 2), 3)]
STATS_CASES = [(0, (5, 8, 8, 32, 32, 1), 5), (0, (2, 8, 8, 32, 192, 1), 3), (1, (6, 9, 9, 128, 32, 2), 5), (1, (2, 10, 10, 32, 32, 2), 1)]
# real-valued data: K = 32, 288 and 800, both directions
PRECISION_CASES = [(0, (4, 8, 8, 32, 64, 1), 1), (1, (4, 8, 8, 64, 32, 1), 1), (0, (4, 8, 8, 32, 64, 1), 3), (1, (4, 8, 8, 64, 32, 1), 3),
                   (0, (4, 8, 8, 32, 64, 1), 5), (1, (4, 8, 8, 64, 32, 1), 5)]
SCALING_CASES = [(0, (4, 8, 8, 32, 64, 1), 5), (1, (4, 16, 16, 64, 32, 2), 5)]
RECIPES = ("pieces", "dense", "decode")


def case_id(case):
    bwd, shape, k = case[:3]
    return ("dgrad-" if bwd else "fwd-") + CC.case_id(shape) + f"k{k}"


# ===================================================================================================================================
# data
# ===================================================================================================================================
def act_shape(bwd, shape):
    B, H, W, Ci, Co, s = shape
    return (B, CC.cdiv(H, s), CC.cdiv(W, s), Co) if bwd else (B, H, W, Ci)


def out_shape(bwd, shape):
    B, H, W, Ci, Co, s = shape
    return (B, H, W, Ci) if bwd else (B, CC.cdiv(H, s), CC.cdiv(W, s), Co)


def _impulse_sites(bwd, shape, k, seed):
    """Occupancy [B, Ha, Wa] of conv_cases.impulses for the activation of the case, the pixels beside its 128-row M-tile seams included.
    An output of the data gradient reads (k - 1) // s + 1 rows and columns of dy, so that is the distance its impulses keep."""
    B, H, W, Ci, Co, s = shape
    d = dict(family="conv_igemm", pos_major=False, BM=K_BM, mtiles=launch(bwd, shape, k)["mtiles"])
    rows, cols = CC.seams(bwd, B, H, W, Ci, Co, s, d)
    kk = (k - 1) // s + 1 if bwd else k
    occ = CC.impulses(act_shape(bwd, shape), rows, cols, seed, kk).sum(-1) != 0
    # then every pixel that still keeps the distance, in a seeded order: a stride-2 forward site reaches only the taps of its parity
    rng = np.random.default_rng([seed, 65, bwd, k, *shape])
    _, Ha, Wa = occ.shape
    for b in range(B):
        for q in rng.permutation(Ha * Wa):
            y, x = divmod(int(q), Wa)
            if not occ[b, max(0, y - kk + 1):y + kk, max(0, x - kk + 1):x + kk].any():
                occ[b, y, x] = True
    return occ


def _site_taps(bwd, shape, k, y, x):
    """The taps through which the activation pixel (y, x) reaches an output pixel."""
    B, H, W, Ci, Co, s = shape
    (Ho, pt), (Wo, pl) = CC.same_pads(H, k, s), CC.same_pads(W, k, s)
    if bwd:
        ok = lambda q, kk, pad, n: 0 <= q * s + kk - pad < n
        return {kh * k + kw for kh in range(k) if ok(y, kh, pt, H) for kw in range(k) if ok(x, kw, pl, W)}
    ok = lambda q, kk, pad, n: (q + pad - kk) % s == 0 and 0 <= (q + pad - kk) // s < n
    return {kh * k + kw for kh in range(k) if ok(y, kh, pt, Ho) for kw in range(k) if ok(x, kw, pl, Wo)}


def live_taps(bwd, shape, k):
    """The taps that read real data at some pixel (a one-row map leaves the other kernel rows to the padding)."""
    _, Ha, Wa, _ = act_shape(bwd, shape)
    return set().union(*[_site_taps(bwd, shape, k, y, x) for y in range(Ha) for x in range(Wa)])


def _deal_sites(bwd, shape, k, seed, G, cover=True):
    """-> (impulse sites [n, 3], the 16-channel k-slice of each).  A site goes to the k-slice that still lacks most of the taps it
    reaches (a corner reaches 9 of 25, a stride-2 forward site only the taps of its parity); the impulse seed is the first from
    `seed` on with which every (live tap, k-slice) feeds an output (cover=False: `seed` itself -- a 4 x 4 map holds one impulse)."""
    live = live_taps(bwd, shape, k)
    for trial in range(seed, seed + 64):
        sites = np.argwhere(_impulse_sites(bwd, shape, k, trial))
        seen = [set() for _ in range(G)]
        grp = np.zeros(len(sites), np.int64)
        for i, (b, y, x) in enumerate(sites):
            taps = _site_taps(bwd, shape, k, int(y), int(x))
            grp[i] = max(range(G), key=lambda g: (len(taps - seen[g]), -((g - i) % G)))
            seen[grp[i]] |= taps
        if not cover or all(sg == live for sg in seen):
            return sites, grp
    raise AssertionError(f"no impulse set reaches every (tap, k-slice) of {shape} k {k}")


def _piece_values(rng, shape):
    """+-(2^16 + m 2^6 + l 2^-4) with sign, m, l seeded per element -> (values, m, l)."""
    m, l = rng.integers(1, 4, shape), rng.integers(1, 4, shape)
    sign = 1.0 - 2.0 * rng.integers(0, 2, shape)
    return sign * (65536.0 + 64.0 * m + l / 16.0), m, l


def make(bwd, shape, k, recipe, seed=0, cover=True):
    """-> (activation [B, Ha, Wa, Ck], w [k, k, Cin, Cout]) in float64: x for the forward, dy for the data gradient."""
    B, H, W, Ci, Co, s = shape
    if recipe == "dense":
        x, w, dy = CC.dense(B, H, W, Ci, Co, s, "dgrad" if bwd else "fwd", seed + bwd, k)
        return (dy if bwd else x), w
    C = Co if bwd else Ci
    G = C // 16
    sites, grp = _deal_sites(bwd, shape, k, seed + bwd, G, cover)
    act = np.zeros(act_shape(bwd, shape))
    rng = np.random.default_rng([seed, 66, bwd, k, *shape])
    n = np.arange(len(sites))
    ch = 16 * grp + (n // G * 7 + n) % 16
    if recipe == "decode":
        act[sites[:, 0], sites[:, 1], sites[:, 2], ch] = 1.0
        return act, CC.decode_weights(Ci, Co, k)
    act[sites[:, 0], sites[:, 1], sites[:, 2], ch] = _piece_values(rng, len(sites))[0]
    return act, _piece_values(rng, (k, k, Ci, Co))[0]


def real_data(bwd, shape, k, seed=0):
    """uniform(-1, 1) operands as float32-representable float64."""
    B, H, W, Ci, Co, s = shape
    rng = np.random.default_rng([seed, 67, bwd, k, *shape])
    f = lambda sh: rng.uniform(-1, 1, sh).astype(np.float32).astype(np.float64)
    return f(act_shape(bwd, shape)), f((k, k, Ci, Co))


def conv(bwd, shape, act, w):
    """oracle.np_ops in the dtype of its operands."""
    return O.conv2d_bwd_data(act, w, shape[5], shape[1:3]) if bwd else O.conv2d_fwd(act, w, shape[5])


def expected(bwd, shape, act, w):
    """RNE(float64 oracle) as float64: the exact result on the integer recipes, the correctly rounded product on "pieces"."""
    return conv(bwd, shape, act, w).astype(np.float32).astype(np.float64)


def piece_convs(bwd, shape, act, w, lift=False, dtype=np.float64):
    """The nine convolutions of an activation piece with a weight piece: P[i][j] = conv(act piece i, w piece j)."""
    a, b = split3(act, lift), split3(w, lift)
    return [[conv(bwd, shape, a[i].astype(dtype), b[j].astype(dtype)) for j in range(3)] for i in range(3)]


def combine(P, coef):
    return sum(coef[i][j] * P[i][j] for i in range(3) for j in range(3) if coef[i][j])


def kept_coef():
    c = np.zeros((3, 3))
    for i, j in KEPT_TERMS:
        c[i, j] = 1
    return c


def mutants(one_term_only=False):
    """{name: 3 x 3 coefficients}: each kept term dropped; each doubled; the planes of an asymmetric term swapped (its mirror issued
    twice); mid.mid replaced by mid.lo / lo.mid."""
    out = {}
    nm = lambda i, j: f"{PIECES[i]}.{PIECES[j]}"
    for i, j in KEPT_TERMS:
        c = kept_coef(); c[i, j] = 0; out["drop " + nm(i, j)] = c
    if one_term_only:
        return out
    for i, j in KEPT_TERMS:
        c = kept_coef(); c[i, j] = 2; out["double " + nm(i, j)] = c
        if i != j:
            c = kept_coef(); c[i, j] = 0; c[j, i] = 2; out[f"{nm(j, i)} in place of {nm(i, j)}"] = c
    for i, j in ((1, 2), (2, 1)):
        c = kept_coef(); c[1, 1] = 0; c[i, j] = 1; out[f"{nm(i, j)} in place of mid.mid"] = c
    return out


def slice_tags(bwd, shape, k, act):
    """Per output pixel [B, Hd, Wd]: 1 + tap + k k (16-channel k-slice of the contraction) of the ONE impulse it reads, 0 for none."""
    B, H, W, Ci, Co, s = shape
    C = Co if bwd else Ci
    tag = 1.0 + np.arange(k * k).reshape(k, k, 1, 1) + k * k * (np.arange(C) // 16).reshape((1, 1, 1, C) if bwd else (1, 1, C, 1))
    return conv(bwd, shape, (act != 0).astype(np.float64), np.ascontiguousarray(np.broadcast_to(tag, (k, k, 1, C) if bwd else (k, k, C, 1))))[..., 0]


def claimed_tags(bwd, shape, k):
    """Every (tap that reads real data at some pixel, 16-channel k-slice of every K chunk) of the case, as slice_tags numbers them."""
    C = shape[4] if bwd else shape[3]
    return {1 + t + k * k * g for t in live_taps(bwd, shape, k) for g in range(C // 16)}


def adder_unit(amax, wmax):
    """What the matrix pipe's adder may take from an INTEGER result (tools/probes/mfma_tiny_accumulator.hip, MI355X): when the
    accumulator that enters v_mfma_f32_32x32x16_bf16 is a NEGATIVE lifted residue (-n 2^-126, the sum so far being 0) it is
    aligned to the largest product of the instruction and floored, not dropped: the result is the exact integer sum minus one unit
    in the last place of the adder, 2^-25 of the power of two above the largest product (c = -2^-125, products 3 x 3 ... -> S - 2^-22;
    a tiny PRODUCT beside large ones, of either sign, and a positive residue are dropped).  Once the accumulator holds that unit it
    is no residue any more, so a further unit can only come from an instruction with larger products: the units are powers of two
    and add up to less than twice the largest, 2 x 2^-25 x 2 max|a| max|w|."""
    return 2.0 ** -23 * amax * wmax


def compare(got, ref, K, amax, wmax, factor=1.0, adder=False):
    """None, or what is wrong: array_equal where the reference is nonzero, the lifted-zero bound where it is zero (times `factor`
    behind an epilogue that multiplies the accumulator: 3 for the settings of epilogue_data -- |multiplier| <= 3, dropout scale 2).
    adder=True (the integer recipes, whose partial sums pass through 0 again and again): |got - ref| <= adder_unit on top of that --
    a wrong tap, pixel or channel moves an integer output by at least 1."""
    nz = ref != 0
    slack = factor * adder_unit(amax, wmax) if adder else 0.0
    with np.errstate(invalid="ignore"):
        bad = nz & ~(np.abs(got - ref) <= slack)
        badz = ~nz & ~(np.abs(got) <= factor * lifted_zero_bound(K, amax, wmax) + slack)
    if not bad.any() and not badz.any():
        return None
    if bad.any():
        return dict(mask=bad, zero=False, n=int(bad.sum()), nz=int(badz.sum()))
    return dict(mask=badz, zero=True, n=0, nz=int(badz.sum()))


def locate(bwd, shape, k, act, idx):
    """(kh, kw, contraction channel) of the impulse that output pixel idx = (b, h, w) reads, or None."""
    B, H, W, Ci, Co, s = shape
    p = CC.gather_params(bwd, B, H, W, Ci, Co, k, s)
    b, h, w = idx
    if bwd:
        g = p["ph"][(h % s) * s + (w % s)]
        ay, ax = h // s, w // s
    else:
        g = p["ph"][0]
        ay, ax = h * s, w * s
    for (dy, dx, wi) in g["taps"]:
        y, x = ay + dy, ax + dx
        if 0 <= y < p["Hs"] and 0 <= x < p["Ws"] and act[b, y, x].any():
            return wi // k, wi % k, int(np.flatnonzero(act[b, y, x])[0])
    return None


def piece_digits(v):
    """A value of the "pieces" recipe -> (hi.hi count, first-order digit, second-order digit) or None."""
    q = abs(float(v)) / 4096.0
    if not np.isfinite(q) or q != int(q):
        return None
    q = int(q)
    return q >> 20, (q >> 10) & 1023, q & 1023


def describe_wrong(bwd, shape, k, recipe, act, w, got, ref, res):
    """Text for a failed compare(): counts, the first wrong output, the (tap, ci, co) it came from, and for "pieces" the cross terms
    its digits hold."""
    i = tuple(int(v) for v in np.argwhere(res["mask"])[0])
    txt = (f"{res['n']} of {int((ref != 0).sum())} nonzero outputs wrong, {res['nz']} of {int((ref == 0).sum())} zero outputs past the lifted-zero bound, "
           f"{int(np.isnan(got).sum())} never written; first at (b, h, w, n)={i}: got {got[i]!r}, expected {ref[i]!r}")
    src = locate(bwd, shape, k, act, i[:3])
    if src is None:
        return txt + "; no impulse in its window"
    kh, kw, c = src
    ci, co = (i[3], c) if bwd else (c, i[3])
    txt += f"; its window holds (kh, kw, ci, co)=({kh}, {kw}, {ci}, {co})"
    if recipe == "decode":
        txt += f"; got weight {CC.decode_weight(got[i], shape[3], k)}"
    if recipe == "pieces":
        g, e = piece_digits(got[i]), piece_digits(ref[i])
        if g is None:
            return txt + "; not a multiple of 2^12: an omitted term or a foreign value was added"
        names = ("hi.hi", "hi.mid + mid.hi (m_a + m_b)", "hi.lo + lo.hi + mid.mid (l_a + l_b + m_a m_b)")
        txt += "; digits got / expected: " + ", ".join(f"{n} {a} / {b}" + (" WRONG" if a != b else "") for n, a, b in zip(names, g, e))
    return txt


# ===================================================================================================================================
# epilogue and statistics data (the settings of conv_cases.epilogue_ref)
# ===================================================================================================================================
def epilogue_data(bwd, shape, k, z):
    """Integer bias and multipliers, a dropout mask, a LeakyReLU-gradient reference with zeros, keep_elems short of the last sample."""
    rng = np.random.default_rng([9, bwd, k, *shape])
    N = z.shape[-1]
    return dict(bias=rng.integers(-5, 6, N).astype(np.float64), mul=rng.integers(-3, 4, N).astype(np.float64),
                keep=(rng.uniform(size=z.shape) >= 0.5).astype(np.uint8), ref_act=rng.integers(-2, 3, z.shape).astype(np.float64),
                keep_elems=(shape[0] - 1) * z[0].size if shape[0] > 1 else z.size // 2 // 4 * 4)
