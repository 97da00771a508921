"""Case table, exact integer data, float64 reference and restated host predicates for the blur kernels of csrc/blur.hip and
csrc/blur_panel.hip (tests/test_blur_cases_cpu.py checks the table on the CPU, tests/test_blur_exact_gpu.py runs it on the GPU).

The method is the one of tests/misc_cases.py: on integer taps and integer pixels whose products sum to less than 2^24 in both
passes, every partial sum in every order -- with or without fused multiply-add, through any MFMA blocking -- is a float32 number,
so a correct kernel equals the float64 reference bit for bit and a dropped, doubled, reversed or mis-paired tap moves an output
by at least 1.  The taps go straight to bg_blur_nhwc_f32; the Gaussian policy is not involved and the taps are NOT symmetric
(include/bgan.h promises n_taps floats, nothing about symmetry).

Two recipes:
  dense     taps i.i.d. from +-{1,2,3} (no zero: a zero tap hides its pairing), redrawn until t != t[::-1]; pixels integers in
            [-m, m], m = min(8, (2^24 - 1) // (sum|t|)^2).  Bound: (sum|t|)^2 m < 2^24 covers both passes.
            For T <= 65 the ramp taps below also serve dense pixels in [-3, 3] ("ramp"): (T (T + 1) / 2)^2 3 <= 2145^2 3 < 2^24.
  impulse   taps t[j] = j + 1, all distinct; the image is zero but for at most 64 ones per image, at the corners, on either side
            of the row-block / column-tile seams of the case's route, the rest seeded at random.  An output is a sum of
            (a + 1)(b + 1) over the impulses in reach, so a wrong value names the (tap, pixel) pair it came from (decode()).
            Bound: 64 T^2 < 2^24, T <= 511.

Convention (oracle.np_ops.blur_1d_axis): out[n] = sum_j t[j] x[n + j - T // 2], zero padding, along H then along W.

The predicates restate the host code; each cites the lines it restates.  The switches blur.hip reads into `static const` variables
(BG_BLUR_STRIP_MIN_SIZE 65, BG_BLUR_STRIP_MAX_TAPS 65, BG_BLUR_MFMA_MIN_TAPS 13, BG_BLUR_BANDT_MIN_TAPS 13, BG_BLUR_PANEL_MIN_TAPS 67,
BG_BLUR_PANEL16_MAX_TAPS 208, BG_BLUR_COLS_WAVES 2048) cannot be toggled inside one process: their defaults are restated and they are
not used.  BG_BLUR_NO_ROWS, BG_BLUR_NO_PANEL, BG_BLUR_PANEL16 and BG_BLUR_BAND_LD are read per call and appear in the `env` of a case.

Not reachable at test sizes, and therefore not in the table: the band passes' 64-bit loader by its natural condition (an image of
2^29 floats or more; BG_BLUR_BAND_LD=0 forces it instead) and the `band_ok` / strip guards of blur_path (2^31 / 2^29 floats).
"""
import numpy as np

from oracle import np_ops as O

TWO24 = 1 << 24
STATIC_SWITCHES = ("BG_BLUR_STRIP_MIN_SIZE", "BG_BLUR_STRIP_MAX_TAPS", "BG_BLUR_MFMA_MIN_TAPS", "BG_BLUR_BANDT_MIN_TAPS",
                   "BG_BLUR_PANEL_MIN_TAPS", "BG_BLUR_PANEL16_MAX_TAPS", "BG_BLUR_COLS_WAVES")
CALL_SWITCHES = ("BG_BLUR_NO_ROWS", "BG_BLUR_NO_PANEL", "BG_BLUR_PANEL16", "BG_BLUR_BAND_LD")


def cdiv(a, b):
    return -(-a // b)


def up(a, m):
    return cdiv(a, m) * m


# ------------------------------------------------------------------ host predicates, restated
K_TZ_PAD = 64                 # blur.hip:113 kTzPad
FUSED_LDS_CAP = 150 * 1024    # blur.hip:1329 kFusedLdsCap
ROWS_BLOCK = 32               # blur.hip:207 kRowsBlock
BT_ROWS, BT_PAD_LO, BT_PAD_HI = 128, 128, 208     # blur.hip:403
K_SP = 32                     # blur.hip:749 kSP
K_STRIP_W, K_R = 64, 4        # blur.hip:1197, :30
PANEL_PAD, PANEL_PITCH_PAD, PANEL_STAGE_PITCH = 64, 1, 100    # blur_panel.hip:29, :33, :31


def rows_geom(H, W, C, T):
    """blur.hip:214-231 rows_pitch / rows_geom."""
    pitch = lambda q, r: q + ((r - q) & 63)
    half = T >> 1
    Q, Wp = W * C, up(W, 32)
    Qp = up(Wp * C, 32)
    pX, pY, pZ = pitch(Qp, 16), pitch(Qp, 4), pitch(Qp, 4)
    nb = cdiv(H, ROWS_BLOCK)
    src = max(min(H, rb * ROWS_BLOCK + ROWS_BLOCK + half) - max(0, rb * ROWS_BLOCK - half) for rb in range(nb))
    rows = (src + 3) & ~3
    xfloats = (max(rows * pX, ROWS_BLOCK * pZ) + 3) & ~3
    lds = (xfloats + ((ROWS_BLOCK * pY + 3) & ~3) + T + 2 * K_TZ_PAD) * 4
    return dict(Q=Q, Wp=Wp, Qp=Qp, nb=nb, src_rows=src, xfloats=xfloats, lds=lds)


def mfma_lds_bytes(H, W, C, T):
    """blur.hip:1384-1385 (and :1444-1445): the whole-image MFMA kernel's planes, padded to 32 x 32 tiles."""
    Hp, Wp = up(H, 32), up(W, 32)
    return (2 * C * Hp * (Wp + 1) + T + 2 * K_TZ_PAD) * 4


def fused_lds_bytes(H, W, C):
    """blur.hip:1328."""
    return (2 * ((H * W * C + 3) & ~3) + 512) * 4


def panel_lds_bytes(W, T):
    """blur_panel.hip:452-455."""
    return (32 * (3 * W + PANEL_PITCH_PAD) + ((T + 2 * PANEL_PAD + 3) & ~3) + (W // 32) * 16 * PANEL_STAGE_PITCH + 4) * 4


def panel16_lds_bytes(W, T):
    """blur_panel.hip:435-437."""
    return (16 * (3 * W + PANEL_PITCH_PAD) + ((T + 2 * PANEL_PAD + 3) & ~3) + (W // 32) * 8 * PANEL_STAGE_PITCH + 4) * 4


def blur_panel_ok(B, H, W, C, T):
    """blur_panel.hip:429-433."""
    if C != 3 or W % 32 or H % 32 or W > 256 or H > 512 or W < 32 or B <= 0:
        return False
    if T < 3 or not T & 1 or T > 1023:
        return False
    return panel_lds_bytes(W, T) <= 160 * 1024 - 512


def panel16_on(H, W, T, env=None):
    """blur_panel.hip:445-450 and the LDS condition of :460 / :490: True = blur_panel16_kernel, False = blur_panel_kernel."""
    sw = int((env or {}).get("BG_BLUR_PANEL16", "1"))
    return sw != 0 and T <= 208 and H % 16 == 0 and H // 16 <= 32 and panel16_lds_bytes(W, T) <= 160 * 1024 - 512


def blur_path(B, H, W, C, T, env=None):
    """blur.hip:1376-1402."""
    env = env or {}
    if C in (1, 3) and (W * C) & 3 == 0 and T <= 65 and (H >= 65 or W >= 65) and H * W * C < 1 << 29:
        return 4
    rows_ok = H <= 64 and W <= 64 and C <= 4 and (W * C) & 3 == 0
    if "BG_BLUR_NO_ROWS" not in env and rows_ok and T >= 13 and rows_geom(H, W, C, T)["lds"] <= 80 * 1024:
        return 5
    if H <= 64 and W <= 64 and C <= 16 and T >= 13 and mfma_lds_bytes(H, W, C, T) <= FUSED_LDS_CAP:
        return 0
    fused_fits = fused_lds_bytes(H, W, C) <= FUSED_LDS_CAP and T <= 500
    band_ok = C <= 4 and B * H * W * C < 1 << 31
    if band_ok and T >= 67 and (H > 64 or W > 64) and blur_panel_ok(B, H, W, C, T) and "BG_BLUR_NO_PANEL" not in env:
        return 6
    if fused_fits and not (band_ok and T >= 31 and (H > 64 or W > 64)):
        return 1
    return 2 if band_ok else 3


def workspace_bytes(B, H, W, C, T, env=None):
    """blur.hip:1404-1408."""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0:
        return 0
    return B * H * W * C * 4 if blur_path(B, H, W, C, T, env) in (2, 3) else 0


def blur3_supported(B, H, W, C, T, env=None):
    """blur.hip:1533-1542."""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0 or T < 1 or not T & 1:
        return False
    if blur_path(3 * B, H, W, C, T, env) == 5:
        return True
    return ("BG_BLUR_NO_ROWS" not in (env or {}) and H <= 64 and W <= 64 and C <= 4 and (W * C) & 3 == 0 and T >= 3
            and rows_geom(H, W, C, T)["lds"] <= 80 * 1024)


def launch_cols(B, H, W, C, T):
    """blur.hip:992-1018 (launch_cols, launch_cols_c) with ColsCfg :798-813."""
    reach = T >> 1
    P = 4 if reach <= 4 else 8 if reach <= 8 else 16
    pxo = 16 if C == 3 else 48
    strips = cdiv(W, pxo)
    segs = min(max(1, cdiv(2048, B * strips)), max(1, H // 32))
    seg_rows = cdiv(cdiv(H, segs), 16) * 16
    segs = cdiv(H, seg_rows)
    wpi = (strips * segs + 3) // 4
    return dict(P=P, pxo=pxo, strips=strips, segs=segs, seg_rows=seg_rows, grid=8 * cdiv(B, 8) * wpi)


def launch_strip(B, H, W, C, T):
    """blur.hip:1322-1326 launch_strip_c and the grid of :1455-1456."""
    strips = cdiv(W, K_SP)
    return dict(P=24 if (T >> 1) <= 24 else 32, strips=strips, grid=8 * cdiv(B, 8) * strips)


def launch_band_t(B, R, S, C, T, aligned=True, env=None):
    """blur.hip:717-728 with BandCfg :410-421: loader (2 float4, 1 dword, 0 64-bit), row groups of 128, column groups of PXW pixels."""
    pxw = (3 if C == 3 else 4) * 32 // C
    ld = 0 if R * S * C >= 1 << 29 else 2 if (S * C) & 3 == 0 and aligned else 1
    if env and "BG_BLUR_BAND_LD" in env:
        ld = min(ld, max(0, int(env["BG_BLUR_BAND_LD"])))
    return dict(ld=ld, rgs=cdiv(R, BT_ROWS), cgs=cdiv(S, pxw), pxw=pxw, lds=(((T + BT_PAD_LO + BT_PAD_HI + 3) & ~3) + (3 if C == 3 else 4) * 2 * 32 * 40) * 4)


def launch_lines(H, W, C, T):
    """blur.hip:1502-1505: the line kernels while both of their LDS tiles fit 140 KB, else the generic pass."""
    WC = W * C
    lds_h = (H * K_STRIP_W + T + K_R + 4) * 4
    rows_per = min(8, max(1, (48 * 1024 // 4) // WC))
    lds_w = (rows_per * WC + T + K_R + 4) * 4
    return dict(kind="lines" if lds_h <= 140 * 1024 and lds_w <= 140 * 1024 else "pass", rows_per=rows_per, lds_h=lds_h, lds_w=lds_w,
                strips=cdiv(WC, K_STRIP_W))


def panel_clips(n, half, block):
    """Which sides of its band each row block of `block` rows loses to the image edge (blur_panel.hip:415-423 band_ranges16 /
    band_ranges): the set of 'none' / 'lo' / 'hi' / 'both' over the blocks."""
    out = set()
    for rb in range(n // block):
        lo, hi = block * rb - half < 0, block * rb + block + half > n
        out.add("both" if lo and hi else "lo" if lo else "hi" if hi else "none")
    return out


FAMILY = {0: "mfma", 1: "fused", 2: "band", 3: "lines", 4: "cols", 5: "rows", 6: "panel"}
NAMES = {"fused": ["blur_fused"], "mfma": ["blur_mfma"], "rows": ["blur_rows"], "cols": ["blur_cols"], "strip": ["blur_strip"],
         "panel": ["blur_panel"], "band": ["blur_band_t1", "blur_band_t2"], "lines": ["blur_lines_h", "blur_lines_w"],
         "pass": ["blur_pass_h", "blur_pass_w"], "rows3": ["blur_rows3"]}


def describe(shape, T, env=None):
    """Route and loop shape of bg_blur_nhwc_f32 on a 16-byte-aligned x / scratch image: family, launch names (the first argument of
    bg::Launch, blur.hip:1428-1530) and the properties the case table claims."""
    B, H, W, C = shape
    path = blur_path(B, H, W, C, T, env)
    d = dict(path=path, family=FAMILY[path], C=C, B=B, n4=(H * W * C) % 4 == 0)
    if path == 1:
        d.update(hw4=H % 4 == 0 and W % 4 == 0, big=H > 64 or W > 64)
    elif path == 0:
        d.update(padded=H % 32 != 0 or W % 32 != 0, lds=mfma_lds_bytes(H, W, C, T))
    elif path == 5:
        g = rows_geom(H, W, C, T)
        d.update(nb=g["nb"], last_rows=H - 32 * (g["nb"] - 1), col_pad=g["Wp"] != W, src4=g["src_rows"] % 4 == 0, lds=g["lds"])
    elif path == 4:
        if (T >> 1) <= 16:
            d.update(launch_cols(B, H, W, C, T))
            d.update(partial_strip=W % d["pxo"] != 0, h16=H % 16 == 0, idle=B % 8 != 0)
        else:
            d.update(launch_strip(B, H, W, C, T), family="strip")
            d.update(partial_strip=W % K_SP != 0, h32=H % 32 == 0)
    elif path == 2:
        p1, p2 = launch_band_t(B, H, W, C, T, env=env), launch_band_t(B, W, H, C, T, env=env)
        d.update(ld=(p1["ld"], p2["ld"]), rgs=(p1["rgs"], p2["rgs"]), cgs=(p1["cgs"], p2["cgs"]), pxw=p1["pxw"],
                 ragged_cg=(W % p1["pxw"] != 0, H % p1["pxw"] != 0), wide=T >= 67)
    elif path == 6:
        k16 = panel16_on(H, W, T, env)
        blk = 16 if k16 else 32
        d.update(k16=k16, wt=W // 32, clips=panel_clips(H, T >> 1, blk) | panel_clips(W, T >> 1, blk), wider=(T >> 1) >= min(H, W))
    else:
        d.update(launch_lines(H, W, C, T))
        d["family"] = d["kind"]
    d["names"] = NAMES[d["family"]]
    return d


# ------------------------------------------------------------------ the case table
# (shape, n_taps, claimed family, claimed instantiation / loop shape, env).  A claim is a subset of describe()'s answer.
def _c(shape, T, family, env=None, **claim):
    return (shape, T, family, claim, env or {})


CASES = [
    # blur_fused (path 1)
    _c((3, 8, 8, 3), 3, "fused", n4=True, hw4=True),
    _c((2, 5, 7, 3), 5, "fused", n4=False, hw4=False),
    _c((2, 28, 28, 1), 1, "fused"),
    _c((2, 9, 13, 5), 11, "fused", n4=False),
    _c((2, 66, 40, 2), 13, "fused", big=True),
    _c((1, 70, 36, 4), 29, "fused", big=True),
    # blur_mfma (path 0)
    _c((2, 30, 30, 1), 13, "mfma", padded=True, n4=True),
    _c((2, 31, 31, 3), 31, "mfma", padded=True, n4=False),
    _c((1, 40, 24, 5), 17, "mfma", padded=True),
    _c((1, 20, 20, 8), 21, "mfma", padded=True),
    _c((2, 64, 64, 4), 65, "mfma", padded=False),                       # the row-block kernel would need more than 80 KB
    _c((2, 32, 64, 3), 13, "mfma", {"BG_BLUR_NO_ROWS": "1"}, padded=False),
    # blur_rows (path 5)
    _c((2, 33, 64, 3), 13, "rows", nb=2, last_rows=1, col_pad=False, src4=False),
    _c((3, 28, 28, 1), 29, "rows", nb=1, col_pad=True, src4=True),
    _c((2, 17, 4, 1), 17, "rows", nb=1, col_pad=True, src4=False),
    _c((2, 60, 32, 4), 15, "rows", nb=2, col_pad=False),
    _c((2, 64, 64, 2), 65, "rows", nb=2, last_rows=32, src4=True),
    _c((1, 64, 64, 3), 129, "rows", nb=2, lds=79364),                   # a tap count beyond the policy's
    # blur_cols (path 4, reach <= 16): C x P, segs, partial strips, H % 16, idle workgroups
    _c((2, 66, 100, 3), 3, "cols", C=3, P=4, partial_strip=True, h16=False, idle=True),
    _c((9, 130, 68, 3), 13, "cols", C=3, P=8, partial_strip=True, B=9),
    _c((1, 96, 48, 3), 33, "cols", C=3, P=16, partial_strip=False, h16=True, B=1),
    _c((3, 72, 40, 1), 31, "cols", C=1, P=16, partial_strip=True),
    _c((2, 100, 48, 1), 17, "cols", C=1, P=8, partial_strip=False, h16=False),
    _c((2, 80, 20, 3), 7, "cols", C=3, P=4, h16=True),
    _c((1, 65, 4, 1), 1, "cols", C=1, P=4),
    _c((16, 70, 96, 1), 9, "cols", C=1, P=4, B=16, idle=False, partial_strip=False),
    _c((2, 40, 68, 3), 11, "cols", C=3, P=8, segs=1),
    _c((1, 48, 100, 1), 5, "cols", C=1, P=4, segs=1),
    # blur_strip (path 4, 35..65 taps): C x P, partial strips, H % 32
    _c((2, 66, 32, 3), 35, "strip", C=3, P=24, partial_strip=False, h32=False),
    _c((1, 100, 44, 3), 49, "strip", C=3, P=24, partial_strip=True),
    _c((3, 96, 80, 1), 49, "strip", C=1, P=24, partial_strip=True, h32=True),
    _c((2, 72, 40, 1), 51, "strip", C=1, P=32, partial_strip=True),
    _c((9, 70, 36, 3), 65, "strip", C=3, P=32, B=9, partial_strip=True),
    _c((1, 130, 100, 1), 65, "strip", C=1, P=32, h32=False),
    _c((1, 96, 64, 3), 51, "strip", C=3, P=32, partial_strip=False, h32=True),
    # blur_band_t (path 2)
    _c((1, 72, 33, 3), 73, "band", C=3, ld=(1, 2)),
    _c((1, 66, 67, 3), 31, "band", C=3, ld=(1, 1), wide=False),
    _c((1, 70, 35, 1), 33, "band", C=1, wide=False),
    _c((2, 66, 70, 2), 33, "band", C=2, ld=(2, 2), wide=False),
    _c((2, 130, 66, 2), 131, "band", C=2, ld=(2, 2), rgs=(2, 1), wide=True),
    _c((1, 136, 150, 4), 121, "band", C=4, ld=(2, 2), rgs=(2, 2), wide=True),
    _c((2, 150, 131, 1), 151, "band", C=1, ld=(1, 1), rgs=(2, 2), ragged_cg=(True, True)),
    _c((1, 129, 20, 4), 67, "band", C=4, rgs=(2, 1), wide=True),
    _c((2, 96, 96, 3), 73, "band", {"BG_BLUR_NO_PANEL": "1"}, C=3, ld=(2, 2), rgs=(1, 1), ragged_cg=(False, False)),
    _c((1, 140, 76, 1), 69, "band", {"BG_BLUR_BAND_LD": "0"}, C=1, ld=(0, 0)),
    _c((1, 68, 70, 2), 37, "band", {"BG_BLUR_BAND_LD": "0"}, C=2, ld=(0, 0)),
    _c((1, 100, 44, 3), 71, "band", {"BG_BLUR_BAND_LD": "0"}, C=3, ld=(0, 0)),
    _c((1, 66, 30, 4), 45, "band", {"BG_BLUR_BAND_LD": "0"}, C=4, ld=(0, 0)),
    # blur_panel16 / blur_panel (path 6)
    _c((1, 96, 32, 3), 97, "panel", k16=True, wt=1, wider=True),
    _c((2, 96, 96, 3), 73, "panel", k16=True, wt=3),
    _c((1, 64, 96, 3), 97, "panel", k16=True, wt=3),
    _c((9, 96, 64, 3), 97, "panel", k16=True, wt=2, B=9),
    _c((1, 256, 32, 3), 209, "panel", k16=False, wt=1),
    _c((1, 256, 32, 3), 255, "panel", k16=False, wt=1),
    _c((1, 512, 32, 3), 255, "panel", k16=False, wt=1),
    _c((8, 64, 256, 3), 67, "panel", k16=True, wt=8, B=8),
    _c((16, 96, 64, 3), 69, "panel", {"BG_BLUR_PANEL16": "0"}, k16=False, wt=2, B=16),
    _c((2, 64, 256, 3), 131, "panel", {"BG_BLUR_PANEL16": "0"}, k16=False, wt=8),
    # blur_lines_h/w and blur_pass (path 3, more than 4 channels)
    _c((1, 80, 72, 5), 13, "lines"),
    _c((1, 30, 200, 8), 31, "lines"),
    _c((1, 4, 4000, 5), 3, "lines", rows_per=1),
    _c((1, 200, 300, 5), 301, "lines"),
    _c((1, 64, 64, 16), 65, "lines"),                                   # past the whole-image MFMA kernel's LDS cap
    _c((3, 60, 72, 5), 15, "lines"),
    _c((1, 600, 8, 5), 9, "pass"),                                      # past the line kernel's 140 KB
    _c((2, 600, 8, 5), 5, "pass"),
]

# one case per family (the panel kernels and the band passes twice) for the isolation (NaN image) and run-twice tests: (shape, T, env)
PER_FAMILY = [((2, 66, 40, 2), 13, {}), ((2, 31, 31, 3), 31, {}), ((2, 33, 64, 3), 13, {}), ((9, 130, 68, 3), 13, {}), ((9, 70, 36, 3), 65, {}),
              ((2, 150, 131, 1), 151, {}), ((2, 96, 96, 3), 73, {"BG_BLUR_NO_PANEL": "1"}), ((9, 96, 64, 3), 97, {}),
              ((2, 64, 256, 3), 131, {"BG_BLUR_PANEL16": "0"}), ((3, 60, 72, 5), 15, {}), ((2, 600, 8, 5), 5, {})]

# bg_blur3_lerp_nhwc_f32: (B, H, W, C, T); below 13 taps only this entry point reaches blur_rows_kernel
CASES3 = [(2, 28, 28, 1, 3), (3, 28, 28, 1, 7), (2, 33, 64, 3, 13), (2, 64, 64, 3, 31), (1, 17, 4, 1, 17), (2, 60, 32, 4, 15),
          (2, 40, 24, 2, 5), (5, 8, 8, 3, 3)]
ALPHAS = (0.0, 0.25, 0.5, 0.75, 1.0)


def case_id(case):
    (B, H, W, C), T, fam, _, env = case
    return f"{fam}-{B}x{H}x{W}x{C}-T{T}" + "".join(f"-{k[8:]}={v}" for k, v in sorted(env.items()))


# Every cell the table has to hit: (name, predicate on describe()'s answer)
def _cells():
    cells = []
    add = lambda name, fn: cells.append((name, fn))
    fam = lambda f: (lambda d: d["family"] == f)
    both = lambda f, key, label=None: [add(f"{f}: {label or key} {v}", (lambda v: lambda d: d["family"] == f and d.get(key) == v)(v))
                                      for v in (True, False)]
    add("fused: T = 1", lambda d: d["family"] == "fused" and d["T"] == 1)
    both("fused", "n4", "n % 4 == 0")
    both("fused", "hw4", "H, W multiples of 4")
    for c in (1, 2, 3, 4, 5):
        add(f"fused: C = {c}", (lambda c: lambda d: d["family"] == "fused" and d["C"] == c)(c))
    for c in (2, 4):
        add(f"fused: larger than 64, C = {c}", (lambda c: lambda d: d["family"] == "fused" and d["big"] and d["C"] == c and d["T"] < 31)(c))
    both("mfma", "padded")
    both("mfma", "n4", "n % 4 == 0")
    for c in (1, 3, 4, 5, 8):
        add(f"mfma: C = {c}", (lambda c: lambda d: d["family"] == "mfma" and d["C"] == c)(c))
    add("mfma: BG_BLUR_NO_ROWS", lambda d: d["family"] == "mfma" and "BG_BLUR_NO_ROWS" in d["env"])
    for c in (1, 2, 3, 4):
        add(f"rows: C = {c}", (lambda c: lambda d: d["family"] == "rows" and d["C"] == c)(c))
    for nb in (1, 2):
        add(f"rows: {nb} row block(s)", (lambda nb: lambda d: d["family"] == "rows" and d["nb"] == nb)(nb))
    add("rows: last block of 1 row", lambda d: d["family"] == "rows" and d["nb"] == 2 and d["last_rows"] == 1)
    both("rows", "col_pad", "column padding")
    both("rows", "src4", "source rows % 4 == 0")
    add("rows: beyond the policy's tap counts", lambda d: d["family"] == "rows" and d["T"] == 129)
    for c in (1, 3):
        for p in (4, 8, 16):
            add(f"cols: C = {c}, P = {p}", (lambda c, p: lambda d: d["family"] == "cols" and d["C"] == c and d["P"] == p)(c, p))
        for p in (24, 32):
            add(f"strip: C = {c}, P = {p}", (lambda c, p: lambda d: d["family"] == "strip" and d["C"] == c and d["P"] == p)(c, p))
    add("cols: segs == 1", lambda d: d["family"] == "cols" and d["segs"] == 1)
    add("cols: segs > 1", lambda d: d["family"] == "cols" and d["segs"] > 1)
    both("cols", "partial_strip")
    both("cols", "h16", "H % 16 == 0")
    for b in (1, 9, 16):
        add(f"cols: B = {b}", (lambda b: lambda d: d["family"] == "cols" and d["B"] == b)(b))
    add("cols: T = 1", lambda d: d["family"] == "cols" and d["T"] == 1)
    both("strip", "partial_strip")
    both("strip", "h32", "H % 32 == 0")
    add("strip: B = 9", lambda d: d["family"] == "strip" and d["B"] == 9)
    for c in (1, 2, 3, 4):
        add(f"band: C = {c}", (lambda c: lambda d: d["family"] == "band" and d["C"] == c and "BG_BLUR_BAND_LD" not in d["env"])(c))
        add(f"band: C = {c}, loader 0 forced", (lambda c: lambda d: d["family"] == "band" and d["C"] == c and d["ld"] == (0, 0))(c))
    for ld in ((2, 2), (1, 1)):
        add(f"band: loaders {ld}", (lambda ld: lambda d: d["family"] == "band" and d["ld"] == ld)(ld))
    add("band: loaders mixed", lambda d: d["family"] == "band" and sorted(d["ld"]) == [1, 2])
    for n in (1, 2):
        add(f"band: {n} row group(s)", (lambda n: lambda d: d["family"] == "band" and n in d["rgs"])(n))
    add("band: ragged last column group", lambda d: d["family"] == "band" and any(d["ragged_cg"]))
    add("band: whole column groups", lambda d: d["family"] == "band" and not all(d["ragged_cg"]))
    both("band", "wide", "67 taps and more")
    add("band: RGB panel geometry, BG_BLUR_NO_PANEL", lambda d: d["family"] == "band" and "BG_BLUR_NO_PANEL" in d["env"] and d["C"] == 3)
    for wt in (1, 2, 3, 8):
        add(f"panel: W / 32 = {wt}", (lambda wt: lambda d: d["family"] == "panel" and d["wt"] == wt)(wt))
    add("panel: 16-row kernel", lambda d: d["family"] == "panel" and d["k16"])
    add("panel: 32-row kernel beyond 208 taps", lambda d: d["family"] == "panel" and not d["k16"] and d["T"] > 208)
    add("panel: 32-row kernel by BG_BLUR_PANEL16=0", lambda d: d["family"] == "panel" and not d["k16"] and d["T"] <= 208)
    add("panel: band clipped on one side", lambda d: d["family"] == "panel" and d["clips"] & {"lo", "hi"})
    add("panel: band clipped on both sides", lambda d: d["family"] == "panel" and "both" in d["clips"])
    add("panel: band wider than the image", lambda d: d["family"] == "panel" and d["wider"])
    for b in (1, 8, 9, 16):
        add(f"panel: B = {b}", (lambda b: lambda d: d["family"] == "panel" and d["B"] == b)(b))
    add("panel: 256 pixels wide", lambda d: d["family"] == "panel" and d["wt"] == 8)
    add("lines: line kernels", fam("lines"))
    add("lines: rows_per == 1", lambda d: d["family"] == "lines" and d["rows_per"] == 1)
    add("lines: rows_per > 1", lambda d: d["family"] == "lines" and d["rows_per"] > 1)
    add("lines: more taps than rows and columns", lambda d: d["family"] == "lines" and d["T"] > 300)
    add("lines: 16 channels past the MFMA kernel's LDS", lambda d: d["family"] == "lines" and d["C"] == 16)
    add("pass: generic pass", fam("pass"))
    return cells


CELLS = _cells()


def described(case):
    shape, T, _, _, env = case
    d = describe(shape, T, env)
    d.update(T=T, env=env)
    return d


def missing_cells(cases=None):
    ds = [described(c) for c in (CASES if cases is None else cases)]
    return [name for name, fn in CELLS if not any(fn(d) for d in ds)]


# ------------------------------------------------------------------ data
def dense_taps(T, rng):
    """i.i.d. from +-{1,2,3}, asymmetric (a single tap cannot be; T = 1 keeps its one value)."""
    while True:
        t = rng.choice([-3, -2, -1, 1, 2, 3], size=T).astype(np.float64)
        if T == 1 or not np.array_equal(t, t[::-1]):
            return t


def ramp_taps(T):
    return np.arange(1, T + 1, dtype=np.float64)


def dense_m(t):
    return min(8, (TWO24 - 1) // int(np.abs(t).sum()) ** 2)


def seams(case):
    """Rows and pixel columns that begin a block of the case's route, and (pixel, channel) pairs a tile boundary splits.
    The band passes transpose (pass 2 runs along W with H as its columns), so their seams apply to both axes."""
    (B, H, W, C), T, _, _, env = case
    d = describe((B, H, W, C), T, env)
    f = d["family"]
    every = lambda n, k: set(range(k, n, k))
    rows, cols, split_r, split_c = set(), set(), [], []
    if f in ("mfma", "rows"):
        rows, cols = every(H, 32), every(W, 16)
    elif f == "cols":
        rows, cols = every(H, 16) | every(H, d["seg_rows"]), every(W, 16) | every(W, d["pxo"])
    elif f == "strip":
        rows, cols = every(H, 16), every(W, 16) | every(W, K_SP)
    elif f == "band":
        rows, cols = every(H, 32) | every(H, d["pxw"]), every(W, 32) | every(W, d["pxw"])
        if C == 3:        # a 32-float tile of a 96-float group ends inside pixel 10 (floats 30 31 | 32) and pixel 21 (63 | 64 65)
            for n, out in ((W, split_c), (H, split_r)):
                for g in range(0, n, 32):
                    out += [(g + 10, 1), (g + 10, 2), (g + 21, 0), (g + 21, 1)]
    elif f == "panel":
        blk = 16 if d["k16"] else 32
        rows, cols = every(H, blk), every(W, 16)
    elif f == "lines":
        rows = every(H, d["rows_per"]) if d["rows_per"] > 1 else set()
        for q in range(K_STRIP_W, W * C, K_STRIP_W):           # blur_lines_h: strips of 64 floats of a row
            split_c += [divmod(q - 1, C), divmod(q, C)]
    return rows, cols, [p for p in split_r if p[0] < H], [p for p in split_c if p[0] < W]


def impulse_image(case, rng):
    """Zero but for at most 64 ones per image: corners, both sides of the seams (subsampled per image when there are more than
    fit), the rest at random; a random channel unless the seam is between channels."""
    (B, H, W, C), T, _, _, _ = case
    assert 64 * T * T < TWO24
    rows, cols, split_r, split_c = seams(case)
    x = np.zeros((B, H, W, C), np.float64)
    for b in range(B):
        pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
        cand = []
        for s in rows:
            cand += [(s - 1, int(rng.integers(W)), None), (s, int(rng.integers(W)), None)]
        for s in cols:
            cand += [(int(rng.integers(H)), s - 1, None), (int(rng.integers(H)), s, None)]
        cand += [(p, int(rng.integers(W)), c) for p, c in split_r] + [(int(rng.integers(H)), p, c) for p, c in split_c]
        want = min(60, H * W * C // 2)
        if len(cand) > want:
            cand = [cand[i] for i in rng.permutation(len(cand))[:want]]
        while len(cand) < want:
            cand.append((int(rng.integers(H)), int(rng.integers(W)), None))
        for h, w in pts:
            x[b, h, w, int(rng.integers(C))] = 1.0
        for h, w, c in cand:
            x[b, h, w, int(rng.integers(C)) if c is None else c] = 1.0
        assert x[b].sum() <= 64
    return x


def recipes(case):
    T = case[1]
    return ["dense", "impulse"] + (["ramp"] if T <= 65 else [])


def make(case, recipe, seed=0):
    """(x, taps) in float64 for one recipe; the bound of the recipe is asserted."""
    shape, T = case[0], case[1]
    rng = np.random.default_rng([seed, T, *shape, ["dense", "impulse", "ramp"].index(recipe)])
    if recipe == "dense":
        t = dense_taps(T, rng)
        m = dense_m(t)
        x = rng.integers(-m, m + 1, size=shape).astype(np.float64)
    elif recipe == "ramp":
        t, m = ramp_taps(T), 3
        x = rng.integers(-3, 4, size=shape).astype(np.float64)
    else:
        t = ramp_taps(T)
        return impulse_image(case, rng), t
    assert m >= 1 and int(np.abs(t).sum()) ** 2 * m < TWO24
    return x, t


def blur_axis(x, t, axis, descending=False):
    """blur_1d_axis in x's dtype with a chosen tap order (the float32 exactness proof sums in two orders)."""
    T, half, n = len(t), len(t) // 2, x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (half, half)
    xp = np.pad(x, pad)
    out = np.zeros_like(x)
    for j in (range(T - 1, -1, -1) if descending else range(T)):
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(j, j + n)
        out = out + x.dtype.type(t[j]) * xp[tuple(sl)]
    return out


def reference(x, t):
    """float64: oracle.np_ops.blur_1d_axis along H, then along W, same taps."""
    return O.blur_1d_axis(O.blur_1d_axis(np.asarray(x, np.float64), np.asarray(t, np.float64), 1), np.asarray(t, np.float64), 2)


def f32_two_orders(x, t):
    x32 = x.astype(np.float32)
    a = blur_axis(blur_axis(x32, t, 1), t, 2)
    b = blur_axis(blur_axis(x32, t, 2, descending=True), t, 1, descending=True)
    return a, b


def make3(case3, seed=0):
    """f, r multiples of 4 in [-8, 8], alpha from ALPHAS: r + a (f - r) is an integer in [-8, 8], exact with or without
    contraction (a (f - r) is an integer of at most 16, the sum one of at most 8)."""
    B, H, W, C, T = case3
    rng = np.random.default_rng([seed, 3, B, H, W, C, T])
    t = dense_taps(T, rng)
    assert int(np.abs(t).sum()) ** 2 * 8 < TWO24
    f = 4.0 * rng.integers(-2, 3, size=(B, H, W, C))
    r = 4.0 * rng.integers(-2, 3, size=(B, H, W, C))
    a = np.array([ALPHAS[(i + seed) % len(ALPHAS)] for i in range(B)])
    return f, r, a, t


def reference3(f, r, a, t):
    xhat = r + a[:, None, None, None] * (f - r)
    return np.concatenate([reference(f, t), reference(r, t), reference(xhat, t)], 0)


def decode(x, t, got, ref):
    """The first wrong output of an impulse case, spelled out: the (tap along H, tap along W) pairs it should have summed and,
    where its value is a single product of two ramp taps, the pairs that value corresponds to."""
    bad = np.argwhere(np.asarray(got, np.float64) != ref)
    if not len(bad):
        return "equal"
    b, h, w, c = (int(v) for v in bad[0])
    T, half = len(t), len(t) // 2
    want = [(int(hh - h + half), int(ww - w + half)) for hh, ww in np.argwhere(x[b, :, :, c] != 0)
            if 0 <= hh - h + half < T and 0 <= ww - w + half < T]
    g = float(np.asarray(got, np.float64)[b, h, w, c])
    if np.isfinite(g) and g == int(g) and 0 < g <= T * T:
        seen = [(a - 1, int(g) // a - 1) for a in range(1, T + 1) if int(g) % a == 0 and int(g) // a <= T]
    else:
        seen = "no single pair"
    return (f"{len(bad)} of {ref.size} wrong; first at [b {b}, h {h}, w {w}, c {c}]: got {g}, want {ref[b, h, w, c]}; taps (jh, jw) it "
            f"should sum: {want[:8]}; pairs its value is the product of: {seen if isinstance(seen, str) else seen[:8]}")
