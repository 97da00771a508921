"""Case tables, exact integer data, float64 reference and restated host dispatch for the k x k convolutions of csrc/conv_igemm.hip,
csrc/conv_c16.hip, csrc/conv_rows.hip and csrc/conv_wgrad.hip.  The tables of this file are the 5x5 ones (tests/test_conv_cases_cpu.py
checks them on the CPU, tests/test_conv_exact_gpu.py runs them on the GPU); tests/conv_ksize_cases.py holds the tables at k = 3 and 1
on the same functions.  A case shape is (B, H, W, Cin, Cout, stride) with an optional seventh element k; without it k = 5 (ksize).

The method is the one of tests/misc_cases.py and tests/blur_cases.py.  The conv contractions are fp32 arithmetic
(v_mfma_f32_32x32x2_f32 and plain FMAs): on integer operands whose products sum to less than 2^24 every
partial sum in every order -- per MFMA block, per split-K slab, per cross-wave reduction, with or without fused multiply-add -- is a
float32 number, so a correct kernel equals the float64 oracle bit for bit and a dropped, doubled or misplaced tap moves an output
by at least 1.

Two recipes per case:
  dense     x, w, dy integers in [-m, m], m = min(3, isqrt((2^24 - 1) // K)) with K the contraction length (k k Cin forward,
            k k Cout data gradient, M = B Ho Wo filter gradient): K m^2 < 2^24.
  decode    forward / data gradient: the activation is one-hot in the channel at impulses at Chebyshev distance >= k from each
            other (no output window holds two; at k = 1 every pixel may hold one), placed at the four corners, on both sides of
            the tile / strip seams of the case's route, then a seeded fill, a different set per image; the weights are
            1 + tap + k k (ci + Cin co), all distinct and < 2^24 up to 512 x 512 channels at k = 5.  Every output is ONE weight or
            0, so a wrong output names the (tap, ci, co) that reached it (decode_weight).
            filter gradient: x dense in [-3, 3]; every dy channel is zero but for at most 7 pixels that hold 8^0 .. 8^6 -- at the
            first and last pixel, on both sides of the split (chunk) seams, of the 32-pixel steps and of the image seams, the
            rest seeded.  dw[tap, ci, co] = sum_j x[pixel_j + tap, ci] 8^j is a balanced base-8 number whose digit j is the x
            value pixel j of channel co fed, so a wrong element names the pixel (decode_wgrad).  Bound: 3 (8^7 - 1) / 7 < 2^24.

Convention (oracle.np_ops): w is [kh, kw, ci, co]; the forward takes wT [tap][co][ci], the data gradient w [tap][ci][co].

The restatements cite the C++ they follow.  The tuning switches the library reads once into `static const` variables (BG_NO_C16,
BG_NO_ROWS, BG_WGRAD_NO_STRIP, BG_WGRAD_NO_TC, BG_WGRAD_NO_TG, BG_WGRAD_TARGET, BG_WGRAD_SWZ*, BG_NO_POS_MAJOR, BG_POS_MAJOR_MAX,
BG_NO_TILE_SORT, BG_NO_XCD_SWIZZLE, BG_PMERGE, BG_MFAST, BG_IGEMM_TILE, BG_IGEMM_BK, BG_SPLITK_*, BG_NO_THIN_N_MFMA,
BG_NO_THIN_N_ALL, BG_ROWS_R, BG_ROWSG_R, BG_CONV_X6_FORCE) cannot be toggled inside one process.  The five that take a 5x5-only fast
path away (SWITCHED_ENV) are read here the way the library reads them -- once, from the environment of the process (OFF) -- so the
restatement follows them; tests/conv_switched_child.py, started as a FRESH process with them set, runs the fallbacks they expose
(SWITCHED_ROUTES / SWITCHED_WGRAD).  The others are tuning aids: their defaults are restated and they must not be set.
"""
import math
import os

import numpy as np

from oracle import np_ops as O

TWO24 = 1 << 24
K5 = 5
STATIC_SWITCHES = ("BG_NO_C16", "BG_NO_ROWS", "BG_WGRAD_NO_STRIP", "BG_WGRAD_NO_TC", "BG_WGRAD_NO_TG", "BG_WGRAD_TARGET", "BG_WGRAD_SWZ",
                   "BG_WGRAD_SWZ_TG", "BG_NO_POS_MAJOR", "BG_POS_MAJOR_MAX", "BG_NO_TILE_SORT", "BG_NO_XCD_SWIZZLE", "BG_PMERGE", "BG_MFAST",
                   "BG_IGEMM_TILE", "BG_IGEMM_BK", "BG_SPLITK_MIN_WGS", "BG_SPLITK_TARGET", "BG_SPLITK_FORCE", "BG_NO_THIN_N_MFMA",
                   "BG_NO_THIN_N_ALL", "BG_ROWS_R", "BG_ROWSG_R", "BG_CONV_X6_FORCE")


SWITCHED_ENV = {"BG_NO_C16": "1", "BG_NO_ROWS": "1", "BG_WGRAD_NO_STRIP": "1", "BG_WGRAD_NO_TC": "1", "BG_WGRAD_NO_TG": "1"}
OFF = frozenset(k for k in SWITCHED_ENV if k in os.environ)      # getenv(...) ? 1 : 0, once per process, as in the library


def cdiv(a, b):
    return -(-a // b)


def ksize(case):
    """The kernel size of a case shape (B, H, W, Cin, Cout, stride[, k]): the optional seventh element, 5 without it."""
    return case[6] if len(case) > 6 else K5


def same_pads(n, k, s):
    """conv_common.h:71-77."""
    o = cdiv(n, s)
    return o, max((o - 1) * s + k - n, 0) // 2


# ===================================================================================================================================
# forward / data gradient: host dispatch, restated
# ===================================================================================================================================
K_DG_CK = 32                                             # conv_c16.hip:42 kDgCk
K_RG_HALO = 16                                           # conv_rows.hip:306 kRgHalo
K_TN_COLS, K_TN_PX = 64, 80                              # conv_igemm.hip:702 kTnCols, kTnPx
K_TK_TH, K_TK_TW, K_TK_MAX_KF = 8, 16, 104               # conv_igemm.hip:816


def gather_params(bwd, B, H, W, Ci, Co, k, s):
    """conv_common.h:80-117 make_fwd_params / make_bwd_data_params; a tap is (dy, dx, wi)."""
    Ho, pt = same_pads(H, k, s)
    Wo, pl = same_pads(W, k, s)
    if not bwd:
        taps = [(kh - pt, kw - pl, kh * k + kw) for kh in range(k) for kw in range(k)]
        return dict(B=B, Hs=H, Ws=W, Ck=Ci, Hd=Ho, Wd=Wo, N=Co, ss=s, ds=1, ph=[dict(Ha=Ho, Wa=Wo, py=0, px=0, taps=taps)])
    ph = []
    for py in range(s):
        for px in range(s):
            taps = [((py + pt - kh) // s, (px + pl - kw) // s, kh * k + kw)
                    for kh in range(k) if (py + pt - kh) % s == 0 for kw in range(k) if (px + pl - kw) % s == 0]
            ph.append(dict(Ha=(H - py + s - 1) // s, Wa=(W - px + s - 1) // s, py=py, px=px, taps=taps))
    return dict(B=B, Hs=Ho, Ws=Wo, Ck=Co, Hd=H, Wd=W, N=Ci, ss=1, ds=s, ph=ph)


def max_phase_m(p):
    """conv_igemm.hip:1161-1165."""
    return max(p["B"] * g["Ha"] * g["Wa"] for g in p["ph"])


def plan_splitk(p, bm, bn):
    """conv_igemm.hip:1210-1239 with the default thresholds (512 / 768 workgroups)."""
    nph = len(p["ph"])
    wgs = cdiv(max_phase_m(p), bm) * cdiv(p["N"], bn) * nph
    plan_bk = 32 if p["Ck"] % 32 == 0 else 16
    min_steps = min(len(g["taps"]) * (p["Ck"] // plan_bk) for g in p["ph"])
    min_wgs, tgt_wgs = 512, 768
    maxpos = max(g["Ha"] * g["Wa"] for g in p["ph"])
    skipping = maxpos <= 16 and p["B"] >= bm and p["B"] % bm == 0
    if skipping and min_wgs <= wgs <= 2 * min_wgs and min_steps >= 64:
        ks = max(1, 2 * min_wgs // wgs)
        return max(1, min(ks, min_steps // 32))
    if wgs >= 2 * min_wgs or min_steps < 32:
        return 1
    if wgs >= min_wgs:
        return 2 if min_steps >= 200 else 1
    ks = min(8, cdiv(tgt_wgs, wgs))
    return max(min(ks, min_steps // 16), 1)


def splitk_workspace_bytes(bwd, B, H, W, Ci, Co, k, s):
    """conv_igemm.hip:1571-1581 bg_conv2d_splitk_workspace_bytes."""
    p = gather_params(bwd, B, H, W, Ci, Co, k, s)
    if p["Ck"] % 16 or p["N"] <= 4:
        return 0
    ks = plan_splitk(p, 128, 32) if p["N"] <= 32 else plan_splitk(p, 64, 64)
    return ks * p["B"] * p["Hd"] * p["Wd"] * p["N"] * 4 if ks > 1 else 0


def _live(p, g, ay, ax):
    """Taps of phase g that read real data at anchor (ay, ax) (conv_igemm.hip:1199-1202, :1318-1320)."""
    sy, sx = ay * p["ss"], ax * p["ss"]
    return sum(1 for (dy, dx, _) in g["taps"] if 0 <= sy + dy < p["Hs"] and 0 <= sx + dx < p["Ws"])


def igemm_plan(p, stats=False, workspace=True):
    """conv_igemm.hip:1242-1360 launch_igemm, :1362-1369 dispatch_igemm and the K-step choice of run_gather (:1404), for a plain call
    (no bias / activation) that is given the split-K workspace it asks for (workspace=True) or none."""
    BM, BN = (128, 32) if p["N"] <= 32 else (64, 64)
    BK = 32 if p["Ck"] % 32 == 0 and p["Ck"] > 64 else 16
    nph, ph, B, N, Ck = len(p["ph"]), p["ph"], p["B"], p["N"], p["Ck"]
    Mmax = max_phase_m(p)
    ks = plan_splitk(p, BM, BN) if workspace else 1
    maxpos = max(g["Ha"] * g["Wa"] for g in ph)
    pos_major = maxpos <= 64 and B >= BM and B % BM == 0
    mtiles, ntiles = cdiv(Mmax, BM), cdiv(N, BN)
    pmerge = 1
    if nph == 4 and ks == 1 and all(g["Ha"] == ph[0]["Ha"] and g["Wa"] == ph[0]["Wa"] for g in ph):
        kc = Ck // BK
        nt = [len(g["taps"]) for g in ph]
        lds = 2 * (BM + BN) * (BK + 4) * 4
        slots = 256 * max(1, min(160 * 1024 // lds, 4))
        longest = [float(max(nt) * kc), float(max(nt[0] + nt[3], nt[1] + nt[2]) * kc), float(sum(nt) * kc)]
        best = 1e30
        for i in range(3):
            pmv = 1 << i
            cost = math.ceil(mtiles * ntiles * (4 // pmv) / slots) * (longest[i] + 2.5)
            if cost < best * 0.97:
                best, pmerge = cost, pmv
    ngroups = nph // pmerge
    phase_of = lambda g, q: (g if q == 0 else nph - 1 - g) if pmerge == 2 else g * pmerge + q
    uniform = all(g["Ha"] * g["Wa"] == ph[0]["Ha"] * ph[0]["Wa"] for g in ph)
    order_n, m_fast, grid = 0, 0, mtiles * ntiles * ngroups * ks
    if pos_major and (uniform or not stats):
        n, fits = 0, True
        for g in range(ngroups):
            g0 = ph[phase_of(g, 0)]
            for pos in range(g0["Ha"] * g0["Wa"]):
                if n == 256 or pos >= 64 or g >= 4:
                    fits = False
                    break
                n += 1
            if not fits:
                break
        if fits and n > 0:
            order_n = n
            a_bytes, w_bytes = B * p["Hs"] * p["Ws"] * Ck * 4, _ntap_w(p) * N * Ck * 4
            m_fast = int(ntiles > 1 and w_bytes <= 4 << 20 and a_bytes >= 2 * w_bytes)
            grid = n * ks * ntiles * (B // BM)
    srows = ngroups * mtiles
    st_ok = bool(stats) and ks == 1
    ntile = ntiles * BN
    ex = 0.0
    for g in ph:
        if not pos_major:
            ex += 2.0 * cdiv(B * g["Ha"] * g["Wa"], BM) * BM * ntile * Ck * len(g["taps"])
        else:
            ex += sum(2.0 * B * ntile * Ck * _live(p, g, ay, ax) for ay in range(g["Ha"]) for ax in range(g["Wa"]))
    return dict(BM=BM, BN=BN, BK=BK, ks=ks, pos_major=pos_major, pmerge=pmerge, sorted=order_n > 0, m_fast=m_fast, grid=grid,
                stats_rows=srows if st_ok else 0, exec_flops=ex, ragged_m=Mmax % BM != 0 and not pos_major, mtiles=mtiles,
                odd_phases=nph == 4 and not uniform, nphase=nph)


def _ntap_w(p):
    """conv_igemm.hip:1387-1389: weight taps the launch addresses."""
    w = [t[2] + 1 for g in p["ph"] for t in g["taps"]]
    return max(w) if w else 0


def tapless_groups(p, pmerge):
    """Phase groups of a launch (conv_igemm.hip:100-135: group g is phases g and nphase - 1 - g at pmerge 2, else pmerge consecutive
    phases) none of whose phases has a tap: a 1x1 stride-2 data gradient has three such phases, and the merged pair (1, 2) is one."""
    nph = len(p["ph"])
    phases = lambda g: (g, nph - 1 - g) if pmerge == 2 else range(g * pmerge, (g + 1) * pmerge)
    return [g for g in range(nph // pmerge) if not any(p["ph"][q]["taps"] for q in phases(g))]


def try_c16(bwd, B, H, W, Ci, Co, k, s):
    """conv_c16.hip:383-438: None, or the launch's geometry."""
    if "BG_NO_C16" in OFF or k != 5 or s != 2 or H & 1 or W & 1:
        return None
    Hh, Wh = H // 2, W // 2
    if Ci != 16 or Co != (K_DG_CK if bwd else 32) or Wh not in (32, 64) or Hh & 1:
        return None
    if B * H * W * 16 >= 1 << 29 or B * Hh * Wh * 32 >= 1 << 29:
        return None
    nstrips = B * (Hh // 2)
    return dict(Wo=Wh, nstrips=nstrips, grid=min(nstrips, 256))


def try_rows(bwd, B, H, W, Ci, Co, k, s):
    """conv_rows.hip:504-549 (scatter form: thin OUTPUT side)."""
    if "BG_NO_ROWS" in OFF or k not in (5, 3):
        return None
    Ho, _ = same_pads(H, k, s)
    Wo, _ = same_pads(W, k, s)
    if bwd:
        if Ci * k > 16 or Co not in (16, 32, 64):
            return None
        Hi, Wi, Ck, oH, oW, N = Ho, Wo, Co, H, W, Ci
    else:
        if s != 1 or Co * k > 16 or Ci not in (16, 32, 64):
            return None
        Hi, Wi, Ck, oH, oW, N = H, W, Ci, H, W, Co
    if Wi not in (16, 32, 64, 128):
        return None
    if B * Hi * Wi * Ck >= 1 << 31 or B * oH * oW * N >= 1 << 31:
        return None
    R = min(32 if s == 1 else 16, oH)
    wpr = Wi // 16
    ipw = 1 if Wi == 128 else 4 // wpr
    pixw = 128 if Wi == 128 else 64
    if ipw * oW * N > ((s * (16 // k) + 3) // 4) * pixw * 4:
        return None
    if ipw * Hi * Wi * Ck >= 1 << 29 or ipw * oH * oW * N >= 1 << 29:
        return None
    return dict(Wi=Wi, Ck=Ck, N=N, R=R, strips=cdiv(oH, R), ragged_strip=oH % R != 0, ipw=ipw, groups=cdiv(B, ipw), short_last=B % ipw != 0,
                Ho=oH)


def try_rows_gather(bwd, B, H, W, Ci, Co, k, s):
    """conv_rows.hip:456-497 (gather form: thin CONTRACTION side)."""
    if "BG_NO_ROWS" in OFF or k not in (5, 3):
        return None
    Ho, _ = same_pads(H, k, s)
    Wo, _ = same_pads(W, k, s)
    if bwd:
        if s != 1 or Co * k > 16 or Ci not in (16, 32, 64):
            return None
        Wi, Ct, oH, oW, N, ss = W, Co, H, W, Ci, 1
    else:
        if Ci * k > 16 or Co not in (16, 32, 64):
            return None
        Wi, Ct, oH, oW, N, ss = W, Ci, Ho, Wo, Co, s
    if oW % 16 or B * oH * oW * N >= 1 << 31:
        return None
    tiles = oW // 16
    R = min(8 if s == 2 else 16, oH)
    if ((R - 1) * ss + k) * (Wi * Ct + 2 * K_RG_HALO) * 4 > 64 * 1024:
        return None
    return dict(tg=4 if tiles % 4 == 0 else (2 if tiles % 2 == 0 else 1), nt=N // 16, R=R, strips=cdiv(oH, R), ragged_strip=oH % R != 0, Ho=oH)


def _halo(taps):
    if not taps:
        return 0, 0
    return max(t[0] for t in taps) - min(t[0] for t in taps), max(t[1] for t in taps) - min(t[1] for t in taps)


def route(bwd, B, H, W, Ci, Co, s, k=K5, stats=False, workspace=True):
    """bg_conv2d_fwd / bg_conv2d_bwd_data (conv_igemm.hip:1583-1621) and run_gather (:1371-1555) for 16-byte-aligned operands:
    {"family", "names" (the launches the profiler records), and the variant the family's launcher picks}."""
    tag = "dgrad" if bwd else "fwd"
    d = try_c16(bwd, B, H, W, Ci, Co, k, s)
    if d:
        return dict(d, family="conv_c16", names=["conv_c16_" + tag])
    d = try_rows(bwd, B, H, W, Ci, Co, k, s)
    if d:
        return dict(d, family="conv_rows", names=["conv_rows_" + tag])
    d = try_rows_gather(bwd, B, H, W, Ci, Co, k, s)
    if d:
        return dict(d, family="conv_rows_thin_k", names=["conv_rows_thin_k_" + tag])
    p = gather_params(bwd, B, H, W, Ci, Co, k, s)
    N, Ck, ph, nph, ss = p["N"], p["Ck"], p["ph"], len(p["ph"]), p["ss"]
    if Ck % 16 == 0 and N > 4 and N % 4 == 0:                                            # :1396 (vec_ok: aligned operands, N % 4 == 0)
        d = igemm_plan(p, stats, workspace)
        return dict(d, family="conv_igemm", N=N, Ck=Ck, names=["conv_igemm_" + tag] + (["conv_igemm_splitk_reduce"] if d["ks"] > 1 else []))
    if nph == 1 and ss == 1 and p["ds"] == 1 and Ck % 4 == 0 and Ck >= 16 and B <= 65535:  # :1407-1424
        taps = ph[0]["taps"]
        kk = 1
        while kk * kk < len(taps):
            kk += 1
        pt, pl = -taps[0][0], -taps[0][1]
        rect = kk * kk == len(taps) and kk <= 5 and N * kk <= 16 and \
            all(t == (i // kk - pt, i % kk - pl, i) for i, t in enumerate(taps))
        if rect and pl + K_TN_COLS + (kk - 1 - pl) <= K_TN_PX:
            return dict(family="conv_thin_n_mfma", names=["conv_thin_n_mfma_" + tag])
    if N <= 4 and Ck in (16, 32, 64):                                                      # :1425-1506
        wmax = max(g["Wa"] for g in ph)
        TW = 16 if wmax <= 16 else 32
        TH = 256 // TW
        lds = 0
        for g in ph:
            hy, hx = _halo(g["taps"])
            lds = max(lds, ((TH - 1) * ss + hy + 1) * ((TW - 1) * ss + hx + 1) * (Ck + 4) * 4)
        if 1 < nph <= 4 and B <= 65535:
            allt = [t for g in ph for t in g["taps"]]
            hy, hx = (max(t[0] for t in allt) - min(t[0] for t in allt), max(t[1] for t in allt) - min(t[1] for t in allt)) if allt else (-254, -254)
            hamax, wamax = max(g["Ha"] for g in ph), max(g["Wa"] for g in ph)
            PHu, PWu = (min(64 // TW, hamax) - 1) * ss + hy + 1, (min(TW, wamax) - 1) * ss + hx + 1
            if (PHu * PWu * (Ck + 4) + _ntap_w(p) * N * Ck) * 4 <= 150 * 1024:
                return dict(family="conv_thin_n_patch_all", Ck=Ck, TW=TW, N=N, names=["conv_thin_n_patch_all_" + tag])
        if lds <= 150 * 1024 and B * nph <= 65535:
            return dict(family="conv_thin_n_patch", Ck=Ck, TW=TW, N=N, names=["conv_thin_n_patch_" + tag])
    if N <= 4 and Ck % 4 == 0:                                                             # :1507-1512
        return dict(family="conv_thin_n", names=["conv_thin_n_" + tag])
    if Ck <= 4 and N <= 64 and B * nph <= 65535:                                           # :1513-1544
        NT = 1 if N <= 32 else 2
        lds = kfmax = 0
        for g in ph:
            hy, hx = _halo(g["taps"])
            lds = max(lds, (K_TK_MAX_KF * 32 * NT + ((K_TK_TH - 1) * ss + hy + 1) * ((K_TK_TW - 1) * ss + hx + 1) * Ck) * 4)
            kfmax = max(kfmax, len(g["taps"]) * Ck)
        if kfmax + 1 <= K_TK_MAX_KF and lds <= 60 * 1024:
            return dict(family="conv_thin_k_mfma", NT=NT, names=["conv_thin_k_mfma_" + tag])
    if Ck <= 4:                                                                            # :1545-1550
        return dict(family="conv_thin_k", names=["conv_thin_k_" + tag])
    return dict(family="conv_direct", names=["conv_direct_" + tag])


X6_TABLE = ((0, 32, 32, 64, 128, 2), (0, 64, 64, 32, 64, 2))      # conv_igemm_x6.hip:308-311 kX6Table (bwd, H, W, Cin, Cout, s)


def math_taken(bwd, B, H, W, Ci, Co, k, s):
    """bg_conv2d_math_taken(..., bf16x6): conv_igemm_x6.hip:315-348 (table entry AND a geometry the x6 kernel can run)."""
    if k != 5 or (int(bool(bwd)), H, W, Ci, Co, s) not in X6_TABLE:
        return False
    p = gather_params(bwd, B, H, W, Ci, Co, k, s)
    if p["Ck"] % 32 or p["N"] % 32 or max(g["Ha"] * g["Wa"] for g in p["ph"]) <= 16:
        return False
    return B * p["Hs"] * p["Ws"] * p["Ck"] * 4 < 1 << 31 and B * p["Hd"] * p["Wd"] * p["N"] < 1 << 31 and _ntap_w(p) * p["N"] * p["Ck"] * 4 < 1 << 31


def route_cells(bwd, d, B):
    """The cells of ROUTE_CELLS that a described forward / data-gradient case covers."""
    f = d["family"]
    way = "dgrad" if bwd else "fwd"
    if f == "conv_igemm":
        c = {f"igemm:{d['BM']}x{d['BN']}:bk{d['BK']}"}
        if d["ragged_m"]:
            c.add("igemm:ragged_m")
        if (d["N"], d["BN"]) in ((48, 64), (24, 32)):
            c.add(f"igemm:n{d['N']}of{d['BN']}")
        if d["ks"] > 1:
            c.add(f"igemm:splitk{d['ks']}")
        if d["sorted"]:
            c |= {"igemm:pos_major_sorted", f"igemm:m_fast{d['m_fast']}"}
        if d["nphase"] == 4:
            c.add(f"igemm:pmerge{d['pmerge']}")
        if d["odd_phases"]:
            c.add("igemm:odd_map_phases")
        return c
    if f == "conv_c16":
        return {f"c16:{way}:wo{d['Wo']}", "c16:one_strip_per_wg" if d["nstrips"] <= 256 else "c16:strips_not_a_multiple_of_256"}
    if f == "conv_rows":
        c = {f"rows:{way}:w{d['Wi']}", f"rows:ipw{d['ipw']}"}
        if d["short_last"]:
            c.add(f"rows:ipw{d['ipw']}:short_last")
        if d["ragged_strip"]:
            c.add("rows:ragged_strip")
        return c
    if f == "conv_rows_thin_k":
        c = {f"rowsg:{way}", f"rowsg:tg{d['tg']}", f"rowsg:nt{d['nt']}"}
        if d["ragged_strip"]:
            c.add("rowsg:ragged_strip")
        return c
    if f == "conv_thin_n_patch_all":
        return {f"patch_all:ck{d['Ck']}", f"patch_all:tw{d['TW']}", f"patch_all:n{d['N']}"}
    if f == "conv_thin_k_mfma":
        return {f"thin_k_mfma:nt{d['NT']}"}
    return {f[5:]}


ROUTE_CELLS = (
    {f"igemm:{t}:bk{b}" for t in ("128x32", "64x64") for b in (16, 32)} |
    {"igemm:ragged_m", "igemm:n48of64", "igemm:n24of32", "igemm:splitk2", "igemm:splitk4", "igemm:splitk8", "igemm:pos_major_sorted",
     "igemm:m_fast0", "igemm:m_fast1", "igemm:pmerge1", "igemm:pmerge2", "igemm:pmerge4", "igemm:odd_map_phases"} |
    {f"c16:{w}:wo{o}" for w in ("fwd", "dgrad") for o in (32, 64)} | {"c16:one_strip_per_wg", "c16:strips_not_a_multiple_of_256"} |
    {f"rows:{w}:w{o}" for w in ("fwd", "dgrad") for o in (16, 32, 64, 128)} |
    {"rows:ipw4", "rows:ipw2", "rows:ipw1", "rows:ipw4:short_last", "rows:ipw2:short_last", "rows:ragged_strip"} |
    {"rowsg:fwd", "rowsg:dgrad", "rowsg:tg1", "rowsg:tg2", "rowsg:tg4", "rowsg:nt1", "rowsg:nt2", "rowsg:nt4", "rowsg:ragged_strip"} |
    {"thin_n_mfma", "thin_n_patch", "thin_n", "thin_k", "thin_k_mfma:nt1", "thin_k_mfma:nt2", "direct"} |
    {f"patch_all:ck{c}" for c in (16, 32, 64)} | {"patch_all:tw16", "patch_all:tw32"} | {f"patch_all:n{n}" for n in (1, 2, 3, 4)})


# ===================================================================================================================================
# filter gradient: plan_wgrad, restated
# ===================================================================================================================================
K_TC_ROWS, K_TC_HALO, K_TI_HALO = 16, 8, 16              # conv_wgrad.hip:836, :946
ROW_LDS_MAX = 64 * 1024                                  # conv_wgrad.hip:1531 kRowLdsMax
WG_NAMES = {0: "conv_wgrad_direct", 32: "conv_wgrad_c16", 31: "conv_wgrad_mfma_thin_ci", 30: "conv_wgrad_mfma_thin_co"}


def plan_wgrad(B, H, W, Ci, Co, s, k=K5):
    """conv_wgrad.hip:1540-1689 plan_wgrad with the default switches, plus what bg_conv2d_bwd_filter (:1702-1866) derives from the
    plan: pow2 (:1733-1740), the tap-sorted order (:1754), the slab reducer (:1852-1862) and the recorded launch names."""
    Ho, _ = same_pads(H, k, s)
    Wo, _ = same_pads(W, k, s)
    M, kk = B * Ho * Wo, k * k
    nout = kk * Ci * Co
    mfma = Ci % 4 == 0 and Co % 4 == 0 and Ci >= 16 and Co >= 16
    thin_ci = Ci <= 4 and Co % 4 == 0 and Co >= 16 and kk * Ci <= 128
    thin_co = Co <= 4 and Ci % 4 == 0 and Ci >= 16 and s == 1 and kk * Co <= 128
    pl = dict(mode=None, ksplit=1, chunk=0, tiles_m=1, tiles_n=1, bkp=0, always_slab=0, taps_in_grid=0, M=M, Ho=Ho, Wo=Wo, nout=nout, k=k)

    def done():
        lg2 = lambda v: max(0, (v - 1).bit_length())
        pow2 = int(1 << lg2(Wo) == Wo and 1 << lg2(Ho) == Ho)
        if pow2 and B % 128 == 0 and B >= 128 and Ho * Wo <= 16:
            pow2 = 2
        pl["pow2"] = pow2
        pl["tap_sorted"] = pow2 == 2 and pl["taps_in_grid"] == 1 and 1 <= pl["mode"] <= 5
        pl["slabs"] = pl["ksplit"] > 1 or bool(pl["always_slab"])
        pl["ws_bytes"] = pl["ksplit"] * nout * 4 if pl["slabs"] else 0
        pl["reducer"] = None if not pl["slabs"] else ("tall" if nout % 4 == 0 and pl["ksplit"] >= 64 and nout <= 65536 else
                                                      ("float4" if nout % 4 == 0 else "scalar"))
        m = pl["mode"]
        name = WG_NAMES.get(m) or ("conv_wgrad_mfma_thin_co" if 20 <= m < 30 else ("conv_wgrad_mfma_thin_ci" if 10 <= m < 20 else "conv_wgrad_mfma"))
        pl["names"] = [name] + (["conv_wgrad_reduce"] if pl["slabs"] else [])
        return pl

    if not mfma and not thin_ci and not thin_co:                                           # :1551-1559
        pl["mode"] = 0
        want = max(1, 2048 // cdiv(nout, 256))
        pl["chunk"] = max(256, cdiv(M, want))
        pl["ksplit"] = cdiv(M, pl["chunk"])
        return done()
    strip_ok = k == 5 and s == 2 and not (H & 1 or W & 1 or Ci % 32 or Co % 64) and W // 2 in (8, 16, 32) and (H // 2) % (64 // (W // 2)) == 0
    if strip_ok and "BG_WGRAD_NO_STRIP" not in OFF:                                        # :1522-1527, :1560-1577
        nstrips, ntile = B * (Ho // (64 // Wo)), (Ci // 32) * (Co // 64)
        ks = max(1, min(nstrips, max(1, 256 // ntile)))
        spw = cdiv(nstrips, ks)
        pl.update(mode=33, bkp=2, tiles_m=Ci // 32, tiles_n=Co // 64, ksplit=cdiv(nstrips, spw), chunk=spw, always_slab=1, nstrips=nstrips)
        return done()
    if Ci == 16 and Co == 32 and k == 5 and s == 2 and not (H & 1 or W & 1) and Wo in (32, 64) and not Ho & 1 and "BG_NO_C16" not in OFF:   # :1578-1588
        nstrips = B * (Ho // 2)
        pl.update(mode=32, bkp=4, ksplit=max(2, min(nstrips, 256)), chunk=nstrips)
        return done()
    rb = 8 if s == 2 else 16                                                               # :1532 thin_ci_rows
    ti_lds = max(((rb - 1) * s + k) * (W * Ci + 2 * K_TI_HALO), k * (Co // 16) * 4 * 64) * 4   # :1533-1535
    tc_lds = max((K_TC_ROWS + k - 1) * (W * Co + 2 * K_TC_HALO), 4 * k * (Ci // 16) * 4 * 64) * 4   # :1536-1538
    no_tc = "BG_WGRAD_NO_TC" in OFF                                                       # :1589
    if thin_ci and k * Ci <= 16 and k in (5, 3) and Co in (16, 32, 64) and Wo % 4 == 0 and not no_tc and ti_lds <= ROW_LDS_MAX:    # :1590-1601
        nblocks = B * cdiv(Ho, rb)
        pl.update(mode=31, bkp=4, ksplit=max(2, min(nblocks, 1024)), chunk=nblocks, rb=rb, nt=Co // 16)
        return done()
    if thin_ci:                                                                            # :1602-1610
        g = kk * Ci
        pl["mode"], bm, bn = (10, 32, 64) if g <= 32 else ((11, 96, 32) if g <= 96 else (12, 128, 32))
        pl.update(bkp=64, tiles_m=1, tiles_n=cdiv(Co, bn))
    elif thin_co and Ci in (16, 32) and k in (5, 3) and k * Co <= 16 and W % 4 == 0 and not no_tc and tc_lds <= ROW_LDS_MAX:       # :1611-1621
        nblocks = B * cdiv(H, K_TC_ROWS)
        pl.update(mode=30, bkp=4, ksplit=max(2, min(nblocks, 1024)), chunk=nblocks, mt=Ci // 16)
        return done()
    elif thin_co:                                                                          # :1622-1630
        g = kk * Co
        pl["mode"], bm, bn = (20, 64, 32) if g <= 32 else ((21, 32, 96) if g <= 96 else (22, 32, 128))
        pl.update(bkp=64, tiles_m=cdiv(Ci, bm), tiles_n=1)
    elif k == 5 and Ci <= 64 and "BG_WGRAD_NO_TG" not in OFF and M >= 131072:              # :1632-1638
        bm = 32
        pl["mode"], bn = (6, 64) if Co > 32 else (7, 32)
        pl.update(bkp=32, tiles_m=cdiv(Ci, bm), tiles_n=cdiv(Co, bn), taps_in_grid=2)
    else:                                                                                  # :1640-1647
        if Ci > 64 and Co > 64:
            pl["mode"], bm, bn, bkp = 1, 128, 128, 32
        elif Ci > 32 and Co > 32:
            pl["mode"], bm, bn, bkp = 2, 64, 64, 32
        elif Ci > 32:
            pl["mode"], bm, bn, bkp = 3, 64, 32, 64
        elif Co > 32:
            pl["mode"], bm, bn, bkp = 4, 32, 64, 64
        else:
            pl["mode"], bm, bn, bkp = 5, 32, 32, 128
        pl.update(bkp=bkp, tiles_m=cdiv(Ci, bm), tiles_n=cdiv(Co, bn), taps_in_grid=1)
    tig, bkp = pl["taps_in_grid"], pl["bkp"]
    base = pl["tiles_m"] * pl["tiles_n"] * (kk if tig == 1 else (k if tig == 2 else 1))   # :1650
    steps = cdiv(M, bkp)
    skipping = Ho * Wo <= 16 and B >= 128 and B % 128 == 0
    if tig != 1 or skipping:                                                               # :1656-1664
        tgt = 1536 if tig == 2 and M >= 200000 else 768
        want = max(1, cdiv(tgt, base))
        want = min(want, max(1, steps // (8 if skipping else 4)))
        if nout * 4 > 8 << 20:
            want = min(want, 2)
    else:                                                                                  # :1665-1684: rounds x (steps + overhead) + slab reduce
        lds = 2 * bkp * (bm + bn) * 4
        per_cu = max(1, min(160 * 1024 // lds, 5))
        slots = 256.0 * per_cu
        t_step = 2.0 * bm * bn * bkp * per_cu / 614e9 * 1e6
        ovh = 5.0 / t_step
        nout_bytes = kk * Ci * Co * 4.0
        best, want = 1e30, 1
        for ks in range(1, min(64, max(1, steps // 4)) + 1):
            rounds = float(math.ceil(base * ks / slots))
            per_wg = float(math.ceil(steps / ks))
            cost = rounds * (per_wg + ovh) * t_step + (5.0 + (ks + 1) * nout_bytes / 3.5e6 + ks * nout_bytes / 5e6 if ks > 1 else 0.0)
            if cost < best * 0.999:
                best, want = cost, ks
    pl["chunk"] = cdiv(cdiv(M, want), bkp) * bkp                                           # :1685-1687
    pl["ksplit"] = cdiv(M, pl["chunk"])
    return done()


def wgrad_cells(pl, B, s):
    m = pl["mode"]
    c = {f"reduce:{pl['reducer']}"} if pl["reducer"] else set()
    if 1 <= m <= 5:
        c.add(f"mode{m}:pow2_{pl['pow2']}")
        if pl["tap_sorted"]:
            c.add("tap_sorted")
    elif m == 30:
        c.add(f"mode30:mt{pl['mt']}")
    elif m == 31:
        c |= {f"mode31:nt{pl['nt']}", f"mode31:rb{pl['rb']}"}
    elif m == 32:
        c.add(f"mode32:wo{pl['Wo']}")
    elif m == 33:
        c.add(f"mode33:wo{pl['Wo']}")
        if pl["nstrips"] % pl["ksplit"]:
            c.add("mode33:uneven_strips")
    else:
        c.add(f"mode{m}")
    return c


WGRAD_CELLS = ({f"mode{m}:pow2_{q}" for m in range(1, 6) for q in (0, 1, 2)} | {"tap_sorted"} |
               {f"mode{m}" for m in (0, 6, 7, 10, 11, 12, 20, 21, 22)} | {"mode30:mt1", "mode30:mt2", "mode31:nt1", "mode31:nt2", "mode31:nt4",
                "mode31:rb8", "mode31:rb16", "mode32:wo32", "mode32:wo64", "mode33:wo8", "mode33:wo16", "mode33:wo32", "mode33:uneven_strips",
                "reduce:tall", "reduce:float4", "reduce:scalar"})


# ===================================================================================================================================
# data
# ===================================================================================================================================
def dense_m(K):
    return max(1, min(3, math.isqrt((TWO24 - 1) // K)))


def dense(B, H, W, Ci, Co, s, op, seed=0, k=K5):
    """Integers in [-m, m] -> (x, w, dy) in float64; op names the contraction the bound is taken for ("fwd" / "dgrad" / "wgrad")."""
    Ho, Wo = cdiv(H, s), cdiv(W, s)
    m = dense_m({"fwd": k * k * Ci, "dgrad": k * k * Co, "wgrad": B * Ho * Wo}[op])
    rng = np.random.default_rng([seed, B, H, W, Ci, Co, s])
    draw = lambda shape: rng.integers(-m, m + 1, size=shape).astype(np.float64)
    return draw((B, H, W, Ci)), draw((k, k, Ci, Co)), draw((B, Ho, Wo, Co))


def decode_weights(Ci, Co, k=K5):
    """w[kh, kw, ci, co] = 1 + tap + k k (ci + Cin co): all distinct, < 2^24 (asserted; up to 512 x 512 channels at k = 5)."""
    tap = np.arange(k * k).reshape(k, k, 1, 1)
    w = 1 + tap + k * k * (np.arange(Ci).reshape(1, 1, Ci, 1) + Ci * np.arange(Co).reshape(1, 1, 1, Co))
    assert w.max() < TWO24
    return w.astype(np.float64)


def decode_weight(v, Ci, k=K5):
    """A value of decode_weights -> (kh, kw, ci, co), or None if it is not one."""
    v = float(v)
    if not (v >= 1 and v == int(v)):
        return None
    t, c = (int(v) - 1) % (k * k), (int(v) - 1) // (k * k)
    return t // k, t % k, c % Ci, c // Ci


def impulses(shape, seam_rows=(), seam_cols=(), seed=0, k=K5):
    """One-hot activation [B, H, W, C]: impulses at Chebyshev distance >= k, at the corners, beside the given seam rows / columns,
    then a seeded fill; the candidates are taken in another order for every image."""
    B, H, W, C = shape
    a = np.zeros(shape)
    rng = np.random.default_rng([seed, B, H, W, C])
    rows = sorted({r for r in seam_rows if 0 <= r < H})
    cols = sorted({c for c in seam_cols if 0 <= c < W})
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    pri = [(r, c) for r in rows for c in (0, W // 2, W - 1)] + [(r, c) for c in cols for r in (0, H // 2, H - 1)]
    nfill = min(H * W, 2 * H * W // (k * k) + 4)
    for b in range(B):
        blocked = np.zeros((H + 2 * k, W + 2 * k), bool)
        cand = pri[b % len(pri):] + pri[:b % len(pri)] if pri else []
        if b % 2:                                       # odd images favour the far side of each seam
            cand = cand[::-1]
        cand = corners + cand
        fill = np.stack([rng.integers(0, H, nfill), rng.integers(0, W, nfill)], 1)
        n = 0
        for (r, c) in cand + [tuple(q) for q in fill]:
            if blocked[r + k, c + k]:
                continue
            blocked[r + 1:r + 2 * k, c + 1:c + 2 * k] = True
            a[b, r, c, (n + b) % C if n else (C - 1 if b % 2 else 0)] = 1.0
            n += 1
    return a


def seams(bwd, B, H, W, Ci, Co, s, d, k=K5):
    """Rows and columns of the ACTIVATION (x forward, dy data gradient) that lie beside a tile / strip / phase seam of route d; for
    k < 5 also the rows and columns on either side of the line where a window stops holding padding taps (the 5x5 tables keep the
    impulse sets they were proven on)."""
    Ho, Wo = cdiv(H, s), cdiv(W, s)
    Ha, Wa = (Ho, Wo) if bwd else (H, W)                # the activation's map
    to_act = (lambda o: o // s) if bwd else (lambda o: o * s)     # an output row / column -> the activation row / column under it
    oH, oW = (H, W) if bwd else (Ho, Wo)
    rows, cols = set(), set()
    f = d["family"]
    if f == "conv_igemm" and not d["pos_major"]:
        gh, gw = (cdiv(H, s), cdiv(W, s)) if bwd else (Ho, Wo)       # anchor grid of phase 0
        for t in range(1, min(d["mtiles"], 6)):
            for m in (t * d["BM"] - 1, t * d["BM"]):
                rem = m % (gh * gw)
                rows.add(rem // gw if bwd else rem // gw * s)
                cols.add(rem % gw if bwd else rem % gw * s)
    elif f in ("conv_rows", "conv_rows_thin_k"):
        for j in range(1, d["strips"]):
            rows |= {to_act(j * d["R"] - 1), to_act(j * d["R"])}
        cols |= {to_act(c) for c in range(15, oW, 16)} | {to_act(c) for c in range(16, oW, 16)}
    elif f == "conv_c16":
        for j in (1, 2, Ho // 4, Ho // 2 - 1):              # strips of two rows of the stride-2 map (the output forward, dy backward)
            rows |= {2 * j - 1, 2 * j} if bwd else {to_act(2 * j - 1), to_act(2 * j)}
        cols |= {Wa // 2 - 1, Wa // 2}
    elif f in ("conv_thin_n_patch_all", "conv_thin_n_patch", "conv_thin_k_mfma", "conv_thin_n_mfma"):
        rows |= {to_act(r) for r in (3, 4, 7, 8, 15, 16) if r < oH}
        cols |= {to_act(c) for c in (15, 16, 31, 32, 63, 64) if c < oW}
    if k < K5:
        lo = k // 2                                          # the widest SAME pad: rows / columns lo - 1 and lo straddle its reach
        rows |= {r for r in (lo - 1, lo, Ha - 1 - lo, Ha - lo) if r >= 0}
        cols |= {c for c in (lo - 1, lo, Wa - 1 - lo, Wa - lo) if c >= 0}
    return [r for r in rows if r < Ha], [c for c in cols if c < Wa]


def make_fwd(case, recipe, seed=0):
    """-> (x, w) float64 for conv2d_fwd."""
    (B, H, W, Ci, Co, s), k = case[:6], ksize(case)
    if recipe == "dense":
        x, w, _ = dense(B, H, W, Ci, Co, s, "fwd", seed, k)
        return x, w
    r, c = seams(0, B, H, W, Ci, Co, s, route(0, B, H, W, Ci, Co, s, k), k)
    return impulses((B, H, W, Ci), r, c, seed, k), decode_weights(Ci, Co, k)


def make_dgrad(case, recipe, seed=0):
    """-> (dy, w) float64 for conv2d_bwd_data."""
    (B, H, W, Ci, Co, s), k = case[:6], ksize(case)
    if recipe == "dense":
        _, w, dy = dense(B, H, W, Ci, Co, s, "dgrad", seed + 1, k)
        return dy, w
    r, c = seams(1, B, H, W, Ci, Co, s, route(1, B, H, W, Ci, Co, s, k), k)
    return impulses((B, cdiv(H, s), cdiv(W, s), Co), r, c, seed + 1, k), decode_weights(Ci, Co, k)


WG_DIGITS = 7          # 8^0 .. 8^6 per dy channel: 3 (8^7 - 1) / 7 = 898 779 < 2^24


def wgrad_seam_pixels(pl, B):
    """Flat output-pixel indices m = (b Ho + oh) Wo + ow beside the seams of the filter-gradient plan: first / last pixel, the split
    (chunk) seams, 32-pixel steps, image seams and row seams."""
    M, HoWo, Wo = pl["M"], pl["Ho"] * pl["Wo"], pl["Wo"]
    S = [0, M - 1]
    chunk = pl["chunk"] if pl["mode"] in range(0, 23) and pl["chunk"] else HoWo
    nz = cdiv(M, chunk)
    for z in sorted({1, 2, nz // 2, nz - 1}):
        S += [z * chunk - 1, z * chunk, z * chunk + 31, z * chunk + 32]
    for b in sorted({1, B // 2, B - 1}):
        S += [b * HoWo - 1, b * HoWo, b * HoWo + Wo - 1, b * HoWo + Wo]
    S += [31, 32, 63, 64, M - 2, M - 32, M - 33, (M // 32) * 32 - 1, (M // 32) * 32]
    out = []
    for m in S:
        if 0 <= m < M and m not in out:
            out.append(m)
    return out


def make_wgrad(case, recipe, seed=0):
    """-> (x, dy) float64 for conv2d_bwd_filter, plus the pixel table [Co, 7] of the decode recipe (None for dense)."""
    (B, H, W, Ci, Co, s), k = case[:6], ksize(case)
    x, _, dy = dense(B, H, W, Ci, Co, s, "wgrad", seed + 2, k)
    if recipe == "dense":
        return x, dy, None
    pl = plan_wgrad(B, H, W, Ci, Co, s, k)
    M = pl["M"]
    rng = np.random.default_rng([seed, 77, B, H, W, Ci, Co, s])
    x = rng.integers(-3, 4, size=x.shape).astype(np.float64)
    S = wgrad_seam_pixels(pl, B)
    nd = min(WG_DIGITS, M)
    pix = np.empty((Co, nd), np.int64)
    for co in range(Co):
        own = S[co::Co][:nd]                              # the seam pixels are dealt round the channels
        rest = [int(m) for m in rng.permutation(M)[:2 * nd] if m not in own] if M <= 4096 else \
               [int(m) for m in rng.integers(0, M, 4 * nd) if m not in own]
        rest = list(dict.fromkeys(rest))
        pix[co] = (own + rest)[:nd]
    dy = np.zeros((M, Co))
    for j in range(nd):
        dy[pix[:, j], np.arange(Co)] = 8.0 ** j
    return x, dy.reshape(B, pl["Ho"], pl["Wo"], Co), pix


def decode_wgrad(got, ref, pix, case):
    """First wrong dw element of a decode-recipe case -> text naming the dy pixels whose x values it holds in the wrong digits."""
    B, H, W, Ci, Co, s = case[:6]
    bad = np.argwhere(got != ref)
    kh, kw, ci, co = (int(v) for v in bad[0])

    def digits(v):
        if not np.isfinite(v) or v != np.rint(v):
            return None
        v, out = int(v), []
        for _ in range(pix.shape[1] + 1):
            dgt = ((v + 3) % 8) - 3
            out.append(dgt)
            v = (v - dgt) // 8
        return out

    g, r = digits(got[kh, kw, ci, co]), digits(ref[kh, kw, ci, co])
    Ho, Wo = cdiv(H, s), cdiv(W, s)
    where = "not an integer"
    if g is not None:
        js = [j for j in range(pix.shape[1]) if g[j] != r[j]]
        where = "; ".join(f"digit {j}: got {g[j]} for {r[j]} from dy pixel m={int(pix[co, j])} (b, oh, ow)="
                          f"{(int(pix[co, j]) // (Ho * Wo), int(pix[co, j]) % (Ho * Wo) // Wo, int(pix[co, j]) % Wo)}" for j in js[:4])
        if len(g) > pix.shape[1] and g[-1] != r[-1]:
            where += f"; overflow digit {g[-1]}"
    return (f"{len(bad)} of {ref.size} dw elements wrong, first at tap ({kh}, {kw}) ci {ci} co {co}: got {got[kh, kw, ci, co]!r}, "
            f"expected {ref[kh, kw, ci, co]!r}; {where}")


def describe_wrong(y, ref, Ci, recipe, bwd, k=K5):
    """Text for a wrong forward / data-gradient output: how many, never-written count, and for the decode recipe the weights."""
    bad = np.argwhere(y != ref)
    i = tuple(int(v) for v in bad[0])
    txt = f"{len(bad)} of {ref.size} wrong, {int(np.isnan(y).sum())} never written; first at (b, h, w, c)={i}: got {y[i]!r}, expected {ref[i]!r}"
    if recipe == "decode":
        txt += f"; got weight (kh, kw, ci, co)={decode_weight(y[i], Ci, k)}, expected {decode_weight(ref[i], Ci, k)}"
    return txt


# ===================================================================================================================================
# references (oracle.np_ops in float64; the same functions on float32 arrays are the float32 evaluation the CPU test compares)
# ===================================================================================================================================
def ref_fwd(x, w, s):
    return O.conv2d_fwd(x, w, s)


def ref_dgrad(dy, w, s, hw):
    return O.conv2d_bwd_data(dy, w, s, hw)


def ref_wgrad(x, dy, s, k=K5):
    return O.conv2d_bwd_filter(x, dy, s, k)


def epilogue_ref(z, mode, bias=None, mul=None, ref_act=None, keep=None, keep_elems=0, alpha=0.25, scale=2.0):
    """conv_common.h:150-175 apply_epilogue in float64 on the accumulator z [B, H, W, N]; the mask covers the first keep_elems
    elements of the flattened output (0 = all)."""
    if mode == "affine_lrelu":
        v = z * mul + bias
        return np.where(v > 0, v, alpha * v)
    v = z + (bias if bias is not None else 0.0)
    if mode == "bias_lrelu":
        v = np.where(v > 0, v, alpha * v)
        f = np.ones_like(v)
    elif mode == "mul_grad":
        f = np.where(ref_act > 0, 1.0, alpha)
    else:
        return v
    if keep is not None:
        m = np.where(keep != 0, scale, 0.0).ravel()
        if keep_elems:
            m[keep_elems:] = 1.0
        f = f * m.reshape(v.shape)
    return v * f


# ===================================================================================================================================
# tables.  (B, H, W, Cin, Cout, stride) on the conv's input side, as in the C ABI
# ===================================================================================================================================
IG, C16, RS, RG = "conv_igemm", "conv_c16", "conv_rows", "conv_rows_thin_k"

# (shape, forward family, forward cells, data-gradient family, data-gradient cells): the cells are the ones the case is IN THE TABLE
# FOR (it may cover more); tests/test_conv_cases_cpu.py holds every claim to route() and the union to ROUTE_CELLS
ROUTE_CASES = [
    # ---- gather-GEMM: 128x32 for N <= 32 else 64x64; K step 16 up to 64 channels per tap, 32 from 96 on
    ((2, 8, 8, 32, 32, 2), IG, {"igemm:128x32:bk16", "igemm:ragged_m"}, IG, {"igemm:128x32:bk16", "igemm:pmerge1"}),
    ((3, 8, 8, 32, 64, 1), IG, {"igemm:64x64:bk16"}, IG, {"igemm:128x32:bk16"}),
    ((2, 16, 16, 64, 128, 2), IG, {"igemm:64x64:bk16"}, IG, {"igemm:64x64:bk32", "igemm:pmerge1"}),
    ((2, 4, 4, 128, 256, 2), IG, {"igemm:64x64:bk32", "igemm:ragged_m"}, IG, {"igemm:splitk2", "igemm:ragged_m"}),
    ((5, 2, 2, 256, 512, 2), IG, {"igemm:splitk8"}, IG, {"igemm:splitk4"}),                   # M = 5 rows
    ((9, 4, 4, 512, 512, 1), IG, {"igemm:splitk8"}, IG, {"igemm:splitk8"}),                   # K = 12800, the longest contraction
    ((3, 7, 7, 32, 48, 2), IG, {"igemm:n48of64", "igemm:ragged_m"}, IG, {"igemm:odd_map_phases", "igemm:ragged_m"}),
    ((3, 9, 7, 48, 24, 2), IG, {"igemm:n24of32", "igemm:splitk4"}, "conv_direct", {"direct"}),   # dy has 24 channels: no 16-channel K step
    ((2, 8, 8, 128, 32, 1), IG, {"igemm:128x32:bk32"}, IG, {"igemm:64x64:bk16"}),
    ((128, 4, 4, 64, 64, 1), IG, {"igemm:pos_major_sorted", "igemm:m_fast0"}, IG, {"igemm:pos_major_sorted", "igemm:m_fast0"}),
    ((128, 8, 8, 32, 128, 2), IG, {"igemm:pos_major_sorted", "igemm:m_fast1"}, IG, {"igemm:pos_major_sorted", "igemm:128x32:bk32"}),
    ((64, 4, 4, 256, 256, 2), IG, {"igemm:pos_major_sorted", "igemm:splitk8"}, IG, {"igemm:pos_major_sorted", "igemm:splitk2"}),
    ((520, 16, 16, 16, 32, 2), IG, {"igemm:128x32:bk16"}, IG, {"igemm:pmerge2"}),             # phases merged in pairs, image-major
    ((1024, 16, 16, 16, 32, 2), IG, {"igemm:pos_major_sorted"}, IG, {"igemm:pmerge2", "igemm:pos_major_sorted"}),
    ((1152, 16, 16, 16, 16, 2), IG, {"igemm:pos_major_sorted"}, IG, {"igemm:pmerge4", "igemm:pos_major_sorted"}),   # 576 M tiles: all four phases in one workgroup
    # ---- row-staged 16-channel kernels: one strip per workgroup; 260 strips on 256 persistent workgroups
    ((3, 64, 64, 16, 32, 2), C16, {"c16:fwd:wo32", "c16:one_strip_per_wg"}, C16, {"c16:dgrad:wo32", "c16:one_strip_per_wg"}),
    ((2, 128, 128, 16, 32, 2), C16, {"c16:fwd:wo64", "c16:one_strip_per_wg"}, C16, {"c16:dgrad:wo64", "c16:one_strip_per_wg"}),
    ((5, 208, 64, 16, 32, 2), C16, {"c16:fwd:wo32", "c16:strips_not_a_multiple_of_256"}, C16, {"c16:dgrad:wo32", "c16:strips_not_a_multiple_of_256"}),
    ((5, 208, 128, 16, 32, 2), C16, {"c16:fwd:wo64", "c16:strips_not_a_multiple_of_256"}, C16, {"c16:dgrad:wo64", "c16:strips_not_a_multiple_of_256"}),
    # ---- row kernels: scatter form on the thin OUTPUT side, gather form on the thin CONTRACTION side
    ((5, 24, 16, 16, 3, 1), RS, {"rows:fwd:w16", "rows:ipw4", "rows:ipw4:short_last"}, RG, {"rowsg:dgrad", "rowsg:tg1", "rowsg:nt1", "rowsg:ragged_strip"}),
    ((3, 40, 32, 32, 2, 1), RS, {"rows:fwd:w32", "rows:ipw2", "rows:ipw2:short_last", "rows:ragged_strip"}, RG, {"rowsg:tg2", "rowsg:nt2"}),
    ((2, 36, 64, 64, 1, 1), RS, {"rows:fwd:w64", "rows:ipw1", "rows:ragged_strip"}, RG, {"rowsg:tg4", "rowsg:nt4"}),
    ((2, 20, 128, 16, 3, 1), RS, {"rows:fwd:w128", "rows:ipw1"}, RG, {"rowsg:dgrad", "rowsg:tg4"}),
    ((5, 32, 32, 3, 32, 2), RG, {"rowsg:fwd", "rowsg:tg1", "rowsg:nt2"}, RS, {"rows:dgrad:w16", "rows:ipw4:short_last"}),
    ((3, 40, 64, 2, 16, 2), RG, {"rowsg:fwd", "rowsg:tg2", "rowsg:nt1", "rowsg:ragged_strip"}, RS, {"rows:dgrad:w32", "rows:ipw2:short_last", "rows:ragged_strip"}),
    ((2, 44, 128, 3, 64, 2), RG, {"rowsg:fwd", "rowsg:tg4", "rowsg:nt4", "rowsg:ragged_strip"}, RS, {"rows:dgrad:w64", "rows:ragged_strip"}),
    ((2, 24, 256, 3, 16, 2), RG, {"rowsg:fwd", "rowsg:tg4"}, RS, {"rows:dgrad:w128", "rows:ragged_strip"}),
    ((2, 18, 16, 1, 16, 1), RG, {"rowsg:fwd", "rowsg:ragged_strip"}, RS, {"rows:dgrad:w16", "rows:ipw4:short_last"}),
    # ---- the families behind them
    ((2, 20, 24, 32, 2, 1), "conv_thin_n_mfma", {"thin_n_mfma"}, "conv_thin_k_mfma", {"thin_k_mfma:nt1"}),       # 24-pixel rows: no row kernel
    ((3, 27, 25, 1, 64, 2), "conv_thin_k_mfma", {"thin_k_mfma:nt2"}, "conv_thin_n_patch_all", {"patch_all:ck64", "patch_all:n1", "patch_all:tw16"}),
    ((2, 44, 40, 2, 16, 2), "conv_thin_k_mfma", {"thin_k_mfma:nt1"}, "conv_thin_n_patch_all", {"patch_all:ck16", "patch_all:n2", "patch_all:tw32"}),
    ((5, 13, 14, 4, 32, 2), "conv_thin_k_mfma", {"thin_k_mfma:nt1"}, "conv_thin_n_patch_all", {"patch_all:ck32", "patch_all:n4", "patch_all:tw16"}),
    ((2, 14, 14, 3, 16, 2), "conv_thin_k_mfma", {"thin_k_mfma:nt1"}, "conv_thin_n_patch_all", {"patch_all:ck16", "patch_all:n3"}),
    ((2, 14, 14, 16, 1, 2), "conv_thin_n_patch", {"thin_n_patch"}, "conv_thin_k_mfma", {"thin_k_mfma:nt1"}),
    ((2, 12, 12, 4, 16, 1), "conv_thin_k_mfma", {"thin_k_mfma:nt1"}, "conv_thin_n_patch", {"thin_n_patch"}),
    ((2, 14, 14, 64, 1, 2), "conv_thin_n", {"thin_n"}, "conv_thin_k_mfma", {"thin_k_mfma:nt2"}),                # the stride-2 patch of 64 channels is past 150 KB
    ((2, 12, 12, 4, 24, 2), "conv_thin_k_mfma", {"thin_k_mfma:nt1"}, "conv_thin_n", {"thin_n"}),
    ((2, 9, 7, 3, 96, 2), "conv_thin_k", {"thin_k"}, "conv_thin_n", {"thin_n"}),
    ((2, 9, 7, 128, 3, 2), "conv_thin_n", {"thin_n"}, "conv_thin_k", {"thin_k"}),
    ((2, 9, 7, 20, 12, 2), "conv_direct", {"direct"}, "conv_direct", {"direct"}),
]

# (shape, mode, slabs the planner reports (1 = none), cells)
WGRAD_CASES = [
    ((2, 7, 7, 96, 96, 1), 1, 1, {"mode1:pow2_0"}), ((2, 8, 8, 96, 96, 1), 1, 1, {"mode1:pow2_1"}),
    ((128, 4, 4, 96, 96, 1), 1, 8, {"mode1:pow2_2", "tap_sorted"}),
    ((2, 7, 9, 48, 48, 1), 2, 1, {"mode2:pow2_0"}), ((2, 8, 8, 64, 64, 1), 2, 1, {"mode2:pow2_1"}),
    ((128, 4, 4, 64, 64, 1), 2, 8, {"mode2:pow2_2", "tap_sorted"}), ((4, 64, 64, 64, 64, 1), 2, 47, {"mode2:pow2_1", "reduce:float4"}),
    ((3, 9, 7, 48, 24, 2), 3, 1, {"mode3:pow2_0"}), ((2, 16, 16, 64, 32, 2), 3, 1, {"mode3:pow2_1"}),
    ((128, 8, 8, 64, 32, 2), 3, 4, {"mode3:pow2_2", "tap_sorted"}),
    ((3, 9, 7, 32, 48, 2), 4, 1, {"mode4:pow2_0"}), ((3, 8, 8, 32, 64, 1), 4, 1, {"mode4:pow2_1"}),
    ((128, 8, 8, 32, 64, 2), 4, 4, {"mode4:pow2_2", "tap_sorted"}),
    ((2, 7, 9, 16, 16, 1), 5, 1, {"mode5:pow2_0"}), ((2, 16, 16, 16, 16, 1), 5, 1, {"mode5:pow2_1"}),
    ((128, 4, 4, 32, 32, 2), 5, 1, {"mode5:pow2_2", "tap_sorted"}), ((16, 32, 32, 32, 32, 1), 5, 19, {"mode5:pow2_1", "reduce:float4"}),
    ((2, 28, 28, 1, 48, 2), 10, 1, {"mode10"}), ((2, 18, 18, 3, 16, 1), 11, 2, {"mode11"}), ((5, 13, 14, 4, 32, 2), 12, 1, {"mode12"}),
    ((2, 14, 14, 64, 1, 1), 20, 1, {"mode20"}), ((3, 20, 12, 48, 3, 1), 21, 3, {"mode21"}), ((2, 12, 12, 16, 4, 1), 22, 1, {"mode22"}),
    ((3, 20, 12, 16, 3, 1), 30, 6, {"mode30:mt1"}), ((2, 40, 16, 32, 2, 1), 30, 6, {"mode30:mt2"}),
    ((2, 18, 16, 3, 16, 1), 31, 4, {"mode31:nt1", "mode31:rb16"}), ((2, 36, 32, 2, 32, 2), 31, 6, {"mode31:nt2", "mode31:rb8"}),
    ((3, 24, 24, 1, 64, 2), 31, 6, {"mode31:nt4", "mode31:rb8"}), ((8, 128, 32, 3, 32, 2), 31, 64, {"mode31:nt2", "reduce:tall"}),
    ((3, 64, 64, 16, 32, 2), 32, 48, {"mode32:wo32"}), ((2, 128, 128, 16, 32, 2), 32, 64, {"mode32:wo64", "reduce:tall"}),
    ((5, 208, 64, 16, 32, 2), 32, 256, {"mode32:wo32"}),                                     # 260 strips on 256 workgroups
    ((3, 16, 16, 32, 64, 2), 33, 3, {"mode33:wo8"}), ((2, 32, 32, 64, 128, 2), 33, 8, {"mode33:wo16"}),
    ((2, 64, 64, 32, 64, 2), 33, 32, {"mode33:wo32"}), ((33, 16, 16, 64, 256, 2), 33, 17, {"mode33:wo8", "mode33:uneven_strips"}),
    ((2, 12, 12, 8, 4, 2), 0, 1, {"mode0"}), ((3, 20, 20, 3, 5, 1), 0, 5, {"mode0", "reduce:scalar"}),
    # ---- the tap-grouped kernel (modes 6 / 7): the smallest shapes with M >= 131072
    ((2, 256, 256, 16, 16, 1), 7, 152, {"mode7", "reduce:tall"}), ((2, 256, 256, 16, 64, 1), 6, 152, {"mode6", "reduce:tall"}),
    ((32, 130, 130, 16, 64, 2), 6, 151, {"mode6"}),                  # Wo = 65: not a power of two, carries on an odd map
    ((8192, 4, 4, 16, 16, 1), 7, 152, {"mode7"}), ((131072, 1, 1, 16, 32, 1), 7, 152, {"mode7"}),     # maps smaller than one 32-pixel step
    ((14564, 3, 3, 32, 48, 1), 6, 152, {"mode6"}),                   # M = 131076: ragged tail, ragged Co tile, 9-pixel maps
    ((8, 128, 128, 20, 36, 1), 6, 152, {"mode6"}),                   # ragged Ci and Co tiles
    ((2, 255, 257, 16, 16, 1), 5, 20, {"mode5:pow2_0"}),             # M = 131070: the last shape that stays on mode 5
    ((33, 63, 65, 48, 40, 1), 6, 77, {"mode6"}),
]

# epilogues, per kernel family with its own epilogue code: (data gradient?, shape)
EPI_CASES = [
    (0, (2, 8, 8, 32, 32, 2)), (1, (2, 8, 8, 32, 32, 2)), (0, (3, 8, 8, 32, 64, 1)),          # gather-GEMM float4 epilogue, both tiles
    (0, (2, 4, 4, 128, 256, 2)),                                                              # ... applied by the split-K reduce
    (0, (3, 64, 64, 16, 32, 2)), (1, (3, 64, 64, 16, 32, 2)),                                 # c16
    (0, (5, 24, 16, 16, 3, 1)), (1, (5, 32, 32, 3, 32, 2)), (0, (2, 20, 128, 16, 3, 1)),      # scatter rows (64- and 128-pixel workgroups)
    (0, (5, 32, 32, 3, 32, 2)), (1, (5, 24, 16, 16, 3, 1)),                                   # gather rows
    (0, (2, 20, 24, 32, 2, 1)), (1, (5, 13, 14, 4, 32, 2)), (0, (2, 14, 14, 16, 1, 2)), (0, (2, 14, 14, 64, 1, 2)),
    (0, (2, 12, 12, 4, 24, 2)), (0, (2, 9, 7, 3, 96, 2)), (0, (2, 9, 7, 20, 12, 2)),          # thin and direct kernels
]

# statistics epilogue of the gather-GEMM: (data gradient?, shape): both tiles, four phases, position-major, phases of different extents
STATS_CASES = [(0, (3, 8, 8, 32, 64, 1)), (0, (2, 8, 8, 32, 32, 2)), (1, (2, 8, 8, 32, 32, 2)), (1, (2, 16, 16, 64, 128, 2)),
               (0, (128, 4, 4, 64, 64, 1)), (1, (3, 7, 7, 32, 48, 2)), (1, (520, 16, 16, 16, 32, 2))]

# isolation (a NaN image; two runs): one case per family of ROUTE_CASES, and one per filter-gradient kernel for the two runs
ISOLATION_ROUTES = [(0, (2, 8, 8, 32, 32, 2)), (1, (2, 4, 4, 128, 256, 2)), (0, (128, 4, 4, 64, 64, 1)), (1, (520, 16, 16, 16, 32, 2)),
                    (0, (3, 64, 64, 16, 32, 2)), (1, (3, 64, 64, 16, 32, 2)), (0, (5, 24, 16, 16, 3, 1)), (1, (5, 32, 32, 3, 32, 2)),
                    (0, (5, 32, 32, 3, 32, 2)), (1, (5, 24, 16, 16, 3, 1)), (0, (2, 20, 24, 32, 2, 1)), (1, (5, 13, 14, 4, 32, 2)),
                    (0, (2, 14, 14, 16, 1, 2)), (0, (2, 14, 14, 64, 1, 2)), (0, (2, 12, 12, 4, 24, 2)), (0, (2, 9, 7, 3, 96, 2)),
                    (0, (2, 9, 7, 20, 12, 2))]
ISOLATION_WGRAD = [(128, 4, 4, 64, 64, 1), (4, 64, 64, 64, 64, 1), (2, 18, 18, 3, 16, 1), (3, 20, 12, 48, 3, 1), (3, 20, 12, 16, 3, 1),
                   (2, 36, 32, 2, 32, 2), (3, 64, 64, 16, 32, 2), (33, 16, 16, 64, 256, 2), (3, 20, 20, 3, 5, 1), (2, 256, 256, 16, 16, 1),
                   (33, 63, 65, 48, 40, 1)]


# The fallbacks behind SWITCHED_ENV (run only by tests/conv_switched_child.py, in a process started with those variables set):
# (data gradient?, shape, family) -- the c16 and row-kernel shapes on the generic kernels
SWITCHED_ROUTES = [(0, (3, 64, 64, 16, 32, 2), IG), (1, (3, 64, 64, 16, 32, 2), IG), (0, (2, 128, 128, 16, 32, 2), IG), (1, (2, 128, 128, 16, 32, 2), IG),
                   (0, (5, 24, 16, 16, 3, 1), "conv_thin_n_mfma"), (1, (5, 24, 16, 16, 3, 1), "conv_thin_k_mfma"),
                   (0, (5, 32, 32, 3, 32, 2), "conv_thin_k_mfma"), (1, (5, 32, 32, 3, 32, 2), "conv_thin_n_patch_all"),
                   (0, (2, 20, 128, 16, 3, 1), "conv_thin_n_mfma"), (1, (2, 24, 256, 3, 16, 2), "conv_thin_n_patch_all")]
# (shape, mode, slabs): the c16, strip, row-MFMA and tap-grouped shapes on the generic filter-gradient kernels -- modes 4 and 5 at
# M >= 131072, which the tap-grouped kernel otherwise keeps from them
SWITCHED_WGRAD = [((3, 64, 64, 16, 32, 2), 5), ((2, 64, 64, 32, 64, 2), 4), ((2, 32, 32, 64, 128, 2), 2), ((33, 16, 16, 64, 256, 2), 2),
                  ((3, 20, 12, 16, 3, 1), 21), ((2, 36, 32, 2, 32, 2), 11), ((3, 24, 24, 1, 64, 2), 10),
                  ((2, 256, 256, 16, 16, 1), 5), ((2, 256, 256, 16, 64, 1), 4), ((14564, 3, 3, 32, 48, 1), 4), ((33, 63, 65, 48, 40, 1), 2)]


def run_switched_child(mode):
    """Starts tests/conv_switched_child.py in a fresh process whose environment sets SWITCHED_ENV; its output ends in "ok"."""
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_switched_child.py")
    r = subprocess.run([sys.executable, script, mode], env={**os.environ, **SWITCHED_ENV}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout.strip().splitlines()[-1]


def case_id(shape):
    """B x H x W x Cin x Cout s stride, and k<size> for a shape that carries one."""
    return "x".join(map(str, shape[:5])) + f"s{shape[5]}" + (f"k{shape[6]}" if len(shape) > 6 else "")
