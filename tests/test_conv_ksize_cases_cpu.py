"""CPU: the k = 3 and k = 1 conv case tables of tests/conv_ksize_cases.py held to their claims, as tests/test_conv_cases_cpu.py holds
the 5x5 ones -- every case and recipe exact in float32 (the float32 oracle equals the float64 oracle bit for bit, K m^2 < 2^24, no
k x k window with two impulses), every output a weight that decodes to a tap below k k, every case on the family, mode, variant
and cells it is listed under, the union of the cells equal to the sets written out below -- and the restated planners held to the
library's host-only entry points (bg_conv2d_bwd_filter_workspace_bytes, bg_conv2d_splitk_workspace_bytes in both directions,
bg_conv2d_math_taken, which must decline every k != 5 geometry) over the tables and a seeded sweep of 3000 geometries with k drawn
from {1, 3}."""
import os

import numpy as np
import pytest

import conv_cases as CC
import conv_ksize_cases as KC
from test_conv_cases_cpu import _check_impulses, _same_in_float32

ROUTE_IDS = [CC.case_id(c[0]) for c in KC.ROUTE_CASES]
WGRAD_IDS = [CC.case_id(c[0]) for c in KC.WGRAD_CASES]

# The cells the route table is held to, by set equality.  Written out: a case that drifts off its cell, or a cell nobody lists, fails.
ROUTE_CELLS = {
    # gather-GEMM: tiles x K steps, ragged M / N, split-K (nine taps both ways, one tap), odd maps, position-major, merged and empty phases
    "igemm:128x32:bk16", "igemm:128x32:bk32", "igemm:64x64:bk16", "igemm:64x64:bk32", "igemm:ragged_m", "igemm:n48of64", "igemm:n24of32",
    "igemm:splitk2", "igemm:splitk4", "igemm:splitk8", "igemm:splitk:9tap:fwd", "igemm:splitk:9tap:dgrad", "igemm:splitk:1tap:fwd",
    "igemm:odd_map_phases", "igemm:odd_map_phases:7x7", "igemm:odd_map_phases:9x7", "igemm:odd_map_phases:7x9",
    "igemm:pos_major:k3:padding_skipped", "igemm:pos_major:k1:no_padding_tap", "igemm:m_fast0", "igemm:m_fast1",
    "igemm:pmerge1", "igemm:pmerge2", "igemm:pmerge2:k3:pos_major", "igemm:pmerge2:k3:image_major", "igemm:pmerge2:k1:pos_major",
    "igemm:pmerge2:k1:image_major", "igemm:pmerge2:tapless_pair", "igemm:empty_phases:128x32", "igemm:empty_phases:64x64",
    "k3s2:pad00", "k3s2:pad11",
    # row kernels at k = 3
    "rows:fwd:w16", "rows:fwd:w32", "rows:fwd:w64", "rows:fwd:w128", "rows:dgrad:w16", "rows:dgrad:w32", "rows:dgrad:w64", "rows:dgrad:w128",
    "rows:ipw4", "rows:ipw2", "rows:ipw1", "rows:ipw4:short_last", "rows:ipw2:short_last", "rows:ragged_strip",
    "rows:thin1", "rows:thin3", "rows:thin4", "rows:thin5", "rows:fwd:s1", "rows:dgrad:s1", "rows:dgrad:s2",
    "rowsg:fwd", "rowsg:dgrad", "rowsg:tg1", "rowsg:tg2", "rowsg:tg4", "rowsg:nt1", "rowsg:nt2", "rowsg:nt4", "rowsg:ragged_strip",
    "rowsg:thin1", "rowsg:thin3", "rowsg:thin4", "rowsg:thin5", "rowsg:fwd:s1", "rowsg:fwd:s2", "rowsg:dgrad:s1", "rowsg:scalar_staging",
    # the families behind them
    "thin_n_mfma:k3:n5", "thin_n_mfma:k3:n3", "thin_n_mfma:ck48", "thin_n_mfma:k1:n12", "thin_n_mfma:k1:n16", "thin_n_mfma:k1:n3",
    "thin_k_mfma:nt1", "thin_k_mfma:nt2", "patch_all:live_phases4", "patch_all:live_phases1", "patch_all:ck64", "patch_all:n1", "patch_all:n4",
    "thin_n_patch", "thin_n", "thin_k", "direct:k3", "direct:k1",
    "thin_n_patch_all:empty_phases", "thin_k_mfma:empty_phases", "thin_n:empty_phases", "thin_k:empty_phases", "direct:empty_phases",
}
WGRAD_CELLS = ({f"mode{m}:pow2_{q}" for m in range(1, 6) for q in (0, 1, 2)} | {f"k3:mode{m}" for m in (0, 1, 2, 3, 4, 5, 10, 11, 20, 21, 30, 31)} |
               {f"k1:mode{m}" for m in (0, 1, 2, 3, 4, 5, 10, 20)} |
               {"tap_sorted:9tap", "tap_sorted:1tap", "wide_row:mode10", "wide_row:mode11", "wide_row:mode20", "mode0", "mode10", "mode11",
                "mode20", "mode21", "mode30:mt1", "mode30:mt2", "mode31:nt1", "mode31:nt2", "mode31:nt4", "mode31:rb8", "mode31:rb16", "reduce:tall", "reduce:float4", "reduce:scalar"})
# every launch name a k != 5 call can record (the 5x5-only conv_c16_* are not among them)
FWD_NAMES = {"conv_igemm_fwd", "conv_rows_fwd", "conv_rows_thin_k_fwd", "conv_thin_n_mfma_fwd", "conv_thin_n_patch_fwd", "conv_thin_n_fwd",
             "conv_thin_k_mfma_fwd", "conv_thin_k_fwd", "conv_direct_fwd"}
DGRAD_NAMES = {"conv_igemm_dgrad", "conv_rows_dgrad", "conv_rows_thin_k_dgrad", "conv_thin_n_mfma_dgrad", "conv_thin_n_patch_all_dgrad",
               "conv_thin_n_patch_dgrad", "conv_thin_n_dgrad", "conv_thin_k_mfma_dgrad", "conv_thin_k_dgrad", "conv_direct_dgrad"}


@pytest.fixture(scope="module")
def lib():
    from blurred_gan_amd import _lib
    assert not [k for k in CC.STATIC_SWITCHES if k in os.environ], "conv tuning switches set in the environment"
    return _lib.load()


def test_case_ids_are_unique_and_carry_k():
    assert len(set(ROUTE_IDS)) == len(ROUTE_IDS) and len(set(WGRAD_IDS)) == len(WGRAD_IDS)
    assert all(i.endswith(("k3", "k1")) for i in ROUTE_IDS + WGRAD_IDS)
    assert CC.case_id((2, 8, 8, 32, 32, 2)) == "2x8x8x32x32s2" and CC.ksize((2, 8, 8, 32, 32, 2)) == 5        # a 6-tuple still means 5x5
    tables = [c[0] for c in KC.ROUTE_CASES + KC.WGRAD_CASES] + [c for _, c in KC.EPI_CASES + KC.STATS_CASES + KC.ISOLATION_ROUTES] + KC.ISOLATION_WGRAD
    assert {c[6] for c in tables} == {1, 3} and all(len(c) == 7 for c in tables)


@pytest.mark.parametrize("case", KC.ROUTE_CASES, ids=ROUTE_IDS)
def test_forward_and_data_gradient_cases_are_exact_in_float32(case):
    shape, ffam, _, dfam, _ = case
    B, H, W, Ci, Co, s, k = shape
    kk = k * k
    assert kk * max(Ci, Co) * CC.dense_m(kk * max(Ci, Co)) ** 2 < CC.TWO24 and kk * Ci * Co + kk < CC.TWO24
    for bwd, fam in ((0, ffam), (1, dfam)):
        if fam is None:
            continue
        Ck = Co if bwd else Ci
        fn = (lambda a, b: CC.ref_dgrad(a, b, s, (H, W))) if bwd else (lambda a, b: CC.ref_fwd(a, b, s))
        for recipe in ("dense", "decode"):
            act, w = (CC.make_dgrad if bwd else CC.make_fwd)(shape, recipe)
            assert w.shape == (k, k, Ci, Co)
            if recipe == "dense":
                m = CC.dense_m(kk * Ck)
                assert np.abs(act).max() <= m and np.abs(w).max() <= m and kk * Ck * m * m < CC.TWO24
            else:
                _check_impulses(act, k)                   # no k x k window holds two impulses (k = 1: every pixel may hold one)
                assert len(np.unique(w)) == w.size and w.min() == 1 and w.max() == kk * Ci * Co < CC.TWO24
            ref = fn(act, w)
            _same_in_float32(fn, ref, act, w)
            if recipe == "decode":                        # every output IS one weight (or 0) and decodes to a tap below k k
                nz = np.unique(ref[ref != 0])
                assert nz.size and np.isin(nz, w).all()
                for v in nz[:: max(1, nz.size // 64)]:
                    kh, kw, ci, co = CC.decode_weight(v, Ci, k)
                    assert kh * k + kw < kk and kh < k and kw < k and w[kh, kw, ci, co] == v


@pytest.mark.parametrize("case", KC.WGRAD_CASES, ids=WGRAD_IDS)
def test_filter_gradient_cases_are_exact_in_float32(case):
    shape = case[0]
    B, H, W, Ci, Co, s, k = shape
    M = B * CC.cdiv(H, s) * CC.cdiv(W, s)
    fn = lambda a, b: CC.ref_wgrad(a, b, s, k)
    for recipe in ("dense", "decode"):
        x, dy, pix = CC.make_wgrad(shape, recipe)
        if recipe == "dense":
            m = CC.dense_m(M)
            assert np.abs(x).max() <= m and np.abs(dy).max() <= m and M * m * m < CC.TWO24
        else:
            assert np.abs(x).max() <= 3 and 3 * (8 ** CC.WG_DIGITS - 1) // 7 < CC.TWO24
            flat = dy.reshape(M, Co)
            for co in (0, Co - 1):
                assert len(set(pix[co])) == pix.shape[1] and np.array_equal(flat[pix[co], co], 8.0 ** np.arange(pix.shape[1]))
            assert (flat != 0).sum() == Co * pix.shape[1] and {0, M - 1} <= set(pix.ravel().tolist())
        ref = fn(x, dy)
        assert ref.shape == (k, k, Ci, Co) and 2 * np.abs(ref).max() + 8 < CC.TWO24      # the accumulate form: 0.5 dw0 + 2 grad, |dw0| <= 8
        _same_in_float32(fn, ref, x, dy)


def test_a_wrong_output_names_its_tap_and_a_wrong_filter_gradient_element_its_pixel():
    shape = (2, 7, 9, 16, 16, 1, 3)
    x, w = CC.make_fwd(shape, "decode")
    ref = CC.ref_fwd(x, w, 1)
    got = ref.copy()
    i = tuple(np.argwhere(ref != 0)[5])
    got[i] = w[2, 1, 3, 4]
    msg = CC.describe_wrong(got, ref, 16, "decode", 0, 3)
    assert "got weight (kh, kw, ci, co)=(2, 1, 3, 4)" in msg and f"expected {CC.decode_weight(ref[i], 16, 3)}" in msg, msg
    x, dy, pix = CC.make_wgrad(shape, "decode")
    ref = CC.ref_wgrad(x, dy, 1, 3)
    got = ref.copy()
    got[1, 2, 3, 4] -= 2 * 8.0 ** 3                     # digit 3 of channel 4 is off by 2
    msg = CC.decode_wgrad(got, ref, pix, shape)
    assert "tap (1, 2) ci 3 co 4" in msg and "digit 3" in msg and f"m={int(pix[4, 3])} " in msg, msg


@pytest.mark.parametrize("case", KC.ROUTE_CASES, ids=ROUTE_IDS)
def test_forward_and_data_gradient_cases_are_on_their_claimed_routes(case):
    shape, ff, fc, df, dc = case
    for bwd, fam, cells in ((0, ff, fc), (1, df, dc)):
        if fam is None:
            assert not cells
            continue
        d = CC.route(bwd, *shape)
        assert d["family"] == fam and d["names"][0] == fam + ("_dgrad" if bwd else "_fwd"), d
        assert cells <= KC.route_cells(bwd, d, shape), (bwd, cells - KC.route_cells(bwd, d, shape))


@pytest.mark.parametrize("case", KC.WGRAD_CASES, ids=WGRAD_IDS)
def test_filter_gradient_cases_are_on_their_claimed_modes(case, lib):
    shape, mode, slabs, cells = case
    B, H, W, Ci, Co, s, k = shape
    pl = CC.plan_wgrad(*shape)
    assert (pl["mode"], pl["ksplit"]) == (mode, slabs), (pl["mode"], pl["ksplit"])
    assert cells <= KC.wgrad_cells(pl, shape), cells - KC.wgrad_cells(pl, shape)
    nb = lib.bg_conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, k, s)       # the slab count, from the library itself
    assert nb == (slabs * k * k * Ci * Co * 4 if slabs > 1 else 0)


def test_the_tables_hit_every_cell():
    routes = {c[0]: c for c in KC.ROUTE_CASES}
    fwd = set().union(*[c[2] for c in KC.ROUTE_CASES])
    bwd = set().union(*[c[4] for c in KC.ROUTE_CASES])
    assert fwd | bwd == ROUTE_CELLS, ((fwd | bwd) ^ ROUTE_CELLS)
    assert set().union(*[c[3] for c in KC.WGRAD_CASES]) == WGRAD_CELLS, set().union(*[c[3] for c in KC.WGRAD_CASES]) ^ WGRAD_CELLS
    # every launch name a k != 5 call can record, in both directions
    assert {c[1] + "_fwd" for c in KC.ROUTE_CASES if c[1]} == FWD_NAMES and {c[3] + "_dgrad" for c in KC.ROUTE_CASES if c[3]} == DGRAD_NAMES
    # a case that is split forward and unsplit in the data gradient
    assert CC.route(0, 5, 2, 2, 256, 512, 2, 3)["ks"] == 4 and CC.route(1, 5, 2, 2, 256, 512, 2, 3)["ks"] == 1
    # k = 1 stride 2: three of the four data-gradient phases have no tap, on both tiles, and the merged pair (1, 2) has none
    for shape in ((128, 8, 8, 32, 64, 2, 1), (3, 6, 6, 64, 32, 2, 1), (3, 14, 14, 4, 32, 2, 1), (513, 16, 16, 8, 16, 2, 1)):
        p = CC.gather_params(1, *shape[:5], 1, 2)
        assert [len(g["taps"]) for g in p["ph"]] == [1, 0, 0, 0]
    p = CC.gather_params(1, 513, 16, 16, 8, 16, 1, 2)
    assert CC.tapless_groups(p, 2) == [1] and CC.tapless_groups(p, 1) == [1, 2, 3] and CC.tapless_groups(p, 4) == []
    assert CC.tapless_groups(CC.gather_params(1, 513, 16, 16, 8, 16, 3, 2), 2) == []
    # SAME pads of k = 3 stride 2: (0, 1) on even maps, (1, 1) on odd ones
    assert KC.k3s2_pads(8, 8) == (0, 0) and KC.k3s2_pads(7, 7) == (1, 1) and KC.k3s2_pads(9, 7) == (1, 1) and KC.k3s2_pads(31, 32) == (1, 0)
    # the 24-pixel row: both row kernels decline, in both directions
    assert all(f(b, 2, 20, 24, 2, 32, 3, 1) is None for f in (CC.try_rows, CC.try_rows_gather) for b in (0, 1))
    # production geometry is 3x3 stride 1 and in the route table
    assert set(KC.PRODUCTION) <= set(routes) and all(c[5:] == (1, 3) for c in KC.PRODUCTION)
    # the 5x5-only fast paths step aside: the same geometry is on them at k = 5 and on the generic family / mode at k = 3
    for shape in KC.C16_SHAPES:
        for b in (0, 1):
            assert CC.route(b, *shape[:6])["family"] == CC.C16 and CC.route(b, *shape)["family"] == CC.IG and routes[shape][1 + 2 * b] == CC.IG
    wg = {c[0]: c for c in KC.WGRAD_CASES}
    assert set(KC.STEP_ASIDE_WGRAD) <= set(wg) and {m5 for m5, _ in KC.STEP_ASIDE_WGRAD.values()} == {32, 33, 7}
    assert sorted(CC.plan_wgrad(*c[:6])["Wo"] for c, (m5, _) in KC.STEP_ASIDE_WGRAD.items() if m5 == 33) == [8, 16, 32]
    for shape, (m5, m3) in KC.STEP_ASIDE_WGRAD.items():
        assert CC.plan_wgrad(*shape[:6])["mode"] == m5 and CC.plan_wgrad(*shape)["mode"] == m3 == wg[shape][1], shape
    # the wide rows fall back from the row-MFMA kernels to the generic thin kernels; at half the width they are on mode 31 / 30
    for (B, H, W, Ci, Co, s, k), (wide, half) in KC.WIDE_ROWS.items():
        assert CC.plan_wgrad(B, H, W, Ci, Co, s, k)["mode"] == wide == wg[B, H, W, Ci, Co, s, k][1]
        assert CC.plan_wgrad(B, H, W // 2, Ci, Co, s, k)["mode"] == half
    # the largest case is the tap-grouped step-aside shape; above a million elements only the merged-phase data gradients
    size = lambda c: max(c[0] * c[1] * c[2] * c[3], c[0] * CC.cdiv(c[1], c[5]) * CC.cdiv(c[2], c[5]) * c[4])
    big = {c for c in list(routes) + list(wg) if size(c) > 1 << 20}
    assert big == {(128, 32, 32, 16, 16, 1, 3), (640, 16, 16, 8, 16, 2, 3), (513, 16, 16, 8, 16, 2, 3), (640, 16, 16, 8, 16, 2, 1),
                   (513, 16, 16, 8, 16, 2, 1)} and max(map(size, big)) == 128 * 32 * 32 * 16
    # the per-family tables stay inside the route tables, in a direction the case lists
    for b, c in KC.EPI_CASES + KC.STATS_CASES + KC.ISOLATION_ROUTES:
        assert c in routes and routes[c][1 + 2 * b] is not None, (b, c)
    assert set(KC.ISOLATION_WGRAD) <= set(wg)
    assert all(CC.route(b, *c, stats=True, workspace=False)["stats_rows"] > 0 for b, c in KC.STATS_CASES)
    st = {(b, c): CC.route(b, *c, stats=True, workspace=False) for b, c in KC.STATS_CASES}
    assert st[0, (128, 4, 4, 64, 64, 1, 3)]["sorted"] and st[1, (513, 16, 16, 8, 16, 2, 1)]["pmerge"] == 2
    name = lambda tbl: {CC.route(b, *c)["names"][0] for b, c in tbl}
    family = lambda names: {n.rsplit("_", 1)[0] for n in names}
    assert family(name(KC.ISOLATION_ROUTES)) == family(name(KC.EPI_CASES)) == family(FWD_NAMES | DGRAD_NAMES)
    assert all(c[0] >= 2 for _, c in KC.ISOLATION_ROUTES)
    assert {CC.plan_wgrad(*c)["names"][0] for c in KC.ISOLATION_WGRAD} == set(CC.WG_NAMES[m] for m in (0, 30, 31)) | {"conv_wgrad_mfma"}


def _sweep(n, seed):
    """The geometry distribution of tests/test_conv_cases_cpu.py with k drawn from {1, 3}, and widths the row kernels take."""
    rng = np.random.default_rng(seed)
    chans = [1, 2, 3, 4, 5, 8, 12, 16, 20, 24, 32, 36, 48, 64, 96, 128, 256, 512, 1024]
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 16, 17, 20, 24, 31, 32, 33, 63, 64, 65, 128, 130, 255, 256, 257]
    out = []
    while len(out) < n:
        B = int(rng.choice([1, 2, 3, 5, 8, 16, 32, 33, 64, 128, 130, 256, 384, 512, 513, 640, 1024, 2048, 8192, 14564, 131072]))
        H = int(rng.choice(sizes))
        W = int(rng.choice(sizes)) if rng.uniform() < 0.5 else H
        Ci, Co, s, k = int(rng.choice(chans)), int(rng.choice(chans)), int(rng.choice([1, 2])), int(rng.choice([1, 3]))
        if B * H * W * max(Ci, Co) < 1 << 29:
            out.append((B, H, W, Ci, Co, s, k))
    return out


def test_the_restated_planners_agree_with_the_library_at_k_1_and_3(lib):
    cases = [c[0] for c in KC.ROUTE_CASES] + [c[0] for c in KC.WGRAD_CASES] + _sweep(3000, 20261019)
    cases += [(B, H, W, Ci, Co, s, k) for (_, H, W, Ci, Co, s) in CC.X6_TABLE for B in (1, 8, 256) for k in (1, 3)]     # the bf16x6 table is 5x5 only
    modes, families = {1: set(), 3: set()}, {1: set(), 3: set()}
    for (B, H, W, Ci, Co, s, k) in cases:
        pl = CC.plan_wgrad(B, H, W, Ci, Co, s, k)
        modes[k].add(pl["mode"])
        assert lib.bg_conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, k, s) == pl["ws_bytes"], (B, H, W, Ci, Co, s, k, pl)
        for bwd in (0, 1):
            assert lib.bg_conv2d_splitk_workspace_bytes(bwd, B, H, W, Ci, Co, k, s) == CC.splitk_workspace_bytes(bwd, B, H, W, Ci, Co, k, s), \
                (bwd, B, H, W, Ci, Co, s, k)
            assert not lib.bg_conv2d_math_taken(bwd, B, H, W, Ci, Co, k, s, 1) and not CC.math_taken(bwd, B, H, W, Ci, Co, k, s)
            assert not lib.bg_conv2d_math_taken(bwd, B, H, W, Ci, Co, k, s, 0)
            families[k].add(CC.route(bwd, B, H, W, Ci, Co, s, k)["family"])                     # total: every geometry has a route
    # the filter-gradient modes the sweep and the tables reach: never a 5x5-only one (6, 7, 32, 33), never 12 / 22 (k k C <= 36), and
    # at k = 1 no row-MFMA mode (30 / 31 take k = 5 and 3) and no mode 11 / 21 (C <= 4 rows of taps x channels)
    assert modes[3] == {0, 1, 2, 3, 4, 5, 10, 11, 20, 21, 30, 31}, modes[3]
    assert modes[1] == {0, 1, 2, 3, 4, 5, 10, 20}, modes[1]
    every = {"conv_igemm", "conv_thin_n_mfma", "conv_thin_n_patch_all", "conv_thin_n_patch", "conv_thin_n", "conv_thin_k_mfma", "conv_thin_k", "conv_direct"}
    assert families[3] == every | {CC.RS, CC.RG} and families[1] == every, (families[3] ^ every, families[1] ^ every)
