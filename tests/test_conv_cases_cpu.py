"""CPU: the 5x5 conv case tables of tests/conv_cases.py held to their claims -- every case exact in float32 (the float32 oracle
equals the float64 oracle bit for bit, and the magnitude bound is below 2^24), on the family, mode and variant it is listed under,
every cell of the route list hit -- and the restated planners held to the library's own host-only entry points
(bg_conv2d_bwd_filter_workspace_bytes, bg_conv2d_splitk_workspace_bytes, bg_conv2d_math_taken) over the tables and a seeded sweep,
once more in a fresh process with the once-read switches that take the 5x5-only fast paths away."""
import os

import numpy as np
import pytest

import conv_cases as CC

ROUTE_IDS = [CC.case_id(c[0]) for c in CC.ROUTE_CASES]
WGRAD_IDS = [CC.case_id(c[0]) for c in CC.WGRAD_CASES]
f32 = lambda a: a.astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    from blurred_gan_amd import _lib
    assert not [k for k in CC.STATIC_SWITCHES if k in os.environ], "conv tuning switches set in the environment"
    return _lib.load()


def test_case_ids_are_unique():
    assert len(set(ROUTE_IDS)) == len(ROUTE_IDS) and len(set(WGRAD_IDS)) == len(WGRAD_IDS)


def _same_in_float32(fn, ref, *arrays):
    got = fn(*[f32(a) for a in arrays])
    assert got.dtype == np.float32
    assert np.abs(ref).max() < CC.TWO24
    assert np.array_equal(got.astype(np.float64), ref)


def _check_impulses(a, k=5):
    """One-hot in the channel, the four corners where the map has room for them, no two within a k x k window, images differ."""
    B, H, W, C = a.shape
    assert set(np.unique(a)) <= {0.0, 1.0}
    occ = a.sum(-1)
    assert occ.max() == 1 and occ[:, 0, 0].all()
    if min(H, W) > k:
        assert occ[:, 0, W - 1].all() and occ[:, H - 1, 0].all() and occ[:, H - 1, W - 1].all()
    pad = np.pad(occ, ((0, 0), (k - 1, k - 1), (k - 1, k - 1)))
    win = sum(pad[:, i:i + H + k - 1, j:j + W + k - 1] for i in range(k) for j in range(k))     # impulses per k x k window
    assert win.max() == 1
    only_corners = C == 1 and max(H, W) <= 2 * k - 1          # one channel and no pixel k away from every corner: one possible set
    assert B == 1 or only_corners or any(not np.array_equal(a[0], a[b]) for b in range(1, B))


@pytest.mark.parametrize("case", CC.ROUTE_CASES, ids=ROUTE_IDS)
def test_forward_and_data_gradient_cases_are_exact_in_float32(case):
    shape = case[0]
    B, H, W, Ci, Co, s = shape
    assert 25 * max(Ci, Co) * CC.dense_m(25 * max(Ci, Co)) ** 2 < CC.TWO24 and 25 * Ci * Co + 25 < CC.TWO24
    for recipe in ("dense", "decode"):
        x, w = CC.make_fwd(shape, recipe)
        dy, w2 = CC.make_dgrad(shape, recipe)
        if recipe == "dense":
            m = CC.dense_m(25 * Ci)
            assert np.abs(x).max() <= m and np.abs(w).max() <= m and 25 * Ci * m * m < CC.TWO24
            m = CC.dense_m(25 * Co)
            assert np.abs(dy).max() <= m and np.abs(w2).max() <= m and 25 * Co * m * m < CC.TWO24
        else:
            _check_impulses(x)
            _check_impulses(dy)
            assert np.array_equal(w, w2) and len(np.unique(w)) == w.size and w.min() == 1 and w.max() < CC.TWO24
        ref = CC.ref_fwd(x, w, s)
        _same_in_float32(lambda a, b: CC.ref_fwd(a, b, s), ref, x, w)
        refd = CC.ref_dgrad(dy, w2, s, (H, W))
        _same_in_float32(lambda a, b: CC.ref_dgrad(a, b, s, (H, W)), refd, dy, w2)
        if recipe == "decode":                         # every output IS one weight (or 0): the decoder reads it back
            nz = ref[ref != 0]
            assert nz.size and np.isin(nz, w).all() and np.isin(refd[refd != 0], w).all()
            kh, kw, ci, co = CC.decode_weight(nz[0], Ci)
            assert w[kh, kw, ci, co] == nz[0]


@pytest.mark.parametrize("case", CC.WGRAD_CASES, ids=WGRAD_IDS)
def test_filter_gradient_cases_are_exact_in_float32(case):
    shape = case[0]
    B, H, W, Ci, Co, s = shape
    M = B * CC.cdiv(H, s) * CC.cdiv(W, s)
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
        ref = CC.ref_wgrad(x, dy, s)
        assert 2 * np.abs(ref).max() + 8 < CC.TWO24          # the accumulate form: 0.5 dw0 + 2 grad, |dw0| <= 8
        _same_in_float32(lambda a, b: CC.ref_wgrad(a, b, s), ref, x, dy)


def test_a_wrong_filter_gradient_element_names_its_pixel():
    shape = (2, 7, 9, 16, 16, 1)
    x, dy, pix = CC.make_wgrad(shape, "decode")
    ref = CC.ref_wgrad(x, dy, 1)
    got = ref.copy()
    got[1, 2, 3, 4] -= 2 * 8.0 ** 3                     # digit 3 of channel 4 is off by 2
    msg = CC.decode_wgrad(got, ref, pix, shape)
    assert "tap (1, 2) ci 3 co 4" in msg and "digit 3" in msg and f"m={int(pix[4, 3])} " in msg, msg


@pytest.mark.parametrize("case", CC.ROUTE_CASES, ids=ROUTE_IDS)
def test_forward_and_data_gradient_cases_are_on_their_claimed_routes(case):
    shape, ff, fc, df, dc = case
    for bwd, fam, cells in ((0, ff, fc), (1, df, dc)):
        d = CC.route(bwd, *shape)
        assert d["family"] == fam and d["names"][0] == fam + ("_dgrad" if bwd else "_fwd"), d
        assert cells <= CC.route_cells(bwd, d, shape[0]), (bwd, cells - CC.route_cells(bwd, d, shape[0]))


@pytest.mark.parametrize("case", CC.WGRAD_CASES, ids=WGRAD_IDS)
def test_filter_gradient_cases_are_on_their_claimed_modes(case, lib):
    shape, mode, slabs, cells = case
    pl = CC.plan_wgrad(*shape)
    assert (pl["mode"], pl["ksplit"]) == (mode, slabs), (pl["mode"], pl["ksplit"])
    assert cells <= CC.wgrad_cells(pl, shape[0], shape[5]), cells - CC.wgrad_cells(pl, shape[0], shape[5])
    B, H, W, Ci, Co, s = shape
    nb = lib.bg_conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, 5, s)       # the slab count, from the library itself
    assert nb == (slabs * 25 * Ci * Co * 4 if slabs > 1 or mode == 33 else 0)


def test_the_tables_hit_every_cell():
    fwd = set().union(*[c[2] for c in CC.ROUTE_CASES])
    bwd = set().union(*[c[4] for c in CC.ROUTE_CASES])
    assert fwd | bwd == CC.ROUTE_CELLS, ((fwd | bwd) ^ CC.ROUTE_CELLS)
    assert set().union(*[c[3] for c in CC.WGRAD_CASES]) == CC.WGRAD_CELLS
    assert all(any(c.startswith("igemm:splitk") for c in got) for got in (fwd, bwd))             # split-K in both directions
    # the tap-grouped kernel in depth: the shapes, with the slab counts of the planner
    tg = {c[0]: (c[1], c[2]) for c in CC.WGRAD_CASES if c[1] in (6, 7) or c[0] == (2, 255, 257, 16, 16, 1)}
    assert tg == {(2, 256, 256, 16, 16, 1): (7, 152), (2, 256, 256, 16, 64, 1): (6, 152), (32, 130, 130, 16, 64, 2): (6, 151),
                  (8192, 4, 4, 16, 16, 1): (7, 152), (131072, 1, 1, 16, 32, 1): (7, 152), (14564, 3, 3, 32, 48, 1): (6, 152),
                  (8, 128, 128, 20, 36, 1): (6, 152), (2, 255, 257, 16, 16, 1): (5, 20), (33, 63, 65, 48, 40, 1): (6, 77)}
    # the per-family tables stay inside the route tables
    routes = {c[0] for c in CC.ROUTE_CASES}
    assert {c for _, c in CC.EPI_CASES + CC.STATS_CASES + CC.ISOLATION_ROUTES} <= routes
    assert set(CC.ISOLATION_WGRAD) <= {c[0] for c in CC.WGRAD_CASES}
    assert all(CC.route(b, *c, stats=True, workspace=False)["stats_rows"] > 0 for b, c in CC.STATS_CASES)
    fam = lambda tbl: {CC.route(b, *c)["names"][0] for b, c in tbl}
    every = {CC.route(b, *c[0])["names"][0] for c in CC.ROUTE_CASES for b in (0, 1)}
    assert fam(CC.ISOLATION_ROUTES) | {"conv_thin_n_patch_dgrad", "conv_thin_k_dgrad", "conv_thin_n_dgrad", "conv_direct_dgrad",
                                       "conv_thin_k_mfma_dgrad"} == every
    assert all(c[0] >= 2 for _, c in CC.ISOLATION_ROUTES)


def _sweep(n, seed):
    rng = np.random.default_rng(seed)
    chans = [1, 2, 3, 4, 5, 8, 12, 16, 20, 24, 32, 36, 48, 64, 96, 128, 256, 512]
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 128, 130, 255, 256, 257]
    out = []
    while len(out) < n:
        B = int(rng.choice([1, 2, 3, 5, 8, 16, 32, 33, 64, 128, 130, 256, 384, 512, 1024, 2048, 8192, 14564, 131072]))
        H = int(rng.choice(sizes))
        W = int(rng.choice(sizes)) if rng.uniform() < 0.5 else H
        Ci, Co, s = int(rng.choice(chans)), int(rng.choice(chans)), int(rng.choice([1, 2]))
        if B * H * W * max(Ci, Co) < 1 << 29:
            out.append((B, H, W, Ci, Co, s))
    return out


def test_the_restated_planners_agree_with_the_library(lib):
    cases = [c[0] for c in CC.ROUTE_CASES] + [c[0] for c in CC.WGRAD_CASES] + _sweep(3000, 20261019)
    cases += [(B, H, W, Ci, Co, s) for (_, H, W, Ci, Co, s) in CC.X6_TABLE for B in (1, 8, 256)]
    cases += [(256, 32, 32, 64, 128, 1), (256, 64, 64, 64, 32, 2), (8, 8, 8, 64, 128, 2)]            # near misses of the bf16x6 table
    modes = set()
    for (B, H, W, Ci, Co, s) in cases:
        pl = CC.plan_wgrad(B, H, W, Ci, Co, s)
        modes.add(pl["mode"])
        assert lib.bg_conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, 5, s) == pl["ws_bytes"], (B, H, W, Ci, Co, s, pl)
        for bwd in (0, 1):
            assert lib.bg_conv2d_splitk_workspace_bytes(bwd, B, H, W, Ci, Co, 5, s) == CC.splitk_workspace_bytes(bwd, B, H, W, Ci, Co, 5, s), \
                (bwd, B, H, W, Ci, Co, s)
            assert bool(lib.bg_conv2d_math_taken(bwd, B, H, W, Ci, Co, 5, s, 1)) == CC.math_taken(bwd, B, H, W, Ci, Co, 5, s), (bwd, B, H, W, Ci, Co, s)
            assert not lib.bg_conv2d_math_taken(bwd, B, H, W, Ci, Co, 5, s, 0)
            CC.route(bwd, B, H, W, Ci, Co, s)                                                      # total: every geometry has a route
    assert modes == {0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 20, 21, 22, 30, 31, 32, 33}
    assert any(CC.math_taken(b, *c[:5], 5, c[5]) for c in cases for b in (0, 1))


def test_the_restated_planners_agree_with_the_library_under_the_once_read_switches(lib):
    """BG_NO_C16, BG_NO_ROWS, BG_WGRAD_NO_STRIP, BG_WGRAD_NO_TC, BG_WGRAD_NO_TG are process-wide statics of the library: a fresh
    process started with them set compares the planners again (no fast-path family or mode may remain) and holds the cases of the
    fallbacks to the families and modes they are listed under."""
    assert not CC.OFF
    print(CC.run_switched_child("plan"))
