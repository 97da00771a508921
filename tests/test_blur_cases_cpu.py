"""CPU: the blur case table of tests/blur_cases.py held to its claims -- every case exact in float32 in two summation orders, on
the route and instantiation it is in the table for, every cell of the table hit -- and the restated host predicates held to the
library's own host-only entry points (bg_blur_workspace_bytes, bg_blur3_lerp_supported)."""
import os

import numpy as np
import pytest

import blur_cases as BC

IDS = [BC.case_id(c) for c in BC.CASES]


@pytest.fixture(scope="module")
def lib():
    from blurred_gan_amd import _lib
    assert not [k for k in BC.STATIC_SWITCHES + BC.CALL_SWITCHES if k in os.environ], "blur switches set in the environment"
    return _lib.load()


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_case_is_exact_in_float32(case):
    """Both bounds, and the proof by evaluation: float32 along H then W with the taps ascending, and along W then H with the taps
    descending, equal the float64 reference bit for bit."""
    shape, T = case[0], case[1]
    long_line = shape in ((1, 4, 4000, 5), (1, 600, 8, 5), (2, 600, 8, 5))          # the rows_per == 1 and generic-pass cases: one long, thin image
    assert T & 1 and shape[0] <= 16 and (max(shape[1:3]) <= 512 or long_line) and np.prod(shape) <= 1 << 20
    for recipe in BC.recipes(case):
        x, t = BC.make(case, recipe)
        if recipe == "dense":
            assert (t != 0).all() and set(np.abs(t)) <= {1.0, 2.0, 3.0}
            assert T == 1 or not np.array_equal(t, t[::-1])
            assert np.abs(t).sum() ** 2 * np.abs(x).max() < BC.TWO24 and np.abs(x).max() <= 8
        elif recipe == "ramp":
            assert T <= 65 and t.sum() ** 2 * 3 < BC.TWO24
        else:
            assert len(set(t)) == T and x.reshape(shape[0], -1).sum(1).max() <= 64 and 64 * T * T < BC.TWO24
            assert set(np.unique(x)) <= {0.0, 1.0}
            assert x[:, 0, 0].any(-1).all() and x[:, -1, -1].any(-1).all() and x[:, 0, -1].any(-1).all() and x[:, -1, 0].any(-1).all()
            assert shape[0] == 1 or any(not np.array_equal(x[0], x[b]) for b in range(1, shape[0]))
        ref = BC.reference(x, t)
        assert np.abs(ref).max() < BC.TWO24
        a, b = BC.f32_two_orders(x, t)
        assert a.dtype == np.float32 and b.dtype == np.float32
        assert np.array_equal(a.astype(np.float64), ref) and np.array_equal(b.astype(np.float64), ref), recipe


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_case_is_on_its_claimed_route(case):
    shape, T, family, claim, env = case
    d = BC.described(case)
    assert d["family"] == family and d["names"] == BC.NAMES[family], d
    wrong = {k: (v, d.get(k)) for k, v in claim.items() if d.get(k) != v}
    assert not wrong, f"claimed != restated: {wrong}"
    assert set(env) <= set(BC.CALL_SWITCHES)


def test_the_table_hits_every_cell():
    assert BC.missing_cells() == []
    # the check can fail: without the forced-loader cases their cells are reported
    fewer = [c for c in BC.CASES if "BG_BLUR_BAND_LD" not in c[4]]
    assert BC.missing_cells(fewer) == [f"band: C = {c}, loader 0 forced" for c in (1, 2, 3, 4)]


def test_impulses_sit_on_both_sides_of_the_seams():
    """Over the images of a case the impulses cover the seam rows and columns of its route (a single image takes at most 64)."""
    for case in BC.CASES:
        x, _ = BC.make(case, "impulse")
        rows, cols, split_r, split_c = BC.seams(case)
        hit_r, hit_c = set(np.nonzero(x.any((0, 2, 3)))[0]), set(np.nonzero(x.any((0, 1, 3)))[0])
        n_seam = 2 * (len(rows) + len(cols)) + len(split_r) + len(split_c)
        if n_seam <= 60:
            assert all(s - 1 in hit_r and s in hit_r for s in rows), BC.case_id(case)
            assert all(s - 1 in hit_c and s in hit_c for s in cols), BC.case_id(case)
            assert all(x[:, :, p, c].any() for p, c in split_c) and all(x[:, p, :, c].any() for p, c in split_r), BC.case_id(case)
        else:
            on_seam = len(hit_r & (rows | {s - 1 for s in rows})) + len(hit_c & (cols | {s - 1 for s in cols}))
            on_seam += sum(bool(x[:, :, p, c].any()) for p, c in split_c) + sum(bool(x[:, p, :, c].any()) for p, c in split_r)
            assert on_seam >= 20, BC.case_id(case)


def test_three_source_cases_are_exact_and_supported():
    for c3 in BC.CASES3:
        B, H, W, C, T = c3
        assert BC.blur3_supported(B, H, W, C, T)
        f, r, a, t = BC.make3(c3)
        assert (f % 4 == 0).all() and (r % 4 == 0).all() and np.abs(f).max() <= 8 and np.abs(r).max() <= 8 and set(a) <= set(BC.ALPHAS)
        a32 = a.astype(np.float32)[:, None, None, None]
        f32, r32 = f.astype(np.float32), r.astype(np.float32)
        xhat = r32 + a32 * (f32 - r32)
        assert xhat.dtype == np.float32 and np.array_equal(xhat.astype(np.float64), r + a[:, None, None, None] * (f - r))
        assert (xhat == np.round(xhat)).all() and np.abs(xhat).max() <= 8
        ref = BC.reference3(f, r, a, t)
        for i, src in enumerate((f32, r32, xhat)):
            p, q = BC.f32_two_orders(src, t)
            assert np.array_equal(p.astype(np.float64), ref[i * B:(i + 1) * B]) and np.array_equal(q.astype(np.float64), ref[i * B:(i + 1) * B])
    assert {c[4] for c in BC.CASES3} >= {3, 7} and len({a for c in BC.CASES3 for a in BC.make3(c)[2]}) == 5


def test_decode_names_the_taps():
    case = BC.CASES[0]
    x, t = BC.make(case, "impulse")
    ref = BC.reference(x, t)
    assert BC.decode(x, t, ref, ref) == "equal"
    wrong = BC.reference(x, t[::-1].copy())                 # the kernel that applies the taps reversed
    msg = BC.decode(x, t, wrong, ref)
    assert "first at" in msg and "should sum" in msg


def _sweep(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        kind = int(rng.integers(4))
        if kind == 0:          # around the small-image limits
            H, W = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        elif kind == 1:        # panel geometries
            H, W = 32 * int(rng.integers(1, 18)), 32 * int(rng.integers(1, 10))
        else:
            H, W = int(rng.integers(1, 600)), int(rng.integers(1, 600))
        C = int(rng.choice([1, 2, 3, 3, 4, 5, 8, 16, 17]))
        T = 2 * int(rng.choice([rng.integers(0, 8), rng.integers(0, 40), rng.integers(0, 300), rng.integers(0, 520)])) + 1
        out.append((int(rng.integers(1, 17)), H, W, C, T))
    return out


def test_restated_path_matches_the_library(lib, monkeypatch):
    """bg_blur_workspace_bytes is zero exactly where the restated path is not 2 or 3 and B H W C 4 otherwise; bg_blur3_lerp_supported
    equals the restated rule -- for every case (under its switches) and a seeded sweep, plain and under each per-call switch."""
    def check(B, H, W, C, T, env):
        want = BC.workspace_bytes(B, H, W, C, T, env)
        assert (want != 0) == (BC.blur_path(B, H, W, C, T, env) in (2, 3)) and want in (0, B * H * W * C * 4)
        assert lib.bg_blur_workspace_bytes(B, H, W, C, T) == want, (B, H, W, C, T, env)
        assert bool(lib.bg_blur3_lerp_supported(B, H, W, C, T)) == BC.blur3_supported(B, H, W, C, T, env), (B, H, W, C, T, env)

    for shape, T, _, _, env in BC.CASES:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            check(*shape, T, env)
    for c3 in BC.CASES3:
        check(*c3, {})
    sweep = _sweep(4000, 20261019)
    paths = {BC.blur_path(*s) for s in sweep}
    assert paths == {0, 1, 2, 3, 4, 5, 6}
    for s in sweep:
        check(*s, {})
    for env in ({"BG_BLUR_NO_ROWS": "1"}, {"BG_BLUR_NO_PANEL": "1"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for s in sweep[:1500]:
                check(*s, env)
    assert lib.bg_blur_workspace_bytes(0, 8, 8, 3, 3) == 0 and not lib.bg_blur3_lerp_supported(2, 8, 8, 3, 4)
