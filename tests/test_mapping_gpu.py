"""GPU tests of the mapping-network kernels (csrc/mapping.hip; include/bgan.h "mapping network") against tests/mapping_reference.py:
bg_dense_lrelu_f32, bg_lrelu_bias_bwd_f32 and bg_truncate_f32 exactly on small-integer data (every intermediate is exact in float32:
sums stay far below 2^24, the factors are powers of two), on sizes around the tile and the K-step as the library reports them, 16-byte
aligned and one float off, with guard bands around every output; then bg_dense_lrelu_f32 on normal data against float64 with the
tolerance tests/test_misc_gpu.py holds bg_gemm_f32 to."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import Guarded
import mapping_reference as R

pytestmark = pytest.mark.gpu

PLAN = None


def _plan():
    global PLAN
    if PLAN is None:
        PLAN = ops.mapping.plan(256, 512, 512)
    return PLAN


def _ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _dense_cases():
    """A covering set: every M and N of {1, T - 1, T, T + 1, 2 T + 3} and every K of {1, T_K - 1, T_K, T_K + 1, 3 T_K + 2} in three
    rotations against each other, and the two workload shapes.  T = 32 and T_K = 64 as built: the test asserts that the library
    still reports them, so a changed tile fails here first."""
    T, TK = 32, 64
    S, Ks = [1, T - 1, T, T + 1, 2 * T + 3], [1, TK - 1, TK, TK + 1, 3 * TK + 2]
    out = [(S[i], S[(i + r) % 5], Ks[(i + 2 * r) % 5]) for r in range(3) for i in range(5)]
    return out + [(256, 512, 512), (256, 100, 100)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("idx,shape", list(enumerate(_dense_cases())))
def test_dense_lrelu_exact(idx, shape, offset):
    p = _plan()
    assert (p["tile_m"], p["tile_n"], p["tile_k"]) == (32, 32, 64), p
    M, N, K = shape
    rng = np.random.default_rng(100 + idx)
    x, W, b = _ints(rng, M, K), _ints(rng, K, N), _ints(rng, N)
    # null and non-null bias, both alphas, both c and both bias multipliers all occur at either offset and on either side of a tile edge
    has_bias, alpha = (idx + offset) % 2 == 0, (1.0, 0.25)[(idx // 2) % 2]
    c, bm = (1.0, 0.5)[(idx // 3) % 2], (1.0, 0.25)[idx % 2]
    gx, gW, gb, gy = Guarded(M * K, x, offset=offset), Guarded(K * N, W, offset=offset), Guarded(N, b, offset=offset), Guarded(M * N, offset=offset)
    ops.mapping.dense_lrelu(gx.t(M, K), gW.t(K, N), gb.view if has_bias else None, gy.t(M, N), M, N, K, c=c, bias_mul=bm, alpha=alpha)
    ref = R.np_dense_lrelu(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64) if has_bias else None, c, bm, alpha)
    got = gy.get(M, N)
    assert np.array_equal(got, ref.astype(np.float32)), (shape, np.abs(got - ref).max())
    assert gy.guards_intact() and gx.unchanged() and gW.unchanged() and gb.unchanged()
    first = got.view(np.uint32).copy()
    ops.mapping.dense_lrelu(gx.t(M, K), gW.t(K, N), gb.view if has_bias else None, gy.t(M, N), M, N, K, c=c, bias_mul=bm, alpha=alpha)
    assert np.array_equal(gy.get(M, N).view(np.uint32), first)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", [(256, 512, 512), (256, 100, 100), (33, 67, 194), (5, 3, 65)])
def test_dense_lrelu_float(shape, offset):
    """Normal data against float64: rtol 1e-4, atol 1e-4 * sqrt(K), bg_gemm_f32's tolerance in tests/test_misc_gpu.py; two runs give
    the same bits."""
    M, N, K = shape
    rng = np.random.default_rng(7)
    x, W, b = (rng.normal(size=s).astype(np.float32) for s in ((M, K), (K, N), (N,)))
    c, bm, alpha = float(np.float32(np.sqrt(2.0 / K))), 0.5, 0.2
    gx, gW, gb, gy = Guarded(M * K, x, offset=offset), Guarded(K * N, W, offset=offset), Guarded(N, b, offset=offset), Guarded(M * N, offset=offset)
    ops.mapping.dense_lrelu(gx.t(M, K), gW.t(K, N), gb.view, gy.t(M, N), M, N, K, c=c, bias_mul=bm, alpha=alpha)
    got = gy.get(M, N)
    ref = R.np_dense_lrelu(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), c, bm, alpha)
    err = np.abs(got - ref)
    print(f"{shape} offset {offset}: max err {err.max():.3e}")
    assert np.all(err <= 1e-4 * np.sqrt(K) + 1e-4 * np.abs(ref))
    assert gy.guards_intact()
    ops.mapping.dense_lrelu(gx.t(M, K), gW.t(K, N), gb.view, gy.t(M, N), M, N, K, c=c, bias_mul=bm, alpha=alpha)
    assert np.array_equal(gy.get(M, N).view(np.uint32), got.view(np.uint32))


def test_dense_lrelu_refusals():
    t = torch.zeros(16, device="cuda")
    with pytest.raises(ValueError):
        ops.mapping.dense_lrelu(t, t, None, t, 4, 4, 4)            # y aliases x
    from blurred_gan_amd import _lib
    assert _lib.load().bg_dense_lrelu_f32(None, None, None, None, 1, 1, 1, 1.0, 1.0, 1.0, None) != 0


# N: one float per row; float4 units with 1, 2 and 4 per lane; the same by single floats; the chunked routes of either kind.
# M: fewer rows than a workgroup visits at once, a ragged last visit, and (N = 512: 4 rows per visit, 1024 workgroups) a second trip.
BWD_CASES = [(1, 1), (5, 1), (300, 1), (2, 3), (257, 4), (64, 8), (70, 100), (33, 101), (19, 256), (9, 260), (6, 512), (4101, 512),
             (3, 1028), (5, 301), (1030, 36)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("idx,shape", list(enumerate(BWD_CASES)))
def test_lrelu_bias_bwd_exact(idx, shape, inplace, offset):
    M, N = shape
    rng = np.random.default_rng(200 + idx)
    g, y, old = _ints(rng, M, N), _ints(rng, M, N), _ints(rng, N)            # y holds zeros: the kink goes with alpha
    alpha, beta, scale = 0.25, float((idx + offset) % 2), (1.0, 0.5)[idx % 2]
    gg, gy_, gd = Guarded(M * N, g, offset=offset), Guarded(M * N, y, offset=offset), Guarded(N, old, offset=offset)
    gp = gg if inplace else Guarded(M * N, offset=offset)
    ws = torch.empty(ops.mapping.workspace_bytes(M, N) // 4 + 4, device="cuda")
    ops.mapping.lrelu_bias_bwd(gg.t(M, N), gy_.t(M, N), gp.t(M, N), gd.view, M, N, ws, alpha=alpha, beta=beta, scale=scale)
    rgp, rdb = R.np_lrelu_bias_bwd(g.astype(np.float64), y.astype(np.float64), alpha, old.astype(np.float64), beta, scale)
    assert np.array_equal(gp.get(M, N), rgp.astype(np.float32))
    assert np.array_equal(gd.get(), rdb.astype(np.float32)), np.abs(gd.get() - rdb).max()
    assert gp.guards_intact() and gd.guards_intact() and gy_.unchanged() and (inplace or gg.unchanged())
    if not inplace:             # a second run: the same bits (beta = 0) / one more multiple (beta = 1)
        ops.mapping.lrelu_bias_bwd(gg.t(M, N), gy_.t(M, N), gp.t(M, N), gd.view, M, N, ws, alpha=alpha, beta=0.0, scale=scale)
        assert np.array_equal(gd.get(), (scale * rgp.sum(0)).astype(np.float32))


def test_lrelu_bias_bwd_refusals():
    t, d = torch.zeros(16, device="cuda"), torch.zeros(4, device="cuda")
    ws = torch.empty(4096, device="cuda")
    with pytest.raises(ValueError):
        ops.mapping.lrelu_bias_bwd(t, t, t, d, 4, 4, ws)             # gp aliases y
    from blurred_gan_amd import _lib
    with pytest.raises(_lib.BgError):
        ops.mapping.lrelu_bias_bwd(t, t.clone(), t, d, 4, 4, None)     # no workspace


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,U", [(1, 1), (4, 7), (5, 100), (256, 512), (3, 2050)])
def test_truncate_exact(B, U, offset):
    rng = np.random.default_rng(B * 1000 + U)
    w, avg = _ints(rng, B, U), _ints(rng, U)
    for psi in (0.0, 0.5, 1.0):
        gw, ga, go = Guarded(B * U, w, offset=offset), Guarded(U, avg, offset=offset), Guarded(B * U, offset=offset)
        ops.mapping.truncate(gw.t(B, U), ga.view, go.t(B, U), psi, B, U)
        ref = R.np_truncate(w.astype(np.float64), avg.astype(np.float64), psi).astype(np.float32)
        assert np.array_equal(go.get(B, U), ref), psi
        assert go.guards_intact() and gw.unchanged() and ga.unchanged()
        ops.mapping.truncate(gw.t(B, U), ga.view, gw.t(B, U), psi, B, U)          # in place
        assert np.array_equal(gw.get(B, U), ref) and gw.guards_intact()
    # on any data: psi = 1 returns w bit for bit, psi = 0 returns w_avg in every row
    wf, af = rng.normal(size=(B, U)).astype(np.float32), rng.normal(size=U).astype(np.float32)
    gw, ga, go = Guarded(B * U, wf, offset=offset), Guarded(U, af, offset=offset), Guarded(B * U, offset=offset)
    ops.mapping.truncate(gw.t(B, U), ga.view, go.t(B, U), 1.0, B, U)
    assert np.array_equal(go.get(B, U).view(np.uint32), wf.view(np.uint32))
    ops.mapping.truncate(gw.t(B, U), ga.view, go.t(B, U), 0.0, B, U)
    assert np.array_equal(go.get(B, U).view(np.uint32), np.tile(af, (B, 1)).view(np.uint32))
