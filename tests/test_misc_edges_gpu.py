"""GPU: the support kernels of csrc/misc.hip on the routes and loop tails no other direct test enters, on data for which float32
is exact (tests/misc_cases.py; tests/test_misc_cases_cpu.py proves the exactness and the route of every case on the CPU).  Every
exact comparison is array_equal against the float64 reference.  Every output is a view into a larger buffer filled with NaN: the
bands before and after it must stay untouched and no NaN may remain inside.

Cases -> routes and loops:
  test_reductions          colsum (plain, square, beta / scale), bn_stats, bn_bwd_stats (y given / None): flat_reduce with fewer quads than
                           threads, main loop only, main + tail, ragged and empty blocks, G = 256; col_reduce under the flat threshold,
                           with empty blocks and a ragged column group, and ON THE FLAT GRID (x offset by one float); nblk 450 / 512 in
                           wave_sum_partials
  test_partial_rows        wave_sum_partials through bg_bn_sums_from_partials and bg_bn_train_fwd_partials: tail only, 8-deep loop
                           only, and lanes of one wave in different loops (449, 511, 513, 1061)
  test_train_fwd_partials_in_place   y is x
  test_bn_apply_family     bn_apply_kernel / bn_bwd_apply_kernel: two-in-flight loop + epilogue, its second entry, fixed channels,
                           per-iteration parameters (also with a second iteration), scalar path, pa == false, M_total in {M, 2M, 4M},
                           y None against y given
  test_bn_param_grads, test_bn_finalize_apply (bit-identical to finalize + apply, M_total in {M, 2M, 4M}; real-valued)
  test_gemv_t / test_rowdot / test_gemm_tiled_and_naive   route names asserted (dense_gemv_t, dense_rowdot, dense_gemm_tiled, dense_gemm)
  test_pointwise           lerp, outer, mul_grad (+keep), tanh_bwd, fill, scale below / at / beyond one grid-stride pass
  test_copy, test_row_norm, test_losses (norm_b given / None, B below a wave and beyond one pass)
  test_*_real              the outputs that round, against the float64 oracle: bound = max(bound of tests/test_misc_gpu.py,
                           3 x float32-numpy deviation); each prints "[misc parity] <op> <case>: max error / bound"
"""
import math

import numpy as np
import pytest
import torch

import misc_cases as MC
from oracle import np_ops as O

pytestmark = pytest.mark.gpu

PAD = 64          # floats of guard band on either side (256 bytes: the view keeps the alignment its offset asks for)


class Guard:
    """n floats at `off` floats past a 16-byte boundary, inside a NaN-filled buffer."""

    def __init__(self, n, off=0, init=None):
        self.n, self.lo = n, PAD + off
        self.buf = torch.full((n + 2 * PAD + 4,), float("nan"), device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + n]
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).ravel()))

    def get(self, shape=None):
        b = self.buf.cpu().numpy()
        assert np.isnan(b[:self.lo]).all() and np.isnan(b[self.lo + self.n:]).all(), "guard band written"
        inner = b[self.lo:self.lo + self.n]
        assert not np.isnan(inner).any(), "sentinel left inside the output"
        return inner.astype(np.float64).reshape(shape or (self.n,))


def put(a, off=0, dtype=torch.float32):
    """Input tensor `off` elements past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + off + 4, dtype=dtype, device="cuda")
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(a.ravel()).to(dtype))
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    return v


def eq(got, want):
    assert np.array_equal(np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()), \
        f"max |diff| {np.abs(np.asarray(got, np.float64).ravel() - np.asarray(want, np.float64).ravel()).max()}"


def launches(fn):
    from blurred_gan_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.prof_records()]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


def report(op, case, got, ref64, ref32, rtol, atol):
    err, bound, ratio = MC.parity(got, ref64, ref32, rtol, atol)
    print(f"[misc parity] {op} {case}: {err:.3e} / {bound:.3e} (ratio {ratio:.3f})")
    assert ratio <= 1.0, f"{op} {case}: error {err:.3e} exceeds bound {bound:.3e}"


# ------------------------------------------------------------------ column reductions
@pytest.mark.parametrize("shape,off", MC.RED_CASES, ids=[f"{s[0]}x{s[1]}-off{o}" for s, o in MC.RED_CASES])
def test_reductions(shape, off):
    from blurred_gan_amd import ops
    M, C = shape
    d = MC.red_inputs(M, C)
    ref = MC.red_ref(d, np.float64, "pairwise")
    x, dy, y = put(d["x"], off), put(d["dy"], off), put(d["y"], off)
    mean, inv, gamma, beta = put(d["mean"]), put(d["inv"]), put(d["gamma"]), put(d["beta"])
    ws = Guard(ops.colsum_workspace_bytes(M, C) // 4)
    ws.view.zero_()
    out = Guard(C, init=d["out0"])
    ops.colsum(x, out.view, M, C, ws.view, beta=MC.RED_BETA, scale=MC.RED_SCALE)
    eq(out.get(), ref["colsum"])
    out = Guard(C)
    ops.colsum(x, out.view, M, C, ws.view, square=True)
    eq(out.get(), ref["colsq"])
    sums = Guard(2 * C)
    ops.bn_stats(x, M, C, sums.view, ws.view)
    eq(sums.get(), ref["stats"])
    for yy in (y, None):
        sums = Guard(2 * C)
        ops.bn_bwd_stats(dy, yy, x, M, C, mean, inv, sums.view, ws.view, lrelu_alpha=MC.RED_ALPHA, gamma=gamma, beta=beta)
        eq(sums.get(), ref["bwd"])
    ws.get()


# ------------------------------------------------------------------ wave_sum_partials
PARTIAL_CASES = [(n, C) for n in MC.PARTIAL_NROWS for C in MC.PARTIAL_C]


@pytest.mark.parametrize("nrows,C", PARTIAL_CASES)
def test_partial_rows(nrows, C):
    from blurred_gan_amd import ops
    d = MC.partial_inputs(nrows, C)
    ref = MC.partial_ref(d, np.float64, "pairwise")
    partial = put(d["partial"])
    sums = Guard(2 * C)
    ops.bn_sums_from_partials(partial, nrows, C, sums.view)
    eq(sums.get(), ref["sums"])
    M = MC.PARTIAL_M
    x = put(np.random.default_rng(nrows + C).normal(size=(M, C)))
    y, sm, si = Guard(M * C), Guard(C), Guard(C)
    mm, mv = Guard(C, init=d["mm"]), Guard(C, init=np.ones(C))
    ops.bn_train_fwd_partials(partial, nrows, x, y.view, M, C, put(np.ones(C)), put(np.zeros(C)), mm.view, mv.view, sm.view, si.view,
                              momentum=MC.PARTIAL_MOMENTUM)
    eq(sm.get(), ref["save_mean"])
    eq(mm.get(), ref["moving_mean"])
    y.get(), si.get(), mv.get()


def _real_partials(nrows, C):
    rng = np.random.default_rng(9000 + 13 * nrows + C)
    M = max(64, 2 * nrows)
    x = (rng.normal(size=(M, C)) * 2 + 0.5).astype(np.float32)
    chunks = np.array_split(np.arange(M), nrows)
    partial = np.stack([np.stack([x[i].astype(np.float64).sum(0), (x[i].astype(np.float64) ** 2).sum(0)]) for i in chunks]).astype(np.float32)
    return M, x, partial, (1 + 0.3 * rng.normal(size=C)).astype(np.float32), (0.2 * rng.normal(size=C)).astype(np.float32), \
        rng.normal(size=C).astype(np.float32), (1 + rng.uniform(size=C)).astype(np.float32)


@pytest.mark.parametrize("nrows,C", PARTIAL_CASES)
def test_train_fwd_partials_real(nrows, C):
    from blurred_gan_amd import ops
    M, x, partial, gamma, beta, mm0, mv0 = _real_partials(nrows, C)
    refs = []
    for dt in (np.float64, np.float32):
        p = partial.astype(dt)
        refs.append(MC.bn_fwd_ref(np.concatenate([p[:, 0].sum(0, dtype=dt), p[:, 1].sum(0, dtype=dt)]), M, x, gamma, beta, mm0, mv0, dt))
    y, sm, si, mm, mv = Guard(M * C), Guard(C), Guard(C), Guard(C, init=mm0), Guard(C, init=mv0)
    ops.bn_train_fwd_partials(put(partial), nrows, put(x), y.view, M, C, put(gamma), put(beta), mm.view, mv.view, sm.view, si.view,
                              lrelu_alpha=MC.BN_REAL_ALPHA)
    for k, g in (("y", y), ("save_mean", sm), ("save_inv", si), ("moving_mean", mm), ("moving_var", mv)):
        report(f"train_fwd_partials.{k}", f"nrows={nrows} C={C}", g.get(), refs[0][k], refs[1][k], *MC.BN_BOUNDS[k])


def test_train_fwd_partials_in_place():
    """y is x, as the engine may call it: bit-identical to the out-of-place call."""
    from blurred_gan_amd import ops
    nrows, C = 449, 64
    M, x, partial, gamma, beta, mm0, mv0 = _real_partials(nrows, C)
    outs = []
    for in_place in (False, True):
        xg = Guard(M * C, init=x)
        y = xg if in_place else Guard(M * C)
        sm, si, mm, mv = Guard(C), Guard(C), Guard(C, init=mm0), Guard(C, init=mv0)
        ops.bn_train_fwd_partials(put(partial), nrows, xg.view, y.view, M, C, put(gamma), put(beta), mm.view, mv.view, sm.view, si.view)
        outs.append([g.get() for g in (y, sm, si, mm, mv)])
    for a, b in zip(*outs):
        eq(a, b)


# ------------------------------------------------------------------ BatchNorm apply family
def _params(d, names, p_off):
    """Per-channel parameters: separate aligned tensors, or slices at offsets 1, 2, 3 (mod 4) of ONE flat buffer."""
    if not p_off:
        return [put(d[n]) for n in names]
    C = d[names[0]].size
    flat = torch.zeros(len(names) * (C + 8) + 8, device="cuda")
    out, pos = [], 0
    for i, n in enumerate(names):
        pos += (1 + i % 3 - pos) % 4                       # start % 4 == 1, 2, 3, 1, ...
        flat[pos:pos + C].copy_(torch.from_numpy(d[n].astype(np.float32)))
        out.append(flat[pos:pos + C])
        assert out[-1].data_ptr() % 16 != 0
        pos += C
    return out


@pytest.mark.parametrize("case", MC.APPLY_CASES, ids=[f"{c[0]}x{c[1]}-x{c[2]}-p{c[3]}" for c in MC.APPLY_CASES])
def test_bn_apply_family(case):
    from blurred_gan_amd import ops
    M, C, x_off, p_off, m_totals, _, _ = case
    d = MC.apply_inputs(M, C)
    d["sums"] = np.concatenate([d["db"], d["dg"]])
    gamma, beta, mean, inv = _params(d, ["gamma", "beta", "mean", "inv"], p_off)
    sums = _params(d, ["sums"], p_off)[0] if p_off else put(d["sums"])
    x, dy = put(d["x"], x_off), put(d["dy"])
    y = Guard(M * C)
    ops.bn_apply(x, y.view, M, C, gamma, beta, mean, inv, lrelu_alpha=MC.APPLY_ALPHA)
    eq(y.get(), MC.apply_ref(d, np.float64)["y"])
    for Mt in m_totals:
        want = MC.apply_ref(d, np.float64, Mt)["dx"]
        for yy in (y.view, None):
            dx = Guard(M * C)
            ops.bn_bwd_apply(dy, yy, x, dx.view, M, Mt, C, gamma, mean, inv, sums, lrelu_alpha=MC.APPLY_ALPHA, beta=beta)
            eq(dx.get(), want)


@pytest.mark.parametrize("C", MC.PARAM_GRADS_C)
def test_bn_param_grads(C):
    from blurred_gan_amd import ops
    s = MC.ints(np.random.default_rng(C), (2 * C,), -99, 99)
    dg, db = Guard(C), Guard(C, off=1)
    ops.bn_param_grads(put(s), C, 0.5, dg.view, db.view)
    eq(db.get(), 0.5 * s[:C])
    eq(dg.get(), 0.5 * s[C:])


FIN_CASES = [(M, C, f) for (M, C) in ((64, 12), (100, 12), (50, 7), (4096, 64)) for f in (1, 2, 4)] + [(83000, 64, 1)]


@pytest.mark.parametrize("M,C,factor", FIN_CASES)
def test_bn_finalize_apply(M, C, factor):
    """bg_bn_finalize_apply_f32 == bg_bn_finalize_f32 + bg_bn_apply_f32 on the same sums, all five outputs bit for bit (the kernel's
    stated contract), with M_total = factor * M; and both within the real-valued bound of the float64 formula."""
    from blurred_gan_amd import ops
    rng = np.random.default_rng(M + C + factor)
    x = (rng.normal(size=(M, C)) * 2 + 0.5).astype(np.float32)
    gamma, beta = (1 + 0.3 * rng.normal(size=C)).astype(np.float32), (0.2 * rng.normal(size=C)).astype(np.float32)
    mm0, mv0 = rng.normal(size=C).astype(np.float32), (1 + rng.uniform(size=C)).astype(np.float32)
    x64 = x.astype(np.float64)
    s = (factor * np.concatenate([x64.sum(0), (x64 * x64).sum(0)])).astype(np.float32)     # `factor` replicas with the same rows
    Mt = factor * M
    sums, xd, g, b = put(s), put(x), put(gamma), put(beta)
    y1, sm1, si1, mm1, mv1 = Guard(M * C), Guard(C), Guard(C), Guard(C, init=mm0), Guard(C, init=mv0)
    ops.bn_finalize_apply(sums, Mt, xd, y1.view, M, C, g, b, sm1.view, si1.view, mm1.view, mv1.view, lrelu_alpha=MC.BN_REAL_ALPHA)
    y2, sm2, si2, mm2, mv2 = Guard(M * C), Guard(C), Guard(C), Guard(C, init=mm0), Guard(C, init=mv0)
    ops.bn_finalize(sums, Mt, C, sm2.view, si2.view, mm2.view, mv2.view)
    ops.bn_apply(xd, y2.view, M, C, g, b, sm2.view, si2.view, lrelu_alpha=MC.BN_REAL_ALPHA)
    refs = [MC.bn_fwd_ref(s, Mt, x, gamma, beta, mm0, mv0, dt) for dt in (np.float64, np.float32)]
    for k, a, c in (("y", y1, y2), ("save_mean", sm1, sm2), ("save_inv", si1, si2), ("moving_mean", mm1, mm2), ("moving_var", mv1, mv2)):
        got = a.get()
        eq(got, c.get())
        report(f"finalize_apply.{k}", f"M={M} C={C} M_total={Mt}", got, refs[0][k], refs[1][k], *MC.BN_BOUNDS[k])


# ------------------------------------------------------------------ Dense
def _gemm(M, N, K, tA, tB, route, full=True, a_off=0, b_off=0):
    from blurred_gan_amd import ops
    d = MC.gemm_inputs(M, N, K)
    A, Bm = put(d["A"].T if tA else d["A"], a_off), put(d["B"].T if tB else d["B"], b_off)
    Cg = Guard(M * N, init=d["C0"])
    kw = dict(bias=put(d["bias"]), beta=MC.GEMM_BETA) if full else {}
    names = launches(lambda: ops.gemm(A, Bm, Cg.view, M, N, K, tA, tB, scale=MC.GEMM_SCALE, **kw))
    assert names == [route], names
    eq(Cg.get(), MC.gemm_ref(d, np.float64, "pairwise", full))


@pytest.mark.parametrize("M,K,full", MC.GEMV_T_CASES)
def test_gemv_t(M, K, full):
    _gemm(M, 1, K, True, False, "dense_gemv_t", full)


@pytest.mark.parametrize("M,K,a_off,w_off,path,iters", MC.ROWDOT_CASES)
def test_rowdot(M, K, a_off, w_off, path, iters):
    _gemm(M, 1, K, False, False, "dense_rowdot", True, a_off, w_off)


@pytest.mark.parametrize("route,case", [("dense_gemm_tiled", c) for c in MC.TILED_CASES] + [("dense_gemm", c) for c in MC.NAIVE_CASES])
def test_gemm_tiled_and_naive(route, case):
    _gemm(*case, route)


# ------------------------------------------------------------------ pointwise and small kernels
@pytest.mark.parametrize("op", MC.POINT_OPS)
@pytest.mark.parametrize("total", sorted(MC.POINT_TOTALS))
def test_pointwise(total, op):
    from blurred_gan_amd import ops
    B, n_per = MC.POINT_TOTALS[total]
    d = MC.point_inputs(total)
    want = MC.point_ref(op, d, np.float64)
    r, f = put(d["r"]).view(B, n_per), put(d["f"]).view(B, n_per)
    out = Guard(total, init=d["r"] if op == "scale" else None)
    o = out.view.view(B, n_per)
    if op == "lerp":
        ops.lerp(r, f, put(d["a"]), o)
    elif op == "outer":
        ops.outer(put(d["s"]), put(d["w"]), o)
    elif op == "mul_grad":
        ops.mul_grad(r, f, o, alpha=MC.POINT_ALPHA)
    elif op == "mul_grad_keep":
        ops.mul_grad(r, f, o, keep=put(d["keep"], dtype=torch.uint8), alpha=MC.POINT_ALPHA, scale=MC.POINT_SCALE)
    elif op == "tanh_bwd":
        ops.tanh_bwd(f, put(d["y"]).view(B, n_per), o)
    elif op == "fill":
        ops.fill(out.view, -2.5)
    else:
        ops.scale_(out.view, 0.25)
    eq(out.get(), want)


@pytest.mark.parametrize("total", sorted(MC.POINT_TOTALS))
def test_gp_seed_real(total):
    from blurred_gan_amd import ops
    B, n_per = MC.POINT_TOTALS[total]
    rng = np.random.default_rng(total)
    g, n = rng.normal(size=(B, n_per)).astype(np.float32), (0.5 + rng.uniform(size=B)).astype(np.float32)
    refs = [np.asarray(dt(0.7) * ((n.astype(dt) - dt(1)) / n.astype(dt))[:, None] * g.astype(dt)) for dt in (np.float64, np.float32)]
    out = Guard(total)
    ops.gp_seed(put(g).view(B, n_per), put(n), 0.7, out.view.view(B, n_per))
    report("gp_seed", f"total={total}", out.get(), refs[0], refs[1], 1e-4, 1e-6)


@pytest.mark.parametrize("n,d_off,s_off", MC.COPY_CASES)
def test_copy(n, d_off, s_off):
    from blurred_gan_amd import ops
    src = (np.arange(n) % 8191 - 4000).astype(np.float64)
    dst = Guard(n, off=d_off)
    ops.copy_(dst.view, put(src, s_off))
    eq(dst.get(), src)


@pytest.mark.parametrize("n_per,off", MC.ROW_NORM_CASES)
def test_row_norm(n_per, off):
    from blurred_gan_amd import ops
    rows, ks = zip(*[MC.row_norm_inputs(n_per, b) for b in range(MC.ROW_NORM_B)])
    out = Guard(MC.ROW_NORM_B)
    ops.row_norm(put(np.stack(rows), off).view(MC.ROW_NORM_B, n_per), out.view)
    eq(out.get(), np.array(ks))
    g = np.random.default_rng(n_per).normal(size=(MC.ROW_NORM_B, n_per)).astype(np.float32)
    out = Guard(MC.ROW_NORM_B)
    ops.row_norm(put(g, off).view(MC.ROW_NORM_B, n_per), out.view)
    ref32 = np.sqrt((g * g).sum(1, dtype=np.float32))
    report("row_norm", f"n_per={n_per} off={off}", out.get(), np.linalg.norm(g.astype(np.float64), axis=1), ref32, 1e-5, 0.0)


@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("B", MC.LOSS_B)
def test_losses(B, with_norm):
    from blurred_gan_amd import ops
    d = MC.loss_inputs(B)
    ref = MC.loss_ref(d, np.float64, "pairwise", with_norm)
    ref32 = MC.loss_ref(d, np.float32, "sequential", with_norm)
    fs, rs = put(d["fs"]), put(d["rs"])
    dfs, drs, met = Guard(B), Guard(B, off=1), Guard(6)
    ops.wgangp_d_loss(fs, rs, put(d["norm"]) if with_norm else None, MC.LOSS["inv_gbs"], MC.LOSS["gp_coef"], MC.LOSS["e_drift"],
                      MC.LOSS["vec_scale"], dfs.view, drs.view, met.view)
    eq(dfs.get(), ref["dfs"])
    eq(drs.get(), ref["drs"])
    ds, gmet = Guard(B), Guard(2)
    ops.wgan_g_loss(fs, MC.LOSS["inv_gbs"], ds.view, gmet.view)
    eq(ds.get(), ref["ds"])
    if MC.is_pow2(B):                                    # the divisions by B are exact: every slot bit for bit
        eq(met.get(), ref["met"])
        eq(gmet.get(), ref["gmet"])
    else:                                                # exact sums, one rounding per division: the bound of test_pointwise_and_losses
        report("d_loss.metrics", f"B={B} norm={with_norm}", met.get(), ref["met"], ref32["met"], 1e-5, 1e-6)
        report("g_loss.metrics", f"B={B}", gmet.get(), ref["gmet"], ref32["gmet"], 1e-5, 1e-7)


@pytest.mark.parametrize("n", MC.ADAM_N)
def test_adam_real(n):
    from blurred_gan_amd import ops
    rng = np.random.default_rng(n)
    th0 = rng.normal(size=n).astype(np.float32)
    state = {dt: (th0.astype(dt), np.zeros(n, dt), np.zeros(n, dt)) for dt in (np.float64, np.float32)}
    th, m, v = Guard(n, init=th0), Guard(n, init=np.zeros(n)), Guard(n, off=1, init=np.zeros(n))
    for t in range(1, 4):
        g = (rng.normal(size=n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(np.float32)
        for dt in state:
            state[dt] = O.adam_update(*state[dt], g.astype(dt), t, 1e-3)
        ops.adam(th.view, m.view, v.view, put(g), 1e-3 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
    for k, gd, (rtol, atol) in (("theta", th, (1e-5, 1e-6)), ("m", m, (1e-5, 2e-7)), ("v", v, (3e-5, 1e-12))):   # test_adam_matches_oracle
        i = ("theta", "m", "v").index(k)
        report(f"adam.{k}", f"n={n}", gd.get(), state[np.float64][i], state[np.float32][i], rtol, atol)
