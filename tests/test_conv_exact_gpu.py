"""GPU: the 5x5 convolutions -- forward, data gradient, filter gradient -- on exact integer data, one case per route of the
dispatchers (tests/conv_cases.py; tests/test_conv_cases_cpu.py proves every case exact in float32 and on its claimed route on the CPU).

Every comparison is array_equal against the float64 oracle.  Inputs, outputs, the split-K scratch and the filter-gradient slabs are
16-byte-aligned views inside larger buffers whose guard bands hold a finite sentinel and must stay bit-unchanged; outputs and
workspaces start out as NaN, so an element that is never written shows; each workspace is exactly as long as
bg_conv2d_splitk_workspace_bytes / bg_conv2d_bwd_filter_workspace_bytes report; inputs must be bit-unchanged afterwards.  The launch
names recorded by the profiler must be the claimed route's; routes that share a name are told apart by the slab count of the
workspace query and, for the gather-GEMM, by the matrix-pipe flops the launch reports (they depend on the tile).  A failing decode
case names the (tap, ci, co) or the dy pixel its first wrong output came from.

The fallbacks behind the once-read switches that take a 5x5-only fast path away (conv_cases.SWITCHED_ENV) run in ONE fresh child
process started with them set (tests/conv_switched_child.py); no process that has initialised the GPU replaces its program.

The runner and the check_* bodies take the kernel size from the case shape (its optional seventh element, 5 without one):
tests/test_conv_ksize_exact_gpu.py imports them and runs the tables of tests/conv_ksize_cases.py at k = 3 and 1 through them.

Not here: tanh (inexact; tests/test_conv_gpu.py holds it to a tolerance) and the tuning
aids among the once-read switches (the rest of conv_cases.STATIC_SWITCHES).  The split-bf16 kernel (conv_math="bf16x6") has its own
exact file, tests/test_conv_x6_exact_gpu.py, which borrows the guarded buffers of this one."""
import numpy as np
import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu

PAD = 256                     # floats (bytes for the masks) of guard band on either side
SENTINEL = -98765.0
ROUTE_IDS = [CC.case_id(c[0]) for c in CC.ROUTE_CASES]
WGRAD_IDS = [CC.case_id(c[0]) for c in CC.WGRAD_CASES]
way_id = lambda t: ("dgrad-" if t[0] else "fwd-") + CC.case_id(t[1])


class Guarded:
    """n floats (or bytes) at a 16-byte boundary inside a buffer whose bands on either side hold a sentinel; NaN unless init is given."""

    def __init__(self, n, init=None, dtype=torch.float32):
        self.n, self.np_dtype = n, np.float32 if dtype == torch.float32 else np.uint8
        self.sent = SENTINEL if dtype == torch.float32 else 0xA5
        self.buf = torch.full((n + 2 * PAD,), self.sent, device="cuda", dtype=dtype)
        self.view = self.buf[PAD:PAD + n]
        assert self.view.data_ptr() % 16 == 0
        self.init = None
        if init is None:
            self.view.fill_(float("nan"))
        else:
            self.init = np.ascontiguousarray(init, dtype=self.np_dtype).ravel()
            self.view.copy_(torch.from_numpy(self.init))

    def guards_intact(self):
        b = self.buf.cpu().numpy().view(np.uint32 if self.np_dtype == np.float32 else np.uint8)
        s = np.array(self.sent, self.np_dtype).view(b.dtype)
        return bool((b[:PAD] == s).all() and (b[PAD + self.n:] == s).all())

    def unchanged(self):
        bits = np.uint32 if self.np_dtype == np.float32 else np.uint8
        return np.array_equal(self.view.cpu().numpy().view(bits), self.init.view(bits))

    def get(self, shape):
        return self.view.cpu().numpy().reshape(shape).astype(np.float64)

    def t(self, *shape):
        return self.view.view(*shape)


def check_buffers(inputs, outputs):
    assert all(g.guards_intact() for g in inputs + outputs if g is not None), "a guard band was written"
    assert all(g.unchanged() for g in inputs if g is not None), "an input was written"


def launches(fn):
    """-> [(name, matrix-pipe flops issued)] of the launches fn makes."""
    from blurred_gan_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [(r[0], r[4]) for r in ops.prof_records(with_exec=True)]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()


def run_route(bwd, shape, act, w, epi_kw=None, out_init=None, stats=None, profile=True, workspace=True):
    """bg_conv2d_fwd / bg_conv2d_bwd_data on guarded buffers -> (output as float64, route description); checks the workspace query,
    the launch names, the gather-GEMM's tile and slab count, the guard bands and the inputs."""
    from blurred_gan_amd import ops
    (B, H, W, Ci, Co, s), k = shape[:6], CC.ksize(shape)
    Ho, Wo = CC.cdiv(H, s), CC.cdiv(W, s)
    out_shape = (B, H, W, Ci) if bwd else (B, Ho, Wo, Co)
    d = CC.route(bwd, B, H, W, Ci, Co, s, k, stats=stats is not None, workspace=workspace)
    ga = Guarded(act.size, act)
    gw = Guarded(w.size, w if bwd else np.transpose(w, (0, 1, 3, 2)))
    go = Guarded(int(np.prod(out_shape)), out_init)
    nb = ops.conv2d_splitk_workspace_bytes(bwd, B, H, W, Ci, Co, k, s)
    assert nb == CC.splitk_workspace_bytes(bwd, B, H, W, Ci, Co, k, s)
    gs = Guarded(nb // 4) if nb and workspace else None
    kw = dict(epi_kw or {})
    held = {k: v for k, v in kw.items() if isinstance(v, Guarded)}
    kw.update({k: g.view for k, g in held.items()})
    if kw.pop("alias_ref", False):                                              # the reference activation IS the output buffer
        kw["ref"] = go.view
    epi = ops.epilogue(ws=gs.view if gs else None, stats=stats.view if stats else None, **kw) if (kw or gs or stats) else None
    a4 = ga.t(B, Ho, Wo, Co) if bwd else ga.t(B, H, W, Ci)
    fn = (lambda: ops.conv2d_bwd_data(a4, gw.view, go.t(*out_shape), k, s, epi)) if bwd else \
         (lambda: ops.conv2d_fwd(a4, gw.view, go.t(*out_shape), k, s, epi))
    if profile:
        rec = launches(fn)
        assert [r[0] for r in rec] == d["names"], ([r[0] for r in rec], d)
        if d["family"] == "conv_igemm":
            assert rec[0][1] == d["exec_flops"], (rec[0][1], d)                 # BM x BN tiles issued, padding taps skipped or not
            assert (nb // (4 * go.n) if gs else 1) == d["ks"]
    else:
        fn()
        torch.cuda.synchronize()
    check_buffers([ga, gw] + list(held.values()), [go, gs, stats])
    d["epi"] = epi
    return go.get(out_shape), d


def make_route(bwd, shape, recipe, seed=0):
    """-> (activation, w, float64 reference) of the forward (x) or the data gradient (dy) of a case shape."""
    act, w = (CC.make_dgrad if bwd else CC.make_fwd)(shape, recipe, seed)
    return act, w, (CC.ref_dgrad(act, w, shape[5], shape[1:3]) if bwd else CC.ref_fwd(act, w, shape[5]))


def check_route_exact(bwd, shape):
    """Both recipes of one direction of a case (k is the shape's seventh element, 5 without one), on its restated route."""
    for recipe in ("dense", "decode"):
        act, w, ref = make_route(bwd, shape, recipe)
        out, _ = run_route(bwd, shape, act, w)
        if not np.array_equal(out, ref):
            pytest.fail(f"{'data gradient' if bwd else 'forward'} {CC.case_id(shape)} [{recipe}]: "
                        f"{CC.describe_wrong(out, ref, shape[3], recipe, bwd, CC.ksize(shape))}")


@pytest.mark.parametrize("case", CC.ROUTE_CASES, ids=ROUTE_IDS)
def test_forward_exact_on_its_route(case):
    check_route_exact(0, case[0])


@pytest.mark.parametrize("case", CC.ROUTE_CASES, ids=ROUTE_IDS)
def test_data_gradient_exact_on_its_route(case):
    check_route_exact(1, case[0])


def run_wgrad(shape, x, dy, dw0=None, beta=0.0, scale=1.0, profile=True):
    from blurred_gan_amd import ops
    (B, H, W, Ci, Co, s), k = shape[:6], CC.ksize(shape)
    pl = CC.plan_wgrad(B, H, W, Ci, Co, s, k)
    nb = ops.conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, k, s)
    assert nb == pl["ws_bytes"], (nb, pl)                                       # the slab count pins the modes that share a name
    gx, gy, gd = Guarded(x.size, x), Guarded(dy.size, dy), Guarded(k * k * Ci * Co, dw0)
    gs = Guarded(nb // 4) if nb else None
    fn = lambda: ops.conv2d_bwd_filter(gx.t(*x.shape), gy.t(*dy.shape), gd.t(k, k, Ci, Co), k, s, beta, scale, gs.view if gs else None)
    if profile:
        names = [r[0] for r in launches(fn)]
        assert names == pl["names"], (names, pl)
    else:
        fn()
        torch.cuda.synchronize()
    check_buffers([gx, gy], [gd, gs])
    return gd.get((k, k, Ci, Co))


def check_filter_gradient_exact(shape):
    """beta = 0 into a NaN dw, then the accumulate form 0.5 dw0 + 2 grad on a dw of even integers (powers of two: exact)."""
    Ci, Co, k = shape[3], shape[4], CC.ksize(shape)
    dw0 = 2.0 * np.random.default_rng(5).integers(-4, 5, size=(k, k, Ci, Co))
    for recipe in ("dense", "decode"):
        x, dy, pix = CC.make_wgrad(shape, recipe)
        ref = CC.ref_wgrad(x, dy, shape[5], k)
        for form, (init, beta, scale, want) in {"beta=0": (None, 0.0, 1.0, ref), "accumulate": (dw0, 0.5, 2.0, 0.5 * dw0 + 2.0 * ref)}.items():
            dw = run_wgrad(shape, x, dy, init, beta, scale)
            if not np.array_equal(dw, want):
                back = dw if init is None else (dw - 0.5 * dw0) / 2.0
                detail = CC.decode_wgrad(back, ref, pix, shape) if recipe == "decode" else \
                    f"{int((dw != want).sum())} of {want.size} wrong, first at (kh, kw, ci, co)={np.argwhere(dw != want)[0].tolist()}"
                pytest.fail(f"filter gradient {CC.case_id(shape)} [{recipe}, {form}]: {int(np.isnan(dw).sum())} never written; {detail}")


@pytest.mark.parametrize("case", CC.WGRAD_CASES, ids=WGRAD_IDS)
def test_filter_gradient_exact_on_its_mode(case):
    check_filter_gradient_exact(case[0])


# ------------------------------------------------------------------------------------------------------------------------------------
# epilogues: everything but tanh is exact on this data (integer bias and multipliers, alpha = 1/4, dropout scale 2)
# ------------------------------------------------------------------------------------------------------------------------------------
def check_epilogues_exact(bwd, shape):
    from blurred_gan_amd._lib import EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_NONE, EPI_AFFINE_LRELU
    B, Ci, k = shape[0], shape[3], CC.ksize(shape)
    act, w, z = make_route(bwd, shape, "dense", seed=3)
    N = z.shape[-1]
    rng = np.random.default_rng([9, bwd, *shape])
    bias, mul = rng.integers(-5, 6, N).astype(np.float64), rng.integers(-3, 4, N).astype(np.float64)
    keep = (rng.uniform(size=z.shape) >= 0.5).astype(np.uint8)
    ref_act = rng.integers(-2, 3, z.shape).astype(np.float64)               # zeros included: the derivative at 0 is alpha
    nk = (B - 1) * z[0].size                                                # the mask covers all samples but the last
    assert 3 * np.abs(z).max() + 5 < CC.TWO24
    gb, gm = Guarded(N, bias), Guarded(N, mul)
    gk, gr = Guarded(keep.size, keep, torch.uint8), Guarded(z.size, ref_act)
    common = dict(alpha=0.25, scale=2.0)
    variants = {
        "bias": (dict(mode=EPI_NONE, bias=gb), None, CC.epilogue_ref(z, "none", bias)),
        "bias_lrelu": (dict(mode=EPI_BIAS_LRELU, bias=gb, **common), None, CC.epilogue_ref(z, "bias_lrelu", bias)),
        "bias_lrelu+dropout": (dict(mode=EPI_BIAS_LRELU, bias=gb, keep=gk, keep_elems=nk, **common), None,
                               CC.epilogue_ref(z, "bias_lrelu", bias, keep=keep, keep_elems=nk)),
        "mul_grad": (dict(mode=EPI_MUL_GRAD, ref=gr, **common), None, CC.epilogue_ref(z, "mul_grad", ref_act=ref_act)),
        "mul_grad+dropout": (dict(mode=EPI_MUL_GRAD, ref=gr, keep=gk, keep_elems=nk, **common), None,
                             CC.epilogue_ref(z, "mul_grad", ref_act=ref_act, keep=keep, keep_elems=nk)),
        "mul_grad+dropout, ref is the output": (dict(mode=EPI_MUL_GRAD, alias_ref=True, keep=gk, keep_elems=nk, **common), ref_act,
                                                CC.epilogue_ref(z, "mul_grad", ref_act=ref_act, keep=keep, keep_elems=nk)),
        "affine_lrelu": (dict(mode=EPI_AFFINE_LRELU, bias=gb, ref=gm, **common), None, CC.epilogue_ref(z, "affine_lrelu", bias, mul)),
    }
    for name, (kw, out_init, want) in variants.items():
        got, d = run_route(bwd, shape, act, w, epi_kw=kw, out_init=out_init)
        assert np.array_equal(got, want), f"{d['names'][0]} {CC.case_id(shape)} [{name}]: {CC.describe_wrong(got, want, Ci, 'dense', bwd, k)}"


@pytest.mark.parametrize("bwd,shape", CC.EPI_CASES, ids=[way_id(t) for t in CC.EPI_CASES])
def test_epilogues_exact(bwd, shape):
    check_epilogues_exact(bwd, shape)


def check_statistics_epilogue_exact(bwd, shape):
    """bg_epilogue.stats: the partial rows sum EXACTLY to the column sums and sums of squares of the stored tensor (impulse
    activations and weights in [-3, 3]: every output is one weight, so a partial row's sum of squares is far below 2^24); the rows
    past the reported count are never written, and the rows of a workgroup whose phases have no tap at all (one row per phase group
    and M tile, conv_igemm.hip:143) are exact zeros."""
    from blurred_gan_amd import ops
    (B, H, W, Ci, Co, s), k = shape[:6], CC.ksize(shape)
    act, _ = (CC.make_dgrad if bwd else CC.make_fwd)(shape, "decode", seed=4)
    _, w, _ = CC.dense(B, H, W, Ci, Co, s, "fwd", 4, k)
    ref = CC.ref_dgrad(act, w, s, (H, W)) if bwd else CC.ref_fwd(act, w, s)
    N = ref.shape[-1]
    assert np.abs(ref).max() <= 3 and ref.any()
    gst = Guarded((ref.size // N // 32 + 64) * 2 * N)
    out, d = run_route(bwd, shape, act, w, stats=gst, workspace=False)
    rows = ops.conv2d_stats_rows(d["epi"])
    assert rows == d["stats_rows"] > 0, (rows, d)
    assert np.array_equal(out, ref), CC.describe_wrong(out, ref, Ci, "dense", bwd, k)
    st = gst.get(-1)
    part = st[:rows * 2 * N].reshape(rows, 2, N)
    assert np.isfinite(part).all(), f"{int((~np.isfinite(part)).sum())} partial sums never written"
    assert np.isnan(st[rows * 2 * N:]).all(), "rows past the reported count were written"
    flat = ref.reshape(-1, N)
    assert np.array_equal(part[:, 0].sum(0), flat.sum(0)) and np.array_equal(part[:, 1].sum(0), (flat ** 2).sum(0))
    for grp in CC.tapless_groups(CC.gather_params(bwd, B, H, W, Ci, Co, k, s), d["pmerge"]):
        assert not part[grp * d["mtiles"]:(grp + 1) * d["mtiles"]].any(), f"phase group {grp} has no tap: its rows are not exact zeros"


@pytest.mark.parametrize("bwd,shape", CC.STATS_CASES, ids=[way_id(t) for t in CC.STATS_CASES])
def test_statistics_epilogue_exact(bwd, shape):
    check_statistics_epilogue_exact(bwd, shape)


# ------------------------------------------------------------------------------------------------------------------------------------
# isolation
# ------------------------------------------------------------------------------------------------------------------------------------
def check_a_nan_image_stays_inside_itself(bwd, shape):
    """One image of the batch is NaN throughout: every other image equals its reference."""
    B = shape[0]
    act, w, ref = make_route(bwd, shape, "dense", seed=6)
    k = B // 2
    act[k] = np.nan
    out, _ = run_route(bwd, shape, act, w, profile=False)
    for b in range(B):
        if b != k:
            assert np.array_equal(out[b], ref[b]), f"image {b} (the NaN image is {k}): {int((out[b] != ref[b]).sum())} of {ref[b].size} wrong"
    assert np.isnan(out[k]).any()


@pytest.mark.parametrize("bwd,shape", CC.ISOLATION_ROUTES, ids=[way_id(t) for t in CC.ISOLATION_ROUTES])
def test_a_nan_image_stays_inside_itself(bwd, shape):
    check_a_nan_image_stays_inside_itself(bwd, shape)


def check_two_runs_are_bit_identical(bwd, shape):
    """No route of the forward / data gradient has atomics: two runs into different buffers agree bit for bit (and are right)."""
    act, w, ref = make_route(bwd, shape, "dense", seed=7)
    a, _ = run_route(bwd, shape, act, w, profile=False)
    b, _ = run_route(bwd, shape, act, w, profile=False)
    assert np.array_equal(a, b) and np.array_equal(a, ref)


@pytest.mark.parametrize("bwd,shape", CC.ISOLATION_ROUTES, ids=[way_id(t) for t in CC.ISOLATION_ROUTES])
def test_two_runs_are_bit_identical(bwd, shape):
    check_two_runs_are_bit_identical(bwd, shape)


def check_two_filter_gradient_runs_are_bit_identical(shape):
    """The filter gradients reduce through slabs, not atomics: two runs into different buffers agree bit for bit."""
    x, dy, _ = CC.make_wgrad(shape, "dense", seed=8)
    a = run_wgrad(shape, x, dy, profile=False)
    b = run_wgrad(shape, x, dy, profile=False)
    assert np.array_equal(a, b) and np.array_equal(a, CC.ref_wgrad(x, dy, shape[5], CC.ksize(shape)))


@pytest.mark.parametrize("shape", CC.ISOLATION_WGRAD, ids=[CC.case_id(c) for c in CC.ISOLATION_WGRAD])
def test_two_filter_gradient_runs_are_bit_identical(shape):
    check_two_filter_gradient_runs_are_bit_identical(shape)


def test_fallbacks_behind_the_once_read_switches_in_a_fresh_process():
    """The c16 and row-kernel shapes on the gather-GEMM and the thin kernels, the c16 / strip / row-MFMA / tap-grouped filter-gradient
    shapes on the generic modes (modes 4 and 5 at M >= 131072 included): exact, on their restated routes, in a child process started
    with conv_cases.SWITCHED_ENV -- the library reads those switches once per process."""
    assert not CC.OFF
    print(CC.run_switched_child("gpu"))
