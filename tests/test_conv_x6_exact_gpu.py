"""GPU: the split-bf16 gather-GEMM (csrc/conv_igemm_x6.hip, conv_math="bf16x6") held to fp32 precision piece by piece
(tests/x6_cases.py; tests/test_x6_cases_cpu.py proves the recipes and the mutant table on the CPU).

The kernel's other tests (test_conv_math_gpu.py, test_step_math_gpu.py) use conv_tol, about 1e-4 of the output scale: a kernel that
drops its three second-order terms, reads a wrong piece plane in one MFMA or forms `lo` from the wrong remainder passes them with a
tenfold margin.  Here every route case runs three recipes -- "pieces" (each output ONE product whose six cross terms sit in separate
digits of one float32 number; the expectation is RNE(float64 product)), and the integer recipes "dense" and "decode" of
conv_cases.py -- and every comparison is array_equal where the float64 reference is nonzero and the lifted-zero bound
5 K 2^-126 max(max|a|, max|w|) where it is zero.  The integer recipes get one unit in the last place of the matrix pipe's adder on
top (x6_cases.adder_unit, 2^-23 max|a| max|w|: v_mfma_f32_32x32x16_bf16 floors a NEGATIVE lifted residue in its accumulator against
large products instead of dropping it -- tools/probes/mfma_tiny_accumulator.hip; MI355X: 52 of the dense outputs of the route cases
are 2^-22 below their integer, no "pieces" and no decode output differs); an integer output that is wrong is wrong by 1.  Buffers are the guarded ones of test_conv_exact_gpu.py (guard bands bit-unchanged,
outputs start as NaN, inputs unchanged) and the recorded launch name must be conv_igemm_x6_fwd / conv_igemm_x6_dgrad -- or absent
for the 16-position geometries the kernel must not take.

BG_CONV_X6_FORCE is read once per process, so everything off the dispatch table runs in ONE fresh child started with it
(tests/x6_forced_child.py: route cases, epilogues with AFFINE_LRELU, the statistics epilogue, the precision leg on real-valued
data against the fp32 kernels and the one-term mutants, scaling invariance); the two table geometries run here, unforced, at B = 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_cases as CC
import x6_cases as X
from test_conv_exact_gpu import Guarded, check_buffers, launches

pytestmark = pytest.mark.gpu


def run_x6(bwd, shape, k, act, w, math="bf16x6", expect=True, epi_kw=None, out_init=None, stats=None):
    """bg_conv2d_fwd_math / bg_conv2d_bwd_data_math on guarded buffers -> (output as float64, the epilogue).  With math "bf16x6" the
    recorded launches must be exactly the x6 kernel of the direction (expect) or hold no x6 launch at all (not expect)."""
    from blurred_gan_amd import ops
    s = shape[5]
    oshape = X.out_shape(bwd, shape)
    ga = Guarded(act.size, act)
    gw = Guarded(w.size, w if bwd else np.transpose(w, (0, 1, 3, 2)))
    go = Guarded(int(np.prod(oshape)), out_init)
    kw = dict(epi_kw or {})
    held = {n: v for n, v in kw.items() if isinstance(v, Guarded)}
    kw.update({n: g.view for n, g in held.items()})
    if kw.pop("alias_ref", False):                                              # the reference activation IS the output buffer
        kw["ref"] = go.view
    epi = ops.epilogue(stats=stats.view if stats else None, **kw) if (kw or stats) else None
    a4 = ga.t(*act.shape)
    fn = (lambda: ops.conv2d_bwd_data(a4, gw.view, go.t(*oshape), k, s, epi, math=math)) if bwd else \
         (lambda: ops.conv2d_fwd(a4, gw.view, go.t(*oshape), k, s, epi, math=math))
    names = [r[0] for r in launches(fn)]
    if math == "bf16x6" and expect:
        assert names == [X.launch(bwd, shape, k)["name"]], names
    else:
        assert names and not [n for n in names if "x6" in n], names
    check_buffers([ga, gw] + list(held.values()), [go, stats])
    return go.get(oshape), epi


INEXACT = {}          # recipe -> outputs with a nonzero reference that were not bit-equal to it (the adder's unit, x6_cases.adder_unit)


def check_case(bwd, shape, k, expect=True):
    """The three recipes of one geometry, exact as x6_cases.compare defines it."""
    assert X.x6_can_run(bwd, *shape[:5], k, shape[5]) == expect
    K = CC.gather_params(bwd, *shape[:5], k, shape[5])["Ck"] * k * k
    for recipe in X.RECIPES:
        act, w = X.make(bwd, shape, k, recipe, cover=expect)
        ref = X.expected(bwd, shape, act, w)
        got, _ = run_x6(bwd, shape, k, act, w, expect=expect)
        res = X.compare(got, ref, K, np.abs(act).max(), np.abs(w).max(), adder=recipe != "pieces")
        INEXACT[recipe] = INEXACT.get(recipe, 0) + int(((ref != 0) & (got != ref)).sum())
        assert res is None, f"{X.case_id((bwd, shape, k))} [{recipe}]: {X.describe_wrong(bwd, shape, k, recipe, act, w, got, ref, res)}"


def check_epilogues(bwd, shape, k):
    """Every exact epilogue on the dense integers, with the settings of conv_cases.epilogue_ref: integer bias, LeakyReLU alpha 1/4,
    dropout scale 2 with keep_elems short of the last sample, MUL_GRAD plain and with ref aliasing the output, AFFINE_LRELU."""
    from blurred_gan_amd._lib import EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_NONE, EPI_AFFINE_LRELU
    act, w = X.make(bwd, shape, k, "dense", seed=3)
    z = X.conv(bwd, shape, act, w)
    d = X.epilogue_data(bwd, shape, k, z)
    bias, mul, keep, ref_act, nk = d["bias"], d["mul"], d["keep"], d["ref_act"], d["keep_elems"]
    assert 3 * np.abs(z).max() + 5 < CC.TWO24 and nk % 4 == 0 and 0 < nk < z.size
    gb, gm = Guarded(z.shape[-1], bias), Guarded(z.shape[-1], mul)
    gk, gr = Guarded(keep.size, keep, torch.uint8), Guarded(z.size, ref_act)
    common = dict(alpha=0.25, scale=2.0)
    E = CC.epilogue_ref
    variants = {
        "bias": (dict(mode=EPI_NONE, bias=gb), None, E(z, "none", bias)),
        "bias_lrelu": (dict(mode=EPI_BIAS_LRELU, bias=gb, **common), None, E(z, "bias_lrelu", bias)),
        "bias_lrelu+dropout": (dict(mode=EPI_BIAS_LRELU, bias=gb, keep=gk, keep_elems=nk, **common), None,
                               E(z, "bias_lrelu", bias, keep=keep, keep_elems=nk)),
        "mul_grad": (dict(mode=EPI_MUL_GRAD, ref=gr, **common), None, E(z, "mul_grad", ref_act=ref_act)),
        "mul_grad+dropout": (dict(mode=EPI_MUL_GRAD, ref=gr, keep=gk, keep_elems=nk, **common), None,
                             E(z, "mul_grad", ref_act=ref_act, keep=keep, keep_elems=nk)),
        "mul_grad+dropout, ref is the output": (dict(mode=EPI_MUL_GRAD, alias_ref=True, keep=gk, keep_elems=nk, **common), ref_act,
                                                E(z, "mul_grad", ref_act=ref_act, keep=keep, keep_elems=nk)),
        "affine_lrelu": (dict(mode=EPI_AFFINE_LRELU, bias=gb, ref=gm, **common), None, E(z, "affine_lrelu", bias, mul)),
    }
    K = X.launch(bwd, shape, k)["K"]
    for name, (kw, out_init, want) in variants.items():
        got, _ = run_x6(bwd, shape, k, act, w, epi_kw=kw, out_init=out_init)
        res = X.compare(got, want, K, np.abs(act).max(), np.abs(w).max(), factor=3.0, adder=True)
        assert res is None, f"{X.case_id((bwd, shape, k))} [{name}]: {X.describe_wrong(bwd, shape, k, 'dense', act, w, got, want, res)}"


def check_statistics(bwd, shape, k):
    """bg_epilogue.stats on impulse activations and weights in [-3, 3] (every output one weight or a lifted zero): the partial rows
    sum to the column sums and sums of squares of the stored tensor up to M lifted zeros, the rows of the empty tiles of a smaller
    phase are exact zeros, the rows past the reported count stay unwritten."""
    from blurred_gan_amd import ops
    act, _ = X.make(bwd, shape, k, "decode", seed=4)
    w = CC.dense(*shape, "fwd", 4, k)[1]
    ref = X.expected(bwd, shape, act, w)
    d = X.launch(bwd, shape, k)
    N, rows, mt = d["N"], d["stats_rows"], d["mtiles"]
    assert np.abs(ref).max() <= 3 and ref.any()
    gst = Guarded((rows + 3) * 2 * N)
    out, epi = run_x6(bwd, shape, k, act, w, stats=gst)
    assert ops.conv2d_stats_rows(epi) == rows, (ops.conv2d_stats_rows(epi), rows)
    bound = X.lifted_zero_bound(d["K"], 1.0, 3.0) + X.adder_unit(1.0, 3.0)
    res = X.compare(out, ref, d["K"], 1.0, 3.0, adder=True)
    assert res is None, X.describe_wrong(bwd, shape, k, "dense", act, w, out, ref, res)
    st = gst.get(-1)
    part = st[:rows * 2 * N].reshape(d["nphase"], mt, 2, N)
    assert np.isfinite(part).all(), f"{int((~np.isfinite(part)).sum())} partial sums never written"
    assert np.isnan(st[rows * 2 * N:]).all(), "rows past the reported count were written"
    for ph, m in enumerate(d["M"]):
        assert not part[ph, CC.cdiv(m, X.K_BM):].any(), f"phase {ph}: the rows of its empty tiles are not exact zeros"
    flat = ref.reshape(-1, N)
    tol = flat.shape[0] * bound * 7                      # ... squared: (r + e)^2 - r^2 <= (2 x 3 + 1) e
    assert np.abs(part[:, :, 0].sum((0, 1)) - flat.sum(0)).max() <= tol and np.abs(part[:, :, 1].sum((0, 1)) - (flat ** 2).sum(0)).max() <= tol


def rel_l2(y, ref):
    return float(np.linalg.norm(y - ref) / np.linalg.norm(ref))


def check_precision(bwd, shape, k):
    """uniform(-1, 1) operands: e6 <= 3 e32 (the fp32 kernels on the same inputs: independent code; 3 allows for two fp32
    summation orders of the same K products and the omitted terms below 2^-24), and e_mu >= 4 (3 e32) for the closest mutant of the
    six-term sum (float64 accumulation of the split3 pieces) -- otherwise the bound would not catch it."""
    act, w = X.real_data(bwd, shape, k)
    ref = X.conv(bwd, shape, act, w)
    y6, _ = run_x6(bwd, shape, k, act, w)
    y32, _ = run_x6(bwd, shape, k, act, w, math="fp32")
    P = X.piece_convs(bwd, shape, act, w)
    e6, e32, ekept = rel_l2(y6, ref), rel_l2(y32, ref), rel_l2(X.combine(P, X.kept_coef()), ref)
    emu, who = min((rel_l2(X.combine(P, c), ref), n) for n, c in X.mutants().items())
    print(f"[x6 precision] {X.case_id((bwd, shape, k))} K={X.launch(bwd, shape, k)['K']}: e6 {e6:.3e} / e32 {e32:.3e} / e_mu {emu:.3e} ({who}); "
          f"six terms in float64 {ekept:.3e}", flush=True)
    assert 0 < e32 < 1e-6 and ekept < 1e-7
    assert emu >= 4 * (3 * e32), f"not discriminating: the closest mutant ({who}) is at {emu:.3e}, inside 12 e32 = {12 * e32:.3e}"
    assert e6 <= 3 * e32, f"x6 is at {e6:.3e} of the float64 oracle, the fp32 kernel at {e32:.3e}"


def check_scaling(bwd, shape, k):
    """y(2^10 a, 2^-7 w) = 2^3 y(a, w) bit for bit: the split does not depend on the exponent."""
    act, w = X.real_data(bwd, shape, k, seed=1)
    y, _ = run_x6(bwd, shape, k, act, w)
    ys, _ = run_x6(bwd, shape, k, act * 1024.0, w / 128.0)
    assert np.isfinite(y).all() and np.array_equal(ys, 8.0 * y), f"{int((ys != 8.0 * y).sum())} of {y.size} outputs differ"


@pytest.mark.parametrize("case", X.TABLE_CASES, ids=[X.case_id(c) for c in X.TABLE_CASES])
def test_table_geometries_exact_without_the_force(case):
    assert "BG_CONV_X6_FORCE" not in os.environ
    bwd, shape, k = case
    assert X.in_table(bwd, *shape[1:5], k, shape[5])
    check_case(bwd, shape, k)


def test_forced_cases_in_one_fresh_process():
    """x6_cases.ROUTE_CASES, MUST_NOT_RUN, EPI_CASES, STATS_CASES, PRECISION_CASES and SCALING_CASES in a child started with
    BG_CONV_X6_FORCE=1 (the library reads it once per process); the child stops at its first failure and its output is shown."""
    assert "BG_CONV_X6_FORCE" not in os.environ
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "x6_forced_child.py")
    r = subprocess.run([sys.executable, script], env={**os.environ, "BG_CONV_X6_FORCE": "1"}, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("[x6 precision]") == len(X.PRECISION_CASES)
