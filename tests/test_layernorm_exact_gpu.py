"""GPU: the layer normalisation kernels (csrc/layernorm.hip) on the case table of tests/ln_cases.py, whose data makes every output
exact in float32 in any summation order (tests/test_ln_cases_cpu.py proves it per case), so every comparison is ``array_equal``
against float64 and a dropped term, a neighbour's statistic or a missing partial row cannot hide in a tolerance.

Every operand, output and workspace is a ``helpers.Guarded`` view: guard bands of a finite sentinel on both sides, outputs NaN (mu, r,
u_out, dgamma / dbeta at acc_beta = 0 among them), the workspace exactly bg_ln_workspace_bytes long and NaN.  After every call the
guard bands and the inputs must hold their bits, the launch names must be the claimed list, and the partial rows the launch owns must
all have been written.  Each kernel runs alone: backward, tangent and source take mu and r from the reference, not from the forward
(the hard inputs alone chain them, as a step does).

Hard inputs (4096 + N(0, 1), 1e4 * N(0, 1), a single 1e4 spike) are bounded, not exact: per output max(the bound of
tests/test_layernorm_gpu.py, 3 x the deviation of a float32 numpy two-pass evaluation from float64), from the reference alone."""
import ctypes

import numpy as np
import pytest
import torch

from blurred_gan_amd import _lib, ops
from helpers import Guarded
import ln_cases as LC

pytestmark = pytest.mark.gpu

ln = ops.layernorm
U8 = torch.uint8


# ------------------------------------------------------------------ harness
class Pool:
    """The guarded buffers of one test; ``check`` holds every guard band, every input and the launch list."""

    def __init__(self, case):
        self.case, self.R, self.C, self.off, self.all = case, case["R"], case["C"], case.get("offset", 0), []
        self.nan_rows = False                   # a test that feeds a NaN row: the partial rows may hold NaN

    def new(self, n, init=None, dtype=torch.float32):
        g = Guarded(n, init, dtype, offset=self.off)
        self.all.append(g)
        return g

    def rc(self, init=None):
        return self.new(self.R * self.C, init)

    def ws(self):
        n = ln.workspace_bytes(self.R, self.C)
        assert n == LC.workspace_bytes(self.R, self.C) and n % 4 == 0
        return self.new(n // 4)

    def run(self, what, names, fn, written=()):
        torch.cuda.synchronize()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            fn()
            torch.cuda.synchronize()
            got = [r[0] for r in ops.prof_records()]
        finally:
            ops.prof_enable(False)
            ops.prof_reset()
        assert got == names, (what, got)
        for i, g in enumerate(self.all):
            assert g.guards_intact(), f"{what}: buffer {i} ({g.n} elements): guard band written"
            if g.init is not None and not any(g is w for w in written):
                assert g.unchanged(), f"{what}: input buffer {i} ({g.n} elements) changed"
        for w in written:                       # what a later call of the same pool must find unchanged
            if w.init is not None:
                w.init = w.get().copy()


def same(got, want, case, what):
    """array_equal against float64; a failure names the first wrong element and where the route keeps it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    at = tuple(int(x) for x in bad[0])
    where = LC.position(case["C"], at[0], at[1]) if len(at) == 2 else {}
    raise AssertionError(f"{LC.case_id(case)} {what}: {len(bad)} of {got.size} differ, first at {at} {where}: got {got[at]!r}, want {want[at]!r} "
                         f"(route {LC.route_for(case['C'])})")


def partial_rows_written(ws, p, nq, what):
    """The launch owns grid.x * nq partial rows at the front of the workspace: all written; what lies behind stays NaN."""
    n = LC.grid_for(p.R, p.C)[0] * nq * p.C
    w = ws.get()
    assert p.nan_rows or not np.isnan(w[:n]).any(), f"{what}: {int(np.isnan(w[:n]).sum())} floats of the {n} partial-row floats never written"
    assert np.isnan(w[n:]).all(), f"{what}: written behind the partial rows"


def keep_args(p, d, rows):
    if not rows:
        return {}
    k = p.new(rows * p.C, d["keep"][:rows], U8)
    return dict(keep=k.view, scale=LC.KEEP_SCALE, keep_elems=0 if rows == p.R else rows * p.C)


def chunked(case):
    return LC.route_for(case["C"])["chunks"] > 1


def run_fwd(p, d, alpha, rows, z=None):
    R, C = p.R, p.C
    z = z or p.rc(d["z"])
    a, mu, r = p.rc(), p.new(R), p.new(R)
    gamma, beta = p.new(C, d["gamma"]), p.new(C, d["beta"])
    kw = keep_args(p, d, rows)
    p.run("fwd", ["ln_fwd"], lambda: ln.fwd(z.view, a.view, R, C, gamma.view, beta.view, mu.view, r.view, eps=d["eps"], lrelu_alpha=alpha, **kw))
    return dict(a=a.get(R, C), mu=mu.get(), r=r.get())


def run_bwd(p, d, e, alpha, rows, addend=False, dw=0, acc_beta=0.0, acc_scale=1.0, sums=False, inplace=None, window=None, g=None, z=None, stats=None):
    R, C = p.R, p.C
    g, z = g or p.rc(d["g"]), z or p.rc(d["z"])
    mu, r = stats or (p.new(R, e.mu), p.new(R, e.r))
    gamma, beta = p.new(C, d["gamma"]), p.new(C, d["beta"])
    ad = p.rc(d["addend"]) if addend else None
    dz = g if inplace == "g" else ad if inplace == "addend" else p.rc()
    kw = keep_args(p, d, rows)
    out = {}
    if sums:
        lo, hi = window
        uo, ws = p.new((hi - lo) * C), p.ws()
        dg, db = (p.new(C, None if not acc_beta else d["old"][k]) for k in (0, 1))
        kw.update(u_out=uo.view, u_rows=(lo, hi), dgamma=dg.view, dbeta=db.view, dw_rows=dw, acc_beta=acc_beta, acc_scale=acc_scale, ws=ws.view)
    p.run("bwd", ["ln_bwd"] + (["ln_finish"] if sums else []),
          lambda: ln.bwd(g.view, z.view, dz.view, R, C, gamma.view, beta.view, mu.view, r.view, lrelu_alpha=alpha,
                         addend=None if ad is None else ad.view, **kw), written=[dz] + ([dg, db] if sums else []))
    out["dz"] = dz.get(R, C)
    if sums:
        partial_rows_written(ws, p, 2, "bwd")
        out.update(u=uo.get(hi - lo, C), dgamma=dg.get(), dbeta=db.get())
    return out


def run_tangent(p, d, e, alpha, inplace=False, zdot=None, z=None, stats=None):
    R, C = p.R, p.C
    zdot, z = zdot or p.rc(d["zdot"]), z or p.rc(d["z"])
    mu, r = stats or (p.new(R, e.mu), p.new(R, e.r))
    gamma, beta = p.new(C, d["gamma"]), p.new(C, d["beta"])
    v = zdot if inplace else p.rc()
    p.run("tangent", ["ln_tangent"], lambda: ln.tangent(zdot.view, z.view, v.view, R, C, gamma.view, beta.view, mu.view, r.view, lrelu_alpha=alpha),
          written=[v])
    return dict(v=v.get(R, C))


def run_source(p, d, e, u, acc_beta, acc_scale, zdot=None, z=None, stats=None):
    R, C = p.R, p.C
    u, zdot, z = p.rc(u), zdot or p.rc(d["zdot"]), z or p.rc(d["z"])
    mu, r = stats or (p.new(R, e.mu), p.new(R, e.r))
    gamma = p.new(C, d["gamma"])
    s, ws, dg = p.rc(), p.ws(), p.new(C, None if not acc_beta else d["old"][0])
    p.run("source", ["ln_gp_source", "ln_finish"],
          lambda: ln.gp_source(u.view, zdot.view, z.view, s.view, R, C, gamma.view, mu.view, r.view, dg.view, ws.view, acc_beta=acc_beta,
                               acc_scale=acc_scale), written=[dg])
    partial_rows_written(ws, p, 1, "source")
    return dict(s=s.get(R, C), dgamma=dg.get())


def _variants(case, op):
    return [(name, args) for name, o, args in LC.variants(case) if o == op]


def _cases(op):
    return [pytest.param(i, id=LC.IDS[i]) for i, c in enumerate(LC.CASES) if op in c["ops"]]


# ------------------------------------------------------------------ the case table, kernel by kernel
@pytest.mark.parametrize("i", _cases("fwd"))
def test_forward_is_exact(i):
    case = LC.CASES[i]
    d, e = LC.reference(i)
    for name, (alpha, rows) in _variants(case, "fwd"):
        got, want = run_fwd(Pool(case), d, alpha, rows), e.fwd(alpha, rows)
        for k in ("mu", "r", "a"):
            same(got[k], want[k], case, f"{name}: {k}")


@pytest.mark.parametrize("i", _cases("bwd"))
def test_backward_is_exact(i):
    case = LC.CASES[i]
    d, e = LC.reference(i)
    lo, hi = case["u_lo"], case["u_hi"]
    for name, args in _variants(case, "bwd"):
        want = e.bwd(*args)
        if name == "bwd no sums":                    # the generator step's form, in place over g where the row stays in registers
            got = run_bwd(Pool(case), d, e, args[0], args[1], inplace=None if chunked(case) else "g")
        elif name == "bwd dz over addend":
            got = run_bwd(Pool(case), d, e, args[0], args[1], addend=True, inplace=None if chunked(case) else "addend")
        else:
            alpha, rows, _, dw, acc_beta, acc_scale = args
            got = run_bwd(Pool(case), d, e, alpha, rows, addend=True, dw=dw, acc_beta=acc_beta, acc_scale=acc_scale, sums=True, window=(lo, hi))
            same(got["u"], want["u"][lo:hi], case, f"{name}: u rows [{lo}, {hi})")
            same(got["dgamma"], want["dgamma"], case, f"{name}: dgamma")
            same(got["dbeta"], want["dbeta"], case, f"{name}: dbeta")
        same(got["dz"], want["dz"], case, f"{name}: dz")


@pytest.mark.parametrize("i", _cases("tangent"))
def test_tangent_is_exact(i):
    case = LC.CASES[i]
    d, e = LC.reference(i)
    for name, (alpha,) in _variants(case, "tangent"):
        got = run_tangent(Pool(case), d, e, alpha, inplace=name.endswith("in place") and not chunked(case))
        same(got["v"], e.tangent(alpha)["v"], case, name)


@pytest.mark.parametrize("i", _cases("source"))
def test_source_is_exact(i):
    case = LC.CASES[i]
    d, e = LC.reference(i)
    for name, (alpha, acc_beta, acc_scale) in _variants(case, "source"):
        want = e.source(alpha, acc_beta, acc_scale)
        got = run_source(Pool(case), d, e, want["u"], acc_beta, acc_scale)
        same(got["s"], want["s"], case, f"{name}: s")
        same(got["dgamma"], want["dgamma"], case, f"{name}: dgamma")


# ------------------------------------------------------------------ one case per route class: a NaN row, two runs
def _class_case(C):
    """The table's case of this C with the most rows short of the grid-stride ones."""
    own = [i for i, c in enumerate(LC.CASES) if c["C"] == C and c["kind"] == "exact" and c["cells"][0][0] == "C"]
    return max(own, key=lambda i: LC.CASES[i]["R"])


def _rows_but(got, want, row, case, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isnan(got[row]).all(), f"{LC.case_id(case)} {what}: the NaN row came out finite: {np.ravel(got[row])[:8]}"
    keep = np.arange(case["R"]) != row
    same(got[keep], want[keep], case, f"{what}: the rows beside the NaN row {row}")


@pytest.mark.parametrize("C", LC.CLASS_C)
@pytest.mark.parametrize("which", ["z", "g", "zdot"])
def test_a_nan_row_stays_in_its_row(C, which):
    """A row's outputs depend on that row alone: a shuffle tree that left its lane group would carry the NaN to a neighbour.  The
    column sums take the NaN and are not asserted."""
    i = _class_case(C)
    case = LC.CASES[i]
    d, e = LC.reference(i)
    R, row = case["R"], min(case["R"] // 2 + 1, case["R"] - 1)
    assert R >= 3
    bad = dict(d, **{which: d[which].copy()})
    bad[which][row] = np.nan
    mu, r = e.mu.copy(), e.r.copy()

    def pool():
        p = Pool(case)
        p.nan_rows = True
        return p
    if which == "z":
        mu[row] = r[row] = np.nan
        got = run_fwd(pool(), bad, LC.ALPHA, 0)
        want = e.fwd(LC.ALPHA, 0)
        for k in ("mu", "r", "a"):
            _rows_but(got[k], want[k], row, case, f"fwd {k}")
    stats = lambda p: (p.new(R, mu), p.new(R, r))
    if which in ("z", "g"):
        p = pool()
        got = run_bwd(p, bad, e, LC.ALPHA, 0, addend=True, dw=case["dw_rows"], sums=True, window=(case["u_lo"], case["u_hi"]), stats=stats(p))
        _rows_but(got["dz"], e.bwd(LC.ALPHA, 0, True)["dz"], row, case, "bwd dz")
    if which in ("z", "zdot"):
        p = pool()
        _rows_but(run_tangent(p, bad, e, LC.ALPHA, stats=stats(p))["v"], e.tangent(LC.ALPHA)["v"], row, case, "tangent")
    want = e.source(LC.ALPHA)
    u = want["u"].copy()
    if which == "g":
        u[row] = np.nan
    p = pool()
    _rows_but(run_source(p, bad, e, u, 0.0, 1.0, stats=stats(p))["s"], want["s"], row, case, "source s")


@pytest.mark.parametrize("C", LC.CLASS_C)
def test_two_runs_into_different_buffers_give_the_same_bits(C):
    i = _class_case(C)
    case = LC.CASES[i]
    d, e = LC.reference(i)
    u = e.source(LC.ALPHA)["u"]
    runs = []
    for _ in range(2):
        out = {f"fwd {k}": v for k, v in run_fwd(Pool(case), d, LC.ALPHA, case["keep_rows"]).items()}
        out.update({f"bwd {k}": v for k, v in run_bwd(Pool(case), d, e, LC.ALPHA, case["keep_rows"], addend=True, dw=case["dw_rows"], acc_beta=1.0,
                                                      acc_scale=0.5, sums=True, window=(case["u_lo"], case["u_hi"])).items()})
        out.update({f"source {k}": v for k, v in run_source(Pool(case), d, e, u, 1.0, 1.0).items()})
        out["tangent"] = run_tangent(Pool(case), d, e, LC.ALPHA)["v"]
        runs.append(out)
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), (LC.case_id(case), k)


# ------------------------------------------------------------------ hard inputs under a bound measured from the reference
@pytest.mark.parametrize("case", LC.HARD_CASES, ids=[f"C{c['C']}" for c in LC.HARD_CASES])
def test_hard_inputs_stay_under_the_reference_bound(case):
    ref = LC.hard_reference(case)
    d, e, R, C = ref["data"], ref["eval"], case["R"], case["C"]
    pc = dict(case, offset=0)
    failed = []

    def held(run, got):
        for k, v in got.items():
            want, bound = ref["out"][f"{run} {k}"][:2]
            err = np.abs(np.asarray(v, np.float64).reshape(want.shape) - want)
            worst = float(np.nanmax(np.where(np.isnan(err), np.inf, err) / bound))
            print(f"[ln parity] {run} {k} C={C} R={R}: max error / bound {worst:.3f} (max error {float(np.nanmax(err)):.2e})")
            if not worst <= 1.0:
                failed.append((run, k, worst))

    runs = LC.hard_runs(case)
    p = Pool(pc)
    z, gamma, beta, mu, r, a = p.rc(d["z"]), p.new(C, d["gamma"]), p.new(C, d["beta"]), p.new(R), p.new(R), p.rc()
    kr = case["keep_rows"]
    keep = p.new(kr * C, d["keep"][:kr], U8)
    p.run("fwd", ["ln_fwd"], lambda: ln.fwd(z.view, a.view, R, C, gamma.view, beta.view, mu.view, r.view, eps=LC.HARD_EPS, lrelu_alpha=LC.HARD_ALPHA,
                                            keep=keep.view, scale=LC.HARD_SCALE, keep_elems=kr * C), written=[mu, r])
    held("fwd", dict(a=a.get(R, C), mu=mu.get(), r=r.get()))
    # the kernels that follow take the forward's own mu and r, as a step does
    mu.init, r.init = mu.get().copy(), r.get().copy()
    g, ad, dz, uo, ws = p.rc(d["g"]), p.rc(d["addend"]), p.rc(), p.rc(), p.ws()
    dg, db = p.new(C, d["old"][0]), p.new(C, d["old"][1])
    p.run("bwd", ["ln_bwd", "ln_finish"],
          lambda: ln.bwd(g.view, z.view, dz.view, R, C, gamma.view, beta.view, mu.view, r.view, lrelu_alpha=LC.HARD_ALPHA, keep=keep.view,
                         scale=LC.HARD_SCALE, keep_elems=kr * C, addend=ad.view, u_out=uo.view, u_rows=(0, R), dgamma=dg.view, dbeta=db.view,
                         dw_rows=case["dw_rows"], acc_beta=runs["bwd"][1][4], acc_scale=runs["bwd"][1][5], ws=ws.view), written=[dg, db])
    held("bwd", dict(dz=dz.get(R, C), u=uo.get(R, C), dgamma=dg.get(), dbeta=db.get()))
    zdot, v = p.rc(d["zdot"]), p.rc()
    p.run("tangent", ["ln_tangent"], lambda: ln.tangent(zdot.view, z.view, v.view, R, C, gamma.view, beta.view, mu.view, r.view, lrelu_alpha=LC.HARD_ALPHA))
    held("tangent", dict(v=v.get(R, C)))
    u, s, ws2, dg2 = p.rc(e.source(LC.HARD_ALPHA)["u"]), p.rc(), p.ws(), p.new(C, d["old"][0])
    p.run("source", ["ln_gp_source", "ln_finish"],
          lambda: ln.gp_source(u.view, zdot.view, z.view, s.view, R, C, gamma.view, mu.view, r.view, dg2.view, ws2.view, acc_beta=1.0, acc_scale=1.0),
          written=[dg2])
    held("source", dict(s=s.get(R, C), dgamma=dg2.get()))
    assert not failed, failed


# ------------------------------------------------------------------ refusals
FWD = "z a R C gamma beta eps alpha keep keep_scale keep_elems mu_o r_o stream".split()
BWD = ("g z dz R C gamma beta mu r alpha keep keep_scale keep_elems addend u_out u_row0 u_rows dgamma dbeta dw_rows acc_beta acc_scale ws ws_bytes "
       "stream").split()
TAN = "zdot z vout R C gamma beta mu r alpha stream".split()
SRC = "u zdot z s R C gamma mu r dgamma_s acc_beta acc_scale ws ws_bytes stream".split()
ENTRY = {"bg_ln_fwd_f32": FWD, "bg_ln_bwd_f32": BWD, "bg_ln_tangent_f32": TAN, "bg_ln_gp_source_f32": SRC}
POINTERS = {"bg_ln_fwd_f32": "z a gamma beta mu_o r_o".split(), "bg_ln_bwd_f32": "g z dz gamma beta mu r".split(),
            "bg_ln_tangent_f32": "zdot z vout gamma beta mu r".split(), "bg_ln_gp_source_f32": "u zdot z s gamma mu r dgamma_s".split()}
SHAPE, UNSUPPORTED, WORKSPACE, NULL = -1, -3, -5, -6          # include/bgan.h: BG_ERR_BAD_SHAPE, _UNSUPPORTED, _WORKSPACE, _NULL


def _refusals(R, C):
    """(entry point, arguments replaced -- a string names the buffer to alias --, the code of its BG_REQUIRE line)."""
    out = [(fn, {p: None}, NULL) for fn, ps in POINTERS.items() for p in ps]
    out += [("bg_ln_bwd_f32", {"dbeta": None}, NULL), ("bg_ln_bwd_f32", {"dgamma": None}, NULL)]
    out += [(fn, {k: v}, SHAPE) for fn in ENTRY for k, v in (("R", 0), ("R", -1), ("C", 0), ("C", -4))]
    out += [("bg_ln_fwd_f32", {"eps": 0.0}, SHAPE), ("bg_ln_fwd_f32", {"eps": -1.0}, SHAPE)]
    out += [(fn, {"keep_elems": n}, SHAPE) for fn in ("bg_ln_fwd_f32", "bg_ln_bwd_f32") for n in (C + 1, R * C - 1, (R + 1) * C)]
    out += [(fn, {"alpha": -0.25}, UNSUPPORTED) for fn in ("bg_ln_bwd_f32", "bg_ln_tangent_f32")]
    out += [("bg_ln_bwd_f32", w, SHAPE) for w in ({"u_row0": -1}, {"u_rows": 0}, {"u_row0": R - 1, "u_rows": 2}, {"u_row0": R, "u_rows": 1})]
    out += [("bg_ln_bwd_f32", {"dw_rows": R + 1}, SHAPE)]
    need = LC.workspace_bytes(R, C)
    out += [(fn, {"ws_bytes": need - 1}, WORKSPACE) for fn in ("bg_ln_bwd_f32", "bg_ln_gp_source_f32")]
    out += [(fn, {"ws": None}, WORKSPACE) for fn in ("bg_ln_bwd_f32", "bg_ln_gp_source_f32")]
    out += [("bg_ln_fwd_f32", {"a": "z"}, UNSUPPORTED)]
    out += [("bg_ln_gp_source_f32", {"s": k}, UNSUPPORTED) for k in ("u", "zdot", "z")]
    if LC.route_for(C)["chunks"] > 1:
        out += [("bg_ln_bwd_f32", {"dz": "g"}, UNSUPPORTED), ("bg_ln_bwd_f32", {"dz": "addend"}, UNSUPPORTED),
                ("bg_ln_tangent_f32", {"vout": "zdot"}, UNSUPPORTED)]
    return out


@pytest.mark.parametrize("R,C", [(8, 16), (6, 257), (6, 1028)])
def test_refusals_return_their_code_name_their_function_and_write_nothing(R, C):
    lib = _lib.load()
    rng = np.random.default_rng(C)
    p = Pool(dict(R=R, C=C))
    ins = {k: p.rc(rng.integers(-3, 4, size=R * C)) for k in ("z", "g", "zdot", "u", "addend")}
    ins.update(gamma=p.new(C, np.ones(C)), beta=p.new(C, np.zeros(C)), mu=p.new(R, np.zeros(R)), r=p.new(R, np.ones(R)),
               keep=p.new(R * C, np.ones(R * C), U8))
    outs = {k: p.rc() for k in ("a", "dz", "vout", "s", "u_out")}
    outs.update(mu_o=p.new(R), r_o=p.new(R), dgamma=p.new(C), dbeta=p.new(C), dgamma_s=p.new(C), ws=p.ws())
    need = LC.workspace_bytes(R, C)
    assert outs["ws"].n * 4 == need == lib.bg_ln_workspace_bytes(R, C)
    base = dict(ins, **outs, R=R, C=C, eps=2.0, alpha=0.25, keep_scale=2.0, keep_elems=0, u_row0=0, u_rows=R, dw_rows=0, acc_beta=0.0, acc_scale=1.0,
                ws_bytes=need, stream=ops._stream())
    torch.cuda.synchronize()
    cases = _refusals(R, C)
    for fn, repl, code in cases:
        vals = dict(base)
        for k, v in repl.items():
            vals[k] = base[v] if isinstance(v, str) else v
        args = [ctypes.c_void_p(v.view.data_ptr()) if isinstance(v, Guarded) else v for v in (vals[k] for k in ENTRY[fn])]
        rc = getattr(lib, fn)(*args)
        msg = lib.bg_last_error().decode()
        assert rc == code, (fn, repl, rc, code, msg)
        assert msg.startswith(fn + ":"), (fn, repl, msg)
    torch.cuda.synchronize()
    for k, g in outs.items():
        assert bool(torch.isnan(g.view).all()), f"a refused call wrote {k}"
    for g in p.all:
        assert g.guards_intact() and (g.init is None or g.unchanged())
    print(f"[ln refusals] R={R} C={C}: {len(cases)} calls refused")
    # the same buffers, nothing replaced: every entry point accepts them (the refusals above were the replaced argument's doing)
    for fn in ENTRY:
        args = [ctypes.c_void_p(v.view.data_ptr()) if isinstance(v, Guarded) else v for v in (base[k] for k in ENTRY[fn])]
        assert getattr(lib, fn)(*args) == 0, (fn, lib.bg_last_error().decode())
    torch.cuda.synchronize()
    for k in ("a", "dz", "vout", "s", "u_out", "mu_o", "r_o", "dgamma", "dbeta", "dgamma_s"):
        assert not bool(torch.isnan(outs[k].view).any()), k
    assert all(g.guards_intact() for g in p.all)
