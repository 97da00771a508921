"""The layer normalisation kernels (csrc/layernorm.hip; include/bgan.h "layer normalisation") against numpy float64.

Channel counts: 1, 3, 4, 5, 16, 20, 64 and, read from the library itself (ops.layernorm.route), the first C past every route
boundary of the kernels as built -- a change of the lanes that share a row (rows per wave), of the units a lane keeps in
registers, of the chunks a row is swept in -- with the last C before it, on the float4 route (C % 4 == 0) and the scalar one.
Rows: 1, one workgroup's rows - 1 / exactly / + 1, two workgroups' rows + 3; one case per route beyond the 1024-workgroup grid
(grid-stride loop).  Rows are N(0, 1) scaled by 0.1 ... 10, plus one row of constants (variance 0: xh = 0, r = 1 / sqrt(eps)) and
one row with a single nonzero.  Tolerances are the BatchNorm kernels' (tests/test_misc_gpu.py; the same arithmetic): outputs rtol
1e-4 / atol 2e-5; dgamma, dbeta rtol 2e-4 / atol 2e-4 * sqrt(R); dz, tangent, s rtol 2e-4 / atol 2e-5 * max(1, max|ref|).

The reference decides LeakyReLU's branch from its float64 pre-activation; every case first asserts, on the reference alone,
that none lies within 1e-5 of zero (float32 could sit on the other branch there); rows where one does are drawn again."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops

pytestmark = pytest.mark.gpu

EPS, ALPHA, SCALE = 1e-3, 0.3, 1.0 / 0.7
KINK = 1e-5
ln = ops.layernorm


# ------------------------------------------------------------------ cases
def _boundaries(limit=1100):
    """The first C past every change of route within the float4 class and within the scalar class, and the last before it."""
    out = set()
    for cls in (lambda c: c % 4 == 0, lambda c: c % 4 != 0):
        cs = [c for c in range(1, limit + 1) if cls(c)]
        key = lambda c: tuple(ln.route(c)[k] for k in ("vec", "lanes", "regs", "chunks"))
        for a, b in zip(cs, cs[1:]):
            if key(a) != key(b):
                out.update((a, b))
    return out


def _channels():
    try:
        return sorted({1, 3, 4, 5, 16, 20, 64} | _boundaries())
    except Exception:           # no library (collection on a host that has not built it): the named channel counts alone
        return [1, 3, 4, 5, 16, 20, 64]


def _rows(C):
    w = ln.route(C)["rows_per_workgroup"]
    return sorted({1, max(w - 1, 1), w, w + 1, 2 * w + 3})


# ------------------------------------------------------------------ float64 reference
def _stats(z):
    mu = z.mean(1, keepdims=True)
    r = 1.0 / np.sqrt(((z - mu) ** 2).mean(1, keepdims=True) + EPS)
    return mu, r, (z - mu) * r


def _M(y, xh, r):
    yc = y - y.mean(1, keepdims=True)
    return r * (yc - xh * (yc * xh).mean(1, keepdims=True))


def _factor(n, keep, keep_rows):
    f = np.where(n > 0, 1.0, ALPHA)
    if keep is not None:
        f[:keep_rows] = np.where(keep[:keep_rows] != 0, f[:keep_rows] * SCALE, 0.0)
    return f


def _data(R, C, seed):
    """Inputs of one case.  Rows with a reference pre-activation within KINK of zero are drawn again (the reference alone decides)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    rows = lambda n: f32(rng.normal(size=(n, C)) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=(n, 1))))
    z = rows(R)
    if R >= 3:
        z[1] = 1.5                                   # a row of constants
        z[2] = 0.0
        z[2, rng.integers(C)] = 2.25                 # a row with a single nonzero
    gamma = f32(1 + 0.2 * rng.uniform(size=C))
    beta = f32(rng.choice([-1.0, 1.0], size=C) * rng.uniform(0.05, 0.3, size=C))
    for _ in range(50):
        mu, r, xh = _stats(z)
        bad = np.flatnonzero(np.abs(gamma * xh + beta).min(1) <= KINK)
        if not bad.size:
            break
        z[bad] = rows(bad.size)
        if R >= 3 and 2 in bad:                      # the single nonzero again, elsewhere (the row of constants has n = beta: never close)
            z[2] = 0.0
            z[2, rng.integers(C)] = np.float32(rng.uniform(1.0, 3.0))
    assert np.abs(gamma * _stats(z)[2] + beta).min() > KINK
    return dict(z=z, gamma=gamma, beta=beta, g=f32(rng.normal(size=(R, C))), zdot=f32(rng.normal(size=(R, C))),
                addend=f32(rng.normal(size=(R, C))), keep=(rng.uniform(size=(R, C)) >= 0.3).astype(np.uint8),
                old=f32(rng.normal(size=(2, C))))


def dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def close(got, want, rtol, atol, what):
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"[{what}] max|err| {err:.2e} max|ref| {float(np.abs(want).max()):.2e} atol {atol:.1e}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


def wide(ref):
    return 2e-5 * max(1.0, float(np.abs(ref).max()))


def _ws(R, C):
    return torch.empty(max(ln.workspace_bytes(R, C) // 4, 4), dtype=torch.float32, device="cuda")


def check_case(R, C, seed, keep_rows_list=None):
    d = _data(R, C, seed)
    z, gamma, beta = d["z"], d["gamma"], d["beta"]
    mu, r, xh = _stats(z)
    n = gamma * xh + beta
    zt, gt, bt = dev(z), dev(gamma), dev(beta)
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device="cuda")
    mut, rt = new(R), new(R)
    tag = f"R={R} C={C}"
    # ---- forward and backward: without a mask, with a full one, with one that covers only the first rows
    for keep_rows in keep_rows_list if keep_rows_list is not None else (None, R, max(R // 2, 1)):
        keep = None if keep_rows is None else d["keep"]
        kw = {} if keep is None else dict(keep=dev(keep[:keep_rows], torch.uint8), scale=SCALE, keep_elems=0 if keep_rows == R else keep_rows * C)
        f = _factor(n, keep, keep_rows)
        a = ln.fwd(zt, new(R, C), R, C, gt, bt, mut, rt, eps=EPS, lrelu_alpha=ALPHA, **kw)
        close(host(a), n * f, 1e-4, 2e-5, f"{tag} keep_rows={keep_rows} a")
        close(host(mut), mu[:, 0], 1e-4, 2e-5, f"{tag} mu")
        close(host(rt), r[:, 0], 1e-4, 2e-5, f"{tag} r")
        u = d["g"] * f
        dz_ref = _M(gamma * u, xh, r)
        # backward: the generator step's form (no sums), dz in place where the route allows it
        chunked = ln.route(C)["chunks"] > 1
        gbuf = dev(d["g"])
        dz = ln.bwd(gbuf, zt, new(R, C) if chunked else gbuf, R, C, gt, bt, mut, rt, lrelu_alpha=ALPHA, **kw)
        close(host(dz), dz_ref, 2e-4, wide(dz_ref), f"{tag} keep_rows={keep_rows} dz (no sums)")
        # backward with sums over a row sub-range, u of a row sub-range, an addend, beta = 0 and beta = 1
        dw = max(R - R // 3, 1)
        lo, hi = R // 4, R
        for acc_beta, acc_scale in ((0.0, 1.0), (1.0, 0.5)):
            dg, db, uo = dev(d["old"][0]), dev(d["old"][1]), new(hi - lo, C)
            dz = ln.bwd(dev(d["g"]), zt, new(R, C), R, C, gt, bt, mut, rt, lrelu_alpha=ALPHA, addend=dev(d["addend"]), u_out=uo,
                        u_rows=(lo, hi), dgamma=dg, dbeta=db, dw_rows=dw, acc_beta=acc_beta, acc_scale=acc_scale, ws=_ws(R, C), **kw)
            close(host(dz), dz_ref + d["addend"], 2e-4, wide(dz_ref + d["addend"]), f"{tag} dz + addend")
            close(host(uo), u[lo:hi], 1e-4, 2e-5, f"{tag} u rows [{lo}, {hi})")
            close(host(dg), acc_beta * d["old"][0] + acc_scale * (u * xh)[:dw].sum(0), 2e-4, 2e-4 * np.sqrt(R), f"{tag} dgamma beta={acc_beta}")
            close(host(db), acc_beta * d["old"][1] + acc_scale * u[:dw].sum(0), 2e-4, 2e-4 * np.sqrt(R), f"{tag} dbeta beta={acc_beta}")
    # ---- tangent and second-order source (no Dropout on the x-hat rows)
    f = _factor(n, None, 0)
    Mz = _M(d["zdot"], xh, r)
    v = ln.tangent(dev(d["zdot"]), zt, new(R, C), R, C, gt, bt, mut, rt, lrelu_alpha=ALPHA)
    close(host(v), f * gamma * Mz, 2e-4, wide(f * gamma * Mz), f"{tag} tangent")
    u = d["g"] * f
    p = gamma * u - (gamma * u).mean(1, keepdims=True)
    q = d["zdot"] - d["zdot"].mean(1, keepdims=True)
    A, Bq, D = ((p * xh).mean(1, keepdims=True), (q * xh).mean(1, keepdims=True), (p * q).mean(1, keepdims=True))
    s_ref = -r ** 2 * (p * Bq + q * A + xh * (D - 3 * A * Bq))
    for acc_beta in (0.0, 1.0):
        dg = dev(d["old"][0])
        s = ln.gp_source(dev(u), dev(d["zdot"]), zt, new(R, C), R, C, gt, mut, rt, dg, _ws(R, C), acc_beta=acc_beta)
        close(host(s), s_ref, 2e-4, wide(s_ref), f"{tag} s")
        close(host(dg), acc_beta * d["old"][0] + (u * Mz).sum(0), 2e-4, 2e-4 * np.sqrt(R), f"{tag} source dgamma beta={acc_beta}")
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", _channels())
def test_kernels_match_float64_at_every_route_and_row_count(C):
    for R in _rows(C):
        check_case(R, C, seed=1000 * C + R)


@pytest.mark.parametrize("C,workgroups", [(16, 1024 + 1), (516, 1024 + 1), (5, 1024 + 2)])
def test_kernels_match_float64_beyond_one_grid_of_workgroups(C, workgroups):
    """More row groups than the grid holds workgroups: the grid-stride loop, and column sums a lane carries across its visits."""
    R = workgroups * ln.route(C)["rows_per_workgroup"] + 5
    check_case(R, C, seed=7 + C, keep_rows_list=(R // 2,))


def test_the_route_table_is_what_the_cases_assume():
    assert ln.route(1) == dict(vec=1, lanes=1, regs=1, chunks=1, rows_per_workgroup=256)
    assert ln.route(16) == dict(vec=4, lanes=4, regs=1, chunks=1, rows_per_workgroup=64)
    assert ln.route(512)["regs"] == 2 and ln.route(1024)["regs"] == 4 and ln.route(1024)["chunks"] == 1
    assert ln.route(1028) == dict(vec=4, lanes=64, regs=1, chunks=5, rows_per_workgroup=4) and ln.route(257)["chunks"] == 5
    assert ln.route(255)["chunks"] == 1 and ln.route(255)["regs"] == 4
    cs = _channels()
    assert {8, 1024, 1028, 255, 257} <= set(cs), cs


def test_special_rows_alone():
    """R = 1 constant row: mu = the value, xh = 0, r = 1 / sqrt(eps) exactly as float32 gives it; a = LeakyReLU(beta)."""
    C = 20
    z = torch.full((1, C), 1.5, device="cuda")
    gamma, beta = torch.ones(C, device="cuda"), torch.linspace(-0.5, 0.5, C, device="cuda")
    mu, r = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    a = ln.fwd(z, torch.empty_like(z), 1, C, gamma, beta, mu, r, eps=EPS, lrelu_alpha=ALPHA)
    assert float(mu) == 1.5
    np.testing.assert_allclose(float(r), 1.0 / np.sqrt(EPS), rtol=1e-6)
    assert torch.equal(a[0], torch.where(beta > 0, beta, ALPHA * beta))


def test_backward_sums_are_bit_identical_from_run_to_run():
    R, C = 3 * 1024 * 4 + 77, 512
    d = _data(R, C, 5)
    zt, gt, bt, g = dev(d["z"]), dev(d["gamma"]), dev(d["beta"]), dev(d["g"])
    mu, r = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    ln.fwd(zt, torch.empty_like(zt), R, C, gt, bt, mu, r, eps=EPS, lrelu_alpha=ALPHA)
    runs = []
    for _ in range(2):
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        ln.bwd(g, zt, torch.empty_like(zt), R, C, gt, bt, mu, r, lrelu_alpha=ALPHA, dgamma=dg, dbeta=db, ws=_ws(R, C))
        runs.append((dg.clone(), db.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("which", ["z", "a", "g", "dz", "gamma", "keep", "zdot", "s"])
def test_misaligned_views_are_refused_and_nothing_is_launched(which):
    R, C = 8, 16
    n = R * C
    off = lambda dt=torch.float32: torch.zeros(n + 4, dtype=dt, device="cuda")[1:1 + n]       # 4 (or 1) bytes past a 16-byte boundary
    ok = lambda dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    t = {k: (off() if k == which else ok()) for k in ("z", "a", "g", "dz", "zdot", "s")}
    keep = off(torch.uint8) if which == "keep" else ok(torch.uint8)
    gamma = torch.ones(C + 4, device="cuda")[1:1 + C] if which == "gamma" else torch.ones(C, device="cuda")
    beta, mu, r = torch.zeros(C, device="cuda"), torch.zeros(R, device="cuda"), torch.ones(R, device="cuda")
    sentinel = lambda x: x.fill_(-7.0)
    outs = [sentinel(t["a"]), sentinel(t["dz"]), sentinel(t["s"])]
    dg = sentinel(torch.empty(C, device="cuda"))
    calls = {
        "fwd": lambda: ln.fwd(t["z"], t["a"], R, C, gamma, beta, mu, r, keep=keep, scale=SCALE),
        "bwd": lambda: ln.bwd(t["g"], t["z"], t["dz"], R, C, gamma, beta, mu, r, keep=keep, scale=SCALE, dgamma=dg, dbeta=dg.clone(), ws=_ws(R, C)),
        "tangent": lambda: ln.tangent(t["zdot"], t["z"], t["dz"], R, C, gamma, beta, mu, r),
        "source": lambda: ln.gp_source(t["g"], t["zdot"], t["z"], t["s"], R, C, gamma, mu, r, dg, _ws(R, C)),
    }
    uses = {"z": calls, "a": ["fwd"], "g": ["bwd", "source"], "dz": ["bwd", "tangent"], "gamma": calls, "keep": ["fwd", "bwd"],
            "zdot": ["tangent", "source"], "s": ["source"]}[which]
    for name in uses:
        with pytest.raises(ValueError, match="16-byte aligned"):
            calls[name]()
    torch.cuda.synchronize()
    for o in outs + [dg]:
        assert bool((o == -7.0).all()), "a refused call wrote"
