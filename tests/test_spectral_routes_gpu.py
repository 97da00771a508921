"""GPU: the spectral normalisation kernels on the case table of tests/spectral_cases.py -- one case per route, loop trip and tail of
csrc/spectral.hip that tests/test_spectral_gpu.py does not reach (tests/test_spectral_cases_cpu.py holds each case to its claim).

Every run lays its buffers out with a guard band of a finite sentinel behind each region (W, grad, u, v, sigma, eff, the transposed
copy, the workspace); outputs start as NaN.  Parity of a full round, the scale and the gradient map is held to
sn_reference.kernel_case's bound unchanged (4 x what float32 numpy loses against float64, floor 16 * 2^-24); the sigma-only pass runs
on integer data where v^T W u is exact in any order and must equal the int64 reference; one table of all thirteen layers, in either
order, must give the bits of the thirteen single-layer runs."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import SENTINEL, rel_l2
import sn_reference as SR
import spectral_cases as SC

pytestmark = pytest.mark.gpu

G = 64                                        # floats of a guard band: a whole tile row, a multiple of 4
SENT = np.float32(SENTINEL[torch.float32])
pad4 = lambda n: -(-n // 4) * 4


class Layout:
    """Device buffers and the table of a list of matrices, every region followed by a guard band (offsets stay multiples of 4 floats).
    The room of a transposed copy is laid out for every layer; a layer with taps == 1 gets tr_off = -1 and the room must keep the
    sentinel."""

    def __init__(self, mats, taps):
        rows, ot, os_, oe = [], 0, 0, 0
        for m, t in zip(mats, taps):
            K, N = m["W"].shape
            u_off, v_off = os_, pad4(os_ + N) + G
            sigma_off = pad4(v_off + K) + G
            tr_room = pad4(oe + K * N) + G
            rows.append(dict(w_off=ot, u_off=u_off, v_off=v_off, sigma_off=sigma_off, eff_off=oe, tr_off=tr_room if t > 1 else -1, K=K, N=N,
                             taps=t, tr_room=tr_room))
            ot, os_, oe = pad4(ot + K * N) + G, pad4(sigma_off + 1) + G, pad4(tr_room + K * N) + G
        self.rows = rows
        nan = np.float32("nan")
        host = {k: np.full(n, SENT, np.float32) for k, n in (("theta", ot), ("grad", ot), ("state", os_), ("eff", oe))}
        inside = {k: np.zeros(a.size, bool) for k, a in host.items()}

        def put(name, off, values):
            v = np.asarray(values, np.float32).ravel()
            host[name][off:off + v.size] = v
            inside[name][off:off + v.size] = True
        for r, m in zip(rows, mats):
            K, N = r["K"], r["N"]
            put("theta", r["w_off"], m["W"])
            put("grad", r["w_off"], m["g"])
            put("state", r["u_off"], m["u0"])
            put("state", r["v_off"], m["v0"] if "v0" in m else np.full(K, nan))
            put("state", r["sigma_off"], [nan])
            put("eff", r["eff_off"], np.full(K * N, nan))
            if r["tr_off"] >= 0:
                put("eff", r["tr_off"], np.full(K * N, nan))
        self.host, self.inside = host, inside
        for k, a in host.items():
            setattr(self, k, torch.from_numpy(a.copy()).cuda())
        self.table = ops.SpectralTable(ops.spectral.rows(rows), "cuda")
        self.ws_floats = self.table.ws_bytes // 4
        assert self.ws_floats > 0 and self.ws_floats == sum(ops.spectral.route(r["K"], r["N"], r["taps"])["ws_floats"] for r in rows)
        self.ws = torch.full((self.ws_floats + G,), float(SENT), dtype=torch.float32, device="cuda")
        self.table.ws = self.ws[:self.ws_floats]              # the calls are told of ws_floats floats and not one more

    def run(self, sigma_only=False, power_only=False):
        ops.spectral.power(self.theta, self.state, self.table, sigma_only=sigma_only)
        if not power_only:
            ops.spectral.scale(self.theta, self.state, self.eff, self.table)
            ops.spectral.grad(self.grad, self.eff, self.state, self.table)
        torch.cuda.synchronize()
        return self

    def check_guards(self, what):
        bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
        for k in ("theta", "grad", "state", "eff"):
            got = getattr(self, k).cpu().numpy()
            band = ~self.inside[k]
            bad = np.flatnonzero(bits(got)[band] != bits(SENT))
            assert bad.size == 0, f"{what}: {k}: {bad.size} guard floats written, first at float {np.flatnonzero(band)[bad[0]]}"
        tail = self.ws[self.ws_floats:].cpu().numpy()
        assert (bits(tail) == bits(SENT)).all(), f"{what}: written behind the workspace's last float"
        assert np.array_equal(bits(self.theta.cpu().numpy()), bits(self.host["theta"])), f"{what}: theta changed"

    def out(self, i):
        r = self.rows[i]
        K, N, t = r["K"], r["N"], r["taps"]
        st, eff = self.state.cpu().numpy(), self.eff.cpu().numpy()
        o = dict(u=st[r["u_off"]:r["u_off"] + N], v=st[r["v_off"]:r["v_off"] + K], sigma=st[r["sigma_off"]],
                 Wbar=eff[r["eff_off"]:r["eff_off"] + K * N].reshape(K, N), grad=self.grad.cpu().numpy()[r["w_off"]:r["w_off"] + K * N].reshape(K, N))
        if r["tr_off"] >= 0:
            o["WbarT"] = eff[r["tr_off"]:r["tr_off"] + K * N].reshape(t, N, K // t)
        return o


_ref, _alone = {}, {}


def ref(c):
    """One reference per case, shared by the tests and left unchanged."""
    key = SC.case_id(c)
    if key not in _ref:
        _ref[key] = SR.kernel_case(c["K"], c["N"], seed=1000 * c["K"] + c["N"])
    return _ref[key]


def alone(c):
    """The case as the only layer of its table: one full round, scale, grad.  Run once; (layout, outputs)."""
    key = SC.case_id(c)
    if key not in _alone:
        lay = Layout([ref(c)], [c["taps"]]).run()
        _alone[key] = (lay, lay.out(0))
    return _alone[key]


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_full_round_scale_and_grad_match_float64(case):
    K, N, taps = case["K"], case["N"], case["taps"]
    c, what = ref(case), SC.case_id(case)
    lay, got = alone(case)
    failed = []
    for k in ("u", "v", "Wbar", "grad"):
        assert not np.isnan(got[k]).any(), (what, k)
        err = rel_l2(got[k], c["ref"][k])
        print(f"[{what}] {k}: rel-L2 {err:.2e} / bound {c['bound'][k]:.2e} = {err / c['bound'][k]:.2f}")
        failed += [(k, err, c["bound"][k])] if not err <= c["bound"][k] else []
    err = abs(float(got["sigma"]) - c["ref"]["sigma"]) / c["ref"]["sigma"]
    print(f"[{what}] sigma: rel {err:.2e} / bound {c['bound']['sigma']:.2e} = {err / c['bound']['sigma']:.2f}")
    failed += [("sigma", err, c["bound"]["sigma"])] if not err <= c["bound"]["sigma"] else []
    # <dL/dW, W> = 0, with the bound and the derivation of tests/test_spectral_gpu.py
    dW, W = got["grad"].astype(np.float64), c["W"].astype(np.float64)
    cos = abs((dW * W).sum()) / (np.linalg.norm(dW) * np.linalg.norm(W))
    print(f"[{what}] <dW, W> / (|dW| |W|) = {cos:.2e} / bound {42 * 2.0 ** -24 + c['bound']['sigma']:.2e}")
    failed += [("cos", cos, 42 * 2.0 ** -24 + c["bound"]["sigma"])] if not cos <= 42 * 2.0 ** -24 + c["bound"]["sigma"] else []
    assert not failed, (what, failed)
    if taps > 1:        # the transposed copy is the effective kernel's own bits, [taps][N][R]
        assert np.array_equal(got["WbarT"].view(np.uint32), got["Wbar"].reshape(taps, K // taps, N).transpose(0, 2, 1).view(np.uint32)), what


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_guard_bands_theta_and_the_absent_transposed_copy(case):
    lay, got = alone(case)
    lay.check_guards(SC.case_id(case))          # with taps == 1 the transposed copy's room is all guard band
    r = lay.rows[0]
    assert (r["tr_off"] >= 0) == (case["taps"] > 1) and ("WbarT" in got) == (case["taps"] > 1)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_sigma_only_is_exact_on_integer_data(case):
    W, u, v, want = SC.exact_data(case)
    lay = Layout([dict(W=W, u0=u, v0=v, g=np.zeros_like(W))], [case["taps"]])
    before = lay.state.clone()
    lay.run(sigma_only=True, power_only=True)
    got = lay.out(0)
    print(f"[{SC.case_id(case)}] sigma {float(got['sigma'])!r}, int64 reference {want}")
    assert float(got["sigma"]) == float(want), (SC.case_id(case), float(got["sigma"]), want, float(got["sigma"]) - want)
    assert np.array_equal(got["u"].view(np.uint32), u.view(np.uint32)) and np.array_equal(got["v"].view(np.uint32), v.view(np.uint32))
    r = lay.rows[0]
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[r["sigma_off"]] = False
    assert torch.equal(before[keep].view(torch.int32), lay.state[keep].view(torch.int32))      # nothing of the state but sigma
    lay.check_guards(SC.case_id(case))


@pytest.mark.parametrize("order", ["table order", "reverse order"])
def test_one_table_of_all_cases_gives_the_bits_of_the_single_runs(order):
    """find_layer with multi-unit layers in front, in all three unit numberings."""
    cases = SC.CASES if order == "table order" else SC.CASES[::-1]
    lay = Layout([ref(c) for c in cases], [c["taps"] for c in cases]).run()
    lay.check_guards(order)
    firsts = lay.table.host[:, 9:12]
    assert (np.diff(firsts, axis=0) > 0).all() and (firsts[0] == 0).all()
    for i, c in enumerate(cases):
        want, got = alone(c)[1], lay.out(i)
        assert set(want) == set(got)
        for k in want:
            assert np.array_equal(np.asarray(want[k]).view(np.uint32), np.asarray(got[k]).view(np.uint32)), (order, SC.case_id(c), k)
