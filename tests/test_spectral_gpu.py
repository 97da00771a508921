"""GPU tests of the spectral normalisation kernels (csrc/spectral.hip) on their own: parity with float64 numpy on every route and
tail, known answers, determinism.

The bound of every comparison comes from the reference side only (tests/sn_reference.py kernel_case): 4 x the error a float32
numpy evaluation of the same formulas shows against the float64 one, never below 16 * 2^-24.  The margin of 4 covers a summation
order that differs from numpy's; both are trees of logarithmic depth."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import rel_l2
import sn_reference as SR

pytestmark = pytest.mark.gpu

CASES = [(25, 4), (100, 8), (72, 1),            # tiny_mnist: packed rows, N = 1
         (75, 16), (400, 32), (128, 1),         # tiny
         (800, 3),                              # the generator's RGB conv: rows misaligned for float4
         (16, 32),                              # a 1x1 kernel
         (25, 64),                              # MNIST's transposed conv
         (7, 67),                               # prime width above one wave
         (1, 5),                                # one row: sigma is its norm
         (100, 8192),                           # chunked rows
         (2048, 1), (6400, 512), (12800, 512)]  # real sizes
TAPS = {(25, 4): 25, (100, 8): 25, (75, 16): 25, (400, 32): 25, (800, 3): 25, (16, 32): 1, (25, 64): 25, (6400, 512): 25, (12800, 512): 25}


class Batch:
    """Device buffers and the table for a list of matrices, laid out as layers.ParamStore lays them out."""

    def __init__(self, mats, taps=None):
        pad = lambda n: -(-n // 4) * 4
        self.shapes = [m["W"].shape for m in mats]
        taps = taps or [1] * len(mats)
        rows, ot, os_, oe = [], 0, 0, 0
        for (K, N), t in zip(self.shapes, taps):
            rows.append(dict(w_off=ot, u_off=os_, v_off=os_ + pad(N), sigma_off=os_ + pad(N) + pad(K), eff_off=oe,
                             tr_off=oe + pad(K * N) if t > 1 else -1, K=K, N=N, taps=t))
            ot, os_, oe = ot + pad(K * N), os_ + pad(N) + pad(K) + 4, oe + 2 * pad(K * N)
        self.rows = rows
        theta, state, grad = np.zeros(ot, np.float32), np.zeros(os_, np.float32), np.zeros(ot, np.float32)
        for r, m in zip(rows, mats):
            K, N = r["K"], r["N"]
            theta[r["w_off"]:r["w_off"] + K * N] = m["W"].ravel()
            grad[r["w_off"]:r["w_off"] + K * N] = m["g"].ravel()
            state[r["u_off"]:r["u_off"] + N] = m["u0"]
            if "v0" in m:
                state[r["v_off"]:r["v_off"] + K] = m["v0"]
        dev = lambda a: torch.from_numpy(a).cuda()
        self.theta, self.state, self.grad = dev(theta), dev(state), dev(grad)
        self.eff = torch.full((max(oe, 4),), float("nan"), dtype=torch.float32, device="cuda")
        self.table = ops.SpectralTable(ops.spectral.rows(rows), "cuda")

    def run(self, rounds=1, sigma_only=False):
        for _ in range(rounds):
            ops.spectral.power(self.theta, self.state, self.table, sigma_only=sigma_only)
        ops.spectral.scale(self.theta, self.state, self.eff, self.table)
        ops.spectral.grad(self.grad, self.eff, self.state, self.table)
        torch.cuda.synchronize()
        return self

    def out(self, i):
        r = self.rows[i]
        K, N, t = r["K"], r["N"], r["taps"]
        st, eff = self.state.cpu().numpy(), self.eff.cpu().numpy()
        o = dict(u=st[r["u_off"]:r["u_off"] + N], v=st[r["v_off"]:r["v_off"] + K], sigma=st[r["sigma_off"]],
                 Wbar=eff[r["eff_off"]:r["eff_off"] + K * N].reshape(K, N), grad=self.grad.cpu().numpy()[r["w_off"]:r["w_off"] + K * N].reshape(K, N))
        if r["tr_off"] >= 0:
            o["WbarT"] = eff[r["tr_off"]:r["tr_off"] + K * N].reshape(t, N, K // t)
        return o


_cache = {}


def case(K, N):
    """One reference per (K, N), shared by the tests and left unchanged."""
    if (K, N) not in _cache:
        _cache[(K, N)] = SR.kernel_case(K, N, seed=1000 * K + N)
    return _cache[(K, N)]


def _check(got, c, what):
    for k in ("u", "v", "Wbar", "grad"):
        err = rel_l2(got[k], c["ref"][k])
        print(f"[{what}] {k}: rel-L2 {err:.2e}, bound {c['bound'][k]:.2e}")
        assert err <= c["bound"][k], (what, k, err, c["bound"][k])
    err = abs(float(got["sigma"]) - c["ref"]["sigma"]) / c["ref"]["sigma"]
    print(f"[{what}] sigma: rel {err:.2e}, bound {c['bound']['sigma']:.2e}")
    assert err <= c["bound"]["sigma"], (what, err, c["bound"]["sigma"])


@pytest.mark.parametrize("K,N", CASES)
def test_parity_with_float64_numpy(K, N):
    c = case(K, N)
    taps = TAPS.get((K, N), 1)
    got = Batch([c], [taps]).run().out(0)
    _check(got, c, f"{K}x{N}")
    if taps > 1:        # the transposed copy is the effective kernel's own bits, [taps][N][R]
        assert np.array_equal(got["WbarT"], got["Wbar"].reshape(taps, K // taps, N).transpose(0, 2, 1))
    # <dL/dW, W> = 0: the loss does not change when W is rescaled.  sigma <dW, W> = <g, W-bar> sigma - d v^T W u with d the computed
    # dot, so |cos| <= |d - <g, W-bar>| / (|g| |W-bar|) + |v^T W u - sigma| / sigma + the roundings of W-bar and of dW themselves.
    # No path through the dot's fixed-order summation is longer than 40 additions (3 in a float4, 16 per thread, 6 + 3 in the
    # workgroup, 2 + 6 + 3 over the partials), each 2^-24 relative to the sum of magnitudes, itself <= |g| |W-bar|
    dW, W = got["grad"].astype(np.float64), c["W"].astype(np.float64)
    cos = abs((dW * W).sum()) / (np.linalg.norm(dW) * np.linalg.norm(W))
    print(f"[{K}x{N}] <dW, W> / (|dW| |W|) = {cos:.2e}")
    assert cos <= 42 * 2.0 ** -24 + c["bound"]["sigma"]


def test_one_row_and_one_column():
    got = Batch([case(1, 5)]).run().out(0)
    w = case(1, 5)["W"].astype(np.float64)
    assert abs(got["sigma"] - np.linalg.norm(w)) <= SR.FLOOR * np.linalg.norm(w)
    c = case(72, 1)
    got = Batch([c]).run().out(0)
    w, g = c["W"].astype(np.float64).ravel(), c["g"].astype(np.float64).ravel()
    n = np.linalg.norm(w)
    assert abs(got["sigma"] - n) <= c["bound"]["sigma"] * n and abs(abs(got["u"][0]) - 1) <= SR.FLOOR
    want = (g - (g @ (w / n)) * (w / n)) / n
    assert rel_l2(got["grad"].ravel(), want) <= c["bound"]["grad"]


def test_rank_one():
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=37), rng.normal(size=12)
    c = SR.kernel_case(37, 12, seed=8, W=np.outer(a, b).astype(np.float32))
    got = Batch([c]).run().out(0)
    W = c["W"].astype(np.float64)
    s = np.linalg.svd(W, compute_uv=False)[0]
    assert abs(got["sigma"] - s) <= c["bound"]["sigma"] * s
    # float32 W is a b^T with every entry rounded, so u is held against the rounded matrix's own first right singular vector (b / |b|
    # up to those roundings); its second singular value is at rounding level, and one round leaves (s2 / s1)^2 of it: nothing
    bn = b / np.linalg.norm(b)
    top = np.linalg.svd(W)[2][0]
    assert min(rel_l2(top, bn), rel_l2(top, -bn)) < 1e-6
    assert min(rel_l2(got["u"], top), rel_l2(got["u"], -top)) <= c["bound"]["u"]


def test_prescribed_singular_values_after_twenty_rounds():
    rng = np.random.default_rng(11)
    K, N = 40, 24
    U, _ = np.linalg.qr(rng.normal(size=(K, N)))
    V, _ = np.linalg.qr(rng.normal(size=(N, N)))
    sv = np.array([3.0, 1.0] + [0.5] * (N - 2))
    W = ((U * sv) @ V.T).astype(np.float32)
    c = SR.kernel_case(K, N, seed=12, rounds=20, W=W)
    got = Batch([c]).run(rounds=20).out(0)
    s = np.linalg.svd(W.astype(np.float64), compute_uv=False)[0]
    err = abs(got["sigma"] - s) / s
    print(f"sigma {got['sigma']:.8f} svd {s:.8f} rel {err:.2e} bound {c['bound']['sigma']:.2e}")
    assert err <= c["bound"]["sigma"]


def test_sigma_only_leaves_the_vectors_and_equals_vWu():
    c = dict(case(400, 32))
    rng = np.random.default_rng(3)
    c["v0"] = SR.normalize(rng.normal(size=400)).astype(np.float32)
    b = Batch([c], [25])
    before = b.state.clone()
    b.run(sigma_only=True)
    r = b.rows[0]
    after = b.state
    assert torch.equal(before[r["u_off"]:r["u_off"] + 32], after[r["u_off"]:r["u_off"] + 32])
    assert torch.equal(before[r["v_off"]:r["v_off"] + 400], after[r["v_off"]:r["v_off"] + 400])
    want = SR.sigma_only(c["W"].astype(np.float64), c["u0"].astype(np.float64), c["v0"].astype(np.float64))
    lost = abs(SR.sigma_only(c["W"], c["u0"], c["v0"]) - want)
    got = float(b.out(0)["sigma"])
    # the floor: a few roundings relative to the sum of the terms' magnitudes, which is what a summation's error scales with
    assert abs(got - want) <= max(4 * lost, SR.FLOOR * float(np.abs(c["v0"]) @ np.abs(c["W"]) @ np.abs(c["u0"])))


def test_runs_are_bit_identical_and_batching_changes_no_bit():
    shapes = [((75, 16), 25), ((400, 32), 25), ((128, 1), 1), ((800, 3), 25), ((100, 8192), 1), ((6400, 512), 25), ((7, 67), 1)]
    mats = [case(*s) for s, _ in shapes]
    taps = [t for _, t in shapes]
    one, two = Batch(mats, taps).run(), Batch(mats, taps).run()
    for name in ("state", "eff", "grad"):
        a, b = getattr(one, name), getattr(two, name)
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)), name
    for i, (m, t) in enumerate(zip(mats, taps)):
        alone, batched = Batch([m], [t]).run().out(0), one.out(i)
        for k in alone:
            assert np.array_equal(alone[k], batched[k]), (shapes[i], k)
