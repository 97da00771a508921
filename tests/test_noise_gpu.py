"""GPU tests of bg_normal_f32 (csrc/misc.hip) and of the NoiseInjection kernels (csrc/noise.hip) against tests/noise_reference.py:
the draw against its float64 restatement computed from the same Philox words, the add bit for bit against numpy float32 arithmetic,
the strength gradient exactly on integer data, on every case of tests/noise_cases.py, 16-byte aligned and one float off."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import Guarded
import noise_cases as NC
import noise_reference as NR

pytestmark = pytest.mark.gpu

# Largest |got - ref| / max(|ref|, 1e-3) of the device draw against the float64 restatement.  Measured on an MI355X over one 2^20
# draw (seed 0x1234567, offset 77): 2.163e-07 (1.8 ulp of float32: logf, sqrtf, cospi / sinpi and the product, one rounding each);
# the bound is 4 x that, 8.7e-07, and may not exceed 1e-5 (beyond, a wrong formula would pass, not rounding).
NORMAL_ERR_MEASURED = 2.163e-7
NORMAL_TOL = 4 * NORMAL_ERR_MEASURED
assert NORMAL_TOL <= 1e-5


def _rel_err(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-3)).max())


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("n,shift", [(4096, 0), (1000, 0), (1003, 1), (37, 5), (16 * 700 + 9, 16)])
def test_normal_draw_is_counter_addressed_and_matches_the_restatement(n, shift):
    """Element e is value e % 4 of the Box-Muller block on the Philox words with counter offset + e / 4 (third counter word 2),
    whatever the output's alignment; nothing is written outside; the same (seed, offset) gives the same bits; draws of n and n'
    agree on their common prefix; a draw at offset + k is the tail of the draw at offset."""
    seed, offset = 0x1234567, 77
    ref = NR.np_normal(n, seed, offset)
    buf = torch.zeros(n + shift + 16, dtype=torch.float32, device="cuda")
    got = ops.rng.normal(buf[shift:shift + n], seed, offset).cpu().numpy()
    err = _rel_err(got, ref)
    print(f"n={n} shift={shift}: max rel err {err:.3e}")
    assert err <= NORMAL_TOL
    assert np.abs(got).max() <= NR.MAX_ABS
    assert not buf[:shift].any().item() and not buf[shift + n:].any().item()          # nothing written outside
    again = ops.rng.normal(torch.empty(n, device="cuda"), seed, offset).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))                 # aligned or not: the same bits
    for m in (n // 2 + 1, n - 1, 3):
        part = ops.rng.normal(torch.empty(m, device="cuda"), seed, offset).cpu().numpy()
        assert np.array_equal(part.view(np.uint32), got[:m].view(np.uint32)), m
    tail = ops.rng.normal(torch.empty(n - 8, device="cuda"), seed, offset + 2).cpu().numpy()
    assert np.array_equal(tail.view(np.uint32), got[8:].view(np.uint32))
    other = ops.rng.normal(torch.empty(n, device="cuda"), seed + 1, offset).cpu().numpy()
    assert not np.array_equal(other, got)


def test_normal_draw_accuracy_over_a_million_values():
    """The measurement behind NORMAL_TOL (printed), and the bound itself, over one 2^20 draw.  Measured on an MI355X: 2.163e-07."""
    n, seed, offset = 1 << 20, 0x1234567, 77
    got = ops.rng.normal(torch.empty(n, device="cuda"), seed, offset).cpu().numpy()
    err = _rel_err(got, NR.np_normal(n, seed, offset))
    print(f"bg_normal_f32 over 2^20 values: max |got - ref| / max(|ref|, 1e-3) = {err:.3e} (bound {NORMAL_TOL:.1e})")
    assert err <= NORMAL_TOL


@pytest.mark.parametrize("seed,offset", [(0x1234567, 77), (123, 0), (5, 2 ** 33), (99, 1000)])
def test_normal_draw_statistics(seed, offset):
    got = ops.rng.normal(torch.empty(1 << 20, device="cuda"), seed, offset).cpu().numpy()
    st = NR.statistics(got)
    print(seed, offset, st)
    NR.check_statistics(st)


def test_normal_draw_uniform_edges():
    """Both ends of u1, at counters found by searching the restatement's Philox words (seed 7): block 4952199 has word 0 =
    0xffffffac, so u1 = 1 and elements 0 and 1 are exact zeros; block 137486 has word 2 = 0x17, so u1 = 2^-24 and elements 2 and 3 lie
    on the circle of radius sqrt(48 log 2) = 5.768, the largest the draw can give.  Then the bound over 2^24 values."""
    seed = 7
    w = NR.philox4x32_10(np.array([4952199, 137486], np.uint64), seed, 2)
    assert int(w[0, 0]) >> 8 == 0xFFFFFF and int(w[1, 2]) >> 8 == 0
    one = ops.rng.normal(torch.empty(4, device="cuda"), seed, 4952199).cpu().numpy()
    ref = NR.np_normal(4, seed, 4952199)
    assert one[0] == 0.0 and one[1] == 0.0 and ref[0] == 0.0 and ref[1] == 0.0
    assert _rel_err(one[2:], ref[2:]) <= NORMAL_TOL
    far = ops.rng.normal(torch.empty(4, device="cuda"), seed, 137486).cpu().numpy()
    ref = NR.np_normal(4, seed, 137486)
    assert _rel_err(far, ref) <= NORMAL_TOL
    radius = float(np.hypot(np.float64(far[2]), np.float64(far[3])))
    assert abs(radius - np.sqrt(48 * np.log(2))) <= 2 * NORMAL_TOL * radius and radius <= NR.MAX_ABS
    got = ops.rng.normal(torch.empty(1 << 24, device="cuda"), seed, 0)
    assert got.abs().max().item() <= NR.MAX_ABS and torch.isfinite(got).all().item()


# ------------------------------------------------------------------ the add
@pytest.mark.parametrize("off", NC.OFFSETS)
@pytest.mark.parametrize("name", [c[0] for c in NC.CASES])
def test_add_is_bit_exact(name, off):
    _, R, Cc = NC.case(name)
    rng = np.random.default_rng(R * 131 + Cc)
    x = rng.normal(size=(R, Cc)).astype(np.float32)
    nz = rng.normal(size=R).astype(np.float32)
    s = np.float32(0.37)
    sd = torch.tensor([s], device="cuda")
    for alpha in NC.ALPHAS:
        want = NR.np_add(x, nz, s, alpha)
        for alias in (False, True):
            gx, gn = Guarded(R * Cc, x, offset=off), Guarded(R, nz, offset=off)
            gy = gx if alias else Guarded(R * Cc, offset=off)
            ops.noise.add(gx.view, gn.view, sd, gy.view, R, Cc, lrelu_alpha=alpha)
            got = gy.get(R, Cc)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, off, alpha, alias)
            assert gx.guards_intact() and gy.guards_intact() and gn.guards_intact() and gn.unchanged()
            assert alias or gx.unchanged()
    assert ops.noise.route(Cc, aligned=off == 0)["vec"] == (4 if Cc % 4 == 0 and off == 0 else 1)


def test_add_reads_the_strength_from_device_memory():
    """A changed strength is seen by the next launch (a replayed step program holds the address, not the value); strength 0
    leaves LeakyReLU(x)."""
    rng = np.random.default_rng(5)
    x, nz = rng.normal(size=(9, 8)).astype(np.float32), rng.normal(size=9).astype(np.float32)
    xd, nd, y = (torch.from_numpy(a).cuda() for a in (x, nz, np.empty_like(x)))
    sd = torch.zeros(1, device="cuda")
    for s in (0.0, -1.5, 0.25):
        sd.fill_(s)
        got = ops.noise.add(xd, nd, sd, y, 9, 8, lrelu_alpha=0.2).cpu().numpy()
        assert np.array_equal(got, NR.np_add(x, nz, np.float32(s), 0.2)), s
    sd.fill_(0.0)
    assert np.array_equal(ops.noise.add(xd, nd, sd, y, 9, 8, lrelu_alpha=0.2).cpu().numpy(), np.where(x > 0, x, np.float32(0.2) * x))


# ------------------------------------------------------------------ the strength's gradient
def _ws(R, Cc):
    return Guarded(max(ops.noise.workspace_bytes(R, Cc) // 4, 1))


@pytest.mark.parametrize("off", NC.OFFSETS)
@pytest.mark.parametrize("name", [c[0] for c in NC.CASES])
def test_gradient_is_exact_on_integer_data(name, off):
    _, R, Cc = NC.case(name)
    dz, nz = NC.integer_data(R, Cc, R * 17 + Cc)
    total = NR.np_grad(dz, nz)
    assert total == float(np.float32(total))
    gd, gn, ws = Guarded(R * Cc, dz, offset=off), Guarded(R, nz, offset=off), _ws(R, Cc)
    for beta, scale, old in ((0.0, 1.0, float("nan")), (1.0, 0.5, 5.0)):          # beta = 0: the old value is not read
        out = Guarded(1, [old])
        bits = []
        for _ in range(2):
            out.view.fill_(old)
            ops.noise.grad(gd.view, gn.view, out.view, R, Cc, ws.view, beta=beta, scale=scale)
            bits.append(out.get().view(np.uint32).copy())
        assert out.get()[0] == (beta * old if beta else 0.0) + scale * total, (name, off, beta, scale, out.get()[0], total)
        assert np.array_equal(bits[0], bits[1])
        assert out.guards_intact() and ws.guards_intact() and gd.guards_intact() and gd.unchanged() and gn.unchanged()


# (R, C), the data's seed and, from the reference alone, sum_r |n_r| sum_c |dz_rc| / |sum_r n_r sum_c dz_rc|: how much larger
# than the result the terms are that cancel in it (seeds 1-8 on a CPU: 49, 125, 13.2, 186, 11.6, 22.5, 33.5, 15.5; a float32
# row-by-row sum of seed 5 is then within 1e-7 of the float64 one, a hundredth of the bound)
NORMAL_GRAD_CASE = ("c64_r17", 5, 12.0)


def test_gradient_on_normal_data():
    name, seed, max_cond = NORMAL_GRAD_CASE
    _, R, Cc = NC.case(name)
    dz, nz = NC.normal_data(R, Cc, seed)
    dz32, nz32 = dz.astype(np.float32), nz.astype(np.float32)
    ref = NR.np_grad(dz32, nz32, old=0.75, beta=1.0, scale=0.5)
    cond = float((np.abs(nz32.astype(np.float64)) * np.abs(dz32.astype(np.float64)).sum(1)).sum() / abs(NR.np_grad(dz32, nz32)))
    assert cond < max_cond, cond
    for off in NC.OFFSETS:
        gd, gn, ws, out = Guarded(R * Cc, dz32, offset=off), Guarded(R, nz32, offset=off), _ws(R, Cc), Guarded(1, [0.75])
        ops.noise.grad(gd.view, gn.view, out.view, R, Cc, ws.view, beta=1.0, scale=0.5)
        first = out.get().copy()
        print(f"offset {off}: got {first[0]!r}, reference {ref!r}, rel err {abs(first[0] - ref) / abs(ref):.2e}, cond {cond:.1f}")
        np.testing.assert_allclose(first[0], ref, rtol=1e-5)
        out.view.fill_(0.75)
        ops.noise.grad(gd.view, gn.view, out.view, R, Cc, ws.view, beta=1.0, scale=0.5)
        assert np.array_equal(out.get().view(np.uint32), first.view(np.uint32))          # two runs, the same bits
