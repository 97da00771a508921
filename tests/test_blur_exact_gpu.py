"""GPU: every blur kernel route of csrc/blur.hip and csrc/blur_panel.hip on exact integer data with asymmetric taps
(tests/blur_cases.py; tests/test_blur_cases_cpu.py proves every case exact in float32 and on its claimed route on the CPU).

Every comparison is array_equal against the float64 reference.  x, y and the scratch image are 16-byte-aligned views inside larger
buffers whose guard bands hold a finite sentinel and must stay bit-unchanged; y and the scratch image start out as NaN, so an element
that is never written shows; the scratch image is exactly bg_blur_workspace_bytes long.  The launch names recorded by the profiler
must be the claimed family's.  A failing impulse case decodes its first wrong output into tap indices (blur_cases.decode).

Not asserted: the footprint of a single non-finite pixel inside its own image -- the Toeplitz kernels multiply it by out-of-band zeros,
so it reaches further than the tap window.  What is asserted is that a non-finite IMAGE stays inside itself.
"""
import numpy as np
import pytest
import torch

import blur_cases as BC

pytestmark = pytest.mark.gpu

PAD = 256                     # floats of guard band on either side (1 KB)
SENTINEL = -98765.0
IDS = [BC.case_id(c) for c in BC.CASES]


class Guarded:
    """n floats at a 16-byte boundary inside a buffer whose bands on either side hold SENTINEL."""

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda")
        self.view = self.buf[PAD:PAD + n]
        assert self.view.data_ptr() % 16 == 0
        if init is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).ravel()))

    def guards_intact(self):
        b = self.buf.cpu().numpy().view(np.uint32)
        s = np.float32(SENTINEL).view(np.uint32)
        return bool((b[:PAD] == s).all() and (b[PAD + self.n:] == s).all())

    def get(self, shape):
        return self.view.cpu().numpy().reshape(shape)


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


def run(x, t, profile=True):
    """bg_blur_nhwc_f32 on guarded buffers -> (y as float32 numpy, launch names); the guards and the input are checked here."""
    from blurred_gan_amd import ops
    B, H, W, C = x.shape
    T = len(t)
    gx, gy = Guarded(x.size, x), Guarded(x.size)
    nb = ops.blur_workspace_bytes(B, H, W, C, T)
    assert nb in (0, x.size * 4)
    gt = Guarded(nb // 4) if nb else None
    taps = torch.from_numpy(np.asarray(t, np.float32)).cuda()
    call = lambda: ops.blur_nhwc(gx.view.view(B, H, W, C), gy.view.view(B, H, W, C), taps, T, gt.view if gt else None)
    if profile:
        names = launches(call)
    else:
        call()
        torch.cuda.synchronize()
        names = None
    assert gx.guards_intact() and gy.guards_intact() and (gt is None or gt.guards_intact()), "a guard band was written"
    assert np.array_equal(gx.get(x.shape).view(np.uint32), x.astype(np.float32).view(np.uint32)), "the input was written"
    return gy.get(x.shape), names


def set_env(monkeypatch, env):
    for k in BC.CALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", BC.CASES, ids=IDS)
def test_exact_on_its_route(case, monkeypatch):
    shape, T, family, _, env = case
    set_env(monkeypatch, env)
    for recipe in BC.recipes(case):
        x, t = BC.make(case, recipe)
        ref = BC.reference(x, t)
        y, names = run(x, t)
        assert names == BC.NAMES[family], (recipe, names)
        if not np.array_equal(y.astype(np.float64), ref):
            n_nan = int(np.isnan(y).sum())
            detail = BC.decode(x, t, y, ref) if recipe == "impulse" else \
                f"{int((y.astype(np.float64) != ref).sum())} of {ref.size} wrong, first at {np.argwhere(y.astype(np.float64) != ref)[0].tolist()}"
            pytest.fail(f"{BC.case_id(case)} [{recipe}]: {n_nan} outputs never written; {detail}")


@pytest.mark.parametrize("case3", BC.CASES3, ids=lambda c: "x".join(map(str, c)))
def test_three_sources_exact(case3):
    from blurred_gan_amd import ops
    B, H, W, C, T = case3
    assert ops.blur3_lerp_supported(B, H, W, C, T)
    f, r, a, t = BC.make3(case3)
    ref = BC.reference3(f, r, a, t)
    gf, gr, ga, gy = Guarded(f.size, f), Guarded(r.size, r), Guarded(4 * ((B + 3) // 4), np.resize(a, 4 * ((B + 3) // 4))), Guarded(3 * f.size)
    taps = torch.from_numpy(t.astype(np.float32)).cuda()
    names = launches(lambda: ops.blur3_lerp(gf.view.view(B, H, W, C), gr.view.view(B, H, W, C), ga.view[:B], gy.view.view(3 * B, H, W, C), taps, T))
    assert names == BC.NAMES["rows3"]
    assert gf.guards_intact() and gr.guards_intact() and ga.guards_intact() and gy.guards_intact()
    y = gy.get(ref.shape).astype(np.float64)
    for i, group in enumerate(("f", "r", "x-hat")):
        assert np.array_equal(y[i * B:(i + 1) * B], ref[i * B:(i + 1) * B]), \
            f"group {group}: {int((y[i * B:(i + 1) * B] != ref[i * B:(i + 1) * B]).sum())} wrong, {int(np.isnan(y[i * B:(i + 1) * B]).sum())} never written"


def _family_case(key):
    found = [c for c in BC.CASES if (c[0], c[1], c[4]) == key]
    assert len(found) == 1, key
    return found[0]


FAMILY_CASES = [_family_case(k) for k in BC.PER_FAMILY]
FAMILY_IDS = [BC.case_id(c) for c in FAMILY_CASES]


@pytest.mark.parametrize("case", FAMILY_CASES, ids=FAMILY_IDS)
def test_a_nan_image_stays_inside_itself(case, monkeypatch):
    """One image of the batch is NaN throughout: every other image equals its reference, and the NaN image's output is NaN
    everywhere (the dense taps have no zeros, so every output touches an in-image NaN)."""
    set_env(monkeypatch, case[4])
    shape, T = case[0], case[1]
    x, t = BC.make(case, "dense", seed=1)
    ref = BC.reference(x, t)
    k = shape[0] // 2
    x[k] = np.nan
    y, _ = run(x, t, profile=False)
    assert np.isnan(y[k]).all(), f"{int((~np.isnan(y[k])).sum())} outputs of the NaN image are numbers"
    for b in range(shape[0]):
        if b != k:
            assert np.array_equal(y[b].astype(np.float64), ref[b]), f"image {b} (NaN image is {k}): {int((y[b].astype(np.float64) != ref[b]).sum())} wrong"


@pytest.mark.parametrize("case", FAMILY_CASES, ids=FAMILY_IDS)
def test_two_runs_are_bit_identical(case, monkeypatch):
    set_env(monkeypatch, case[4])
    x, t = BC.make(case, "dense", seed=2)
    y1, _ = run(x, t, profile=False)
    y2, _ = run(x, t, profile=False)
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))
    assert np.array_equal(y1.astype(np.float64), BC.reference(x, t))


def test_families_of_the_per_family_tests():
    assert sorted({c[2] for c in FAMILY_CASES}) == sorted(set(BC.NAMES) - {"rows3"})
    assert {BC.described(c)["k16"] for c in FAMILY_CASES if c[2] == "panel"} == {True, False}       # the 16-row and the 32-row kernel
    assert all(c[0][0] >= 2 for c in FAMILY_CASES)                 # isolation needs a second image
