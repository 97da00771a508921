"""CPU tests of tests/optim_reference.py, which the bit-for-bit GPU tests of the optimizer kernels (test_optim_exact_gpu.py)
stand on: the float32 statement of every update lies within the derived rounding bound of the independent float64 statement,
the drawn inputs tell apart the mistakes the GPU test exists to catch, and the size lists reach every shape of the loops."""
import numpy as np
import pytest

import optim_reference as R

N = 20011
SEEDS = (0, 1, 2)


@pytest.mark.parametrize("hp_name", list(R.HP_MAIN))
@pytest.mark.parametrize("kind", R.KINDS)
def test_ref32_lies_within_the_rounding_bound_of_ref64(kind, hp_name):
    hp, worst = R.HP_MAIN[hp_name], {}
    for seed in SEEDS:
        for scalar in R.SCALARS:
            x = R.inputs(kind, N, seed, hp)
            got, want, bound = R.ref32(kind, *R.args(x), scalar, hp), R.ref64(kind, *R.args(x), scalar, hp), R.bound64(kind, x, scalar, hp)
            for name, a, b, u in zip(R.OUTPUTS, got, want, (True,) + R.used(kind)):
                if not u:
                    assert a is x[name] and (bound[name] == 0).all()        # returned unchanged
                    continue
                assert a.dtype == np.float32 and b.dtype == np.float64 and (bound[name] > 0).all()
                ratio = float((np.abs(a.astype(np.float64) - b) / bound[name]).max())
                worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"ref32 vs ref64, worst error / bound, {kind} {hp_name}:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    exact = {"s1"} if kind.startswith("adam") and hp["b1"] == 0.0 else set()                   # b1 = 0: m is g, no rounding at all
    assert all((v == 0.0) if k in exact else (v > 0.1) for k, v in worst.items()), worst       # a rounding bound, not a loose tolerance


def _differs(kind, hp, wrong, output, seed=0, scalar=R.SCALARS[0]):
    """Fraction of the elements on which a mistaken float32 update differs from ref32 in ``output``."""
    x = R.inputs(kind, N, seed, hp)
    want = R.ref32(kind, *R.args(x), scalar, hp)[R.OUTPUTS.index(output)]
    got = wrong(*R.args(x), np.float32(scalar), {k: np.float32(v) for k, v in hp.items()})
    assert got.dtype == np.float32
    return float((got.view(np.int32) != want.view(np.int32)).mean())


ONE = np.float32(1.0)


def _d(r, mg, g, h, centered):
    r = h["rho"] * r + (ONE - h["rho"]) * g * g
    if not centered:
        return r
    mg = h["rho"] * mg + (ONE - h["rho"]) * g
    return r - mg * mg


@pytest.mark.parametrize("hp_name", list(R.HP_MAIN))
def test_inputs_tell_the_mistakes_apart(hp_name):
    hp = R.HP_MAIN[hp_name]
    frac = {}
    # epsilon on the wrong side of the root, both directions: without momentum only theta lies behind the root, with it p too
    for cen in (False, True):
        k = "rmsprop_centered" if cen else "rmsprop"
        frac[k, "eps inside"] = _differs(k, hp, lambda t, r, p, mg, g, lr, h, cen=cen: t - lr * g / np.sqrt(_d(r, mg, g, h, cen) + h["eps"]), "theta")
        k += "_momentum"
        frac[k, "eps outside"] = _differs(k, hp, lambda t, r, p, mg, g, lr, h, cen=cen: h["mu"] * p + lr * g / (np.sqrt(_d(r, mg, g, h, cen)) + h["eps"]), "s2")
    frac["sgd_nesterov", "old a"] = _differs("sgd_nesterov", hp, lambda t, a, _2, _3, g, lr, h: t + (h["mu"] * a - lr * g), "theta")
    frac["adam_amsgrad", "vhat = v"] = _differs("adam_amsgrad", hp, lambda t, m, v, vh, g, lr, h: h["b2"] * v + (ONE - h["b2"]) * g * g, "s3")
    frac["rmsprop_centered", "no - mg^2"] = _differs("rmsprop_centered", hp, lambda t, r, p, mg, g, lr, h: t - lr * g / (np.sqrt(_d(r, mg, g, h, False)) + h["eps"]), "theta")
    frac["rmsprop_centered_momentum", "no - mg^2"] = _differs(
        "rmsprop_centered_momentum", hp, lambda t, r, p, mg, g, lr, h: h["mu"] * p + lr * g / np.sqrt(_d(r, mg, g, h, False) + h["eps"]), "s2")
    # The association of (1 - rho) * g * g moves the last place of the smaller of the two terms of r, which survives the sum
    # on a few elements in a hundred: measured 2.2 % (default) and 3.9 % (other) for RMSprop's r, so the variant stays, held
    # to its own threshold of 1 %.  For Adam's v it is 2.2 % with b2 = 0.9 and below 1 % (none in 20011) with b2 = 0.999, where
    # the term is a thousandth of v: that one is dropped.
    assoc = {("rmsprop", "(1-rho)*(g*g)"): _differs("rmsprop", hp, lambda t, r, p, mg, g, lr, h: h["rho"] * r + (ONE - h["rho"]) * (g * g), "s1")}
    if hp["b2"] < 0.99:
        assoc["adam", "(1-b2)*(g*g)"] = _differs("adam", hp, lambda t, m, v, _3, g, lr, h: h["b2"] * v + (ONE - h["b2"]) * (g * g), "s2")
    print(f"fraction of elements that differ from ref32, {hp_name}:", {" / ".join(k): round(v, 3) for k, v in {**frac, **assoc}.items()})
    for key, v in frac.items():
        assert v > 0.10, (key, v)
    for key, v in assoc.items():
        assert v > 0.01, (key, v)


def test_size_lists_reach_every_loop_shape():
    s = sorted(R.SIZES_SWEEP)
    assert R.BLOCK == 256 * 4 and R.FULL == 2048 * 256 * 4 and R.QUAD == 4
    assert s == sorted([1, 2, 3, 4, 5, 6, 7, R.BLOCK - 1, R.BLOCK, R.BLOCK + 1, R.BLOCK + 4 + 2, R.FULL - 1, R.FULL, R.FULL + 4 + 1,
                        R.FULL + R.BLOCK + 3])
    assert {n % R.QUAD for n in s} == {0, 1, 2, 3}
    assert {n for n in s if n < R.QUAD} == {1, 2, 3}                                # no float4 body at all, every tail
    assert {n % R.QUAD for n in s if n > R.FULL} == {1, 3} and {n % R.QUAD for n in s if R.QUAD < n < R.BLOCK} == {1, 2, 3}
    for edge in (R.BLOCK, R.FULL):
        assert edge in s and any(n < edge and edge - n < R.QUAD for n in s) and any(n > edge and n - edge <= R.QUAD + 2 for n in s)
    assert max(s) < R.FULL + 2 * R.BLOCK                                            # nothing larger than the loops need
    a = sorted(R.SIZES_ADAM)
    assert R.BLOCK_ADAM == 256 and R.FULL_ADAM == 2048 * 256
    assert a == [1, R.BLOCK_ADAM - 1, R.BLOCK_ADAM, R.BLOCK_ADAM + 1, R.FULL_ADAM - 1, R.FULL_ADAM, R.FULL_ADAM + 1]
    assert all(isinstance(why, str) and why for why in list(R.SIZES_SWEEP.values()) + list(R.SIZES_ADAM.values()))
    assert R.sizes("adam") is R.SIZES_ADAM and all(R.sizes(k) is R.SIZES_SWEEP for k in R.SWEEP_KINDS)
    assert len(R.KINDS) == 9 and len(R.SWEEP_KINDS) == 8


def test_inputs_are_as_the_gpu_test_needs_them():
    for hp in R.HP_MAIN.values():
        for kind in R.KINDS:
            x = R.inputs(kind, 1031, 5, hp)
            y = R.inputs(kind, 1031, 5, hp)
            assert all(np.array_equal(x[k], y[k]) for k in x)                        # a function of its arguments
            new = R.ref32(kind, *R.args(x), R.SCALARS[0], hp)
            assert all(np.isfinite(a).all() for a in new)
            for name, u, a in zip(("s1", "s2", "s3"), R.used(kind), new[1:]):
                assert u == bool((a != R.SENTINEL).any())
            if "centered" in kind:
                d = new[1].astype(np.float64) - new[3].astype(np.float64) ** 2
                assert (d >= 0.499 * new[1]).all()
            if kind == "adam_amsgrad":
                grew = new[3] != x["s3"]
                assert 0.3 < grew.mean() < 0.7 and np.array_equal(new[3][grew], new[2][grew])
    assert set(np.log10(np.abs(R._draws(1031, 5)["scale"])).round().astype(int)) == {-2, -1, 0}
    x = R.inputs("rmsprop_centered", 9, 1, R.HP_EDGE)                                # rho = 0: d is exactly 0, the step is finite
    new = R.ref32("rmsprop_centered", *R.args(x), R.SCALARS[0], R.HP_EDGE)
    assert np.array_equal(new[1], new[3] * new[3]) and np.isfinite(new[0]).all()
