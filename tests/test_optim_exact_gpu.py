"""GPU tests of the nine optimizer update kernels (include/bgan.h bg_sgd_f32 / bg_rmsprop_f32 / bg_adam_amsgrad_f32 /
bg_adam_f32), BIT FOR BIT against the float32 numpy statement of each rule (tests/optim_reference.py ref32), on every template
variant, at every size where the sweep's loops change shape, from non-zero slots, inside guarded buffers.

The library is built without fp contraction and with correctly rounded fp32 division and square root, so numpy float32
arithmetic written operation for operation IS the kernel's arithmetic.  Every case checks theta and every slot the variant
uses with np.array_equal on the int32 views, that the gradient is read only, that every guard float on either side of every
buffer is intact, and that the buffers of the slots a variant does not use, which are passed anyway, are left alone."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops

import optim_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64                  # floats: 256 bytes, so the view keeps the allocation's alignment
POISON = -7777.0
SEED = 11
NAMES = ("theta", "s1", "s2", "s3", "g")


class Guarded:
    """A device vector inside a poisoned buffer: what a kernel writes beyond the vector shows.  The view is 16-byte aligned."""

    def __init__(self, fill):
        self.n = n = fill.size
        self.buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        self.t.copy_(torch.from_numpy(fill))
        assert self.t.data_ptr() % 16 == 0

    def off_by_one(self):
        """The same length one float further on: not 16-byte aligned."""
        return self.buf[GUARD + 1:GUARD + 1 + self.n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == POISON).all()) and bool((self.buf[GUARD + self.n:] == POISON).all())

    def np(self):
        return self.t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def same_bits(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ; first at {i} (lane {i % 4}, last {int(bad[-1])}): "
                             f"got {got[i]!r} want {want[i]!r}")


def launch(kind, d, scalar, hp):
    """One update through blurred_gan_amd.ops; every slot buffer is passed, used or not."""
    th, s1, s2, s3, g = (d[k] for k in NAMES)
    if kind.startswith("sgd"):
        ops.sgd(th, s1, g, scalar, momentum=0.0 if kind == "sgd" else hp["mu"], nesterov=kind == "sgd_nesterov")
    elif kind.startswith("rmsprop"):
        ops.rmsprop(th, s1, s2, s3, g, scalar, rho=hp["rho"], momentum=hp["mu"] if "momentum" in kind else 0.0, eps=hp["eps"],
                    centered="centered" in kind)
    elif kind == "adam":
        ops.adam(th, s1, s2, g, scalar, hp["b1"], hp["b2"], hp["eps"])
    else:
        assert kind == "adam_amsgrad"
        ops.adam_amsgrad(th, s1, s2, s3, g, scalar, hp["b1"], hp["b2"], hp["eps"])


def update_and_check(kind, hp, x, scalars, what):
    """``len(scalars)`` updates from the inputs ``x`` on the device and in ref32, state carried on both sides; every check of the
    module's docstring.  Returns the device's outputs."""
    G = {k: Guarded(x[k]) for k in NAMES}
    want = R.args(x)[:4]
    for scalar in scalars:
        launch(kind, {k: v.t for k, v in G.items()}, scalar, hp)
        want = R.ref32(kind, *want, x["g"], scalar, hp)           # built once per case
    torch.cuda.synchronize()
    got = {k: G[k].np() for k in NAMES}
    for k, w, u in zip(NAMES[:4], want, (True,) + R.used(kind)):
        same_bits(got[k], w, f"{what} {k}" + ("" if u else " (a slot this variant does not use)"))
        assert u or (got[k] == R.SENTINEL).all()
    same_bits(got["g"], x["g"], f"{what} g (read only)")
    assert all(G[k].guards_intact() for k in NAMES), (what, [k for k in NAMES if not G[k].guards_intact()])
    return got


CASES = [(n, hp_name, kind) for n in sorted(set(R.SIZES_SWEEP) | set(R.SIZES_ADAM)) for hp_name in R.HP_MAIN for kind in R.KINDS
         if n in R.sizes(kind)]         # size slowest: the draws of a size are shared by every kind and hyper-parameter set
assert len(CASES) == 2 * (8 * len(R.SIZES_SWEEP) + len(R.SIZES_ADAM))


@pytest.mark.parametrize("n,hp_name,kind", CASES, ids=[f"{kind}-{hp_name}-{n}" for n, hp_name, kind in CASES])
def test_one_update_bit_for_bit(n, hp_name, kind):
    hp = R.HP_MAIN[hp_name]
    update_and_check(kind, hp, R.inputs(kind, n, SEED, hp), R.SCALARS[:1], f"{kind} {hp_name} n={n} ({R.sizes(kind)[n]})")


CHAINED = [(n, hp_name, kind) for kind in R.KINDS for n in ((R.BLOCK + R.QUAD + 2, R.FULL + R.QUAD + 1) if kind != "adam" else
                                                            (R.BLOCK_ADAM + 1, R.FULL_ADAM + 1)) for hp_name in R.HP_MAIN]
CHAINED.sort(key=lambda c: c[0])


@pytest.mark.parametrize("n,hp_name,kind", CHAINED, ids=[f"{kind}-{hp_name}-{n}" for n, hp_name, kind in CHAINED])
def test_two_chained_updates_bit_for_bit(n, hp_name, kind):
    """A second update with another scalar on the state the first one left, on the device and in the reference."""
    hp = R.HP_MAIN[hp_name]
    assert R.SCALARS[0] != R.SCALARS[1]
    update_and_check(kind, hp, R.inputs(kind, n, SEED + 1, hp), R.SCALARS, f"{kind} {hp_name} n={n}, two updates")


N_EDGE = R.BLOCK + R.QUAD + 2


@pytest.mark.parametrize("kind", R.KINDS)
def test_edge_hyper_parameters_and_a_zero_scalar(kind):
    """SGD momentum 1 and RMSprop rho 0, the ends the entry points accept.  With a scalar of 0.0 the slots move as ever; theta
    stays where it was bit for bit in every variant without a momentum slot (with one, theta moves by the slot: ref32)."""
    x = R.inputs(kind, N_EDGE, SEED + 2, R.HP_EDGE)
    update_and_check(kind, R.HP_EDGE, x, R.SCALARS[:1], f"{kind} edge")
    got = update_and_check(kind, R.HP_EDGE, x, (0.0,), f"{kind} edge, scalar 0")
    if "momentum" not in kind and kind != "sgd_nesterov":
        same_bits(got["theta"], x["theta"], f"{kind} edge, scalar 0: theta")
    if kind.startswith("rmsprop") or kind.startswith("adam"):
        assert (bits(got["s1"]) != bits(x["s1"])).mean() > 0.99          # the gradient still reaches the slots


@pytest.mark.parametrize("kind", R.KINDS)
def test_zero_gradients_and_zero_slots(kind):
    """n = 7: elements 1 and 3 of the quad and 4 and 6 of the tail have g = +0.0 or -0.0 and all-zero slots, next to ordinary
    elements.  Finite, equal to ref32, and theta does not move where nothing pushes it."""
    hp = R.HP_DEFAULT
    x = {k: v.copy() for k, v in R.inputs(kind, 7, SEED + 3, hp).items()}
    zero = np.array([1, 3, 4, 6])
    x["g"][zero] = np.float32([0.0, -0.0, 0.0, -0.0])
    assert np.signbit(x["g"][zero]).tolist() == [False, True, False, True]
    for k, u in zip(NAMES[1:4], R.used(kind)):
        if u:
            x[k][zero] = 0.0
    got = update_and_check(kind, hp, x, R.SCALARS[:1], f"{kind} zeros")
    assert all(np.isfinite(got[k]).all() for k in NAMES)
    same_bits(got["theta"][zero], x["theta"][zero], f"{kind} zeros: theta of the zero elements")
    assert (got["theta"][[0, 2, 5]] != x["theta"][[0, 2, 5]]).all()


N_ID = R.BLOCK + R.QUAD + 3


@pytest.mark.parametrize("hp_name", list(R.HP_MAIN))
def test_cross_kernel_identities(hp_name):
    hp = R.HP_MAIN[hp_name]
    # Adam-amsgrad's m and v are Adam's; its theta is Adam's on exactly the elements where the old vhat does not win the max
    x = R.inputs("adam_amsgrad", N_ID, SEED + 4, hp)
    ams = update_and_check("adam_amsgrad", hp, x, R.SCALARS[:1], "adam_amsgrad")
    adam = update_and_check("adam", hp, dict(x, s3=np.full(N_ID, R.SENTINEL, np.float32)), R.SCALARS[:1], "adam on amsgrad's inputs")
    same_bits(ams["s1"], adam["s1"], "m")
    same_bits(ams["s2"], adam["s2"], "v")
    v_wins = x["s3"] <= ams["s2"]
    assert 0.3 < v_wins.mean() < 0.7
    assert np.array_equal(bits(ams["theta"]) == bits(adam["theta"]), v_wins)
    # SGD with momentum and Nesterov keep the same a
    x = R.inputs("sgd_momentum", N_ID, SEED + 4, hp)
    plain, nest = (update_and_check(k, hp, x, R.SCALARS[:1], k) for k in ("sgd_momentum", "sgd_nesterov"))
    same_bits(plain["s1"], nest["s1"], "a")
    assert (bits(plain["theta"]) != bits(nest["theta"])).mean() > 0.9
    # centering does not change r (the non-centered kernels get the centered inputs, and leave mg alone)
    for mom in ("", "_momentum"):
        x = R.inputs("rmsprop_centered" + mom, N_ID, SEED + 4, hp)
        flat = dict(x, s3=np.full(N_ID, R.SENTINEL, np.float32))
        cen, non = update_and_check("rmsprop_centered" + mom, hp, x, R.SCALARS[:1], "centered"), update_and_check("rmsprop" + mom, hp, flat, R.SCALARS[:1], "flat")
        same_bits(cen["s1"], non["s1"], "r" + mom)
        assert (bits(cen["theta"]) != bits(non["theta"])).mean() > 0.9


def test_adam_takes_views_that_are_not_16_byte_aligned():
    """bg_adam_f32 is a scalar sweep and asks for no alignment: the same update one float off, bit for bit."""
    n, hp = R.BLOCK_ADAM + 1, R.HP_OTHER
    x = R.inputs("adam", n, SEED + 5, hp)
    G = {k: Guarded(x[k]) for k in ("theta", "s1", "s2", "g")}
    v = {k: g.off_by_one() for k, g in G.items()}
    for k in v:
        v[k].copy_(torch.from_numpy(x[k]))
        G[k].buf[GUARD] = POISON
    ops.adam(v["theta"], v["s1"], v["s2"], v["g"], R.SCALARS[0], hp["b1"], hp["b2"], hp["eps"])
    torch.cuda.synchronize()
    want = R.ref32("adam", *R.args(x), R.SCALARS[0], hp)
    for k, w in zip(("theta", "s1", "s2"), want):
        same_bits(v[k].cpu().numpy(), w, k)
    same_bits(v["g"].cpu().numpy(), x["g"], "g")
    for g in G.values():
        buf = g.buf.cpu().numpy()
        assert (buf[:GUARD + 1] == POISON).all() and (buf[GUARD + 1 + n:] == POISON).all()


# ------------------------------------------------------------------ refused calls
def _refusals(G):
    """(entry point, what, call) for every call that must be refused; ``m(k)`` is buffer k one float off alignment."""
    t = {k: g.t for k, g in G.items()}
    th, s1, s2, s3, g = (t[k] for k in NAMES)

    def m(k):
        return G[k].off_by_one()

    out = [("sgd", "a missing with momentum", lambda: ops.sgd(th, None, g, 0.1, momentum=0.9)),
           ("sgd", "a missing with Nesterov momentum", lambda: ops.sgd(th, None, g, 0.1, momentum=0.9, nesterov=True)),
           ("sgd", "momentum -0.1", lambda: ops.sgd(th, s1, g, 0.1, momentum=-0.1)),
           ("sgd", "momentum 1.5", lambda: ops.sgd(th, s1, g, 0.1, momentum=1.5)),
           ("sgd", "theta misaligned", lambda: ops.sgd(m("theta"), s1, g, 0.1, momentum=0.9)),
           ("sgd", "theta misaligned, no momentum", lambda: ops.sgd(m("theta"), None, g, 0.1)),
           ("sgd", "a misaligned", lambda: ops.sgd(th, m("s1"), g, 0.1, momentum=0.9)),
           ("sgd", "g misaligned", lambda: ops.sgd(th, s1, m("g"), 0.1, momentum=0.9)),
           ("sgd", "g misaligned, no momentum", lambda: ops.sgd(th, None, m("g"), 0.1)),
           ("rmsprop", "p missing with momentum", lambda: ops.rmsprop(th, s1, None, s3, g, 0.1, momentum=0.5, centered=True)),
           ("rmsprop", "mg missing when centered", lambda: ops.rmsprop(th, s1, s2, None, g, 0.1, momentum=0.5, centered=True)),
           ("rmsprop", "mg missing when centered, no momentum", lambda: ops.rmsprop(th, s1, None, None, g, 0.1, centered=True)),
           ("rmsprop", "momentum -0.1", lambda: ops.rmsprop(th, s1, s2, s3, g, 0.1, momentum=-0.1, centered=True))]
    for k in NAMES:
        a = [m(j) if j == k else t[j] for j in NAMES]
        out.append(("rmsprop", f"{k} misaligned", lambda a=a: ops.rmsprop(*a, 0.1, momentum=0.5, centered=True)))
        out.append(("adam_amsgrad", f"{k} misaligned", lambda a=a: ops.adam_amsgrad(*a, 0.1)))
    return out


def test_refused_calls_raise_and_launch_nothing():
    n = 64
    x = R.inputs("rmsprop_centered_momentum", n, SEED + 6, R.HP_DEFAULT)
    G = {k: Guarded(x[k]) for k in NAMES}
    before = {k: g.buf.clone() for k, g in G.items()}
    calls = _refusals(G)
    assert {c[0] for c in calls} == {"sgd", "rmsprop", "adam_amsgrad"} and len(calls) == 23
    for entry, what, call in calls:
        why = "aligned" if "misaligned" in what else "needs the" if "missing" in what else "momentum="
        with pytest.raises(ValueError, match=why):
            call()
        torch.cuda.synchronize()
        for k in NAMES:
            assert torch.equal(G[k].buf.view(torch.int32), before[k].view(torch.int32)), (entry, what, k)
    # and the same buffers are accepted once nothing is wrong with the call, so the refusals above were for the reason named
    ops.rmsprop(*(G[k].t for k in NAMES), 0.1, momentum=0.5, centered=True)
    torch.cuda.synchronize()
    assert not torch.equal(G["theta"].buf, before["theta"]) and all(g.guards_intact() for g in G.values())
