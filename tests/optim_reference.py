"""References, inputs and sizes for the bit-for-bit tests of the nine optimizer update kernels (csrc/optim.hip: three SGD
variants, four RMSprop variants, Adam-amsgrad; csrc/misc.hip: bg_adam_f32).  CPU only: numpy, no torch.cuda.

The library is compiled without fp contraction and with correctly rounded fp32 ``/`` and ``sqrtf``, so every update is a fixed
sequence of individually rounded fp32 operations.  ``ref32`` writes that sequence in numpy float32, one numpy operation per C
operation in the same association, and is what the kernels must equal BIT FOR BIT.  ``ref64`` states the same rules in float64
and shares no code with it; ``bound64`` is the first-order fp32 rounding bound between the two, which is what makes ``ref32``
trustworthy (tests/test_optim_reference_cpu.py) and what a kernel output behind a root or a division falls back to if the
device's root or division should not be the correctly rounded one.

Slot order (``s1, s2, s3``) by kind; a slot a kind does not use is returned unchanged:

    sgd                                     -
    sgd_momentum, sgd_nesterov              a
    rmsprop                                 r
    rmsprop_centered                        r, -, mg
    rmsprop_momentum                        r, p
    rmsprop_centered_momentum               r, p, mg
    adam                                    m, v
    adam_amsgrad                            m, v, vhat
"""
import functools

import numpy as np

KINDS = ("sgd", "sgd_momentum", "sgd_nesterov", "rmsprop", "rmsprop_centered", "rmsprop_momentum", "rmsprop_centered_momentum",
         "adam", "adam_amsgrad")
SWEEP_KINDS = tuple(k for k in KINDS if k != "adam")          # the eight float4 sweeps of optim.hip
SLOT_NAMES = {"sgd": (None, None, None), "sgd_momentum": ("a", None, None), "sgd_nesterov": ("a", None, None),
              "rmsprop": ("r", None, None), "rmsprop_centered": ("r", None, "mg"), "rmsprop_momentum": ("r", "p", None),
              "rmsprop_centered_momentum": ("r", "p", "mg"), "adam": ("m", "v", None), "adam_amsgrad": ("m", "v", "vhat")}
OUTPUTS = ("theta", "s1", "s2", "s3")


def used(kind):
    """Which of s1, s2, s3 the kind reads and writes."""
    return tuple(name is not None for name in SLOT_NAMES[kind])


HP_DEFAULT = dict(mu=0.9, rho=0.9, eps=1e-7, b1=0.9, b2=0.999)
HP_OTHER = dict(mu=0.5, rho=0.8, eps=1e-3, b1=0.0, b2=0.9)      # b1 = 0: this project's WGAN-GP Adam, m becomes g exactly
HP_EDGE = dict(mu=1.0, rho=0.0, eps=1e-7, b1=0.9, b2=0.999)     # the ends the entry points accept: SGD mu = 1, RMSprop rho = 0
HP_MAIN = {"default": HP_DEFAULT, "other": HP_OTHER}

SCALARS = (1e-2, 3e-3)            # the step scalar (lr, Adam: lr_t) of the first and of a chained second update
SENTINEL = np.float32(-12345.678)  # what the buffer of an unused slot holds

# ------------------------------------------------------------------ sizes
# bg::grid_cap(n, kT, per_thread) (csrc/common.h): min(ceil(n / (kT * per_thread)), 256 * 8) workgroups of kT = 256 threads.
THREADS = 256
MAX_GROUPS = 256 * 8
QUAD = 4                                  # floats a thread of the sweeps moves per trip (one float4)
BLOCK = THREADS * QUAD                    # floats one workgroup of a sweep covers per trip
FULL = MAX_GROUPS * THREADS * QUAD        # floats one trip of the capped grid covers: beyond it the grid-stride loop repeats

SIZES_SWEEP = {
    1: "only a tail (one element), no float4 body",
    2: "only a tail of two",
    3: "only a tail of three, the longest",
    QUAD: "first full quad, no tail",
    QUAD + 1: "one quad and a tail of one",
    QUAD + 2: "one quad and a tail of two",
    QUAD + 3: "one quad and a tail of three",
    BLOCK - 1: "last quad of the workgroup absent (255 quads), tail of three",
    BLOCK: "exactly one workgroup: every thread one quad, no tail",
    BLOCK + 1: "one full workgroup, tail of one; the grid grows to two and the second workgroup has no quad",
    BLOCK + QUAD + 2: "second workgroup with one quad, tail of two",
    FULL - 1: "capped grid one quad short of a full trip, tail of three",
    FULL: "exactly one full trip of the capped grid: no thread takes a second trip, no tail",
    FULL + QUAD + 1: "second grid-stride trip of one quad (one thread of workgroup 0), tail of one",
    FULL + BLOCK + 3: "second trip of exactly one whole workgroup, tail of three",
}

# adam_kernel (misc.hip, grid_for(n) = grid_cap(n, kT, 1)) is scalar: one float per thread per trip.
BLOCK_ADAM = THREADS
FULL_ADAM = MAX_GROUPS * THREADS          # tests/misc_cases.py ADAM_N's 524289 is FULL_ADAM + 1

SIZES_ADAM = {
    1: "one element: one live thread",
    BLOCK_ADAM - 1: "last thread of the only workgroup idle",
    BLOCK_ADAM: "exactly one workgroup",
    BLOCK_ADAM + 1: "second workgroup with one live thread",
    FULL_ADAM - 1: "capped grid, its last thread idle",
    FULL_ADAM: "exactly one full trip of the capped grid",
    FULL_ADAM + 1: "second grid-stride trip of one element",
}


def sizes(kind):
    return SIZES_ADAM if kind == "adam" else SIZES_SWEEP


# ------------------------------------------------------------------ references
def ref32(kind, theta, s1, s2, s3, g, scalar, hp):
    """One update in float32, operation for operation as the kernels write it (every intermediate rounded to fp32):
    ``a*b + c*d*e`` below is ((a*b) + ((c*d)*e)) in numpy as in C."""
    f = np.float32
    t, s1, s2, s3, g = (np.asarray(x) for x in (theta, s1, s2, s3, g))
    assert all(x.dtype == np.float32 for x in (t, s1, s2, s3, g))
    lr, one = f(scalar), f(1.0)
    if kind in ("sgd", "sgd_momentum", "sgd_nesterov"):
        mu = f(hp["mu"])
        if kind == "sgd":
            out = (t - lr * g, s1, s2, s3)
        else:
            a = mu * s1 - lr * g
            out = (t + (mu * a - lr * g) if kind == "sgd_nesterov" else t + a, a, s2, s3)      # Nesterov: the NEW a
    elif kind.startswith("rmsprop"):
        rho, mu, eps = f(hp["rho"]), f(hp["mu"]), f(hp["eps"])
        cen, mom = "centered" in kind, "momentum" in kind
        r = rho * s1 + (one - rho) * g * g
        d, mg, p = r, s3, s2
        if cen:
            mg = rho * s3 + (one - rho) * g
            d = r - mg * mg
        if mom:
            p = mu * s2 + lr * g / np.sqrt(d + eps)           # epsilon inside the root
            t = t - p
        else:
            t = t - lr * g / (np.sqrt(d) + eps)               # epsilon outside the root
        out = (t, r, p, mg)
    elif kind in ("adam", "adam_amsgrad"):
        b1, b2, eps = f(hp["b1"]), f(hp["b2"]), f(hp["eps"])
        m = b1 * s1 + (one - b1) * g
        v = b2 * s2 + (one - b2) * g * g
        if kind == "adam_amsgrad":
            vh = np.maximum(s3, v)
            out = (t - lr * m / (np.sqrt(vh) + eps), m, v, vh)
        else:
            out = (t - lr * m / (np.sqrt(v) + eps), m, v, s3)
    else:
        raise ValueError(kind)
    assert all(x.dtype == np.float32 for x in out), [x.dtype for x in out]
    return out


def _hp64(hp):
    return {k: float(np.float32(v)) for k, v in hp.items()}


def ref64(kind, theta, s1, s2, s3, g, scalar, hp):
    """The same rules in float64 (TF 2.5 keras/optimizer_v2); hyper-parameters and the scalar enter as the float32 values the
    kernels receive."""
    t, s1, s2, s3, g = (np.asarray(x, np.float64) for x in (theta, s1, s2, s3, g))
    h, lr = _hp64(hp), float(np.float32(scalar))
    if kind == "sgd":
        return t - lr * g, s1, s2, s3
    if kind in ("sgd_momentum", "sgd_nesterov"):
        a = h["mu"] * s1 - lr * g
        step = h["mu"] * a - lr * g if kind == "sgd_nesterov" else a
        return t + step, a, s2, s3
    if kind.startswith("rmsprop"):
        r = h["rho"] * s1 + (1.0 - h["rho"]) * np.square(g)
        dd = r
        if "centered" in kind:
            s3 = h["rho"] * s3 + (1.0 - h["rho"]) * g
            dd = r - np.square(s3)
        if "momentum" in kind:
            s2 = h["mu"] * s2 + lr * g / np.sqrt(dd + h["eps"])
            return t - s2, r, s2, s3
        return t - lr * g / (np.sqrt(dd) + h["eps"]), r, s2, s3
    if kind in ("adam", "adam_amsgrad"):
        m = h["b1"] * s1 + (1.0 - h["b1"]) * g
        v = h["b2"] * s2 + (1.0 - h["b2"]) * np.square(g)
        if kind == "adam_amsgrad":
            s3 = np.maximum(s3, v)
            return t - lr * m / (np.sqrt(s3) + h["eps"]), m, v, s3
        return t - lr * m / (np.sqrt(v) + h["eps"]), m, v, s3
    raise ValueError(kind)


# ------------------------------------------------------------------ rounding bound
U = 2.0 ** -24          # unit roundoff of fp32: one correctly rounded operation is off by at most U * |result|

COUNTS = {"a": 2, "theta sgd": 1, "theta sgd_momentum": 2, "theta sgd_nesterov": 4,
          "r": 4, "mg": 3, "d": 5, "theta rmsprop": 6, "p, theta rmsprop_momentum": 6.5,
          "theta rmsprop_centered": "2.5 * kappa + 4", "p, theta rmsprop_centered_momentum": "2.5 * kappa + 4.5",
          "m": 3, "v": 4, "vhat": 4, "theta adam, adam_amsgrad": 9}


def bound64(kind, inputs, scalar, hp):
    """Per-element first-order bound of |fp32 result - ref64| for every output: {"theta", "s1", "s2", "s3"} -> float64 array
    (zeros for a slot the kind leaves alone).  A slot's bound is c * 2^-24 * S with S the sum of the absolute values of the terms
    added and c the number of roundings on the longest path into it, one per fp32 operation; theta's is half a unit in the last
    place of max(|theta|, |theta'|), for the final subtraction, plus c * 2^-24 * S of its step.  Hyper-parameters are exact
    (ref64 takes their float32 values); ``1 - rho`` and ``1 - b`` are counted as a rounding although they are exact for values
    in [0.5, 1].  The counts (COUNTS):

      a      = mu*a - lr*g                     each product 1, the difference 1: c = 2, S_a = |mu a| + |lr g|
      theta  sgd: step lr*g, c = 1.  momentum: step a', c = 2, S_a.
             Nesterov: step mu*a' - lr*g: a' 2, the product 1, the difference 1: c = 4, S = mu S_a + |lr g|
      r      = rho*r + ((1-rho)*g)*g           1-rho 1, two products 2, the sum 1: c = 4, S_r = r' (all terms positive)
      mg     = rho*mg + (1-rho)*g              c = 3, S_mg = |rho mg| + |(1-rho) g|
      d      = r' - mg'*mg' (centered)         r' 4 or mg' 3 and the square 1, then the difference 1: c = 5,
             S_d = S_r + 2 |mg'| S_mg.  kappa = S_d / d is the cancellation factor of the difference, which ``inputs`` keeps
             small (d >= r'/2); without centering d = r', c = 4 and kappa = 1.  The relative error of d is c_d kappa U.
      theta  rmsprop: lr*g / (sqrt(d) + eps): d halved through the root c_d kappa / 2, the root 1, + eps 1, lr*g 1, the
             division 1: c = c_d kappa / 2 + 4 (6 without centering, 2.5 kappa + 4 with), S = |step|
      p      = mu*p + lr*g / sqrt(d + eps): d + eps adds 1 before the halving, so the quotient has c_d kappa / 2 + 3.5 and
             the sum 1 more: c = c_d kappa / 2 + 4.5 (6.5; 2.5 kappa + 4.5), S_p = |mu p| + |quotient|; theta's step is p'
      m      = b1*m + (1-b1)*g                 c = 3, S_m = |b1 m| + |(1-b1) g|
      v      = b2*v + ((1-b2)*g)*g             c = 4, S_v = v';   vhat = max(vhat, v'): exact, so v's c = 4 with S = vhat'
      theta  adam, amsgrad: lr*m' / (sqrt(v) + eps): m' 3 and lr*m' 1; v 4 halved through the root 2, the root 1, + eps 1;
             the division 1: c = 9, S = lr S_m / (sqrt(v) + eps)  (>= |step|; m' may cancel, its error does not)
    """
    th, s1, s2, s3, g = (np.asarray(inputs[k], np.float64) for k in ("theta", "s1", "s2", "s3", "g"))
    h, lr = _hp64(hp), float(np.float32(scalar))
    t2, n1, n2, n3 = ref64(kind, th, s1, s2, s3, g, scalar, hp)
    zero = np.zeros_like(th)
    half_ulp = 0.5 * np.spacing(np.maximum(np.abs(th), np.abs(t2)).astype(np.float32)).astype(np.float64)
    out = {"s1": zero, "s2": zero, "s3": zero}
    if kind == "sgd":
        step = 1 * U * np.abs(lr * g)
    elif kind in ("sgd_momentum", "sgd_nesterov"):
        S_a = np.abs(h["mu"] * s1) + np.abs(lr * g)
        out["s1"] = 2 * U * S_a
        step = 2 * U * S_a if kind == "sgd_momentum" else 4 * U * (h["mu"] * S_a + np.abs(lr * g))
    elif kind.startswith("rmsprop"):
        S_r = np.abs(h["rho"] * s1) + (1.0 - h["rho"]) * g * g
        out["s1"] = 4 * U * S_r
        c_d, kappa, d = 4.0, 1.0, n1
        if "centered" in kind:
            S_mg = np.abs(h["rho"] * s3) + np.abs((1.0 - h["rho"]) * g)
            out["s3"] = 3 * U * S_mg
            d = n1 - n3 * n3
            c_d, kappa = 5.0, (S_r + 2.0 * np.abs(n3) * S_mg) / d
        if "momentum" in kind:
            q = np.abs(lr * g) / np.sqrt(d + h["eps"])
            out["s2"] = step = (c_d * kappa / 2 + 4.5) * U * (np.abs(h["mu"] * s2) + q)
        else:
            step = (c_d * kappa / 2 + 4) * U * np.abs(lr * g) / (np.sqrt(d) + h["eps"])
    elif kind in ("adam", "adam_amsgrad"):
        S_m = np.abs(h["b1"] * s1) + np.abs((1.0 - h["b1"]) * g)
        out["s1"], out["s2"] = 3 * U * S_m, 4 * U * n2
        vv = n2
        if kind == "adam_amsgrad":
            out["s3"], vv = 4 * U * n3, n3
        step = 9 * U * lr * S_m / (np.sqrt(vv) + h["eps"])
    else:
        raise ValueError(kind)
    out["theta"] = half_ulp + step
    return out


# ------------------------------------------------------------------ inputs
_TINY = 2.0 ** -10        # |normal draw| is kept above this, so no product of the updates comes near the denormal range


@functools.lru_cache(maxsize=2)
def _draws(n, seed):
    """The random material of one (n, seed), shared by every kind and hyper-parameter set: read-only float64 arrays."""
    rng = np.random.default_rng([seed, n])

    def normal():
        z = rng.normal(size=n)
        return np.copysign(np.maximum(np.abs(z), _TINY), z)

    d = {"theta": normal(), "scale": 10.0 ** rng.integers(-2, 1, size=n), "zg": normal(), "z1": normal(), "z2": normal(),
         "w": rng.uniform(0.25, 4.0, size=n), "pick": rng.random(n) < 0.5}
    for x in d.values():
        x.setflags(write=False)
    return d


def inputs(kind, n, seed, hp):
    """float32 inputs of one update: {"theta", "s1", "s2", "s3", "g"}.  theta ~ N(0, 1); g ~ N(0, 1) * 10**k, k per element from
    {-2, -1, 0}; every slot the kind uses is non-zero and a slot it does not use holds SENTINEL.  Slots live on the scale a
    running optimizer would have them: momenta on the gradient's (``a``, ``p``: the step's), variances positive and on the
    squared gradient's.  Every value is a normal number far inside the fp32 range, and so is every intermediate of the update.

    Centered RMSprop: r = 4 mg'^2 + w (w > 0), so that with rho >= 0.5 the new d = r' - mg'^2 is at least half of r': no
    cancellation, no negative d.  (With rho = 0, HP_EDGE, r' = g^2 and mg' = g whatever the slots hold: d is exactly 0.)
    Amsgrad: vhat is half or twice the new v, per element, so both branches of the max occur (asserted for n >= 2)."""
    f = np.float32
    D = _draws(n, seed)
    scale = D["scale"]
    out = {"theta": f(D["theta"]), "g": f(D["zg"] * scale)}
    s = [np.full(n, SENTINEL, f) for _ in range(3)]
    g, one = out["g"], f(1.0)
    if kind in ("sgd_momentum", "sgd_nesterov"):
        s[0] = f(1e-2 * D["z1"] * scale)
    elif kind.startswith("rmsprop"):
        rho = f(hp["rho"])
        if "momentum" in kind:
            s[1] = f(1e-2 * D["z2"])
        if "centered" in kind:
            s[2] = f(0.5 * D["z1"] * scale)
            mg2 = rho * s[2] + (one - rho) * g
            s[0] = f(4.0) * mg2 * mg2 + f(D["w"] * scale * scale)
            if rho >= 0.5:
                r2 = rho * s[0] + (one - rho) * g * g
                assert (r2 - mg2 * mg2 >= f(0.5) * r2).all()
        else:
            s[0] = f(D["w"] * scale * scale)
    elif kind in ("adam", "adam_amsgrad"):
        s[0], s[1] = f(0.5 * D["z1"] * scale), f(D["w"] * scale * scale)
        if kind == "adam_amsgrad":
            b2 = f(hp["b2"])
            v2 = b2 * s[1] + (one - b2) * g * g
            s[2] = np.where(D["pick"], f(0.5), f(2.0)) * v2
            keep = s[2] > v2
            if n >= 2 and not (keep.any() and (~keep).any()):       # a draw all on one side: put one element on the other
                s[2][0] = (f(0.5) if keep[0] else f(2.0)) * v2[0]
                keep = s[2] > v2
            assert n < 2 or (keep.any() and (~keep).any())
    elif kind != "sgd":
        raise ValueError(kind)
    out.update(s1=s[0], s2=s[1], s3=s[2])
    for k, x in out.items():
        assert x.dtype == np.float32 and x.shape == (n,), k
        assert (np.abs(x) >= 2.0 ** -40).all() and (np.abs(x) <= 2.0 ** 40).all(), k       # normal, nowhere near either end
    for i, u in enumerate(used(kind)):
        assert not u or (s[i] != SENTINEL).all()
        assert u or (s[i] == SENTINEL).all()
    assert all((out[k] > 0).all() for k, name in zip(("s1", "s2", "s3"), SLOT_NAMES[kind]) if name in ("r", "v", "vhat"))
    return out


def args(x):
    """The positional arrays of ref32 / ref64 from an ``inputs`` dictionary."""
    return x["theta"], x["s1"], x["s2"], x["s3"], x["g"]
