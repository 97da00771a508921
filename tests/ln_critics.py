"""Critic shapes with LayerNormalization stages beyond models.DCGANDiscriminator(normalization="layer") (a helper, not a test
file): data plus a builder.  The stock critic has LN on every conv, exactly two LN stages, a Dropout behind every LN, a bias on
every conv and channel counts on the float4 route with one chunk; each shape below leaves that in one direction, so that the
branches of engine.Net that the stock shape never takes run against the float64 reference (tests/test_layernorm_shapes_gpu.py),
in the launch recorder (tests/test_layernorm_shapes_cpu.py) and under data parallelism (tests/test_layernorm_dp_gpu.py).

Every shape is a layers.Sequential on the ``tiny`` generator's 8x8x3 images that ends in Flatten and Dense(1).  A stage is
(filters, kernel size, stride, LayerNormalization?, Dropout(0.3)?, bias?); every conv pads "same" and is followed by a LeakyReLU.

Two constraints hold for every shape and must survive a change: every per-sample activation size is a multiple of 4 floats (the
ctx.rows(lo, hi) slices handed to the convolutions stay 16-byte aligned at any batch), and no contraction Cin * k * k exceeds
400, ``tiny``'s own 16 * 25 (ln_reference.KINK was set at that contraction length)."""
import numpy as np
import torch

import blurred_gan_amd as bg
from blurred_gan_amd import layers, models, ops
from ln_reference import DT, make_gan, randomize, ref_forward, ref_params, ref_step_grads

ARCH = "tiny"
IMAGE = tuple(models.IMAGE_SHAPE[ARCH])        # (8, 8, 3)
B = 4
RATE = 0.3
MAX_CONTRACTION = 400

#            filters k  s  LN     Dr     bias
SHAPES = {
    # a plain stage between two LN stages: the source backward's fused data gradient (EPI_MUL_GRAD, ref = a[i-1]), no s_i there
    "ln_plain_ln": [(16, 5, 2, True, True, True), (16, 3, 1, False, False, True), (32, 3, 2, True, True, True)],
    # top == 0: the source backward's loop runs once and breaks; the plain stage above top hands its slice over itself
    "ln_then_plain": [(16, 5, 2, True, True, True), (32, 5, 2, False, True, True)],
    # a plain stage below top, with a Dropout of its own
    "plain_then_ln": [(16, 5, 2, False, True, True), (32, 5, 2, True, True, True)],
    # three LN stages; LN without Dropout; a conv without bias; C = 12, where three float4 units share four lanes
    "three_ln_bare": [(8, 5, 2, True, False, False), (16, 3, 1, True, False, True), (12, 3, 2, True, True, True)],
    # C % 4 != 0: the one-float route inside the engine, through the merged pass's row sub-ranges
    "scalar": [(5, 5, 2, True, True, True), (10, 3, 2, True, True, True)],
    # chunks > 1 below top: Net._input_grad's ctx.gin and gp_ln_source_backward's ctx.zdot[i-1]
    "chunked": [(257, 3, 2, True, True, True), (8, 1, 2, True, True, True)],
}

# what each shape claims of ops.layernorm.route, per LN stage index: the tests assert it first, so that a change of the route
# table cannot quietly turn a case into a copy of another
ROUTES = {
    "ln_plain_ln": {0: dict(vec=4, chunks=1), 2: dict(vec=4, chunks=1)},
    "ln_then_plain": {0: dict(vec=4, chunks=1)},
    "plain_then_ln": {1: dict(vec=4, chunks=1)},
    "three_ln_bare": {0: dict(vec=4, chunks=1), 1: dict(vec=4, chunks=1), 2: dict(vec=4, lanes=4, chunks=1)},
    "scalar": {0: dict(vec=1, chunks=1), 1: dict(vec=1, chunks=1)},
    "chunked": {0: dict(vec=1, chunks=5), 1: dict(vec=4, chunks=1)},
}

# the structure each shape claims of engine.Net: indices of the LN stages and of the top-most one
LN_STAGES = {name: [i for i, st in enumerate(stages) if st[3]] for name, stages in SHAPES.items()}
TOP = {name: max(idx) for name, idx in LN_STAGES.items()}


def build(name):
    """The critic of ``name``, unbuilt, as models.DCGANDiscriminator returns its own."""
    m = layers.Sequential()
    for i, (c, k, s, ln, drop, bias) in enumerate(SHAPES[name]):
        kw = dict(input_shape=list(IMAGE)) if i == 0 else {}
        m.add(layers.Conv2D(c, k, strides=s, padding="same", use_bias=bias, **kw))
        if ln:
            m.add(layers.LayerNormalization())
        m.add(layers.LeakyReLU())
        if drop:
            m.add(layers.Dropout(RATE))
    m.add(layers.Flatten())
    m.add(layers.Dense(1, activation="linear"))
    return m


def geometry(name):
    """[(H, W, Cin, Cout, k, stride)] of the shape's convs on their input side."""
    out, (H, W, C) = [], IMAGE
    for c, k, s, *_ in SHAPES[name]:
        out.append((H, W, C, c, k, s))
        H, W, C = -(-H // s), -(-W // s), c
    return out


def assert_claims(name, net=None):
    """The shape's constraints and its route claims; with ``net`` (engine.Net of the built critic) also its stage structure."""
    for (H, W, Cin, Cout, k, s) in geometry(name):
        assert Cin * k * k <= MAX_CONTRACTION, (name, Cin, k)
        assert (-(-H // s) * -(-W // s) * Cout) % 4 == 0, (name, H, W, Cout, s)
    assert sorted(ROUTES[name]) == LN_STAGES[name]
    for i, claim in ROUTES[name].items():
        route = ops.layernorm.route(SHAPES[name][i][0])
        assert {k: route[k] for k in claim} == claim, (name, i, route)
    if net is not None:
        stages = SHAPES[name]
        assert [st.kind for st in net.stages] == ["conv"] * len(stages) + ["dense"]
        for st, (c, k, s, ln, drop, bias) in zip(net.stages, stages):
            assert (st.out_shape[-1], st.lin.k, st.lin.stride) == (c, k, s)
            assert (st.ln is not None, bool(st.drop), "bias" in st.lin.vars, st.act) == (ln, drop, bias, "lrelu"), (name, c)
        assert net._gp_kinds() == ["ln" if st[3] else "conv" for st in stages] + ["dense"]


# ------------------------------------------------------------------ the cases: seeds, and the reference's side of each
# Every seed was chosen by running the float64 reference alone on a CPU (device="cpu"), so that no LeakyReLU pre-activation of any
# reference pass lies within ln_reference.KINK of zero and no x-hat gradient norm is below ln_reference.MIN_NORM; the minima the
# reference gave for seeds 1-5 stand beside each choice.  tests/test_layernorm_shapes_cpu.py re-asserts them without a GPU.
NET_SEED = {                    # min |LeakyReLU pre-activation|, seeds 1-5
    "ln_plain_ln": 3,           # 2.2e-4, 1.6e-4, 1.5e-3, 4.4e-4, 2.4e-4
    "ln_then_plain": 2,         # 6.0e-5, 3.5e-4, 3.0e-4, 2.5e-4, 5.1e-5
    "plain_then_ln": 3,         # 1.3e-6, 1.5e-4, 3.8e-4, 1.5e-4, 3.8e-4
    "three_ln_bare": 1,         # 1.2e-3, 2.4e-4, 1.0e-3, 4.8e-4, 3.5e-5
    "scalar": 1,                # 1.0e-2, 1.2e-3, 3.4e-3, 9.1e-3, 7.9e-3
    "chunked": 1,               # 1.7e-4, 5.3e-5, 9.3e-5, 8.4e-5, 4.6e-6
}
STEP_SEED = {                   # (min |LeakyReLU pre-activation| over all passes of the step, min x-hat gradient norm), seeds 1-5
    "ln_plain_ln": 4,           # (3.2e-6, 2.4), (1.6e-6, 1.8), (2.2e-5, 1.4), (2.5e-5, 2.2), (2.3e-6, 1.3)
    "ln_then_plain": 5,         # (3.4e-6, 1.2), (2.7e-6, 1.0), (1.1e-6, 0.85), (1.1e-5, 1.3), (2.6e-5, 0.81)
    "plain_then_ln": 4,         # (3.3e-6, 1.5), (2.8e-5, 1.5), (4.3e-7, 1.4), (4.6e-5, 1.8), (1.8e-6, 1.4)
    "three_ln_bare": 4,         # (6.4e-6, 4.0), (2.7e-6, 2.2), (7.2e-6, 2.4), (2.5e-5, 1.9), (5.8e-6, 2.3)
    "scalar": 3,                # (7.8e-6, 2.5), (9.9e-6, 2.2), (4.5e-5, 2.1), (1.3e-5, 3.6), (8.0e-6, 2.5)
    "chunked": 2,               # (1.2e-5, 1.3), (4.1e-5, 0.96), (2.6e-5, 2.6), (1.3e-5, 1.1), (2.1e-6, 1.3)
}
# ln_plain_ln behind the blur (std 0.9): (3.2e-6, 0.85), (1.6e-6, 0.93), (2.2e-5, 0.78), (2.5e-5, 1.3), (2.3e-6, 1.0)
BLUR_STD, BLUR_SEED = 0.9, 4
D_STEP_CONFIGS = {"merged": {}, "merged_separate_wgrad": dict(merge_gp_filter_gradients=False), "unmerged": dict(merge_critic_passes=False)}
# two data-parallel ranks of 3 against the single-process step at the global batch 6 (tests/test_layernorm_dp_gpu.py): "stock" is the
# ``tiny`` critic of models.DCGANDiscriminator(normalization="layer") behind the blur (std 0.9).  Both sides of that comparison
# are the HIP path; the seeds keep the reference of the global-batch step off the kinks all the same
DP_LOCAL, DP_WORLD = 3, 2
DP_CASES = {                    # name: (blur std, seed)
    "stock": (BLUR_STD, 1),     # (3.3e-5, 1.2), (2.1e-5, 1.1), (5.3e-6, 1.6), (1.5e-5, 1.5), (3.1e-5, 1.2)
    "ln_plain_ln": (None, 5),   # (2.5e-6, 2.5), (4.5e-6, 1.7), (7.3e-6, 1.7), (5.8e-6, 2.0), (1.2e-5, 1.4)
}
ALL_CONFIGS = ("ln_plain_ln", "chunked")           # the shapes that also run merged_separate_wgrad, the agreement and the replay


def net_case(name, seed, device=None):
    """The net-level case of tests/test_layernorm_step_gpu.py for shape ``name``: (model, x, Dropout masks, dout) and the float64
    reference's (output, [parameter gradients..., input gradient], min |LeakyReLU pre-activation|).  ``device``: where the model
    is built (``"cpu"``: reference-only use)."""
    bg.set_seed(seed)
    rng = np.random.default_rng(seed)
    model = build(name)
    x = rng.uniform(-1, 1, size=(B,) + IMAGE)
    if device is not None:
        model.build(device)
    randomize(model, rng)
    masks = [(rng.uniform(size=(B,) + tuple(s)) >= RATE).astype(np.uint8) for l, s in model.flat_layers() if l.kind == "dropout"]
    dout = rng.normal(size=(B,) + model.output_shape[1:])
    W, train = ref_params(model)
    xt = torch.as_tensor(x).to(DT).requires_grad_(True)
    pre = []
    y = ref_forward(model, W, xt, True, masks, pre)
    grads = torch.autograd.grad((y * torch.as_tensor(dout).to(DT)).sum(), train + [xt])
    return (model, x, masks, dout), (y.detach().numpy(), [g.numpy() for g in grads], min(pre))


def step_case(name, seed, device=None, Bs=B, gbs=None, std=None, **kw):
    """The whole-step case: (gan, reals, randomness) of ln_reference.make_gan with shape ``name`` as the critic (``"stock"``: the
    ``tiny`` critic of models.DCGANDiscriminator(normalization="layer")), global batch Bs + 1 unless ``gbs`` says otherwise."""
    disc = None if name == "stock" else (lambda: build(name))
    return make_gan(ARCH, Bs, seed, gbs=Bs + 1 if gbs is None else gbs, std=std, device=device, disc=disc, **kw)


def dp_case(name, device=None):
    """The global-batch case of DP_CASES[name]: (gan, reals, randomness) at batch = global batch = DP_LOCAL * DP_WORLD."""
    std, seed = DP_CASES[name]
    n = DP_LOCAL * DP_WORLD
    return step_case(name, seed, device=device, Bs=n, gbs=n, std=std)


def step_reference(gan, reals, rnd, gbs=None):
    """ln_reference.ref_step_grads of a step_case: (critic gradients, generator gradients, fakes, min |pre-activation|, min norm)."""
    return ref_step_grads(gan.generator, gan.discriminator, reals, rnd, gbs=reals.shape[0] + 1 if gbs is None else gbs)
