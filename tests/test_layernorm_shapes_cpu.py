"""What a critic step enqueues for the critic shapes of tests/ln_critics.py, without a GPU: one recorded step (the recorder of
tests/test_layernorm_cpu.py) per shape and D-step configuration -- when each slice of the flat gradient buffer goes to the reducer,
how often the LayerNormalization launches occur, which buffers the chunked route is given -- and, on the float64 reference alone,
the conditions under which tests/test_layernorm_shapes_gpu.py compares (no LeakyReLU pre-activation near zero, no small x-hat
gradient norm) for every seed it uses."""
import functools
import os

import numpy as np
import pytest
import torch

from blurred_gan_amd._lib import EPI_MUL_GRAD, EPI_NONE
from ln_reference import KINK, MIN_NORM
from test_layernorm_cpu import _Recorder, _grad_writes, maker, recording
import ln_critics as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = sorted(LC.SHAPES)
CONFIGS = sorted(LC.D_STEP_CONFIGS)
B = LC.B


# ------------------------------------------------------------------ 1. the reference's conditions, per seed
@pytest.mark.parametrize("name", SHAPES)
def test_net_seed_keeps_the_reference_off_the_kinks(name):
    _, (_, _, kink) = LC.net_case(name, LC.NET_SEED[name], device="cpu")
    print(name, kink)
    assert kink > KINK, kink


@pytest.mark.parametrize("name,std", [(n, None) for n in SHAPES] + [("ln_plain_ln", LC.BLUR_STD)])
def test_step_seed_keeps_the_reference_off_the_kinks_and_the_norms_up(name, std):
    seed = LC.STEP_SEED[name] if std is None else LC.BLUR_SEED
    *_, kink, norm = LC.step_reference(*LC.step_case(name, seed, device="cpu", std=std))
    print(name, std, kink, norm)
    assert kink > KINK, kink
    assert norm > MIN_NORM, norm


@pytest.mark.parametrize("name", sorted(LC.DP_CASES))
def test_data_parallel_seed_keeps_the_global_batch_reference_off_the_kinks(name):
    gan, reals, rnd = LC.dp_case(name, device="cpu")
    *_, kink, norm = LC.step_reference(gan, reals, rnd, gbs=reals.shape[0])
    print(name, kink, norm)
    assert kink > KINK, kink
    assert norm > MIN_NORM, norm


# ------------------------------------------------------------------ 2. recorded steps
class _Step:
    """One recorded critic step: its events up to the reducer's finish(), and the x-hat rows' view of the pass's buffers."""

    def __init__(self, name, config):
        maker.ensure_library(ROOT)
        rec = _Recorder()
        with recording(rec):
            gan, _, _ = LC.step_case(name, LC.STEP_SEED[name], device="cpu", step_replay=False, **LC.D_STEP_CONFIGS[config])
            gan.train_on_batch(np.zeros((B,) + LC.IMAGE, np.float32))
        self.D = D = gan.discriminator.net()
        LC.assert_claims(name, D)
        self.grad = D.store.grad
        self.ev = rec.events[:[n for n, _ in rec.events].index("finish") + 1]
        self.names = [n for n, _ in self.ev]
        self.ln = [i for i, st in enumerate(D.stages) if st.ln is not None]
        self.top = max(self.ln)
        assert self.ln == LC.LN_STAGES[name] and self.top == LC.TOP[name]
        self.handed = [(k, a) for k, (n, a) in enumerate(self.ev) if n == "ready"]
        self.first_source = self.names.index("layernorm.gp_source")
        self.last_source = len(self.names) - 1 - self.names[::-1].index("layernorm.gp_source")
        # the Dense head's hand-over ends the linearised forward: what follows is the source backward
        self.head = next(k for k, a in self.handed if a == D._train_range(D.stages[-1]))
        # the penalty's buffers: the x-hat rows of the merged pass, or the pass of their own
        if config == "unmerged":
            ctx = D.context(B, "hat")
            self.a, self.zdot = list(ctx.a), ctx.zdot
        else:
            ctx = D.context(3 * B, "fr3", drop_rows=2 * B)
            self.a, self.zdot = [t[2 * B:3 * B] for t in ctx.a], ctx._extra[("rowview_zdot", 2 * B, 3 * B)]

    def where(self, name, lo=0, hi=None, **match):
        """Indices of the launches ``name`` in events [lo, hi) whose arguments equal ``match``."""
        hi = len(self.ev) if hi is None else hi
        return [k for k in range(lo, hi) if self.names[k] == name and all(self.ev[k][1][m] == v for m, v in match.items())]

    def slot(self, layer, var):
        g = self.D.store.grad_of(layer, var)
        return g.storage_offset(), g.storage_offset() + g.numel()


step = functools.lru_cache(maxsize=None)(_Step)


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _overlap(a, b):
    (a0, a1), (b0, b1) = _span(a), _span(b)
    return a0 < b1 and b0 < a1


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", SHAPES)
def test_no_slice_goes_to_the_reducer_before_its_last_write(name, config):
    """The invariants of tests/test_layernorm_cpu.py's test of the same name, for every shape, and the plain stages' own rule."""
    s = step(name, config)
    D, ev, names, handed = s.D, s.ev, s.names, s.handed
    assert handed and names.index("finish") > handed[-1][0]
    for k, (lo, hi) in handed:
        late = [(names[j], w) for j in range(k + 1, len(ev)) if names[j] not in ("ready", "finish", "adam")
                for w in _grad_writes(ev[j][1], s.grad) if w[0] < hi and w[1] > lo]
        assert not late, f"[{lo}, {hi}) handed over at event {k}, written again by {late}"
    # each stage's slice is handed over exactly once
    assert sorted(a for _, a in handed) == sorted(D._train_range(st) for st in D.stages)
    assert s.last_source < s.head
    for i, st in enumerate(D.stages[:-1]):
        k = next(k for k, a in handed if a == D._train_range(st))
        kernel = s.slot(st.lin, "kernel")
        filt = [j for j in s.where("conv2d_bwd_filter") if kernel in _grad_writes(ev[j][1], s.grad)]
        if st.ln is not None:           # an LN stage: only behind the last source, from the source backward
            assert i <= s.top and k > s.last_source and k > s.head
        if i > s.top:                   # a plain stage above top: from the linearised forward, right behind its filter gradient
            assert s.last_source < k < s.head and filt[-1] == k - 1 and ev[k - 1][1]["beta"] == 1.0
            assert names[k + 1] == "conv2d_fwd" and ev[k + 1][1]["epi"].mode == EPI_MUL_GRAD
        else:                           # at or below top: from the source backward, behind the filter gradient it adds
            assert k > s.head
            added = [j for j in filt if s.head < j < k]
            assert len(added) == 1 and ev[added[0]][1]["beta"] == 1.0 and ev[added[0]][1]["scale"] == 1.0
            assert ev[added[0]][1]["dy"].shape[0] == B          # over the x-hat rows only
            if "bias" in st.lin.vars:
                bias = [j for j in s.where("colsum", s.head, k) if s.slot(st.lin, "bias") in _grad_writes(ev[j][1], s.grad)]
                assert len(bias) == 1 and ev[bias[0]][1]["beta"] == 1.0
    # the first-order backward keeps u for exactly the x-hat rows
    bwd = [a for n, a in ev[:s.first_source] if n == "layernorm.bwd" and a["u_out"] is not None]
    assert len(bwd) == len(s.ln) and all(a["u_out"].shape[0] == B for a in bwd)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", SHAPES)
def test_layernorm_launch_counts_and_the_source_backward_chain(name, config):
    s = step(name, config)
    D, ev, names = s.D, s.ev, s.names
    n_ln, below = len(s.ln), sum(i < s.top for i in s.ln)
    assert names.count("layernorm.tangent") == n_ln == names.count("layernorm.gp_source")
    assert [ev[k][1]["Cc"] for k in s.where("layernorm.gp_source")] == [D.stages[i].out_shape[-1] for i in s.ln]
    src_bwd = s.where("layernorm.bwd", s.head)
    assert names[s.last_source:].count("layernorm.bwd") == len(src_bwd) == below == {"ln_then_plain": 0, "plain_then_ln": 0,
                                                                                     "ln_plain_ln": 1, "three_ln_bare": 2}.get(name, 1)
    assert [ev[k][1]["Cc"] for k in src_bwd] == [D.stages[i].out_shape[-1] for i in reversed(s.ln) if i < s.top]
    for k in src_bwd:                   # the LN backward below top: accumulates, no Dropout on the x-hat rows, its own source added
        a = ev[k][1]
        assert a["addend"] is not None and a["keep"] is None and a["keep_elems"] == 0 and a["acc_beta"] == 1.0 and a["u_out"] is None
    # the data gradients of the source backward, top down: fused with LeakyReLU' into a plain stage (ref: its x-hat activations,
    # no mask), bare into an LN stage
    data = s.where("conv2d_bwd_data", s.head)
    assert len(data) == s.top
    for k, i in zip(data, range(s.top, 0, -1)):
        prev, epi = D.stages[i - 1], ev[k][1]["epi"]
        if prev.ln is None:
            _, ref, keep, _, _ = epi._hold
            assert epi.mode == EPI_MUL_GRAD and ref.data_ptr() == s.a[i - 1].data_ptr() and ref.shape == s.a[i - 1].shape
            assert keep is None and epi.keep_elems == 0 and epi.alpha == pytest.approx(prev.alpha) and epi.scale == 1.0
        else:
            assert epi.mode == EPI_NONE and epi._hold[1] is None
    assert not s.where("mul_grad", s.head)


@pytest.mark.parametrize("config", CONFIGS)
def test_stages_without_dropout_or_bias(config):
    """three_ln_bare: the Dropout-less LN stages give no mask -- and no keep_elems -- to the forward and the backward of the
    training passes; the stage with a Dropout does; nothing sums a bias for the bias-free conv."""
    s = step("three_ln_bare", config)
    D, ev = s.D, s.ev
    bare = [st.out_shape[-1] for st in D.stages if st.ln is not None and not st.drop]
    assert bare == [8, 16]
    for kind in ("layernorm.fwd", "layernorm.bwd"):
        for C in bare:
            calls = [ev[k][1] for k in s.where(kind, Cc=C)]
            assert calls and all(a["keep"] is None and a["keep_elems"] == 0 and a["scale"] == 1.0 for a in calls), (kind, C)
        masked = [ev[k][1] for k in s.where(kind, 0, s.first_source, Cc=12) if ev[k][1]["keep"] is not None]
        assert len(masked) == 1 and masked[0]["scale"] == pytest.approx(1 / 0.7), kind
        assert masked[0]["keep_elems"] == (0 if config == "unmerged" else 2 * B * 2 * 2 * 12)
    # the column sums of a step: the biases of stages 1 and 2 and of the head, and the head's kernel in the linearised forward
    targets = {s.slot(st.lin, "bias") for st in D.stages if "bias" in st.lin.vars} | {s.slot(D.stages[-1].lin, "kernel")}
    assert "bias" not in D.stages[0].lin.vars and len(targets) == 4
    sums = [w for k in s.where("colsum") for w in _grad_writes(ev[k][1], s.grad)]
    assert set(sums) == targets and not s.where("colsum", N=8)
    lo, hi = D._train_range(D.stages[0])
    assert hi - lo == 5 * 5 * 3 * 8 + 8 + 8


@pytest.mark.parametrize("config", CONFIGS)
def test_the_chunked_route_gets_buffers_of_its_own(config):
    """chunked: where a row exceeds what a wave holds in registers the kernels refuse dz aliasing g or addend, and vout aliasing
    zdot; the source backward writes the stage's tangent buffer instead, which nothing reads as a tangent any more."""
    s = step("chunked", config)
    ev, names = s.ev, s.names
    C = 257
    bwd = s.where("layernorm.bwd", Cc=C)
    assert len(bwd) == (3 if config == "unmerged" else 2)          # first order (fakes + reals; x-hat), then the source backward
    for k in bwd:
        a = ev[k][1]
        assert not _overlap(a["dz"], a["g"]) and (a["addend"] is None or not _overlap(a["dz"], a["addend"])), k
        assert not _overlap(a["dz"], a["z"])
    for k in s.where("layernorm.tangent", Cc=C):
        assert not _overlap(ev[k][1]["vout"], ev[k][1]["zdot"])
    # the source backward's write into ctx.zdot[0]
    w = bwd[-1]
    assert w > s.head and ev[w][1]["addend"] is not None
    zdot = s.zdot[0]
    assert ev[w][1]["dz"].data_ptr() == zdot.data_ptr() and ev[w][1]["dz"].numel() == zdot.numel() == B * 4 * 4 * C
    touches = lambda k: [m for m, v in ev[k][1].items() if isinstance(v, torch.Tensor) and v.numel() and _overlap(v, zdot)]
    # before it: the tangent conv wrote it, the tangent and the source read it -- all done
    before = [(names[k], touches(k)) for k in range(w) if names[k] not in ("ready", "finish") and touches(k)]
    assert before == [("conv2d_fwd", ["y"]), ("layernorm.tangent", ["zdot"]), ("layernorm.gp_source", ["zdot"])], before
    # behind it: only what consumes that call's output -- stage 0's filter gradient and bias sum
    after = [(names[k], touches(k)) for k in range(w + 1, len(ev)) if names[k] not in ("ready", "finish") and touches(k)]
    assert after == [("conv2d_bwd_filter", ["dy"]), ("colsum", ["x"])], after
    # the 8-channel stage above stays in place
    top = [ev[k][1] for k in s.where("layernorm.bwd", Cc=8)]
    assert top and all(a["dz"].data_ptr() == a["g"].data_ptr() for a in top)
