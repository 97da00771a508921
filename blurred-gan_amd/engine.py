"""Executor: compiles a flattened layer list into fused stages and runs forward / backward / the
gradient-penalty linearised forward on the HIP kernels.  There is no tape: every backward formula is
written out (SURVEY.md 8a, rows T1-T8 and the GP second-order derivation).

A stage = one linear op (Dense | Conv2D | Conv2DTranspose) [+ bias] [+ BatchNormalization | LayerNormalization | NoiseInjection]
[+ LeakyReLU | tanh] [+ Dropout | PixelNormalization]; Reshape / Flatten are views.  UpSampling2D / AveragePooling2D are stages of their own: linear, parameter-free,
one launch each way (bg_upsample2x_nhwc_f32 / bg_pool2x_sum_nhwc_f32, each the other's transpose), and so are their FIR-filtered
counterparts FilteredUpSampling2D / FilteredDownSampling2D (bg_fir_upsample2x_nhwc_f32 / bg_fir_downsample2x_nhwc_f32 with the taps
flipped for the transpose).  MinibatchStdDev is a stage of its
own too (csrc/mbstd.hip; one launch each way, one more for the penalty's tangent and source).  Stage fusion on the device:
  conv (+bias) + LeakyReLU + Dropout      -> one launch (epilogue of the MFMA kernel)
  dgrad + LeakyReLU'/Dropout' of the stage below -> one launch (BG_EPI_MUL_GRAD epilogue)
  pooling backward + LeakyReLU'/Dropout' of the stage below -> one launch (the upsample with ref / keep)
  BatchNormalization + LeakyReLU          -> stats pass + one apply pass
  LayerNormalization + LeakyReLU + Dropout -> one pass over the conv's stored output (per-pixel statistics, csrc/layernorm.hip)
  LeakyReLU + PixelNormalization          -> one pass over the linear op's stored output (csrc/pixelnorm.hip); a PixelNormalization
                                             that is the network's first layer normalises the latents, one launch, no backward
  NoiseInjection + LeakyReLU              -> one in-place pass over the conv's stored output (csrc/noise.hip), in front of the
                                             PixelNormalization pass where the stage has one; all noise maps of a pass are one draw
  MappingNetwork (not a stage)            -> one launch per layer in front of the first stage: Dense + bias + LeakyReLU in the
                                             epilogue (csrc/mapping.hip); its output is the first Dense's input and the style source

Net.forward and Net.backward are input / pass set-up, a loop over the stages, and one helper per concern (DESIGN.md §5
"Engine map"); tests/test_engine_trace_cpu.py holds the order and the arguments of everything they enqueue.
"""
from __future__ import annotations

import functools
import os
from typing import List, Optional

import numpy as np
import torch

from . import dist, ops
from ._lib import EPI_NONE, EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_TANH, EPI_AFFINE_LRELU
from .layers import MAPPING_RULE, MOD_RULE, EqualizedLearningRate, SpectralNormalization, StyleModulation


RESAMPLE = ("upsample", "avgpool", "firup", "firdown")      # "fir*": the FIR-filtered pair (layers.Filtered*Sampling2D)
UPSAMPLERS = ("upsample", "firup")          # their backward is a down-sampler: nothing to fuse a LeakyReLU' into
PARAMETER_FREE = RESAMPLE + ("mbstd",)      # stages of their own without variables (layers.MinibatchStdDev: not linear, see mbstd_*)
SOURCE_KINDS = ("ln", "mbstd")              # _gp_kinds: stages that are not piecewise linear and add a source term to the penalty


class Stage:
    def __init__(self, lin, in_shape):
        self.lin = lin
        self.kind = lin.kind
        self.in_shape = tuple(in_shape)
        self.out_shape = tuple(lin.out_shape(in_shape))
        self.bn = None
        self.ln = None              # layers.LayerNormalization between a Conv2D and its LeakyReLU (the critic's normalisation)
        self.pn = None              # layers.PixelNormalization directly behind the stage's LeakyReLU (the generator's normalisation)
        self.pn_channels = None     # the C it normalises over: the last axis of the map at the layer (a Dense's, behind its Reshape)
        self.noise = None           # layers.NoiseInjection directly behind the stage's Conv2D / Conv2DTranspose (the generator's noise input)
        self.mod = lin if isinstance(lin, StyleModulation) else None      # layers.StyleModulation: the stage's conv is modulated by the styles
        self.act = getattr(lin, "activation", None)
        self.alpha = 1.0
        self.drop = None
        self.mask_index = None      # which of the pass's Dropout masks is this stage's (forward(masks=...))
        # inference BatchNorm behind a bias-free conv (the generator inside the D-step) is folded into the conv's epilogue: no z,
        # no BatchNorm pass (set once the stage is complete)
        self.folds_inference_bn = False
        # conv stages: (H, W, Cin, Cout, k, stride) on the conv-INPUT side.  A Conv2DTranspose is the data gradient of the conv
        # whose input side is this layer's output, with the same kernel array
        self.geom = None
        if self.kind == "conv":
            self.geom = (*self.in_shape, lin.filters, lin.k, lin.stride)
        elif self.kind == "convT":
            self.geom = (*self.out_shape[:2], lin.filters, self.in_shape[2], lin.k, lin.stride)

    @property
    def fusable_grad(self):
        return self.bn is None and self.ln is None and self.pn is None and self.act == "lrelu"

    @property
    def drop_scale(self):
        return 1.0 / (1.0 - self.drop) if self.drop else 1.0

    def bn_args(self):
        """The BatchNorm's parameters as the keywords every ops.bn_* function names them by (in bn_fold's positional order)."""
        v = self.bn.vars
        return dict(gamma=v["gamma"], beta=v["beta"], moving_mean=v["moving_mean"], moving_var=v["moving_variance"], eps=self.bn.epsilon)

    @property
    def ln_pixels(self):
        """Rows of an LN stage's [R, C] view per sample: its map's pixels."""
        return int(np.prod(self.out_shape[:-1]))

    @property
    def mod_pixels(self):
        """(P_in, P_out) of a modulated stage: the pixels per sample of its input and of its output map."""
        return int(np.prod(self.in_shape[:-1])), int(np.prod(self.out_shape[:-1]))

    @property
    def noise_pixels(self):
        """Noise values of a NoiseInjection stage per sample: its map's pixels."""
        return int(np.prod(self.out_shape[:-1]))

    @property
    def pn_rows(self):
        """Rows of a PixelNormalization stage's [R, C] view per sample."""
        return int(np.prod(self.out_shape)) // self.pn_channels


class _StageBuffers:
    def buf(self, lst, i):
        if lst[i] is None:
            lst[i] = torch.empty((self.B,) + self._net.stages[i].out_shape, dtype=torch.float32, device=self._device)
        return lst[i]

    def mbstd_source(self, i):
        """(src, fdot) of MinibatchStdDev stage i: the penalty's source at the stage's primal input (kept in s[i]) and the groups'
        tangent scalar."""
        st = self._net.stages[i]
        if self.s[i] is None:
            self.s[i] = torch.empty((self.B,) + st.in_shape, dtype=torch.float32, device=self._device)
        return self.s[i], self.mbstd_stats(i)[4]


class Context(_StageBuffers):
    """Activation / gradient buffers of one pass at a fixed batch size (caller-owned HBM)."""

    def __init__(self, net, B, device, drop_rows=None):
        self.B = B
        # Dropout applies to the first ``drop_rows`` samples of the batch only (default: all).  The critic step runs
        # [fakes; reals] (training=True) and x-hat (training=False) through ONE pass: 2B rows with masks, B without.
        self.drop_rows = B if drop_rows is None else int(drop_rows)
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
        self.a0 = f(B, *net.in_shape)
        self.din = None
        self.a, self.z, self.keep, self.mean, self.inv, self.dz, self.v = [], [], [], [], [], [], []
        # LayerNormalization stages: the rows' mean / 1 / sqrt(var + eps) live in mean / inv ([B * pixels] each); the penalty keeps
        # u (the first-order gradient at the normalised pre-activation, x-hat rows), the tangent zdot and the source s
        n = len(net.stages)
        self.u, self.u_rows, self.zdot, self.s, self.gin = [None] * n, None, [None] * n, [None] * n, [None] * n
        self.xin: List[Optional[torch.Tensor]] = [None] * len(net.stages)
        for st in net.stages:
            self.a.append(f(B, *st.out_shape))
            self.dz.append(None)
            self.v.append(None)
            self.z.append(f(B, *st.out_shape) if st.bn is not None or st.ln is not None or st.pn is not None
                          or (st.mod is not None and st.mod.demodulate) else None)
            c = B * st.ln_pixels if st.ln is not None else B * st.pn_rows if st.pn is not None else st.out_shape[-1]
            self.mean.append(f(c) if st.bn is not None or st.ln is not None else None)
            self.inv.append(f(c) if st.bn is not None or st.ln is not None or st.pn is not None else None)      # PixelNormalization: the rows' r
            self.keep.append(None)
        # dropout masks of all stages live in ONE uint8 buffer (16-byte aligned slices): a pass draws them with one launch
        DR = self.drop_rows
        sizes = [int(np.prod((DR,) + st.out_shape)) if st.drop else 0 for st in net.stages]
        offs, total = [], 0
        for n in sizes:
            offs.append(total)
            total += -(-n // 16) * 16
        self.keep_flat = torch.empty(max(total, 16), dtype=torch.uint8, device=device)
        self.keep_total = total
        for i, (st, n) in enumerate(zip(net.stages, sizes)):
            if n:
                self.keep[i] = self.keep_flat[offs[i]:offs[i] + n].view((DR,) + st.out_shape)
        rates = {float(st.drop) for st in net.stages if st.drop}
        self.keep_rate = rates.pop() if len(rates) == 1 else None      # None: stages differ, draw per stage
        # the noise maps of all NoiseInjection stages live in ONE fp32 buffer of B * P floats, P = the stages' pixels per sample:
        # a pass draws them with one launch.  Stage by stage ([stage][B][H * W]: the kernels read a stage's map as one contiguous
        # [R] vector); maps handed in are [B, P], per sample in network order, and are dealt out by Net.noise_load
        self.noise = [None] * len(net.stages)
        self.noise_flat, self.noise_active = None, False
        if net.has_noise:
            P = sum(st.noise_pixels for st in net.stages if st.noise is not None)
            self.noise_flat, o = f(B * P), 0
            for i, st in enumerate(net.stages):
                if st.noise is not None:
                    self.noise[i] = self.noise_flat[o:o + B * st.noise_pixels]
                    o += B * st.noise_pixels
        # StyleModulation stages: the styles s [B, I], the demodulation d [B, O] and the modulated input xs of the pass (the raw
        # conv output is z[i]); w is the pass's style source, the assembled input behind latent_pn
        self.mod_w = None
        self.mod_s, self.mod_d, self.mod_xs = ([None] * len(net.stages) for _ in range(3))
        for i, st in enumerate(net.stages):
            if st.mod is not None:
                self.mod_s[i], self.mod_xs[i] = f(B, st.in_shape[-1]), f(B, *st.in_shape)
                self.mod_d[i] = f(B, st.out_shape[-1]) if st.mod.demodulate else None
        # MappingNetwork prefix: its input of the pass (z, or the normalised latents), the layers' outputs h_1 .. h_n (h_n = w), dL/dw
        # as the backward collects it, a second [B, U] buffer the mapping backward alternates with, the truncated w and the batch
        # mean of w that the running average takes
        self.map_in, self.map_h, self.mod_dw, self.map_g, self.map_trunc, self.map_mean = None, [], None, None, None, None
        if net.has_mapping:
            U = net.style_dim
            self.map_h = [f(B, U) for _ in range(net.mapping.num_layers)]
            self.mod_dw, self.map_g = f(B, U), f(B, U)
        self._net, self._device = net, device
        net.check_rows(B)
        self._extra = {}
        self._bn_grad_scratch = {}
        self.dropout_active = False
        self.aug = None             # (DiffAugment, params [B, 8]) of this pass's last forward: what its backward applies L^T with

    def keep_elems(self, i):
        """Output elements of stage i covered by its dropout mask (0 = all of them): the bg_epilogue.keep_elems field."""
        return 0 if self.drop_rows >= self.B else self.drop_rows * int(np.prod(self._net.stages[i].out_shape))

    def dropout(self, i):
        """(keep mask or None, 1 / (1 - rate), keep_elems) of stage i as this pass's last forward left it: what the LeakyReLU
        epilogue and the three LeakyReLU' / Dropout' sites of the backward multiply by.  (None, 1.0, 0) without Dropout or
        with training=False."""
        st = self._net.stages[i]
        if not (st.drop and self.dropout_active):
            return None, 1.0, 0
        return self.keep[i], st.drop_scale, self.keep_elems(i)

    def masked_then_tail(self, i, launch):
        """Runs ``launch(rows, keep, scale)`` for the Dropout' factor of stage i over the whole batch -- as one call, or, where
        the masks cover the first drop_rows samples only, for the masked rows first and for the unmasked tail separately."""
        keep, scale, _ = self.dropout(i)
        if keep is not None and self.drop_rows < self.B:
            launch(slice(0, self.drop_rows), keep, scale)
            launch(slice(self.drop_rows, None), None, 1.0)
        else:
            launch(slice(None), keep, scale)

    def rows(self, lo, hi):
        """A view of this pass restricted to samples [lo, hi): what gp_second_order needs of the x-hat rows of a merged pass."""
        return _RowView(self, lo, hi)

    def bn_partials(self, i, rows, C):
        """Room for the per-workgroup BatchNorm statistics the conv of stage i leaves behind (bg_epilogue.stats)."""
        key = ("bn_partials", i)
        n = rows * 2 * C
        if key not in self._extra or self._extra[key].numel() < n:
            self._extra[key] = torch.empty(n, dtype=torch.float32, device=self._device)
        return self._extra[key]

    def bn_sums(self, i, C):
        key = ("bn_sums", i)
        if key not in self._extra:
            self._extra[key] = torch.empty(2 * C, dtype=torch.float32, device=self._device)
        return self._extra[key]

    def bn_grad_scratch(self, i, C):
        """(dgamma, dbeta) of stage i's BatchNorm for a backward that wants no weight gradients (the kernels write them anyway)."""
        if i not in self._bn_grad_scratch:
            self._bn_grad_scratch[i] = tuple(torch.empty(C, dtype=torch.float32, device=self._device) for _ in range(2))
        return self._bn_grad_scratch[i]

    def mbstd_stats(self, i):
        """(mu, rs, f, q, fdot) of MinibatchStdDev stage i: the groups' column means and 1 / s the forward leaves, the groups'
        statistic, the sum of the incoming gradient's new channel the backward leaves (the penalty's source reads it) and the
        tangent's scalar."""
        key = ("mbstd", i)
        if key not in self._extra:
            st = self._net.stages[i]
            n, E = self.B // st.lin.group_size, int(np.prod(st.in_shape))
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self._device)
            self._extra[key] = (f(n, E), f(n, E), f(n), f(n), f(n))
        return self._extra[key]

    def keep_u(self, i, rows):
        """Room for u of LN stage i on samples ``rows`` = (lo, hi): what the first-order backward leaves for the penalty."""
        n = rows[1] - rows[0]
        if self.u[i] is None or self.u[i].size(0) != n:
            self.u[i] = torch.empty((n,) + self._net.stages[i].out_shape, dtype=torch.float32, device=self._device)
        self.u_rows = tuple(rows)
        return self.u[i]

    def aug_input(self):
        """The augmented input batch T(blur(x)): stage 0's input of a pass with DiffAugment, next to the (blurred) batch in a0."""
        if "aug_input" not in self._extra:
            self._extra["aug_input"] = torch.empty_like(self.a0)
        return self._extra["aug_input"]

    def blur_grad(self):
        """Where blur^T of the input gradient goes when the blurred input itself has to survive the backward."""
        if "blur_grad" not in self._extra:
            self._extra["blur_grad"] = torch.empty_like(self.a0)
        return self._extra["blur_grad"]

    def mod_scratch(self, i):
        """(dd [B, O], dq [B, O], ds [B, I], s2 [B, I], dQ [I, O]) of modulated stage i's backward."""
        key = ("mod", i)
        if key not in self._extra:
            st = self._net.stages[i]
            I, O = st.in_shape[-1], st.out_shape[-1]
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self._device)
            self._extra[key] = (f(self.B, O), f(self.B, O), f(self.B, I), f(self.B, I), f(I, O))
        return self._extra[key]

    def input_grad(self):
        if self.din is None:
            self.din = torch.empty((self.B,) + self._net.in_shape, dtype=torch.float32, device=self._device)
        return self.din


class _RowView(_StageBuffers):
    """Samples [lo, hi) of a Context: sliced activations / gradients, own scratch for the linearised forward."""

    def __init__(self, ctx, lo, hi):
        self._ctx, self.lo, self.hi, self.B = ctx, lo, hi, hi - lo
        self.a = [t[lo:hi] for t in ctx.a]
        self.dz = [None if t is None else t[lo:hi] for t in ctx.dz]
        key = ("rowview_v", lo, hi)
        self.v = ctx._extra.setdefault(key, [None] * len(ctx.a))
        self._net, self._device = ctx._net, ctx._device
        # LayerNormalization stages (the penalty's second order): the rows' saved statistics, the u the backward kept for exactly
        # these samples, own scratch for the tangent and the source
        px = [st.ln_pixels for st in ctx._net.stages]
        self.z = [None if t is None else t[lo:hi] for t in ctx.z]
        self.mean = [t[lo * n:hi * n] if st.ln is not None else None for t, n, st in zip(ctx.mean, px, ctx._net.stages)]
        self.inv = [t[lo * n:hi * n] if st.ln is not None else None for t, n, st in zip(ctx.inv, px, ctx._net.stages)]
        self.xin = [None if t is None else t[lo:hi] for t in ctx.xin]
        self.u, self.u_rows = ctx.u, (None if ctx.u_rows is None else (ctx.u_rows[0] - lo, ctx.u_rows[1] - lo))
        self.zdot = ctx._extra.setdefault(("rowview_zdot", lo, hi), [None] * len(ctx.a))
        self.s = ctx._extra.setdefault(("rowview_s", lo, hi), [None] * len(ctx.a))

    def mbstd_stats(self, i):
        """The groups of samples [lo, hi) out of the pass's (groups are consecutive and the slices whole multiples of a group)."""
        G = self._net.stages[i].lin.group_size
        assert self.lo % G == 0 and self.hi % G == 0, (self.lo, self.hi, G)
        return tuple(t[self.lo // G:self.hi // G] for t in self._ctx.mbstd_stats(i))


class _BackwardPass:
    """What one Net.backward call carries from stage to stage."""

    def __init__(self, ctx, need_dw, beta, scale, reducer, dw_rows, defer_conv_dw, sync_bn, keep_u_rows=None):
        self.dw_started = False         # a mapping prefix: dL/dw has its first contribution of the pass (the next ones add)
        self.ctx, self.need_dw, self.beta, self.scale, self.reducer = ctx, need_dw, beta, scale, reducer
        self.keep_u_rows = keep_u_rows      # LN stages keep u of these samples for the penalty's second order
        self.dw_rows = ctx.B if dw_rows is None else int(dw_rows)
        self.defer_conv_dw, self.sync_bn = defer_conv_dw, sync_bn
        self.pending_stats = None       # SyncBN: the all-reduce of the NEXT (lower) stage's backward statistics, in flight
        self.deferred_ready = []        # SyncBN overlap: gradient slices finished but not yet handed to the reducer

    def release_deferred(self):
        if self.reducer is not None:
            for rng in self.deferred_ready:
                self.reducer.ready(*rng)
        self.deferred_ready.clear()


_GP_SHAPE_MESSAGE = ("gradient penalty second order supports the reference critic shape only: "
                     "[Conv2D+LeakyReLU(+Dropout) | UpSampling2D | AveragePooling2D]* -> Flatten -> Dense(1) (demo_celeba.py:96-124)")


class Net:
    def __init__(self, flat_layers, store):
        self.store = store
        self.device = store.device
        self.blur = None
        self.capture_branches = None     # test instrumentation (gp_second_order_merged): a list collects the x-hat rows' LeakyReLU signs
        self.stages: List[Stage] = []
        self.latent_pn = None            # layers.PixelNormalization as the network's first layer: the latents' normalisation
        self.mapping = None              # layers.MappingNetwork in front of the first stage: z -> w, the style source
        self.in_shape = tuple(flat_layers[0][1])
        self.style_dim = self.in_shape[0] if len(self.in_shape) == 1 else None      # the size of the style source: L, or the prefix's units
        cur = None
        n_masks = 0
        for idx, (l, s) in enumerate(flat_layers):
            k = l.kind
            if k == "blur":
                if idx != 0:
                    raise NotImplementedError("GaussianBlur2D is only supported as the first layer (blurred_gan.py:31-34)")
                self.blur = l
            elif k in ("dense", "conv", "convT") + PARAMETER_FREE:
                if k == "mbstd":
                    self.mbstd_check_position(flat_layers, idx, cur)
                    if cur.pn is not None:
                        raise NotImplementedError(self.PN_RULE + " (MinibatchStdDev behind a PixelNormalization stage is not supported)")
                cur = Stage(l, s)
                self.stages.append(cur)
                if cur.mod is not None: self.mod_place(flat_layers, idx, cur)      # noqa: E701
            elif k in ("bn", "layernorm", "dropout", "pixelnorm") and cur is not None and cur.mod is not None:
                raise NotImplementedError(MOD_RULE + f" (a {type(l).__name__} in the stage of a StyleModulation)")
            elif k == "mapping":
                self.mapping_place(flat_layers, idx, cur)
            elif k == "pixelnorm":
                self.pn_place(flat_layers, idx, cur)
            elif k in ("bn", "layernorm", "dropout", "lrelu") and cur is not None and cur.pn is not None:
                raise NotImplementedError(self.PN_RULE + f" (a {type(l).__name__} follows the PixelNormalization of its stage)")
            elif k == "noise":
                self.noise_place(flat_layers, idx, cur)
            elif k in ("bn", "layernorm", "dropout") and cur is not None and cur.noise is not None:
                raise NotImplementedError(self.NOISE_RULE + f" (a {type(l).__name__} in the stage of a NoiseInjection)")
            elif k == "bn":
                if cur is not None and cur.ln is not None:
                    raise NotImplementedError("LayerNormalization together with BatchNormalization in one stage is not supported")
                if cur is None or cur.kind in PARAMETER_FREE or cur.bn is not None or cur.act is not None or cur.drop:
                    raise NotImplementedError("BatchNormalization must directly follow a linear layer")
                cur.bn = l
            elif k == "layernorm":
                if cur is not None and cur.bn is not None:
                    raise NotImplementedError("LayerNormalization together with BatchNormalization in one stage is not supported")
                if cur is not None and cur.act == "tanh":
                    raise NotImplementedError("LayerNormalization and tanh in one stage are not supported")
                if cur is None or cur.kind != "conv" or cur.ln is not None or cur.act is not None or cur.drop:
                    raise NotImplementedError("LayerNormalization must directly follow a Conv2D (not a Dense, a Conv2DTranspose or a "
                                              "resampling layer)")
                cur.ln = l
            elif k == "lrelu":
                if cur is None or cur.kind in PARAMETER_FREE or cur.act is not None or cur.drop:
                    raise NotImplementedError("LeakyReLU must follow a linear layer or its BatchNormalization")
                cur.act, cur.alpha = "lrelu", l.alpha
            elif k == "dropout":
                if cur is None or cur.kind in PARAMETER_FREE or cur.drop or cur.bn is not None or cur.act != "lrelu":
                    raise NotImplementedError("Dropout is supported after conv + LeakyReLU (demo_celeba.py:99-121)")
                cur.drop = l.rate
                if cur.drop:
                    cur.mask_index, n_masks = n_masks, n_masks + 1
            elif k in ("reshape", "flatten"):
                pass
            else:
                raise NotImplementedError(f"layer kind {k!r}")
        for st in self.stages:
            st.folds_inference_bn = st.bn is not None and st.kind != "dense" and st.lin.vars.get("bias") is None
            if st.kind == "dense" and st.bn is None and st.pn is None and st.act is not None:
                raise NotImplementedError("Dense + activation without BatchNormalization is not on the reference path")
            if st.act == "tanh" and st.bn is not None:
                raise NotImplementedError("tanh after BatchNormalization is not on the reference path")
            if st.ln is not None and st.act != "lrelu":
                raise NotImplementedError("LayerNormalization must be followed by a LeakyReLU")
            if st.noise is not None and st.act != "lrelu":
                raise NotImplementedError(self.NOISE_RULE + " (the stage has no LeakyReLU)")
        if self.stages and (self.stages[0].kind in RESAMPLE or self.stages[-1].kind in RESAMPLE):
            raise NotImplementedError("UpSampling2D / AveragePooling2D must stand between two linear layers, not first or last in a network")
        self.out_shape = self.stages[-1].out_shape
        self.conv_layers = [st.lin for st in self.stages if st.kind in ("conv", "convT")]
        # layers.SpectralNormalization: the engine reads W / sigma (and its transposed copy) of these from the store's effective-weight
        # buffer, which spectral_update() fills; the plain conv layers keep their batched transpose
        self.spectral_layers = [st.lin for st in self.stages if isinstance(st.lin, SpectralNormalization)]
        # layers.EqualizedLearningRate: c * W (and its transposed copy) likewise, filled by eqlr_update()
        self.eqlr_layers = [l for l in (self.weight_layer(st.lin) for st in self.stages) if isinstance(l, EqualizedLearningRate)]
        if self.spectral_layers and self.eqlr_layers:
            raise NotImplementedError("SpectralNormalization and EqualizedLearningRate layers in one model are not supported: both lay "
                                      "out the store's effective-weight buffer")
        self.plain_conv_layers = [l for l in self.conv_layers if not isinstance(self.weight_layer(l), (SpectralNormalization, EqualizedLearningRate))]
        # power rounds per optimizer step, read ONCE here (0: no wrapped layer): part of the step-program key; changing a layer's
        # power_iterations on a built model has no effect
        rounds = {l.power_iterations for l in self.spectral_layers}
        if len(rounds) > 1:
            raise NotImplementedError(f"SpectralNormalization layers of one model must share power_iterations, got {sorted(rounds)}")
        self.spectral_rounds = rounds.pop() if rounds else 0
        self.has_ln = any(st.ln is not None for st in self.stages)
        self.mbstd_layers = [st.lin for st in self.stages if st.kind == "mbstd"]
        # a stage with a source term in the penalty (LayerNormalization, MinibatchStdDev): such a critic takes the separate
        # second-order route, and its first-order backward keeps what the source needs
        self.has_source = self.has_ln or bool(self.mbstd_layers)
        self.has_pn = self.latent_pn is not None or any(st.pn is not None for st in self.stages)
        self.has_noise = any(st.noise is not None for st in self.stages)
        self.noise_pixels = sum(st.noise_pixels for st in self.stages if st.noise is not None)     # P: noise values per sample
        self.mod_layers = [st.lin for st in self.stages if st.mod is not None]
        self.has_mod = bool(self.mod_layers)
        self.has_mapping = self.mapping is not None
        self._ctx = {}
        self._rows_checked = set()
        self._ws = None
        self._taps_cache = {}
        self._taps_ring = {"i": 0, "bufs": [], "evs": []}     # pinned staging of the tap uploads (blur_taps)
        self._splitk_bytes = {}
        self.rng_offset = 0
        self.conv_math = "fp32"   # conv forward / data-gradient math of every call site below (ops.CONV_MATH; WGAN(conv_math=...))
        self.sync_bn = True       # data parallel: BatchNormalization statistics over the global batch
        # statistics in the producing conv's epilogue: off since round 3 -- the plain gather-GEMM variant now stores float4
        # (transposed accumulators), the statistics variant cannot, and the separate statistics pass costs less than that (C2
        # +0.24 %, C4 +0.3 % in a same-box A/B); tests set it to compare the two routes
        self.fuse_bn_stats = False

    # ------------------------------------------------------------------ resources
    def context(self, B, tag="default", drop_rows=None) -> Context:
        key = (B, tag, drop_rows)
        if key not in self._ctx:
            self._ctx[key] = Context(self, B, self.device, drop_rows=drop_rows)
        return self._ctx[key]

    def workspace(self, nbytes):
        n = max(int(nbytes), 1024)
        if self._ws is None or self._ws.numel() * 4 < n:
            self._ws = torch.empty((n + 3) // 4 + 1024, dtype=torch.float32, device=self.device)
        return self._ws

    def _epi(self, bwd_data, B, H, W, Cin, Cout, k, stride, mode, **kw):
        """Epilogue descriptor for one conv launch; attaches split-K scratch when the library's plan wants it."""
        key = (bool(bwd_data), B, H, W, Cin, Cout, k, stride)
        nb = self._splitk_bytes.get(key)
        if nb is None:
            nb = self._splitk_bytes[key] = ops.conv2d_splitk_workspace_bytes(bwd_data, B, H, W, Cin, Cout, k, stride)
        return ops.epilogue(mode, ws=self.workspace(nb) if nb else None, **kw)

    def _conv(self, st, x, y, transpose, mode, **kw):
        """One launch of conv stage ``st`` with an epilogue, in one of its two directions.  Apply (the layer's forward): Conv2D ->
        conv2d_fwd with the transposed kernel copy, Conv2DTranspose -> conv2d_bwd_data with the kernel array.  ``transpose``
        (its input gradient): the other way round.  Returns the epilogue (conv2d_stats_rows reads it)."""
        bwd_data = (st.kind == "convT") != transpose
        lin = st.lin
        epi = self._epi(bwd_data, x.size(0), *st.geom, mode, **kw)
        if bwd_data:
            ops.conv2d_bwd_data(x, self.store.kernel(lin), y, lin.k, lin.stride, epi, math=self.conv_math)
        else:
            ops.conv2d_fwd(x, self.store.kernel(lin, transposed=True), y, lin.k, lin.stride, epi, math=self.conv_math)
        return epi

    def _filter_grad(self, st, a, dz, beta, scale):
        """store.grad[kernel] = beta * old + scale * wgrad of conv stage ``st`` from its input ``a`` and output gradient ``dz``
        (for a Conv2DTranspose the two swap sides)."""
        x, dy = (a, dz) if st.kind == "conv" else (dz, a)
        dW = self.store.grad_of(st.lin, "kernel")
        nb = ops.conv2d_bwd_filter_workspace_bytes(x.size(0), *st.geom)
        ops.conv2d_bwd_filter(x, dy, dW, st.lin.k, st.lin.stride, beta, scale, self.workspace(nb) if nb else None)

    def prepare_weights(self):
        """(Re)builds what the passes read in place of changed weights: W / sigma of the spectrally normalised layers (sigma = v^T W u
        refreshed, no power round), c * W of the equalised-learning-rate layers, and the transposed kernel copies the 'other
        direction' of each conv needs."""
        self.spectral_update(iterate=False)
        self.eqlr_update()
        self.store.refresh_transposed(self.plain_conv_layers)
        self.mod_update()

    # ---- spectral normalisation (DESIGN.md §5 "Spectral normalisation").  Public names, as the LayerNormalization helpers below:
    # the engine-trace fixture's configurations have no such layer; tests/test_spectral_cpu.py records what these enqueue.
    def spectral_update(self, iterate=True):
        """The wrapped layers' sigma and effective weights.  ``iterate``: the layers' power rounds (the start of this model's optimizer
        step), else sigma = v^T W u with the stored vectors, and only if the weights changed since the last update.  Then W / sigma
        with its transposed copies, one launch for all layers."""
        if not self.spectral_layers or not (iterate or self.store.sn_dirty):
            return
        table = self.store.spectral_table(self.spectral_layers)
        for _ in range(self.spectral_rounds if iterate else 1):
            ops.spectral.power(self.store.theta, self.store.state, table, sigma_only=not iterate)
        ops.spectral.scale(self.store.theta, self.store.state, self.store.eff, table)
        self.store.sn_dirty = False

    def spectral_project_gradients(self):
        """store.grad holds dL/dW-bar of the wrapped layers (the passes ran on W-bar = W / sigma): in place, dL/dW =
        (g - <g, W-bar> v u^T) / sigma, u and v held constant.  Linear, with u, v, sigma equal on all ranks: after the all-reduce."""
        if self.spectral_layers:
            ops.spectral.grad(self.store.grad, self.store.eff, self.store.state, self.store.spectral_table(self.spectral_layers))

    # ---- equalised learning rate (DESIGN.md §5 "Equalised learning rate").  Public names for the reason above;
    # tests/test_eqlr_cpu.py records what these enqueue.
    def eqlr_update(self):
        """The wrapped layers' effective weights c * W with their transposed copies: one launch for all layers."""
        if self.eqlr_layers:
            table = self.store.eqlr_table(self.eqlr_layers)        # lays out store.eff
            ops.eqlr.scale(self.store.theta, self.store.eff, table)

    def eqlr_scale_gradients(self):
        """store.grad holds dL/dW_eff of the wrapped layers (the passes ran on W_eff = c * W): in place, dL/dW = c * dL/dW_eff.
        Linear, with c equal on all ranks: after the all-reduce, in front of the optimizer."""
        if self.eqlr_layers:
            ops.eqlr.grad(self.store.grad, self.store.eqlr_table(self.eqlr_layers))

    def blur_taps(self, H, W):
        """(device buffer, tap count) of the layer's CURRENT std for H x W images (gaussian_blur.py:21-31,83-88 through
        bg_blur_policy / bg_gauss_kernel_1d).  The taps of one image size live in ONE persistent device buffer whose address never
        changes (a recorded step program holds it); when std has changed since the last call the new weights are copied into it
        in stream order.  sigma changes every batch under BlurDecayController: the upload goes through a pinned staging ring and
        an asynchronous copy (a pageable copy would wait for the stream to drain)."""
        std = float(self.blur.std)
        ent = self._taps_cache.get((H, W))
        if ent is None:
            ent = self._taps_cache[(H, W)] = {"std": None, "nt": 0, "dev": torch.zeros(1024, dtype=torch.float32, device=self.device)}
        if ent["std"] != std:
            ks, se, nt = ops.blur_policy(std, H, W)
            taps = ops.gauss_kernel_1d(se, ks)
            assert len(taps) == nt
            if nt > 1024:
                raise NotImplementedError(f"blur with {nt} taps (> 1024)")
            ring = self._taps_ring
            if not ring["bufs"]:
                for _ in range(8):
                    ring["bufs"].append(torch.empty(1024, dtype=torch.float32, pin_memory=self.device.type == "cuda"))
                    ring["evs"].append(None)
            i = ring["i"] = (ring["i"] + 1) % len(ring["bufs"])
            if ring["evs"][i] is not None:
                ring["evs"][i].synchronize()                  # slot re-used 8 uploads later: normally long complete
            host = ring["bufs"][i][:nt]
            host.copy_(torch.tensor(taps, dtype=torch.float32))
            ent["dev"][:nt].copy_(host, non_blocking=True)
            if self.device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record()
                ring["evs"][i] = ev
            ent["std"], ent["nt"] = std, nt
        return ent["dev"], ent["nt"]

    def blur_n_taps(self, H=None, W=None):
        """Tap count of the current std (uploads the taps if std changed): part of a step program's key."""
        if self.blur is None:
            return 0
        H = self.in_shape[0] if H is None else H
        W = self.in_shape[1] if W is None else W
        return self.blur_taps(H, W)[1]

    def apply_blur(self, x, y):
        """y = blur(x) with the layer's current std (blurred_gan.py:30; self-adjoint, so also its backward)."""
        B, H, W, C = x.shape
        taps, nt = self.blur_taps(H, W)
        nb = ops.blur_workspace_bytes(B, H, W, C, nt)
        tmp = self.workspace(nb) if nb else None
        with ops.trace_range("blur"):
            return ops.blur_nhwc(x, y, taps, nt, tmp)

    # ------------------------------------------------------------------ forward
    def forward(self, ctx: Context, inputs=None, training=False, masks=None, seed=0, lerp_alpha=None, lerp_out=None, augment=None, noise=None,
                w=None, truncation_psi=None):
        """inputs: a tensor [B,...] or a list of tensors concatenated along the batch.  ``training`` switches
        Dropout and BatchNormalization exactly as Keras' ``training=`` argument does.
        ``lerp_alpha`` (with inputs = [f, r]): a third batch slice x-hat = r + alpha (f - r) follows the two (wgan.py:239).  Behind
        a blur layer of a geometry the row-block kernel takes, all three slices are blurred by ONE launch that forms x-hat on the
        fly (bg_blur3_lerp_nhwc_f32); otherwise x-hat is written to ``lerp_out`` by bg_lerp_f32 and joins the list.
        ``augment`` = (DiffAugment, params [B, 8]): the assembled (blurred) batch goes through T into a second input-sized buffer,
        which is what stage 0 reads; the pass's backward applies L^T ahead of blur^T (aug_forward / aug_backward).
        ``w`` (a network with a MappingNetwork prefix, in place of ``inputs``): [B, units] styles; the prefix is skipped.
        ``truncation_psi`` (such a network, inference only): w <- w_avg + psi * (w - w_avg) between prefix and synthesis network.
        ``noise`` (a network with NoiseInjection stages; in training and in inference alike): None draws the maps of all stages
        with ONE launch from ``seed`` and this network's counter, as the one-draw keep mask is drawn; a tensor [B, P] (per sample,
        the stages' maps in network order) is copied in; False leaves the noise launches out, as if every strength were 0."""
        if self.store.tr_dirty:
            self.prepare_weights()
        if w is not None or truncation_psi is not None: self.mapping_check_call(ctx, inputs, w, truncation_psi, training)      # noqa: E701
        ctx.aug = augment
        x = w if w is not None else self._assemble_input(ctx, inputs, lerp_alpha, lerp_out)      # w: the styles stand in for the prefix's output
        if augment is not None: x = self.aug_forward(ctx, x)      # noqa: E701
        if self.latent_pn is not None and w is None: x = self.pn_latents(ctx, x)      # noqa: E701
        if self.has_mapping and w is None: x = self.mapping_forward(ctx, x)      # noqa: E701
        if truncation_psi is not None: x = self.mapping_truncate(ctx, x, truncation_psi)      # noqa: E701
        if self.has_mod or self.has_mapping: ctx.mod_w = x.view(ctx.B, self.style_dim)      # noqa: E701  (the style source of every modulated stage)
        ctx.dropout_active = bool(training)
        # one launch draws the masks of all stages; where their rates differ, or masks are handed in, each stage sets its own
        one_draw = bool(training and masks is None and ctx.keep_rate is not None and ctx.keep_total)
        if one_draw:
            ops.keep_mask(ctx.keep_flat[:ctx.keep_total], 1.0 - ctx.keep_rate, seed, counter=(self, "rng_offset"))
        if self.has_noise: self.noise_draw(ctx, noise, seed)      # noqa: E701
        folded = () if training else self._fold_inference_bns(ctx)
        for i, st in enumerate(self.stages):
            xin = ctx.xin[i] = x.view(ctx.B, *st.in_shape)
            x = ctx.a[i]
            if st.kind == "mbstd": self.mbstd_forward(ctx, i, st, xin, x); continue      # noqa: E701,E702
            if st.kind in RESAMPLE:
                self._resample(st, xin, x)
            else:
                if st.drop and training and masks is not None:
                    ctx.keep[i].copy_(masks[st.mask_index].view(ctx.keep[i].shape))
                elif st.drop and training and not one_draw:
                    ops.keep_mask(ctx.keep[i], 1.0 - st.drop, seed, counter=(self, "rng_offset"))
                self._linear_forward(ctx, i, st, xin, x, training, i in folded)
        return x

    def _assemble_input(self, ctx, inputs, lerp_alpha, lerp_out):
        """The pass's input batch: the single tensor itself, or ctx.a0 filled from the list -- through the blur where the network
        starts with one (per slice, or all three slices of a ``lerp_alpha`` pass in one launch), by copies otherwise."""
        if not isinstance(inputs, (list, tuple)):
            inputs = [inputs]
        if lerp_alpha is not None:
            f, r = inputs
            n = int(f.shape[0])
            assert 3 * n == ctx.B
            if self.blur is not None:
                H, W, C = self.in_shape
                taps, nt = self.blur_taps(H, W)
                if not os.environ.get("BGAN_NO_FUSED_BLUR3") and ops.blur3_lerp_supported(n, H, W, C, nt):
                    with ops.trace_range("blur"):
                        ops.blur3_lerp(f.view(n, *self.in_shape), r.view(n, *self.in_shape), lerp_alpha, ctx.a0, taps, nt)
                    return ctx.a0
            inputs = [f, r, ops.lerp(r, f, lerp_alpha, lerp_out)]
        assert sum(int(t.shape[0]) for t in inputs) == ctx.B, "batch mismatch"
        if self.blur is None and len(inputs) == 1:
            return inputs[0]
        o = 0
        for t in inputs:
            n = int(t.shape[0])
            if self.blur is not None:
                self.apply_blur(t.view(n, *self.in_shape), ctx.a0[o:o + n])
            else:
                ops.copy_(ctx.a0[o:o + n], t.view(n, *self.in_shape).contiguous())
            o += n
        return ctx.a0

    def _fold_inference_bns(self, ctx):
        """Inference BatchNorms (the generator inside the D-step): every layer's fold in ONE launch ahead of the first conv instead
        of a tiny launch between each pair of convs (two kernel boundaries where one would do).  Returns the stages it folded."""
        fl = [j for j, st in enumerate(self.stages) if st.folds_inference_bn]
        if not 1 < len(fl) <= ops.FOLD_MAX:
            return ()
        ops.bn_fold_many([(*self.stages[j].bn_args().values(), *self._fold_out(ctx, j)) for j in fl])
        return set(fl)

    def _fold_out(self, ctx, i):
        """(scale, shift) of stage i's folded BatchNorm: the halves of its sums buffer, unused in inference."""
        C = self.stages[i].out_shape[-1]
        sc = ctx.bn_sums(i, C)
        return sc[:C], sc[C:]

    def _linear_forward(self, ctx, i, st, xin, out, training, folded):
        """Stage i's linear op with what its epilogue fuses (bias, activation, Dropout, folded inference BatchNorm), then its
        BatchNorm + LeakyReLU pass where it has one of its own."""
        if st.ln is not None: return self.ln_forward(ctx, i, st, xin, out)      # noqa: E701
        if st.pn is not None: return self.pn_forward(ctx, i, st, xin, out)      # noqa: E701
        if st.mod is not None: return self.mod_forward(ctx, i, st, xin, out)      # noqa: E701
        if st.noise is not None and ctx.noise_active: return self.noise_forward(ctx, i, st, xin, out)      # noqa: E701
        bias = st.lin.vars.get("bias")
        tgt = ctx.z[i] if st.bn is not None else out
        stat_rows = 0          # rows of BatchNorm statistics partials the conv left behind (0: none)
        if st.kind == "dense":
            ops.gemm(xin, self.store.kernel(st.lin), tgt, ctx.B, st.out_shape[0], st.in_shape[0], bias=bias)
        elif st.folds_inference_bn and not training:
            scale, shift = self._fold_out(ctx, i)
            if not folded:
                ops.bn_fold(**st.bn_args(), scale_out=scale, shift_out=shift)
            self._conv(st, xin, out, False, EPI_AFFINE_LRELU, bias=shift, ref=scale, alpha=st.alpha)
            return
        elif st.bn is not None:
            # training BatchNorm behind a bias-free conv: the MFMA kernel leaves the column sums of what it stores
            # (one row per workgroup); at most one workgroup per 32 output rows and sub-pixel phase
            stats = None
            # under SyncBN the statistics ride in the conv's epilogue (the separate statistics pass would be two more
            # launches on the forward critical path beside every exchange); single-device: opt-in, see __init__
            if training and bias is None and (self.fuse_bn_stats or (self.sync_bn and dist.collectives_active()
                                                                   and not os.environ.get("BGAN_NO_FUSED_BN_STATS"))):
                stats = ctx.bn_partials(i, int(np.prod((ctx.B,) + st.out_shape[:-1])) // 32 + 64, st.out_shape[-1])
            stat_rows = ops.conv2d_stats_rows(self._conv(st, xin, tgt, False, EPI_NONE, bias=bias, stats=stats))
        elif st.act == "lrelu":
            keep, _, keep_elems = ctx.dropout(i)
            # the scale is the stage's in inference too, as this launch has always been made (the kernel reads it with a mask only)
            self._conv(st, xin, tgt, False, EPI_BIAS_LRELU, bias=bias, keep=keep, alpha=st.alpha, scale=st.drop_scale, keep_elems=keep_elems)
        else:
            self._conv(st, xin, tgt, False, EPI_TANH if st.act == "tanh" else EPI_NONE, bias=bias)
        if st.bn is not None:
            self._bn_forward(ctx, i, st, tgt, out, training, stat_rows)

    def _bn_forward(self, ctx, i, st, tgt, out, training, stat_rows):
        """out = LeakyReLU(BatchNorm(tgt)) of stage i, by the route the pass calls for: inference, SyncBN, statistics partials the
        conv left behind (``stat_rows``), or the plain training pass."""
        C = st.out_shape[-1]
        M = tgt.numel() // C
        if not training:
            ops.bn_infer_fwd(tgt, out, M, C, **st.bn_args(), lrelu_alpha=st.alpha)
            return
        train = dict(st.bn_args(), save_mean=ctx.mean[i], save_inv=ctx.inv[i], momentum=st.bn.momentum,
                     unbiased=(len(st.out_shape) == 3), lrelu_alpha=st.alpha)
        if self.sync_bn and dist.collectives_active():
            # SyncBN: batch statistics over the GLOBAL batch -- all-reduce the per-channel sums
            sums = ctx.bn_sums(i, C)
            if stat_rows:
                ops.bn_sums_from_partials(ctx.bn_partials(i, stat_rows, C), stat_rows, C, sums)
            else:
                ops.bn_stats(tgt, M, C, sums, self.workspace(ops.bn_workspace_bytes(M, C)))
            dist.all_reduce_sum_(sums)
            # finalize + apply in one launch: with the statistics out of the conv's epilogue the chain around the
            # exchange is two launches per layer (partials -> sums, this)
            ops.bn_finalize_apply(sums, M * dist.world_size(), tgt, out, M, C, **train)
        elif stat_rows:
            ops.bn_train_fwd_partials(ctx.bn_partials(i, stat_rows, C), stat_rows, tgt, out, M, C, **train)
        else:
            ops.bn_train_fwd(tgt, out, M, C, ws=self.workspace(ops.bn_workspace_bytes(M, C)), **train)

    def ln_args(self, ctx, i, st):
        """What every ops.layernorm call of stage i names the same way: rows, channels, the layer's variables and the rows' statistics."""
        C = st.out_shape[-1]
        return dict(R=ctx.B * st.ln_pixels, Cc=C, gamma=st.ln.vars["gamma"], mu=ctx.mean[i], r=ctx.inv[i])

    def ln_forward(self, ctx, i, st, xin, out):
        """Conv2D (+ bias) into ctx.z[i], then out = Dropout(LeakyReLU(LayerNorm(z))) of stage i in one pass; the rows' statistics
        stay in ctx.mean / ctx.inv."""
        z = ctx.z[i]
        self._conv(st, xin, z, False, EPI_NONE, bias=st.lin.vars.get("bias"))
        keep, scale, keep_elems = ctx.dropout(i)
        ops.layernorm.fwd(z, out, **self.ln_args(ctx, i, st), beta=st.ln.vars["beta"], eps=st.ln.epsilon, lrelu_alpha=st.alpha, keep=keep,
                          scale=scale, keep_elems=keep_elems)

    @staticmethod
    def _resample(st, x, y):
        """Forward of a resampling stage; linear and parameter-free, so also its linearised forward in the gradient penalty."""
        if st.kind == "upsample":
            ops.upsample2x(x, y, 1.0)
        elif st.kind == "avgpool":
            ops.pool2x_sum(x, y, 0.25)
        elif st.kind == "firup":            # StyleGAN2's gain: factor ** 2
            ops.fir_upsample2x(x, y, st.lin.taps, 4.0)
        else:
            ops.fir_downsample2x(x, y, st.lin.taps, 1.0)

    @staticmethod
    def resample_transposed(st, g, tgt, **mul_grad):
        """Backward of a resampling stage: its transpose on the output gradient ``g``.  ``mul_grad`` (ref / keep / alpha / grad_scale,
        down-samplers only): LeakyReLU' / Dropout' of the stage below ride in the same launch.  (A public name, as the
        LayerNormalization helpers below carry: the engine-trace fixture's configurations have no filtered stage;
        tests/test_firsample_cpu.py records what the two filtered kinds enqueue.)"""
        if st.kind == "upsample":
            ops.pool2x_sum(g, tgt, 1.0)
        elif st.kind == "avgpool":
            ops.upsample2x(g, tgt, 0.25, **mul_grad)
        elif st.kind == "firup":            # <UP_f x, g> = <x, DOWN_flip(f) g>
            ops.fir_downsample2x(g, tgt, st.lin.flipped_taps, 4.0)
        else:
            ops.fir_upsample2x(g, tgt, st.lin.flipped_taps, 1.0, **mul_grad)

    def predict(self, x, training=False):
        B = x.size(0)
        ctx = self.context(B, "predict")
        x = x.to(self.device, torch.float32).contiguous()
        return self.forward(ctx, x, training=training, seed=np.random.randint(1 << 30)).clone()

    # ------------------------------------------------------------------ backward
    def backward(self, ctx: Context, dout, need_dx=False, need_dw=True, beta=0.0, scale=1.0, reducer=None, dw_rows=None,
                 dx_rows=None, defer_conv_dw=False, keep_u_rows=None):
        """Reverse pass of the last ``forward`` on ``ctx``.  Weight gradients go to ``store.grad``
        (= beta*old + scale*new).  Returns d(loss)/d(net input) *before* the blur (or None).
        ``reducer`` (dist.GradReducer): this pass completes the gradients, so each stage's slice of the flat buffer is
        handed to the bucketed all-reduce as soon as its kernels are enqueued.
        ``dw_rows``: weight gradients from the first dw_rows samples only; ``dx_rows`` = (lo, hi): the input gradient (last
        data-gradient + blur^T) for those samples only -- the merged critic pass wants weights from [fakes; reals] and the
        image gradient of x-hat.  ``defer_conv_dw``: the conv filter gradients are left to ``gp_second_order_merged`` (bias
        and Dense gradients are still taken here).  ``keep_u_rows`` = (lo, hi): LayerNormalization stages keep u, the gradient at
        their normalised pre-activation, for those samples (the x-hat rows: gp_second_order's source term needs it)."""
        if need_dx and self.latent_pn is not None: raise NotImplementedError("the gradient at the input of a network that starts with a PixelNormalization (the latents' normalisation has no backward)")  # noqa: E701
        if need_dx and self.has_mod and not self.has_mapping: raise NotImplementedError("the gradient at the input of a network with StyleModulation stages (dL/dw, the gradient through the styles, is not built)")  # noqa: E701
        if need_dw:
            self.store.ensure_opt_state()
        p = _BackwardPass(ctx, need_dw, beta, scale, reducer, dw_rows, defer_conv_dw, self.sync_bn and dist.collectives_active(),
                          keep_u_rows if self.has_source else None)
        g, g_is_dz = dout, False
        for i in range(len(self.stages) - 1, -1, -1):
            st = self.stages[i]
            prev = self.stages[i - 1] if i > 0 else None
            has_dw = need_dw and st.kind not in PARAMETER_FREE
            dz = ctx.dz[i] = self._grad_through_activation(p, i, st, g.view(ctx.B, *st.out_shape), g_is_dz)
            if st.mod is not None: g, g_is_dz = self.mod_backward(p, i, st, dz); continue      # noqa: E701,E702
            # SyncBN with a BatchNorm stage below: the data gradient goes FIRST, the lower stage's backward statistics are
            # reduced and their all-reduce is put in flight, and only then this stage's filter gradient runs -- the small
            # latency-bound collective hides behind an MFMA kernel instead of sitting on the critical path of every layer.
            # (The filter gradient's split-K workspace and the statistics' partials share net.workspace(): the statistics
            # kernel has finished with it before the filter gradient is enqueued on the same stream.)
            overlap = has_dw and p.sync_bn and prev is not None and prev.bn is not None
            if has_dw and not overlap:
                self._weight_grads(p, i, st, dz)
            if i == 0 and self.has_mapping and (need_dw or need_dx): return self.mapping_backward(p, st, dz, need_dx)      # noqa: E701
            if i == 0 and not need_dx:
                p.release_deferred()
                return None
            g, g_is_dz = self._input_grad(p, i, st, prev, dz, dx_rows)
            if overlap:
                self._bn_bwd_stats(p, i - 1, prev, g)
                p.release_deferred()        # slices finished before this exchange was issued may go out behind it now
                self._weight_grads(p, i, st, dz, defer_ready=True)
        p.release_deferred()
        if ctx.aug is not None: return self.aug_backward(ctx, g, dx_rows)      # noqa: E701
        if self.blur is not None:
            # forward's blurred input is dead by now; reuse it for blur^T(din) -- unless the penalty's LayerNormalization source
            # backward follows (keep_u_rows): its first filter gradient reads the blurred x-hat
            dst = ctx.a0 if p.keep_u_rows is None else ctx.blur_grad()
            out = dst if dx_rows is None else dst[dx_rows[0]:dx_rows[1]]
            return self.apply_blur(g.view(g.shape[0], *self.in_shape), out)
        return g

    def _grad_through_activation(self, p, i, st, gv, g_is_dz):
        """Through stage i's activation / BatchNorm: the gradient w.r.t. its linear op's output.  ``g_is_dz``: the launch that
        produced ``gv`` has applied LeakyReLU' / Dropout' already."""
        ctx = p.ctx
        if st.bn is not None:
            return self._bn_backward(p, i, st, gv)
        if st.ln is not None: return self.ln_backward(p, i, st, gv)      # noqa: E701
        if st.pn is not None: return self.pn_backward(p, i, st, gv)      # noqa: E701
        if st.act == "tanh":
            return ops.tanh_bwd(gv, ctx.a[i], ctx.buf(ctx.dz, i))
        if st.act != "lrelu" or g_is_dz:
            return gv
        dz, a = ctx.buf(ctx.dz, i), ctx.a[i]
        ctx.masked_then_tail(i, lambda rows, keep, scale: ops.mul_grad(gv[rows], a[rows], dz[rows], keep=keep, alpha=st.alpha, scale=scale))
        return dz

    def _bn_backward(self, p, i, st, gv):
        ctx = p.ctx
        C = st.out_shape[-1]
        M = gv.numel() // C
        dz = ctx.buf(ctx.dz, i)
        dg, db = (self.store.grad_of(st.bn, "gamma"), self.store.grad_of(st.bn, "beta")) if p.need_dw else ctx.bn_grad_scratch(i, C)
        gamma, beta = st.bn.vars["gamma"], st.bn.vars["beta"]
        if not p.sync_bn:
            ops.bn_train_bwd(gv, None, ctx.z[i], dz, M, C, gamma, ctx.mean[i], ctx.inv[i], dg, db,
                             self.workspace(ops.bn_workspace_bytes(M, C)), lrelu_alpha=st.alpha, beta=beta)
            return dz
        world = dist.world_size()
        if p.pending_stats is None:         # nothing above it to overlap with (the last stage, or no filter gradient there)
            self._bn_bwd_stats(p, i, st, gv)
        p.pending_stats.wait()              # issued before the filter gradient of the stage above: it travelled meanwhile
        p.pending_stats = None
        sums = ctx.bn_sums(i, C)
        ops.bn_bwd_apply(gv, None, ctx.z[i], dz, M, M * world, C, gamma, ctx.mean[i], ctx.inv[i], sums, lrelu_alpha=st.alpha, beta=beta)
        if p.need_dw:       # the sums are already global: pre-divide so the flat gradient SUM all-reduce restores them
            ops.bn_param_grads(sums, C, 1.0 / world, dg, db)
        return dz

    def ln_backward(self, p, i, st, gv):
        """Through stage i's Dropout, LeakyReLU and LayerNormalization in one pass: dz, the layer's gamma / beta gradients from the
        pass's first dw_rows samples, and (keep_u_rows) u for the penalty."""
        ctx = p.ctx
        dz = ctx.buf(ctx.dz, i)
        keep, scale, keep_elems = ctx.dropout(i)
        args = self.ln_args(ctx, i, st)
        grads = {}
        if p.need_dw:
            grads = dict(dgamma=self.store.grad_of(st.ln, "gamma"), dbeta=self.store.grad_of(st.ln, "beta"), dw_rows=p.dw_rows * st.ln_pixels,
                         acc_beta=p.beta, acc_scale=p.scale, ws=self.workspace(ops.layernorm.workspace_bytes(args["R"], args["Cc"])))
        if p.keep_u_rows is not None:
            lo, hi = p.keep_u_rows
            grads.update(u_out=ctx.keep_u(i, (lo, hi)), u_rows=(lo * st.ln_pixels, hi * st.ln_pixels))
        return ops.layernorm.bwd(gv, ctx.z[i], dz, **args, beta=st.ln.vars["beta"], lrelu_alpha=st.alpha, keep=keep, scale=scale,
                                 keep_elems=keep_elems, **grads)

    def _bn_bwd_stats(self, p, i, st, g):
        """SyncBN: the backward statistics of BatchNorm stage i from the gradient ``g`` of its output, their all-reduce in flight."""
        ctx = p.ctx
        C = st.out_shape[-1]
        gv = g.view(ctx.B, *st.out_shape)
        M = gv.numel() // C
        sums = ctx.bn_sums(i, C)
        ops.bn_bwd_stats(gv, None, ctx.z[i], M, C, ctx.mean[i], ctx.inv[i], sums, self.workspace(ops.bn_workspace_bytes(M, C)),
                         lrelu_alpha=st.alpha, gamma=st.bn.vars["gamma"], beta=st.bn.vars["beta"])
        p.pending_stats = dist.all_reduce_sum_async(sums)

    def _weight_grads(self, p, i, st, dz, defer_ready=False):
        """Kernel and bias gradients of stage i from the pass's first dw_rows samples; its slice of the flat buffer to the reducer."""
        B, WB, lin = p.ctx.B, p.dw_rows, st.lin
        xin = p.ctx.xin[i]
        xw, dzw = (xin, dz) if WB == B else (xin[:WB], dz.view(B, *st.out_shape)[:WB])
        if st.noise is not None: self.noise_backward(p, i, st, dzw)      # noqa: E701
        deferred = p.defer_conv_dw and st.kind == "conv"        # left to gp_second_order_merged, the reducer's hand-over too
        if st.kind == "dense":
            ops.gemm(xw, dzw, self.store.grad_of(lin, "kernel"), st.in_shape[0], st.out_shape[0], WB, transA=True, beta=p.beta, scale=p.scale)
        elif not deferred:
            self._filter_grad(st, xw, dzw, p.beta, p.scale)
        if "bias" in lin.vars:
            N = st.out_shape[-1]
            rows = dzw.numel() // N
            ops.colsum(dzw, self.store.grad_of(lin, "bias"), rows, N, self.workspace(ops.colsum_workspace_bytes(rows, N)), beta=p.beta, scale=p.scale)
        if p.reducer is not None and not deferred:
            # Under the SyncBN overlap a slice is NOT handed over right away: ready() may flush a 16 MB bucket onto the
            # collective stream, and the small statistics exchange of the next stage down, issued one iteration later,
            # would queue behind it -- back on the critical path.  The slice waits until that exchange is in flight.
            if defer_ready:
                p.deferred_ready.append(self._train_range(st))
            else:
                p.reducer.ready(*self._train_range(st))

    def _train_range(self, st):
        """The slice of the flat trainable buffer that holds stage ``st``'s variables: its linear op's, its normalisation's and its
        noise strength (which lies between the linear op's variables and the next stage's)."""
        return self.store.train_range(st.lin, st.bn if st.ln is None else st.ln, st.noise)

    def _input_grad(self, p, i, st, prev, dz, dx_rows):
        """The gradient w.r.t. stage i's input into the dz buffer of the stage below (the pass's input-gradient buffer at i = 0).
        Returns (it, whether it is already that stage's dz: LeakyReLU' / Dropout' of a conv + LeakyReLU stage below ride in
        the data gradient's epilogue or in the pooling backward)."""
        ctx = p.ctx
        if st.kind == "mbstd": return self.mbstd_backward(p, i, st, prev, dz)      # noqa: E701
        fuse = prev is not None and prev.fusable_grad and st.kind not in ("dense",) + UPSAMPLERS
        # the gradient at an LN (or PixelNormalization) stage's output lands in that stage's dz buffer and is turned into dz in place
        # -- except where a row exceeds what a wave holds in registers (ops.layernorm.route / ops.pixelnorm.route: chunks > 1), where
        # the kernel wants a buffer of its own
        below = ctx.gin if prev is not None and self.rereads_rows(prev) else ctx.dz
        tgt = (ctx.buf(below, i - 1) if i > 0 else ctx.input_grad()).view(ctx.B, *st.in_shape)
        if st.kind in RESAMPLE and not fuse:           # the stage's transpose
            self.resample_transposed(st, dz.view(ctx.B, *st.out_shape), tgt)
        elif st.kind in RESAMPLE:           # a down-sampler's: one launch instead of upsample + mul_grad
            dzp, ref = dz.view(ctx.B, *st.out_shape), ctx.a[i - 1]
            ctx.masked_then_tail(i - 1, lambda rows, keep, scale: self.resample_transposed(st, dzp[rows], tgt[rows], ref=ref[rows], keep=keep,
                                                                                          alpha=prev.alpha, grad_scale=scale))
        else:
            if i == 0 and dx_rows is not None:        # the image gradient is wanted for samples [lo, hi) only
                lo, hi = dx_rows
                dz, tgt = dz.view(ctx.B, *st.out_shape)[lo:hi], tgt[lo:hi]
            if st.kind == "dense":
                ops.gemm(dz, self.store.kernel(st.lin), tgt, tgt.size(0), st.in_shape[0], st.out_shape[0], transB=True)
            elif fuse:
                keep, scale, keep_elems = ctx.dropout(i - 1)
                self._conv(st, dz, tgt, True, EPI_MUL_GRAD, ref=ctx.a[i - 1], keep=keep, alpha=prev.alpha, scale=scale, keep_elems=keep_elems)
            else:
                self._conv(st, dz, tgt, True, EPI_NONE)
        return tgt, fuse

    @staticmethod
    def rereads_rows(st):
        """Whether the backward of ``st``'s normalisation reads a row from memory twice (the chunked route of its kernels), so that
        its output must not overwrite the incoming gradient."""
        if st.ln is not None:
            return ops.layernorm.route(st.out_shape[-1])["chunks"] > 1
        return st.pn is not None and ops.pixelnorm.route(st.pn_channels)["chunks"] > 1

    # ---- PixelNormalization (DESIGN.md §5 "Pixel normalisation").  Public names for the reason the LayerNormalization helpers
    # carry them: no configuration of the engine-trace fixture has the layer; tests/test_pixelnorm_cpu.py records what these enqueue.
    PN_RULE = ("PixelNormalization is supported directly behind the LeakyReLU of a Dense (through its Reshape), Conv2D or Conv2DTranspose "
               "stage without BatchNormalization, LayerNormalization, Dropout or tanh, or as the network's first layer on a [C] vector")

    def pn_place(self, flat_layers, idx, cur):
        """Net.__init__'s placement rule for the PixelNormalization at ``flat_layers[idx]``: the latents' normalisation, or the
        normalisation of stage ``cur``; everything else is refused."""
        l, s = flat_layers[idx]
        if idx == 0:
            if len(s) != 1:
                raise NotImplementedError(self.PN_RULE + f" (first layer on an input of shape {tuple(s)})")
            self.latent_pn = l
            return
        ok = (cur is not None and cur.kind in ("dense", "conv", "convT") and cur.act == "lrelu" and flat_layers[idx - 1][0].kind == "lrelu"
              and cur.bn is None and cur.ln is None and not cur.drop and cur.pn is None)
        if not ok:
            raise NotImplementedError(self.PN_RULE)
        cur.pn, cur.pn_channels = l, int(s[-1])

    def pn_latents(self, ctx, x):
        """The latents' normalisation: one launch into a buffer of the pass's own, nothing kept (it has no backward)."""
        if "pn_latents" not in ctx._extra:
            ctx._extra["pn_latents"] = torch.empty((ctx.B,) + self.in_shape, dtype=torch.float32, device=self.device)
        return ops.pixelnorm.fwd(x.view(ctx.B, *self.in_shape), ctx._extra["pn_latents"], ctx.B, self.in_shape[0], eps=self.latent_pn.epsilon)

    def pn_forward(self, ctx, i, st, xin, out):
        """The linear op (+ bias) into ctx.z[i], then out = PixelNorm(LeakyReLU(z)) of stage i in one pass; the rows' r stays in
        ctx.inv[i].  The same in training and in inference."""
        z, bias = ctx.z[i], st.lin.vars.get("bias")
        if st.kind == "dense":
            ops.gemm(xin, self.store.kernel(st.lin), z, ctx.B, st.out_shape[0], st.in_shape[0], bias=bias)
        else:
            self._conv(st, xin, z, False, EPI_NONE, bias=bias)
        if st.noise is not None and ctx.noise_active: self.noise_add(ctx, i, st, z, 1.0)      # noqa: E701
        ops.pixelnorm.fwd(z, out, ctx.B * st.pn_rows, st.pn_channels, r=ctx.inv[i], eps=st.pn.epsilon, lrelu_alpha=st.alpha)

    def pn_backward(self, p, i, st, gv):
        """Through stage i's PixelNormalization and LeakyReLU in one pass, from the stage's stored output: dz, in place where the
        gradient already stands in the stage's dz buffer (_input_grad put it there)."""
        ctx = p.ctx
        return ops.pixelnorm.bwd(gv, ctx.a[i], ctx.inv[i], ctx.buf(ctx.dz, i), ctx.B * st.pn_rows, st.pn_channels, lrelu_alpha=st.alpha)

    # ---- NoiseInjection (DESIGN.md §5 "Noise inputs").  Public names for the reason the LayerNormalization helpers carry them: no
    # configuration of the engine-trace fixture has the layer; tests/test_noise_cpu.py records what these enqueue.
    NOISE_RULE = ("NoiseInjection is supported directly behind a Conv2D or Conv2DTranspose (not a Dense or a resampling layer), once per "
                  "stage, in front of the stage's LeakyReLU, in a stage without BatchNormalization, LayerNormalization, Dropout or tanh")

    def noise_place(self, flat_layers, idx, cur):
        """Net.__init__'s placement rule for the NoiseInjection at ``flat_layers[idx]``: the noise input of stage ``cur``, whose
        linear layer stands directly in front of it; everything else is refused."""
        l, _ = flat_layers[idx]
        ok = (cur is not None and cur.kind in ("conv", "convT") and idx > 0 and flat_layers[idx - 1][0] is cur.lin and cur.act is None
              and cur.bn is None and cur.ln is None and not cur.drop and cur.pn is None and cur.noise is None)
        if not ok:
            raise NotImplementedError(self.NOISE_RULE)
        cur.noise = l

    def noise_draw(self, ctx, noise, seed):
        """The pass's noise maps: drawn (None: one launch for all stages), handed in (a tensor [B, P]) or left out (False)."""
        ctx.noise_active = noise is not False
        if noise is None:
            ops.rng.normal(ctx.noise_flat, seed, counter=(self, "rng_offset"))
        elif noise is not False:
            self.noise_load(ctx, noise)

    def noise_load(self, ctx, noise):
        """Deals maps handed in as [B, P] (per sample, the stages' maps in network order) out to the stages' slices."""
        P = self.noise_pixels
        if tuple(noise.shape) != (ctx.B, P):
            raise ValueError(f"noise must be [{ctx.B}, {P}] (one value per pixel of the {sum(st.noise is not None for st in self.stages)} "
                             f"NoiseInjection maps, per sample, in network order), got {tuple(noise.shape)}")
        noise, o = noise.to(self.device, torch.float32), 0
        for i, st in enumerate(self.stages):
            if st.noise is not None:
                n = st.noise_pixels
                ctx.noise[i].view(ctx.B, n).copy_(noise[:, o:o + n])
                o += n

    def noise_add(self, ctx, i, st, z, alpha):
        """z = LeakyReLU_alpha(z + strength * noise) of stage i, in place."""
        return ops.noise.add(z, ctx.noise[i], st.noise.vars["noise_strength"], z, ctx.B * st.noise_pixels, st.out_shape[-1], lrelu_alpha=alpha)

    def noise_forward(self, ctx, i, st, xin, out):
        """A NoiseInjection stage without PixelNormalization: the conv (+ bias) into the stage's output, then the noise and the
        LeakyReLU in place on it."""
        self._conv(st, xin, out, False, EPI_NONE, bias=st.lin.vars.get("bias"))
        self.noise_add(ctx, i, st, out, st.alpha)

    def noise_backward(self, p, i, st, dzw):
        """The strength's gradient of stage i from ``dzw``, the gradient at the conv's output of the pass's first dw_rows samples (the
        add passes it on unchanged): one launch sequence with the pass's beta / scale.  A pass without noise leaves beta * old."""
        g = self.store.grad_of(st.noise, "noise_strength")
        if not p.ctx.noise_active:          # beta * old: nothing to launch where the pass accumulates (beta = 1)
            return g if p.beta == 1.0 else ops.fill(g, 0.0) if p.beta == 0.0 else ops.scale_(g, p.beta)
        R, Cc = p.dw_rows * st.noise_pixels, st.out_shape[-1]
        return ops.noise.grad(dzw, p.ctx.noise[i][:R], g, R, Cc, self.workspace(ops.noise.workspace_bytes(R, Cc)), beta=p.beta, scale=p.scale)

    # ---- StyleModulation (DESIGN.md §5 "Style modulation").  Public names for the reason the LayerNormalization helpers carry them:
    # no configuration of the engine-trace fixture has the layer; tests/test_modconv_cpu.py records what these enqueue.
    MOD_RULE = MOD_RULE

    @staticmethod
    def weight_layer(lin):
        """The layer that owns the derived weights of ``lin``: what a StyleModulation wraps (an EqualizedLearningRate keeps its c * W)
        where it wraps a wrapper, else ``lin`` itself."""
        return lin.layer if isinstance(lin, StyleModulation) and isinstance(lin.layer, EqualizedLearningRate) else lin

    def mod_place(self, flat_layers, idx, cur):
        """Net.__init__'s placement rule for the StyleModulation at ``flat_layers[idx]``, the linear layer of the new stage ``cur``:
        the network's input is the [L] style vector and another stage stands in front; everything else is refused.  (What may
        follow in the stage is checked as the layers arrive; what the wrapper may wrap, by the wrapper.)"""
        if len(self.in_shape) != 1 or len(self.stages) < 2 or cur.mod.style_dim != self.style_dim:
            raise NotImplementedError(MOD_RULE + " (a first stage has no style source: the only one is the network's [L] input)")

    def mod_geom(self, st):
        """(taps, I, O, transposed) of modulated stage ``st``'s kernel: [k, k, I, O], or [k, k, O, I] for a Conv2DTranspose."""
        return st.lin.k * st.lin.k, st.in_shape[-1], st.out_shape[-1], st.kind == "convT"

    def mod_update(self):
        """Q = sum over the taps of W_eff^2 of every demodulating layer, from the effective weights as they stand: one launch per
        layer, where prepare_weights refreshes the other derived weights (not per pass)."""
        for st in self.stages:
            if st.mod is not None and st.mod.demodulate:
                taps, I, O, tr = self.mod_geom(st)
                ops.modconv.wsq(self.store.kernel(st.lin), self.store.mod_q(st.lin), taps, I, O, transposed=tr)

    def mod_forward(self, ctx, i, st, xin, out):
        """A modulated stage: s = w . A + a, xs = x * s, the conv on xs; with demodulation z is kept, d = 1 / sqrt((s * s) . Q + eps)
        and out = LeakyReLU(d * z + bias), the stage's noise between the two where it has one; without, the conv writes out
        through its own epilogue.  The same in training and in inference."""
        B, v = ctx.B, st.lin.vars
        (Pi, Po), I, O = st.mod_pixels, st.in_shape[-1], st.out_shape[-1]
        s, xs = ctx.mod_s[i], ctx.mod_xs[i]
        ops.gemm(ctx.mod_w, v["style_kernel"], s, B, I, self.style_dim, bias=v["style_bias"])
        ops.modconv.scale(xin, s, xs, B, Pi, I)
        if not st.mod.demodulate:
            self._conv(st, xs, out, False, EPI_TANH if st.act == "tanh" else EPI_NONE)
            return
        z, d = ctx.z[i], ctx.mod_d[i]
        self._conv(st, xs, z, False, EPI_NONE)
        ops.modconv.demod(s, self.store.mod_q(st.lin), d, B, I, O, eps=st.mod.epsilon)
        noisy = st.noise is not None and ctx.noise_active
        ops.modconv.scale(z, d, out, B, Po, O, bias=v.get("bias"), lrelu_alpha=1.0 if noisy else st.alpha)
        if noisy: self.noise_add(ctx, i, st, out, st.alpha)      # noqa: E701

    def mod_backward(self, p, i, st, dy):
        """Stage i's backward from ``dy``, the gradient at d * z + bias (the activation backward left it in the stage's dz buffer):
        the bias and noise sums, dd = sum dy * z, dz = d * dy in place, the conv's two gradients on xs, ds = sum x * dxs, the
        demodulation's share of ds and of dW_eff, dx = s * dxs, and the style variables' gradients from ds.  Returns (dx, False):
        the stage below applies its own activation backward (ds needs the unmasked dxs, so nothing is fused into the data
        gradient).  The stage's slice goes to the reducer at the end: its last writer is here."""
        ctx, v = p.ctx, st.lin.vars
        B, L = ctx.B, self.style_dim
        if p.dw_rows != B: raise NotImplementedError("weight gradients from a part of the batch through a StyleModulation stage")      # noqa: E701
        (Pi, Po), I, O = st.mod_pixels, st.in_shape[-1], st.out_shape[-1]
        s, xs, xin, demod = ctx.mod_s[i], ctx.mod_xs[i], ctx.xin[i], st.mod.demodulate
        dd, dq, ds, s2, dQ = ctx.mod_scratch(i)
        g = self.store.grad_of
        dz = dy.view(B, *st.out_shape)
        if demod:
            d = ctx.mod_d[i]
            if p.need_dw:
                if st.noise is not None: self.noise_backward(p, i, st, dz)      # noqa: E701
                if "bias" in v:
                    ops.colsum(dz, g(st.lin, "bias"), B * Po, O, self.workspace(ops.colsum_workspace_bytes(B * Po, O)), beta=p.beta, scale=p.scale)
                ops.modconv.dot(dz, ctx.z[i], dd, B, Po, O, self.mod_dot_ws(B, Po, O))
            # in place, unless dy is the caller's own tensor (a last stage without activation)
            dz = ops.modconv.scale(dz, d, ctx.buf(ctx.dz, i), B, Po, O)
        if p.need_dw:
            self._filter_grad(st, xs, dz, p.beta, p.scale)
        below = ctx.gin if self.rereads_rows(self.stages[i - 1]) else ctx.dz
        tgt = ctx.buf(below, i - 1).view(B, *st.in_shape)
        self._conv(st, dz, tgt, True, EPI_NONE)
        if p.need_dw:
            ops.modconv.dot(xin, tgt, ds, B, Pi, I, self.mod_dot_ws(B, Pi, I))
            if demod:
                taps, _, _, tr = self.mod_geom(st)
                ops.modconv.demod_bwd(d, dd, s, self.store.mod_q(st.lin), dq, ds, B, I, O)
                ops.modconv.scale(s, s, s2, B, 1, I)
                ops.gemm(s2, dq, dQ, I, O, B, transA=True)
                ops.modconv.wsq_grad(self.store.kernel(st.lin), dQ, g(st.lin, "kernel"), taps, I, O, transposed=tr, scale=p.scale)
            ops.gemm(ctx.mod_w, ds, g(st.lin, "style_kernel"), L, I, B, transA=True, beta=p.beta, scale=p.scale)
            ops.colsum(ds, g(st.lin, "style_bias"), B, I, self.workspace(ops.colsum_workspace_bytes(B, I)), beta=p.beta, scale=p.scale)
            if self.has_mapping:        # this stage's share of dL/dw = ds . style_kernel^T; the first contributor of the pass overwrites
                ops.gemm(ds, v["style_kernel"], ctx.mod_dw, B, L, I, transB=True, beta=1.0 if p.dw_started else 0.0)
                p.dw_started = True
            if p.reducer is not None:
                p.reducer.ready(*self._train_range(st))
        ops.modconv.scale(tgt, s, tgt, B, Pi, I)
        return tgt, False

    def mod_dot_ws(self, B, P, Cc):
        nb = ops.modconv.dot_workspace_bytes(B, P, Cc)
        return self.workspace(nb) if nb else None

    # ---- MappingNetwork (DESIGN.md §5 "Mapping network").  Public names for the reason the LayerNormalization helpers carry them: no
    # configuration of the engine-trace fixture has the layer; tests/test_mapping_cpu.py holds the placement rules and the formulas,
    # tests/test_mapping_step_gpu.py what these compute.
    MAPPING_RULE = MAPPING_RULE

    def mapping_place(self, flat_layers, idx, cur):
        """Net.__init__'s placement rule for the MappingNetwork at ``flat_layers[idx]``: in front of the first stage, first in the
        network or directly behind the latents' PixelNormalization, once; everything else is refused."""
        l, s = flat_layers[idx]
        ok = (self.mapping is None and cur is None and self.blur is None and len(self.in_shape) == 1 and len(s) == 1
              and (idx == 0 or (idx == 1 and self.latent_pn is not None)))
        if not ok:
            raise NotImplementedError(MAPPING_RULE)
        self.mapping, self.style_dim = l, int(l.units_for(s))

    def mapping_check_call(self, ctx, inputs, w, truncation_psi, training):
        """The arguments of a forward that names ``w`` or ``truncation_psi``."""
        if not self.has_mapping:
            raise ValueError("forward(w=..., truncation_psi=...): this network has no MappingNetwork prefix")
        if w is not None and inputs is not None:
            raise ValueError("forward: either inputs (the latents z) or w (the styles, which skip the mapping network), not both")
        if w is not None and tuple(w.shape) != (ctx.B, self.style_dim):
            raise ValueError(f"forward: w must be [{ctx.B}, {self.style_dim}], got {tuple(w.shape)}")
        if truncation_psi is not None and training:
            raise ValueError("forward: truncation_psi is an inference-time trick; with training=True the backward would not see it")

    def mapping_forward(self, ctx, x):
        """w = the prefix on ``x`` (z, or the normalised latents): one launch per layer, every layer's output kept in ctx.map_h for
        the backward.  The same in training and in inference."""
        mp, B, U = self.mapping, ctx.B, self.style_dim
        x = ctx.map_in = x.view(B, self.in_shape[0])
        for l in range(mp.num_layers):
            K = self.in_shape[0] if l == 0 else U
            x = ops.mapping.dense_lrelu(x, mp.vars[f"kernel_{l}"], mp.vars[f"bias_{l}"], ctx.map_h[l], B, U, K, c=mp.coefficients[l],
                                        bias_mul=mp.bias_multiplier, alpha=mp.alpha)
        return x

    def mapping_truncate(self, ctx, w, psi):
        """The truncation trick on the pass's styles, into a buffer of the pass's own (the prefix's output stays as it is)."""
        if ctx.map_trunc is None:
            ctx.map_trunc = torch.empty((ctx.B, self.style_dim), dtype=torch.float32, device=self.device)
        return ops.mapping.truncate(w.view(ctx.B, self.style_dim), self.mapping.vars["w_avg"], ctx.map_trunc, float(psi), ctx.B, self.style_dim)

    def mapping_backward(self, p, st, dz, need_dx):
        """The end of a backward through a network with a mapping prefix, at its first stage (a Dense on w) with ``dz`` the gradient
        at that Dense's output: the Dense's data gradient is the LAST contribution to dL/dw in ctx.mod_dw, behind the modulated
        stages' (mod_backward); then the prefix from top to bottom: LeakyReLU' and the bias sums in one pass, the kernel gradient,
        the data gradient into the other [B, U] buffer (the bottom layer's into the pass's input gradient, only when ``need_dx``
        asks for dL/dz).  The prefix's slice goes to the reducer last.  Returns dL/dz or None."""
        ctx, mp = p.ctx, self.mapping
        B, U, L = ctx.B, self.style_dim, self.in_shape[0]
        if p.dw_rows != B: raise NotImplementedError("weight gradients from a part of the batch through a MappingNetwork")      # noqa: E701
        if not p.need_dw: raise NotImplementedError("the gradient at the input of a network with a MappingNetwork without its weight gradients (need_dw=False)")  # noqa: E701
        ops.gemm(dz.view(B, st.out_shape[0]), self.store.kernel(st.lin), ctx.mod_dw, B, U, st.out_shape[0], transB=True,
                 beta=1.0 if p.dw_started else 0.0)
        p.dw_started = True
        g, other = ctx.mod_dw, ctx.map_g
        grad = self.store.grad_of
        ws = self.workspace(ops.mapping.workspace_bytes(B, U))
        for l in range(mp.num_layers - 1, -1, -1):
            hin, K, c = (ctx.map_in, L, mp.coefficients[l]) if l == 0 else (ctx.map_h[l - 1], U, mp.coefficients[l])
            ops.mapping.lrelu_bias_bwd(g, ctx.map_h[l], g, grad(mp, f"bias_{l}"), B, U, ws, alpha=mp.alpha, beta=p.beta,
                                       scale=p.scale * mp.bias_multiplier)
            ops.gemm(hin, g, grad(mp, f"kernel_{l}"), K, U, B, transA=True, beta=p.beta, scale=p.scale * c)
            if l > 0 or need_dx:
                tgt = other if l > 0 else ctx.input_grad()
                ops.gemm(g, mp.vars[f"kernel_{l}"], tgt, B, K, U, transB=True, scale=c)
                g, other = tgt, g
        if p.reducer is not None:
            p.reducer.ready(*self.store.train_range(mp))
        p.release_deferred()
        return g if need_dx else None

    def w_avg_update(self, ctx, global_batch):
        """w_avg <- w_avg - (1 - beta) * (w_avg - mean of the pass's w over the GLOBAL batch): the column sums of this rank's w scaled
        by 1 / global batch, their sum over the ranks (one process: no collective), the running average: three launches, recorded
        in a step program like any other."""
        mp, B, U = self.mapping, ctx.B, self.style_dim
        if ctx.map_mean is None:
            ctx.map_mean = torch.empty(U, dtype=torch.float32, device=self.device)
        ops.colsum(ctx.map_h[-1], ctx.map_mean, B, U, self.workspace(ops.colsum_workspace_bytes(B, U)), scale=1.0 / float(global_batch))
        dist.all_reduce_sum_async(ctx.map_mean).wait()
        ops.ema(mp.vars["w_avg"], ctx.map_mean, None, None, 1.0 - mp.w_avg_beta)

    # ---- DiffAugment in front of stage 0 (DESIGN.md §5 "Augmentation").  Public names for the reason the LayerNormalization helpers
    # carry them: the engine-trace fixture's configurations run without augmentation; tests/test_diffaug_cpu.py records these.
    def aug_forward(self, ctx, x):
        """ctx.aug_input() = T(x) for the pass's (blurred) input batch ``x``: always a copy, with or without blur."""
        cfg, params = ctx.aug
        assert len(self.in_shape) == 3, "DiffAugment needs an [H, W, C] network input"
        gate = getattr(cfg, "gate", None)       # diffaugment.GatedAugment: rows of 12 uniforms, p read on the device
        if gate is not None:
            assert tuple(params.shape) == (ctx.B, 12), f"gated augmentation params {tuple(params.shape)} for a pass of {ctx.B} samples"
            return ops.diffaug.fwd_gated(x.view(ctx.B, *self.in_shape), ctx.aug_input(), params, gate, **cfg.kernel_args())
        assert tuple(params.shape) == (ctx.B, 8), f"augmentation params {tuple(params.shape)} for a pass of {ctx.B} samples"
        return ops.diffaug.fwd(x.view(ctx.B, *self.in_shape), ctx.aug_input(), params, **cfg.kernel_args())

    def aug_linear(self, cfg, params, v, out):
        """out = L v: the linear part of T for the rows ``params`` belongs to (the penalty's second-order seed)."""
        gate = getattr(cfg, "gate", None)
        if gate is not None:
            return ops.diffaug.fwd_gated(v.view(-1, *self.in_shape), out.view(-1, *self.in_shape), params, gate, **cfg.kernel_args(), linear=True)
        return ops.diffaug.fwd(v.view(-1, *self.in_shape), out.view(-1, *self.in_shape), params, **cfg.kernel_args(), linear=True)

    def aug_backward(self, ctx, g, dx_rows):
        """The end of a backward whose forward was augmented: L^T of the stage-0 input gradient ``g`` (all rows, or ``dx_rows``),
        then blur^T.  Stage 0 read ctx.aug_input(), so the blurred batch in ctx.a0 has been dead since the forward: L^T lands in
        its rows, and blur^T goes back into the rows of the input-gradient buffer ``g`` came in.  The augmented batch itself is
        left alone: the layer-1 filter gradients of the penalty (merged, or the LayerNormalization source backward) still read it."""
        cfg, params = ctx.aug
        lo, hi = (0, ctx.B) if dx_rows is None else dx_rows
        g = g.view(hi - lo, *self.in_shape)
        gate = getattr(cfg, "gate", None)
        if gate is not None:
            dx = ops.diffaug.adjoint_gated(g, ctx.a0[lo:hi], params[lo:hi], gate, **cfg.kernel_args())
        else:
            dx = ops.diffaug.adjoint(g, ctx.a0[lo:hi], params[lo:hi], **cfg.kernel_args())
        return dx if self.blur is None else self.apply_blur(dx, g)

    # ------------------------------------------------------------------ GP second order
    def _gp_kinds(self):
        """What the linearised forward of the gradient penalty does per stage; refuses any but the reference critic shape."""
        kinds = []
        for i, st in enumerate(self.stages):
            last = i == len(self.stages) - 1
            if st.kind == "mbstd": kinds.append("mbstd"); continue      # noqa: E701,E702  (its place in the network: mbstd_check_position)
            if st.kind == "conv" and st.bn is None and st.act == "lrelu" and not last:
                kinds.append("conv" if st.ln is None else "ln")
            elif st.kind == "dense" and last and st.out_shape == (1,) and st.bn is None and st.act is None:
                kinds.append("dense")
            elif st.kind in RESAMPLE and not last:
                kinds.append("resample")
            else:
                raise NotImplementedError(_GP_SHAPE_MESSAGE)
        return kinds

    def _gp_stage(self, kind, st, wx, wdz, wbeta, v, ref, vout, reducer):
        """One stage of the penalty's second order: the filter gradient wgrad(wx, wdz) into store.grad (beta = ``wbeta``), then the
        linearised forward vout = op(v) with the LeakyReLU signs of ``ref`` frozen.  The Dense(1) head's is the column sum of v."""
        if kind == "resample":
            self._resample(st, v, vout)
            return
        if kind == "conv":
            self._filter_grad(st, wx, wdz, wbeta, 1.0)
        else:
            n, K = v.size(0), st.in_shape[0]
            ws = self.workspace(ops.colsum_workspace_bytes(n, K))
            ops.colsum(v.reshape(n, K), self.store.grad_of(st.lin, "kernel").view(K), n, K, ws, beta=1.0, scale=1.0)
        if reducer is not None:     # this layer's gradient (first-order pass + this wgrad) is complete
            reducer.ready(*self.store.train_range(st.lin, st.bn))
        if kind == "conv":
            self._conv(st, v, vout, False, EPI_MUL_GRAD, ref=ref, alpha=st.alpha)

    def gp_second_order_merged(self, ctx: Context, lo, hi, reducer=None):
        """The second order of the penalty AND the filter gradients of the whole merged critic pass, one launch per layer.

        The first-order gradient of layer i is wgrad(x = a_{i-1}[rows of fakes, reals], dy = dz_i[same rows]); the penalty adds
        wgrad(x = delta-bar_{i-1}, dy = zeta_i) over the x-hat rows (GP derivation step 2).  Rows are the
        contraction index, so with delta-bar_{i-1} written INTO the x-hat rows [lo, hi) of the pass's activation buffer a_{i-1}
        -- dead after the backward except for their signs, which the linearised forward consumes as it overwrites them in
        place -- both are ONE filter gradient over all 3B rows of (a_{i-1}, dz_i): five launches (and their slab reduces)
        fewer per D-step, and the remaining ones run at 3B rows instead of 2B + B.  The caller has put delta-bar_0 into
        ctx.a0[lo:hi] and run ``backward(..., defer_conv_dw=True)``.

        Not with LayerNormalization stages: their source backward (gp_ln_source_backward) needs the x-hat rows of the activations
        this pass overwrites, so such a critic takes ``gp_second_order`` on ``ctx.rows(lo, hi)``."""
        if self.has_mod: raise NotImplementedError("StyleModulation in a critic under the gradient penalty is not built")  # noqa: E701
        if self.has_pn: raise NotImplementedError("PixelNormalization in a critic under the gradient penalty is not built")  # noqa: E701
        if self.has_noise: raise NotImplementedError("NoiseInjection in a critic under the gradient penalty is not built")  # noqa: E701
        kinds = self._gp_kinds()
        if set(kinds) & set(SOURCE_KINDS): raise NotImplementedError("gp_second_order_merged overwrites activations the LayerNormalization / MinibatchStdDev source backward needs")  # noqa: E701
        self.store.ensure_opt_state()
        for i, (kind, st) in enumerate(zip(kinds, self.stages)):
            xin = ctx.xin[i]                # [3B, ...]: activations of [fakes; reals], delta-bar_{i-1} in the x-hat rows
            ah = ctx.a[i][lo:hi]            # delta-bar_i goes where the x-hat rows of a_i are: in place, ref == out
            if self.capture_branches is not None and kind == "conv":      # test instrumentation: the signs about to be overwritten
                self.capture_branches.append((ah > 0).cpu().numpy())
            self._gp_stage(kind, st, xin, ctx.dz[i], 0.0, xin[lo:hi], ah, ah, reducer)

    def gp_second_order(self, ctx: Context, v0, reducer=None):
        """SURVEY.md 8a, GP derivation step 2: one linearised forward of the critic on ``v0`` with the
        LeakyReLU masks of the x-hat pass frozen, plus one wgrad per conv layer against the zeta_i kept by
        the first-order backward (``ctx.dz``); accumulates into ``store.grad`` (beta = 1).

        A LayerNormalization stage is not piecewise linear: its tangent is gp_ln_stage's, and what the linearised forward's
        dependence on the stage's PRIMAL input adds goes down the network once more in gp_ln_source_backward.  That pass writes the
        last contribution to every layer up to the top-most such stage, so those layers' slices go to the reducer from there."""
        if self.has_mod: raise NotImplementedError("StyleModulation in a critic under the gradient penalty is not built")  # noqa: E701
        if self.has_pn: raise NotImplementedError("PixelNormalization in a critic under the gradient penalty is not built")  # noqa: E701
        if self.has_noise: raise NotImplementedError("NoiseInjection in a critic under the gradient penalty is not built")  # noqa: E701
        kinds = self._gp_kinds()
        self.store.ensure_opt_state()
        top = max((i for i, k in enumerate(kinds) if k in SOURCE_KINDS), default=-1)
        v = v0
        for i, (kind, st) in enumerate(zip(kinds, self.stages)):
            vin = v.view(ctx.B, *st.in_shape)
            v = None if kind == "dense" else ctx.buf(ctx.v, i)
            stage = self._gp_stage if kind not in SOURCE_KINDS else functools.partial(getattr(self, f"gp_{kind}_stage"), ctx, i)
            stage(kind, st, vin, ctx.dz[i], 1.0, vin, ctx.a[i], v, reducer if i > top else None)
        self.gp_ln_source_backward(ctx, top, reducer)

    # ---- LayerNormalization in the penalty (DESIGN.md §5 "Penalty with LayerNormalization stages").  These helpers, like
    # ln_forward / ln_backward above, carry public names: the engine-trace fixture asks that its configurations -- none has such a
    # stage -- execute every line of Net's private helpers; tests/test_layernorm_cpu.py records what they enqueue instead.
    def gp_ln_stage(self, ctx, i, kind, st, wx, wdz, wbeta, v, ref, vout, reducer):
        """_gp_stage for a Conv2D + LayerNormalization stage: the filter gradient wgrad(wx, zeta_i) as for any conv, the tangent
        zdot_i = conv(v) (kept), vout = LeakyReLU' * gamma * M(zdot_i), and the source: s_i = dT/dz_i (kept) with
        dgamma_i += sum u_i * M(zdot_i).  Nothing goes to the reducer here: gp_ln_source_backward still writes into the slice."""
        assert reducer is None and ctx.u[i] is not None and ctx.u_rows == (0, ctx.B), "backward(keep_u_rows=...) has not kept u for these rows"
        self._filter_grad(st, wx, wdz, wbeta, 1.0)
        zdot, s = ctx.buf(ctx.zdot, i), ctx.buf(ctx.s, i)
        self._conv(st, v, zdot, False, EPI_NONE)
        args = self.ln_args(ctx, i, st)
        ops.layernorm.tangent(zdot, ctx.z[i], vout, **args, beta=st.ln.vars["beta"], lrelu_alpha=st.alpha)
        ops.layernorm.gp_source(ctx.u[i], zdot, ctx.z[i], s, **args, dgamma=self.store.grad_of(st.ln, "gamma"),
                                ws=self.workspace(ops.layernorm.workspace_bytes(args["R"], args["Cc"])))

    def gp_ln_source_backward(self, ctx, top, reducer=None):
        """An ordinary first-order backward over the x-hat rows that starts at the top-most LayerNormalization stage ``top`` with
        lambda_z = s_top and picks up s_i at every such stage below: filter and bias gradients against the PRIMAL inputs, the
        stages' gamma / beta gradients, all accumulated into store.grad (beta = 1).  The tangent buffers ctx.v are dead by now and
        carry the gradient down.  Each layer's slice goes to the reducer behind the last launch that writes into it."""
        lam = None if top < 0 else ctx.s[top]
        if top >= 0 and self.stages[top].kind == "mbstd":
            # a MinibatchStdDev stage's source is a gradient at its primal INPUT, the output of the stage below: through that
            # stage's activation (and its own source), then down from there
            top -= 1
            lam = self.gp_source_below(ctx, top, lam, False)
        for i in range(top, -1, -1):
            st, prev = self.stages[i], self.stages[i - 1] if i > 0 else None
            if st.kind not in RESAMPLE:
                self._filter_grad(st, ctx.xin[i], lam, 1.0, 1.0)
                if "bias" in st.lin.vars:
                    N = st.out_shape[-1]
                    rows = lam.numel() // N
                    ops.colsum(lam, self.store.grad_of(st.lin, "bias"), rows, N, self.workspace(ops.colsum_workspace_bytes(rows, N)), beta=1.0, scale=1.0)
                if reducer is not None:
                    reducer.ready(*self._train_range(st))
            if i == 0:
                break
            tgt = ctx.v[i - 1].view(ctx.B, *st.in_shape)
            fuse = prev.fusable_grad and st.kind not in UPSAMPLERS
            if st.kind in RESAMPLE:
                self.resample_transposed(st, lam, tgt, **(dict(ref=ctx.a[i - 1], alpha=prev.alpha) if fuse else {}))
            elif fuse:
                self._conv(st, lam, tgt, True, EPI_MUL_GRAD, ref=ctx.a[i - 1], alpha=prev.alpha)
            else:
                self._conv(st, lam, tgt, True, EPI_NONE)
            lam = self.gp_source_below(ctx, i - 1, tgt, fuse)

    def gp_source_below(self, ctx, j, tgt, fused):
        """The source backward through stage j's activation: ``tgt`` is the gradient at its output (``fused``: LeakyReLU' is in it
        already); returns the gradient at its linear op's output, with the stage's own source term where it has one."""
        prev = self.stages[j]
        if prev.ln is not None:
            # LeakyReLU' and the LayerNormalization backward of the stage, plus its own source term
            args = self.ln_args(ctx, j, prev)
            # in place where the kernel allows it, else into the stage's tangent buffer, dead since its source was taken
            out = tgt if ops.layernorm.route(args["Cc"])["chunks"] == 1 else ctx.zdot[j]
            return ops.layernorm.bwd(tgt, ctx.z[j], out, **args, beta=prev.ln.vars["beta"], lrelu_alpha=prev.alpha,
                                     addend=ctx.s[j], dgamma=self.store.grad_of(prev.ln, "gamma"), dbeta=self.store.grad_of(prev.ln, "beta"),
                                     acc_beta=1.0, acc_scale=1.0, ws=self.workspace(ops.layernorm.workspace_bytes(args["R"], args["Cc"])))
        if prev.kind not in RESAMPLE and not fused:      # conv + LeakyReLU below an UpSampling2D (or a MinibatchStdDev): no launch to fuse it into
            ops.mul_grad(tgt, ctx.a[j], tgt, alpha=prev.alpha)
        return tgt

    # ---- MinibatchStdDev (DESIGN.md §5 "Minibatch standard deviation").  Public names for the reason the LayerNormalization helpers
    # carry them: no configuration of the engine-trace fixture has the layer; tests/test_mbstd_cpu.py records what these enqueue.
    def check_rows(self, rows):
        """A pass (or a slice of one) of ``rows`` samples must hold whole groups of every MinibatchStdDev layer; checked once per
        size, on the host."""
        if self.mbstd_layers and rows not in self._rows_checked:
            for l in self.mbstd_layers:
                l.check_rows(rows)
            self._rows_checked.add(rows)

    @staticmethod
    def mbstd_check_position(flat_layers, idx, cur):
        """The layer stands directly before the critic's Flatten -> Dense(1), behind the last conv stage's LeakyReLU / Dropout /
        AveragePooling2D; anywhere else (a generator included) it is refused."""
        tail = [l for l, _ in flat_layers[idx + 1:]]
        head = (len(tail) == 2 and tail[0].kind == "flatten" and tail[1].kind == "dense" and tail[1].units == 1
                and getattr(tail[1], "activation", None) is None)
        below = cur is not None and (cur.kind in ("avgpool", "firdown") or (cur.kind == "conv" and cur.bn is None and cur.act == "lrelu"))
        if not (head and below):
            raise NotImplementedError("MinibatchStdDev is supported directly before the critic's Flatten -> Dense(1) only, behind the last "
                                      "conv stage's LeakyReLU / Dropout / AveragePooling2D (not in a generator, not in front of a conv)")

    def mbstd_args(self, ctx, i, st):
        nb = ops.mbstd.workspace_bytes(ctx.B, st.lin.group_size, st.ln_pixels, st.in_shape[-1])
        return dict(G=st.lin.group_size, eps=st.lin.epsilon, ws=self.workspace(nb) if nb else None)

    def mbstd_forward(self, ctx, i, st, xin, out):
        """out = xin with the groups' statistic as one more channel; the groups' mu and 1 / s stay in ctx.mbstd_stats(i)."""
        mu, rs, f = ctx.mbstd_stats(i)[:3]
        return ops.mbstd.fwd(xin, out, mu, rs, f, **self.mbstd_args(ctx, i, st))

    def mbstd_backward(self, p, i, st, prev, dz):
        """_input_grad of a MinibatchStdDev stage: the gradient at its input into the buffer the stage below reads its output
        gradient from (that stage's LeakyReLU' / Dropout' follow in its own launch); the groups' q stays for the penalty's source."""
        ctx = p.ctx
        below = ctx.gin if self.rereads_rows(prev) else ctx.dz
        tgt = ctx.buf(below, i - 1).view(ctx.B, *st.in_shape)
        mu, rs, _, q = ctx.mbstd_stats(i)[:4]
        ops.mbstd.bwd(dz.view(ctx.B, *st.out_shape), ctx.xin[i], mu, rs, tgt, q, st.lin.group_size)
        return tgt, False

    def gp_mbstd_stage(self, ctx, i, kind, st, wx, wdz, wbeta, v, ref, vout, reducer):
        """_gp_stage for a MinibatchStdDev stage, one launch: the tangent vout (v with the groups' fdot as the new channel) and the
        source (kept in ctx.s[i]): the derivative of <v, J(x)^T u> w.r.t. the stage's primal input, u the first-order gradient the
        backward of these rows saw (its q).  Nothing to hand to the reducer: the stage has no variables."""
        assert reducer is None
        mu, rs, _, q = ctx.mbstd_stats(i)[:4]
        src, fdot = ctx.mbstd_source(i)
        ops.mbstd.gp(v, ctx.xin[i], mu, rs, q, vout, src, fdot, **self.mbstd_args(ctx, i, st))
