"""Keras-shaped layer descriptions and ``Sequential`` container.

Stands in for ``tensorflow.keras.layers`` / ``tf.keras.Sequential`` as the reference demos use them
(demo_celeba.py:51-124, demo_mnist.py:48-86): same class names, constructor arguments, ``add``,
``output_shape`` / ``input_shape``, ``count_params``, ``summary``, ``trainable_variables``,
``get_weights`` / ``set_weights``, call with ``training=``.  The layers hold no arithmetic: a
``Sequential`` is compiled into fused stages and executed by ``engine.Net`` on the HIP kernels.

Parameters of one top-level model live in ONE flat float32 HBM buffer (``ParamStore.theta``) so the
optimiser is a single fused Adam launch and data-parallel training is a single all-reduce; each
Keras variable is a view into it, stored exactly in TF's layout (Dense [in,out], Conv2D
[kh,kw,Cin,Cout], Conv2DTranspose [kh,kw,Cout,Cin]).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

_seed_state = {"seed": 0, "rng": np.random.default_rng(0)}


def set_seed(seed: int):
    """Counterpart of ``tf.random.set_seed`` (demo_mnist.py:96) for weight init and the step RNG."""
    _seed_state["seed"] = int(seed)
    _seed_state["rng"] = np.random.default_rng(int(seed))


def get_seed() -> int:
    return _seed_state["seed"]


def default_device():
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class Layer:
    kind = "layer"

    def __init__(self, input_shape=None, name=None, **kw):
        self._declared_input_shape = tuple(input_shape) if input_shape is not None else None
        self.name = name or self.__class__.__name__.lower()
        self.trainable = True
        self.vars = {}          # name -> torch view into the store (set by ParamStore.bind)

    # (name, shape, trainable, init) for an input shape (without batch)
    def var_specs(self, in_shape):
        return []

    def out_shape(self, in_shape):
        return tuple(in_shape)

    def count_params(self):
        return sum(int(v.numel()) for v in self.vars.values())


def _glorot(shape, fan_in, fan_out):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return lambda rng: rng.uniform(-lim, lim, shape).astype(np.float32)


_zeros = lambda shape: (lambda rng: np.zeros(shape, np.float32))
_ones = lambda shape: (lambda rng: np.ones(shape, np.float32))


class Dense(Layer):
    kind = "dense"

    def __init__(self, units, activation=None, use_bias=True, **kw):
        super().__init__(**kw)
        if activation not in (None, "linear"):
            raise NotImplementedError("Dense activation other than linear is not on the reference path")
        self.units, self.use_bias = int(units), bool(use_bias)

    def out_shape(self, in_shape):
        return (self.units,)

    def var_specs(self, in_shape):
        fan_in = int(in_shape[-1])
        specs = [("kernel", (fan_in, self.units), True, _glorot((fan_in, self.units), fan_in, self.units))]
        if self.use_bias:
            specs.append(("bias", (self.units,), True, _zeros((self.units,))))
        return specs


class _ConvBase(Layer):
    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", use_bias=True, activation=None, **kw):
        super().__init__(**kw)
        kh, kw_ = _pair(kernel_size)
        sh, sw = _pair(strides)
        if kh != kw_ or sh != sw:
            raise NotImplementedError("only square kernels / equal strides are on the reference path")
        if str(padding).lower() != "same":
            raise NotImplementedError("only padding='same' is on the reference path (demo_celeba.py:62-119)")
        if activation not in (None, "linear", "tanh"):
            raise NotImplementedError(f"activation {activation!r} is not on the reference path")
        self.filters, self.k, self.stride = int(filters), int(kh), int(sh)
        self.use_bias = bool(use_bias)
        self.activation = None if activation in (None, "linear") else activation


class Conv2D(_ConvBase):
    kind = "conv"

    def out_shape(self, s):
        return (-(-s[0] // self.stride), -(-s[1] // self.stride), self.filters)

    def var_specs(self, s):
        cin, k, f = int(s[2]), self.k, self.filters
        specs = [("kernel", (k, k, cin, f), True, _glorot((k, k, cin, f), k * k * cin, k * k * f))]
        if self.use_bias:
            specs.append(("bias", (f,), True, _zeros((f,))))
        return specs


class Conv2DTranspose(_ConvBase):
    kind = "convT"

    def out_shape(self, s):
        return (s[0] * self.stride, s[1] * self.stride, self.filters)

    def var_specs(self, s):
        cin, k, f = int(s[2]), self.k, self.filters
        specs = [("kernel", (k, k, f, cin), True, _glorot((k, k, f, cin), k * k * f, k * k * cin))]
        if self.use_bias:
            specs.append(("bias", (f,), True, _zeros((f,))))
        return specs


class BatchNormalization(Layer):
    kind = "bn"

    def __init__(self, momentum=0.99, epsilon=1e-3, **kw):
        super().__init__(**kw)
        self.momentum, self.epsilon = float(momentum), float(epsilon)

    def var_specs(self, s):
        c = int(s[-1])
        return [("gamma", (c,), True, _ones((c,))), ("beta", (c,), True, _zeros((c,))),
                ("moving_mean", (c,), False, _zeros((c,))), ("moving_variance", (c,), False, _ones((c,)))]


class LayerNormalization(Layer):
    """tf.keras.layers.LayerNormalization over the channel axis of an [H, W, C] map: each pixel's C channels are normalised with
    their biased variance, n = gamma * (z - mean) / sqrt(var + epsilon) + beta (the WGAN-GP critic's normalisation)."""
    kind = "layernorm"

    def __init__(self, axis=-1, epsilon=1e-3, center=True, scale=True, **kw):
        super().__init__(**kw)
        ax = tuple(axis) if isinstance(axis, (list, tuple)) else (axis,)
        if len(ax) != 1 or ax[0] not in (-1, 3):
            raise NotImplementedError(f"LayerNormalization axis {axis!r}: only the last axis of an [H, W, C] map (-1 or 3) is supported")
        if not center or not scale:
            raise NotImplementedError("LayerNormalization with center=False or scale=False is not supported")
        self.axis, self.epsilon, self.center, self.scale = -1, float(epsilon), True, True

    def out_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError(f"LayerNormalization needs an [H, W, C] map, got {tuple(s)}")
        return tuple(s)

    def var_specs(self, s):
        self.out_shape(s)
        c = int(s[-1])
        return [("gamma", (c,), True, _ones((c,))), ("beta", (c,), True, _zeros((c,)))]


class PixelNormalization(Layer):
    """The pixel-wise feature normalisation of ProGAN / StyleGAN generators (Karras et al. 2018): every pixel's C channels -- the last
    axis of an [H, W, C] map, or a [C] latent vector -- are divided by their root mean square, y = a / sqrt(mean_c(a^2) + epsilon).
    No variables and no state; the same in training and in inference, and nothing couples the samples of a batch.  It stands
    directly behind the LeakyReLU of a generator stage (in place of BatchNormalization in front of it), or first in the network,
    where it normalises the latents."""
    kind = "pixelnorm"

    def __init__(self, epsilon=1e-8, **kw):
        super().__init__(**kw)
        if not float(epsilon) > 0.0:
            raise ValueError(f"PixelNormalization epsilon={epsilon!r}: must be positive")
        self.epsilon = float(epsilon)

    def out_shape(self, s):
        if len(s) not in (1, 3):
            raise NotImplementedError(f"PixelNormalization needs an [H, W, C] map or a [C] vector, got {tuple(s)}")
        return tuple(s)


class NoiseInjection(Layer):
    """The per-pixel noise input of a StyleGAN synthesis layer (Karras et al. 2019, 2020): ``strength * N(0, 1)`` is added to every
    pixel of an [H, W, C] map, one draw per pixel broadcast over the channels, with ONE learned scalar ``noise_strength`` that
    starts at zero (StyleGAN2's; StyleGAN1's per-channel strengths are not built).  It stands directly behind a Conv2D or
    Conv2DTranspose (its bias included), in front of the stage's LeakyReLU, in the generator only.  The same in training and in
    inference: every forward draws fresh noise unless it is handed maps or told to leave the noise out
    (``engine.Net.forward(noise=...)``)."""
    kind = "noise"

    def out_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError(f"NoiseInjection needs an [H, W, C] map, got {tuple(s)}")
        return tuple(s)

    def var_specs(self, s):
        self.out_shape(s)
        return [("noise_strength", (1,), True, _zeros((1,)))]


def _normalize(x):
    """x / max(||x||, 1e-12): the normalisation of the power iteration."""
    return x / max(float(np.linalg.norm(x)), 1e-12)


class SpectralNormalization(Layer):
    """tf.keras.layers.SpectralNormalization(layer, power_iterations=1) around a Conv2D, Conv2DTranspose or Dense (Miyato et al.
    2018).  The layer's kernel, viewed as the matrix W = reshape(kernel, [-1, shape[-1]]), is divided by sigma, its largest singular
    value as a running power iteration estimates it; ``vector_u``, ``vector_v`` and ``sigma`` are non-trainable state behind the
    layer's own variables.  In a Sequential the wrapper stands for the layer it wraps: same kind, shapes, variables and fusion.
    One power round runs per optimizer step of the model, at the start of that step; every other use of changed weights refreshes
    sigma = v^T W u alone (DESIGN.md section 5 "Spectral normalisation")."""

    def __init__(self, layer, power_iterations=1, **kw):
        if isinstance(layer, EqualizedLearningRate):
            raise NotImplementedError("SpectralNormalization around an EqualizedLearningRate: W / sigma cancels the run-time coefficient c")
        if not isinstance(layer, (Conv2D, Conv2DTranspose, Dense)):
            raise NotImplementedError(f"SpectralNormalization wraps a Conv2D, a Conv2DTranspose or a Dense, not {type(layer).__name__}")
        if int(power_iterations) < 1:
            raise ValueError(f"power_iterations={power_iterations!r}: at least one power round per step")
        kw.setdefault("input_shape", layer._declared_input_shape)
        kw.setdefault("name", "spectral_normalization_" + layer.name)
        super().__init__(**kw)
        self.layer, self.power_iterations = layer, int(power_iterations)
        self.kind = layer.kind
        layer.vars = self.vars      # one set of variables, reachable through either object

    def __getattr__(self, name):    # what the wrapper does not have itself (filters, k, stride, units, activation, ...) is the layer's
        if name == "layer" or name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.layer, name)

    def out_shape(self, in_shape):
        return self.layer.out_shape(in_shape)

    @staticmethod
    def matrix_shape(kernel_shape):
        """(K, N, taps) of a kernel variable: the row-major matrix [K, N] = reshape(kernel, [-1, shape[-1]]), K = taps * R."""
        n = int(kernel_shape[-1])
        k = int(np.prod(kernel_shape)) // n
        return k, n, (int(kernel_shape[0]) * int(kernel_shape[1]) if len(kernel_shape) == 4 else 1)

    def var_specs(self, in_shape):
        specs = list(self.layer.var_specs(in_shape))
        K, N, _ = self.matrix_shape(specs[0][1])
        u0 = lambda rng: _normalize(rng.normal(0.0, 0.02, (N,))).astype(np.float32)
        # vector_v and sigma follow from W and u0: ParamStore sets them once the kernel has its initial value
        return specs + [("vector_u", (N,), False, u0), ("vector_v", (K,), False, _zeros((K,))), ("sigma", (1,), False, _ones((1,)))]

    def init_state(self):
        """v0 = normalize(W u0), sigma = v0^T W u0 from the initial kernel and u0, on the host."""
        W = self.vars["kernel"].detach().cpu().numpy().astype(np.float64).reshape(-1, self.vars["kernel"].shape[-1])
        u = self.vars["vector_u"].detach().cpu().numpy().astype(np.float64)
        v = _normalize(W @ u)
        self.vars["vector_v"].copy_(torch.from_numpy(v.astype(np.float32)))
        self.vars["sigma"].copy_(torch.from_numpy(np.array([v @ W @ u], dtype=np.float32)))


class EqualizedLearningRate(Layer):
    """The equalised learning rate of ProGAN / StyleGAN (Karras et al. 2018) around a Conv2D, Conv2DTranspose or Dense: the kernel is
    drawn from N(0, 1) and the network computes with W_eff = c * W, c = gain / sqrt(fan_in) a constant of the layer, so the optimizer
    sees dL/dW = c * dL/dW_eff and every layer's weights have the same dynamic range.  fan_in = k * k * (input channels): shape[0]
    of a Dense kernel, k * k * shape[2] of a Conv2D's, k * k * shape[3] of a Conv2DTranspose's ([k, k, Cout, Cin]: ProGAN's
    ``upscale2d_conv2d`` rule).  The bias starts at zero and is not scaled.  In a Sequential the wrapper stands for the layer it
    wraps, as SpectralNormalization does: same kind, shapes, fusion and variables, and no state of its own (DESIGN.md section 5
    "Equalised learning rate").  ``coefficient``: the fp32 value of c as a Python float, known once the input shape is."""

    def __init__(self, layer, gain=math.sqrt(2), **kw):
        if isinstance(layer, SpectralNormalization):
            raise NotImplementedError("EqualizedLearningRate around a SpectralNormalization: W / sigma cancels the run-time coefficient c")
        if not isinstance(layer, (Conv2D, Conv2DTranspose, Dense)):
            raise NotImplementedError(f"EqualizedLearningRate wraps a Conv2D, a Conv2DTranspose or a Dense, not {type(layer).__name__}")
        if isinstance(gain, bool) or not isinstance(gain, (int, float, np.integer, np.floating)) or not (math.isfinite(gain) and gain > 0):
            raise ValueError(f"EqualizedLearningRate gain={gain!r}: must be a positive finite number")
        kw.setdefault("input_shape", layer._declared_input_shape)
        kw.setdefault("name", "equalized_learning_rate_" + layer.name)
        super().__init__(**kw)
        self.layer, self.gain = layer, float(gain)
        self.kind = layer.kind
        self.fan_in = self.coefficient = None
        layer.vars = self.vars      # one set of variables, reachable through either object

    def __getattr__(self, name):    # what the wrapper does not have itself (filters, k, stride, units, activation, ...) is the layer's
        if name == "layer" or name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.layer, name)

    def out_shape(self, in_shape):
        self._set_coefficient(in_shape)
        return self.layer.out_shape(in_shape)

    @staticmethod
    def fan_in_of(kind, kernel_shape):
        """k * k * (input channels) of a kernel variable of a layer of ``kind``."""
        sh = tuple(int(v) for v in kernel_shape)
        return sh[0] if kind == "dense" else sh[0] * sh[1] * sh[3 if kind == "convT" else 2]

    def _set_coefficient(self, in_shape):
        cin = int(in_shape[-1])
        self.fan_in = cin if self.kind == "dense" else self.layer.k * self.layer.k * cin
        self.coefficient = float(np.float32(self.gain / math.sqrt(self.fan_in)))      # in double, rounded to fp32 once

    def var_specs(self, in_shape):
        specs = list(self.layer.var_specs(in_shape))
        shape = specs[0][1]
        self._set_coefficient(in_shape)
        assert self.fan_in == self.fan_in_of(self.kind, shape), (self.fan_in, shape)
        normal = lambda rng: rng.standard_normal(shape).astype(np.float32)
        return [("kernel", shape, True, normal)] + specs[1:]         # the bias keeps its zeros


MOD_RULE = ("StyleModulation wraps a Conv2D, a Conv2DTranspose or an EqualizedLearningRate around one of them (not a Dense, not a "
            "SpectralNormalization in either nesting), in a generator whose input is the [L] style vector and behind at least one other "
            "stage, in a stage without BatchNormalization, LayerNormalization, PixelNormalization or Dropout; demodulate=True not with "
            "tanh, demodulate=False not with a bias")


class StyleModulation(Layer):
    """StyleGAN2's modulated convolution (Karras et al. 2020) around a Conv2D, a Conv2DTranspose or an EqualizedLearningRate around
    one of them: a learned affine map of the network's input vector w [L] gives one style per input channel, s = w . style_kernel +
    style_bias, which scales the layer's input map per sample; with ``demodulate`` the output is divided by the norm the scaled
    weights would have, d = 1 / sqrt((s * s) . sum_taps W_eff^2 + epsilon), in place of a normalisation layer, and the bias follows.
    The un-fused form of the paper: the activations are scaled, not the weights.  In a Sequential the wrapper stands for its layer,
    as EqualizedLearningRate does: same kind, shapes, ``kernel`` and ``bias``; it adds the trainables ``style_kernel`` [L, I] (Glorot
    uniform) and ``style_bias`` [I] (ones).  L is the model's input size, known once the wrapper is part of a model with an input
    shape, or the ``units`` of the ``MappingNetwork`` the model starts with: then w is that layer's output and the gradient with
    respect to w runs back into it (DESIGN.md section 5 "Style modulation", "Mapping network")."""

    def __init__(self, layer, demodulate=True, epsilon=1e-8, **kw):
        inner = layer.layer if isinstance(layer, EqualizedLearningRate) else layer
        if isinstance(layer, SpectralNormalization) or isinstance(inner, SpectralNormalization) or not isinstance(inner, (Conv2D, Conv2DTranspose)):
            raise NotImplementedError(MOD_RULE + f" (got a {type(layer).__name__}"
                                      + (f" around a {type(inner).__name__})" if inner is not layer else ")"))
        if not float(epsilon) > 0.0:
            raise ValueError(f"StyleModulation epsilon={epsilon!r}: must be positive")
        self.demodulate, self.epsilon = bool(demodulate), float(epsilon)
        if self.demodulate and inner.activation == "tanh":
            raise NotImplementedError(MOD_RULE + " (demodulate=True in a stage with tanh)")
        if not self.demodulate and inner.use_bias:
            raise NotImplementedError(MOD_RULE + " (demodulate=False with a bias)")
        kw.setdefault("input_shape", layer._declared_input_shape)
        kw.setdefault("name", "style_modulation_" + layer.name)
        super().__init__(**kw)
        self.layer = layer
        self.kind = layer.kind
        self.style_dim = None       # L: set by the Sequential that holds the wrapper (flat_layers)
        self.vars = layer.vars      # one set of variables, reachable through every object of the nesting

    def __getattr__(self, name):    # what the wrapper does not have itself (filters, k, stride, activation, coefficient, ...) is the layer's
        if name == "layer" or name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.layer, name)

    def out_shape(self, in_shape):
        return self.layer.out_shape(in_shape)

    def var_specs(self, in_shape):
        if self.style_dim is None:
            raise NotImplementedError(MOD_RULE + " (the model's input is no [L] vector: there is no style source)")
        specs = list(self.layer.var_specs(in_shape))
        L, I = int(self.style_dim), int(in_shape[-1])
        return specs + [("style_kernel", (L, I), True, _glorot((L, I), L, I)), ("style_bias", (I,), True, _ones((I,)))]


MAPPING_RULE = ("MappingNetwork is supported as the first layer of a generator whose input is an [L] vector, or directly behind the leading "
                "PixelNormalization of normalize_latents=True, once per model: not in a critic, not behind a stage, not twice")


class MappingNetwork(Layer):
    """StyleGAN's mapping network ``G_mapping`` (Karras et al. 2019): ``num_layers`` Dense layers z [L] -> w [units] (``units=None``: L),
    h_{l+1} = LeakyReLU_alpha(c_l * (h_l . kernel_l) + m * bias_l), the activation behind every layer, the last one included.  One
    layer object: ``kernel_0 .. kernel_{n-1}`` ([L, U], then [U, U]), ``bias_0 .. bias_{n-1}`` ([U]) and the non-trainable running
    mean ``w_avg`` [U] of the G-steps' w (zeros at the start; decay ``w_avg_beta``), which the truncation trick reads.  With
    ``equalized_lr`` the kernels are drawn from N(0, 1) / lr_multiplier, c_l = sqrt(2) / sqrt(fan_in) * lr_multiplier and m =
    lr_multiplier (StyleGAN's ``mapping_lrmul``: the optimizer sees a learning rate lr_multiplier times smaller); without, Glorot
    uniform kernels and c_l = m = 1.  ``coefficients`` / ``bias_multiplier``: the fp32 values as Python floats, known once the input
    shape is (as ``EqualizedLearningRate.coefficient``); they travel by value in the kernel arguments, not through the
    effective-weight buffer.  The layer's output is the network's style source and the first Dense's input (DESIGN.md section 5
    "Mapping network")."""
    kind = "mapping"

    def __init__(self, units=None, num_layers=8, lr_multiplier=0.01, alpha=0.2, equalized_lr=True, w_avg_beta=0.995, **kw):
        super().__init__(**kw)
        if isinstance(num_layers, bool) or int(num_layers) != num_layers or int(num_layers) < 1:
            raise ValueError(f"MappingNetwork num_layers={num_layers!r}: at least one layer")
        if units is not None and (isinstance(units, bool) or int(units) != units or int(units) < 1):
            raise ValueError(f"MappingNetwork units={units!r}: None (the input size) or a positive size")
        if isinstance(lr_multiplier, bool) or not isinstance(lr_multiplier, (int, float, np.integer, np.floating)) \
                or not (math.isfinite(lr_multiplier) and lr_multiplier > 0):
            raise ValueError(f"MappingNetwork lr_multiplier={lr_multiplier!r}: must be a positive finite number")
        if not equalized_lr and float(lr_multiplier) != 1.0:
            raise ValueError(f"MappingNetwork lr_multiplier={lr_multiplier!r} with equalized_lr=False: the multiplier is a run-time "
                             "coefficient of the equalised learning rate; without it, it must be 1")
        if not (math.isfinite(alpha) and alpha > 0.0):
            raise ValueError(f"MappingNetwork alpha={alpha!r}: must be positive (the backward reads the branch off the stored output's sign)")
        if not 0.0 <= float(w_avg_beta) < 1.0:
            raise ValueError(f"MappingNetwork w_avg_beta={w_avg_beta!r}: a decay in [0, 1)")
        self.units = None if units is None else int(units)
        self.num_layers, self.lr_multiplier, self.alpha = int(num_layers), float(lr_multiplier), float(alpha)
        self.equalized_lr, self.w_avg_beta = bool(equalized_lr), float(w_avg_beta)
        self.coefficients = self.bias_multiplier = None

    def units_for(self, in_shape):
        if len(in_shape) != 1:
            raise NotImplementedError(MAPPING_RULE + f" (on an input of shape {tuple(in_shape)})")
        return int(in_shape[0]) if self.units is None else self.units

    def out_shape(self, in_shape):
        U = self.units_for(in_shape)
        self._set_coefficients(int(in_shape[0]), U)
        return (U,)

    def _set_coefficients(self, L, U):
        fans = [L] + [U] * (self.num_layers - 1)
        if self.equalized_lr:        # in double, rounded to fp32 once
            self.coefficients = [float(np.float32(math.sqrt(2.0) / math.sqrt(f) * self.lr_multiplier)) for f in fans]
            self.bias_multiplier = float(np.float32(self.lr_multiplier))
        else:
            self.coefficients, self.bias_multiplier = [1.0] * self.num_layers, 1.0

    def var_specs(self, in_shape):
        U, L = self.units_for(in_shape), int(in_shape[0])
        self._set_coefficients(L, U)
        shapes = [(L, U)] + [(U, U)] * (self.num_layers - 1)
        if self.equalized_lr:
            inv = 1.0 / self.lr_multiplier
            init = lambda sh: (lambda rng: (rng.standard_normal(sh) * inv).astype(np.float32))
        else:
            init = lambda sh: _glorot(sh, sh[0], sh[1])
        specs = [(f"kernel_{l}", sh, True, init(sh)) for l, sh in enumerate(shapes)]
        specs += [(f"bias_{l}", (U,), True, _zeros((U,))) for l in range(self.num_layers)]
        return specs + [("w_avg", (U,), False, _zeros((U,)))]


class LeakyReLU(Layer):
    kind = "lrelu"

    def __init__(self, alpha=0.3, **kw):
        super().__init__(**kw)
        self.alpha = float(alpha)


class Dropout(Layer):
    kind = "dropout"

    def __init__(self, rate, **kw):
        super().__init__(**kw)
        self.rate = float(rate)


def _channels_last(data_format):
    return data_format is None or str(data_format).lower() == "channels_last"


class UpSampling2D(Layer):
    """tf.keras.layers.UpSampling2D: nearest-neighbour, factor 2 (the resize-convolution generator's resolution step)."""
    kind = "upsample"

    def __init__(self, size=(2, 2), data_format=None, interpolation="nearest", **kw):
        super().__init__(**kw)
        if _pair(size) != (2, 2):
            raise NotImplementedError(f"UpSampling2D size {size!r}: only size 2 is supported")
        if str(interpolation).lower() != "nearest":
            raise NotImplementedError(f"UpSampling2D interpolation {interpolation!r}: only 'nearest' is supported")
        if not _channels_last(data_format):
            raise NotImplementedError("only data_format='channels_last' (NHWC) is supported")
        self.size = (2, 2)

    def out_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError(f"UpSampling2D needs an [H, W, C] map, got {tuple(s)}")
        return (2 * s[0], 2 * s[1], s[2])


class AveragePooling2D(Layer):
    """tf.keras.layers.AveragePooling2D: 2x2 pool, stride 2, on maps of even height and width."""
    kind = "avgpool"

    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", data_format=None, **kw):
        super().__init__(**kw)
        if _pair(pool_size) != (2, 2):
            raise NotImplementedError(f"AveragePooling2D pool_size {pool_size!r}: only a 2x2 pool is supported")
        if strides is not None and _pair(strides) != (2, 2):
            raise NotImplementedError(f"AveragePooling2D strides {strides!r}: only strides equal to the 2x2 pool are supported")
        if str(padding).lower() not in ("valid", "same"):
            raise NotImplementedError(f"AveragePooling2D padding {padding!r}")
        if not _channels_last(data_format):
            raise NotImplementedError("only data_format='channels_last' (NHWC) is supported")
        self.pool_size = self.strides = (2, 2)

    def out_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError(f"AveragePooling2D needs an [H, W, C] map, got {tuple(s)}")
        if s[0] % 2 or s[1] % 2:
            raise NotImplementedError(f"AveragePooling2D on a map of odd height or width {tuple(s)} (Keras would drop the last row)")
        return (s[0] // 2, s[1] // 2, s[2])


def resample_taps(resample_kernel):
    """f = k / sum(k) of an even-length 1-D resampling kernel of at most 8 taps: normalised in double, rounded to fp32 once, as a
    tuple of Python floats (StyleGAN2's ``_setup_kernel``, per axis)."""
    try:
        k = [float(v) for v in resample_kernel]
    except (TypeError, ValueError):
        raise ValueError(f"resample_kernel {resample_kernel!r}: a sequence of numbers is needed") from None
    if not k or not all(math.isfinite(v) for v in k) or not sum(k) > 0.0:
        raise ValueError(f"resample_kernel {resample_kernel!r}: finite numbers with a positive sum are needed")
    if len(k) % 2 or len(k) > 8:
        raise NotImplementedError(f"resample_kernel {resample_kernel!r}: only even lengths up to 8 are supported")
    total = math.fsum(k)
    return tuple(float(np.float32(v / total)) for v in k)


class _FilteredResampling2D(Layer):
    """What the two FIR-filtered resampling layers share: the kernel, its fp32 taps and the refusals."""

    def __init__(self, resample_kernel, factor, data_format, **kw):
        super().__init__(**kw)
        self.taps = resample_taps(resample_kernel)
        self.resample_kernel = tuple(float(v) for v in resample_kernel)
        if _pair(factor) != (2, 2):
            raise NotImplementedError(f"{type(self).__name__} factor {factor!r}: only a factor of 2 is supported")
        if not _channels_last(data_format):
            raise NotImplementedError("only data_format='channels_last' (NHWC) is supported")

    @property
    def flipped_taps(self):
        """flip(f): the taps of the adjoint operator (the layer's backward)."""
        return self.taps[::-1]

    def _map(self, s):
        if len(s) != 3:
            raise NotImplementedError(f"{type(self).__name__} needs an [H, W, C] map, got {tuple(s)}")
        return s


class FilteredUpSampling2D(_FilteredResampling2D):
    """StyleGAN2's ``upsample_2d``: 2x zero-insertion upsampling through the separable low-pass ``resample_kernel`` (normalised to
    sum 1 per axis, gain 4), zero padding at the border.  With the default (1, 3, 3, 1) it is half-pixel bilinear interpolation in
    the interior; (1, 1) is nearest-neighbour ``UpSampling2D``.  No variables."""
    kind = "firup"

    def __init__(self, resample_kernel=(1, 3, 3, 1), size=2, data_format=None, **kw):
        super().__init__(resample_kernel, size, data_format, **kw)
        self.size = (2, 2)

    def out_shape(self, s):
        s = self._map(s)
        return (2 * s[0], 2 * s[1], s[2])


class FilteredDownSampling2D(_FilteredResampling2D):
    """StyleGAN2's ``downsample_2d``: the separable low-pass ``resample_kernel`` (normalised to sum 1 per axis), zero padding at the
    border, then every second sample, on maps of even height and width.  (1, 1) is ``AveragePooling2D``.  No variables."""
    kind = "firdown"

    def __init__(self, resample_kernel=(1, 3, 3, 1), factor=2, data_format=None, **kw):
        super().__init__(resample_kernel, factor, data_format, **kw)
        self.factor = 2

    def out_shape(self, s):
        s = self._map(s)
        if s[0] % 2 or s[1] % 2:
            raise NotImplementedError(f"FilteredDownSampling2D on a map of odd height or width {tuple(s)}")
        return (s[0] // 2, s[1] // 2, s[2])


class MinibatchStdDev(Layer):
    """The minibatch standard deviation layer of ProGAN / StyleGAN / StyleGAN2 (``num_new_features = 1``) at the top of a critic:
    [N, H, W, C] -> [N, H, W, C + 1].  Samples are split into groups of ``group_size`` CONSECUTIVE samples (group g is rows
    [g G, (g + 1) G)); per group and column (pixel, channel) s = sqrt(var_n x + epsilon) with the biased variance over the members,
    f_g = the mean of s over all columns, and f_g becomes channel C of every pixel of every sample of the group.  No variables.

    StyleGAN2 takes its groups strided (n, n + M, ...).  Here they are consecutive: the critic step runs [fakes; reals; x-hat] as one
    pass and a group must not straddle two slices, data-parallel shards are contiguous, and the samples are i.i.d., so the statistic
    has the same distribution.  Every pass of a step has B, 2B or 3B rows: the batch size must be a multiple of ``group_size``
    (ValueError otherwise; the group is never shrunk).  The layer stands directly before the critic's Flatten -> Dense(1)."""
    kind = "mbstd"

    def __init__(self, group_size=4, epsilon=1e-8, num_new_features=1, **kw):
        super().__init__(**kw)
        if int(num_new_features) != 1:
            raise NotImplementedError(f"MinibatchStdDev num_new_features={num_new_features!r}: only one new feature is supported")
        if int(group_size) < 2:
            raise ValueError(f"MinibatchStdDev group_size={group_size!r}: a group needs at least 2 samples")
        if not float(epsilon) > 0.0:
            raise ValueError(f"MinibatchStdDev epsilon={epsilon!r}: must be positive")
        self.group_size, self.epsilon, self.num_new_features = int(group_size), float(epsilon), 1

    def out_shape(self, s):
        if len(s) != 3:
            raise NotImplementedError(f"MinibatchStdDev needs an [H, W, C] map, got {tuple(s)}")
        return (s[0], s[1], s[2] + 1)

    def check_rows(self, rows):
        """``rows``: the samples per slice of a pass.  Groups are consecutive and never straddle the slices of a step's passes."""
        if int(rows) % self.group_size:
            raise ValueError(f"MinibatchStdDev(group_size={self.group_size}): a pass of {rows} rows per slice is no multiple of the group "
                             f"size.  Every pass of a step has B, 2B or 3B rows, so the (per-device) batch size B must satisfy "
                             f"B % group_size == 0; the group is not shrunk")


class Reshape(Layer):
    kind = "reshape"

    def __init__(self, target_shape, **kw):
        super().__init__(**kw)
        self.target_shape = tuple(int(v) for v in target_shape)

    def out_shape(self, s):
        assert int(np.prod(s)) == int(np.prod(self.target_shape)), (s, self.target_shape)
        return self.target_shape


class Flatten(Layer):
    kind = "flatten"

    def out_shape(self, s):
        return (int(np.prod(s)),)


# ----------------------------------------------------------------------------------------------------
class ParamStore:
    """All variables of one top-level model in flat HBM buffers."""

    ALIGN = 4   # floats (16 bytes): every variable view is 16-byte aligned for float4 access

    def __init__(self, layers_with_shapes, device):
        self.device = torch.device(device)
        self.entries = []       # (layer, name, offset, shape, trainable)
        off_t = off_s = 0
        init_vals, fresh_spectral = [], []
        for layer, in_shape in layers_with_shapes:
            for name, shape, trainable, init in layer.var_specs(in_shape):
                n = int(np.prod(shape))
                old = layer.vars.get(name)
                val = old.detach().cpu().numpy().reshape(shape) if old is not None else init(_seed_state["rng"])
                if trainable:
                    self.entries.append((layer, name, off_t, tuple(shape), True))
                    off_t += -(-n // self.ALIGN) * self.ALIGN
                else:
                    self.entries.append((layer, name, off_s, tuple(shape), False))
                    off_s += -(-n // self.ALIGN) * self.ALIGN
                init_vals.append(val)
                if name == "vector_v" and old is None:
                    fresh_spectral.append(layer)
        self.n_train, self.n_state = off_t, off_s
        self.theta = torch.zeros(max(off_t, 1), dtype=torch.float32, device=self.device)
        self.state = torch.zeros(max(off_s, 1), dtype=torch.float32, device=self.device)
        self.grad = self.m = self.v = None
        self.s3 = None              # third optimiser slot (optimizers.py: Adam's vhat, RMSprop's mg), allocated when a variant needs it
        self.slot_owner = None      # the optimizer whose slots m / v / s3 are (optimizers.Optimizer.attach)
        self.step_count = 0
        for (layer, name, off, shape, trainable), val in zip(self.entries, init_vals):
            buf = self.theta if trainable else self.state
            n = int(np.prod(shape))
            view = buf[off:off + n].view(shape)
            view.copy_(torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)))
            layer.vars[name] = view
        # transposed copies of conv kernels ([taps][C][R] from [taps][R][C]) for the direction that needs them
        self._tr = {}           # id(layer) -> tensor
        # spectrally normalised layers: the engine reads W / sigma and its transposed copy from one flat effective-weight buffer,
        # laid out with the descriptor table by spectral_table(); without such layers nothing is allocated
        self.eff = None
        self._sn = {}           # id(layer) -> (effective kernel view, transposed view or None)
        self._sn_table = None
        # equalised-learning-rate layers: c * W and its transposed copy in the same buffer, laid out by eqlr_table() (a model has
        # wrappers of one kind only: engine.Net refuses the mixture)
        self._eq = {}           # id(layer) -> (effective kernel view, transposed view or None)
        self._eq_table = None
        for layer in fresh_spectral:
            layer.init_state()
        self.tr_dirty = True

    @property
    def tr_dirty(self):
        """The weights changed since the copies derived from them (transposed kernels, W / sigma) were made."""
        return self._tr_dirty

    @tr_dirty.setter
    def tr_dirty(self, value):
        self._tr_dirty = self.sn_dirty = bool(value)        # sn_dirty alone is cleared by the step's own power round

    def ensure_opt_state(self):
        if self.grad is None:
            self.grad = torch.zeros_like(self.theta)
            self.m = torch.zeros_like(self.theta)
            self.v = torch.zeros_like(self.theta)

    def view_like(self, buf, layer, name):
        cache = self.__dict__.setdefault("_view_cache", {})
        key = (buf.data_ptr(), id(layer), name)
        v = cache.get(key)
        if v is None:
            for (l, n, off, shape, trainable) in self.entries:
                if l is layer and n == name:
                    assert trainable
                    v = cache[key] = buf[off:off + int(np.prod(shape))].view(shape)
                    break
            else:
                raise KeyError(name)
        return v

    def train_range(self, *layers):
        """[lo, hi) of the flat trainable buffer covered by the variables of ``layers`` (None entries ignored)."""
        cache = self.__dict__.setdefault("_range_cache", {})
        key = tuple(id(x) for x in layers)
        r = cache.get(key)
        if r is None:
            lo, hi = None, None
            for (l, n, off, shape, trainable) in self.entries:
                if trainable and any(l is x for x in layers if x is not None):
                    end = off + -(-int(np.prod(shape)) // self.ALIGN) * self.ALIGN
                    lo = off if lo is None else min(lo, off)
                    hi = end if hi is None else max(hi, end)
            r = cache[key] = (0, 0) if lo is None else (lo, hi)
        return r

    def grad_of(self, layer, name):
        self.ensure_opt_state()
        return self.view_like(self.grad, layer, name)

    def kernel(self, layer, transposed=False):
        """The kernel the engine computes with: the layer's own variable (``transposed``: its [k*k][C][R] copy), or for a spectrally
        normalised layer W / sigma, for an equalised-learning-rate layer c * W, and its transposed copy in the effective-weight
        buffer."""
        if isinstance(layer, StyleModulation) and isinstance(layer.layer, EqualizedLearningRate):
            layer = layer.layer         # the wrapped EqualizedLearningRate owns c * W (engine.Net.eqlr_layers lists it)
        if isinstance(layer, SpectralNormalization):
            views = self._sn.get(id(layer))
            if views is None:
                raise KeyError("effective weights are laid out by spectral_table(); call Net.prepare_weights() first")
            return views[1 if transposed else 0]
        if isinstance(layer, EqualizedLearningRate):
            views = self._eq.get(id(layer))
            if views is None:
                raise KeyError("effective weights are laid out by eqlr_table(); call Net.prepare_weights() first")
            return views[1 if transposed else 0]
        return self.transposed_kernel(layer) if transposed else layer.vars["kernel"]

    def _state_offset(self, layer, name):
        return next(off for (l, n, off, _, tr) in self.entries if l is layer and n == name and not tr)

    def spectral_table(self, layers):
        """The descriptor table (ops.SpectralTable) of the spectrally normalised ``layers`` and, with it, the effective-weight buffer:
        per layer W / sigma [K, N] and, for conv kinds, the transposed copy the other direction of the conv reads."""
        key = [id(l) for l in layers]
        if self._sn_table is not None and self._sn_table[0] == key:
            return self._sn_table[1]
        from . import ops
        pad = lambda n: -(-n // self.ALIGN) * self.ALIGN
        rows, views, off = [], {}, 0
        for layer in layers:
            w = layer.vars["kernel"]
            K, N, taps = SpectralNormalization.matrix_shape(w.shape)
            w_off = (w.data_ptr() - self.theta.data_ptr()) // 4
            assert 0 <= w_off < self.theta.numel() and w_off % 4 == 0
            eff_off, off = off, off + pad(K * N)
            tr_off = -1
            if layer.kind in ("conv", "convT"):
                tr_off, off = off, off + pad(K * N)
            rows.append(dict(w_off=w_off, u_off=self._state_offset(layer, "vector_u"), v_off=self._state_offset(layer, "vector_v"),
                             sigma_off=self._state_offset(layer, "sigma"), eff_off=eff_off, tr_off=tr_off, K=K, N=N, taps=taps))
            views[id(layer)] = (eff_off, tr_off, K * N, tuple(w.shape))
        self.eff = torch.empty(max(off, 4), dtype=torch.float32, device=self.device)
        self._sn = {k: (self.eff[e:e + n].view(shape), None if t < 0 else self.eff[t:t + n]) for k, (e, t, n, shape) in views.items()}
        table = ops.SpectralTable(ops.spectral.rows(rows), self.device)
        self._sn_table = (key, table)
        return table

    def eqlr_table(self, layers):
        """The descriptor table (ops.EqlrTable) of the equalised-learning-rate ``layers`` and, with it, the effective-weight buffer:
        per layer c * W [K, N] and, for conv kinds, the transposed copy the other direction of the conv reads; 4-float aligned."""
        key = [id(l) for l in layers]
        if self._eq_table is not None and self._eq_table[0] == key:
            return self._eq_table[1]
        from . import ops
        pad = lambda n: -(-n // self.ALIGN) * self.ALIGN
        rows, views, off = [], {}, 0
        for layer in layers:
            w = layer.vars["kernel"]
            K, N, taps = SpectralNormalization.matrix_shape(w.shape)
            w_off = (w.data_ptr() - self.theta.data_ptr()) // 4
            assert 0 <= w_off < self.theta.numel() and w_off % 4 == 0
            eff_off, off = off, off + pad(K * N)
            tr_off = -1
            if layer.kind in ("conv", "convT"):
                tr_off, off = off, off + pad(K * N)
            rows.append(dict(w_off=w_off, eff_off=eff_off, tr_off=tr_off, K=K, N=N, taps=taps, c=layer.coefficient))
            views[id(layer)] = (eff_off, tr_off, K * N, tuple(w.shape))
        self.eff = torch.empty(max(off, 4), dtype=torch.float32, device=self.device)
        self._eq = {k: (self.eff[e:e + n].view(shape), None if t < 0 else self.eff[t:t + n]) for k, (e, t, n, shape) in views.items()}
        table = ops.EqlrTable(ops.eqlr.rows(rows), self.device)
        ops.eqlr.check_table(table.host, self.theta.numel(), self.eff.numel())
        self._eq_table = (key, table)
        return table

    def mod_q(self, layer):
        """Q [I, O] = the sum over the taps of W_eff^2 of a demodulating StyleModulation layer: a derived weight like the transposed
        copies, refreshed by engine.Net.mod_update(); one persistent buffer per layer (a recorded step program holds its address)."""
        cache = self.__dict__.setdefault("_mod_q", {})
        q = cache.get(id(layer))
        if q is None:
            w = layer.vars["kernel"]
            I, O = (w.shape[3], w.shape[2]) if layer.kind == "convT" else (w.shape[2], w.shape[3])
            q = cache[id(layer)] = torch.empty((I, O), dtype=torch.float32, device=self.device)
        return q

    def transposed_kernel(self, layer):
        """[k*k][C][R] copy of a conv kernel stored [k*k][R][C]; refreshed after every optimiser step."""
        t = self._tr.get(id(layer))
        if t is None:
            raise KeyError("transposed kernels are laid out by refresh_transposed(); call Net.prepare_weights() first")
        return t

    def _plan_transposed(self, layers):
        """One flat buffer for every transposed copy + the device descriptor table of the batched transpose."""
        offs, desc, off, tile = {}, [], 0, 0
        for layer in layers:
            w = layer.vars["kernel"]
            k2, R, Cc = w.shape[0] * w.shape[1], w.shape[2], w.shape[3]
            src_off = (w.data_ptr() - self.theta.data_ptr()) // 4
            assert 0 <= src_off < self.theta.numel() and src_off % 4 == 0
            desc.append([src_off, off, k2, R, Cc, tile])
            offs[id(layer)] = (off, k2 * R * Cc)
            tile += k2 * (-(-R // 64)) * (-(-Cc // 64))
            off += -(-k2 * R * Cc // self.ALIGN) * self.ALIGN
        self._tr_flat = torch.empty(max(off, 4), dtype=torch.float32, device=self.device)
        self._tr = {k: self._tr_flat[o:o + n] for k, (o, n) in offs.items()}
        self._tr_desc = torch.tensor(desc, dtype=torch.int32, device=self.device).contiguous()
        self._tr_tiles = tile
        self._tr_layers = [id(l) for l in layers]

    def refresh_transposed(self, layers):
        from . import ops
        layers = list(layers)
        if not layers:
            self.tr_dirty = False
            return
        if getattr(self, "_tr_layers", None) != [id(l) for l in layers]:
            self._plan_transposed(layers)
        ops.transpose_last2_batched(self.theta, self._tr_flat, self._tr_desc, len(layers), self._tr_tiles)
        self.tr_dirty = False


class Sequential(Layer):
    """tf.keras.Sequential stand-in (demo_celeba.py:51,96)."""
    kind = "sequential"

    def __init__(self, layers: Optional[Sequence[Layer]] = None, name=None, **kw):
        super().__init__(name=name, **kw)
        self.layers: List[Layer] = []
        self._in_shape: Optional[Tuple[int, ...]] = None
        self._out_shape: Optional[Tuple[int, ...]] = None
        self._store: Optional[ParamStore] = None
        self._net = None
        self.optimizer = None
        for l in (layers or []):
            self.add(l)

    # ---- construction
    def add(self, layer: Layer):
        if self._store is not None:
            raise RuntimeError("cannot add layers to a built model")
        self.layers.append(layer)
        if self._in_shape is None:
            decl = layer._declared_input_shape
            if decl is None and isinstance(layer, Sequential):
                decl = layer._in_shape
            if decl is not None and len(self.layers) == 1:
                self._in_shape = tuple(decl)
                self._out_shape = tuple(decl)
        if self._in_shape is not None:
            self._out_shape = tuple(layer.out_shape(self._out_shape))

    def out_shape(self, s):
        for l in self.layers:
            s = l.out_shape(s)
        return tuple(s)

    @property
    def input_shape(self):
        return None if self._in_shape is None else (None,) + self._in_shape

    @property
    def output_shape(self):
        return None if self._out_shape is None else (None,) + self._out_shape

    def flat_layers(self):
        """[(layer, in_shape)] with nested Sequentials expanded."""
        out, s = [], self._in_shape
        if s is None:
            raise RuntimeError("model has no input shape: give the first layer input_shape=")
        style_dim = int(self._in_shape[0]) if len(self._in_shape) == 1 else None
        head = self.layers[1:2] if self.layers and self.layers[0].kind == "pixelnorm" else self.layers[:1]
        if style_dim is not None and head and isinstance(head[0], MappingNetwork):      # the style source is the mapping network's w
            style_dim = head[0].units_for(self._in_shape)
        for l in self.layers:
            if isinstance(l, Sequential):
                if l._in_shape is None:
                    l._in_shape, l._out_shape = tuple(s), l.out_shape(s)
                for ll, ss in l.flat_layers():
                    out.append((ll, ss))
            else:
                if isinstance(l, StyleModulation):      # its style source is this model's input vector, or the w of its mapping prefix
                    l.style_dim = style_dim
                out.append((l, tuple(s)))
            s = l.out_shape(s)
        return out

    def build(self, device=None):
        """Allocates (or re-binds) the variables.  Wrapping built models into a new Sequential moves their
        variables into the wrapper's store and keeps the inner models bound to it."""
        if self._store is not None:
            return self
        flat = self.flat_layers()
        self._store = ParamStore(flat, device or default_device())
        for l in self.layers:
            if isinstance(l, Sequential):
                l._adopt(self._store)
        return self

    def _adopt(self, store):
        self._store, self._net = store, None
        for l in self.layers:
            if isinstance(l, Sequential):
                l._adopt(store)

    @property
    def store(self) -> ParamStore:
        self.build()
        return self._store

    # conv forward / data-gradient math of this model's engine (ops.CONV_MATH); WGAN(conv_math=...) sets it on both models
    conv_math = "fp32"

    def net(self):
        from .engine import Net
        if self._net is None:
            self.build()
            self._net = Net(self.flat_layers(), self._store)
        self._net.conv_math = self.conv_math
        return self._net

    # ---- Keras surface
    def _own_layers(self):
        return [l for l, _ in self.flat_layers()]

    @property
    def trainable_variables(self):
        self.build()
        own = {id(l) for l in self._own_layers()}
        return [l.vars[n] for (l, n, _, _, tr) in self._store.entries if tr and id(l) in own]

    @property
    def variables(self):
        self.build()
        own = {id(l) for l in self._own_layers()}
        return [l.vars[n] for (l, n, _, _, tr) in self._store.entries if id(l) in own]

    def count_params(self):
        return sum(int(v.numel()) for v in self.variables)

    def get_weights(self):
        return [v.detach().cpu().numpy().copy() for v in self.variables]

    def set_weights(self, weights):
        vs = self.variables
        assert len(vs) == len(weights), (len(vs), len(weights))
        for v, w in zip(vs, weights):
            v.copy_(torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).view(v.shape))
        self._store.tr_dirty = True

    def save_weights(self, filepath, overwrite=True, save_format=None):
        np.savez(filepath if str(filepath).endswith(".npz") else str(filepath) + ".npz",
                 **{f"v{i}": w for i, w in enumerate(self.get_weights())})

    def load_weights(self, filepath):
        p = filepath if str(filepath).endswith(".npz") else str(filepath) + ".npz"
        d = np.load(p)
        self.set_weights([d[f"v{i}"] for i in range(len(d.files))])

    def summary(self):
        print(f'Model: "{self.name}"')
        for l, s in self.flat_layers():
            print(f"  {l.__class__.__name__:<20} in={s!s:<18} out={l.out_shape(s)!s:<18} params={sum(int(np.prod(sh)) for _, sh, _, _ in l.var_specs(s)):,}")
        print(f"Total params: {self.count_params():,}")

    def __call__(self, x, training=False):
        """Forward pass on the HIP kernels; returns a fresh tensor [B, *output_shape]."""
        return self.net().predict(x, training=training)


class SpectralSequential(Sequential):
    """A Sequential that, with its ``spectral_norm`` attribute set, wraps every Conv2D, Conv2DTranspose and Dense added to it into a
    SpectralNormalization (the DCGAN stacks' ``spectral_norm=`` argument), or with ``equalized_lr`` set into an
    EqualizedLearningRate (their ``equalized_lr=`` argument) of gain ``gain``: by default sqrt(2), the gain of a layer in front of a
    LeakyReLU, and 1 for a layer with a fused tanh."""
    spectral_norm = False
    equalized_lr = False

    def add(self, layer, gain=None):
        if isinstance(layer, StyleModulation) and self.spectral_norm:
            raise NotImplementedError(MOD_RULE + " (spectral_norm=True)")
        if isinstance(layer, (Conv2D, Conv2DTranspose, Dense)):
            if self.spectral_norm:
                layer = SpectralNormalization(layer)
            elif self.equalized_lr:
                if gain is None:
                    gain = 1.0 if getattr(layer, "activation", None) == "tanh" else math.sqrt(2)
                layer = EqualizedLearningRate(layer, gain=gain)
        super().add(layer)
