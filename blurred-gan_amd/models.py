"""The DCGAN stacks of the reference demos as ``layers.Sequential`` subclasses (same class names).

``arch``: "mnist" (demo_mnist.py:48-86), "celeba128" (demo_celeba.py:51-124, verbatim), "celeba64"
(build-side definition for BASELINE.json's 64x64 configs: the 128 stack minus its outermost stage on each
side, SURVEY.md 8a "Architecture note"), plus small test geometries ("tiny": MFMA-tileable channel
counts on 8x8x3 images; "tiny_mnist": odd channel counts, 12x12x1, ConvT with fused tanh; "tiny_k3": the "tiny"
stacks with 3x3 kernels -- every other architecture uses the demos' 5x5).

Both stacks have a resampling variant with the same map sizes, variable counts and Dense input: ``upsampling="resize"`` replaces
every stride-2 transposed convolution by nearest-neighbour UpSampling2D + a stride-1 Conv2D (the resize-convolution generator),
``downsampling="pool"`` every stride-2 convolution by a stride-1 one whose LeakyReLU / Dropout output is average-pooled.  Such a
stage convolves at the higher resolution: 4x the multiply-adds of the strided layer it replaces.

``upsampling="filtered"`` / ``downsampling="filtered"`` are the same two stacks with the resampling layer replaced by its FIR-filtered
counterpart: ``layers.FilteredUpSampling2D`` / ``layers.FilteredDownSampling2D`` with ``resample_kernel`` (default (1, 3, 3, 1):
StyleGAN2's ``upsample_2d`` / ``downsample_2d``; an even length up to 8, asymmetric kernels allowed).  Map sizes, variables and the
Dense input are those of ``"resize"`` / ``"pool"``; (1, 1) computes exactly what those compute.  They combine with everything
``"resize"`` / ``"pool"`` combine with.

The critic takes ``normalization="layer"``: a LayerNormalization over the channels between every Conv2D and its LeakyReLU (the
WGAN-GP paper's critic; BatchNormalization cannot stand there, the penalty is defined per sample).  Map sizes are unchanged, every
block gains 2 * C variables; it combines with ``downsampling="pool"``.

``minibatch_stddev=G`` puts a ``layers.MinibatchStdDev(group_size=G)`` in front of the critic's Flatten: one more feature map, the
Dense kernel becomes [P * (C + 1), 1] (flattened in (H, W, C + 1) order); the batch size must be a multiple of G.  It combines with
``downsampling="pool"``, ``normalization="layer"`` and ``spectral_norm=True``.

The generator takes ``normalization="pixel"`` (default ``"batch"``: the reference's stack): no BatchNormalization anywhere; the Dense
and every hidden (transposed) convolution carry a bias, and each hidden block is LeakyReLU -> ``layers.PixelNormalization`` (the
ProGAN / StyleGAN generator's normalisation: per pixel, no variables, no statistics, the same in training and inference, nothing
shared across the batch or across data-parallel ranks).  The Dense's block is Dense -> Reshape -> LeakyReLU -> PixelNormalization: the
normalisation runs over the channels of the reshaped map.  The tanh output layer is unchanged.  ``normalize_latents=True`` puts a
PixelNormalization in front of the Dense (with either normalisation).  Both combine with ``upsampling="resize"`` and
``spectral_norm=True``.

``noise=True`` (the generator, with ``normalization="pixel"`` or ``"style"``; default False: the stack variable for variable as before) puts a
``layers.NoiseInjection`` behind every (transposed) convolution of the stack except the tanh output layer, in front of its LeakyReLU:
StyleGAN's per-pixel noise inputs, one learned scalar ``noise_strength`` per layer, initialised to zero.  It combines with everything
``normalization="pixel"`` combines with.

``normalization="style"`` (the generator) is StyleGAN2's: every hidden (transposed) convolution is a
``layers.StyleModulation(conv, demodulate=True)`` with bias, then the NoiseInjection of ``noise=True``, then LeakyReLU -- no
PixelNormalization; the tanh output layer is ``StyleModulation(conv, demodulate=False)``.  The Dense block is the one ``"pixel"``
builds.  The styles come from the model's own input vector (behind the PixelNormalization of ``normalize_latents=True``), or, with
``mapping_layers=N`` > 0, from StyleGAN's mapping network: a ``layers.MappingNetwork(units=mapping_units, num_layers=N,
lr_multiplier=mapping_lr_multiplier)`` in front of the Dense (behind that PixelNormalization), whose output w [units] is both the
Dense's input and every layer's style source; the stack's ``equalized_lr`` is passed on to it (without it the multiplier must be 1).
``mapping_layers`` needs ``normalization="style"``.  Every modulated layer gains ``style_kernel`` [L, I] and ``style_bias`` [I].  It combines with ``noise=True``,
``equalized_lr=True``, every ``upsampling=`` and ``normalize_latents=True``; ``spectral_norm=True`` is refused.

``spectral_norm=True`` (either stack) wraps every Conv2D, Conv2DTranspose and Dense into ``layers.SpectralNormalization``: the
engine computes with W / sigma, and every wrapped layer gains the non-trainable ``vector_u``, ``vector_v`` and ``sigma``.

``equalized_lr=True`` (either stack) wraps them into ``layers.EqualizedLearningRate`` instead (ProGAN / StyleGAN's equalised
learning rate): kernels drawn from N(0, 1), the engine computes with c * W, c = gain / sqrt(fan_in); gain sqrt(2) for every layer in
front of a LeakyReLU, 1 for the tanh output layer and for the critic's Dense(1).  No new variables.  It combines with every other
argument but ``spectral_norm=True`` (``ValueError``: W / sigma would cancel c)."""
from __future__ import annotations

import math

from . import layers

_G = {  # base_hw, dense_ch, [(filters, stride, activation)], last_conv_filters
    "mnist": (7, 256, [(128, 1, None), (64, 2, None), (1, 2, "tanh")], None),
    "celeba128": (4, 512, [(512, 1, None), (256, 2, None), (128, 2, None), (64, 2, None), (32, 2, None), (16, 2, None)], 3),
    "celeba64": (4, 512, [(512, 1, None), (256, 2, None), (128, 2, None), (64, 2, None), (32, 2, None)], 3),
    "tiny": (2, 32, [(32, 1, None), (16, 2, None), (16, 2, None)], 3),
    "tiny_mnist": (3, 8, [(8, 1, None), (4, 2, None), (1, 2, "tanh")], None),
    "tiny_k3": (2, 32, [(32, 1, None), (16, 2, None), (16, 2, None)], 3),
}
_D = {"mnist": [64, 128], "celeba128": [16, 32, 64, 128, 256, 512], "celeba64": [32, 64, 128, 256, 512],
      "tiny": [16, 32], "tiny_mnist": [4, 8], "tiny_k3": [16, 32]}
KSIZE = {"tiny_k3": 3}      # conv kernel size per architecture; 5 where not listed
IMAGE_SHAPE = {"mnist": (28, 28, 1), "celeba128": (128, 128, 3), "celeba64": (64, 64, 3), "tiny": (8, 8, 3),
               "tiny_mnist": (12, 12, 1), "tiny_k3": (8, 8, 3)}
LATENT = {"mnist": 100, "celeba128": 100, "celeba64": 100, "tiny": 10, "tiny_mnist": 6, "tiny_k3": 10}


class DCGANGenerator(layers.SpectralSequential):
    def __init__(self, latent_size=None, arch="celeba128", *args, upsampling="transpose", spectral_norm=False, normalization="batch",
                 normalize_latents=False, equalized_lr=False, resample_kernel=(1, 3, 3, 1), noise=False, mapping_layers=0, mapping_units=None,
                 mapping_lr_multiplier=0.01, **kwargs):
        super().__init__(*args, **kwargs)
        self.spectral_norm, self.equalized_lr = bool(spectral_norm), bool(equalized_lr)
        if self.spectral_norm and self.equalized_lr:
            raise ValueError("equalized_lr=True together with spectral_norm=True: W / sigma cancels the run-time coefficient")
        if noise and normalization not in ("pixel", "style"):
            raise ValueError("noise=True needs normalization='pixel' or 'style': a NoiseInjection cannot stand in a BatchNormalization stage")
        self.noise = bool(noise)
        if isinstance(mapping_layers, bool) or int(mapping_layers) != mapping_layers or int(mapping_layers) < 0:
            raise ValueError(f"mapping_layers must be a layer count >= 0, got {mapping_layers!r}")
        if mapping_layers and normalization != "style":
            raise ValueError("mapping_layers > 0 needs normalization='style': the mapping network's output is the style source of the "
                             "modulated convolutions")
        self.mapping_layers, self.mapping_units, self.mapping_lr_multiplier = int(mapping_layers), mapping_units, mapping_lr_multiplier
        if upsampling not in ("transpose", "resize", "filtered"):
            raise ValueError(f"upsampling must be 'transpose', 'resize' or 'filtered', got {upsampling!r}")
        if normalization not in ("batch", "pixel", "style"):
            raise ValueError(f"normalization must be 'batch' or 'pixel' (or 'style': modulated convolutions), got {normalization!r}")
        if normalization == "style" and self.spectral_norm:
            raise ValueError("normalization='style' together with spectral_norm=True: W / sigma under weight demodulation is not built")
        self.upsampling, self.normalization, self.normalize_latents = upsampling, normalization, bool(normalize_latents)
        self.resample_kernel = tuple(resample_kernel)
        style = normalization == "style"
        pixel = normalization == "pixel" or style       # "style" keeps the Dense block and the biases of "pixel"
        base, ch, convt, last = _G[arch]
        k = KSIZE.get(arch, 5)
        self.latent_size = latent_size or LATENT[arch]
        first = dict(input_shape=(self.latent_size,))
        if self.normalize_latents:
            self.add(layers.PixelNormalization(**first))
            first = {}
        if self.mapping_layers:
            self.add(layers.MappingNetwork(units=mapping_units, num_layers=self.mapping_layers, lr_multiplier=mapping_lr_multiplier,
                                           equalized_lr=self.equalized_lr, **first))
            first = {}
        self.add(layers.Dense(base * base * ch, use_bias=pixel, **first))
        if pixel:
            self.add(layers.Reshape((base, base, ch)))
            self.add(layers.LeakyReLU())
            self.add(layers.PixelNormalization())
        else:
            self.add(layers.BatchNormalization())
            self.add(layers.LeakyReLU())
            self.add(layers.Reshape((base, base, ch)))
        assert self.output_shape == (None, base, base, ch)
        hw = base
        for filters, stride, act in convt:
            if stride == 2 and upsampling != "transpose":
                self.add(layers.UpSampling2D() if upsampling == "resize" else layers.FilteredUpSampling2D(self.resample_kernel))
                conv = layers.Conv2D(filters, (k, k), strides=(1, 1), padding="same", use_bias=pixel and act is None, activation=act)
            else:
                conv = layers.Conv2DTranspose(filters, (k, k), strides=(stride, stride), padding="same", use_bias=pixel and act is None,
                                              activation=act)
            self.add(self._modulated(conv) if style else conv)
            hw *= stride
            assert self.output_shape == (None, hw, hw, filters), self.output_shape
            if act is None and self.noise:
                self.add(layers.NoiseInjection())
            if act is None and style:
                self.add(layers.LeakyReLU())
            elif act is None and pixel:
                self.add(layers.LeakyReLU())
                self.add(layers.PixelNormalization())
            elif act is None:
                self.add(layers.BatchNormalization())
                self.add(layers.LeakyReLU())
        if last is not None:
            conv = layers.Conv2D(last, (k, k), padding="same", use_bias=False, activation="tanh")
            self.add(self._modulated(conv) if style else conv)
        assert self.output_shape == (None,) + IMAGE_SHAPE[arch], self.output_shape

    def _modulated(self, conv):
        """``conv`` as a modulated convolution: demodulated in front of a LeakyReLU, modulated only where tanh follows (StyleGAN2's
        toRGB); under ``equalized_lr`` around the EqualizedLearningRate the stack would have put there."""
        tanh = conv.activation == "tanh"
        if self.equalized_lr:
            conv = layers.EqualizedLearningRate(conv, gain=1.0 if tanh else math.sqrt(2))
        return layers.StyleModulation(conv, demodulate=not tanh)


class DCGANDiscriminator(layers.SpectralSequential):
    def __init__(self, arch="celeba128", *args, downsampling="stride", normalization=None, spectral_norm=False, minibatch_stddev=None,
                 equalized_lr=False, resample_kernel=(1, 3, 3, 1), **kwargs):
        super().__init__(*args, **kwargs)
        self.spectral_norm, self.equalized_lr = bool(spectral_norm), bool(equalized_lr)
        if self.spectral_norm and self.equalized_lr:
            raise ValueError("equalized_lr=True together with spectral_norm=True: W / sigma cancels the run-time coefficient")
        if downsampling not in ("stride", "pool", "filtered"):
            raise ValueError(f"downsampling must be 'stride', 'pool' or 'filtered', got {downsampling!r}")
        if normalization not in (None, "layer"):
            raise ValueError(f"normalization must be None or 'layer', got {normalization!r}")
        if minibatch_stddev is not None and (isinstance(minibatch_stddev, bool) or int(minibatch_stddev) != minibatch_stddev):
            raise ValueError(f"minibatch_stddev must be None or a group size, got {minibatch_stddev!r}")
        self.downsampling, self.normalization, self.resample_kernel = downsampling, normalization, tuple(resample_kernel)
        self.minibatch_stddev = None if minibatch_stddev is None else int(minibatch_stddev)
        pool = downsampling != "stride"
        for i, c in enumerate(_D[arch]):
            kw = dict(input_shape=list(IMAGE_SHAPE[arch])) if i == 0 else {}
            self.add(layers.Conv2D(c, KSIZE.get(arch, 5), strides=1 if pool else 2, padding="same", **kw))
            if normalization == "layer":
                self.add(layers.LayerNormalization())
            self.add(layers.LeakyReLU())
            self.add(layers.Dropout(0.3))
            if pool:
                self.add(layers.AveragePooling2D() if downsampling == "pool" else layers.FilteredDownSampling2D(self.resample_kernel))
        if self.minibatch_stddev is not None:
            self.add(layers.MinibatchStdDev(group_size=self.minibatch_stddev))
        self.add(layers.Flatten())
        self.add(layers.Dense(1, activation="linear"), gain=1.0)
