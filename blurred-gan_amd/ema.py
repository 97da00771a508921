"""Generator weight averaging: the exponential moving average of the generator's weights that GAN recipes sample from
(``tf.train.ExponentialMovingAverage``; ProGAN's ``Gs``), as ``WGAN(..., generator_ema=...)``.

``GeneratorEMA`` is the schedule: the host computes one scalar per generator update, ``w_k = 1 - beta_k`` in double, and one HIP
launch (include/bgan.h ``bg_ema_f32``) applies TF's ``assign_moving_average`` rule ``avg -= w * (avg - theta)`` over the
generator's flat trainable buffer and its BatchNorm moving statistics.  Under a step program ``w`` is bound to a slot of the
program and recomputed before every replay, like an optimizer's learning rate.

The average is plain fp32, as TF's is: for ``w`` below about 1e-4 an update ``w * (avg - theta)`` can fall under one ulp of the
average and is then lost to rounding.

``clone_structure`` makes the averaged model: a copy of a ``Sequential``'s layer descriptors with its OWN ``ParamStore``."""
from __future__ import annotations

import copy
import numbers

from .layers import EqualizedLearningRate, Sequential, SpectralNormalization, StyleModulation

__all__ = ["GeneratorEMA", "clone_structure"]


def _is_number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


class GeneratorEMA:
    """The decay schedule of the averaged generator.  Exactly one of

    ``decay``            beta per generator update, in [0, 1);
    ``halflife_images``  ProGAN's rule: beta = 0.5 ** (B * world_size * d_steps_per_g_step / halflife_images) with B the batch
                         of the step, so the average does not depend on the batch size and a partial last batch gets its own beta.

    ``warmup=True`` applies TF's ``num_updates`` rule: beta_k = min(beta, (1 + k) / (10 + k)), k = updates done so far."""

    def __init__(self, decay=None, halflife_images=None, warmup=False):
        if (decay is None) == (halflife_images is None):
            raise ValueError("GeneratorEMA: give exactly one of `decay` and `halflife_images`")
        if decay is not None and not (_is_number(decay) and 0.0 <= decay < 1.0):
            raise ValueError(f"GeneratorEMA: `decay` must be a number in [0, 1), got {decay!r}")
        if halflife_images is not None and not (_is_number(halflife_images) and halflife_images > 0):
            raise ValueError(f"GeneratorEMA: `halflife_images` must be a positive number, got {halflife_images!r}")
        self.decay = None if decay is None else float(decay)
        self.halflife_images = None if halflife_images is None else float(halflife_images)
        self.warmup = bool(warmup)

    def get_config(self):
        return {"decay": self.decay, "halflife_images": self.halflife_images, "warmup": self.warmup}

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def static_config(self):
        """The schedule as part of a step program's key."""
        return tuple(sorted(self.get_config().items()))

    def beta_at(self, k, B=None, world_size=1, d_steps_per_g_step=1):
        """beta of update number ``k`` (0-based), in double."""
        if self.decay is not None:
            beta = self.decay
        else:
            if B is None:
                raise ValueError("GeneratorEMA(halflife_images=...) needs the step's batch size")
            beta = 0.5 ** (int(B) * int(world_size) * int(d_steps_per_g_step) / self.halflife_images)
        if self.warmup:
            beta = min(beta, (1.0 + k) / (10.0 + k))
        return beta

    def w_at(self, k, B=None, world_size=1, d_steps_per_g_step=1):
        """``1 - beta_k`` in double: the scalar the update kernel takes (rounded to fp32 once, at the launch)."""
        return 1.0 - self.beta_at(k, B, world_size, d_steps_per_g_step)

    def __repr__(self):
        return f"GeneratorEMA({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


def as_schedule(value):
    """``WGAN(generator_ema=...)``: None (off), a float (``GeneratorEMA(decay=x)``) or a ``GeneratorEMA``."""
    if value is None or isinstance(value, GeneratorEMA):
        return value
    if _is_number(value):
        return GeneratorEMA(decay=value)
    raise ValueError(f"generator_ema must be None, a decay in [0, 1) or a GeneratorEMA, got {value!r}")


def _clone_layer(layer):
    c = copy.copy(layer)
    # the copy starts from the live layer's CURRENT values: ParamStore copies a variable it finds in `vars` and draws from the
    # weight-initialisation RNG only for one it does not find, and it rebinds the COPY's dict, never the live layer's
    c.vars = dict(layer.vars)
    w = c
    while isinstance(w, (SpectralNormalization, EqualizedLearningRate, StyleModulation)):
        # a wrapper shares ONE dict with the layer it wraps (a StyleModulation around an EqualizedLearningRate: all three): the copy
        # gets inner layers of its own, bound to the copy's dict (a shallow copy alone would leave the clone's inner layer on the
        # live model's variables)
        w.layer = copy.copy(w.layer)
        w.layer.vars = c.vars
        w = w.layer
    if isinstance(layer, Sequential):
        c.layers = [_clone_layer(l) for l in layer.layers]
        c._store = c._net = c.optimizer = None
    return c


def clone_structure(model: Sequential) -> Sequential:
    """A built copy of ``model``: the same layer descriptors (nested Sequentials included), copied, in its own ``ParamStore``
    whose variables start as bit-copies of the model's.  Draws nothing from the weight-initialisation RNG and allocates no
    gradient or optimizer slots; the live layers stay bound to the live store."""
    model.build()
    twin = _clone_layer(model)
    twin.build(device=model.store.device)
    a, b = model.store, twin.store
    if (a.n_train, a.n_state) != (b.n_train, b.n_state):
        raise ValueError(f"{model.name}: the model's store holds variables of other models too (it was wrapped into another "
                         "Sequential); weight averaging needs a top-level model")
    b.theta.copy_(a.theta)
    b.state.copy_(a.state)
    b.tr_dirty = True
    return twin
