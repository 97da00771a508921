"""Keras optimizer objects (TF 2.5 ``tf.keras.optimizers``, optimizer_v2) for ``gan.generator.optimizer`` /
``gan.discriminator.optimizer`` (reference wgan.py:56-61,141,167): ``SGD``, ``RMSprop`` and ``Adam`` with Keras' constructor
arguments, defaults, ``learning_rate`` / ``iterations`` attributes and ``get_config`` / ``from_config``.

The host computes one scalar per update -- the effective rate ``lr_k`` (Keras ``_decayed_lr`` with ``k = iterations`` before the
update: ``schedule(k)`` or the float, then ``/ (1 + decay * k)``), for Adam ``lr_t = lr_k * sqrt(1 - beta_2^t) / (1 - beta_1^t)``
with ``t = k + 1`` -- and one fused HIP launch applies the rule over a network's flat trainable buffer (include/bgan.h
"optimisers").  Under a step program that scalar is bound to a slot of the program and recomputed before every replay.

Slots live beside the weights in the network's ``layers.ParamStore``, zero-initialised as Keras' ``add_slot`` does:

    =========  ===========  ===========  ============
    class      ``store.m``  ``store.v``  ``store.s3``
    =========  ===========  ===========  ============
    Adam       m            v            vhat (amsgrad)
    RMSprop    momentum     rms          mg (centered)
    SGD        momentum     --           --
    =========  ===========  ===========  ============

``store.m`` and ``store.v`` always exist; ``store.s3`` only for the variants that use it.  An optimizer keeps its slot buffers
per network: the first optimizer a network steps with adopts the store's (zero, or checkpoint-restored) buffers, any later one
starts from fresh zeros, and an optimizer assigned back finds its own slots again -- as Keras optimizer objects own their slot
variables.  One instance shared by both networks keeps one ``iterations`` counter, advanced by each ``apply``."""
from __future__ import annotations

import math
import numbers
import weakref

import torch

from . import ops, program, _lib

__all__ = ["Optimizer", "SGD", "RMSprop", "Adam", "get_optimizer"]

_EPSILON = 1e-7                 # tf.keras.backend.epsilon()


def _is_number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


class Optimizer:
    """The part of ``optimizer_v2.OptimizerV2`` these classes share."""

    _ALLOWED = {"lr", "decay", "clipnorm", "clipvalue", "global_clipnorm"}

    def __init__(self, name, learning_rate, **kwargs):
        for k in kwargs:
            if k not in self._ALLOWED:
                raise TypeError(f"Unexpected keyword argument passed to optimizer: {k}")
        for k in ("clipnorm", "clipvalue", "global_clipnorm"):
            if kwargs.get(k) is not None:
                raise NotImplementedError(f"{type(self).__name__}: gradient clipping ({k}) is not implemented")
        decay = kwargs.get("decay", 0.0)
        if not _is_number(decay) or decay < 0:
            raise ValueError(f"decay cannot be less than 0: {decay}")
        self._name = name
        self.decay = float(decay)
        self.learning_rate = kwargs.get("lr", learning_rate)
        self.iterations = 0
        self._slot_bufs = weakref.WeakKeyDictionary()      # ParamStore -> [m, v, s3] of this optimizer

    @property
    def learning_rate(self):
        return self._learning_rate

    @learning_rate.setter
    def learning_rate(self, value):
        if not (_is_number(value) or callable(value)):
            raise ValueError(f"learning_rate must be a number or a callable step -> rate, got {value!r}")
        self._learning_rate = value

    lr = learning_rate

    # ---- Keras surface
    def get_config(self):
        lr = self._learning_rate
        if callable(lr):
            lr = {"class_name": type(lr).__name__, "config": lr.get_config() if hasattr(lr, "get_config") else dict(vars(lr))}
        return {"name": self._name, "learning_rate": lr, "decay": self.decay, **self._hyper()}

    @classmethod
    def from_config(cls, config, custom_objects=None):
        config = dict(config)
        if "lr" in config:
            config["learning_rate"] = config.pop("lr")
        lr = config.get("learning_rate")
        if isinstance(lr, dict):
            from . import callbacks
            sched = (custom_objects or {}).get(lr["class_name"]) or getattr(callbacks, lr["class_name"])
            config["learning_rate"] = sched(**lr["config"])
        return cls(**config)

    def static_config(self):
        """What shapes the launch (kernel variant and the constants baked into its arguments); learning rate and decay are
        per-step scalars and are not part of it."""
        return tuple(sorted(self._hyper().items()))

    # ---- the per-step scalar
    def lr_at(self, k):
        """Keras ``_decayed_lr`` at iteration ``k``."""
        lr = self._learning_rate
        lr = float(lr(k)) if callable(lr) else float(lr)
        if self.decay > 0:
            lr /= 1.0 + self.decay * k
        return lr

    def _scalar(self, k):
        return self.lr_at(k)

    def _advance(self):
        """The scalar of the next update; advances ``iterations``."""
        s = self._scalar(self.iterations)
        self.iterations += 1
        return s

    # ---- slots
    def _slot_names(self):
        raise NotImplementedError

    def attach(self, store):
        """Makes ``store.m`` / ``store.v`` / ``store.s3`` this optimizer's slots of that network (see the module docstring)."""
        if store.slot_owner is self and (store.s3 is not None or "s3" not in self._slot_names()):
            return
        store.ensure_opt_state()
        bufs = self._slot_bufs.get(store)
        if bufs is None:
            if store.slot_owner is None:
                bufs = [store.m, store.v, store.s3]
            else:
                bufs = [torch.zeros_like(store.theta), torch.zeros_like(store.theta), None]
            self._slot_bufs[store] = bufs
        if "s3" in self._slot_names() and bufs[2] is None:
            bufs[2] = torch.zeros_like(store.theta)
        store.m, store.v, store.s3 = bufs
        store.slot_owner = self

    def apply(self, store):
        """One update of the network whose flat buffers ``store`` holds, from ``store.grad`` (all-reduced under data parallelism)."""
        self.attach(store)
        rec = program.active()
        if rec is not None:                 # step program: the recorded launch takes the scalar of the NEXT iteration from a slot
            rec.bind_scalar(self._bind_kind(), self._advance)
        n = store.n_train
        self._launch(store.theta[:n], store.m[:n], store.v[:n], None if store.s3 is None else store.s3[:n], store.grad[:n],
                     self._advance())
        store.tr_dirty = True

    def _bind_kind(self):
        return _lib.BIND_OPT_LR

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items() if k != 'name')})"


class SGD(Optimizer):
    """tf.keras.optimizers.SGD(learning_rate=0.01, momentum=0.0, nesterov=False)."""

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, name="SGD", **kwargs):
        if not _is_number(momentum) or momentum < 0 or momentum > 1:
            raise ValueError("`momentum` must be between [0, 1].")
        super().__init__(name, learning_rate, **kwargs)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)

    def _hyper(self):
        return {"momentum": self.momentum, "nesterov": self.nesterov}

    def _slot_names(self):
        return ("m",) if self.momentum > 0 else ()

    def _launch(self, theta, m, v, s3, g, lr):
        ops.sgd(theta, m if self.momentum > 0 else None, g, lr, self.momentum, self.nesterov)


class RMSprop(Optimizer):
    """tf.keras.optimizers.RMSprop(learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-07, centered=False).  Keras' two
    epsilon placements are kept: outside the root without momentum, inside it with momentum (the fused TF kernels)."""

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, name="RMSprop", **kwargs):
        for k, x in (("rho", rho), ("momentum", momentum)):
            if not _is_number(x):
                raise ValueError(f"`{k}` must be a number, got {x!r}")
        if momentum < 0:
            raise ValueError(f"`momentum` must be non-negative, got {momentum}")
        if epsilon is not None and not _is_number(epsilon):
            raise ValueError(f"`epsilon` must be a number, got {epsilon!r}")
        super().__init__(name, learning_rate, **kwargs)
        self.rho, self.momentum = float(rho), float(momentum)
        self.epsilon = float(epsilon or _EPSILON)            # Keras: `epsilon or backend_config.epsilon()`
        self.centered = bool(centered)

    def _hyper(self):
        return {"rho": self.rho, "momentum": self.momentum, "epsilon": self.epsilon, "centered": self.centered}

    def _slot_names(self):
        return ("v",) + (("m",) if self.momentum > 0 else ()) + (("s3",) if self.centered else ())

    def _launch(self, theta, m, v, s3, g, lr):
        ops.rmsprop(theta, v, m if self.momentum > 0 else None, s3 if self.centered else None, g, lr, self.rho, self.momentum,
                    self.epsilon, self.centered)


class Adam(Optimizer):
    """tf.keras.optimizers.Adam(learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-07, amsgrad=False).  Without amsgrad
    the update is bg_adam_f32, the kernel (and program binding) of the constructor's default optimizer."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, name="Adam", **kwargs):
        for k, x in (("beta_1", beta_1), ("beta_2", beta_2)):
            if not _is_number(x):
                raise ValueError(f"`{k}` must be a number, got {x!r}")
        if epsilon is not None and not _is_number(epsilon):
            raise ValueError(f"`epsilon` must be a number, got {epsilon!r}")
        super().__init__(name, learning_rate, **kwargs)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = float(epsilon or _EPSILON)            # Keras: `epsilon or backend_config.epsilon()`
        self.amsgrad = bool(amsgrad)

    def _hyper(self):
        return {"beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon, "amsgrad": self.amsgrad}

    def _slot_names(self):
        return ("m", "v", "s3") if self.amsgrad else ("m", "v")

    def _scalar(self, k):
        t = k + 1
        return self.lr_at(k) * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def _bind_kind(self):
        return _lib.BIND_OPT_LR if self.amsgrad else _lib.BIND_ADAM_LR

    def _launch(self, theta, m, v, s3, g, lr_t):
        if self.amsgrad:
            ops.adam_amsgrad(theta, m, v, s3, g, lr_t, self.beta_1, self.beta_2, self.epsilon)
        else:
            ops.adam(theta, m, v, g, lr_t, self.beta_1, self.beta_2, self.epsilon)


SUPPORTED = (SGD, RMSprop, Adam)


def get_optimizer(model):
    """``model.optimizer``, checked: a step can only run one of the classes above."""
    opt = model.optimizer
    if not isinstance(opt, SUPPORTED):
        raise TypeError(f"{getattr(model, 'name', 'model')}.optimizer is {type(opt).__name__}; supported: "
                        + ", ".join(f"blurred_gan_amd.optimizers.{c.__name__}" for c in SUPPORTED))
    return opt
