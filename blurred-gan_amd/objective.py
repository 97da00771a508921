"""The training objective, as ``WGAN(..., objective=...)``: which loss the scores go through and what the gradient penalty is.

``Objective`` is the configuration.  ``loss`` names the pair of critic and generator losses (include/bgan.h ``bg_gan_loss``):
``wasserstein`` (the reference), ``hinge`` (SN-GAN, SAGAN, BigGAN) or ``nonsaturating`` (the logistic loss of the original GAN,
StyleGAN2, DiffAugment).  The penalty is ``gp_coefficient * mean((||g|| - penalty_target)^2)`` with g the critic's input gradient
at ``penalty_on``: the ``interpolates`` of reals and fakes (the reference, target 1), the ``reals`` (target 0: R1, with the paper's
gamma / 2 as ``gp_coefficient``) or the ``fakes`` (R2).  ``penalty_interval`` = k applies it lazily: on every k-th critic step,
with k times the coefficient; the steps between run no penalty pass at all.  Nothing here is state: the phase of the interval is
``n_batches % k``, which a checkpoint already restores."""
from __future__ import annotations

import numbers

__all__ = ["Objective", "as_objective", "LOSSES", "PENALTY_ON"]

LOSSES = ("wasserstein", "hinge", "nonsaturating")
PENALTY_ON = {"interpolates": None, "reals": 0.0, "fakes": 1.0}       # the constant alpha of x-hat = reals + alpha (fakes - reals)


class Objective:
    """``loss``: one of ``wasserstein``, ``hinge``, ``nonsaturating``.  ``penalty_target``: a number t >= 0.  ``penalty_on``: one of
    ``interpolates``, ``reals``, ``fakes``.  ``penalty_interval``: an integer k >= 1.  The defaults are the reference objective."""

    def __init__(self, loss="wasserstein", penalty_target=1.0, penalty_on="interpolates", penalty_interval=1):
        if not isinstance(loss, str) or loss not in LOSSES:
            raise ValueError(f"Objective: unknown loss {loss!r} (known: {', '.join(LOSSES)})")
        t = penalty_target
        if not (isinstance(t, numbers.Real) and not isinstance(t, bool) and 0.0 <= t < float("inf")):
            raise ValueError(f"Objective: `penalty_target` must be a finite number >= 0, got {t!r}")
        if not isinstance(penalty_on, str) or penalty_on not in PENALTY_ON:
            raise ValueError(f"Objective: unknown `penalty_on` {penalty_on!r} (known: {', '.join(PENALTY_ON)})")
        k = penalty_interval
        if not (isinstance(k, numbers.Integral) and not isinstance(k, bool) and k >= 1):
            raise ValueError(f"Objective: `penalty_interval` must be an integer >= 1, got {k!r}")
        self.loss = loss
        self.penalty_target = float(t)
        self.penalty_on = penalty_on
        self.penalty_interval = int(k)
        self.has_default_penalty = (self.penalty_target, self.penalty_on, self.penalty_interval) == (1.0, "interpolates", 1)
        # the reference's objective: the step then launches exactly what it launched before there was a choice
        self.is_reference = loss == "wasserstein" and self.has_default_penalty
        self._static = tuple(sorted(self.get_config().items()))

    @property
    def penalty_alpha(self):
        """The constant interpolation weight ``penalty_on`` stands for, or None where it is drawn."""
        return PENALTY_ON[self.penalty_on]

    def penalty_at(self, n_batches):
        """Whether the critic step that follows ``n_batches`` finished batches carries the penalty."""
        return self.penalty_interval == 1 or int(n_batches) % self.penalty_interval == 0

    def get_config(self):
        return {"loss": self.loss, "penalty_target": self.penalty_target, "penalty_on": self.penalty_on,
                "penalty_interval": self.penalty_interval}

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def static_config(self):
        """The setting as part of a step program's key."""
        return self._static

    def __eq__(self, other):
        return isinstance(other, Objective) and self.get_config() == other.get_config()

    def __hash__(self):
        return hash(self.static_config())

    def __repr__(self):
        return f"Objective({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


def as_objective(value, has_penalty=True):
    """``objective=`` of the model constructors: None (the reference objective), a loss name or an Objective -> an Objective.
    ``has_penalty`` False (a model class without gradient penalty): penalty fields other than the defaults are refused."""
    if value is None:
        value = Objective()
    elif isinstance(value, str):
        value = Objective(loss=value)
    if not isinstance(value, Objective):
        raise ValueError(f"objective must be None, a loss name or an Objective, got {value!r}")
    if not has_penalty and not value.has_default_penalty:
        raise ValueError(f"{value!r}: this model class has no gradient penalty, so penalty_target, penalty_on and penalty_interval "
                         "must be left at their defaults")
    return value
