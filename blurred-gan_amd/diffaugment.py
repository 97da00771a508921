"""Differentiable augmentation (DiffAugment, Zhao et al. 2020) in front of the critic, as ``WGAN(..., augment=...)``.

``DiffAugment`` is the configuration: which of ``color``, ``translation`` and ``cutout`` act, and the two ratios.  Every image
the critic sees -- fakes and reals of the D-step, the interpolates of the gradient penalty, the fakes of the G-step -- goes through
a per-sample random T(x) = L x + k after the blur (include/bgan.h "differentiable augmentation": ``bg_diffaug_f32``), and the
critic's input gradient comes back through L^T (``bg_diffaug_adjoint_f32``).  The draws are eight uniforms per sample from the
model's own counter-based stream; nothing here is state: a checkpoint carries only the stream position it already saves."""
from __future__ import annotations

import numbers

__all__ = ["DiffAugment", "as_augment", "OPS"]

OPS = {"color": 1, "translation": 2, "cutout": 4}       # include/bgan.h ops_mask bits


class DiffAugment:
    """``policy``: comma-separated names out of ``color``, ``translation``, ``cutout``, any subset in any order (the operations
    always apply in that order); an empty policy switches the augmentation off.  ``translation_ratio``: the largest shift as a
    fraction of the image extent; ``cutout_ratio``: the side of the cut square likewise.  Both in [0, 1]."""

    def __init__(self, policy="color,translation,cutout", translation_ratio=0.125, cutout_ratio=0.5):
        if not isinstance(policy, str):
            raise ValueError(f"DiffAugment: `policy` must be a string of comma-separated names, got {policy!r}")
        names = [p.strip() for p in policy.split(",") if p.strip()]
        for p in names:
            if p not in OPS:
                raise ValueError(f"DiffAugment: unknown operation {p!r} in policy {policy!r} (known: {', '.join(OPS)})")
        if len(set(names)) != len(names):
            raise ValueError(f"DiffAugment: an operation is named twice in policy {policy!r}")
        for name, v in (("translation_ratio", translation_ratio), ("cutout_ratio", cutout_ratio)):
            if not (isinstance(v, numbers.Real) and not isinstance(v, bool) and 0.0 <= v <= 1.0):
                raise ValueError(f"DiffAugment: `{name}` must be a number in [0, 1], got {v!r}")
        self.policy = ",".join(p for p in OPS if p in names)          # canonical: application order
        self.translation_ratio = float(translation_ratio)
        self.cutout_ratio = float(cutout_ratio)

    @property
    def ops_mask(self):
        return sum(OPS[p] for p in self.policy.split(",") if p)

    @property
    def active(self):
        return self.ops_mask != 0

    def get_config(self):
        return {"policy": self.policy, "translation_ratio": self.translation_ratio, "cutout_ratio": self.cutout_ratio}

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def static_config(self):
        """The setting as part of a step program's key."""
        return tuple(sorted(self.get_config().items()))

    def kernel_args(self):
        """The keywords every ops.diffaug call names the setting by."""
        return dict(ops_mask=self.ops_mask, translation_ratio=self.translation_ratio, cutout_ratio=self.cutout_ratio)

    def __eq__(self, other):
        return isinstance(other, DiffAugment) and self.get_config() == other.get_config()

    def __hash__(self):
        return hash(self.static_config())

    def __repr__(self):
        return f"DiffAugment({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


def as_augment(value):
    """``augment=`` of the model constructors: None, a policy string or a DiffAugment -> a DiffAugment that acts, or None."""
    if value is None:
        return None
    if isinstance(value, str):
        value = DiffAugment(value)
    if not isinstance(value, DiffAugment):
        raise ValueError(f"augment must be None, a policy string or a DiffAugment, got {value!r}")
    return value if value.active else None
