"""Differentiable augmentation (DiffAugment, Zhao et al. 2020) in front of the critic, as ``WGAN(..., augment=...)``.

``DiffAugment`` is the configuration: which of ``color``, ``translation`` and ``cutout`` act, and the two ratios.  Every image
the critic sees -- fakes and reals of the D-step, the interpolates of the gradient penalty, the fakes of the G-step -- goes through
a per-sample random T(x) = L x + k after the blur (include/bgan.h "differentiable augmentation": ``bg_diffaug_f32``), and the
critic's input gradient comes back through L^T (``bg_diffaug_adjoint_f32``).  The draws are eight uniforms per sample from the
model's own counter-based stream; nothing here is state: a checkpoint carries only the stream position it already saves.

``AdaptiveAugment`` (ADA, Karras et al. 2020, "Training GANs with limited data") is DiffAugment with a probability: every operation
of the policy fires per sample and per pass with probability ``p`` (twelve uniforms per sample: the eight above and three gates;
include/bgan.h "adaptive augmentation": ``bg_diffaug_gated_f32``), and ``p`` is steered on the device towards a target value of the
overfitting heuristic r_t = E[sign(D(reals))] (``bg_ada_stats_f32`` / ``bg_ada_update_f32``).  Here the model does carry state: eight
floats in a device buffer of its own, which a checkpoint saves."""
from __future__ import annotations

import numbers

__all__ = ["DiffAugment", "AdaptiveAugment", "as_augment", "OPS"]

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


class AdaptiveAugment(DiffAugment):
    """DiffAugment whose operations fire per sample with probability ``p``, adapted during training.

    ``p``: the initial probability in [0, 1]; each operation of the policy is decided independently, per sample and per pass.
    ``target``: the value in (-1, 1) that r_t = E[sign(D(reals))] is steered towards: every ``interval`` critic steps p moves by
    sign(r_t - target) * (images seen in the interval) / ``speed_images``, clamped to [0, 1] (StyleGAN2-ADA's rule; ``speed_images``
    is its ada_kimg * 1000, the number of images over which p can travel from 0 to 1).  ``target=None`` switches the controller off:
    p stays what it is ("DiffAugment with probability").

    The heuristic reads the SIGN of the critic's real scores, so it needs a loss that anchors them around 0.  The hinge and the
    non-saturating loss do.  The Wasserstein loss is invariant to a shift of all scores: only its ``e_drift`` term holds them near
    0, and with ``e_drift = 0`` nothing does, so a model refuses that combination with a target (a fixed p is fine everywhere)."""

    def __init__(self, policy="color,translation,cutout", translation_ratio=0.125, cutout_ratio=0.5, p=0.0, target=0.6, interval=4,
                 speed_images=500_000):
        super().__init__(policy, translation_ratio, cutout_ratio)
        real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)
        if not (real(p) and 0.0 <= p <= 1.0):
            raise ValueError(f"AdaptiveAugment: `p` must be a number in [0, 1], got {p!r}")
        if target is not None and not (real(target) and -1.0 < target < 1.0):
            raise ValueError(f"AdaptiveAugment: `target` must be None or a number in (-1, 1), got {target!r}")
        if not (isinstance(interval, numbers.Integral) and not isinstance(interval, bool) and interval >= 1):
            raise ValueError(f"AdaptiveAugment: `interval` must be an integer >= 1, got {interval!r}")
        if not (real(speed_images) and speed_images > 0 and speed_images != float("inf")):
            raise ValueError(f"AdaptiveAugment: `speed_images` must be a finite number > 0, got {speed_images!r}")
        self.p = float(p)
        self.target = None if target is None else float(target)
        self.interval = int(interval)
        self.speed_images = float(speed_images)

    @property
    def adaptive(self):
        """Whether the controller runs (a target is set)."""
        return self.target is not None

    def get_config(self):
        return dict(super().get_config(), p=self.p, target=self.target, interval=self.interval, speed_images=self.speed_images)

    def static_config(self):
        """The setting as part of a step program's key: the configuration (initial p included), never the live p."""
        return ("adaptive",) + tuple(sorted(self.get_config().items(), key=lambda kv: kv[0]))

    def __eq__(self, other):
        return isinstance(other, AdaptiveAugment) and self.get_config() == other.get_config()

    def __hash__(self):
        return hash(self.static_config())

    def __repr__(self):
        return f"AdaptiveAugment({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


class GatedAugment:
    """An AdaptiveAugment bound to the device float its launches read p from: what the engine's augmentation calls receive in place
    of the configuration (engine.Net.aug_forward / aug_linear / aug_backward go to the gated entry points when they see ``gate``)."""
    row_floats = 12

    def __init__(self, config, state):
        self.config, self.gate = config, state[:1]

    def kernel_args(self):
        return self.config.kernel_args()


def add_ada_arguments(parser):
    """The demos' adaptive-augmentation flags, next to their ``--diffaugment POLICY``."""
    d = AdaptiveAugment()

    def target(s):
        return None if s.strip().lower() == "none" else float(s)

    parser.add_argument("--ada", action="store_true",
                        help="adaptive augmentation (Karras et al. 2020): every operation of --diffaugment POLICY (alone: the full policy) "
                             "fires per sample with a probability p steered by the sign of the critic's real scores")
    parser.add_argument("--ada-target", dest="ada_target", type=target, default=d.target, metavar="R",
                        help=f"the value of E[sign(D(reals))] p is steered towards (default {d.target}); 'none': p stays at --ada-p")
    parser.add_argument("--ada-interval", dest="ada_interval", type=int, default=d.interval, metavar="K",
                        help=f"critic steps between two adjustments of p (default {d.interval})")
    parser.add_argument("--ada-speed-images", dest="ada_speed_images", type=float, default=d.speed_images, metavar="N",
                        help=f"images over which p can travel from 0 to 1 (default {int(d.speed_images)})")
    parser.add_argument("--ada-p", dest="ada_p", type=float, default=d.p, metavar="P",
                        help=f"the initial (with --ada-target none: the fixed) probability (default {d.p})")
    return parser


def augment_from_args(args):
    """``augment=`` from the demos' flags: None, the --diffaugment policy string, or with --ada an AdaptiveAugment over it."""
    if not getattr(args, "ada", False):
        return args.diffaugment
    policy = AdaptiveAugment().policy if args.diffaugment is None else args.diffaugment
    return AdaptiveAugment(policy, p=args.ada_p, target=args.ada_target, interval=args.ada_interval, speed_images=args.ada_speed_images)


def as_augment(value):
    """``augment=`` of the model constructors: None, a policy string, a DiffAugment or an AdaptiveAugment -> one that acts, or None."""
    if value is None:
        return None
    if isinstance(value, str):
        value = DiffAugment(value)
    if not isinstance(value, DiffAugment):
        raise ValueError(f"augment must be None, a policy string, a DiffAugment or an AdaptiveAugment, got {value!r}")
    return value if value.active else None
