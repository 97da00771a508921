"""Mirror of reference wgan.py: ``WGAN``, ``WGANGP``, ``gradient_penalty``, ``TrainingConfig`` with the same
constructor, attributes and method names, executing on the HIP kernels (no tape, no torch autograd).

Step order, training flags and loss algebra follow wgan.py:86-172, 234-285 including its quirks
(SURVEY.md 8a Q1, Q2, Q4, Q6); each quirk that changes numbers is a named constructor switch.
"""
from __future__ import annotations

import numbers
import os
from contextlib import contextmanager
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from . import _lib, diffaugment, dist, ema as ema_mod, objective as objective_mod, ops, optimizers, program
from .gaussian_blur import Variable
from .layers import Sequential, StyleModulation, get_seed
from .utils import JsonSerializable, ParseableFromCommandLine

# the switches the engine / the library read per call that shape a step's launch list ("per call (step key)")
_KEY_ENV = ("BGAN_NO_FUSED_BLUR3", "BGAN_NO_FUSED_BN_STATS", "BG_BLUR_BAND_LD", "BG_BLUR_NO_ROWS", "BG_BLUR_NO_PANEL", "BG_BLUR_PANEL16")


def _env_switches():
    """The per-call switches change a step's launch list: part of the step-program key, so flipping one mid-run records a new
    program instead of replaying a stale launch list."""
    return tuple(os.environ.get(k) for k in _KEY_ENV)


def _plain(v):
    """Hyper-parameter values as plain Python scalars (np.float32(1e-3) and 1e-3 must give the same program key)."""
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (numbers.Integral, np.integer)):
        return int(v)
    if isinstance(v, (numbers.Real, np.floating)):
        return float(v)
    return v


@dataclass
class TrainingConfig(JsonSerializable, ParseableFromCommandLine):
    """Parameters related to the training configuration of the Model (wgan.py:19-25)."""
    log_dir: str = "results/log"
    checkpoint_dir: str = "results/log/checkpoints"
    save_image_summaries_interval: int = 50


class Mean:
    """tf.keras.metrics.Mean stand-in (host side)."""

    def __init__(self, name, dtype=None):
        self.name = name
        self.reset_states()

    def reset_states(self):
        self.total, self.count = 0.0, 0

    def __call__(self, value, weight=1):
        self.total += float(value) * weight
        self.count += weight

    update_state = __call__

    def result(self):
        return self.total / self.count if self.count else 0.0


class _SummaryWriter:
    """Very small stand-in for tf.summary's file writer: scalars appended to <log_dir>/scalars.jsonl."""

    def __init__(self, log_dir):
        self.log_dir = log_dir
        self._fh = None

    @contextmanager
    def as_default(self):
        yield self

    def scalar(self, name, value, step=None):
        import json
        if self._fh is None:
            os.makedirs(self.log_dir, exist_ok=True)
            self._fh = open(os.path.join(self.log_dir, "scalars.jsonl"), "a")
        self._fh.write(json.dumps({"name": name, "value": float(value), "step": None if step is None else int(step)}) + "\n")
        self._fh.flush()


class WGAN:
    """Wasserstein GAN (wgan.py:28-231)."""

    @dataclass
    class HyperParameters(JsonSerializable, ParseableFromCommandLine):
        """Dataclass containing the hyperparameters of the Model (wgan.py:34-43)."""
        learning_rate: float = 0.001
        d_steps_per_g_step: int = 1
        batch_size: int = 32
        global_batch_size: int = 32
        optimizer: str = "adam"

    uses_gradient_penalty = False

    def __init__(self, generator: Sequential, discriminator: Sequential, hyperparams: "WGAN.HyperParameters",
                 config: TrainingConfig, *args, reproduce_vector_loss_quirk: bool = True, sync_metrics: bool = True,
                 sync_batchnorm: bool = True, merge_critic_passes: bool = True, gp_zero_norm_guard: bool = False,
                 merge_gp_filter_gradients: bool = True, step_replay: bool = True, persistent_input: bool = False,
                 conv_math: str = "fp32", generator_ema=None, augment=None, objective=None, latent_distribution: str = "uniform",
                 **kwargs):
        ops.conv_math_code(conv_math)        # ValueError before anything is built
        if latent_distribution not in ("uniform", "normal"):
            raise ValueError(f"latent_distribution must be 'uniform' or 'normal', got {latent_distribution!r}")
        augment = diffaugment.as_augment(augment)      # ValueError likewise
        ema_schedule = ema_mod.as_schedule(generator_ema)      # ValueError likewise
        objective = objective_mod.as_objective(objective, self.uses_gradient_penalty)      # ValueError likewise
        adaptive = isinstance(augment, diffaugment.AdaptiveAugment)
        if adaptive and augment.adaptive and objective.loss == "wasserstein" and \
                not (self.uses_gradient_penalty and float(getattr(hyperparams, "e_drift", 0.0)) != 0.0):
            # r_t reads the SIGN of the real scores; the Wasserstein loss is invariant to a shift of all scores and only the drift
            # term holds them near 0 (diffaugment.AdaptiveAugment)
            raise ValueError("AdaptiveAugment with a target under loss='wasserstein' needs e_drift != 0: nothing else anchors the "
                             "sign of the critic's real scores (use a fixed p with target=None, or the hinge / nonsaturating loss)")
        self.hparams = hyperparams
        if dist.world_size() > 1 and int(hyperparams.global_batch_size) != int(hyperparams.batch_size) * dist.world_size():
            import warnings
            # Q2: the reference never writes the true global batch into the hyper-parameters; under data parallelism the loss
            # scale 1/global_batch_size and the penalty's global mean must agree, so say so instead of training a different model
            warnings.warn(f"global_batch_size={hyperparams.global_batch_size} but {dist.world_size()} replicas x batch_size="
                          f"{hyperparams.batch_size}: the Wasserstein / penalty gradient ratio differs from the single-device "
                          "step at the global batch (set global_batch_size = batch_size * replicas)")
        if str(self.hparams.optimizer).lower() != "adam":
            raise NotImplementedError("of the optimizer names only the reference's default 'adam' is implemented (wgan.py:43,56); "
                                      "other optimizers are objects assigned after construction, e.g. "
                                      "gan.discriminator.optimizer = blurred_gan_amd.optimizers.RMSprop(5e-5)")
        # Keras optimizer objects (optimizers.py); any supported one may be assigned to either network at any time
        self.generator = generator
        self.generator.build()
        if ema_schedule is not None and self.generator.net().spectral_layers:
            raise NotImplementedError("generator_ema with a spectrally normalised generator: an averaged vector_u is no unit vector, and "
                                      "the averaged model would need a power iteration of its own")
        self.generator.optimizer = optimizers.Adam(self.hparams.learning_rate)
        self.discriminator = discriminator
        self.discriminator.build()
        if any(l.kind == "pixelnorm" for l, _ in self.discriminator.flat_layers()):
            raise NotImplementedError("PixelNormalization in the discriminator: the layer is the generator's normalisation; a critic with "
                                      "it has no gradient-penalty route (PixelNormalization in a critic under the gradient penalty is not "
                                      "built)")
        if any(l.kind == "noise" for l, _ in self.discriminator.flat_layers()):
            raise NotImplementedError("NoiseInjection in the discriminator: the layer is the generator's noise input; a critic with it "
                                      "has no gradient-penalty route (NoiseInjection in a critic under the gradient penalty is not built)")
        if any(isinstance(l, StyleModulation) for l, _ in self.discriminator.flat_layers()):
            raise NotImplementedError("StyleModulation in the discriminator: the layer is the generator's modulated convolution; a critic "
                                      "with it has no gradient-penalty route (StyleModulation in a critic under the gradient penalty is not "
                                      "built)")
        self.discriminator.optimizer = optimizers.Adam(self.hparams.learning_rate)
        self.d_steps_per_g_step = self.hparams.d_steps_per_g_step
        self.batch_size = None
        self.config = config
        self.summary_writer = _SummaryWriter(config.log_dir)
        self.n_img = Variable(0, name="n_img", dtype=int)
        self.n_batches = Variable(0, name="n_batches", dtype=int)
        self.real_scores_metric = Mean("real_scores")
        self.fake_scores_metric = Mean("fake_scores")
        self.gen_loss_metric = Mean("gen_loss")
        self.disc_loss_metric = Mean("disc_loss")
        self.optimizer = "unused"
        self.stop_training = False
        self.images = None
        # --- build-side switches (documented in DESIGN.md)
        self.reproduce_vector_loss_quirk = reproduce_vector_loss_quirk
        # Metrics live in one 16-float device buffer (critic step [0:8], generator step [8:12]).  train_on_batch reads it ONCE,
        # after the last kernel of the step has been enqueued (asynchronous copy into pinned memory + event wait): the one
        # host<->device synchronisation of a step, where Keras' train_on_batch converts its metric tensors (wgan.py:114).
        # sync_metrics=False skips even that (the returned metrics are then zeros): a measuring aid, never used by bench.py.
        self.sync_metrics = sync_metrics
        self._defer_metrics = False
        self._met_host = None
        self._met_event = None
        self.sync_batchnorm = sync_batchnorm  # DP: generator BN statistics over the global batch (False = per replica)
        # critic step: [fakes; reals] and x-hat in one 3B-sample forward / backward (False: two passes, as the reference orders them)
        self.merge_critic_passes = merge_critic_passes
        # the penalty's second-order filter gradients ride in the merged pass's own filter-gradient launches
        # (engine.Net.gp_second_order_merged); needs the merged critic pass
        self.merge_gp_filter_gradients = merge_gp_filter_gradients
        # a sample whose critic input-gradient is exactly zero makes the penalty's second-order seed (n-1)/n * g = NaN, in the
        # reference too (tf.norm's gradient at 0); True takes the subgradient 0 for that sample instead
        self.gp_zero_norm_guard = gp_zero_norm_guard
        # train_on_batch records the launch list of its discriminator_step / generator_step once and replays it with one call
        # into the library (program.py, include/bgan.h bg_dstep / bg_gstep); False or BGAN_NO_STEP_REPLAY=1: every step eager
        self.step_replay = step_replay and program.enabled_by_env()
        self._programs = program.StepPrograms()
        self._reals_stage = None
        self.persistent_input = bool(persistent_input)
        self._rng_seed = get_seed()
        self._rng_off = 0
        self._bufs = {}
        self._injected = None
        # the latents' distribution: "uniform" on [0, 1) (the reference's tf.random.uniform, wgan.py:118) or "normal", N(0, I) (the
        # draw the ProGAN / StyleGAN papers take; with it normalize_latents=True normalises what they normalise).  Either comes from
        # the model's own stream and counter, one launch per draw
        self.latent_distribution = latent_distribution
        # weight averaging (ema.py): None / a decay / a GeneratorEMA.  generator_ema is the averaged model -- the generator's
        # structure in its own ParamStore, bit-copies of the live weights and BatchNorm statistics now -- and generator_step
        # updates it with one launch after the optimizer; generate_samples(ema=True) runs it.  Off: nothing is allocated or launched
        self.generator_ema_config = ema_schedule
        self.generator_ema = None if ema_schedule is None else ema_mod.clone_structure(self.generator)
        self.generator_ema_updates = 0
        self.conv_math = conv_math
        # differentiable augmentation (diffaugment.py): None / a policy string / a DiffAugment.  Every batch the critic sees inside
        # the training step -- D-step, G-step, the penalty's interpolates -- goes through a per-sample random T after the blur, and
        # the critic's input gradient comes back through L^T.  Configuration, not state; off (None, or an empty policy): no launch
        # and no draw is added.  self.images, generate_samples, the SWD callbacks and gradient_penalty() never see it
        self._augment = augment
        # adaptive augmentation (diffaugment.AdaptiveAugment): the gated launches read p from ada_state[0], a persistent device
        # buffer {p, acc_sign, acc_count, k, r_last, 0, 0, 0} that the controller kernels of the critic step update (with a target)
        # and a checkpoint saves; the engine gets the configuration bound to that address.  Slots 12 / 13 of the step's metric
        # buffer carry p and the last r_t to the host with the step's one read
        self._ada_state = None
        self._aug_bound = augment
        if adaptive:
            self._ada_state = torch.zeros(ops.ada.STATE_FLOATS, dtype=torch.float32, device=self.device)
            self._ada_stats = torch.zeros(ops.ada.STATS_FLOATS, dtype=torch.float32, device=self.device)
            self._aug_bound = diffaugment.GatedAugment(augment, self._ada_state)
            self.augment_p_metric = Mean("augment_p")
            self.augment_rt_metric = Mean("augment_rt")
            self.set_augment_p(augment.p)
        # the objective (objective.py): None / a loss name / an Objective.  The reference objective runs the reference's loss kernels,
        # launch for launch; any other goes through bg_gan_d_loss / bg_gan_g_loss / bg_gp_seed_target_f32, and with penalty_interval
        # k > 1 only every k-th critic step carries the penalty.  Configuration, not state: the phase is n_batches % k
        self._objective = objective
        if augment is not None and len(self.discriminator.net().in_shape) != 3:
            raise NotImplementedError("augment= needs a critic on [H, W, C] images")

    @property
    def conv_math(self):
        """Math of the conv forward / data-gradient launches of the training step and generate_samples: "fp32" (default, the
        plain kernels) or "bf16x6" (opt-in split-bf16 kernel on the geometries of its dispatch table, include/bgan.h
        BG_CONV_MATH_BF16X6).  Filter gradients, dense GEMMs, BatchNorm, blur and Adam stay fp32 in either mode."""
        return self._conv_math

    @conv_math.setter
    def conv_math(self, value):
        ops.conv_math_code(value)
        self._conv_math = value
        self.generator.conv_math = value
        self.discriminator.conv_math = value
        if self.generator_ema is not None:
            self.generator_ema.conv_math = value

    @property
    def augment(self):
        """The DiffAugment (or AdaptiveAugment) in front of the critic, or None (the constructor's ``augment=``, normalised)."""
        return self._augment

    @property
    def augment_p(self):
        """The live probability of an AdaptiveAugment: ONE device read (not on the step path; the ``augment_p`` metric arrives with the
        step's own read).  None for a model without an AdaptiveAugment."""
        return None if self._ada_state is None else float(self._ada_state[0].item())

    def set_augment_p(self, value):
        """Writes the probability and clears the controller's accumulator and step count (r_last stays)."""
        if self._ada_state is None:
            raise ValueError("set_augment_p: this model has no AdaptiveAugment (construct it with augment=AdaptiveAugment(...))")
        if not (isinstance(value, numbers.Real) and not isinstance(value, bool) and 0.0 <= value <= 1.0):
            raise ValueError(f"set_augment_p: the probability must be a number in [0, 1], got {value!r}")
        r_last = float(self._ada_state[4].item())
        self._ada_state.copy_(torch.tensor([float(value), 0.0, 0.0, 0.0, r_last, 0.0, 0.0, 0.0], dtype=torch.float32))
        self._sync_ada_metric_slots()

    def _sync_ada_metric_slots(self):
        """Metric slots 12 / 13 <- {p, r_last} of the state: what the controller's launch leaves there, after a write from the host."""
        self._metrics_dev()[12:14].copy_(self._ada_state[[0, 4]])

    @property
    def objective(self):
        """The training objective (the constructor's ``objective=``, normalised to an Objective)."""
        return self._objective

    def _penalty_this_step(self):
        """Whether the critic step of the batch at hand carries the gradient penalty: the class has one, and the objective's
        interval says so (n_batches counts the finished batches)."""
        return self.uses_gradient_penalty and self._objective.penalty_at(self.n_batches)

    # ------------------------------------------------------------------ small helpers
    @property
    def device(self):
        return self.generator.store.device

    @property
    def latent_size(self):
        return self.generator.input_shape[-1]

    @property
    def metrics(self) -> List[Mean]:
        base = [self.real_scores_metric, self.fake_scores_metric, self.gen_loss_metric, self.disc_loss_metric]
        return base if self._ada_state is None else base + [self.augment_p_metric, self.augment_rt_metric]

    @property
    def metrics_names(self):
        return ["loss"] + [m.name for m in self.metrics]

    def reset_metrics(self):
        for m in self.metrics:
            m.reset_states()

    def _buf(self, name, shape, dtype=torch.float32):
        key = (name, tuple(shape), dtype)
        b = self._bufs.get(key)
        if b is None:
            b = self._bufs[key] = torch.empty(*shape, dtype=dtype, device=self.device)
        return b

    def _uniform(self, name, shape):
        """tf.random.uniform stand-in (wgan.py:118,237): own counter-based stream, seed + rank."""
        out = self._buf(name, shape)
        ops.uniform(out, self._rng_seed + 7919 * dist.rank(), counter=(self, "_rng_off"))
        return out

    def _latents(self, name, shape):
        """A batch of latents from the model's own stream, in the model's ``latent_distribution``."""
        if self.latent_distribution == "uniform":
            return self._uniform(name, shape)
        out = self._buf(name, shape)
        ops.rng.normal(out, self._rng_seed + 7919 * dist.rank(), counter=(self, "_rng_off"))
        return out

    def _inj(self, key):
        return None if self._injected is None else self._injected.get(key)

    def _noise_seed(self):
        """The seed of the noise maps a generator with NoiseInjection layers draws in its forwards: the generator network's own
        counter (``generator.net().rng_offset``) under a seed that differs per rank -- every replica sees its own noise -- and from
        the seeds of the critic's Dropout masks (104729 * (rank + 1)) and of the model's own stream (7919 * rank)."""
        return self._rng_seed + 15485863 * (dist.rank() + 1)

    def _noise_args(self, G, noise):
        """The keywords a forward of generator network ``G`` takes for its noise maps (none without NoiseInjection layers: such a
        forward is called as it always was).  ``noise``: None (drawn), maps [B, P], or False (left out)."""
        if not G.has_noise:
            return {}
        if noise is not None and noise is not False:
            noise = self._as_device(noise)
        return dict(seed=self._noise_seed(), noise=noise)

    def _aug_params(self, name, keys, B):
        """(DiffAugment, params [len(keys) * B, 8]) for one pass of the critic, or None without augmentation: ONE draw from the
        model's own stream for all row blocks of the pass, or the injected [B, 8] arrays ``keys`` names, stacked in that order.  With
        an AdaptiveAugment the rows are 12 wide (the three gates) and the configuration comes bound to the model's p."""
        if self._augment is None:
            return None
        cfg = self._aug_bound
        w = 8 if self._ada_state is None else cfg.row_floats
        inj = [self._inj(k) for k in keys]
        if any(a is not None for a in inj):
            if any(a is None for a in inj):
                raise ValueError(f"randomness: of {keys} either all or none are injected")
            for k, a in zip(keys, inj):
                if self._ada_state is not None and tuple(a.shape) != (B, w):
                    raise ValueError(f"randomness[{k!r}] must be [{B}, {w}] uniforms for {self._augment!r}, got {tuple(a.shape)}")
            return cfg, torch.cat([self._as_device(a).view(B, w) for a in inj], 0).contiguous()
        return cfg, self._uniform(name, (len(keys) * B, w))

    def _vec_scale(self, B):
        """Q1: the reference adds a [B] drift vector to the scalar loss, and GradientTape sums it, which
        multiplies the Wasserstein and GP gradients by the (global) batch size (wgan.py:279-285)."""
        return float(B * dist.world_size()) if (self.uses_gradient_penalty and self.reproduce_vector_loss_quirk) else 1.0

    # ------------------------------------------------------------------ reference API
    def train_on_batch(self, reals, *args, randomness=None, **kwargs):
        """wgan.py:86-114.  ``randomness`` (build-side, for parity tests) injects the step's random inputs:
        dict(z_d, z_g, alpha, mask_fake, mask_real) and, with ``augment``, the [B, 8] uniforms aug_fake, aug_real, aug_hat (D-step)
        and aug_g (G-step); [B, 12] with an AdaptiveAugment (columns 8..10: the gates of colour, translation, cutout); with a generator
        that has NoiseInjection layers noise_d / noise_g, the [B, P] noise maps of its forward in the D-step / G-step (per sample,
        the layers' maps in network order; P = generator.net().noise_pixels)."""
        self.reset_metrics()
        reals = self._as_device(reals)
        self.batch_size = int(reals.shape[0])
        if randomness is not None and not self.generator.net().has_noise and any(k in randomness for k in ("noise_d", "noise_g")):
            raise ValueError("randomness: noise_d / noise_g are the noise maps of a generator with NoiseInjection layers; this generator "
                             "has none")
        self._injected = randomness
        self._defer_metrics = True
        for model in (self.generator, self.discriminator):
            # the optimizers' slot buffers are in place before the step keys read their addresses
            optimizers.get_optimizer(model).attach(model.store)
        replay = self.step_replay and randomness is None and self._replayable()
        try:
            if replay:
                # a recorded program holds device addresses: the batch goes through ONE persistent staging buffer
                reals = self._stage_reals(reals)
                stream = ops._stream()
                with ops.trace_range("d_step"):
                    disc_loss, self.images = self._programs.run(self._step_key("d", reals), lambda: self.discriminator_step(reals),
                                                                stream, self._exit_state)
                    if self._programs.last_was_replay:
                        self._after_d_step()
                g_ran = int(self.n_batches) % self.d_steps_per_g_step == 0
                if g_ran:
                    with ops.trace_range("g_step"):
                        self._programs.run(self._step_key("g", reals), self.generator_step, stream, self._exit_state)
            else:
                with ops.trace_range("d_step"):
                    disc_loss, self.images = self.discriminator_step(reals)
                g_ran = int(self.n_batches) % self.d_steps_per_g_step == 0
                if g_ran:
                    with ops.trace_range("g_step"):
                        self.generator_step()
        finally:
            self._injected = None
            self._defer_metrics = False
        if self.sync_metrics:
            m = self._read_metrics()
            self._record_d_metrics(m[:8])
            if g_ran:
                self._record_g_metrics(m[8:12])
            self._record_ada_metrics(m)
        self.log_image_summaries()
        self.n_img.assign_add(self.batch_size)
        self.n_batches.assign_add(1)
        return self._organize_metrics()

    def _after_d_step(self):
        """Host-side bookkeeping of discriminator_step that a replayed step program has to repeat (subclasses)."""

    # ---- step programs (program.py)
    def _replayable(self):
        G, D = self.generator.net(), self.discriminator.net()
        return self.device.type == "cuda" and G.capture_branches is None and D.capture_branches is None

    def _stage_reals(self, reals):
        """The batch a recorded program reads.  A program holds device addresses, so by default the batch goes through ONE
        persistent staging buffer (a copy of the batch per step, 4-10 us).  ``persistent_input = True`` (constructor keyword or
        attribute) is the caller's promise that its batches arrive in device buffers that stay allocated and are refilled in
        place (a prefetcher with one or two device buffers): programs are then recorded on those buffers directly -- the address
        is part of the program key -- and no copy is made."""
        if self.persistent_input:
            return reals
        # one staging buffer PER BATCH SHAPE, kept for the life of the model: recorded programs hold its address, so a buffer that
        # was re-allocated on every shape switch (the partial last batch of an epoch) would strand the programs of both shapes at
        # each switch -- two eager steps and a recording per step kind, every epoch
        if self._reals_stage is None:
            self._reals_stage = {}
        key = (tuple(reals.shape), reals.dtype, reals.device)
        st = self._reals_stage.get(key)
        if st is None:
            st = self._reals_stage[key] = torch.empty_like(reals)
        if st.data_ptr() != reals.data_ptr():
            st.copy_(reals, non_blocking=True)
        return st

    def _step_key(self, kind, reals):
        """Everything that shapes the launch list of a step or is baked into its kernel arguments."""
        G, D = self.generator.net(), self.discriminator.net()
        hp = tuple(sorted((k, _plain(v)) for k, v in vars(self.hparams).items() if isinstance(v, (numbers.Number, np.generic, str, bool))))
        key = (kind, tuple(reals.shape), reals.data_ptr(), D.blur_n_taps(), G.store.tr_dirty, D.store.tr_dirty, self.merge_critic_passes,
               self.merge_gp_filter_gradients, self.sync_batchnorm, self.gp_zero_norm_guard, self.reproduce_vector_loss_quirk,
               self.sync_metrics, dist.collectives_active(), dist.world_size(), G.fuse_bn_stats, D.fuse_bn_stats,
               G.store.n_train, D.store.n_train, G.conv_math, D.conv_math, _env_switches(), hp,
               # spectral normalisation: the rounds per step, and whether the effective weights are stale on their own (a round taken by
               # hand between two steps clears sn_dirty and leaves tr_dirty: the step then skips a refresh a recorded program holds)
               G.spectral_rounds, D.spectral_rounds, G.store.sn_dirty, D.store.sn_dirty,
               self._optimizer_key(self.generator), self._optimizer_key(self.discriminator),
               # with penalty_interval k > 1 the critic steps with and without penalty are two programs that alternate and both
               # replay; the generator's step does not depend on the phase
               ("objective", self._objective.static_config(), self._penalty_this_step() if kind == "d" else None),
               # the latents' draw is another kernel.  (A generator with NoiseInjection layers needs no field: the layers are fixed
               # at construction, a program belongs to one model, and n_train differs from the same stack without them)
               self.latent_distribution)
        if G.has_mapping:
            mp = G.mapping
            key += (("mapping", mp.num_layers, G.style_dim, mp.lr_multiplier, mp.equalized_lr, mp.alpha, mp.w_avg_beta),)
        if self.generator_ema is not None:
            # the averaged model's presence, the two buffers the update writes and the schedule's static configuration: a program
            # recorded without the average, or on other buffers, never replays
            E = self.generator_ema.store
            key += (("generator_ema", E.theta.data_ptr(), E.state.data_ptr(), self.generator_ema_config.static_config()),)
        if self._augment is not None:
            key += (("augment", self._augment.static_config()),)
        if self._ada_state is not None:
            key += (("ada", self._ada_state.data_ptr(), self._ada_stats.data_ptr()),)
        return key

    @staticmethod
    def _optimizer_key(model):
        """A network's optimizer as it shapes the launch list: class, static configuration (variant, constants baked into the
        launch) and the addresses of its slot buffers (a program recorded on another optimizer's slots must never replay)."""
        opt, st = model.optimizer, model.store
        return (type(opt).__name__, opt.static_config(), *(0 if b is None else b.data_ptr() for b in (st.m, st.v, st.s3)))

    def _exit_state(self):
        G, D = self.generator.net(), self.discriminator.net()
        state = [(G.store, "tr_dirty", G.store.tr_dirty), (D.store, "tr_dirty", D.store.tr_dirty)]
        if self.generator_ema is not None:
            E = self.generator_ema.store
            state.append((E, "tr_dirty", E.tr_dirty))
        return state

    def _metrics_dev(self):
        return self._buf("step_metrics", (16,))

    def _read_metrics(self):
        """ONE device->host read of the step's metric buffer: asynchronous copy into pinned memory behind everything enqueued
        so far, then wait for that copy only."""
        dev = self._metrics_dev()
        if self._met_host is None:
            self._met_host = torch.empty(16, dtype=torch.float32, pin_memory=dev.is_cuda)
            self._met_event = torch.cuda.Event() if dev.is_cuda else None
        self._met_host.copy_(dev, non_blocking=True)
        if self._met_event is not None:
            self._met_event.record()
            self._met_event.synchronize()
        return self._met_host.tolist()

    def _record_d_metrics(self, m):
        self.fake_scores_metric(m[0])
        self.real_scores_metric(m[1])
        self.disc_loss_metric(m[2])
        self._record_gp_metrics(m)

    def _record_ada_metrics(self, m):
        """Slots 12 / 13 of the step's metric read: p and the last r_t as the critic step's controller launch left them."""
        if self._ada_state is not None:
            self.augment_p_metric(m[12])
            self.augment_rt_metric(m[13])

    def _ada_controller(self, real_scores):
        """The controller's two launches of a critic step, after the loss launch: the sign statistics of the critic's real scores
        (the un-penalised forward scores the loss used), summed over the replicas, then the update of p.  Recorded in a step
        program like any launch; nothing is bound and nothing is read."""
        cfg = self._augment
        if self._ada_state is None or not cfg.adaptive:
            return
        ops.ada.stats(real_scores, self._ada_stats)
        dist.all_reduce_sum_async(self._ada_stats).wait()       # one process: no collective
        ops.ada.update(self._ada_stats, self._ada_state, self._metrics_dev()[12:14], cfg.target, cfg.interval, 1.0 / cfg.speed_images)

    def _record_g_metrics(self, m):
        self.fake_scores_metric(m[0])                      # Q6: second update of the same Mean
        self.gen_loss_metric(m[1])

    def _as_device(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        return x.to(self.device, torch.float32).contiguous()

    def latents_batch(self):
        assert self.batch_size is not None
        return self._latents("latents", (self.batch_size, self.latent_size))

    @property
    def w_avg(self):
        """A host copy of the live generator's running mean of w (``layers.MappingNetwork``); None without a mapping network."""
        mp = self.generator.net().mapping
        return None if mp is None else mp.vars["w_avg"].detach().cpu().numpy().copy()

    def map_latents(self, z, ema=False, truncation_psi=None):
        """w = the mapping network of the (``ema``: averaged) generator on the latents ``z`` [B, L], behind the latents'
        normalisation where the generator has one; ``truncation_psi``: pulled towards that generator's ``w_avg``.  A fresh [B, units]
        tensor, what ``generate_samples(w=...)`` takes."""
        if ema and self.generator_ema is None:
            raise ValueError("map_latents(ema=True): this model has no averaged generator (construct it with generator_ema=...)")
        G = (self.generator_ema if ema else self.generator).net()
        if not G.has_mapping:
            raise ValueError("map_latents: this generator has no MappingNetwork (DCGANGenerator(mapping_layers=N, normalization='style'))")
        z = self._as_device(z)
        ctx = G.context(int(z.shape[0]), "map")
        if G.store.tr_dirty:
            G.prepare_weights()
        x = G.pn_latents(ctx, z) if G.latent_pn is not None else z
        w = G.mapping_forward(ctx, x)
        if truncation_psi is not None:
            w = G.mapping_truncate(ctx, w, truncation_psi)
        return w.clone()

    def generate_samples(self, latents=None, training=False, ema=False, noise=None, w=None, truncation_psi=None):
        """``w`` (a generator with a mapping network): styles [B, units] in place of latents (``map_latents``); ``truncation_psi``:
        the truncation trick, w <- w_avg + psi * (w - w_avg), inference only.  ``ema=True``: the averaged generator (``generator_ema=`` of the constructor), inference BatchNorm on its own averaged
        moving statistics.  ``noise`` (a generator with NoiseInjection layers): None draws fresh noise maps, a [B, P] tensor gives
        them, False leaves the noise out (engine.Net.forward)."""
        if ema and self.generator_ema is None:
            raise ValueError("generate_samples(ema=True): this model has no averaged generator (construct it with generator_ema=...)")
        if ema and training:
            raise ValueError("generate_samples(ema=True) runs inference BatchNorm: training=True would overwrite the averaged statistics")
        G = (self.generator_ema if ema else self.generator).net()
        style = {} if truncation_psi is None else dict(truncation_psi=truncation_psi)
        if w is not None:
            if latents is not None:
                raise ValueError("generate_samples: either latents or w (the styles, which skip the mapping network), not both")
            w = self._as_device(w)
            return G.forward(G.context(int(w.shape[0]), "g"), None, training=training, w=w, **style, **self._noise_args(G, noise))
        if latents is None:
            if self.batch_size is None:
                self.batch_size = self.hparams.batch_size
            latents = self.latents_batch()
        latents = self._as_device(latents)
        ctx = G.context(int(latents.shape[0]), "g")
        return G.forward(ctx, latents, training=training, **style, **self._noise_args(G, noise))

    # ---- discriminator
    def discriminator_loss(self, reals, fakes, real_scores, fake_scores):
        """wgan.py:128-130 (value only; the training step uses the fused device path), for the model's objective."""
        loss = self._objective.loss
        if loss == "hinge":
            terms = torch.relu(1.0 + fake_scores) + torch.relu(1.0 - real_scores)
        elif loss == "nonsaturating":
            terms = torch.nn.functional.softplus(fake_scores) + torch.nn.functional.softplus(-real_scores)
        else:
            terms = fake_scores - real_scores
        return terms.sum() * (1.0 / self.hparams.global_batch_size)

    def discriminator_step(self, reals):
        """wgan.py:132-151."""
        reals = self._as_device(reals)
        B = int(reals.shape[0])
        self.batch_size = B
        hp = self.hparams
        G, D = self.generator.net(), self.discriminator.net()
        D.check_rows(B)             # MinibatchStdDev: the slices of every pass of this step hold whole groups
        D.spectral_update()         # a spectrally normalised critic: its power round, before any forward of this step
        z = self._inj("z_d")
        z = self._as_device(z) if z is not None else self._latents("z_d", (B, self.latent_size))
        fakes = G.forward(G.context(B, "g_dstep"), z, training=False, **self._noise_args(G, self._inj("noise_d")))           # Q4: inference BN in the D-step
        # one draw for every row of the step's critic passes: fakes, reals and (with the penalty) x-hat, each with its own rows
        # penalty: this step carries the gradient penalty.  A WGANGP between two penalty steps of a lazy objective takes the
        # two-slice path of the plain WGAN -- no x-hat, no first or second order, no alpha or aug_hat draw -- with its own drift
        # term and vector-loss scale
        penalty = self._penalty_this_step()
        aug = self._aug_params("aug_d", ("aug_fake", "aug_real", "aug_hat")[:3 if penalty else 2], B)
        masks = None
        if self._inj("mask_fake") is not None:
            masks = [torch.cat([self._as_mask(a), self._as_mask(b)], 0)
                     for a, b in zip(self._inj("mask_fake"), self._inj("mask_real"))]
        inv_gbs = 1.0 / float(hp.global_batch_size)
        gp_c = float(getattr(hp, "gp_coefficient", 0.0)) * self._objective.penalty_interval if penalty else 0.0
        e_d = float(getattr(hp, "e_drift", 0.0)) if self.uses_gradient_penalty else 0.0
        met = self._metrics_dev()[:8]
        vs = self._vec_scale(B)
        store = self.discriminator.store
        store.ensure_opt_state()
        red = dist.GradReducer(store.grad, store.n_train)       # buckets go out while the backward is still running
        seed = self._rng_seed + 104729 * (dist.rank() + 1)
        merged = (penalty and self.merge_critic_passes and all(st.bn is None for st in D.stages))
        if merged:
            # [fakes; reals] (training=True: Dropout) and x-hat (training=False) share every weight: ONE 3B-sample pass forward
            # and ONE backward, the Dropout masks covering the first 2B samples only (bg_epilogue.keep_elems).  The seeds of
            # the backward do not depend on the penalty (d loss / d scores is +-1/gbs and the drift term), so the x-hat rows
            # ride along with seed 1 and come out as the zeta_i the second-order pass needs; weight gradients use rows [0, 2B),
            # the image gradient is taken for rows [2B, 3B) only.
            c3 = D.context(3 * B, "fr3", drop_rows=2 * B)
            # x-hat = reals + a (fakes - reals) (wgan.py:239) joins the batch inside forward: behind the blur it is formed on the fly
            # by the one launch that blurs all three slices (bg_blur3_lerp_nhwc_f32), else bg_lerp_f32 writes it to the buffer
            s3 = D.forward(c3, [fakes, reals], training=True, masks=masks, seed=seed, lerp_alpha=self._gp_alpha(B),
                           lerp_out=self._buf("xhat", tuple(reals.shape)), augment=aug).view(3 * B)
            fs, rs = s3[:B], s3[B:2 * B]
            ds3 = self._buf("ds3", (3 * B,))
            ops.fill(ds3[2 * B:], 1.0)
            self._d_loss(fs, rs, None, inv_gbs, gp_c, e_d, vs, ds3[:B], ds3[B:2 * B], met)      # seeds only; metrics below
            # a critic with LayerNormalization stages (or a MinibatchStdDev: any stage with a source term) takes the separate second-order route whatever the switch says: the merged one
            # overwrites the x-hat rows of the activations that the stages' source backward reads (engine.gp_second_order_merged)
            one_wgrad = self.merge_gp_filter_gradients and not D.has_source
            g = D.backward(c3, ds3.view(3 * B, 1), need_dx=True, need_dw=True, beta=0.0, scale=1.0, dw_rows=2 * B,
                           dx_rows=(2 * B, 3 * B), defer_conv_dw=one_wgrad, keep_u_rows=(2 * B, 3 * B))
            norms = ops.row_norm(g, self._buf("gp_norms", (B,)))
            self._d_loss(fs, rs, norms, inv_gbs, gp_c, e_d, vs, ds3[:B], ds3[B:2 * B], met)    # same seeds, full metrics
            self._ada_controller(rs)
            aug_hat = None if aug is None else (aug[0], aug[1][2 * B:3 * B])
            if one_wgrad:
                # delta-bar_0 goes into the x-hat rows of the pass's (blurred; with augment: augmented) input buffer, where the
                # layer-1 filter gradient reads it beside the activations of [fakes; reals]; g itself lives in those rows (with
                # augment: in the rows of a buffer of the pass that is dead by then) and is dead after the seed
                self._gp_v0(D, g, norms, out=(c3.a0 if aug is None else c3.aug_input())[2 * B:3 * B], aug=aug_hat)
                D.gp_second_order_merged(c3, 2 * B, 3 * B, reducer=red)
            else:
                D.gp_second_order(c3.rows(2 * B, 3 * B), self._gp_v0(D, g, norms, aug=aug_hat), reducer=red)
        else:
            cfr = D.context(2 * B, "fr")
            s2 = D.forward(cfr, [fakes, reals], training=True, masks=masks, seed=seed,
                           augment=None if aug is None else (aug[0], aug[1][:2 * B])).view(2 * B)
            fs, rs = s2[:B], s2[B:]
            norms = g = None
            aug_hat = None if aug is None or not penalty else (aug[0], aug[1][2 * B:3 * B])
            if penalty:
                norms, g = self._gp_first_order(reals, fakes, aug_hat)
            ds2 = self._buf("ds2", (2 * B,))
            self._d_loss(fs, rs, norms, inv_gbs, gp_c, e_d, vs, ds2[:B], ds2[B:], met)
            self._ada_controller(rs)
            D.backward(cfr, ds2.view(2 * B, 1), need_dx=False, need_dw=True, beta=0.0, scale=1.0,
                       reducer=None if penalty else red)
            if penalty:
                D.gp_second_order(D.context(B, "hat"), self._gp_v0(D, g, norms, aug=aug_hat), reducer=red)
        red.finish()
        D.spectral_project_gradients()
        D.eqlr_scale_gradients()    # an equalised-learning-rate critic: dL/dW = c * dL/dW_eff
        optimizers.get_optimizer(self.discriminator).apply(store)
        disc_loss = None              # inside train_on_batch the value is read with the rest of the step's metrics
        if self.sync_metrics and not self._defer_metrics:
            m = self._read_metrics()
            self._record_d_metrics(m[:8])
            self._record_ada_metrics(m)
            disc_loss = m[2]
        return disc_loss, (fakes, reals)

    def _record_gp_metrics(self, m):
        pass

    def _d_loss(self, fs, rs, norms, inv_gbs, gp_c, e_d, vs, dfs, drs, met):
        """The critic's loss launch: the reference objective through the reference's kernel, any other through bg_gan_d_loss."""
        obj = self._objective
        if obj.is_reference:
            return ops.wgangp_d_loss(fs, rs, norms, inv_gbs, gp_c, e_d, vs, dfs, drs, met)
        return ops.objective.d_loss(fs, rs, norms, ops.objective.LOSS[obj.loss], inv_gbs, gp_c, obj.penalty_target, e_d, vs, dfs, drs, met)

    def _gp_seed(self, g, norms, coef, out):
        obj = self._objective
        if obj.is_reference:
            return ops.gp_seed(g, norms, coef, out, self.gp_zero_norm_guard)
        return ops.objective.gp_seed(g, norms, coef, obj.penalty_target, out, self.gp_zero_norm_guard)

    @staticmethod
    def _as_mask(a):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(a)
        return a.to(torch.uint8)

    def _gp_alpha(self, B):
        """The interpolation weights of x-hat (wgan.py:237): injected, or drawn; where the objective puts the penalty on the reals
        or on the fakes, the constant 0 or 1, written by a launch (a step program records it) with nothing drawn or injected."""
        const = self._objective.penalty_alpha
        if const is not None:
            return ops.fill(self._buf("alpha", (B,)), const)
        a = self._inj("alpha")
        return self._as_device(a).view(B) if a is not None else self._uniform("alpha", (B,))

    def _gp_coef(self, B):
        """d/dW of vec_scale * gp_coefficient * mean_global((n-1)^2): the second order's seed carries the whole factor (a lazy
        objective: times its interval, on the steps that carry the penalty)."""
        k = self._objective.penalty_interval
        return self._vec_scale(B) * float(self.hparams.gp_coefficient) * k * 2.0 / float(B * dist.world_size())

    def _gp_v0(self, D, g, norms, out=None, aug=None):
        """The second order's input delta-bar_0: the seed of the image gradient ``g``, through the blur where the critic has one
        and, with ``aug`` = (DiffAugment, the x-hat rows' params), through the linear part L of their augmentation: v0 =
        L(blur(g-bar)).  Lands in ``out`` (the x-hat rows of the merged pass's input buffer) or in a buffer of the model's own."""
        own = lambda name: self._buf(name, tuple(g.shape))
        coef = self._gp_coef(int(g.shape[0]))
        if aug is not None:
            v = self._gp_seed(g, norms, coef, own("gbar"))
            if D.blur is not None:
                v = D.apply_blur(v, own("v0_blur"))
            return D.aug_linear(*aug, v, own("v0") if out is None else out)
        if D.blur is None:      # with ``out``, g is the net's own input-gradient buffer
            return self._gp_seed(g, norms, coef, own("gbar") if out is None else out.view(g.shape))
        gbar = self._gp_seed(g, norms, coef, own("gbar"))
        return D.apply_blur(gbar, own("v0") if out is None else out)

    def _gp_first_order(self, reals, fakes, aug=None):
        """Leaves zeta_i in the 'hat' context for the second order."""
        B = int(reals.shape[0])
        D = self.discriminator.net()
        return _first_order(D, D.context(B, "hat"), reals, fakes, self._gp_alpha(B), self._buf("xhat", tuple(reals.shape)),
                            self._buf("ones", (B, 1)), self._buf("gp_norms", (B,)), keep_u=True, augment=aug)

    # ---- generator
    def generator_loss(self, fake_scores):
        """wgan.py:155-157, for the model's objective."""
        if self._objective.loss == "nonsaturating":
            return torch.nn.functional.softplus(-fake_scores).sum() * (1.0 / self.hparams.global_batch_size)
        return -fake_scores.sum() * (1.0 / self.hparams.global_batch_size)

    def generator_step(self):
        """wgan.py:159-172."""
        B = self.batch_size
        G, D = self.generator.net(), self.discriminator.net()
        G.spectral_update()         # a spectrally normalised generator: its power round
        z = self._inj("z_g")
        z = self._as_device(z) if z is not None else self._latents("z_g", (B, self.latent_size))
        cg = G.context(B, "g")
        G.sync_bn = self.sync_batchnorm
        fakes = G.forward(cg, z, training=True, **self._noise_args(G, self._inj("noise_g")))
        if G.has_mapping: G.w_avg_update(cg, B * dist.world_size())      # noqa: E701  (the running mean of w: the G-step's batches only)
        chat = D.context(B, "hat")
        s = D.forward(chat, fakes, training=False, augment=self._aug_params("aug_g", ("aug_g",), B)).view(B)
        ds = self._buf("ds_g", (B,))
        met = self._metrics_dev()[8:12]
        if self._objective.is_reference:
            ops.wgan_g_loss(s, 1.0 / float(self.hparams.global_batch_size), ds, met)
        else:
            ops.objective.g_loss(s, ops.objective.LOSS[self._objective.loss], 1.0 / float(self.hparams.global_batch_size), ds, met)
        dfakes = D.backward(chat, ds.view(B, 1), need_dx=True, need_dw=False)
        store = self.generator.store
        store.ensure_opt_state()
        red = dist.GradReducer(store.grad, store.n_train)
        G.backward(cg, dfakes, need_dx=False, need_dw=True, beta=0.0, scale=1.0, reducer=red)
        red.finish()
        G.spectral_project_gradients()
        G.eqlr_scale_gradients()
        optimizers.get_optimizer(self.generator).apply(store)
        if self.generator_ema is not None:
            self._update_generator_ema()
        if self.sync_metrics and not self._defer_metrics:
            m = self._read_metrics()
            self._record_g_metrics(m[8:12])
            return m[1 + 8]
        return None

    # ---- weight averaging (ema.py)
    def _advance_generator_ema(self):
        """w = 1 - beta of the next update of the average, in double; advances ``generator_ema_updates``."""
        w = self.generator_ema_config.w_at(self.generator_ema_updates, self.batch_size, dist.world_size(), self.d_steps_per_g_step)
        self.generator_ema_updates += 1
        return w

    def _update_generator_ema(self):
        """avg -= w * (avg - theta) over the generator's trainable buffer and its BatchNorm moving statistics: one launch
        (bg_ema_f32).  Every data-parallel rank applies the same update to identical inputs, so nothing is communicated."""
        G, E = self.generator.store, self.generator_ema.store
        rec = program.active()
        if rec is not None:                 # step program: the recorded launch takes w of the NEXT update from a slot
            rec.bind_scalar(_lib.BIND_EMA_W, self._advance_generator_ema)
        n, n2 = G.n_train, G.n_state
        ops.ema(E.theta[:n], G.theta[:n], E.state[:n2] if n2 else None, G.state[:n2] if n2 else None, self._advance_generator_ema())
        E.tr_dirty = True                   # the transposed kernel copies are refreshed by the averaged model's next forward

    def reset_generator_ema(self):
        """averages <- live weights, update count <- 0 (after ``set_weights`` / ``load_weights`` on the live generator)."""
        if self.generator_ema is None:
            raise ValueError("reset_generator_ema: this model has no averaged generator (construct it with generator_ema=...)")
        G, E = self.generator.store, self.generator_ema.store
        E.theta.copy_(G.theta)
        E.state.copy_(G.state)
        E.tr_dirty = True
        self.generator_ema_updates = 0

    # ---- bookkeeping / Keras surface
    def log_image_summaries(self):
        """wgan.py:176-180: image summaries are a TensorBoard feature; not written by this build."""
        return None

    def _organize_metrics(self) -> List[float]:
        """wgan.py:182-200: [0.0] + metric results in metrics_names order."""
        by_name = {m.name: m for m in self.metrics}
        assert len(by_name) == len(self.metrics), "duplicate metric names"
        return [0.0] + [by_name[n].result() for n in self.metrics_names if n != "loss"]

    @contextmanager
    def record_image_summaries(self):
        yield

    def summary(self):
        print("Discriminator:")
        self.discriminator.summary()
        print("Generator:")
        self.generator.summary()
        print(f"Total params: {self.count_params():,}")

    def count_params(self):
        return self.discriminator.count_params() + self.generator.count_params()

    def save_weights(self, filepath, overwrite=True, save_format=None):
        """wgan.py:229-231."""
        self.discriminator.save_weights(filepath + "_discriminator", overwrite, save_format)
        self.generator.save_weights(filepath + "_generator", overwrite, save_format)
        if self.generator_ema is not None:
            self.generator_ema.save_weights(filepath + "_generator_ema", overwrite, save_format)

    def fit(self, x, y=None, epochs=1, initial_epoch=0, callbacks=None, steps_per_epoch=None, verbose=0):
        """The slice of ``tf.keras.Model.fit`` the reference demos rely on (demo_mnist.py:187-206): iterate
        batches, call the Keras callback hooks around ``train_on_batch``, honour ``stop_training``."""
        callbacks = list(callbacks or [])
        for cb in callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
            else:
                cb.model = self
        call = lambda name, *a: [getattr(cb, name)(*a) for cb in callbacks if hasattr(cb, name)]
        call("on_train_begin", {})
        history = []
        for epoch in range(int(initial_epoch), int(epochs)):
            call("on_epoch_begin", epoch, {})
            logs = {}
            for batch, reals in enumerate(x):
                if steps_per_epoch is not None and batch >= steps_per_epoch:
                    break
                size = int(reals.shape[0])
                call("on_batch_begin", batch, {"batch": batch, "size": size})
                values = self.train_on_batch(reals)
                logs = {"batch": batch, "size": size}
                logs.update(dict(zip(self.metrics_names, values)))
                call("on_batch_end", batch, logs)
                if self.stop_training:
                    break
            history.append(dict(logs))
            call("on_epoch_end", epoch, logs)
            if self.stop_training:
                break
        call("on_train_end", {})
        return history


def _first_order(D, ctx, reals, fakes, alpha, xhat, ones, norms, keep_u=False, augment=None):
    """wgan.py:234-245 on the device: x_hat, critic forward (training=False), gradient w.r.t. x_hat (through blur^T),
    per-sample L2 norms.  ``xhat``, ``ones`` and ``norms`` are the caller's buffers; returns (norms, gradient).  ``keep_u``: the
    second order follows, so LayerNormalization stages keep what its source term needs (engine.Net.backward keep_u_rows)."""
    D.forward(ctx, ops.lerp(reals, fakes, alpha, xhat), training=False, augment=augment)
    g = D.backward(ctx, ops.fill(ones, 1.0), need_dx=True, need_dw=False, keep_u_rows=(0, int(reals.shape[0])) if keep_u else None)
    return ops.row_norm(g, norms), g


def gradient_penalty(discriminator, reals, fakes, alpha=None, target=1.0):
    """wgan.py:234-246 (value only): mean((||d D(x_hat)/d x_hat|| - target)^2) on the HIP kernels."""
    if not (isinstance(target, numbers.Real) and target >= 0.0):
        raise ValueError(f"gradient_penalty: `target` must be a number >= 0, got {target!r}")
    D = discriminator.net()
    dev = D.device
    reals = reals.to(dev, torch.float32).contiguous()
    fakes = fakes.to(dev, torch.float32).contiguous()
    B = int(reals.shape[0])
    if alpha is None:
        alpha = ops.uniform(torch.empty(B, dtype=torch.float32, device=dev), get_seed() + 17, np.random.randint(1 << 30))
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    n, _ = _first_order(D, D.context(B, "gp_fn"), reals, fakes, alpha.to(dev, torch.float32).contiguous().view(B), torch.empty_like(reals),
                        new(B, 1), new(B))
    # mean((n - 1)^2) by the loss kernel itself (metric slot 5 of bg_wgangp_d_loss), not by torch arithmetic
    zero = ops.fill(torch.empty(B, dtype=torch.float32, device=dev), 0.0)
    scratch, met = torch.empty(2, B, dtype=torch.float32, device=dev), torch.empty(8, dtype=torch.float32, device=dev)
    if float(target) == 1.0:
        ops.wgangp_d_loss(zero, zero, n, 1.0, 0.0, 0.0, 1.0, scratch[0], scratch[1], met)
    else:
        ops.objective.d_loss(zero, zero, n, ops.objective.LOSS["wasserstein"], 1.0, 0.0, float(target), 0.0, 1.0, scratch[0], scratch[1], met)
    return met[5]


class WGANGP(WGAN):
    """Wasserstein GAN with Gradient Penalty loss (wgan.py:249-285)."""

    @dataclass
    class HyperParameters(WGAN.HyperParameters):
        """Hyperparameters of a WGAN model with Gradient Penalty loss (wgan.py:255-261)."""
        e_drift: float = 1e-4
        gp_coefficient: float = 10.0

    uses_gradient_penalty = True

    def __init__(self, generator, discriminator, hyperparams, config, *args, **kwargs):
        super().__init__(generator, discriminator, hyperparams, config, *args, **kwargs)
        self.gp_term_metric = Mean("gp_term")
        self.norm_term_metric = Mean("norm_term")

    @property
    def metrics(self):
        return super().metrics + [self.gp_term_metric, self.norm_term_metric]

    def _record_gp_metrics(self, m):
        self.gp_term_metric(m[3])
        self.norm_term_metric(m[4])

    def discriminator_loss(self, reals, fakes, real_scores, fake_scores):
        """wgan.py:272-285 (value only): a [B] vector, as in the reference.  The penalty is the objective's -- its target, at its
        points -- with the plain coefficient: what a lazy objective adds per step on average."""
        loss = super().discriminator_loss(reals, fakes, real_scores, fake_scores)
        obj = self._objective
        alpha = None if obj.penalty_alpha is None else torch.full((int(reals.shape[0]),), obj.penalty_alpha, device=self.device)
        gp_term = self.hparams.gp_coefficient * gradient_penalty(self.discriminator, reals, fakes, alpha, obj.penalty_target)
        norm_term = self.hparams.e_drift * (fake_scores.abs().view(-1) + real_scores.abs().view(-1))
        return loss + gp_term + norm_term
