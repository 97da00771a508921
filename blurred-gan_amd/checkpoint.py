"""Checkpoint / resume: stands in for ``tf.train.Checkpoint(gan=gan)`` + ``CheckpointManager``
(demo_mnist.py:145-163, callbacks.py:239-246).  One ``.npz`` per checkpoint holding both networks' variables
(weights + BN moving statistics), both optimizers (class, ``get_config()`` as JSON, learning rate, step count and every slot
buffer in use), ``n_img``, ``n_batches``, ``blur.std`` and the positions of the step's random streams (latents / alpha /
dropout), so a resumed run continues the uninterrupted one.  With weight averaging on (``WGAN(generator_ema=...)``) the averaged
generator's two buffers, its update count and its schedule are saved too (``g_ema_*``); a checkpoint without them restores into
such a model with the averages reset to the restored live weights (and a warning), one with them into a model without the
feature, which ignores them.  With adaptive augmentation (``WGAN(augment=AdaptiveAugment(...))``) the controller's eight floats and
its configuration are saved as ``aug_state`` / ``aug_config``; a checkpoint with another ``aug_config`` is refused, one without the
keys restores into the initial state (and a warning).  A checkpoint restores only into a model whose optimizers have the
same class and static configuration (``ValueError`` otherwise); one written before optimizers were recorded (``m`` / ``v``
only) is a default Adam's.

Like ``tf.train.CheckpointManager`` the manager orders checkpoints by SAVE ORDER, not by the number in the file name
(``SaveModelCallback`` numbers files with a counter that restarts at every ``fit``, callbacks.py:245): the order lives in
a small ``checkpoint`` index file next to the ``.npz`` files, as TF keeps it."""
from __future__ import annotations

import json
import os
import re
import warnings

import numpy as np
import torch

from . import optimizers

INDEX = "checkpoint"

_LEGACY_OPT = ("Adam", optimizers.Adam().static_config())       # checkpoints without an optimizer record


def _json_default(x):
    return repr(x)


_CKPT_NAME = re.compile(r"^ckpt-\d+\.npz$")


def _eqlr_signature(model):
    """The fp32 coefficients of the model's EqualizedLearningRate layers, in layer order ([]: a plain model).  The wrapper adds no
    variable and changes no shape, so only this list tells a checkpoint of raw N(0, 1) kernels from one of plain weights."""
    return [float(np.float32(l.coefficient)) for l in model.net().eqlr_layers]


def _mapping_signature(model):
    """The configuration of the model's MappingNetwork prefix as a JSON string ("null": none): the layer count and width behind its
    variables, and the multiplier and switch that decide what its raw kernels mean."""
    mp = model.net().mapping
    return json.dumps(None if mp is None else dict(num_layers=mp.num_layers, units=model.net().style_dim, lr_multiplier=mp.lr_multiplier,
                                                    equalized_lr=mp.equalized_lr), sort_keys=True)


class CheckpointManager:
    def __init__(self, gan, directory, max_to_keep=5, keep_checkpoint_every_n_hours=None):
        self.gan, self.directory = gan, directory
        self.max_to_keep = None if not max_to_keep else int(max_to_keep)        # None / 0: keep everything

    # ---- save-order index
    def _index_path(self):
        return os.path.join(self.directory, INDEX)

    def _read_index(self):
        """File names in save order (oldest first).  A directory without an index (written by hand, or by the first
        version of this module) is ordered by modification time."""
        try:
            with open(self._index_path()) as f:
                names = [n for n in json.load(f)["all_model_checkpoint_paths"]]
        except (OSError, ValueError, KeyError):
            names = None
        if names is None:
            if not os.path.isdir(self.directory):
                return []
            names = [n for n in os.listdir(self.directory) if _CKPT_NAME.match(n)]      # never the ckpt-N.npz.tmp.npz of a crashed save
            names.sort(key=lambda n: os.path.getmtime(os.path.join(self.directory, n)))
        return [n for n in names if os.path.exists(os.path.join(self.directory, n))]

    def _write_index(self, names):
        tmp = self._index_path() + ".tmp"
        with open(tmp, "w") as f:
            json.dump({"model_checkpoint_path": names[-1] if names else None, "all_model_checkpoint_paths": names}, f)
        os.replace(tmp, self._index_path())

    @property
    def checkpoints(self):
        return [os.path.join(self.directory, n) for n in self._read_index()]

    @property
    def latest_checkpoint(self):
        ps = self.checkpoints
        return ps[-1] if ps else None

    # ---- save / restore
    def state_dict(self):
        g = self.gan
        d = {"n_img": np.int64(int(g.n_img)), "n_batches": np.int64(int(g.n_batches)),
             "rng_seed": np.int64(int(g._rng_seed)), "rng_off": np.int64(int(g._rng_off))}
        if hasattr(g, "blur"):
            d["std"] = np.float32(float(g.std))
        for tag, model in (("g", g.generator), ("d", g.discriminator)):
            st, opt = model.store, optimizers.get_optimizer(model)
            opt.attach(st)
            d[f"{tag}_theta"] = st.theta.cpu().numpy()
            d[f"{tag}_state"] = st.state.cpu().numpy()
            d[f"{tag}_m"] = st.m.cpu().numpy()
            d[f"{tag}_v"] = st.v.cpu().numpy()
            if st.s3 is not None:
                d[f"{tag}_s3"] = st.s3.cpu().numpy()
            d[f"{tag}_iterations"] = np.int64(opt.iterations)
            d[f"{tag}_opt_class"] = np.str_(type(opt).__name__)
            d[f"{tag}_opt_config"] = np.str_(json.dumps(opt.get_config(), default=_json_default))
            lr = opt.learning_rate
            d[f"{tag}_opt_lr"] = np.float64(lr if not callable(lr) else np.nan)      # a schedule lives in the config
            d[f"{tag}_rng_offset"] = np.int64(int(model.net().rng_offset))        # dropout-mask stream of this network
            d[f"{tag}_eqlr"] = np.asarray(_eqlr_signature(model), dtype=np.float32)
            d[f"{tag}_mapping"] = np.str_(_mapping_signature(model))
        if getattr(g, "generator_ema", None) is not None:
            st = g.generator_ema.store
            d["g_ema_theta"] = st.theta.cpu().numpy()
            d["g_ema_state"] = st.state.cpu().numpy()
            d["g_ema_updates"] = np.int64(g.generator_ema_updates)
            d["g_ema_config"] = np.str_(json.dumps(g.generator_ema_config.get_config()))
        if getattr(g, "_ada_state", None) is not None:
            d["aug_state"] = g._ada_state.cpu().numpy()
            d["aug_config"] = np.str_(json.dumps(g.augment.get_config(), sort_keys=True))
        return d

    def save(self, checkpoint_number=None):
        g = self.gan
        os.makedirs(self.directory, exist_ok=True)
        n = int(g.n_img) if checkpoint_number is None else int(checkpoint_number)
        name = f"ckpt-{n}.npz"
        path = os.path.join(self.directory, name)
        tmp = path + ".tmp.npz"
        for stale in os.listdir(self.directory):                     # temp files a crashed save left behind
            if stale.endswith(".tmp.npz") and stale.startswith("ckpt-"):
                try:
                    os.remove(os.path.join(self.directory, stale))
                except OSError:
                    pass
        np.savez(tmp, **self.state_dict())
        os.replace(tmp, path)                   # a crash mid-write never leaves a truncated "latest" checkpoint
        names = [x for x in self._read_index() if x != name] + [name]
        if self.max_to_keep is not None:
            for old in names[:-self.max_to_keep]:
                try:
                    os.remove(os.path.join(self.directory, old))
                except OSError:
                    pass
            names = names[-self.max_to_keep:]
        self._write_index(names)
        return path

    def restore(self, path):
        g = self.gan
        d = np.load(path)
        for tag, model in (("g", g.generator), ("d", g.discriminator)):        # before anything of either model is overwritten
            saved_eqlr = [float(c) for c in d[f"{tag}_eqlr"]] if f"{tag}_eqlr" in d.files else []      # older files: a plain model
            if saved_eqlr != _eqlr_signature(model):
                raise ValueError(f"{path}: the {'generator' if tag == 'g' else 'discriminator'} was saved with the equalised-learning-rate "
                                 f"coefficients {saved_eqlr}, the model's wrapped layers have {_eqlr_signature(model)}: the raw kernels of "
                                 "one are not the weights of the other (an empty list is a plain model)")
            saved_map = str(d[f"{tag}_mapping"]) if f"{tag}_mapping" in d.files else "null"      # older files: no mapping network
            if json.loads(saved_map) != json.loads(_mapping_signature(model)):
                raise ValueError(f"{path}: the {'generator' if tag == 'g' else 'discriminator'} was saved with the mapping network "
                                 f"{saved_map}, the model's is {_mapping_signature(model)}: layer count, width, lr_multiplier and "
                                 "equalized_lr must match (the raw kernels of one are not the weights of the other)")
        ada = getattr(g, "_ada_state", None) is not None
        if ada and "aug_config" in d.files and json.loads(str(d["aug_config"])) != g.augment.get_config():
            raise ValueError(f"{path}: saved with the adaptive augmentation {json.loads(str(d['aug_config']))}, the model's is "
                             f"{g.augment.get_config()}: the controller's state belongs to its configuration")
        g.n_img.assign(int(d["n_img"]))
        g.n_batches.assign(int(d["n_batches"]))
        if "rng_off" in d.files:
            g._rng_seed, g._rng_off = int(d["rng_seed"]), int(d["rng_off"])
        if "std" in d.files and hasattr(g, "blur"):
            g.std.assign(float(d["std"]))
        for tag, model in (("g", g.generator), ("d", g.discriminator)):
            st, opt = model.store, optimizers.get_optimizer(model)
            if f"{tag}_opt_class" in d.files:
                saved = (str(d[f"{tag}_opt_class"]), json.loads(str(d[f"{tag}_opt_config"])))
                saved_static = tuple(sorted((k, v) for k, v in saved[1].items() if k in dict(opt.static_config())))
            else:
                saved = saved_static = None
            if (saved[0] if saved else _LEGACY_OPT[0]) != type(opt).__name__ or \
                    (saved_static if saved else _LEGACY_OPT[1]) != opt.static_config():
                what = f"{saved[0]}({saved[1]})" if saved else "Adam() (a checkpoint without an optimizer record)"
                raise ValueError(f"{path}: the {'generator' if tag == 'g' else 'discriminator'} was saved with {what}, the model's "
                                 f"optimizer is {opt!r}: the class and static configuration must match")
            opt.attach(st)
            if st.s3 is not None and f"{tag}_s3" not in d.files:
                raise ValueError(f"{path}: no third slot saved for the {tag} optimizer {opt!r}")
            bufs = [("theta", st.theta), ("state", st.state), ("m", st.m), ("v", st.v)] + ([("s3", st.s3)] if st.s3 is not None else [])
            for name, buf in bufs:
                buf.copy_(torch.from_numpy(d[f"{tag}_{name}"]))
            opt.iterations = int(d[f"{tag}_iterations"])
            if f"{tag}_opt_lr" in d.files and not callable(opt.learning_rate) and np.isfinite(d[f"{tag}_opt_lr"]):
                opt.learning_rate = float(d[f"{tag}_opt_lr"])
            if f"{tag}_rng_offset" in d.files:
                model.net().rng_offset = int(d[f"{tag}_rng_offset"])
            st.tr_dirty = True
        if getattr(g, "generator_ema", None) is not None:
            if "g_ema_theta" in d.files:
                st = g.generator_ema.store
                st.theta.copy_(torch.from_numpy(d["g_ema_theta"]))
                st.state.copy_(torch.from_numpy(d["g_ema_state"]))
                st.tr_dirty = True
                g.generator_ema_updates = int(d["g_ema_updates"])
            else:
                g.reset_generator_ema()          # the live weights are in place
                if not getattr(g, "_warned_no_ema", False):          # once per model
                    g._warned_no_ema = True
                    warnings.warn(f"{path} holds no averaged generator: the averages start from the restored live weights, "
                                  "update count 0", RuntimeWarning, stacklevel=2)
        if ada:
            if "aug_state" in d.files:
                g._ada_state.copy_(torch.from_numpy(d["aug_state"]))
                g._sync_ada_metric_slots()
            else:
                g.set_augment_p(g.augment.p)          # the initial state
                if not getattr(g, "_warned_no_ada", False):          # once per model
                    g._warned_no_ada = True
                    warnings.warn(f"{path} holds no adaptive-augmentation state: p starts from the configured {g.augment.p}, the "
                                  "accumulator empty", RuntimeWarning, stacklevel=2)
        return path
