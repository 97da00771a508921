"""Device-resident uint8 dataset: the reference's ``tfds.load(...).map(normalise/resize).shuffle(...).batch(...)`` input chain
(demo_celeba.py:15-48, demo_mnist.py:17-45) with the whole dataset in HBM.  CelebA is 23.6 GB as uint8 at 218x178 and the card has
288 GB, so the images go up ONCE; after that a batch is a list of indices, and one HIP launch (include/bgan.h
``bg_u8_gather_normalize_resize_f32``: gather -> (x - 127.5) / 127.5 -> bilinear resize -> optional mirror) turns it into the
step's float32 input.  No host work and no PCIe traffic per batch.

``EpochPlan`` is the host side (which sample goes to which rank, in which order, in which batch); ``DeviceDataset`` owns the
device memory and the launches."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import dist, ops

MAX_FRACTION_OF_FREE = 0.9       # default max_bytes: this share of the free device memory at construction


class EpochPlan:
    """One rank's share of one epoch -- pure host code.

    ``np.random.default_rng([seed, epoch]).permutation(N)`` is the epoch's order, identical on every rank (``shuffle=False``: the
    identity).  Rank ``r`` takes the contiguous slice ``[r * per, (r + 1) * per)`` of it, ``per = N // world_size``: the shards are
    disjoint and equal, the ``N % world_size`` samples at the end of the epoch's order are dropped (other ones every epoch).
    ``indices`` (int32 [per]) is that slice and ``bounds`` the ``(start, stop)`` of every batch in it; without ``drop_remainder``
    the last batch is short when ``per % batch_size != 0``."""

    def __init__(self, N, batch_size, shuffle=True, seed=0, epoch=0, rank=0, world_size=1, drop_remainder=False):
        N, batch_size, rank, world_size = int(N), int(batch_size), int(rank), int(world_size)
        if N <= 0 or batch_size <= 0:
            raise ValueError(f"EpochPlan: N={N} and batch_size={batch_size} must be positive")
        if N >= 2 ** 31:
            raise ValueError(f"EpochPlan: N={N} does not fit the int32 indices of the gather kernel")
        if world_size <= 0 or not 0 <= rank < world_size:
            raise ValueError(f"EpochPlan: rank {rank} outside [0, {world_size})")
        per = N // world_size
        if per == 0:
            raise ValueError(f"EpochPlan: {N} samples cannot be split over {world_size} ranks")
        order = np.random.default_rng([int(seed), int(epoch)]).permutation(N) if shuffle else np.arange(N)
        self.N, self.batch_size, self.epoch, self.rank, self.world_size = N, batch_size, int(epoch), rank, world_size
        self.indices = np.ascontiguousarray(order[rank * per:(rank + 1) * per], dtype=np.int32)
        stop = per - per % batch_size if drop_remainder else per
        self.bounds = [(s, min(s + batch_size, stop)) for s in range(0, stop, batch_size)]

    @property
    def batch_sizes(self):
        return [e - s for s, e in self.bounds]

    def __len__(self):
        return len(self.bounds)


def _open_images(images):
    """The dataset as something sliceable by image, [N,H,W,C] uint8, without reading a file into host memory."""
    if isinstance(images, (str, os.PathLike)):
        images = np.load(images, mmap_mode="r")
    if isinstance(images, torch.Tensor):
        if not images.is_cuda:
            raise ops.BgDeviceError("DeviceDataset: a tensor must already live on the GPU (pass host data as a numpy array, a "
                                    "memmap or a .npy path); there is no host-side fallback")
    elif not isinstance(images, np.ndarray):
        raise TypeError(f"DeviceDataset: images must be a uint8 numpy array / memmap, a .npy path or a device tensor, got {type(images)}")
    if images.dtype != (torch.uint8 if isinstance(images, torch.Tensor) else np.uint8):
        raise ValueError(f"DeviceDataset: images must be uint8, got {images.dtype}")
    if images.ndim == 3:
        images = images.reshape(*images.shape, 1)          # a view, for a memmap too
    if images.ndim != 4 or min(images.shape) <= 0:
        raise ValueError(f"DeviceDataset: images must be [N,H,W,C] or [N,H,W], got shape {tuple(images.shape)}")
    return images


class DeviceDataset:
    """Iterable of float32 NHWC batches in [-1, 1] out of a uint8 dataset that lives on the card.

    ``images``: uint8 ``[N,H,W,C]`` / ``[N,H,W]`` numpy array or memmap, a path to such a ``.npy`` (opened as a memmap), or a uint8
    tensor already on the GPU (used in place).  Host data is uploaded once, ``chunk_bytes`` (whole images) at a time through one
    pinned staging buffer, so a 24 GB file is never materialised in host memory.  The upload may take at most ``max_bytes`` of
    device memory -- default ``MAX_FRACTION_OF_FREE`` (0.9) of what ``torch.cuda.mem_get_info()`` reports free -- and raises
    ``ValueError`` naming both figures otherwise; nothing falls back to the host.  A CPU tensor or a machine without a GPU raises
    ``ops.BgDeviceError``.

    ``image_size``: ``(H, W)`` or one int, the size batches are resized to (TF bilinear, half-pixel centres, normalise first);
    None keeps the stored size.  ``rank`` / ``world_size`` default to ``dist.rank()`` / ``dist.world_size()``; see ``EpochPlan``
    for the sharding.  ``len(ds)`` is the number of batches per epoch, ``ds.samples_per_epoch`` the samples they hold.

    Every ``iter(ds)`` starts a new epoch: it takes the plan of ``ds.epoch`` and then increments ``ds.epoch`` (a plain attribute: a
    resumed run sets it) -- tf.data's ``shuffle(buffer_size=N, reshuffle_each_iteration=True)``.  Per epoch the rank's int32 index
    sequence is uploaded once; with ``flip=True`` one uint8 flag per position of that sequence is drawn on the device by
    ``ops.keep_mask(flags, 0.5, seed=ds.flip_seed, offset=ds.flip_offset(epoch))``, ``flip_seed = seed + 7919 * rank`` and
    ``flip_offset(epoch) = epoch * ceil(samples_of_the_rank / 4)`` (the Philox blocks one epoch consumes): epochs differ, a re-run
    repeats.  A sample is mirrored left-right where its flag is non-zero.  Per batch there is EXACTLY ONE launch, on the current
    stream, whose index / flag arguments are offsets into those per-epoch arrays.

    Ring contract: batches are written into ``buffers`` persistent float32 tensors allocated at construction, used in turn across
    epochs; a short last batch is a leading view of the same storage.  The tensor yielded as batch k is left untouched until batch
    k + ``buffers`` is requested from the iterator -- ``WGAN.images`` keeps a reference to the step's reals for the callbacks, so
    consume a batch (or clone it) before asking for ``buffers`` more.  The addresses never change, so the batches suit
    ``WGAN(persistent_input=True)`` (step programs are then recorded per ring buffer and batch shape, no staging copy) as well as
    the default ``persistent_input=False``."""

    def __init__(self, images, image_size=None, batch_size=32, shuffle=True, seed=0, flip=False, drop_remainder=False, rank=None,
                 world_size=None, buffers=2, chunk_bytes=64 << 20, max_bytes=None):
        images = _open_images(images)
        if not torch.cuda.is_available():
            raise ops.BgDeviceError("DeviceDataset needs a GPU: the dataset lives in device memory and there is no host-side fallback")
        if int(buffers) < 1 or int(batch_size) < 1 or int(chunk_bytes) < 1:
            raise ValueError(f"DeviceDataset: buffers={buffers}, batch_size={batch_size}, chunk_bytes={chunk_bytes} must be positive")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.N, self.H, self.W, self.C = (int(s) for s in images.shape)
        if image_size is None:
            image_size = (self.H, self.W)
        elif isinstance(image_size, int):
            image_size = (image_size, image_size)
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.batch_size, self.shuffle, self.seed, self.flip, self.drop_remainder = int(batch_size), bool(shuffle), int(seed), bool(flip), bool(drop_remainder)
        self.rank = dist.rank() if rank is None else int(rank)
        self.world_size = dist.world_size() if world_size is None else int(world_size)
        self.epoch = 0
        plan = self.plan(0)                      # validates N / batch / rank / world_size before anything is allocated
        self._per = len(plan.indices)
        self.samples_per_epoch = sum(plan.batch_sizes)
        self._n_batches = len(plan)
        self.flip_seed = self.seed + 7919 * self.rank
        self.data = images if isinstance(images, torch.Tensor) else self._upload(images, int(chunk_bytes), max_bytes)
        if not self.data.is_contiguous():
            raise ValueError("DeviceDataset: a device tensor must be contiguous")
        self._ring = [torch.empty(self.batch_size, *self.image_size, self.C, dtype=torch.float32, device=self.device)
                      for _ in range(int(buffers))]
        self._produced = 0                       # batches handed out so far, over all epochs: batch k lives in ring slot k % buffers

    # ------------------------------------------------------------------ upload
    def _upload(self, images, chunk_bytes, max_bytes):
        need = self.N * self.H * self.W * self.C
        free = torch.cuda.mem_get_info(self.device)[0]
        limit = int(MAX_FRACTION_OF_FREE * free) if max_bytes is None else int(max_bytes)
        if need > limit:
            raise ValueError(f"DeviceDataset: the dataset needs {need} bytes of device memory but at most {limit} may be used "
                             f"({free} bytes are free); datasets larger than device memory are not supported")
        data = torch.empty((self.N, self.H, self.W, self.C), dtype=torch.uint8, device=self.device)
        per_chunk = max(1, chunk_bytes // (self.H * self.W * self.C))
        stage = torch.empty((min(per_chunk, self.N), self.H, self.W, self.C), dtype=torch.uint8).pin_memory()
        stage_np = stage.numpy()
        stream = torch.cuda.current_stream()
        for i in range(0, self.N, per_chunk):
            n = min(per_chunk, self.N - i)
            np.copyto(stage_np[:n], images[i:i + n])
            data[i:i + n].copy_(stage[:n], non_blocking=True)
            stream.synchronize()                 # ONE staging buffer: it is refilled only after its copy has left
        return data

    # ------------------------------------------------------------------ epochs
    def plan(self, epoch):
        return EpochPlan(self.N, self.batch_size, self.shuffle, self.seed, epoch, self.rank, self.world_size, self.drop_remainder)

    def flip_offset(self, epoch):
        return int(epoch) * ((self._per + 3) // 4)

    def __len__(self):
        return self._n_batches

    def __iter__(self):
        epoch = int(self.epoch)
        self.epoch = epoch + 1
        plan = self.plan(epoch)
        idx_d = torch.from_numpy(plan.indices).to(self.device)
        flip_d = None
        if self.flip:
            flip_d = ops.keep_mask(torch.empty(self._per, dtype=torch.uint8, device=self.device), 0.5, self.flip_seed, self.flip_offset(epoch))
        return self._batches(plan, idx_d, flip_d)

    def _batches(self, plan, idx_d, flip_d):
        for s, e in plan.bounds:
            out = self._ring[self._produced % len(self._ring)][:e - s]
            self._produced += 1
            ops.u8_gather_normalize_resize(self.data, idx_d[s:e], out, None if flip_d is None else flip_d[s:e])
            yield out
