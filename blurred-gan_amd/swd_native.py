"""Sliced Wasserstein distance on the device through the library's own kernels (include/bgan.h "SWD metric", csrc/swd.hip): the
functions of ``sliced_wasserstein.py`` -- pyramid, descriptors, finalize, distance -- over float32 device tensors, as launch
sequences.  ``torch`` allocates the buffers and makes views of them, nothing else: no torch arithmetic, indexing, ``cat``,
``sort``, ``pad`` or reduction runs here.  The random DRAWS (patch centres, directions) are made on the host from the caller's
``numpy.random.RandomState`` in the host path's order, so a seed gives the same patches and directions on every path.

The launches go on the stream of ``ops._stream()``, behind the training step that produced ``model.images``.  They must never be
recorded into a step program: every entry raises while ``program.active()`` is set."""
from __future__ import annotations

import numpy as np
import torch

from . import ops, program


def _guard():
    if program.active() is not None:
        raise RuntimeError("swd_native: the metric's launches must not be recorded into a step program; call it between steps")


def _check_dev(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise TypeError(f"{what}: the native SWD path takes float32 tensors on the GPU, got {type(x).__name__}"
                        + (" on the CPU" if isinstance(x, torch.Tensor) else ""))
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32, got {x.dtype}")


def _bytes(n, device):
    return torch.empty(max(int(n), 8), dtype=torch.uint8, device=device)


def ingest(images, data_format="NCHW", scale=1.0, shift=0.0):
    """A fresh [B,3,H,W] float32 buffer = images * scale + shift from an NCHW or NHWC batch of 1 or 3 channels (one channel is
    replicated three times, tf.image.grayscale_to_rgb).  ``model.images`` (NHWC, [-1, 1]) enter with scale = shift = 127.5."""
    _guard()
    _check_dev(images, "ingest")
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"data_format must be 'NCHW' or 'NHWC', got {data_format!r}")
    if images.dim() != 4:
        raise ValueError(f"expected a 4-d minibatch, got shape {tuple(images.shape)}")
    nhwc = data_format == "NHWC"
    B, H, W = (images.shape[0], images.shape[1], images.shape[2]) if nhwc else (images.shape[0], images.shape[2], images.shape[3])
    dst = torch.empty((B, 3, H, W), dtype=torch.float32, device=images.device)
    return ops.swd_ingest(images.detach(), dst, nhwc, scale, shift)


def pyr_down(minibatch):
    """Gaussian-pyramid step down (NCHW): the host ``pyr_down`` bit for bit."""
    _guard()
    _check_dev(minibatch, "pyr_down")
    n, c, h, w = minibatch.shape
    out = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=minibatch.device)
    return ops.pyr_down(minibatch, out)


def pyr_up(minibatch):
    """Gaussian-pyramid step up (NCHW): the host ``pyr_up`` bit for bit."""
    _guard()
    _check_dev(minibatch, "pyr_up")
    n, c, h, w = minibatch.shape
    out = torch.empty((n, c, 2 * h, 2 * w), dtype=torch.float32, device=minibatch.device)
    return ops.pyr_up(minibatch, out)


def generate_laplacian_pyramid(minibatch, num_levels, in_place=False):
    """[L0 .. L_{n-1}]: band-pass residuals, last level the low-pass image; one pyr_down and one fused ``level - pyr_up(low)``
    launch per level.  ``in_place``: the caller owns ``minibatch`` (an ``ingest`` result) and gives it up as level 0."""
    _guard()
    _check_dev(minibatch, "generate_laplacian_pyramid")
    if in_place:
        first = minibatch
    else:
        first = ops.copy_(torch.empty_like(minibatch, memory_format=torch.contiguous_format), minibatch)
    levels = [first]
    for _ in range(1, num_levels):
        low = pyr_down(levels[-1])
        ops.pyr_up(low, levels[-1], minuend=levels[-1])
        levels.append(low)
    return levels


def draw_centres(shape, nhood_size, nhoods_per_image, rng):
    """The host path's draws for one level (x first, then y), as int32 vectors."""
    n_img, chans, height, width = shape
    total = nhoods_per_image * n_img
    half = nhood_size // 2
    cx = rng.randint(half, width - half, size=(total, 1, 1, 1))
    cy = rng.randint(half, height - half, size=(total, 1, 1, 1))
    return np.ascontiguousarray(cx.reshape(-1), dtype=np.int32), np.ascontiguousarray(cy.reshape(-1), dtype=np.int32)


def gather_descriptors(level, cx, cy, nhood_size, nhoods_per_image):
    """[N, 3, n, n] patches of ``level`` around the given centres (host int32 vectors): 8 bytes uploaded per descriptor.  The
    kernel cannot check a centre, so their range is checked here, once, on the host."""
    _guard()
    _check_dev(level, "gather_descriptors")
    half = nhood_size // 2
    n_img, chans, height, width = level.shape
    cx, cy = np.ascontiguousarray(cx, dtype=np.int32).reshape(-1), np.ascontiguousarray(cy, dtype=np.int32).reshape(-1)
    total = n_img * nhoods_per_image
    if chans != 3 or cx.size != total or cy.size != total:
        raise ValueError(f"level {tuple(level.shape)} with {nhoods_per_image} patches per image needs {total} centres")
    if cx.min() < half or cx.max() >= width - half or cy.min() < half or cy.max() >= height - half:
        raise ValueError("patch centre outside the image")
    cx_d, cy_d = torch.from_numpy(cx).to(level.device), torch.from_numpy(cy).to(level.device)
    desc = torch.empty((total, 3, nhood_size, nhood_size), dtype=torch.float32, device=level.device)
    return ops.swd_gather(level, cx_d, cy_d, desc, nhood_size, nhoods_per_image)


def get_descriptors_for_minibatch(minibatch, nhood_size, nhoods_per_image, rng):
    """Random nhood_size x nhood_size x 3 patches, nhoods_per_image per image -> [N, 3, n, n] on the device."""
    assert minibatch.shape[1] == 3
    cx, cy = draw_centres(tuple(minibatch.shape), nhood_size, nhoods_per_image, rng)
    return gather_descriptors(minibatch, cx, cy, nhood_size, nhoods_per_image)


def finalize_descriptors(desc, stats=None):
    """Concatenate, standardise per channel (float64 statistics), flatten to [N, 3*n*n].  The inputs are left as they are;
    ``stats``: an optional float64 device tensor of 6 entries that receives mean and standard deviation per channel."""
    _guard()
    pieces = desc if isinstance(desc, list) else [desc]
    for p in pieces:
        _check_dev(p, "finalize_descriptors")
        assert p.dim() == 4 and p.shape[1] == 3 and p.shape[2] == p.shape[3] == pieces[0].shape[2]
    nhood = pieces[0].shape[2]
    rows = sum(p.shape[0] for p in pieces)
    out = torch.empty((rows, 3 * nhood * nhood), dtype=torch.float32, device=pieces[0].device)
    at = 0
    for p in pieces:
        ops.copy_(out.narrow(0, at, p.shape[0]), p)
        at += p.shape[0]
    ws = _bytes(ops.swd_standardize_workspace_bytes(rows, nhood), out.device)
    ops.swd_standardize(out, rows, nhood, ws, stats)
    return out


def draw_directions(dim, dir_repeats, dirs_per_repeat, rng):
    """The host path's unit directions, repeat by repeat, side by side: float32 [dim, dir_repeats * dirs_per_repeat]."""
    cols = []
    for _ in range(dir_repeats):
        dirs = rng.randn(dim, dirs_per_repeat)
        cols.append((dirs / np.sqrt((dirs ** 2).sum(axis=0, keepdims=True))).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def projected_distances(A, B, dirs, dir_repeats, out):
    """out[r] (float64 device view of dir_repeats entries) = mean |sort(A d) - sort(B d)| over the directions d of repeat r.
    One GEMM per set gives P[direction, descriptor], each direction a contiguous row for the sort."""
    _guard()
    assert A.dim() == 2 and A.shape == B.shape and dirs.shape[0] == A.shape[1] and dirs.shape[1] % dir_repeats == 0
    rows, dim = A.shape
    n_dirs = dirs.shape[1]
    d = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32)).to(A.device)
    proj = []
    for X in (A, B):
        P = torch.empty((n_dirs, rows), dtype=torch.float32, device=A.device)
        ops.gemm(d, X, P, n_dirs, rows, dim, transA=True, transB=True)
        proj.append(ops.sort_rows(P, n_dirs, rows))
    seg = (n_dirs // dir_repeats) * rows
    ws = _bytes(ops.abs_diff_mean_workspace_bytes(seg, dir_repeats), A.device)
    return ops.abs_diff_mean(proj[0], proj[1], seg, dir_repeats, out, ws)


def level_distances(real, fake, dir_repeats, dirs_per_repeat, rng):
    """Per-level distances of finalized descriptor sets (lists of [N, D] tensors): the draws of every level and repeat in the host
    path's order, every launch queued, then ONE read-back of levels x repeats doubles."""
    _guard()
    assert len(real) == len(fake) and len(real) >= 1
    out = torch.empty(len(real) * dir_repeats, dtype=torch.float64, device=real[0].device)
    for lod, (a, b) in enumerate(zip(real, fake)):
        dirs = draw_directions(a.shape[1], dir_repeats, dirs_per_repeat, rng)
        projected_distances(a, b, dirs, dir_repeats, out.narrow(0, lod * dir_repeats, dir_repeats))
    per_repeat = out.cpu().numpy().reshape(len(real), dir_repeats)
    return [float(np.mean(r)) for r in per_repeat]


def sliced_wasserstein(A, B, dir_repeats, dirs_per_repeat, rng):
    """Mean |sorted projection difference| over random unit directions."""
    return level_distances([A], [B], dir_repeats, dirs_per_repeat, rng)[0]
