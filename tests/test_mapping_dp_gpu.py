"""GPU check of a generator with a MappingNetwork prefix under data parallelism, after tests/test_modconv_dp_gpu.py: 2 ranks sharing
the one GPU of the test box (gloo rendezvous, gradients staged through the host), B_local = 4.

The prefix's gradients, dL/dw included, are sums over the rank's own samples; the flat gradient all-reduce adds the ranks' sums, so
the gradients and the updated theta equal those of a single process on the global batch B = 8.  The one new exchange is the batch
mean of w behind the G-step's forward ([units] floats, each rank's column sums scaled by 1 / global batch): w_avg is the same on
both ranks, bit for bit, and equals the single process's within float32 summation order."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
LOCAL, WORLD, SEED, STD, UNITS = 4, 2, 2, 0.9, 7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build():
    """The case at the global batch: every rank and the single process build the same weights, images and randomness."""
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mapping_reference as R
    n = LOCAL * WORLD
    with warnings.catch_warnings():
        # a rank's model is made with the global batch as its batch_size, which the constructor remarks on; the step takes the
        # batch from the images it is given
        warnings.simplefilter("ignore", UserWarning)
        return R.make_gan("tiny", n, SEED, dict(noise=True, equalized_lr=True, mapping_layers=2, mapping_units=UNITS), gbs=n, std=STD)


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    gan, reals, rnd = _build()
    sh = lambda a: dist.shard(torch.from_numpy(np.asarray(a))).numpy()
    rnd_local = {k: ([sh(m) for m in v] if isinstance(v, list) else sh(v)) for k, v in rnd.items()}
    local = sh(reals)
    assert local.shape[0] == LOCAL and np.array_equal(local, reals[rank * LOCAL:(rank + 1) * LOCAL])       # contiguous shards
    calls = []
    for name in ("all_reduce_sum_", "all_reduce_sum_async"):       # the two entry points of the engine's SyncBN exchanges
        real = getattr(dist, name)
        setattr(dist, name, lambda t, *a, _real=real, **k: (calls.append(int(t.numel())), _real(t, *a, **k))[1])
    gan.train_on_batch(local, randomness=rnd_local)
    assert calls == [UNITS], f"the one exchange besides the gradients is the batch mean of w, saw all-reduces of {calls} floats"
    np.save(os.path.join(out_dir, f"w_avg_{rank}.npy"), gan.w_avg)
    for tag, store in (("d", gan.discriminator.store), ("g", gan.generator.store)):
        np.save(os.path.join(out_dir, f"{tag}_grad_{rank}.npy"), store.grad[:store.n_train].cpu().numpy())
        np.save(os.path.join(out_dir, f"{tag}_theta_{rank}.npy"), store.theta[:store.n_train].cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_match_single_process_global_batch(tmp_path):
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    gan, reals, rnd = _build()
    net = gan.generator.net()
    assert reals.shape[0] == LOCAL * WORLD and net.has_mapping and net.has_mod and net.has_noise and all(st.bn is None for st in net.stages)
    gan.train_on_batch(reals, randomness=rnd)
    store = gan.generator.store
    at = [(off, int(np.prod(shape))) for (l, n, off, shape, tr) in store.entries if l is net.mapping and tr]
    assert len(at) == 4
    g0 = np.load(tmp_path / "g_grad_0.npy")
    w0, w1 = np.load(tmp_path / "w_avg_0.npy"), np.load(tmp_path / "w_avg_1.npy")
    assert np.array_equal(w0.view(np.uint32), w1.view(np.uint32)) and np.abs(w0).max() > 0          # the same bits on both ranks
    np.testing.assert_allclose(w0, gan.w_avg, rtol=1e-5, atol=1e-7)            # the mean over the global batch, another summation order
    for off, n in at:          # the prefix's gradients on their own
        ref = store.grad[off:off + n].cpu().numpy()
        print("mapping gradient: max |two ranks|", float(np.abs(g0[off:off + n]).max()), "single process", float(np.abs(ref).max()))
        assert np.abs(ref).max() > 1e-6
        np.testing.assert_allclose(g0[off:off + n], ref, rtol=2e-3, atol=2e-4 * np.abs(ref).max())
    for tag, st in (("g", gan.generator.store), ("d", gan.discriminator.store)):
        ref_g, ref_t = st.grad[:st.n_train].cpu().numpy(), st.theta[:st.n_train].cpu().numpy()
        g0, g1 = np.load(tmp_path / f"{tag}_grad_0.npy"), np.load(tmp_path / f"{tag}_grad_1.npy")
        np.testing.assert_array_equal(g0, g1)                                   # all-reduced: identical on both ranks
        print(tag, "gradients: max|err|", float(np.abs(g0 - ref_g).max()), "max|ref|", float(np.abs(ref_g).max()))
        np.testing.assert_allclose(g0, ref_g, rtol=2e-3, atol=2e-4 * np.abs(ref_g).max())
        t0, t1 = np.load(tmp_path / f"{tag}_theta_0.npy"), np.load(tmp_path / f"{tag}_theta_1.npy")
        np.testing.assert_array_equal(t0, t1)                                   # replicas stay in lock step
        np.testing.assert_allclose(t0, ref_t, rtol=1e-3, atol=2e-4)
