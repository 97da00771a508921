"""GPU check of a critic with the MinibatchStdDev layer under data parallelism, after tests/test_layernorm_dp_gpu.py: 2 ranks
sharing the one GPU of the test box (gloo rendezvous, gradients staged through the host), B_local = 4, G = 2.

Groups are local to a rank.  Shards are contiguous and B_local % G == 0, so the groups of the two ranks are exactly the groups of
the single process at the global batch B = 8: the SUM of the ranks' critic gradients equals the single-process gradients.  As in
that file the ranks run with BGAN_DP_BUCKET_MB set to a few bytes, so that every hand-over to the reducer issues its all-reduce at
once: a slice that the penalty's source backward still writes into would go out without its last contribution."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
BUCKET_MB = "0.00001"        # 10 bytes: a bucket is full with its first slice
LOCAL, WORLD, G, SEED, STD = 4, 2, 2, 2, 0.9


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
    from blurred_gan_amd import models
    import objective_reference as OR
    n = LOCAL * WORLD
    with warnings.catch_warnings():
        # a rank's model is made with the global batch as its batch_size, which the constructor remarks on; the step takes the
        # batch from the images it is given
        warnings.simplefilter("ignore", UserWarning)
        return OR.make_gan("tiny", n, SEED, gbs=n, std=STD, disc=lambda: models.DCGANDiscriminator(arch="tiny", minibatch_stddev=G))


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      BGAN_DP_BUCKET_MB=BUCKET_MB)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    gan, reals, rnd = _build()
    sh = lambda a: dist.shard(torch.from_numpy(np.asarray(a))).numpy()
    rnd_local = {k: ([sh(m) for m in v] if isinstance(v, list) else sh(v)) for k, v in rnd.items()}
    local = sh(reals)
    assert local.shape[0] == LOCAL and np.array_equal(local, reals[rank * LOCAL:(rank + 1) * LOCAL])       # contiguous shards
    gan.train_on_batch(local, randomness=rnd_local)
    assert dist.GradReducer(gan.discriminator.store.grad, 1).bucket <= 4         # floats: the switch above is the one it reads
    for tag, store in (("d", gan.discriminator.store), ("g", gan.generator.store)):
        np.save(os.path.join(out_dir, f"{tag}_grad_{rank}.npy"), store.grad[:store.n_train].cpu().numpy())
        np.save(os.path.join(out_dir, f"{tag}_theta_{rank}.npy"), store.theta[:store.n_train].cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_match_single_process_global_batch(tmp_path):
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    gan, reals, rnd = _build()
    net = gan.discriminator.net()
    assert reals.shape[0] == LOCAL * WORLD and net.mbstd_layers[0].group_size == G and net.blur is not None
    gan.train_on_batch(reals, randomness=rnd)
    st = gan.discriminator.store
    ref_g, ref_t = st.grad[:st.n_train].cpu().numpy(), st.theta[:st.n_train].cpu().numpy()
    g0, g1 = np.load(tmp_path / "d_grad_0.npy"), np.load(tmp_path / "d_grad_1.npy")
    np.testing.assert_array_equal(g0, g1)                                   # all-reduced: identical on both ranks
    print("critic gradients: max|err|", float(np.abs(g0 - ref_g).max()), "max|ref|", float(np.abs(ref_g).max()))
    np.testing.assert_allclose(g0, ref_g, rtol=2e-3, atol=2e-4 * np.abs(ref_g).max())
    t0, t1 = np.load(tmp_path / "d_theta_0.npy"), np.load(tmp_path / "d_theta_1.npy")
    np.testing.assert_array_equal(t0, t1)                                   # replicas stay in lock step
    np.testing.assert_allclose(t0, ref_t, rtol=1e-3, atol=2e-4)
    np.testing.assert_array_equal(np.load(tmp_path / "g_grad_0.npy"), np.load(tmp_path / "g_grad_1.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "g_theta_0.npy"), np.load(tmp_path / "g_theta_1.npy"))
