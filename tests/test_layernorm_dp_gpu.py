"""GPU check of critics with LayerNormalization stages under data parallelism, in the pattern of tests/test_dp_gpu.py's
test_two_ranks_match_single_process_global_batch: 2 ranks sharing the one GPU of the test box (gloo rendezvous, gradients staged
through the host).  The penalty's source backward hands each layer's slice of the flat gradient buffer to the reducer behind the
last launch that writes into it; a slice that went out earlier would be all-reduced without its last contribution, and the SUM of
the ranks' critic gradients would differ from the single-process gradients at the global batch.

dist.GradReducer merges slices into buckets of 16 MB and these critics hold a few thousand floats, so at the default every slice
would wait for finish() and the order of the hand-overs could not show.  The ranks therefore run with BGAN_DP_BUCKET_MB set to a
few bytes: every ready() issues its all-reduce at once, from what the stream has computed up to there."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
BUCKET_MB = "0.00001"        # 10 bytes: a bucket is full with its first slice


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(name):
    """The case at the global batch (tests/ln_critics.py dp_case): every rank and the single process build the same weights,
    images and randomness from the same seed."""
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ln_critics as LC
    with warnings.catch_warnings():
        # a rank's model is made with the global batch as its batch_size, which the constructor remarks on; the step takes the
        # batch from the images it is given
        warnings.simplefilter("ignore", UserWarning)
        return LC.dp_case(name)


def _worker(rank, world, port, out_dir, name):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      BGAN_DP_BUCKET_MB=BUCKET_MB)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    gan, reals, rnd = _build(name)
    sh = lambda a: dist.shard(torch.from_numpy(np.asarray(a))).numpy()
    rnd_local = {k: ([sh(m) for m in v] if isinstance(v, list) else sh(v)) for k, v in rnd.items()}
    gan.train_on_batch(sh(reals), randomness=rnd_local)
    assert dist.GradReducer(gan.discriminator.store.grad, 1).bucket <= 4         # floats: the switch above is the one it reads
    for tag, store in (("d", gan.discriminator.store), ("g", gan.generator.store)):
        np.save(os.path.join(out_dir, f"{tag}_grad_{rank}.npy"), store.grad[:store.n_train].cpu().numpy())
        np.save(os.path.join(out_dir, f"{tag}_theta_{rank}.npy"), store.theta[:store.n_train].cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("name", ["stock", "ln_plain_ln"])
def test_two_ranks_match_single_process_global_batch(tmp_path, name):
    import ln_critics as LC
    world = LC.DP_WORLD
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), name), nprocs=world, join=True)
    gan, reals, rnd = _build(name)
    assert reals.shape[0] == LC.DP_LOCAL * world and gan.discriminator.net().has_ln
    assert (gan.discriminator.net().blur is not None) == (LC.DP_CASES[name][0] is not None)
    if name != "stock":
        LC.assert_claims(name, gan.discriminator.net())
    gan.train_on_batch(reals, randomness=rnd)
    st = gan.discriminator.store
    ref_g, ref_t = st.grad[:st.n_train].cpu().numpy(), st.theta[:st.n_train].cpu().numpy()
    g0, g1 = np.load(tmp_path / "d_grad_0.npy"), np.load(tmp_path / "d_grad_1.npy")
    np.testing.assert_array_equal(g0, g1)                                   # all-reduced: identical on both ranks
    print(name, "critic gradients: max|err|", float(np.abs(g0 - ref_g).max()), "max|ref|", float(np.abs(ref_g).max()))
    np.testing.assert_allclose(g0, ref_g, rtol=2e-3, atol=2e-4 * np.abs(ref_g).max())
    t0, t1 = np.load(tmp_path / "d_theta_0.npy"), np.load(tmp_path / "d_theta_1.npy")
    np.testing.assert_array_equal(t0, t1)                                   # replicas stay in lock step
    np.testing.assert_allclose(t0, ref_t, rtol=1e-3, atol=2e-4)
    np.testing.assert_array_equal(np.load(tmp_path / "g_grad_0.npy"), np.load(tmp_path / "g_grad_1.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "g_theta_0.npy"), np.load(tmp_path / "g_theta_1.npy"))
