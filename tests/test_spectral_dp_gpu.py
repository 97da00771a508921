"""GPU check of spectrally normalised models under data parallelism, in the pattern of tests/test_layernorm_dp_gpu.py: 2 ranks sharing
the one GPU of the test box (gloo rendezvous, gradients staged through the host), buckets of a few bytes so every hand-over to the
reducer issues its all-reduce at once.  The gradient map dL/dW-bar -> dL/dW is linear and u, v, sigma are equal on all ranks, so it
is applied once, behind the reducer's finish(): every rank's gradients equal the single-process gradients at the global batch, and
the power iteration's state equals the single process's bit for bit (learning rates 0: the G-step's sigma is of the same weights)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
BUCKET_MB = "0.00001"        # 10 bytes: a bucket is full with its first slice
WORLD, LOCAL = 2, 3
# the reference alone at the global batch 6, both models normalised, seeds 1-5 (min |LeakyReLU pre-activation|, min x-hat gradient norm,
# min signal ratio): (2.2e-6, 0.25, 0.77), (2.7e-6, 0.23, 0.89), (1.1e-5, 0.2, 0.87), (4.2e-5, 0.29, 0.77), (8.8e-6, 0.26, 0.85)
SEED = 4


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
    import sn_reference as SR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)        # a rank's model is made with the global batch as its batch_size
        n = LOCAL * WORLD
        gan, reals, rnd = SR.make_gan("tiny", n, SEED, generator_sn=True, gbs=n)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    return gan, reals, rnd


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
    gan.train_on_batch(sh(reals), randomness=rnd_local)
    assert dist.GradReducer(gan.discriminator.store.grad, 1).bucket <= 4         # floats: the switch above is the one it reads
    for tag, store in (("d", gan.discriminator.store), ("g", gan.generator.store)):
        np.save(os.path.join(out_dir, f"{tag}_grad_{rank}.npy"), store.grad[:store.n_train].cpu().numpy())
        np.save(os.path.join(out_dir, f"{tag}_state_{rank}.npy"), store.state[:store.n_state].cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_match_single_process_global_batch(tmp_path):
    import sn_reference as SR
    from ln_reference import assert_close
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    gan, reals, rnd = _build()
    ref = SR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, gbs=LOCAL * WORLD)
    SR.check_conditions(ref)
    gan.train_on_batch(reals, randomness=rnd)
    for tag, model in (("d", gan.discriminator), ("g", gan.generator)):
        st = model.store
        single = st.grad[:st.n_train].cpu().numpy()
        g0, g1 = np.load(tmp_path / f"{tag}_grad_0.npy"), np.load(tmp_path / f"{tag}_grad_1.npy")
        np.testing.assert_array_equal(g0, g1)                               # all-reduced, then the same map on the same state
        # per tensor, the bound of the step tests: rtol 2e-3, atol 2e-4 * max|reference| of that tensor
        own = {id(l) for l in model._own_layers()}
        views = [(off, int(np.prod(shape))) for (l, n, off, shape, tr) in st.entries if tr and id(l) in own]
        assert_close([g0[o:o + k] for o, k in views], [single[o:o + k] for o, k in views], f"{tag} gradients, ranks against the single process")
        # and the single process itself against the float64 reference
        assert_close([single[o:o + k] for o, k in views], ref["dgrads" if tag == "d" else "ggrads"], f"{tag} gradients, single process against torch")
        # u, v and sigma of every wrapped layer: bit for bit the single process's (the generator's BatchNorm statistics, which
        # share the buffer, are sums over the ranks and agree to rounding only)
        s0, s1, ss = np.load(tmp_path / f"{tag}_state_0.npy"), np.load(tmp_path / f"{tag}_state_1.npy"), st.state[:st.n_state].cpu().numpy()
        for (l, n, off, shape, tr) in st.entries:
            if n in ("vector_u", "vector_v", "sigma"):
                k = int(np.prod(shape))
                np.testing.assert_array_equal(s0[off:off + k], ss[off:off + k], err_msg=n)
                np.testing.assert_array_equal(s1[off:off + k], ss[off:off + k], err_msg=n)
