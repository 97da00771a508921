"""GPU check of a non-default objective under data parallelism, in the pattern of tests/test_spectral_dp_gpu.py: 2 ranks sharing the
one GPU of the test box (gloo rendezvous, gradients staged through the host), the non-saturating loss with R1 at global batch 6.
The loss scale 1 / global batch, the vector-loss scale and the penalty's mean are global quantities: every rank's gradients equal
the float64 reference's at the global batch, within the bound of the step tests (tests/ln_reference.py)."""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
WORLD, LOCAL = 2, 3
CHILD_LIMIT = 120           # seconds: ONE limit shared by both children, which start together and run side by side; they take a few
# the reference alone at the global batch 6, tiny behind the blur (std 0.9), score scale 10, seeds 1-5 (min |LeakyReLU pre-activation|,
# min gradient norm at the reals): (2.0e-6, 0.48), (6.1e-7, 0.46), (1.1e-5, 0.66), (3.4e-5, 0.69), (4.6e-6, 0.55)
SEED = 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(device=None):
    """The case at the global batch: every rank and the single process build the same weights, images and randomness."""
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import blurred_gan_amd as bg
    import objective_reference as OR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)        # a rank's model is made with the global batch as its batch_size
        n = LOCAL * WORLD
        r1 = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals")
        gan, reals, rnd = OR.make_gan("tiny", n, SEED, r1, gbs=n, std=0.9, score_scale=10.0, device=device)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    return gan, reals, rnd


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    gan, reals, rnd = _build()
    sh = lambda a: dist.shard(torch.from_numpy(np.asarray(a))).numpy()
    rnd_local = {k: ([sh(m) for m in v] if isinstance(v, list) else sh(v)) for k, v in rnd.items()}
    gan.train_on_batch(sh(reals), randomness=rnd_local)
    for tag, store in (("d", gan.discriminator.store), ("g", gan.generator.store)):
        np.save(os.path.join(out_dir, f"{tag}_grad_{rank}.npy"), store.grad[:store.n_train].cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _run_children(out_dir):
    """Both ranks under ONE shared time limit (they start together and wait for each other in the collectives, so a limit per child
    would be the same deadline twice).  ``join`` raises as soon as a child has failed (after ending the other one); a child still
    running at the limit is ended, and the test fails there: nothing more is started."""
    ctx = mp.spawn(_worker, args=(WORLD, _free_port(), out_dir), nprocs=WORLD, join=False)
    deadline = time.monotonic() + CHILD_LIMIT
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            for p in ctx.processes:
                p.join()
            pytest.fail(f"the ranks did not finish within {CHILD_LIMIT} s")


def test_two_ranks_match_the_reference_at_the_global_batch(tmp_path):
    import objective_reference as OR
    from ln_reference import assert_close
    _run_children(str(tmp_path))
    gan, reals, rnd = _build()
    ref = OR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, LOCAL * WORLD, gan.objective)
    OR.check_conditions(ref)
    for tag, model in (("d", gan.discriminator), ("g", gan.generator)):
        st = model.store
        g0, g1 = np.load(tmp_path / f"{tag}_grad_0.npy"), np.load(tmp_path / f"{tag}_grad_1.npy")
        np.testing.assert_array_equal(g0, g1)
        own = {id(l) for l in model._own_layers()}
        views = [(off, int(np.prod(shape))) for (l, n, off, shape, tr) in st.entries if tr and id(l) in own]
        assert_close([g0[o:o + k] for o, k in views], ref["dgrads" if tag == "d" else "ggrads"], f"{tag} gradients, ranks against torch")
