"""GPU check of adaptive augmentation under data parallelism, in the pattern of tests/test_objective_dp_gpu.py: 2 ranks sharing the one
GPU of the test box (gloo rendezvous, collectives staged through the host).  The controller's 4-float statistics are sum-all-reduced
before the update, so the count is the global batch and every rank holds the same p: after ``interval`` steps both ranks' controller
states are identical bit for bit, and equal to the single process's on the concatenated batch with the same injected randomness.

The single process and the ranks compute the same real scores up to fp32 rounding (other batch sizes take other kernel routes), so the
case asserts first -- on the float64 reference of tests/ada_reference.py alone -- that no real score lies within 1e-2 of the scores'
scale of zero (what the reference alone gave for other seeds stands beside SEED): the signs are then the same everywhere."""
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
INTERVAL, SPEED = 2, 64     # an adjustment is 2 * 6 / 64: exact
CHILD_LIMIT = 120           # seconds: ONE limit shared by both children, which start together and run side by side; they take a few
# smallest |real score| / scale of either step, seeds 1-5 (see the module text): 2: (0.31, 0.079), 3: (0.25, 0.17), 4: (0.069, 0.14), 5: (0.19, 0.043)
SEED = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build():
    """The case at the global batch: every rank and the single process build the same weights, images and per-step randomness."""
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import blurred_gan_amd as bg
    import ada_reference as AR
    import diffaug_reference as DR
    import ln_reference as LN
    n = LOCAL * WORLD
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)        # a rank's model is made with the global batch as its batch_size
        r1 = bg.Objective("nonsaturating", penalty_target=0.0, penalty_on="reals")
        cfg = bg.AdaptiveAugment(p=0.5, target=0.0, interval=INTERVAL, speed_images=SPEED)
        gan, reals, _ = AR.make_gan("tiny", n, SEED, cfg, objective=r1, gbs=n, std=0.9, score_scale=10.0)
    gan.discriminator.optimizer.learning_rate = 0.0
    gan.generator.optimizer.learning_rate = 0.0
    steps = []
    for i in range(INTERVAL):
        seed = SEED + 100 * i
        rnd = AR.add_gates(DR.draw_aug(LN.draw(gan.discriminator, n, gan.generator.latent_size, np.random.default_rng(seed)), n, seed), n, seed)
        steps.append((np.roll(reals, i, axis=0), rnd))
    return gan, steps


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from blurred_gan_amd import dist
    torch.cuda.set_device(0)
    torch.distributed.init_process_group(backend="gloo")
    gan, steps = _build()
    sh = lambda a: dist.shard(torch.from_numpy(np.asarray(a))).numpy()
    for reals, rnd in steps:
        rnd_local = {k: ([sh(m) for m in v] if isinstance(v, list) else sh(v)) for k, v in rnd.items()}
        gan.train_on_batch(sh(reals), randomness=rnd_local)
    np.save(os.path.join(out_dir, f"ada_state_{rank}.npy"), gan._ada_state.cpu().numpy())
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _run_children(out_dir):
    """Both ranks under ONE shared time limit; a child still running at the limit is ended, and the test fails there."""
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


def test_both_ranks_hold_the_single_process_p(tmp_path):
    _run_children(str(tmp_path))
    s0, s1 = np.load(tmp_path / "ada_state_0.npy"), np.load(tmp_path / "ada_state_1.npy")
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), (s0, s1)
    import ada_reference as AR
    gan, steps = _build()
    n = LOCAL * WORLD
    rule = AR.Controller(0.5, 0.0, INTERVAL, SPEED)
    for reals, rnd in steps:
        rs = AR.ref_step_grads(gan.generator, gan.discriminator, reals, rnd, n, gan.objective, gan.augment, float(rule.p))["rs"]
        print("[ada dp] reference real scores:", rs)
        assert np.abs(rs).min() > 1e-2 * max(1.0, float(np.abs(rs).max())), rs          # no sign hangs on a rounding
        rule.step(rs.astype(np.float32))
        gan.train_on_batch(reals, randomness=rnd)
    single = gan._ada_state.cpu().numpy()
    print("[ada dp] states:", s0, single, rule.state())
    assert np.array_equal(s0.view(np.uint32), single.view(np.uint32)), (s0, single)
    assert np.array_equal(single.view(np.uint32), rule.state().view(np.uint32)), (single, rule.state())
    assert single[0] != 0.5 and single[2] == 0 and single[3] == 0                       # one adjustment, over the global count
    assert abs(float(single[0]) - 0.5) == INTERVAL * n / SPEED
