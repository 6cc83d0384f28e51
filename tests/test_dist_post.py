"""Pooling PosteriorSums over ranks with dist.reduce_summary, world_size 2 over gloo (CPU):
each rank holds the sums of its own chains; the reduced pooled vector gives every rank the
means over all chains of all ranks."""
import os

import numpy as np
import torch.multiprocessing as mp

from gibbs_student_t_amd import dist
from gibbs_student_t_amd.post import PosteriorSums
from support import free_port

C, S, N, M = 3, 40, 6, 4


def _rank_chains(rank):
    rng = np.random.default_rng([8, rank])
    p = np.array([0.05, 0.97, 0.5, 0.93, 0.0, 1.0])
    return (rng.uniform(size=(C, S, N)) < p).astype(float), rng.normal(size=(C, S, M))


def _rank_sums(rank):
    z, b = _rank_chains(rank)
    # the ranks need not have counted the same number of sweeps
    lo = 10 * rank
    return PosteriorSums(np.full(C, S - lo), z_sum=z[:, lo:].sum(axis=1),
                         b_sum=b[:, lo:].sum(axis=1), b_sq=(b[:, lo:] ** 2).sum(axis=1))


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init("gloo")
    mine = _rank_sums(rank)
    vec, _ = dist.reduce_summary(mine.pooled_vector(), np.zeros(1))
    allp = mine.from_pooled_vector(vec)
    out.put((rank, int(allp.count[0]), allp.z_mean().tolist(), allp.b_mean().tolist(),
             allp.b_var().tolist(), allp.outliers().tolist()))
    dist.finalize()


def test_two_rank_posterior_pooling():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1:] == res[1][1:]                    # every rank has the same pooled result
    zs, bs = [], []
    for r in range(2):
        z, b = _rank_chains(r)
        zs.append(z[:, 10 * r:].reshape(-1, N))
        bs.append(b[:, 10 * r:].reshape(-1, M))
    z, b = np.concatenate(zs), np.concatenate(bs)
    _, count, z_mean, b_mean, b_var, outl = res[0]
    assert count == C * S + C * (S - 10)
    np.testing.assert_allclose(z_mean, z.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(b_mean, b.mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(b_var, b.var(axis=0), rtol=1e-10)
    assert outl == np.flatnonzero(z.mean(axis=0) > 0.9).tolist()


def test_single_process_pooling_is_identity():
    mine = _rank_sums(0)
    vec, _ = dist.reduce_summary(mine.pooled_vector(), np.zeros(1))
    np.testing.assert_array_equal(mine.from_pooled_vector(vec).z_mean(), mine.z_mean())
