"""PosteriorSums' exceedance counts and residual sums (post.py; include/gst.h gst_accum_toa):
the notebook's median rule np.median(poutchain, axis=0) > tau decided exactly from counts --
with the one undecidable case reported, never guessed -- and the mean and spread of the
signal T b at every TOA from the sums of y = r - T b and y^2.  Host arithmetic only."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from gibbs_student_t_amd import dist
from gibbs_student_t_amd.post import PosteriorSums
from support import free_port

THR = (0.2, 0.5, 0.9)
N, M = 11, 4


def _pout(C, S, seed):
    """pout chains [C, S, N] with the notebook's look (mostly ~1 or ~0, a few in between);
    values exactly at a threshold are in, since the compare is strict"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(size=(C, S, N)) ** rng.choice([0.05, 1.0, 8.0], size=N)
    p[rng.uniform(size=p.shape) < 0.1] = 0.5
    return p


def _sums(p, b=None, T=None, r=None, thr=THR):
    C, S, _ = p.shape
    kw = dict(pout_sum=p.sum(axis=1), pout_thr=thr,
              pout_gt=np.stack([(p > t).sum(axis=1).astype(float) for t in thr]))
    if b is not None:
        y = r - b @ T.T                       # [C, S, n]
        kw.update(b_sum=b.sum(axis=1), b_sq=(b * b).sum(axis=1), resid_sum=y.sum(axis=1),
                  resid_sq=(y * y).sum(axis=1))
    return PosteriorSums(np.full(C, S), **kw)


def _tie_chain(S):
    """TOA 0 of one chain with exactly S/2 values above 0.5"""
    p = _pout(1, S, 77)
    p[0, :, 0] = np.where(np.arange(S) % 2 == 0, 0.8, 0.3)
    return p


@pytest.mark.parametrize("C,S", [(3, 31), (2, 40), (1, 7), (4, 6)])
def test_median_rule_equals_numpy(C, S):
    p = _pout(C, S, [C, S])
    if (C * S) % 2 == 0:
        p[:, :, 0] = np.where(np.arange(C * S).reshape(C, S) % 2 == 0, 0.8, 0.3)   # exact tie at 0.5
    post = _sums(p)
    flat = p.reshape(-1, N)
    Ntot = C * S
    for thr in THR:
        got, amb = post.pout_median_gt(thr)
        cnt = (flat > thr).sum(axis=0)
        np.testing.assert_array_equal(amb, 2 * cnt == Ntot)      # ambiguous is exactly count == N/2
        want = np.median(flat, axis=0) > thr
        np.testing.assert_array_equal(got[~amb], want[~amb])
        assert not got[amb].any()
        np.testing.assert_array_equal(post.pout_exceed_frac(thr), cnt / Ntot)
        np.testing.assert_array_equal(post.pout_exceed_frac(thr, pool=False),
                                      (p > thr).sum(axis=1) / S)
    if Ntot % 2:
        assert not any(post.pout_median_gt(t)[1].any() for t in THR)   # an odd total never ties
        for thr in THR:
            np.testing.assert_array_equal(post.outliers(thr, rule="median"),
                                          np.flatnonzero(np.median(flat, axis=0) > thr))
    else:
        assert post.pout_median_gt(0.5)[1][0]
        with pytest.raises(ValueError, match="undecided"):
            post.outliers(0.5, rule="median")


def test_constructed_tie_is_reported_not_guessed():
    post = _sums(_tie_chain(10))
    got, amb = post.pout_median_gt(0.5)
    assert amb[0] and not got[0]
    # the same TOA is decided at the other thresholds: 0.3 and 0.8 both above 0.2, both below 0.9
    assert post.pout_median_gt(0.2)[0][0] and not post.pout_median_gt(0.2)[1][0]
    assert not post.pout_median_gt(0.9)[0][0] and not post.pout_median_gt(0.9)[1][0]


def test_threshold_must_be_kept_and_rules():
    p = _pout(3, 31, 5)
    post = _sums(p)
    with pytest.raises(ValueError, match="not kept"):
        post.pout_median_gt(0.3)
    with pytest.raises(ValueError, match="rule"):
        post.outliers(0.5, rule="mode")
    with pytest.raises(ValueError, match="not accumulated"):
        PosteriorSums([4], pout_sum=np.zeros((1, N))).pout_median_gt(0.5)
    # the default rule is the mean of z, as before
    z = (np.random.default_rng(2).uniform(size=(3, 31, N)) < 0.6).astype(float)
    pz = PosteriorSums(np.full(3, 31), z_sum=z.sum(axis=1))
    np.testing.assert_array_equal(pz.outliers(0.5),
                                  np.flatnonzero(z.reshape(-1, N).mean(axis=0) > 0.5))
    np.testing.assert_array_equal(pz.outliers(0.5), pz.outliers(0.5, rule="mean"))


def _signal(C, S, seed):
    rng = np.random.default_rng(seed)
    T, r = rng.normal(size=(N, M)), rng.normal(size=N)
    return rng.normal(size=(C, S, M)) + 3.0, T, r


def test_signal_moments():
    b, T, r = _signal(3, 31, 9)
    post = _sums(_pout(3, 31, 1), b, T, r)
    tb = (b @ T.T).reshape(-1, N)
    np.testing.assert_allclose(post.signal_mean_toa(r), tb.mean(axis=0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(post.signal_mean_toa(r), post.signal_mean(T), rtol=1e-12,
                               atol=1e-13)
    np.testing.assert_allclose(post.signal_sd(), tb.std(axis=0), rtol=1e-10)
    np.testing.assert_allclose(post.signal_sd(pool=False), (b @ T.T).std(axis=1), rtol=1e-10)


def test_merging_and_files(tmp_path):
    b, T, r = _signal(3, 40, 4)
    p = _pout(3, 40, 6)
    whole = _sums(p, b, T, r)
    a, c = _sums(p[:, :15], b[:, :15], T, r), _sums(p[:, 15:], b[:, 15:], T, r)
    both = a + c
    np.testing.assert_array_equal(both.count, whole.count)
    np.testing.assert_array_equal(both.pout_gt, whole.pout_gt)
    np.testing.assert_allclose(both.resid_sq, whole.resid_sq, rtol=1e-13)
    np.testing.assert_array_equal(both.pout_thr, THR)
    with pytest.raises(ValueError, match="thresholds differ"):
        a + _sums(p[:, 15:], b[:, 15:], T, r, thr=(0.2, 0.5, 0.8))
    with pytest.raises(ValueError, match="one operand only"):
        a + _sums(p[:, 15:])
    cat = _sums(p[:2], b[:2], T, r).concat(_sums(p[2:], b[2:], T, r))
    assert cat.pout_gt.shape == (3, 3, N) and cat.resid_sum.shape == (3, N)
    for k in ("pout_gt", "resid_sum", "resid_sq", "b_sum", "count"):
        np.testing.assert_array_equal(getattr(cat, k), getattr(whole, k))
    with pytest.raises(ValueError, match="thresholds differ"):
        whole.concat(_sums(p, b, T, r, thr=(0.1, 0.5, 0.9)))
    sel = whole.select(slice(1, 3), n=7)
    assert sel.pout_gt.shape == (3, 2, 7) and sel.resid_sq.shape == (2, 7)
    assert sel.b_sum.shape == (2, M)
    np.testing.assert_array_equal(sel.pout_gt, whole.pout_gt[:, 1:3, :7])
    # the pooled vector: today's entries first, the new arrays appended
    old = PosteriorSums(whole.count, pout_sum=whole.pout_sum, b_sum=whole.b_sum, b_sq=whole.b_sq)
    v_old, v = old.pooled_vector(), whole.pooled_vector()
    np.testing.assert_array_equal(v[:v_old.shape[0]], v_old)
    assert v.shape[0] == v_old.shape[0] + (len(THR) + 2) * N
    back = whole.from_pooled_vector(v)
    assert back.nchains == 1 and back.count[0] == 120
    np.testing.assert_array_equal(back.pout_gt[:, 0], whole.pout_gt.sum(axis=1))
    np.testing.assert_array_equal(back.pout_median_gt(0.5)[0], whole.pout_median_gt(0.5)[0])
    np.testing.assert_allclose(back.signal_sd(), whole.signal_sd(), rtol=1e-12)
    # files, with and without the new arrays
    whole.save(tmp_path / "new.npz")
    got = PosteriorSums.load(tmp_path / "new.npz")
    for k in ("count", "pout_sum", "b_sum", "b_sq", "pout_thr", "pout_gt", "resid_sum",
              "resid_sq"):
        np.testing.assert_array_equal(getattr(got, k), getattr(whole, k))
    assert got.z_sum is None
    old.save(tmp_path / "old.npz")
    with np.load(tmp_path / "old.npz") as f:
        assert sorted(f.files) == ["b_sq", "b_sum", "count", "pout_sum"]   # today's file
    got = PosteriorSums.load(tmp_path / "old.npz")
    assert got.pout_gt is None and got.pout_thr is None and got.resid_sum is None


# ---- gloo all-reduce of the pooled vector at world 2 -----------------------------------
C2, S2 = 3, 31


def _rank_data(rank):
    b, T, r = _signal(C2, S2, 12)
    b = b + np.random.default_rng([3, rank]).normal(size=b.shape)
    lo = 10 * rank                  # the ranks need not have counted the same number of sweeps
    return _pout(C2, S2, [21, rank])[:, lo:], b[:, lo:], T, r


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init("gloo")
    mine = _sums(*_rank_data(rank))
    vec, _ = dist.reduce_summary(mine.pooled_vector(), np.zeros(1))
    allp = mine.from_pooled_vector(vec)
    gt, amb = allp.pout_median_gt(0.5)
    out.put((rank, int(allp.count[0]), gt.tolist(), amb.tolist(), allp.signal_sd().tolist(),
             allp.pout_exceed_frac(0.9).tolist()))
    dist.finalize()


def test_two_rank_pooling_of_counts_and_band():
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
    assert res[0][1:] == res[1][1:]
    ps, tbs = [], []
    for rank in range(2):
        p, b, T, r = _rank_data(rank)
        ps.append(p.reshape(-1, N))
        tbs.append((b @ T.T).reshape(-1, N))
    p, tb = np.concatenate(ps), np.concatenate(tbs)
    _, count, gt, amb, sd, frac = res[0]
    assert count == C2 * S2 + C2 * (S2 - 10) and count % 2 == 0
    amb = np.array(amb)
    np.testing.assert_array_equal(amb, 2 * (p > 0.5).sum(axis=0) == count)
    np.testing.assert_array_equal(np.array(gt)[~amb], (np.median(p, axis=0) > 0.5)[~amb])
    np.testing.assert_allclose(sd, tb.std(axis=0), rtol=1e-10)
    np.testing.assert_array_equal(frac, (p > 0.9).mean(axis=0))
