"""post.PosteriorSums against numpy on synthetic chains: means, variance, pooling, merging
with +, the pooled vector that ranks exchange and the .npz round trip."""
import numpy as np
import pytest

from gibbs_student_t_amd.post import PosteriorSums

C, S, N, M = 3, 50, 7, 5


@pytest.fixture(scope="module")
def chains():
    rng = np.random.default_rng(4)
    p = np.array([0.02, 0.95, 0.5, 0.99, 0.0, 1.0, 0.91])
    return dict(z=(rng.uniform(size=(C, S, N)) < p).astype(float),
                pout=rng.uniform(size=(C, S, N)), alpha=rng.gamma(2.0, size=(C, S, N)),
                b=rng.normal(size=(C, S, M)) * np.arange(1, M + 1))


def sums(ch, lo=0, hi=S, chains_=slice(None)):
    sl = (chains_, slice(lo, hi))
    return PosteriorSums(np.full(len(range(C)[chains_]), hi - lo), z_sum=ch["z"][sl].sum(axis=1),
                         pout_sum=ch["pout"][sl].sum(axis=1), alpha_sum=ch["alpha"][sl].sum(axis=1),
                         b_sum=ch["b"][sl].sum(axis=1), b_sq=(ch["b"][sl] ** 2).sum(axis=1))


def test_means_per_chain_and_pooled(chains):
    ps = sums(chains)
    for name, key in (("z_mean", "z"), ("pout_mean", "pout"), ("alpha_mean", "alpha"),
                      ("b_mean", "b")):
        np.testing.assert_allclose(getattr(ps, name)(pool=False), chains[key].mean(axis=1),
                                   rtol=1e-13)
        np.testing.assert_allclose(getattr(ps, name)(), chains[key].reshape(C * S, -1).mean(axis=0),
                                   rtol=1e-13)
    np.testing.assert_allclose(ps.b_var(pool=False), chains["b"].var(axis=1), rtol=1e-10)
    np.testing.assert_allclose(ps.b_var(), chains["b"].reshape(C * S, -1).var(axis=0), rtol=1e-10)


def test_outliers_signal_and_standard_error(chains):
    ps = sums(chains)
    zc = chains["z"].reshape(C * S, N)
    np.testing.assert_array_equal(ps.outliers(), np.flatnonzero(zc.mean(axis=0) > 0.9))
    np.testing.assert_array_equal(ps.outliers(0.4), np.flatnonzero(zc.mean(axis=0) > 0.4))
    T = np.random.default_rng(1).normal(size=(N, M))
    np.testing.assert_allclose(ps.signal_mean(T),
                               (chains["b"].reshape(C * S, M) @ T.T).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(ps.z_mean_se(),
                               chains["z"].mean(axis=1).std(axis=0, ddof=1) / np.sqrt(C), rtol=1e-13)
    with pytest.raises(ValueError):
        sums(chains, chains_=slice(0, 1)).z_mean_se()


def test_unequal_counts_pool_by_total(chains):
    # chain 0 counted 20 sweeps, the others 50: the pooled mean divides by the total count
    z = chains["z"]
    ps = PosteriorSums([20, S, S], z_sum=np.stack([z[0, :20].sum(0), z[1].sum(0), z[2].sum(0)]))
    want = (z[0, :20].sum(0) + z[1].sum(0) + z[2].sum(0)) / (20 + 2 * S)
    np.testing.assert_allclose(ps.z_mean(), want, rtol=1e-14)
    with pytest.raises(ValueError):
        ps.b_mean()              # not accumulated


def test_add_merges_successive_runs(chains):
    both = sums(chains, 0, 20) + sums(chains, 20, S)
    whole = sums(chains)
    np.testing.assert_array_equal(both.count, whole.count)
    for k in ("z_sum", "pout_sum", "alpha_sum", "b_sum", "b_sq"):
        np.testing.assert_allclose(getattr(both, k), getattr(whole, k), rtol=1e-13)
    with pytest.raises(ValueError):
        sums(chains) + sums(chains, chains_=slice(0, 2))
    with pytest.raises(ValueError):
        sums(chains) + PosteriorSums(np.full(C, S), z_sum=chains["z"].sum(axis=1))


def test_concat_and_pooled_vector(chains):
    a, b = sums(chains, chains_=slice(0, 2)), sums(chains, chains_=slice(2, 3))
    whole = sums(chains)
    np.testing.assert_array_equal(a.concat(b).z_sum, whole.z_sum)
    # what two ranks exchange: pooled vectors add up to the pooled sums of all chains
    merged = a.from_pooled_vector(a.pooled_vector() + b.pooled_vector())
    assert merged.count.tolist() == [C * S]
    np.testing.assert_allclose(merged.z_mean(), whole.z_mean(), rtol=1e-14)
    np.testing.assert_allclose(merged.b_var(), whole.b_var(), rtol=1e-10)
    np.testing.assert_array_equal(merged.outliers(), whole.outliers())
    assert (a.pooled() + b.pooled()).count.tolist() == [C * S]


def test_npz_round_trip(chains, tmp_path):
    ps = PosteriorSums(np.full(C, S), z_sum=chains["z"].sum(axis=1), b_sum=chains["b"].sum(axis=1))
    path = tmp_path / "post.npz"
    ps.save(path)
    back = PosteriorSums.load(path)
    np.testing.assert_array_equal(back.count, ps.count)
    assert back.count.dtype == np.int64
    np.testing.assert_array_equal(back.z_sum, ps.z_sum)
    np.testing.assert_array_equal(back.b_sum, ps.b_sum)
    assert back.pout_sum is None and back.alpha_sum is None and back.b_sq is None
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["b_sum", "count", "z_sum"]
