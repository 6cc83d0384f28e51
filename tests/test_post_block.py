"""post.PosteriorSums with the block second moment of b (b_outer, b_block): covariance and
waveforms against a long-double computation on the chain itself, within the derived rounding
bound (block_support.waveform_reference); the block travels through every merge and file
form, and objects without it look as they always did."""
import io
import zipfile

import numpy as np
import pytest

from block_support import LD, assert_waveform, packed_outer_sums, tri_index
from gibbs_student_t_amd.post import PosteriorSums

C, N, M = 3, 40, 12
BLOCK = (2, 7)
COLS = slice(BLOCK[0], BLOCK[0] + BLOCK[1])


@pytest.fixture(scope="module")
def bchain():
    """[C, N, m] with strongly correlated columns (a steep spectrum on a common factor) and a
    mean far from zero in some of them"""
    rng = np.random.default_rng(2017)
    common = rng.standard_normal((C, N, 1))
    scale = 10.0 ** -np.arange(M)[None, None, :] ** 0.7
    b = scale * (common + 0.3 * rng.standard_normal((C, N, M)))
    b[..., 3] += 5.0 * scale[..., 3]
    b[..., 6] -= 2.0 * scale[..., 6]
    return b


def sums_of(b, block=BLOCK, first=0):
    """The sums a device run would leave: sequential fp64 additions of the records first.."""
    bs, bq = np.zeros((b.shape[0], b.shape[2])), np.zeros((b.shape[0], b.shape[2]))
    for s in range(first, b.shape[1]):
        bs = bs + b[:, s]
        bq = bq + b[:, s] * b[:, s]
    kw = {}
    if block is not None:
        kw = dict(b_outer=packed_outer_sums(b, block, first), b_block=block)
    return PosteriorSums(np.full(b.shape[0], b.shape[1] - first), b_sum=bs, b_sq=bq, **kw)


@pytest.fixture(scope="module")
def B():
    rng = np.random.default_rng(7)
    return rng.standard_normal((25, BLOCK[1])) * 10.0 ** rng.uniform(-1, 1, size=(25, 1))


def cov_ld(bs):
    bs = bs.astype(LD)
    mu = bs.mean(axis=0)
    d = bs - mu
    return d.T @ d / bs.shape[0]                 # np.cov(bs.T, bias=True)


def test_b_cov_pooled_and_per_chain(bchain):
    ps = sums_of(bchain)
    K = BLOCK[1]
    for label, got, samples in [("pooled", ps.b_cov(), bchain[..., COLS].reshape(-1, K))] + \
            [(f"chain {c}", ps.b_cov(pool=False)[c], bchain[c, :, COLS]) for c in range(C)]:
        assert got.shape == (K, K)
        np.testing.assert_array_equal(got, got.T)
        want = cov_ld(samples)
        # element (i, j) is the waveform covariance of the unit rows e_i, e_j: the same bound
        n = samples.shape[0]
        s = samples.astype(LD)
        mu = s.mean(axis=0)
        tol = (n + K + 4) * 2.0 ** -52 * (np.abs(s[:, :, None] * s[:, None, :]).sum(axis=0) / n
                                          + np.abs(mu[:, None] * mu[None, :]))
        err = np.abs(got.astype(LD) - want)
        print(f"{label}: worst err / tol {float(np.max(err / tol)):.3g}")
        assert np.all(err <= tol), label
    assert ps.b_cov(pool=False).shape == (C, K, K)
    # the diagonal is b_var's
    np.testing.assert_allclose(np.diagonal(ps.b_cov()), ps.b_var()[COLS], rtol=1e-9)


def test_waveform_against_long_double(bchain, B):
    ps = sums_of(bchain)
    K = BLOCK[1]
    mean, sd = ps.waveform(B)
    assert mean.shape == sd.shape == (25,)
    assert_waveform(mean, sd, B, bchain[..., COLS].reshape(-1, K), "pooled")
    mean_c, sd_c = ps.waveform(B, pool=False)
    assert mean_c.shape == sd_c.shape == (C, 25)
    for c in range(C):
        assert_waveform(mean_c[c], sd_c[c], B, bchain[c, :, COLS], f"chain {c}")
    # the pooled band is not the mean of the chains' bands: the chains' means differ
    assert not np.allclose(sd, sd_c.mean(axis=0), rtol=1e-6)
    # a slice inside the block
    sub = slice(1, 5)
    m2, s2 = ps.waveform(B[:, sub], cols=sub)
    assert_waveform(m2, s2, B[:, sub], bchain[..., BLOCK[0] + 1:BLOCK[0] + 5].reshape(-1, 4),
                    "cols 1:5")
    with pytest.raises(ValueError, match="need \\[T, 7\\]"):
        ps.waveform(B[:, :5])
    with pytest.raises(ValueError, match="contiguous slice"):
        ps.waveform(B[:, ::2], cols=slice(0, 7, 2))
    with pytest.raises(ValueError, match="b_outer was not accumulated"):
        sums_of(bchain, block=None).waveform(B)


def test_sd_is_clamped_at_zero():
    """A coefficient that never moves: M / N - mu mu^T may round below zero"""
    b = np.full((1, 7, 3), 0.1) * np.array([1.0, 3.0, 7.0])
    ps = sums_of(b, block=(0, 3))
    _, sd = ps.waveform(np.eye(3))
    assert np.all(sd >= 0.0) and np.all(sd < 1e-8)


def test_merges_keep_the_block(bchain):
    full = sums_of(bchain)
    i, _ = tri_index(BLOCK[1])
    assert full.b_outer.shape == (C, len(i)) and full.b_block == BLOCK
    # + : the same chains over more sweeps
    a, b = sums_of(bchain[:, :15]), sums_of(bchain, first=15)
    both = a + b
    assert both.b_block == BLOCK and np.all(both.count == N)
    np.testing.assert_allclose(both.b_outer, full.b_outer, rtol=1e-13)
    np.testing.assert_allclose(both.b_cov(), full.b_cov(), rtol=1e-9, atol=1e-30)
    # concat / select: other chains
    cat = sums_of(bchain[:2]).concat(sums_of(bchain[2:]))
    assert cat.b_block == BLOCK
    np.testing.assert_array_equal(cat.b_outer, full.b_outer)
    sel = full.select([2, 0], n=5)
    assert sel.b_block == BLOCK and sel.b_sum.shape == (2, M)
    np.testing.assert_array_equal(sel.b_outer, full.b_outer[[2, 0]])      # never cut to n
    np.testing.assert_array_equal(full.select(slice(1, 3)).b_cov(pool=False),
                                  full.b_cov(pool=False)[1:3])
    # pooled: one pseudo-chain with the pooled covariance
    p = full.pooled()
    assert p.nchains == 1 and p.b_block == BLOCK
    np.testing.assert_allclose(p.b_cov(pool=False)[0], full.b_cov(), rtol=1e-12, atol=1e-30)


def test_pooled_vector_round_trip(bchain):
    full = sums_of(bchain)
    vec = full.pooled_vector()
    ne = BLOCK[1] * (BLOCK[1] + 1) // 2
    assert vec.shape == (1 + 2 * M + ne,)
    # the block comes after every other sum
    np.testing.assert_array_equal(vec[-ne:], full.pooled().b_outer[0])
    np.testing.assert_array_equal(vec[:1 + 2 * M], sums_of(bchain, block=None).pooled_vector())
    back = full.from_pooled_vector(2.0 * vec)          # two ranks with the same sums
    assert back.b_block == BLOCK and back.count[0] == 2 * C * N
    np.testing.assert_array_equal(back.b_outer, 2.0 * full.pooled().b_outer)
    np.testing.assert_allclose(back.b_cov(), full.b_cov(), rtol=1e-12, atol=1e-30)
    with pytest.raises(ValueError, match="expected"):
        full.from_pooled_vector(vec[:-1])


def test_save_load_keep_the_block(bchain, tmp_path):
    full = sums_of(bchain)
    full.save(tmp_path / "post.npz")
    back = PosteriorSums.load(tmp_path / "post.npz")
    assert back.b_block == BLOCK and isinstance(back.b_block, tuple)
    np.testing.assert_array_equal(back.b_outer, full.b_outer)
    np.testing.assert_array_equal(back.b_cov(), full.b_cov())


def test_different_blocks_do_not_merge(bchain):
    a, b = sums_of(bchain), sums_of(bchain, block=(3, 7))
    none = sums_of(bchain, block=None)
    for x, y in ((a, b), (a, none), (none, a)):
        with pytest.raises(ValueError, match="b blocks differ"):
            x + y
        with pytest.raises(ValueError, match="b blocks differ"):
            x.concat(y)
    with pytest.raises(ValueError, match="go together"):
        PosteriorSums([4], b_outer=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="go together"):
        PosteriorSums([4], b_block=(0, 2))
    with pytest.raises(ValueError, match="block of 2 columns"):
        PosteriorSums([4], b_outer=np.zeros((1, 4)), b_block=(0, 2))


def test_objects_without_a_block_serialise_as_before(bchain, tmp_path):
    """The file of an object without a block holds the arrays it always held, byte for byte
    what numpy writes for them in the old order; its pooled vector is unchanged"""
    rng = np.random.default_rng(3)
    z = rng.random((C, 9))
    gt = rng.integers(0, 5, size=(2, C, 9)).astype(float)
    ps = PosteriorSums(np.full(C, N), z_sum=z, b_sum=bchain.sum(axis=1),
                       b_sq=(bchain ** 2).sum(axis=1), pout_thr=[0.5, 0.9], pout_gt=gt,
                       resid_sum=z + 1.0)
    assert ps.b_outer is None and ps.b_block is None
    ps.save(tmp_path / "plain.npz")
    old = io.BytesIO()
    np.savez(old, count=ps.count, z_sum=ps.z_sum, b_sum=ps.b_sum, b_sq=ps.b_sq, pout_gt=ps.pout_gt,
             resid_sum=ps.resid_sum, pout_thr=ps.pout_thr)
    # (member by member: a zip archive also holds the time it was written)
    with zipfile.ZipFile(tmp_path / "plain.npz") as new, zipfile.ZipFile(old) as ref:
        assert new.namelist() == ref.namelist()
        for name in ref.namelist():
            assert new.read(name) == ref.read(name), name
    with np.load(tmp_path / "plain.npz") as f:
        assert f.files == ["count", "z_sum", "b_sum", "b_sq", "pout_gt", "resid_sum", "pout_thr"]
    back = PosteriorSums.load(tmp_path / "plain.npz")
    assert back.b_outer is None and back.b_block is None
    p = ps.pooled()
    want = np.concatenate([[C * N], p.z_sum[0], p.b_sum[0], p.b_sq[0], p.pout_gt.reshape(-1),
                           p.resid_sum[0]])
    np.testing.assert_array_equal(ps.pooled_vector(), want)
    assert (ps + ps).b_block is None and ps.concat(ps).b_block is None
    assert ps.select([0]).b_block is None and ps.from_pooled_vector(want).b_block is None
