"""The draw-law harness on a CPU (no device): the Philox mirror against its known answers and
its own laws, every statistic of draw_laws.py on draws the oracle makes with numpy's generator
at each (state, N) that test_gpu_draw_laws.py uses, and the calibration of the covariance
test.  The oracle's fp64 draws of the exact algorithm stay inside the bounds at those states'
condition numbers, so a failure of the same statistic on the device is the kernel's."""
import warnings

import numpy as np
import pytest
import scipy.stats

import draw_laws as dl
from oracle import philox_variates as pv
from oracle.gibbs_oracle import DF_GRID, MH_PROBS, Oracle, OutlierModel
from support import KAT


class NumpyVariates:
    """Oracle variate source on numpy's Generator (the draws of the exact laws)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def b_normals(self, m):
        return self.rng.standard_normal(m)

    def beta(self, a, b):
        return self.rng.beta(a, b)

    def bernoulli(self, q):
        return (self.rng.random(len(q)) < np.minimum(q, 1.0)).astype(np.float64)

    def gamma(self, shape):
        return self.rng.standard_gamma(shape)

    def df_choice(self, p):
        return self.rng.choice(DF_GRID, p=p)


# ---- the Philox mirror ------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", KAT)
def test_mirror_known_answers(ctr, key, want):
    c = [int(w, 16) for w in ctr.split()]
    k = [int(w, 16) for w in key.split()]
    got = pv.philox4x32_10(*c, *k)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_mirror_counter_layout():
    """(index, tag, sweep, chain) are counter words 0..3, the seed's halves the key."""
    seed = 0x299F31D0A4093822
    a, b = pv.uniform2(seed, chain=0x03707344, sweep=0x13198A2E, tag=0x85A308D3, index=0x243F6A88)
    w = [int(v, 16) for v in KAT[2][2].split()]
    assert a == ((w[1] << 32 | w[0]) >> 11) * 2.0 ** -53
    assert b == ((w[3] << 32 | w[2]) >> 11) * 2.0 ** -53


@pytest.fixture(scope="module")
def mirror_draws():
    """About 1e7 MH variates of the mirror: 2048 chains x 164 sweeps x 30 steps."""
    wind, hind = np.array([0, 1, 2]), np.array([3, 4, 5, 6, 7])
    t = pv.mh_tape(0x1234567887654321, 1000 + np.arange(2048), 77 + np.arange(164), wind, hind)
    return wind, hind, t[..., :80].reshape(-1, 4), t[..., 80:].reshape(-1, 4)


def test_mirror_index_and_scale_laws(mirror_draws):
    wind, hind, white, hyper = mirror_draws
    cdf = np.cumsum(MH_PROBS) / np.sum(MH_PROBS)
    for ind, e in ((wind, white), (hind, hyper)):
        p, cells = dl.categorical_chi2(e[:, 1], ind, np.full(len(ind), 1.0 / len(ind)))
        assert cells == len(ind) and p > dl.P_MIN, p
        p, cells = dl.categorical_chi2(pv.scale_class(e[:, 0], cdf), np.arange(5), MH_PROBS)
        assert cells == 5 and p > dl.P_MIN, p
        assert dl.ks_uniform(e[:, 3])[0] > dl.P_MIN


def test_mirror_normal_law(mirror_draws):
    xi = np.concatenate([mirror_draws[2][:, 2], mirror_draws[3][:, 2]])
    N = len(xi)
    assert N > 9e6
    assert dl.ks_normal(xi) > dl.P_MIN
    assert abs(xi.mean()) * np.sqrt(N) <= dl.Z_MAX
    assert abs(xi.var() - 1.0) / np.sqrt(2.0 / N) <= dl.Z_MAX
    for k in (3, 4, 5):
        p = 2.0 * scipy.stats.norm.sf(k)
        cnt = (np.abs(xi) > k).sum()
        assert abs(cnt - N * p) <= dl.Z_MAX * np.sqrt(N * p * (1 - p)), (k, cnt, N * p)


# ---- harness self-test: the oracle's own draws ------------------------------------------------
@pytest.mark.parametrize("name", dl.B_STATES)
def test_oracle_b_draws_pass(name):
    pta, kw, st, x = dl.b_case(name)
    orc = Oracle(pta, OutlierModel(**kw))
    Sigma, d = orc.sigma_matrix(st, x)
    assert st.z.sum() >= 1 and orc.floor_shift(Sigma) == 0.0
    N = dl.C_B * dl.b_sweeps(pta.m)
    assert N >= 64 * pta.m
    src = NumpyVariates(101)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b = np.stack([orc.draw_b(st, x, src, mean="floor") for _ in range(N)])
    stats = dl.b_draw_stats(dl.Whitener(Sigma, d)(b))
    dl.assert_b_draw(stats, name)


@pytest.mark.parametrize("name", sorted({c[0] for c in dl.THETA_CASES}))
@pytest.mark.parametrize("k", dl.THETA_K)
def test_oracle_theta_draws_pass(name, k):
    pta, kw, st, _ = dl.fixture_case(name)
    st.z = dl.flag_first(pta.n, k)
    orc = Oracle(pta, OutlierModel(**kw))
    src = NumpyVariates(102)
    N = dl.THETA_CS[0] * dl.THETA_CS[1]
    th = np.array([orc.draw_theta(st, src) for _ in range(N)])
    dl.assert_beta(dl.beta_stats(th, *dl.theta_shapes(pta, kw, k)), (name, k))


@pytest.mark.parametrize("name", sorted({c[0] for c in dl.Z_CASES}))
def test_oracle_z_draws_pass(name):
    pta, kw, st, x = dl.z_case(name)
    orc = Oracle(pta, OutlierModel(**kw))
    q = orc.outlier_prob(st, x)
    assert ((q > 0.02) & (q < 0.98)).mean() >= 0.5, name
    C, S = dl.Z_CS
    src = NumpyVariates(103)
    z = np.stack([orc.draw_z(st, x, src)[0] for _ in range(C * S)]).reshape(C, S, -1)
    dl.assert_bernoulli(dl.bernoulli_stats(z, np.minimum(q, 1.0)), name)


@pytest.mark.parametrize("name", sorted({c[0] for c in dl.ALPHA_CASES}))
@pytest.mark.parametrize("nu", dl.ALPHA_NU)
def test_oracle_alpha_draws_pass(name, nu):
    pta, kw, st, x = dl.fixture_case(name)
    st.nu = nu
    assert 1 <= st.z.sum() < pta.n
    orc = Oracle(pta, OutlierModel(**kw))
    rate, shape = dl.alpha_law(orc, st, x)
    C, S = dl.ALPHA_CS
    src = NumpyVariates(104)
    al = np.stack([orc.draw_alpha(st, x, src) for _ in range(C * S)]).reshape(C, S, -1)
    dl.assert_pit(dl.pit_stats(dl.alpha_pit(al, rate, shape)), (name, nu))


@pytest.mark.parametrize("name", dl.NU_FIXTURES)
def test_oracle_nu_draws_pass(name):
    pta, kw, st, x, p = dl.nu_case(name)
    N = dl.NU_CS[0] * dl.NU_CS[1]
    assert dl.big_cells(p, N) >= 4
    orc = Oracle(pta, OutlierModel(**kw))
    src = NumpyVariates(105)
    nu = np.array([orc.draw_nu(st, src) for _ in range(N)])
    pval, cells = dl.categorical_chi2(nu, DF_GRID, p)
    assert cells >= 4 and pval > dl.P_MIN, (name, pval, cells)


# ---- calibration of the covariance test -------------------------------------------------------
B_M = (54, 58, 62, 74, 94, 134, 164, 180)     # the b-draw states' basis sizes (checked below)


@pytest.mark.parametrize("m", B_M)
def test_covariance_test_is_calibrated(m):
    """200 replications of N x m numpy normals at the (N, m) of a b-draw case: the Bartlett-
    corrected p-values are uniform (KS p > 1e-3)."""
    N = dl.C_B * dl.b_sweeps(m)
    rng = np.random.default_rng(1000 + m)
    p = np.array([dl.covariance_lr(rng.standard_normal((N, m)))[1] for _ in range(200)])
    assert dl.ks_uniform(p)[0] > 1e-3, (m, N, dl.ks_uniform(p)[0])


def test_calibrated_sizes_are_the_cases_sizes():
    assert {dl.b_case(s)[0].m for s in dl.B_STATES} == set(B_M)
