"""PTA.process_basis: a process's Fourier basis at arbitrary epochs on the model's own ladder
(the design matrix of its waveform on any grid), and the column range arguments of
Gibbs.sample(b_cov=) that need no device."""
import numpy as np
import pytest

from block_support import mgp_model
from gibbs_student_t_amd.model import DM_K, FREF_MHZ, PTA
from gibbs_student_t_amd.sampler import b_cov_block
from support import cached_ref


@pytest.fixture(scope="module")
def dm3():
    """red 30 + DM 25 + chromatic 10 components on 390 TOAs in three bands"""
    return mgp_model("dm3")


def test_rebuilt_model_is_the_fixtures(dm3):
    pta, d = dm3
    nf = pta.nfourier
    assert [(q.name, q.col0, q.ncol) for q in pta.procs] == \
        [("red", 0, 60), ("dm_gp", 60, 50), ("chrom_gp", 110, 20)]
    np.testing.assert_array_equal(pta.T[:, :nf], d["T"][:, :nf])
    np.testing.assert_array_equal(pta.Ffreqs, d["Ffreqs"])
    assert pta.Tspan == float(d["toas"].max() - d["toas"].min())


@pytest.mark.parametrize("name", ["red", "dm_gp", "chrom_gp"])
def test_own_epochs_give_the_columns_of_T_bitwise(dm3, name):
    pta, d = dm3
    lo, hi = pta.process_columns(name)
    np.testing.assert_array_equal(pta.process_basis(name), pta.T[:, lo:hi])
    np.testing.assert_array_equal(pta.process_basis(name, toas=d["toas"], freqs=d["freqs"]),
                                  pta.T[:, lo:hi])


@pytest.mark.parametrize("name,chi", [("red", 0), ("dm_gp", 2), ("chrom_gp", 4)])
def test_unscaled_times_weight_is_scaled(dm3, name, chi):
    pta, d = dm3
    w = (FREF_MHZ / d["freqs"]) ** chi
    F = pta.process_basis(name, scaled=False)
    np.testing.assert_array_equal(F * w[:, None] if chi else F, pta.process_basis(name))
    if chi:
        assert not np.array_equal(F, pta.process_basis(name))


def test_other_epochs_same_ladder(dm3):
    pta, d = dm3
    t = np.linspace(d["toas"].min() - 0.1 * pta.Tspan, d["toas"].max() + 0.1 * pta.Tspan, 57)
    F = pta.process_basis("dm_gp", toas=t, scaled=False)
    assert F.shape == (57, 50)
    k = np.arange(1, 26)
    arg = 2.0 * np.pi * t[:, None] * (k / pta.Tspan)[None, :]
    np.testing.assert_allclose(F[:, ::2], np.sin(arg), rtol=0, atol=1e-9)
    np.testing.assert_allclose(F[:, 1::2], np.cos(arg), rtol=0, atol=1e-9)
    # one radio frequency for the whole grid
    np.testing.assert_array_equal(pta.process_basis("dm_gp", toas=t, freqs=700.0), F * 4.0)
    with pytest.raises(ValueError, match="freqs"):
        pta.process_basis("dm_gp", toas=t)
    with pytest.raises(ValueError, match="unknown process"):
        pta.process_basis("ecorr")


def test_explicit_span_is_remembered():
    pta, _ = mgp_model("dmg")
    p2 = PTA(pta.psr, components=7, dm_gp=dict(components=5), Tspan=2.0 * pta.Tspan)
    assert p2.Tspan == 2.0 * pta.Tspan
    np.testing.assert_array_equal(p2.process_basis("dm_gp"), p2.T[:, 14:24])
    assert not np.array_equal(p2.T[:, 14:24], pta.T[:, 14:24])


def test_dm_units_factor(dm3):
    from gibbs_student_t_amd.post import PosteriorSums
    pta, _ = dm3
    assert DM_K == 2.41e-4
    K = 50
    rng = np.random.default_rng(5)
    b = rng.standard_normal((1, 9, pta.m))
    i, j = np.tril_indices(K)
    v = b[:, :, 60:110]
    ps = PosteriorSums([9], b_sum=b.sum(axis=1), b_outer=(v[:, :, i] * v[:, :, j]).sum(axis=1),
                       b_block=(60, K))
    F = pta.process_basis("dm_gp", scaled=False)
    mean_dm, sd_dm = ps.process_waveform(pta, "dm_gp", units="dm")
    mean_u, sd_u = ps.waveform(F * (DM_K * 1400.0 ** 2))
    np.testing.assert_array_equal(mean_dm, mean_u)
    np.testing.assert_array_equal(sd_dm, sd_u)
    mean_s, sd_s = ps.process_waveform(pta, "dm_gp")
    mean_w, sd_w = ps.waveform(pta.T[:, 60:110])
    np.testing.assert_array_equal(mean_s, mean_w)
    np.testing.assert_array_equal(sd_s, sd_w)
    # the factor itself: at 1400 MHz the scaled and unscaled bases agree, so "dm" is "s" x DM_K nu^2
    t = pta.psr.toas[:11]
    m1, s1 = ps.process_waveform(pta, "dm_gp", toas=t, freqs=1400.0)
    m2, s2 = ps.process_waveform(pta, "dm_gp", toas=t, units="dm")
    np.testing.assert_allclose(m2, m1 * 2.41e-4 * 1400.0 ** 2, rtol=1e-13)
    np.testing.assert_allclose(s2, s1 * 2.41e-4 * 1400.0 ** 2, rtol=1e-12)
    with pytest.raises(ValueError, match="block kept"):
        ps.process_waveform(pta, "red")
    with pytest.raises(ValueError, match="units"):
        ps.process_waveform(pta, "dm_gp", units="pc")


def test_from_arrays_model_raises():
    pta = cached_ref("dmg_beta_fixed")["pta"]
    assert pta.Tspan is None
    assert pta.process_columns("dm_gp") == (14, 24)
    with pytest.raises(ValueError, match="rebuilt from arrays"):
        pta.process_basis("dm_gp")
    with pytest.raises(ValueError, match="rebuilt from arrays"):
        pta.process_basis("red", toas=np.arange(4.0))


def test_b_cov_column_ranges(dm3):
    """Gibbs.sample(b_cov=)'s argument, resolved without a device"""
    pta, _ = dm3
    assert b_cov_block(pta, "red") == (0, 60)
    assert b_cov_block(pta, "dm_gp") == (60, 50)
    assert b_cov_block(pta, "chrom_gp") == (110, 20)
    assert b_cov_block(pta, ("chrom_gp", "dm_gp")) == (60, 70)
    assert b_cov_block(pta, ("red", "chrom_gp")) == (0, 130)    # covers dm_gp in between
    assert b_cov_block(pta, "fourier") == (0, 130)
    assert b_cov_block(pta, "all") == (0, pta.m)
    assert b_cov_block(pta, (3, 9)) == (3, 9)
    assert b_cov_block(pta, np.array([128, 4])) == (128, 4)
    one = cached_ref("beta_fixed")["pta"]
    assert b_cov_block(one, "red") == (0, 60) and b_cov_block(one, "all") == (0, 74)
    for bad, msg in (("dm", "unknown process"), (("red", "ecorr"), "unknown process"),
                     ((-1, 4), "columns must lie"), ((0, 0), "columns must lie"),
                     ((140, 10), "columns must lie"), ((1, 2, 3), "need \\(col0, ncol\\)"),
                     (7, "need \\(col0, ncol\\)")):
        with pytest.raises(ValueError, match=msg):
            b_cov_block(pta, bad)
    with pytest.raises(ValueError, match="unknown process"):
        b_cov_block(one, "dm_gp")
    # past GST_BLOCK_MAX: a model wider than 256 columns
    big = PTA.from_arrays("big", np.zeros(4), np.ones(4), np.zeros((4, 300)), np.ones(280), 140)
    assert b_cov_block(big, (10, 256)) == (10, 256)
    for spec in ("all", "fourier", "red", (0, 257)):
        with pytest.raises(ValueError, match="GST_BLOCK_MAX"):
            b_cov_block(big, spec)


def test_run_sims_b_cov_needs_post(capsys):
    from gibbs_student_t_amd import run_sims
    with pytest.raises(SystemExit):
        run_sims.main(["--b-cov", "red"])
    assert "--b-cov need --post" in capsys.readouterr().err
