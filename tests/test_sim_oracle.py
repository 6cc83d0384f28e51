"""The batched-generator oracle (oracle/sim_oracle.py): its Philox against the Random123
known answers, and its recipe against the host restatement of simulate_data.py."""
import numpy as np
import pytest

from oracle import sim_oracle as so
from gibbs_student_t_amd import data
from gibbs_student_t_amd.model import FYR, fourier_basis, svd_tm_basis

from support import KAT, j1713_epochs as _j1713


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_numpy_philox_known_answers(ctr, key, want):
    c = [int(x, 16) for x in ctr.split()]
    k = [int(x, 16) for x in key.split()]
    out = so.philox(*c, *k)
    assert " ".join(f"{int(v):08x}" for v in out) == want


def test_recipe_properties():
    """Refit residuals are orthogonal to the timing model; the clean twin is the refit on
    the kept TOAs (the host restatement's SVD of M[keep] gives the same vector)."""
    toas, M, raw = _j1713()
    U = svd_tm_basis(M)[0]
    F, ff = fourier_basis(toas, 30)
    f = ff[::2]
    df = np.diff(np.concatenate(([0.0], f)))
    zs = []
    for d in range(40):
        r, err, z, r2 = so.simulate(F, U, seed=11, dataset=d, theta=0.2, sigma_out=1e-6,
                                    lf=np.log(ff), ldf=np.log(np.repeat(df, 2)),
                                    log_fyr=np.log(FYR))
        assert np.abs(U.T @ r).max() < 1e-12 * np.abs(r).max() * len(r)
        k = z == 0
        U2 = np.linalg.svd(M[k], full_matrices=False)[0]
        want = r[k] - U2 @ (U2.T @ r[k])
        # cond(M[keep]) ~ 3e11: the host SVD path carries ~1e-11 relative error
        np.testing.assert_allclose(r2[k], want, rtol=0, atol=1e-10 * np.abs(want).max())
        assert np.all(r2[~k] == 0.0)
        assert np.all((err > 1e-8) & (err < 1e-6))
        zs.append(z)
    assert abs(np.mean(zs) - 0.2) < 0.03


def test_student_t_white_noise():
    """dof > 0: sqrt(dof/2) N / sqrt(Gamma(dof/2)) is Student-t(dof) (KS, 4000 draws)."""
    import scipy.stats
    n = 4000
    U = np.zeros((n, 0))
    r, err, z, _ = so.simulate(None, U, seed=3, dataset=0, theta=0.0, sigma_out=1e-6,
                               red=np.zeros(n), toaerrs=np.ones(n), dof=4.0, clean=False)
    assert scipy.stats.kstest(r, scipy.stats.t(4).cdf).pvalue > 1e-3
