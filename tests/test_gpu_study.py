"""run_sims grid on the GPU: one batched launch per chunk, reference output layout."""
import os

import numpy as np
import pytest

import gpu_support  # noqa: F401  (importing it is the device gate)
from gibbs_student_t_amd import run_sims
from gibbs_student_t_amd.native import NativeSampler

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("generator", ["host", "device"])
def test_study_writes_reference_layout(tmp_path, generator):
    entries = run_sims.build_grid(thetas=(0.05, 0.15), realisations=1, generator=generator)
    st = run_sims.Study(entries, chains=1, seed=3)
    _, secs = st.run(260, burn=100, outdir=str(tmp_path), chunk=64)
    st.close()
    for e in entries:
        d = e.outdir(str(tmp_path))
        n, m = e.pta.n, e.pta.T.shape[1]
        shapes = {"chain": (160, 3), "bchain": (160, m), "zchain": (160, n),
                  "poutchain": (160, n), "thetachain": (160,), "alphachain": (160, n),
                  "dfchain": (160,)}
        for f, shp in shapes.items():
            a = np.load(os.path.join(d, f + ".npy"))
            assert a.shape == shp, (d, f, a.shape)
            assert np.all(np.isfinite(a))
        if e.model == "vvh17":                  # vary_alpha=False, alpha=1e10 (run_sims.py:90)
            assert np.all(np.load(os.path.join(d, "alphachain.npy")) == 1e10)
            assert np.all(np.load(os.path.join(d, "dfchain.npy")) == 4.0)  # vary_df=False
        if e.model in ("gaussian", "t"):        # theta never updated (gibbs.py:187-190)
            assert np.all(np.load(os.path.join(d, "thetachain.npy")) == 0.01)


def test_study_chain_equals_standalone_sampler():
    """An entry inside the batched grid == the same (dataset, model) run alone (bitwise)."""
    entries = run_sims.build_grid(thetas=(0.1,), realisations=1)
    st = run_sims.Study(entries, chains=2, seed=11)
    recs, _ = st.run(40, burn=10, chunk=16)
    st.close()
    k = 7   # no_outlier twin (ragged n) under the 'beta' model
    e = entries[k]
    ns = NativeSampler(e.pta, e.cfg, 0)
    ns.alloc(2)
    init = run_sims.initial_state(e, 2, k * 2, 11, e.pta.n)
    ns.set_state(**init)
    rec = ns.alloc_records(40)
    ns.sweep(40, records=rec, seed=11, chain0=k * 2)
    x = rec["x"].cpu().numpy()[:, 10:]
    np.testing.assert_array_equal(recs["x"][k], x)
    np.testing.assert_array_equal(recs["alpha"][k][..., :e.pta.n],
                                  rec["alpha"].cpu().numpy()[:, 10:])
    ns.close()


@pytest.mark.parametrize("generator", ["host", "device"])
def test_outlier_model_finds_injected_outliers(generator):
    """Mixture model on an outlier dataset: true outliers get the high outlier probability
    (with the datasets drawn per dataset on the host or all at once on the GPU)."""
    entries = [e for e in run_sims.build_grid(thetas=(0.15,), realisations=1, models=("beta",),
                                              generator=generator)
               if e.kind == "outlier"]
    st = run_sims.Study(entries, chains=64, seed=5)
    recs, _ = st.run(600, burn=200, chunk=200, keys=("x", "pout"))
    st.close()
    zt = entries[0].meta["z_true"].astype(bool)
    pout = recs["pout"][0].mean(axis=(0, 1))[:entries[0].pta.n]
    assert zt.sum() >= 5
    assert pout[zt].mean() > 0.5 > pout[~zt].mean()
