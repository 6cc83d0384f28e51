"""The law of the chains of a model with a DM process against the reference itself, without
convergence: the scheme of test_gpu_ks.test_same_start_law_matches_reference on dmg
(persistent kernel, red 7 + DM 5 components) and dmx (large path, ECORR epochs first, red 10 +
DM 10 components and 60 ECORR epochs).  tests/golden/mgp_samestart_<ds>_beta.npz holds 256
chains x 2000 sweeps of the reference (tools/same_start_ref.py) from prior draws of x and
gibbs.py:29-51's latent start; 4096 GPU chains from the same start law must pass two-sample
KS tests at five sweeps and on the second-half means, for every parameter, theta and nu."""
import numpy as np
import pytest
import scipy.stats

import mgp_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from gibbs_student_t_amd._abi import STATUS_ERRORS  # noqa: E402
from gibbs_student_t_amd.native import NativeSampler  # noqa: E402
from gibbs_student_t_amd.run_sims import MODELS  # noqa: E402
from test_gpu_ks import SAME_START_P  # noqa: E402


@pytest.mark.parametrize("dataset", ["dmg", "dmx"])
def test_same_start_law_matches_reference(dataset):
    ref = mgp_io.load_samestart(dataset)
    pta = mgp_io.load_dataset(dataset)
    x0r, S, thin = ref["x0"], int(ref["sweeps"]), int(ref["thin"])
    assert (len(x0r), S) == (256, 2000)
    R = ref["x"].shape[1]
    C = 4096
    lo = np.array([p.pmin for p in pta.params])
    hi = np.array([p.pmax for p in pta.params])
    x0 = np.concatenate([x0r, np.random.default_rng(17).uniform(lo, hi, size=(C - len(x0r), len(lo)))])
    ns = NativeSampler(pta, MODELS["beta"], 0)
    assert ns.path == mgp_io.DATASETS[dataset][2] and ns.procs.nproc == 2
    ns.alloc(C)
    ns.set_state(x=x0, z=np.ones((C, pta.n)), alpha=np.ones((C, pta.n)),
                 theta=np.full(C, 0.01), nu=np.full(C, 4.0))
    rec = ns.alloc_records(R, keys=("x", "theta", "nu"))
    ns.sweep(R * thin, records=rec, record_every=thin, seed=2024)
    assert np.all((ns.get_state()["status"] & STATUS_ERRORS) == 0)
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    ns.close()
    names = [str(s) for s in ref["names"]]
    assert names == pta.param_names
    series = [(nm, got["x"][..., j], ref["x"][..., j]) for j, nm in enumerate(names)]
    series += [("theta", got["theta"], ref["theta"]), ("nu", got["nu"], ref["nu"])]
    points = sorted({1, R // 10, R // 4, R // 2, R - 1})
    assert len(points) == 5
    half = R // 2
    bad = []
    for nm, g, r in series:
        for t in points:
            p = scipy.stats.ks_2samp(g[:, t], r[:, t]).pvalue
            print(f"{dataset} {nm}@{t * thin}: p={p:.3g}")
            if p <= SAME_START_P:
                bad.append(f"{nm}@{t * thin}: p={p:.1e} gpu {g[:, t].mean():.4g} ref {r[:, t].mean():.4g}")
        gm, rm = g[:, half:].mean(axis=1), r[:, half:].mean(axis=1)
        p = scipy.stats.ks_2samp(gm, rm).pvalue
        print(f"{dataset} {nm} window mean: p={p:.3g}")
        if p <= SAME_START_P:
            bad.append(f"{nm} window mean: p={p:.1e} gpu {gm.mean():.4g} ref {rm.mean():.4g}")
    assert not bad, bad
