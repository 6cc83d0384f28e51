"""The law of the chains of a model with a DM process against the reference itself, without
convergence: the scheme of test_gpu_ks.test_same_start_law_matches_reference on dmg
(persistent kernel, red 7 + DM 5 components) and dmx (large path, ECORR epochs first, red 10 +
DM 10 components and 60 ECORR epochs).  tests/golden/mgp_samestart_<ds>_beta.npz holds 256
chains x 2000 sweeps of the reference (tools/same_start_ref.py) from prior draws of x and
gibbs.py:29-51's latent start; 4096 GPU chains from the same start law must pass two-sample
KS tests at five sweeps and on the second-half means, for every parameter, theta and nu."""
import pytest

from gpu_support import same_start_ks_failures
from gibbs_student_t_amd.native import NativeSampler
from gibbs_student_t_amd.run_sims import MODELS
from golden_io import MGP_DATASETS, load_dataset, load_samestart

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dataset", ["dmg", "dmx"])
def test_same_start_law_matches_reference(dataset):
    ref = load_samestart(dataset)
    pta = load_dataset(dataset=dataset)
    assert (len(ref["x0"]), int(ref["sweeps"])) == (256, 2000)
    ns = NativeSampler(pta, MODELS["beta"], 0)
    assert ns.path == MGP_DATASETS[dataset][2] and ns.procs.nproc == 2
    bad = same_start_ks_failures(ns, pta, ref, label=dataset)
    assert not bad, bad
