"""The low-rank Gram over 1, 2 and 8 noise classes and at its edges.

The J1713+0747 epochs (n = 130: three TOA slots, the third holding TOAs 128 and 129) with
the error bars quantised to 1, 2 and 8 distinct values, so that the class loop runs one, two
and eight class Grams and the flagged TOAs belong to different classes.  Flagged sets: none,
TOA 129 alone (the third slot), LR_MAX = 32 TOAs (the last sweep the path takes) and 33 (the
first one the MFMA Gram takes; checked with gst_gram_counts).  The likelihoods of the
low-rank Gram agree with the forced MFMA Gram's within 1e-11 relative, the bound of
test_low_rank_gram_matches_mfma_gram, and a launch of 20 sweeps equals 20 one-sweep launches
bitwise (no state of the Gram survives a sweep).
"""
import functools

import numpy as np
import pytest

from gpu_support import open_sampler, single_sweep_differences
from gibbs_student_t_amd import _abi
from gibbs_student_t_amd.model import PTA
from golden_io import sweep_state
from support import cached_ref, prior_box, rel

pytestmark = pytest.mark.gpu

C = 64
LR_MAX = 32
FLAGGED = {
    "none": [],
    "toa129": [129],
    "lr_max": list(range(2, 126, 4)) + [129],           # 31 over slots 0 and 1, one in slot 2
    "lr_max_plus_1": [0] + list(range(2, 126, 4)) + [129],
}
assert len(FLAGGED["lr_max"]) == LR_MAX and len(FLAGGED["lr_max_plus_1"]) == LR_MAX + 1


def _ref():
    return cached_ref("beta_fixed")


@functools.lru_cache(maxsize=None)
def _pta(ncls):
    """J1713 with error bar sigma (1 + (t mod ncls) / 4): ncls distinct values, and every
    class has TOAs in each slot's lanes"""
    p = _ref()["pta"]
    err = p._toaerrs[0] * (1.0 + 0.25 * (np.arange(p.n) % ncls))
    assert len(np.unique(err)) == ncls
    return PTA.from_arrays("J1713+0747", p._r, err, np.hstack([p.F, p.U]), p.Ffreqs,
                           p.components, p.tm_weight)


def _sampler(ncls):
    return open_sampler(dict(pta=_pta(ncls), kw=_ref()["kw"]), C, "persistent")


def _start(ncls, flagged, seed):
    pta = _pta(ncls)
    n = pta.n
    lo, hi = prior_box(pta)
    z = np.zeros((C, n))
    z[:, flagged] = 1.0
    return dict(x=np.random.default_rng(seed).uniform(lo, hi, size=(C, len(lo))),
                b=np.tile(sweep_state(_ref(), 0)["b"], (C, 1)), z=z,
                alpha=np.where(z > 0, 30.0, 1.0), pout=np.zeros((C, n)),
                theta=np.full(C, 0.05), nu=np.full(C, 4.0))


@pytest.mark.parametrize("flagged", list(FLAGGED))
@pytest.mark.parametrize("ncls", [1, 2, 8])
def test_low_rank_gram_classes_and_edges(ncls, flagged):
    st0 = _start(ncls, FLAGGED[flagged], 4)
    got, counts = [], []
    for mfma in (False, True):
        ns = _sampler(ncls)
        ns.set_debug(mfma_gram=mfma)
        ns.set_state(**st0)
        got.append(ns.eval_lnlike())
        ns.gram_counts(reset=True)
        ns.sweep(1, seed=3, mask=_abi.STAGE_GRAM)
        counts.append(ns.gram_counts(reset=True))
        ns.close()
    low = len(FLAGGED[flagged]) <= LR_MAX
    assert counts[1] == {"low_rank": 0, "mfma": C, "large_mfma": 0}, counts[1]
    assert counts[0] == {"low_rank": C if low else 0, "mfma": 0 if low else C,
                         "large_mfma": 0}, counts[0]
    assert np.all(np.isfinite(got[1][1]))
    np.testing.assert_array_equal(got[0][0], got[1][0])
    r = rel(got[0][1], got[1][1])
    print(f"ncls {ncls} {flagged}: max relative difference {r.max():.3e}")
    if low:
        assert np.all(r <= 1e-11), r.max()
    else:
        np.testing.assert_array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("ncls", [1, 2, 8])
def test_low_rank_launch_equals_single_sweep_launches(ncls):
    S, seed, sweep0 = 20, 11, 5
    st0 = _start(ncls, FLAGGED["lr_max"], 21)
    ns = _sampler(ncls)
    ns.set_state(**st0)
    rec = ns.alloc_records(S)
    ns.gram_counts(reset=True)
    ns.sweep(S, records=rec, seed=seed, sweep0=sweep0)
    counts = ns.gram_counts(reset=True)
    long_state = {k: v.clone() for k, v in ns.state.items()}
    ns.close()
    # at least one Gram per chain-sweep (a b draw redone at the noise floor computes another),
    # and the low-rank path took part
    assert counts["low_rank"] >= C and counts["low_rank"] + counts["mfma"] >= C * S, counts

    ns = _sampler(ncls)
    ns.set_state(**st0)
    bad = single_sweep_differences(ns, rec, long_state, S, seed, sweep0)
    assert not bad, f"first difference (sweep, array) {bad[:4]}"
