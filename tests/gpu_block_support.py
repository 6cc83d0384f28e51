"""The launches the tests of gst_set_accum_block share: gpu_support's accumulator scaffold with
a block.  Importing this module is the device gate (through gpu_support)."""
from __future__ import annotations

import functools

import numpy as np

from block_support import packed_outer_reference
from gpu_support import (ACCUM_SEED, ACCUM_SWEEP0, accum_alloc, accum_sampler)
from gibbs_student_t_amd.native import ACCUM_KEYS

BLOCK_KEYS = ACCUM_KEYS + ("b_outer",)
REC_KEYS = ("b", "z", "alpha", "pout")


def block_alloc(ns, n_of, block, keys=BLOCK_KEYS):
    """accum_alloc's sums (sentinels where no TOA is) plus the zeroed block buffer"""
    acc = accum_alloc(ns, n_of, tuple(k for k in keys if k != "b_outer"))
    if "b_outer" in keys:
        acc.update(ns.alloc_accum(("b_outer",), b_block=block))
    return acc


def block_run(name, per, block, *, launches=3, S=8, path="auto", waves=None, every=1, burn=5):
    """gpu_support.accum_run with the block second moment: ``launches`` launches of S sweeps of
    ``per`` chains of the fixture ``name``, sums from sweep ``burn`` on; ``block`` None: the
    same run without a block.  A dict: records, sums, final state."""
    ns, refs, ds_of = accum_sampler([name], per, path, waves)
    n_of = np.array([refs[d]["pta"].n for d in ds_of])
    acc = block_alloc(ns, n_of, block, BLOCK_KEYS if block is not None else ACCUM_KEYS)
    ns.set_accum(acc, from_sweep=ACCUM_SWEEP0 + burn, b_block=block)
    recs = []
    for i in range(launches):
        rec = ns.alloc_records((S + every - 1) // every, REC_KEYS)
        ns.sweep(S, records=rec, record_every=every, seed=ACCUM_SEED, sweep0=ACCUM_SWEEP0 + i * S)
        recs.append({k: v.cpu().numpy() for k, v in rec.items()})
    state = ns.get_state()
    sums = {k: v.cpu().numpy() for k, v in acc.items()}
    out = dict(rec={k: np.concatenate([r[k] for r in recs], axis=1) for k in REC_KEYS},
               sums=sums, state=state, n_of=n_of, m=ns.m, path=ns.path)
    ns.close()
    return out


# one run per configuration, shared by the tests that read it (never written to)
cached_block_run = functools.lru_cache(maxsize=None)(
    lambda name, per, block, path, waves, every=1: block_run(name, per, block, path=path,
                                                             waves=waves, every=every))


def check_block_sums(b_rec, bb, block, burn, label=""):
    """The block sums against the long-double sum of the recorded b from record ``burn`` on:
    every element within (N + 2) 2^-52 sum_s |b_si b_sj|"""
    want, bound = packed_outer_reference(b_rec, block, burn)
    assert bb.shape == want.shape, (bb.shape, want.shape)
    err = np.abs(bb.astype(np.longdouble) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"{label} block {block}: N = {b_rec.shape[1] - burn}, worst err / bound "
          f"{float(ratio.max()):.3g}, elements {bb.shape[1]}")
    assert np.all(err <= bound), f"{label}: {int((err > bound).sum())} elements beyond the bound"
    assert np.any(bb != 0.0)
