"""Load the fixtures of the models with several power-law processes (red noise + DM
(+ chromatic), ``PTA(dm_gp=, chrom_gp=)``): ``tests/golden/mgp_<ds>_dataset.npz``,
``mgp_ref_<ds>_beta_{fixed,prior}.npz`` and ``mgp_samestart_<ds>_beta.npz``, made by
tools/gen_golden.py ``multi_gp`` and tools/same_start_ref.py.  They do not match
``ref_*.npz``: golden_io's loader cannot build their models."""
from __future__ import annotations

import ast
import os

import numpy as np

from gibbs_student_t_amd.model import PTA

from golden_io import GOLDEN

# dataset -> (Fourier columns of each process, ECORR columns, the path it is expected on)
DATASETS = {
    "dmg": ((14, 10), 0, "persistent"),
    "dme": ((10, 10), 24, "persistent"),
    "dmw": ((60, 40), 0, "large"),
    "dm3": ((60, 50, 20), 0, "large"),
    "dmx": ((20, 20), 60, "large"),
}
KINDS = ("fixed", "prior")
NAMES = [f"{ds}_beta_{kind}" for ds in DATASETS for kind in KINDS]


def load_dataset(dataset):
    d = np.load(os.path.join(GOLDEN, f"mgp_{dataset}_dataset.npz"), allow_pickle=False)
    name = str(d["names"][0]).split("_")[0]
    comps = dict(zip((str(v) for v in d["proc_names"]), (int(v) for v in d["proc_components"])))
    kw = {k: dict(components=comps[k]) for k in ("dm_gp", "chrom_gp") if k in comps}
    if "backends" in d.files:
        kw.update(backends=d["backends"], selection=str(d["selection"]),
                  n_ecorr=int(d["n_ecorr"]), ecorr_backend=d["ecorr_backend"],
                  log10_ecorr=tuple(d["log10_ecorr"]) or None)
        efac = (0.2, 10.0) if int(d["efac_varied"]) else 1.0
    else:
        efac = 1.0
    pta = PTA.from_arrays(name, d["residuals"], d["toaerrs"], d["T"], d["Ffreqs"],
                          int(d["components"]), float(d["tm_weight"]), efac=efac, **kw)
    assert pta.param_names == [str(v) for v in d["names"]]
    return pta


def load_ref(name):
    """``name``: ``<ds>_beta_<fixed|prior>``; the dict golden_io.load_ref returns."""
    d = dict(np.load(os.path.join(GOLDEN, f"mgp_ref_{name}.npz"), allow_pickle=False))
    d["kw"] = ast.literal_eval(str(d.pop("model_kw")))
    d["tape"] = {k[5:]: v for k, v in d.items() if k.startswith("tape_")}
    d["pta"] = load_dataset(name.split("_")[0])
    return d


def load_samestart(dataset):
    return np.load(os.path.join(GOLDEN, f"mgp_samestart_{dataset}_beta.npz"), allow_pickle=False)
