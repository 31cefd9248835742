"""Writes tests/golden/nbody_evrard14.npz: 20 NbodyProp steps of po.evrard_state(14) (G = 1, theta = 0.5) composed by
tests/nbody_ref.py from the reference's own functions (oracle/_ref): the per-step dt, ttot, egrav, max|a|^2 and
whether the 1.1 minDt limiter set dt, and the final state.  Needs oracle/_ref; tests/test_nbody_ref.py checks that
the committed file equals a fresh composition.

  python tests/gen_nbody_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import nbody_ref as nr  # noqa: E402
import pyoracle as po  # noqa: E402

SIDE, STEPS, THETA = 14, 20, 0.5
PATH = os.path.join(HERE, "golden", "nbody_evrard14.npz")


def compose(lib):
    st, box = po.evrard_state(SIDE)
    series = nr.run(lib, st, box, lib.params(g=1.0, theta=THETA), STEPS)
    out = {"series_" + k: v for k, v in series.items()}
    out.update({"final_" + k: st.arrays[k].copy() for k in nr.FIELDS})
    ekin, etot = nr.energies(st)
    out["final_scalars"] = np.array([st.minDt, st.minDt_m1, st.ttot, st.egrav, ekin, etot])
    return out


if __name__ == "__main__":
    ref = po.load_ref()
    if ref is None:
        sys.exit("oracle/_ref is not built")
    np.savez_compressed(PATH, **compose(ref))
    print(PATH, os.path.getsize(PATH), "bytes")
