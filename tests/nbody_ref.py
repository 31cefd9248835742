"""The NbodyProp step (main/src/propagator/nbody.hpp:115-163) composed from CPU pieces that are already pinned to the
reference (test infrastructure, no GPU):

* sync: pyoracle.Lib.sfc_keys, then every field sorted by key (stable, as Domain::sync);
* computeForces: ax = ay = az = 0, then Lib.gravity (upsweep + walk, pinned by tests/test_oracle_gravity.py);
* computeTimestep with minDtCourant = INFINITY (ts_global.hpp:47-67, 97-112) in numpy doubles, |a|^2 as
  x x + (y y + z z) of floats promoted to double, as the device's maxAccSqKernel forms it;
* computePositions: Lib.positions with du = du_m1 = 0, so temp stays inert; h is never updated.

`lib` is either library of pyoracle: the restatement (libsphexa_oracle.so) or the reference's own functions (oracle/_ref).
"""
import math

import numpy as np

import pyoracle as po

FIELDS = ["x", "y", "z", "h", "m", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "id"]


def host_state(arrays, minDt, minDt_m1, ttot=0.0):
    """a pyoracle.HostState from the conserved fields of the gravity-only propagator (a dict of arrays)"""
    st = po.HostState(len(arrays["x"]))
    for k in FIELDS:
        st.arrays[k][:] = arrays[k]
    st.minDt, st.minDt_m1, st.ttot = float(minDt), float(minDt_m1), float(ttot)
    return st


def max_acc_sq(st, first=0, last=None):
    s = slice(first, st.n if last is None else last)
    x, y, z = (st.arrays[k][s].astype(np.float64) for k in ("ax", "ay", "az"))
    return float(np.max(x * x + (y * y + z * z))) if x.size else 0.0


def timestep(params, max_a2, minDt):
    """(dt, limited): min(etaAcc sqrt(eps / sqrt(max|a|^2)), minDtRho = inf, maxDtIncrease minDt); limited: the
    increase limiter set it"""
    dt_acc = params.etaAcc * math.sqrt(params.eps / math.sqrt(max_a2)) if max_a2 > 0.0 else math.inf
    dt_inc = params.maxDtIncrease * minDt
    return min(dt_acc, math.inf, dt_inc), dt_inc <= dt_acc


def nbody_step(lib, st, box, params, bucket=64):
    """advance st (a HostState) by one NbodyProp step in place; returns the step's figures"""
    keys = lib.sfc_keys(st, box).copy()
    o = np.argsort(keys, kind="stable")
    for k in po.CONSERVED:
        st.arrays[k][:] = st.arrays[k][o]
    st.keys[:] = keys[o]
    for k in ("ax", "ay", "az"):
        st.arrays[k][:] = 0
    egrav, _, _ = lib.gravity(st, box, params, bucket=bucket)
    acc = {k: st.arrays[k].copy() for k in ("ax", "ay", "az")}
    a2 = max_acc_sq(st)
    dt, limited = timestep(params, a2, st.minDt)
    st.ttot += dt
    st.minDt_m1 = st.minDt
    st.minDt = dt
    st.minDtCourant = math.inf
    st.du[:] = 0
    st.du_m1[:] = 0
    lib.positions(st, box, params=params)
    st.egrav = egrav
    return dict(dt=dt, ttot=st.ttot, egrav=egrav, maxAccSq=a2, limited=limited, acc=acc)


def energies(st):
    """(kinetic, total = kinetic + egrav of the last step) of a state, as conserved_quantities.hpp with neither u nor
    temp (the internal energy is 0)"""
    m = st.m.astype(np.float64)
    v2 = sum(st.arrays[k].astype(np.float64) ** 2 for k in ("vx", "vy", "vz"))
    ekin = 0.5 * float(np.sum(m * v2))
    return ekin, ekin + st.egrav


def run(lib, st, box, params, steps):
    """`steps` steps from st (in place); the per-step series"""
    out = {k: [] for k in ("dt", "ttot", "egrav", "maxAccSq", "limited")}
    for _ in range(steps):
        r = nbody_step(lib, st, box, params)
        for k in out:
            out[k].append(r[k])
    return {k: np.array(v) for k, v in out.items()}
