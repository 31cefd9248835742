"""Stage and kernel times of sx_sim_step under all four propagators (sx_step_timer.hpp).

Every propagator reports the same ten stage names and seven kernel names (the gravity-only one adds nbodyIntegrate), in
the same order; what a propagator does not mark in a step reads exactly 0.0, and what it marks is the interval between
events recorded in that step -- never one left over from an earlier step.
"""
import math

import numpy as np
import pytest

import gpu_util as gutil
import nbody_ref as nr
import pyoracle as po
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

STAGES = ["sync", "FindNeighbors", "XMass", "VeDefGradh", "EOS", "IadDivvCurlv", "AVswitches", "MomentumEnergy",
          "Gravity", "UpdateQuantities"]
KERNELS = ["findNeighbors", "xmass", "veDefGradh", "iadDivvCurlv", "avSwitches", "momentumEnergy", "gravity"]
STEPS = 2


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def sedov_sim(ctx, **params):
    """Sedov side 10 under the propagator of params, skin lists off: every step syncs and searches"""
    st, obox = po.sedov_state(10)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox), params=sx.default_params(**params))
    if not params.get("bdt"):
        sim.set_skin(0.0)
    sim.set_state(st.arrays, st.minDt, st.minDt_m1)
    return sim, st


def evrard_sim(ctx):
    """the Evrard(10) setup of test_gpu_nbody.py"""
    st, obox = po.evrard_state(10)
    arr = {k: st.arrays[k].copy() for k in nr.FIELDS}
    arr["id"] = np.arange(st.n, dtype=np.uint64)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox), params=sx.default_params(g=1.0, theta=0.5), propagator=3)
    sim.set_state(arr, st.minDt, st.minDt)
    return sim


def times(sim, kernels=KERNELS):
    """one step; its (stage times, kernel times) after the checks every propagator shares"""
    sim.step()
    st, kt = sim.stage_times(), sim.kernel_times()
    print(st, kt)
    assert list(st) == STAGES
    assert list(kt) == kernels
    for name, ms in list(st.items()) + list(kt.items()):
        assert math.isfinite(ms) and ms >= 0.0, (name, ms)
    return st, kt


def test_ve(ctx):
    sim, _ = sedov_sim(ctx)
    try:
        for _ in range(STEPS):
            st, kt = times(sim)
            for name in ("sync", "FindNeighbors", "IadDivvCurlv", "MomentumEnergy", "UpdateQuantities"):
                assert st[name] > 0.0, (name, st)
            for name in ("findNeighbors", "iadDivvCurlv", "momentumEnergy"):
                assert kt[name] > 0.0, (name, kt)
            # g = 0: the marks stand around a gravity stage that is not run
            assert st["Gravity"] < 0.05 and kt["gravity"] < 0.05, (st, kt)
    finally:
        sim.close()


def test_std(ctx):
    sim, _ = sedov_sim(ctx, std=True)
    try:
        for _ in range(STEPS):
            st, kt = times(sim)
            for name in ("XMass", "VeDefGradh", "IadDivvCurlv", "MomentumEnergy"):
                assert st[name] > 0.0, (name, st)
            assert st["EOS"] == 0.0 and st["AVswitches"] == 0.0, st
            assert kt["veDefGradh"] == 0.0 and kt["avSwitches"] == 0.0, kt
    finally:
        sim.close()


def test_ve_bdt(ctx):
    sim, _ = sedov_sim(ctx, bdt=True)
    try:
        for _ in range(STEPS):
            st, kt = times(sim)
            assert all(ms == 0.0 for ms in kt.values()), kt
            assert st["sync"] > 0.0 and st["UpdateQuantities"] > 0.0, st
    finally:
        sim.close()


def test_nbody(ctx):
    sim = evrard_sim(ctx)
    try:
        for _ in range(STEPS):
            st, kt = times(sim, KERNELS + ["nbodyIntegrate"])
            assert all(st[name] == 0.0 for name in STAGES[1:8]), st  # stages 2-8: the hydro stages
            assert all(kt[name] == 0.0 for name in KERNELS[:6]), kt  # every hydro kernel
            for name in ("Gravity", "UpdateQuantities"):
                assert st[name] > 0.0, (name, st)
            for name in ("gravity", "nbodyIntegrate"):
                assert kt[name] > 0.0, (name, kt)
    finally:
        sim.close()


def test_times_after_a_state_change(ctx):
    """set_state on a VE sim that has stepped: the next step's times come from that step's events alone"""
    sim, st0 = sedov_sim(ctx)
    try:
        for _ in range(STEPS):
            times(sim)
        sim.set_state(st0.arrays, st0.minDt, st0.minDt_m1)
        times(sim)
    finally:
        sim.close()
