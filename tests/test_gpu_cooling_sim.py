"""Radiative cooling inside the step (Sim.set_cooling): gas at rest follows the exact cooling curve under VE and std, the
energy radiated is the internal energy lost, the cooling-time criterion limits the time-step, a sim whose cooling is off
steps as one that never cooled, a cooling Sedov blast stays finite and above the floor, ve-bdt and the gravity-only
propagator refuse, and a checkpoint continues bit by bit.

Tolerances are the kernel test's (test_gpu_cooling.py): 16 eps_ref T_old per application, eps_ref measured against
mpmath on the shared inputs."""
import math

import numpy as np
import pytest

import cooling_ref as cr
import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx
from sphexa_amd import cooling, ic

pytestmark = pytest.mark.gpu

MARGIN = 16.0
SIDE = 16
FIELDS = {False: ["id", "temp", "m", "kx", "xm"], True: ["id", "temp", "m", "rho"]}


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def eps():
    return max(cr.gpu_reference(0)["eps_ref"], cr.eps_floor())


def lattice():
    return ic.turbulence(SIDE)


def lattice_params(std):
    return ic.turbulence_params(sx.default_params(std=std))


def lattice_cv():
    return float(ic.ideal_gas_cv(np.float32(ic.TURBULENCE_CONSTANTS["muiConst"]), ic.TURBULENCE_CONSTANTS["gamma"]))


def lattice_table(strength):
    """the gas starts on the fourth node; t_cool = u0 / (rho L) = 1000 / strength there"""
    f = lattice()[0]
    return cooling.Cooling(*cr.scaled_table(f["temp"][0], strength))


def lattice_sim(ctx, std, table=None, ct_crit=0.0):
    f, lim, bnd, dt0 = lattice()
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), lattice_params(std))
    sim.set_state(f, dt0, dt0)
    if table is not None:
        sim.set_cooling(table, ct_crit=ct_crit)
    return sim


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_gas_at_rest_follows_the_cooling_curve(ctx, eps, std):
    """six steps without the limiter next to an uncooled twin.  The oracle is applied step by step, with each step's dt
    and the rho the sim had in that step, and the end is held to 6 x the kernel tolerance plus the twin's own drift of
    temp.  One application with the summed dt is asserted too, as a bracket: with the last step's rho alone it misses
    by 7e-7 T_0 on the MI355X, and not through the cooling -- the h iteration moves h from step to step and rho, a
    float sum over the neighbours, with it, by some 1e-6, while the twin's temp drifts by 3e-14 T_0 only -- so the end
    is held between the applications with each particle's largest and smallest rho of the six steps."""
    table = lattice_table(4e5)
    tab = cr.Table(*cr.scaled_table(lattice()[0]["temp"][0], 4e5))
    cooled, twin = lattice_sim(ctx, std, table, ct_crit=0.0), lattice_sim(ctx, std)
    try:
        start = cr.by_id(cooled.get(["id", "temp", "m"]))
        eint0 = cooled.conserved()["eint"]
        cv = lattice_cv()
        total_dt, radiated, want = 0.0, [], start["temp"]
        rho_min = rho_max = None
        for _ in range(6):
            cooled.step()
            twin.step()
            dt = cooled.scalars()["minDt"]
            assert dt == twin.scalars()["minDt"]  # no limiter: the twin's steps
            total_dt += dt
            stats = cooled.cooling_stats()
            assert stats["minDtCool"] == math.inf
            radiated.append(stats["radiated"])
            assert stats["radiated_total"] == pytest.approx(math.fsum(radiated), rel=1e-14)
            # the oracle with this step's dt and the sim's own rho of this step
            end = cr.by_id(cooled.get(FIELDS[std]))
            rho = cr.sim_rho(end, std)
            want = cr.integrate64(tab, want, (rho.astype(np.float64) * dt) / cv)
            rho_min = rho if rho_min is None else np.minimum(rho_min, rho)
            rho_max = rho if rho_max is None else np.maximum(rho_max, rho)
        end_twin = cr.by_id(twin.get(["id", "temp"]))
        eint6 = cooled.conserved()["eint"]
        # hydrodynamic rounding drift is not cooling's to answer for: the twin's own, measured here
        drift = np.max(np.abs(end_twin["temp"] - start["temp"]))
        allow = 6 * MARGIN * eps * start["temp"] + drift
        err = np.abs(end["temp"] - want)
        print("std" if std else "ve", "cooled to %.4f of T_0; max error %.3e, allowance %.3e (twin drift %.3e)"
              % (np.mean(end["temp"] / start["temp"]), err.max(), allow.min(), drift))
        assert np.all(end["temp"] < 0.9 * start["temp"])  # it did cool
        assert np.all(err <= allow)
        # one application with the summed dt (the semigroup through the sim).  The h iteration moves h, and with it
        # rho, by some 1e-6 from step to step; Y_new = Y_old + (L_N / T_N) sum_k rho_k dt_k / cv, and T falls as that sum
        # grows, so the end lies between one application with each particle's largest rho of the six steps and one
        # with its smallest, to the same allowance
        once_hi = cr.integrate64(tab, start["temp"], (rho_max.astype(np.float64) * total_dt) / cv)
        once_lo = cr.integrate64(tab, start["temp"], (rho_min.astype(np.float64) * total_dt) / cv)
        print("   one application with the summed dt: rho moves by up to %.3e of itself over the steps, the bracket is "
              "%.3e T_0 wide, the end leaves it by %.3e T_0 at most"
              % (np.max((rho_max - rho_min) / rho_min), np.max((once_lo - once_hi) / start["temp"]),
                 max(np.max((once_hi - end["temp"]) / start["temp"]), np.max((end["temp"] - once_lo) / start["temp"]), 0.0)))
        assert np.all(end["temp"] >= once_hi - allow) and np.all(end["temp"] <= once_lo + allow)
        # eint_0 - eint_6 is the radiated total: the same allowance summed over the particles
        allow_e = math.fsum(start["m"].astype(np.float64) * cv * allow)
        lost = eint0 - eint6
        print("   eint lost %.12g, radiated %.12g, difference %.3e, allowance %.3e"
              % (lost, stats["radiated_total"], lost - stats["radiated_total"], allow_e))
        assert lost > 0.05 * eint0
        assert abs(lost - stats["radiated_total"]) <= allow_e
    finally:
        cooled.close(), twin.close(), table.close()


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_cooling_time_limits_the_step(ctx, eps, std):
    ct_crit = 0.1
    table = lattice_table(6e5)
    tab = cr.Table(*cr.scaled_table(lattice()[0]["temp"][0], 6e5))
    sim = lattice_sim(ctx, std, table, ct_crit=ct_crit)
    cv = lattice_cv()
    try:
        bound = 0
        for step in range(8):
            before = cr.by_id(sim.get(["id", "temp"]))
            dt_before = sim.scalars()["minDt"]
            sim.step()
            after = cr.by_id(sim.get(FIELDS[std]))
            want = ct_crit * cr.cooling_time64(tab, before["temp"], cr.sim_rho(after, std), cv).min()
            got, dt = sim.cooling_stats()["minDtCool"], sim.scalars()["minDt"]
            print("step %d: minDtCool %.6e (oracle %.6e), minDt %.6e" % (step, got, want, dt))
            assert abs(got - want) <= MARGIN * eps * want
            assert dt <= got
            sc = sim.scalars()
            if got < min(1.1 * dt_before, sc["minDtCourant"], sc["minDtRho"]):
                bound += 1  # the smallest candidate (no gravity: no acceleration criterion)
                assert dt == got
        assert bound >= 1
    finally:
        sim.close(), table.close()


def sedov_sim(ctx, side):
    st, obox = po.sedov_state(side)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox))
    sim.set_state(st.arrays, st.minDt, st.minDt_m1)
    return sim, st


def sedov_table():
    """nodes at u = 0.2 .. 1000: the blast's core (u up to 180) cools in some 1e-4, its skirt reaches the floor within
    the ten steps, and the background (u = 1e-8) is below the floor"""
    cv = float(po.ideal_gas_cv())
    return cooling.Cooling(*cr.scaled_table(50.0 * 0.2 / cv, 3e5))


def test_off_is_off(ctx):
    """never given a table; set and taken away again; told None without ever having had one"""
    table = sedov_table()
    sims = [sedov_sim(ctx, 10)[0] for _ in range(3)]
    try:
        sims[1].set_cooling(table, ct_crit=0.1)
        sims[1].set_cooling(None)
        sims[2].set_cooling(None)
        for _ in range(3):
            for s in sims:
                s.step()
        base = cr.by_id(sims[0].get(sx.Sim.CONSERVED))
        for s in sims[1:]:
            other = cr.by_id(s.get(sx.Sim.CONSERVED))
            for k in sx.Sim.CONSERVED:
                assert np.array_equal(base[k], other[k]), k
            assert s.scalars() == sims[0].scalars()
            with pytest.raises(sx.SxError, match="sx_sim_set_cooling was not called"):
                s.cooling_stats()
    finally:
        for s in sims:
            s.close()
        table.close()


def test_sedov_with_cooling(ctx):
    table = sedov_table()
    floor = table.table()["T"][0]
    sim, st = sedov_sim(ctx, 12)
    try:
        sim.set_cooling(table, ct_crit=0.1)
        start = cr.by_id({"id": st.arrays["id"], "temp": st.arrays["temp"]})
        above = start["temp"] >= floor
        assert 0 < above.sum() < above.size
        totals = [0.0]
        for _ in range(10):
            sim.step()
            got = cr.by_id(sim.get(sx.Sim.CONSERVED + ["du", "ax", "ay", "az"]))
            for k, v in got.items():
                assert np.all(np.isfinite(v.astype(np.float64))), k
            assert np.all(got["temp"][above] >= floor)
            stats = sim.cooling_stats()
            assert stats["radiated"] >= 0.0 and math.isfinite(stats["minDtCool"])
            assert sim.scalars()["minDt"] <= stats["minDtCool"]
            totals.append(stats["radiated_total"])
        assert np.all(np.diff(totals) >= 0.0) and totals[-1] > 0.0
        times = sim.cooling_times()
        assert times["coolingTime"] > 0.0 and times["cool"] > 0.0
    finally:
        sim.close(), table.close()


@pytest.mark.parametrize("kw, reason", [
    (dict(bdt=True), r"sx_sim_set_cooling: cooling with block time-steps \(ve-bdt\) is not supported by sx_sim"),
    (dict(nbody=True, g=1.0), r"sx_sim_set_cooling: the gravity-only propagator does not cool"),
])
def test_refusals(ctx, kw, reason):
    table = sedov_table()
    sim = sx.Sim(ctx, 1000, sx.make_box([-0.5, 0.5] * 3, [0, 0, 0]), sx.default_params(**kw))
    try:
        with pytest.raises(sx.SxError, match=reason):
            sim.set_cooling(table)
        sim.set_cooling(None)  # switching off is always accepted
    finally:
        sim.close(), table.close()


def test_checkpoint(ctx, tmp_path):
    table = lattice_table(4e5)
    sim = lattice_sim(ctx, False, table, ct_crit=0.1)
    new = None
    try:
        for _ in range(4):
            sim.step()
        path = str(tmp_path / "cooling.npz")
        sim.save_checkpoint(path)
        with np.load(path) as d:
            assert np.array_equal(d["cooling::T"], table.table()["T"])
            assert np.array_equal(d["cooling::lambda"], table.table()["lam"])
            assert float(d["cooling::ct_crit"]) == 0.1
            assert float(d["cooling::erad"]) == sim.cooling_stats()["radiated_total"] > 0.0
        f, lim, bnd, _ = lattice()
        plain = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), lattice_params(False))
        try:
            with pytest.raises(ValueError, match="cooling table"):
                plain.load_checkpoint(path)
        finally:
            plain.close()
        new = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), lattice_params(False))
        # another limiter, another curve: the file's account of the energy radiated is not continued under them
        other = lattice_table(5e5)
        try:
            for tab_, crit in ((table, 0.2), (other, 0.1)):
                new.set_cooling(tab_, ct_crit=crit)
                with pytest.raises(ValueError, match="differ from those of this Sim's set_cooling"):
                    new.load_checkpoint(path)
        finally:
            other.close()
        new.set_cooling(table, ct_crit=0.1)
        new.load_checkpoint(path)
        assert new.cooling_stats()["radiated_total"] == sim.cooling_stats()["radiated_total"]
        for _ in range(2):
            sim.step()
            new.step()
        a, b = cr.by_id(sim.get(["id", "temp"])), cr.by_id(new.get(["id", "temp"]))
        assert np.array_equal(a["temp"], b["temp"])
        assert new.cooling_stats()["radiated_total"] == sim.cooling_stats()["radiated_total"]
        assert new.scalars()["minDt"] == sim.scalars()["minDt"]
    finally:
        sim.close(), table.close()
        if new is not None:
            new.close()
