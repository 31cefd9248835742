"""Sim.halos (sx_sim_halos) on one rank: the Evrard sphere under VE with self-gravity behind a density cut, and a Plummer
sphere under the gravity-only propagator without one, each against tests/halo_ref.py on the columns Sim.get copies, with
the sim's G; the call changes no field and no scalar, its buffers are counted once, and the gravity-only layout refuses
what it cannot serve.  The refusal of a communicator with more than one rank is not tested here: one process holds one
rank."""
import numpy as np
import pytest

import fof_ref as fr
import halo_ref as hr
import sphexa_amd as sx
from sphexa_amd import ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def compare(sim, got, box, length, min_members, rho_min=0.0, thermal=False, columns=()):
    names = ["x", "y", "z", "m", "h", "vx", "vy", "vz", "id"] + list(columns)
    cols = sim.get(names)
    lim, bnd = box
    p = sim.params
    cv = float(np.float32(np.float64(np.float32(8.317e7) / np.float32(p.muiConst)) / (p.gamma - 1.0))) if thermal else None
    ref = hr.halo(cols, lim, bnd, length, ids=cols["id"], min_members=min_members, rho_min=rho_min, G=p.g, cv=cv)
    fr.assert_same(got, ref, box)
    about = hr.halo(cols, lim, bnd, length, ids=cols["id"], min_members=min_members, rho_min=rho_min, cv=cv, about=got,
                    potential=False)
    about["epot"] = ref["epot"]
    hr.assert_properties(got, about, thermal=thermal)
    stats = sim.halos_stats()
    assert stats["pair_terms"] == ref["pair_terms"] and stats["with_epot"] == len(ref["count"])
    return ref, cols


def test_evrard_clumps_above_a_density(ctx):
    f, lim, bnd, dt0 = ic.evrard(30)
    box = (lim, bnd)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), params=sx.default_params(g=1.0, theta=0.5))
    try:
        sim.set_state(f, dt0, dt0)
        for _ in range(3):
            sim.step()
        names = sim.allocated_fields()
        before, mem0, sc0 = sim.get(names), sim.memory(), sim.scalars()
        rho_min, length = 1.0 / (2.0 * np.pi * 0.3), 0.05  # the sphere's density at r = 0.3
        got = sim.halos(length=length, min_members=20, rho_min=rho_min, flags=("moments", "thermal", "potential"),
                        labels=True)
        mem1 = sim.memory()
        after = sim.get(names)
        assert all(before[k].tobytes() == after[k].tobytes() for k in names) and sim.scalars() == sc0
        assert mem1["device"] > mem0["device"] and mem1["pinned"] > mem0["pinned"]  # fof.* and halo.*, counted
        ref, cols = compare(sim, got, box, length, 20, rho_min, thermal=True, columns=("kx", "xm", "temp"))
        assert got["count"][0] > 256 and got["num_all"] >= 2
        unselected = got["label"] == hr.NONE
        assert 0.5 * len(unselected) < unselected.sum() < len(unselected)
        assert np.array_equal(unselected, ~ref["selected"])
        again = sim.halos(length=length, min_members=20, rho_min=rho_min, flags=("moments", "thermal", "potential"),
                          labels=True)
        assert sim.memory() == mem1, "the buffers are allocated by the first call"
        for k in ("label", "count", "mass", "com", "vel", "sigma", "shape", "angmom", "rmax", "eint", "epot", "ekin",
                  "alpha_vir", "bound", "axes"):
            assert np.array_equal(got[k], again[k]), k
        # the search alone shares its buffers with Sim.fof
        assert np.array_equal(sim.fof(length=length, min_members=20)["count"],
                              sim.halos(length=length, min_members=20, flags=())["count"])
        assert sim.memory() == mem1
    finally:
        sim.close()


def test_plummer_under_the_gravity_only_propagator(ctx):
    n = 1 << 14
    f, lim, bnd, dt0 = ic.plummer(n)
    box = (lim, bnd)
    sim = sx.Sim(ctx, n, sx.make_box(lim, bnd), sx.default_params(g=1.0, theta=0.5, nbody=True))
    try:
        sim.set_state(f, dt0, dt0)
        sim.step()
        names = sim.allocated_fields()
        before, sc0 = sim.get(names), sim.scalars()
        spec = sim.halos_spec(0.2, None, 20, 4096)
        assert spec.linking == sim.fof_spec(0.2).linking and spec.G == 1.0 and spec.std == 0
        got = sim.halos(spec=spec, labels=True)
        after = sim.get(names)
        assert all(before[k].tobytes() == after[k].tobytes() for k in names) and sim.scalars() == sc0
        ref, _ = compare(sim, got, box, spec.linking, 20)
        assert got["count"][0] > 8192, "the core is one group of many tiles"
        assert got["eint"] is None and bool(got["bound"][0]) and 0.3 < got["alpha_vir"][0] < 3.0
        with pytest.raises(sx.SxError, match="the thermal energy needs temp, which this layout does not keep"):
            sim.halos(spec=sim.halos_spec(flags=("thermal",)))
        with pytest.raises(sx.SxError, match="the density cut needs kx, xm and m, which this layout does not keep"):
            sim.halos(rho_min=1.0)
    finally:
        sim.close()
