"""Sim.spectrum (sx_sim_spectrum) on one rank: it is Context.spectrum of the sim's own fields, bit for bit, under every
propagator; scalar fields a layout does not keep are refused with a reason; nothing is allocated before the first call;
a stirred box gives a finite spectrum."""
import numpy as np
import pytest

import gpu_util as gutil
import nbody_ref as nr
import pyoracle as po
import sphexa_amd as sx
from sphexa_amd import ic

pytestmark = pytest.mark.gpu

SEDOV_BOX = ([-0.5, 0.5] * 3, [1, 1, 1])
N = 16


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def seam(ctx, sim, kind, weight=None, field=None, dtype=np.float32):
    f, _ = sim.fields()
    a = [sx.DeviceArray(ctx, getattr(f, field), int(f.n), dtype)] if field else None
    return ctx.spectrum(f, sim.box, sx.SxSpectrum(kind, weight, N), a=a, K=sim.params.K)


def compare(ctx, sim, scalar_fields):
    ns = sx.spectrum_num_shells(N)
    for weight in (None, "energy", "third"):
        k, power, modes = sim.spectrum(N, "velocity", weight)
        p, m = seam(ctx, sim, "velocity", weight)
        assert np.array_equal(power, p) and np.array_equal(modes, m) and power.shape == (ns,)
        assert np.array_equal(modes, sx.spectrum_modes(N)) and np.isfinite(power).all()
        assert np.array_equal(k, 2.0 * np.pi * np.arange(ns) / (sim.box.lim[1] - sim.box.lim[0]))
    assert sim.spectrum_stats() == ctx.spectrum_stats() and sim.spectrum_stats()["pairs"] > 0
    for name, dtype in [(None, None)] + scalar_fields:
        _, power, _ = sim.spectrum(N, "scalar", field=name)
        p, _ = seam(ctx, sim, "scalar", field=name, dtype=dtype)
        assert np.array_equal(power, p) and power[0] > 0, name


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_hydro_propagators_equal_the_seam(ctx, std):
    sim = sx.Sim(ctx, 1000 + 64, sx.make_box(*SEDOV_BOX), params=sx.default_params(std=std))
    try:
        sim.init_sedov(10)
        sim.step()
        sim.step()
        compare(ctx, sim, [("temp", np.float64), ("c", np.float32), ("h", np.float32)] +
                ([("p", np.float32)] if std else [("divv", np.float32)]))
        # the mesh density of the unit-mass unit box: its mean, mode 0, is 1
        _, power, _ = sim.spectrum(N, "scalar")
        assert abs(power[0] - 1.0) < 1e-2
        if not std:
            with pytest.raises(sx.SxError, match="the field p is not kept"):
                sim.spectrum(N, "scalar", field="p")
        with pytest.raises(sx.SxError, match="SX_SPEC_SCALAR takes weight 0 only"):
            sim.spectrum(N, "scalar", weight="energy")
        with pytest.raises(sx.SxError, match="n must be 16, 32, 64, 128 or 256"):
            sim.spectrum(48)
        with pytest.raises(ValueError):
            sim.spectrum(N, "scalar", field="rho")
    finally:
        sim.close()


def test_ve_bdt_between_substeps(ctx):
    st, obox = po.sedov_state(10)
    sim = sx.Sim(ctx, st.n + 64, sx.make_box(list(obox.lim), list(obox.bnd)), params=sx.default_params(bdt=True))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt)
        for _ in range(3):
            sim.step()
            compare(ctx, sim, [("temp", np.float64)])
    finally:
        sim.close()


def test_gravity_only_propagator(ctx):
    st, obox = po.pbc_wave_state(10)
    arr = {k: st.arrays[k].copy() for k in nr.FIELDS}
    sim = sx.Sim(ctx, len(arr["x"]), gutil.box_to_sx(obox), params=sx.default_params(g=1.0), propagator=3)
    try:
        sim.set_state(arr, st.minDt, st.minDt)
        sim.step()
        compare(ctx, sim, [("vx", np.float32), ("h", np.float32)])
        for name in ("temp", "c", "p", "divv", "curlv", "alpha"):
            with pytest.raises(sx.SxError, match=f"the field {name} is not kept by the gravity-only propagator"):
                sim.spectrum(N, "scalar", field=name)
    finally:
        sim.close()


def test_memory_grows_only_with_the_first_call():
    ctx = sx.Context(0)  # its own context: the module's has made its tables already, a sim's are its own anyway
    sim = sx.Sim(ctx, 1000 + 64, sx.make_box(*SEDOV_BOX))
    try:
        sim.init_sedov(10)
        sim.step()
        before = sim.memory()
        sim.spectrum(N, "velocity", "energy")
        after = sim.memory()
        # four sums, one complex mesh and the permutation came with the first call
        assert after["device"] >= before["device"] + (6 * 8 + 4) * N ** 3 and after["pinned"] > before["pinned"]
        sim.spectrum(N, "velocity", "energy")
        sim.spectrum(N, "scalar", field="temp")
        assert sim.memory() == after
    finally:
        sim.close()
        ctx.close()


def test_stirred_box(ctx):
    f, lim, bnd, dt0 = ic.turbulence(16, 1.0)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params()))
    try:
        sim.set_state(f, dt0, dt0)
        sim.set_turbulence(Lbox=1.0)
        for _ in range(4):
            sim.step()
        k, mean, modes = sim.spectrum(N, "velocity")
        _, energy, _ = sim.spectrum(N, "velocity", "energy")
        assert np.isfinite(mean).all() and np.isfinite(energy).all() and mean[1:].sum() > 0
        # the forcing has no mean (stirring starts from rest and the modes exclude k = 0): the box stays in its rest frame,
        # so the mean over the cells of the mass-weighted velocity, shell 0, is small against the stirred modes: below a
        # hundredth of their amplitude, 1e-4 of the power (the cells weigh the particles by volume, not by mass, so it
        # is the momentum only to the evenness of the density)
        print("shell 0 holds %.2e of the power" % (mean[0] / mean.sum()))
        assert mean[0] <= 1e-4 * mean.sum(), (mean[0], mean.sum())
        # Parseval: the kinetic energy per unit volume on the mesh is what the particles carry, to the mesh's resolution
        g = sim.get(["m", "vx", "vy", "vz"])
        ekin = 0.5 * float((g["m"].astype(np.float64) * (g["vx"].astype(np.float64) ** 2 + g["vy"].astype(np.float64) ** 2
                                                            + g["vz"].astype(np.float64) ** 2)).sum())
        assert 0.5 * ekin < energy.sum() < 1.5 * ekin
    finally:
        sim.close()
