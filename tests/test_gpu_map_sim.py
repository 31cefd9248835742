"""Sim.render (sx_sim_render) on one rank: it is Context.render_map of the sim's own fields, bit for bit, under every
propagator; fields a layout does not keep are refused with a reason; nothing is allocated before the first render."""
import numpy as np
import pytest

import pyoracle as po
import sphexa_amd as sx
from sphexa_amd import ic

pytestmark = pytest.mark.gpu

SEDOV_BOX = ([-0.5, 0.5] * 3, [1, 1, 1])


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sedov(ctx):
    sim = sx.Sim(ctx, 1000 + 64, sx.make_box(*SEDOV_BOX))
    sim.init_sedov(10)
    sim.step()
    sim.step()
    yield sim
    sim.close()


def seam(ctx, sim, spec, field=None, dtype=np.float32):
    f, _ = sim.fields()
    a = sx.DeviceArray(ctx, getattr(f, field), int(f.n), dtype) if field else None
    return ctx.render_map(f, sim.box, spec, a=a, K=sim.params.K)


def test_memory_grows_only_with_the_first_render(ctx):
    sim = sx.Sim(ctx, 1000 + 64, sx.make_box(*SEDOV_BOX))
    try:
        sim.init_sedov(10)
        created = sim.memory()
        sim.step()
        sim.step()
        before = sim.memory()
        assert before["device"] >= created["device"]
        s0, _ = sim.render("column", axis=2, npix=40)
        after = sim.memory()
        assert s0.shape == (40, 40) and (s0 > 0).all()
        # the two images and the pair scratch came with the first render, not at creation and not with a step
        assert after["device"] >= before["device"] + 2 * 40 * 40 * 8 and after["pinned"] > before["pinned"]
        sim.render("column", axis=2, npix=40)
        assert sim.memory() == after
    finally:
        sim.close()


@pytest.mark.parametrize("axis", [0, 2])
def test_column_density_and_temperature_equal_the_seam(ctx, sedov, axis):
    sim = sedov
    spec = sim.map_spec("column", axis=axis, npix=(40, 24))
    s0, mean = sim.render(spec=spec, field="temp")
    r0, r1 = seam(ctx, sim, spec, "temp", np.float64)
    assert np.array_equal(s0, r0) and np.array_equal(sim.last_sum1, r1)
    assert np.array_equal(mean, r1 / r0) and s0.shape == (24, 40)
    # the column density of the unit-mass box integrates to its mass
    assert abs(s0.sum() / (40 * 24) - 1.0) < 1e-5
    assert sim.map_stats() == ctx.map_stats() and sim.map_stats()["footprints"] == 1000
    n0, none = sim.render(spec=spec)
    assert none is None and np.array_equal(n0, s0) and sim.last_sum1 is None


def test_slice_through_the_blast_centre(ctx, sedov):
    sim = sedov
    spec = sim.map_spec("slice", axis=1, center=(0.0, 0.0, 0.0), width=(0.8, 0.6), npix=(40, 24))
    s0, mean = sim.render(spec=spec, field="temp")
    r0, r1 = seam(ctx, sim, spec, "temp", np.float64)
    assert np.array_equal(s0, r0) and np.array_equal(sim.last_sum1, r1)
    assert 0.5 < s0.mean() < 2.0  # the density of the unit box
    # the blast: the hottest pixel is within three pixels (0.06) of the centre of the window
    j, i = np.unravel_index(np.nanargmax(mean), mean.shape)
    assert abs(i - 19.5) <= 3 and abs(j - 11.5) <= 3
    for name in ("c", "vx", "divv", "curlv", "alpha", "h"):
        g0, _ = sim.render(spec=spec, field=name)
        q0, q1 = seam(ctx, sim, spec, name)
        assert np.array_equal(g0, q0) and np.array_equal(sim.last_sum1, q1), name
    with pytest.raises(sx.SxError, match="the field p is not kept"):
        sim.render(spec=spec, field="p")


def test_gravity_only_propagator(ctx):
    f, lim, bnd, dt0 = ic.plummer(512, 3)
    sim = sx.Sim(ctx, 512, sx.make_box(lim, bnd), params=sx.default_params(g=1.0), propagator=3)
    try:
        sim.set_state(f, dt0, dt0)
        sim.step()
        spec = sim.map_spec("column", axis=2, center=(0.0, 0.0, 0.0), width=(6.0, 6.0), npix=48)
        s0, _ = sim.render(spec=spec)
        r0, _ = seam(ctx, sim, spec)
        assert np.array_equal(s0, r0) and s0.max() > 0
        inside = (np.abs(sim.get(["x"])["x"]) < 2.5) & (np.abs(sim.get(["y"])["y"]) < 2.5)
        assert s0.sum() * (6.0 / 48) ** 2 >= 0.99 * inside.sum() / 512  # at least the mass well inside the window
        v0, vmean = sim.render(spec=spec, field="vx")
        assert np.array_equal(v0, s0) and np.isnan(vmean[s0 == 0]).all() and np.isfinite(vmean[s0 > 0]).all()
        for name in ("temp", "c", "p", "divv", "curlv", "alpha"):
            with pytest.raises(sx.SxError, match=f"the field {name} is not kept by the gravity-only propagator"):
                sim.render(spec=spec, field=name)
    finally:
        sim.close()


def test_ve_bdt_renders_between_substeps(ctx):
    st, obox = po.sedov_state(10)
    sim = sx.Sim(ctx, st.n + 64, sx.make_box(list(obox.lim), list(obox.bnd)), params=sx.default_params(bdt=True))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt)
        for _ in range(3):
            sim.step()
            spec = sim.map_spec("column", axis=0, npix=32)
            s0, mean = sim.render(spec=spec, field="temp")
            r0, r1 = seam(ctx, sim, spec, "temp", np.float64)
            assert np.array_equal(s0, r0) and np.array_equal(sim.last_sum1, r1)
            assert abs(s0.sum() / 32 ** 2 - 1.0) < 1e-5
    finally:
        sim.close()


def test_refusals(ctx, sedov):
    sim = sedov
    with pytest.raises(sx.SxError, match="width exceeds the box length on a periodic axis"):
        sim.render("column", width=(1.5, 1.0))
    with pytest.raises(ValueError):
        sim.render(field="rho")
