"""Sim.fof (sx_sim_fof) on one rank: in the VE layout (periodic box) and in the gravity-only layout (open box), each
holding the clustered state of tests/fof_ref.py with 20 000 particles, labels and catalogue equal the oracle on the
columns Sim.get copies, before and after a few steps; the call changes no state; linking= and length= agree.

The VE state needs a smoothing length per particle: it is estimated from cell counts at two scales and capped (the
step's own h iteration takes it from there).  The refusal of a communicator with more than one rank is not tested here: one process
holds one rank, so it would take worker processes for a message.
"""
import numpy as np
import pytest

import fof_ref as fr
import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

N = 20000
COLUMNS = ["x", "y", "z", "m", "vx", "vy", "vz", "id"]


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def smoothing_lengths(f, box, ng0=100):
    """h for about ng0 neighbours within 2 h from the number density in cells of 1/40 (where a cell holds 16 or more)
    and of 1/10 of the box, the finer one where both apply"""
    lim, _ = box
    u = np.stack([(f[k] - lim[2 * a]) / (lim[2 * a + 1] - lim[2 * a]) for a, k in enumerate("xyz")], axis=1)
    vol = np.prod([lim[2 * a + 1] - lim[2 * a] for a in range(3)])
    rho = np.zeros(len(u))
    for cells, least in ((10, 1), (40, 16)):
        c = np.clip(np.floor(u * cells).astype(np.int64), 0, cells - 1)
        key = c[:, 0] + cells * (c[:, 1] + cells * c[:, 2])
        cnt = np.bincount(key, minlength=cells ** 3)[key]
        rho = np.where(cnt >= least, cnt / (vol / cells ** 3), rho)
    # capped on the low side: the step's iteration grows an h that is too small within a step or two, while the
    # coarse cells' estimate next to a blob (far too large) had it diverge and the search run out of candidate space
    return np.minimum(0.5 * np.cbrt(3.0 * ng0 / (4.0 * np.pi * rho)), 0.03).astype(np.float32)


def clustered_state(box, nbody):
    f = fr.clustered(N, box=box, seed=21)
    dt = 1e-5
    st = {k: f[k] for k in ("x", "y", "z", "m")}
    for k in ("vx", "vy", "vz"):
        st[k] = (np.float32(0.1) * f[k]).astype(np.float32)
    for k, v in (("x_m1", "vx"), ("y_m1", "vy"), ("z_m1", "vz")):
        st[k] = (st[v] * np.float32(dt)).astype(np.float32)
    st["h"] = np.full(N, 0.01, np.float32) if nbody else smoothing_lengths(f, box)
    st["id"] = np.random.default_rng(8).permutation(N).astype(np.uint64)
    if not nbody:
        st["temp"] = np.full(N, 0.05 / np.float64(po.ideal_gas_cv()))
        st["du_m1"] = np.zeros(N, np.float32)
        st["alpha"] = np.full(N, 0.05, np.float32)
    return st, dt


def check_against_oracle(sim, box, min_members=20):
    cols = sim.get(COLUMNS)
    lim, bnd = box
    spec = sim.fof_spec(0.2, None, min_members, 4096)
    ref = fr.fof(cols, lim, bnd, spec.linking, ids=cols["id"], min_members=min_members)
    got = sim.fof(labels=True, min_members=min_members)
    fr.assert_same(got, ref, box)  # labels in the sim's order: entry k belongs to cols["id"][k]
    stats = sim.fof_stats()
    assert stats["num_all"] == ref["num_all"] and stats["num_groups"] == ref["num_groups"]
    assert stats["pair_tests"] >= ref["links"]
    assert np.all(np.isin(got["group_label"], cols["id"]))
    without = sim.fof(min_members=min_members)
    assert without["label"] is None and np.array_equal(without["mass"], got["mass"])
    return got, ref


@pytest.mark.parametrize("layout", ["ve", "nbody"])
def test_sim_fof_before_and_after_steps(ctx, layout):
    nbody = layout == "nbody"
    box = fr.OPEN if nbody else fr.PERIODIC
    st, dt = clustered_state(box, nbody)
    params = sx.default_params(g=1.0, nbody=True) if nbody else sx.default_params()
    sim = sx.Sim(ctx, N + 64, sx.make_box(*box), params=params)
    try:
        sim.set_state(st, dt, dt)
        got, ref = check_against_oracle(sim, box)
        assert ref["num_groups"] >= 30 and ref["count"][0] > 100
        assert np.allclose((N / 0.2 ** 3) ** (-1.0 / 3.0), sim.fof_spec().linking, rtol=1e-12)
        before = sim.get(COLUMNS)
        for _ in range(3):
            sim.step()
        after = sim.get(COLUMNS)
        assert not np.array_equal(before["id"], after["id"]) or not np.array_equal(before["x"], after["x"])
        check_against_oracle(sim, box)
        # linking in mean spacings and the absolute length it stands for
        a = sim.fof(linking=0.15, min_members=10, labels=True)
        b = sim.fof(length=0.15 * (1.0 / N) ** (1.0 / 3.0), min_members=10, labels=True)
        assert all(np.array_equal(a[k], b[k]) for k in ("label", "group_label", "count", "mass", "com", "vel"))
        assert a["num_groups"] == b["num_groups"] > 0
        with pytest.raises(sx.SxError, match="exceeds a third of the periodic x extent" if not nbody else "finite and positive"):
            sim.fof(length=0.5 if not nbody else -1.0)
    finally:
        sim.close()


def run_steps(ctx, fof_after):
    st, obox = po.sedov_state(12)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        sim.step()
        sim.step()
        if fof_after:
            names = sim.allocated_fields()
            before, mem0, sc0 = sim.get(names), sim.memory(), sim.scalars()
            cat = sim.fof(linking=1.5, min_members=1, labels=True)  # face and edge neighbours of the lattice are friends
            assert cat["num_all"] >= 1 and int(cat["count"].sum()) == st.n
            mem1 = sim.memory()
            after = sim.get(names)
            assert all(before[k].tobytes() == after[k].tobytes() for k in names) and sim.scalars() == sc0
            assert mem1["device"] > mem0["device"] and mem1["pinned"] > mem0["pinned"]  # the fof.* buffers, counted
            sim.fof(linking=1.5, min_members=1, labels=True)
            assert sim.memory() == mem1
        sim.step()
        return sim.get(["id", "x", "y", "z", "vx", "vy", "vz", "temp", "h"]), sim.scalars()
    finally:
        sim.close()


def test_a_group_search_changes_no_state(ctx):
    """every field is the same before and after the call, and the next step is the one of a run that never asked"""
    asked, sc_a = run_steps(ctx, True)
    never, sc_n = run_steps(ctx, False)
    assert sc_a == sc_n
    for k in asked:
        assert asked[k].tobytes() == never[k].tobytes(), k
