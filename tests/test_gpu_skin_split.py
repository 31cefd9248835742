"""A reuse step's search as three kernels (sph-exa_amd/csrc/sx_skin.hpp: skinDecide, then skinFrozen over the clusters
it marked frozen and skinFilter over those it marked walk; stale clusters rebuilt or searched exactly as before).

Every step of every case is compared with a fresh sync + search of the same state (a second Sim with the skin off,
handed the state before the step), particle by particle by id: nc and h exact, the neighbor sets equal, xm within 2e-6
(the bound of test_gpu_skin.py::test_skin_frozen_steps_equal_fresh_search).  The shapes are the smallest that reach
each path, and each case asserts from skin_stats that its path was taken (per step: stale, exact, kept, frozen
clusters, measured on MI355X, the same before and after the split):
  * Sedov 21^3 (9261 particles: 37 clusters, the last one partly filled), 12 steps: 18 clusters frozen on steps 1, 2, 4,
    5, 8 and 9, the others walked and kept; worst xm difference 1.5e-6;
  * a lattice at rest, 32^3, 4 steps: all 128 clusters frozen on steps 1 and 2 (no cluster is left to the walk), all walked on
    step 3.  32 is the smallest side that freezes every cluster: a lane freezes only where the float test is exact,
    |r| + 2.05 h < 0.49 L on periodic axes (sx_skin.hip), which no 8 x 8 x 4 cluster of a 16^3 lattice meets (0 of 16
    clusters frozen on any step; 20^3: 4 of 32, 24^3: 36 of 54);
  * that 16^3 lattice at rest, 4 steps: no cluster is frozen on any reuse step, the first after the build
    included, and every cluster is walked and keeps its lists (Sedov 21^3 freezes 18 clusters on its first reuse step);
  * Noh 30^3, 10 steps: 42 of 56 clusters stale and rebuilt on step 1 with 7 frozen and 7 walked ones beside them, 36
    stale on step 6 (no cluster takes the exact search at this size: test_gpu_skin.py reaches it at 80^3);
  * Sedov 21^3 in a context whose packed12 threshold lies below every union size: the frozen kernel reads u16 lists;
  * Sedov 21^3 with the frozen kernel's staging cut to 512 entries, packed12 and u16: every union is larger, so the
    entries beyond the staging come from global memory (the path of unions above 1664 entries).
"""
import numpy as np
import pytest

import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx
from test_gpu_skin import STATE, _ic, _sorted_rows, ctx  # noqa: F401  (ctx: the module's context fixture)

pytestmark = pytest.mark.gpu

COUNTS = ("reuse_steps", "stale_clusters", "exact_clusters", "kept_clusters", "frozen_clusters")


def _steps_vs_fresh(ctx, st, obox, steps, factor, label, frozen_stage=0):
    """runs `steps` steps with the skin, each against a fresh search of the same state; returns per step the growth of
    the COUNTS of skin_stats, and the number of clusters.  frozen_stage: the union entries the frozen kernel stages
    (sx_sim_set_skin_frozen_stage_internal; 0: the default)"""
    box = gutil.box_to_sx(obox)
    a = sx.Sim(ctx, st.n, box)
    a.set_skin(factor, 24)
    b = sx.Sim(ctx, st.n, box)
    b.set_skin(0.0, 1)
    a.set_state(st.arrays, st.minDt, st.minDt_m1)
    per_step = []
    try:
        assert a.L.sx_sim_set_skin_frozen_stage_internal(a.h, frozen_stage) == sx.SX_OK
        last = a.skin_stats()
        for s in range(steps):
            g = a.get(STATE)
            sc = a.scalars()
            b.set_state(g, sc["minDt"], sc["minDt_m1"])
            a.step()
            b.step()
            ga, gb = a.get(["id", "nc", "h", "xm"]), b.get(["id", "nc", "h", "xm"])
            oa, ob = np.argsort(ga["id"]), np.argsort(gb["id"])
            ks = a.skin_stats()
            assert np.array_equal(ga["nc"][oa], gb["nc"][ob]), (label, s, ks)
            assert np.array_equal(ga["h"][oa], gb["h"][ob]), (label, s, ks)
            assert np.array_equal(_sorted_rows(a), _sorted_rows(b)), (label, s, ks)
            xa, xb = ga["xm"][oa].astype(np.float64), gb["xm"][ob].astype(np.float64)
            worst = float(np.max(np.abs(xa / xb - 1.0)))
            per_step.append({k: int(ks[k] - last[k]) for k in COUNTS} | {"xm": worst})
            np.testing.assert_allclose(ga["xm"][oa], gb["xm"][ob], rtol=2e-6, err_msg=str((label, s, ks)))
            last = ks
        print(label, factor, (st.n + 255) // 256, "clusters", per_step)
        return per_step, (st.n + 255) // 256
    finally:
        restored = a.L.sx_sim_set_skin_frozen_stage_internal(a.h, 0)
        a.close()
        b.close()
        assert restored == sx.SX_OK


def _walked(p, ncl):
    """clusters of a reuse step neither stale nor frozen when the step's search began (a cluster that goes stale in
    its walk counts as stale: a lower bound)"""
    return p["reuse_steps"] * ncl - p["stale_clusters"] - p["frozen_clusters"]


def test_split_sedov_partly_filled_last_cluster(ctx):
    st, obox = po.sedov_state(21)
    per, ncl = _steps_vs_fresh(ctx, st, obox, 12, 0.05, "sedov 21")
    assert ncl == 37 and st.n % 256 != 0
    assert sum(p["frozen_clusters"] for p in per) > 0, per
    assert sum(p["kept_clusters"] - p["frozen_clusters"] for p in per) > 0, per  # kept by a walk
    assert any(p["reuse_steps"] and p["frozen_clusters"] and _walked(p, ncl) > 0 for p in per), per


def test_split_lattice_at_rest_every_cluster_frozen(ctx):
    st, obox = po.sedov_state(32)
    st.temp[:] = st.temp.min()  # no blast: nothing moves
    per, ncl = _steps_vs_fresh(ctx, st, obox, 4, 0.05, "lattice 32")
    assert all(p["stale_clusters"] == 0 for p in per), per
    assert any(p["frozen_clusters"] == ncl for p in per), per  # no cluster was left to the walk
    assert any(p["reuse_steps"] and p["frozen_clusters"] == 0 and p["kept_clusters"] > 0 for p in per), per


def test_split_no_frozen_cluster_from_first_reuse_step(ctx):
    """a 16^3 lattice at rest: no cluster can freeze (module docstring), so from the first reuse step after the build
    on the frozen kernel finds no cluster of its own and the walk serves, and keeps, every cluster"""
    st, obox = po.sedov_state(16)
    st.temp[:] = st.temp.min()
    per, ncl = _steps_vs_fresh(ctx, st, obox, 4, 0.05, "lattice 16")
    assert [p["reuse_steps"] for p in per] == [0, 1, 1, 1], per
    assert all(p["frozen_clusters"] == 0 and p["stale_clusters"] == 0 for p in per), per
    assert all(p["kept_clusters"] == ncl and _walked(p, ncl) == ncl for p in per[1:]), per


def test_split_noh_stale_rebuild(ctx):
    st, obox = po.noh_state(30)
    per, ncl = _steps_vs_fresh(ctx, st, obox, 10, 0.05, "noh 30")
    assert sum(p["stale_clusters"] for p in per) > 0, per
    assert sum(p["kept_clusters"] for p in per) > sum(p["frozen_clusters"] for p in per) > 0, per
    assert any(p["reuse_steps"] and p["stale_clusters"] and p["frozen_clusters"] and _walked(p, ncl) > 0
               for p in per), per


def test_split_u16_lists(ctx):
    """packMax below every union size (a full cluster's union holds at least its own 256 particles)"""
    st, obox = po.sedov_state(21)
    ctx.set_pack12_max(256)
    try:
        per, ncl = _steps_vs_fresh(ctx, st, obox, 4, 0.05, "sedov 21, u16 lists")
    finally:
        ctx.set_pack12_max(None)
    assert sum(p["frozen_clusters"] for p in per) > 0, per
    assert sum(p["kept_clusters"] for p in per) > sum(p["frozen_clusters"] for p in per), per


@pytest.mark.parametrize("pack_max", [None, 256])
def test_split_union_beyond_the_staging(ctx, pack_max):
    st, obox = po.sedov_state(21)
    ctx.set_pack12_max(pack_max)
    try:
        per, ncl = _steps_vs_fresh(ctx, st, obox, 4, 0.05, f"sedov 21, staging 512, packMax {pack_max}",
                                   frozen_stage=512)
    finally:
        ctx.set_pack12_max(None)
    assert sum(p["frozen_clusters"] for p in per) > 0, per
