"""packed12 exact lists (sx_pack12.hpp) through a skin-list sequence: the filter's list writer (set A or B) and its
frozen-path XMass reader, next to the search's writer.

A side-12 Sedov lattice (1728 particles, 7 clusters) for 8 steps: a fresh build, walked steps that write a cluster's
other list set and steps that keep or switch back to a set.  No cluster of a lattice this small freezes (measured:
42 kept, 0 frozen clusters in the 7 reuse steps), so a side-20 lattice at rest for 12 steps, the case of
test_gpu_skin.py::test_skin_frozen_steps_equal_fresh_search, adds the frozen steps.  After every step nc, h and the
neighbor sets
(sx_sim_export_neighbors, which reads the cluster's current set in its format) equal those of a fresh sync + search of
the same state by a second Sim without skin; the step's xm (the filter's fused XMass) equals the fresh Sim's to float
rounding of a sum in another order.  Once with the default packed12 threshold and once with the threshold lowered
between the lattice's smallest and largest union count, so that packed and u16 clusters are filtered side by side.
"""
import numpy as np
import pytest

import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

STATE = ["x", "y", "z", "h", "m", "temp", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "du_m1", "alpha", "id"]
CASES = {"blast": (12, 8), "quiescent": (20, 12)}  # lattice side, steps


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def union_counts(sim):
    """union count of every cluster from the exported sets: the distinct neighbors of each 256 targets in SFC order"""
    ids = sim.get(["id"])["id"]
    sets = sim.neighbor_sets()
    return [np.unique(np.concatenate([sets[int(i)] for i in ids[c:c + 256]])).size for c in range(0, ids.size, 256)]


@pytest.mark.parametrize("quiescent", [False, True], ids=["blast", "quiescent"])
@pytest.mark.parametrize("threshold", ["default", "lowered"])
def test_skin_sequence_equals_fresh_search(ctx, threshold, quiescent):
    side, steps = CASES["quiescent" if quiescent else "blast"]
    st, obox = po.sedov_state(side)
    if quiescent:
        st.temp[:] = st.temp.min()  # no blast: nothing moves, clusters freeze between the steps on which h changes
    box = gutil.box_to_sx(obox)
    b = sx.Sim(ctx, st.n, box)  # the fresh search: no skin, default threshold
    b.set_skin(0.0, 1)
    a = None
    try:
        thr = 4095
        if threshold == "lowered":
            b.set_state(st.arrays, st.minDt, st.minDt_m1)
            b.step()
            uc = union_counts(b)
            thr = (min(uc) + max(uc)) // 2
            assert min(uc) <= thr < max(uc), uc
        ctx.set_pack12_max(thr)
        a = sx.Sim(ctx, st.n, box)
        ctx.set_pack12_max(None)
        a.set_skin(0.05, 24)
        a.set_state(st.arrays, st.minDt, st.minDt_m1)
        for s in range(steps):
            g = a.get(STATE)
            sc = a.scalars()
            b.set_state(g, sc["minDt"], sc["minDt_m1"])
            a.step()
            b.step()
            ga, gb = a.get(["id", "nc", "h", "xm"]), b.get(["id", "nc", "h", "xm"])
            oa, ob = np.argsort(ga["id"]), np.argsort(gb["id"])
            assert np.array_equal(ga["nc"][oa], gb["nc"][ob]), (s, a.skin_stats())
            assert np.array_equal(ga["h"][oa], gb["h"][ob]), s
            na, nb = a.neighbor_sets(), b.neighbor_sets()
            bad = [k for k in na if not np.array_equal(na[k], nb[k])]
            assert not bad, (s, len(bad), bad[:3])
            xa, xb = ga["xm"][oa].astype(np.float64), gb["xm"][ob].astype(np.float64)
            assert np.all(np.abs(xa - xb) <= 2e-5 * np.abs(xb)), (s, float(np.max(np.abs(xa / xb - 1))))
        ks = a.skin_stats()
        print(threshold, thr, ks)
        assert ks["builds"] >= 1 and ks["reuse_steps"] > 0, ks
        assert ks["kept_clusters"] > 0, ks
        if quiescent:
            assert ks["frozen_clusters"] > 0, ks
    finally:
        ctx.set_pack12_max(None)
        if a is not None:
            a.close()
        b.close()
