"""The CPU oracle (oracle/sph_oracle.c) against the reference's outputs frozen in tests/golden/.

Bit-exact: the restatement evaluates every expression in the reference's order and precision, so with the
same inputs (and the same tree => the same neighbor order) every field must match exactly.
"""
import numpy as np
import pytest

import golden_util as gu
import pyoracle as po


@pytest.fixture(scope="module")
def ora():
    return po.load_oracle()


def test_tables(ora):
    d = gu.load("kernels.npz")
    # the kernel fixture was produced with these tables; K is implied by xm values below, check tables vs K
    assert ora.K == pytest.approx(0.7904495894323034, rel=0, abs=0)
    assert ora.wh[0] == 1.0 and ora.whd[0] == 0.0
    assert d["xm"].dtype == np.float32


@pytest.mark.parametrize("name,steps", [("sedov10.npz", 3), ("noh10.npz", 3)])
def test_full_steps_bitwise(ora, name, steps):
    d = gu.load(name)
    box = gu.box_from(d["box"])
    st = gu.state_from(d, "s0_")
    for s in range(1, steps + 1):
        ora.step(st, box)
        ref = gu.state_from(d, f"s{s}_")
        for k in st.arrays:
            assert np.array_equal(st.arrays[k], ref.arrays[k]), (name, s, k)
        assert (st.minDt, st.minDt_m1, st.ttot) == (ref.minDt, ref.minDt_m1, ref.ttot)


def test_kernels_bitwise(ora):
    d = gu.load("kernels.npz")
    box = gu.box_from(d["box"])
    st = gu.state_from(d, "in_")
    nbr, nc = ora.find_neighbors(st, box, iterate_h=True)
    assert np.array_equal(nc, d["nc"])
    assert np.array_equal(nbr, d["nbr"])
    assert np.array_equal(st.h, d["h_after_iter"])
    st.nc[:] = nc
    ora.xmass(st, box, nbr)
    assert np.array_equal(st.xm, d["xm"])
    ora.ve_def_gradh(st, box, nbr)
    assert np.array_equal(st.kx, d["kx"]) and np.array_equal(st.gradh, d["gradh"])
    ora.eos(st)
    assert np.array_equal(st.prho, d["prho"]) and np.array_equal(st.c, d["c"])
    ora.iad_divv_curlv(st, box, nbr)
    for k in ["c11", "c12", "c13", "c22", "c23", "c33", "divv", "curlv"]:
        assert np.array_equal(st.arrays[k], d[k]), k
    ora.av_switches(st, box, nbr)
    assert np.array_equal(st.alpha, d["alpha"])
    mdt = ora.momentum_energy(st, box, nbr)
    assert mdt == d["minDtCourant"][0]
    for k in ["du", "ax", "ay", "az"]:
        assert np.array_equal(st.arrays[k], d[k]), k


def test_tree_and_neighbors_bitwise(ora):
    d = gu.load("tree_rand.npz")
    box = gu.box_from(d["box"])
    n = d["x"].size
    st = po.HostState(n)
    st.x[:], st.y[:], st.z[:] = d["x"], d["y"], d["z"]
    # keys of the sorted coordinates must equal the sorted reference keys
    keys = ora.sfc_keys(st, box).copy()
    assert np.array_equal(keys, d["keys_unsorted"][d["order"]])
    tree = ora.octree(keys, 16)
    for k, v in tree.items():
        assert np.array_equal(v, d["tree_" + k]), k
    cen, siz = ora.node_centers(tree["prefixes"], box)
    assert np.array_equal(cen, d["centers"]) and np.array_equal(siz, d["sizes"])
    st.h[:] = d["h0"]
    nbr, nc = ora.find_neighbors(st, box, bucket=16, iterate_h=False)
    assert np.array_equal(nc, d["nc_noiter"]) and np.array_equal(nbr, d["nbr_noiter"])
    nbr, nc = ora.find_neighbors(st, box, bucket=16, iterate_h=True)
    assert np.array_equal(nc, d["nc_iter"]) and np.array_equal(nbr, d["nbr_iter"])
    assert np.array_equal(st.h, d["h_iter"])


@pytest.mark.parametrize("name", ["mixed", "gresho"])
def test_boxes_bitwise(ora, name):
    """boxes.npz: the reference's keys and two VE steps in a mixed-boundary off-origin box (16x8x4) and a thin
    periodic one (21x21x3); re-pins the oracle's per-axis box arithmetic where oracle/_ref does not exist"""
    d = gu.load("boxes.npz")
    box = gu.box_from(d[f"{name}_box"])
    n = d[f"{name}_in_x"].size
    st = po.HostState(n)
    for k in po.CONSERVED:
        st.arrays[k][:] = d[f"{name}_in_{k}"]
    sc = d[f"{name}_s2_scalars"]
    st.minDt = st.minDt_m1 = 1e-5
    assert np.array_equal(ora.sfc_keys(st, box), d[f"{name}_keys"])
    for _ in range(2):
        ora.step(st, box)
    stored = [k[len(name) + 4:] for k in d if k.startswith(f"{name}_s2_") and not k.endswith("scalars")]
    assert len(stored) >= len(po.CONSERVED) + 6
    for k in stored:
        assert np.array_equal(st.arrays[k], d[f"{name}_s2_{k}"]), (name, k)
    assert (st.minDt, st.minDt_m1, st.ttot) == (sc[0], sc[1], sc[2])


def test_oracle_rejects_out_of_range_neighbor_indices():
    """a neighbor list exported from the path under test is input to the checker: an index beyond the state fails as
    an assertion (sph_oracle.c lists_ok), it does not crash the process"""
    import pytest

    ora = po.load_oracle()
    st, box = po.sedov_state(8)
    po.converge_h(ora, st, box)
    keys = ora.sfc_keys(st, box).copy()
    o = np.argsort(keys, kind="stable")
    for k in st.arrays:
        st.arrays[k][:] = st.arrays[k][o]
    st.keys[:] = keys[o]
    nbr, nc = ora.find_neighbors(st, box)
    st.nc[:] = nc
    ora.xmass(st, box, nbr)  # a good list passes
    bad = nbr.copy()
    bad[5 * 150 + 3] = st.n + 1000
    with pytest.raises(AssertionError, match="outside"):
        ora.xmass(st, box, bad)
