"""The friends-of-friends oracle (tests/fof_ref.py) against scipy where there is one, hand cases of the link criterion,
and the invariance of labels and catalogue under a permutation of the input."""
import numpy as np
import pytest

import fof_ref as fr


def two(d, ell, axis=0, at=0.4):
    p = [np.array([at, at]), np.array([0.5, 0.5]), np.array([0.5, 0.5])]
    p[axis] = np.array([at, at + d])
    return fr.with_dynamics({"x": p[0], "y": p[1], "z": p[2]})


@pytest.mark.parametrize("box, outside", [(fr.PERIODIC, 0), (fr.OPEN, 12), (fr.MIXED, 12)], ids=["periodic", "open", "mixed"])
def test_oracle_against_scipy(box, outside):
    sp = pytest.importorskip("scipy.spatial")
    cs = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix

    n = 6000
    f = fr.clustered(n, blobs=15, box=box, seed=11, outside=outside)
    lim, bnd = box
    ell = fr.mean_spacing_length(n, box)
    assert fr.near_ties([f["x"], f["y"], f["z"]], lim, bnd, ell) == 0
    got = fr.fof(f, lim, bnd, ell, min_members=5)
    # scipy: periodic axes through the tree's own box size, open and fixed axes shifted into a box far larger than the data
    pts = np.stack([f["x"], f["y"], f["z"]], axis=1)
    size = np.zeros(3)
    for a in range(3):
        L = lim[2 * a + 1] - lim[2 * a]
        if bnd[a] == 1:
            pts[:, a] = np.mod(pts[:, a] - lim[2 * a], L)
            size[a] = L
        else:
            pts[:, a] = pts[:, a] - pts[:, a].min()
            size[a] = 8 * (np.ptp(pts[:, a]) + 1.0)
    pairs = sp.cKDTree(pts, boxsize=size).query_pairs(ell, output_type="ndarray")
    d = pts[pairs[:, 0]] - pts[pairs[:, 1]]
    d -= size * np.round(d / size)
    pairs = pairs[(d * d).sum(axis=1) < ell * ell]
    assert got["links"] == len(pairs)
    nc, comp = cs.connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
    assert nc == got["num_all"]
    first = np.full(nc, n)
    np.minimum.at(first, comp, np.arange(n))
    assert np.array_equal(first[comp].astype(np.uint64), got["label"])
    assert got["num_groups"] == int((np.bincount(comp) >= 5).sum()) and got["num_groups"] > 5


def test_strict_criterion():
    ell = 0.05
    lim, bnd = fr.OPEN
    below = fr.fof(two(0.999999 * ell, ell), lim, bnd, ell, min_members=1)
    above = fr.fof(two(1.000001 * ell, ell), lim, bnd, ell, min_members=1)
    assert below["num_all"] == 1 and below["label"].tolist() == [0, 0] and below["count"].tolist() == [2]
    assert above["num_all"] == 2 and above["label"].tolist() == [0, 1] and above["count"].tolist() == [1, 1]
    assert below["ties"] == 0 and above["ties"] == 0
    # a pair that sits on the criterion is reported as a near tie
    assert fr.near_ties([np.array([0.4, 0.4 + ell]), np.array([0.5, 0.5]), np.array([0.5, 0.5])], lim, bnd, ell) == 1


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pair_across_a_periodic_face(axis):
    ell = 0.05
    f = two(1.0 - 0.6 * ell, ell, axis=axis, at=0.3 * ell)
    lim, bnd = fr.PERIODIC
    got = fr.fof(f, lim, bnd, ell, min_members=2)
    assert got["num_all"] == 1 and got["count"].tolist() == [2]
    # the centre of mass lies between the two through the face, inside the box
    c = got["com"][0][axis]
    assert 0.0 <= c < 1.0 and (c < 0.3 * ell or c > 1.0 - 0.3 * ell)
    assert fr.fof(f, *fr.OPEN, ell, min_members=2)["num_all"] == 2


def test_fixed_axis_is_open():
    ell = 0.05
    lim, bnd = fr.MIXED  # x periodic, y open, z fixed
    for axis, groups in ((0, 1), (1, 2), (2, 2)):
        L, lo = lim[2 * axis + 1] - lim[2 * axis], lim[2 * axis]
        p = [np.array([0.0, 0.0]), np.array([1.0, 1.0]), np.array([0.0, 0.0])]
        p[axis] = np.array([lo + 0.3 * ell, lo + L - 0.3 * ell])
        f = fr.with_dynamics({"x": p[0], "y": p[1], "z": p[2]})
        assert fr.fof(f, lim, bnd, ell, min_members=1)["num_all"] == groups, axis


def test_labels_and_catalogue_do_not_depend_on_the_order_with_ids():
    n = 5000
    f = fr.clustered(n, blobs=12, seed=5)
    lim, bnd = fr.PERIODIC
    ell = fr.mean_spacing_length(n, fr.PERIODIC)
    rng = np.random.default_rng(2)
    ids = rng.permutation(n).astype(np.uint64) + np.uint64(1000)
    a = fr.fof(f, lim, bnd, ell, ids=ids, min_members=10)
    p = rng.permutation(n)
    b = fr.fof({k: v[p] for k, v in f.items()}, lim, bnd, ell, ids=ids[p], min_members=10)
    assert a["ties"] == 0 and a["num_groups"] >= 10
    assert np.array_equal(a["label"][p], b["label"])
    for k in ("group_label", "count", "mass", "com", "vel"):
        assert np.array_equal(a[k], b[k]), k
    assert a["num_all"] == b["num_all"] and a["num_groups"] == b["num_groups"]
    # without ids the labels are indices: the partition is the same, the names are not
    c = fr.fof(f, lim, bnd, ell, min_members=10)
    assert np.array_equal(c["count"], a["count"]) and c["num_all"] == a["num_all"]
    assert np.array_equal(c["label"], c["label"][c["label"].astype(np.int64)])
    same_a = a["label"][:, None][:200] == a["label"][None, :200]
    same_c = c["label"][:, None][:200] == c["label"][None, :200]
    assert np.array_equal(same_a, same_c)


def test_helix_and_dense_ball_are_one_group_each():
    f = fr.helix()
    got = fr.fof(f, *fr.PERIODIC, 0.01, min_members=1)
    assert got["ties"] == 0 and got["links"] == 4096 and got["num_all"] == 1 and got["count"].tolist() == [4097]
    f = fr.dense_ball(600)
    got = fr.fof(f, *fr.OPEN, 0.05, min_members=1)
    assert got["links"] == 600 * 599 // 2 and got["num_all"] == 1
