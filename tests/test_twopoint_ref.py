"""The oracle of the two-point statistics (tests/twopoint_ref.py) pinned against facts that do not come from it: lattice
coordination numbers, hand-placed particles, a Hubble flow, a rigid rotation, the stride identity, and scipy's tree counts
where scipy is installed.  No GPU and no library."""
import math

import numpy as np
import pytest

import twopoint_ref as tr


def test_lattice_coordination_numbers():
    """a simple cubic lattice in a periodic box: 6 neighbours at a, 12 at sqrt(2) a, 8 at sqrt(3) a per point, each pair
    counted once: 3 N, 6 N and 4 N"""
    k, a = 8, 1.0 / 8
    f = tr.columns(tr.lattice(k, a))
    N = k ** 3
    ref = tr.twopoint(f, *tr.PERIODIC, [0.5 * a, 1.2 * a, 1.6 * a, 1.9 * a], series=0)
    assert ref["count"].tolist() == [3 * N, 6 * N, 4 * N]
    assert ref["targets"] == N and ref["nonfinite"] == 0 and ref["coincident"] == 0


def test_hand_placed_edge_face_and_coincident():
    """A and B 0.25 apart along x (exactly an edge: it belongs to the bin that starts there); C across the periodic x face
    from A, 0.125 away through the face; D on top of A"""
    pos = np.array([[0.0625, 0.5, 0.5], [0.3125, 0.5, 0.5], [0.9375, 0.5, 0.5], [0.0625, 0.5, 0.5]])
    f = tr.columns(pos)
    edges = [0.0, 0.25, 0.3]
    ref = tr.twopoint(f, *tr.PERIODIC, edges, series=0)
    # A-B and D-B at 0.25 -> bin 1; A-C and D-C at 0.125 -> bin 0; B-C at 0.375 -> outside; A-D coincident
    assert ref["count"].tolist() == [2, 2] and ref["coincident"] == 1
    # without the periodic face C is 0.875 from A: outside
    ref = tr.twopoint(f, *tr.OPEN, edges, series=0)
    assert ref["count"].tolist() == [0, 2] and ref["coincident"] == 1


def test_hubble_flow_and_rotation():
    rng = np.random.default_rng(3)
    n, H = 300, 0.75
    pos = rng.random((n, 3))
    c = np.array([0.5, 0.25, 0.125])
    f = tr.columns(pos)
    # velocities that are float32 AND exactly H (x - c): positions on a 2^-12 grid
    pos = np.round(pos * 4096) / 4096
    f = tr.columns(pos)
    for a, k in enumerate(("vx", "vy", "vz")):
        f[k] = (H * (pos[:, a] - c[a])).astype(np.float32)
        assert np.array_equal(f[k].astype(np.float64), H * (pos[:, a] - c[a]))
    edges = np.linspace(0.0, 0.4, 9)
    ref = tr.twopoint(f, *tr.OPEN, edges, series=tr.VEL)
    assert ref["pairs"] > 5000
    assert np.all(np.abs(ref["u"] - H * ref["r"]) <= 1e-12 * H * ref["r"])
    mean_r = np.bincount(ref["bin"], ref["r"], minlength=8) / ref["count"]
    s1 = ref["U1"] / ref["count"]
    assert np.all(np.abs(s1 - H * mean_r) <= 1e-12 * H * mean_r)
    # rigid rotation about z: v = Omega x (x - c) changes no separation
    om = 1.5
    f["vx"] = (-om * (pos[:, 1] - c[1])).astype(np.float32)
    f["vy"] = (om * (pos[:, 0] - c[0])).astype(np.float32)
    f["vz"] = np.zeros(n, np.float32)
    ref = tr.twopoint(f, *tr.OPEN, edges, series=tr.VEL)
    vmax = max(float(np.max(np.abs(f[k]))) for k in ("vx", "vy"))
    assert np.all(np.abs(ref["u"]) < 1e-12 * vmax)
    assert np.all(ref["T2"] > 0)


def test_stride_identity():
    """The target sets of phase = 0 .. stride - 1 partition the particles.  A pair with both members in one set is counted
    once for that phase; a pair with members in two sets is counted for both phases.  With c1 the counts of stride 1:
    sum_phase count(stride, phase) = c1 + (pairs whose members lie in different sets), so
    sum_phase count(stride, phase) - c1 = c1 - sum_phase TT(phase), TT(phase) the pairs with both members targets of
    that phase: the target-target pairs of a phase are the count of that phase's targets alone."""
    f = tr.uniform(400, seed=11)
    ids = np.random.default_rng(12).permutation(400).astype(np.uint64)
    edges = [0.0, 0.1, 0.2, 0.3]
    stride = 3
    c1 = tr.twopoint(f, *tr.PERIODIC, edges, series=0)["count"].astype(np.int64)
    total = np.zeros(3, np.int64)
    tt = np.zeros(3, np.int64)
    seen = np.zeros(400, int)
    for phase in range(stride):
        total += tr.twopoint(f, *tr.PERIODIC, edges, series=0, stride=stride, phase=phase, ids=ids)["count"].astype(np.int64)
        sel = ids % stride == phase
        seen += sel
        sub = {k: v[sel] for k, v in f.items()}
        tt += tr.twopoint(sub, *tr.PERIODIC, edges, series=0)["count"].astype(np.int64)
    assert np.all(seen == 1), "the union over the phases is everything, each particle once"
    assert np.array_equal(total - c1, c1 - tt)
    assert np.all(tt > 0) and np.all(total > c1)


def test_fixed_sums_vectorised_equal_scalar():
    rng = np.random.default_rng(5)
    t = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-30, 3, 500), [0.0, -0.0, 5e-324, -5e-324]])
    E = tr.window(t)
    bins = rng.integers(0, 4, len(t))
    sums, ints = tr.bin_sums(t, bins, 4, E)
    for b in range(4):
        want = sum(tr.to_fixed(v, E) for v in t[bins == b])
        assert ints[b] == want
        assert sums[b] == tr.from_fixed(want, E)
    assert tr.window([0.0]) == tr.ZERO_WINDOW and tr.window([5e-324]) == -1073 and tr.window([1.0]) == 1
    assert tr.to_fixed(-1.0, 1) == -(1 << 63) and tr.words(-1) == ((1 << 64) - 1, (1 << 64) - 1)
    assert math.copysign(1.0, tr.from_fixed(0, 0)) == 1.0


def test_counts_against_scipy_tree():
    spatial = pytest.importorskip("scipy.spatial")
    f = tr.uniform(1500, seed=21)
    pos = np.stack([f[k] for k in "xyz"], axis=1)
    edges = np.array([0.02, 0.05, 0.1, 0.2])
    ref = tr.twopoint(f, *tr.PERIODIC, edges, series=0)
    tree = spatial.cKDTree(pos, boxsize=1.0)
    # count_neighbors counts ordered pairs with r <= radius, self pairs included; the radii sit just below the edges so
    # that "<=" there is "<" at the edge
    cum = tree.count_neighbors(tree, np.nextafter(edges, 0.0))
    unordered = (cum - len(pos)) // 2
    assert np.array_equal(ref["count"].astype(np.int64), np.diff(unordered))
