"""Pins of tests/halo_ref.py, the numpy oracle of the group properties: closed forms for two bodies, a rigid rotator and
a lattice cube, the direct sum's own restatement (direct_ref.direct) for the potential, periodic faces, and fof_ref.fof
without a cut.  No GPU."""
import numpy as np

import direct_ref as dr
import fof_ref as fr
import halo_ref as hr


def cols(p, m=None, v=None, h=None):
    p = np.asarray(p, np.float64)
    n = len(p)
    f = {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy()}
    f["m"] = np.asarray(m if m is not None else np.full(n, 1.0 / n), np.float32)
    v = np.zeros((n, 3)) if v is None else np.asarray(v)
    for a, k in enumerate(("vx", "vy", "vz")):
        f[k] = v[:, a].astype(np.float32)
    f["h"] = np.asarray(h if h is not None else np.full(n, 1e-4), np.float32)
    return f


def test_two_bodies_unsoftened_and_softened():
    m1, m2, r, G = np.float32(0.25), np.float32(0.75), (0.5 + 0.03) - 0.5, 2.0  # r as the stored coordinates give it
    hij = np.float32(0.02) + np.float32(0.02)
    h2 = float(hij * hij)  # the sum and its square are float operations, as in the direct sum's P2P
    for h, want in ((0.001, -G * float(m1) * float(m2) / r), (0.02, -G * float(m1) * float(m2) * r * r / h2 ** 1.5)):
        f = cols([[0.5, 0.5, 0.5], [0.5 + r, 0.5, 0.5]], m=[m1, m2], h=[h, h])
        ref = hr.halo(f, *fr.OPEN, 0.05, min_members=1, G=G)
        assert ref["count"].tolist() == [2]
        assert abs(ref["epot"][0] - want) <= 8 * hr.EPS * abs(want)
        assert (ref["soft"][0], ref["hard"][0]) == ((1, 0) if h > 0.01 else (0, 1))


def test_one_member_or_two_coincident_members_give_zero():
    f = cols([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.8, 0.8, 0.8]])
    ref = hr.halo(f, *fr.OPEN, 0.05, min_members=1)
    assert ref["count"].tolist() == [2, 1] and ref["epot"].tolist() == [0.0, 0.0] and ref["pair_terms"] == 1


def test_potential_is_half_the_direct_sum_over_the_members_alone():
    f = dr.inputs(300, 5)
    out4, scale = dr.direct(f, 0)
    lim = [-0.5, 0.5] * 3
    ref = hr.halo(dict(f, vx=np.zeros(300, np.float32), vy=np.zeros(300, np.float32), vz=np.zeros(300, np.float32)),
                  lim, [0, 0, 0], 0.3, min_members=1, G=float(dr.G))
    assert ref["count"].tolist() == [300] and ref["soft"][0] > 0 and ref["hard"][0] > 0
    want = 0.5 * out4[:, 0].sum()
    bound = 0.5 * dr.reorder_bound(300, 0, scale)[:, 0].sum() + 300 * 2.0 ** -52 * abs(want)
    assert abs(ref["epot"][0] - want) <= bound


def test_rigid_rotator():
    """eight equal masses on a ring of radius R in the xy plane, rotating with omega about z and drifting with U"""
    R, omega, n, U = 0.01, 3.0, 8, np.array([0.5, -0.25, 0.125])
    phi = 2 * np.pi * np.arange(n) / n
    p = np.stack([0.5 + R * np.cos(phi), 0.5 + R * np.sin(phi), np.full(n, 0.5)], axis=1)
    v = np.stack([-omega * R * np.sin(phi), omega * R * np.cos(phi), np.zeros(n)], axis=1) + U
    f = cols(p, m=np.full(n, 0.125), v=v)
    ref = hr.halo(f, *fr.OPEN, 0.9 * R, min_members=1)
    assert ref["count"].tolist() == [n]
    tol = 1e-6  # the float velocities
    assert np.allclose(ref["vel"][0], U, atol=tol)
    assert np.allclose(ref["angmom"][0], [0.0, 0.0, omega * R * R], atol=tol * R)
    s = 0.5 * (omega * R) ** 2
    assert np.allclose(ref["sigma"][0], [s, 0, 0, s, 0, 0], atol=tol * omega * R)
    assert np.allclose(ref["shape"][0], [0.5 * R * R, 0, 0, 0.5 * R * R, 0, 0], atol=1e-12)
    assert abs(ref["rmax"][0] - R) < 1e-12


def test_lattice_cube_shape():
    """k^3 equal masses on a lattice of spacing a: shape_aa = a^2 (k^2 - 1) / 12, off-diagonal 0, rmax = half diagonal"""
    k, a = 5, 0.01
    g = np.arange(k) * a + 0.4
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ref = hr.halo(cols(p), *fr.OPEN, 1.5 * a, min_members=1)
    assert ref["count"].tolist() == [k ** 3]
    s = a * a * (k * k - 1) / 12.0
    assert np.allclose(ref["shape"][0], [s, 0, 0, s, 0, s], atol=1e-10 * s + 1e-18)
    assert abs(ref["rmax"][0] - 0.5 * np.sqrt(3.0) * (k - 1) * a) < 1e-14


def test_a_group_astride_a_periodic_face_equals_the_shifted_group():
    rng = np.random.default_rng(2)
    p = hr.ball(rng, 50, (0.5, 0.5, 0.5), 0.01)
    v = rng.standard_normal((50, 3))
    m = rng.uniform(0.5, 1.5, 50) / 50
    h = rng.uniform(1e-4, 6e-3, 50)
    mid = hr.halo(cols(p, m, v, h), *fr.PERIODIC, 0.02, min_members=1)
    shifted = np.mod(p + np.array([0.5, 0.0, -0.5]), 1.0)
    face = hr.halo(cols(shifted, m, v, h), *fr.PERIODIC, 0.02, min_members=1)
    assert mid["count"].tolist() == face["count"].tolist() == [50]
    for key in ("sigma", "shape", "angmom"):
        assert np.allclose(mid[key], face[key], rtol=1e-9, atol=1e-16), key
    assert abs(mid["epot"][0] - face["epot"][0]) <= 1e-10 * abs(mid["epot"][0])
    assert abs(mid["rmax"][0] - face["rmax"][0]) < 1e-12


def test_without_a_cut_it_is_fof_ref():
    f = fr.clustered(3000, seed=3)
    f["h"] = np.full(3000, 0.002, np.float32)
    ell = fr.mean_spacing_length(3000, fr.PERIODIC)
    a = fr.fof(f, *fr.PERIODIC, ell, min_members=5)
    b = hr.halo(f, *fr.PERIODIC, ell, min_members=5, rho_min=0.0)
    for key in ("label", "group_label", "count", "mass", "com", "vel"):
        assert np.array_equal(a[key], b[key]), key
    assert (a["num_groups"], a["num_all"]) == (b["num_groups"], b["num_all"]) and b["selected"].all()


def test_density_cut_takes_the_bridge_out():
    for std in (False, True):
        f, ell, chain = hr.bridge_state(std=std)
        assert fr.near_ties([f[k] for k in "xyz"], *fr.OPEN, ell) == 0
        one = hr.halo(f, *fr.OPEN, ell, min_members=1, std=std)
        two = hr.halo(f, *fr.OPEN, ell, min_members=1, rho_min=5.0, std=std)
        assert one["count"].tolist() == [141] and two["count"].tolist() == [60, 60]
        assert np.all(two["label"][chain] == hr.NONE) and two["num_all"] == 2 and not two["selected"][chain].any()
