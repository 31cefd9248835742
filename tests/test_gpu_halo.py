"""Group properties on the GPU at seam level (sx_halo_compute through Context.halos) on uploaded synthetic columns,
against tests/halo_ref.py.  Without a cut the search is sx_fof's, bit for bit.  Moments and the thermal energy are compared
about the device's own com, vel and mass within the summation bound the oracle returns per group and component; the
potential within the contract 2^-15 |W| of the header, against the oracle and against the direct sum in exact mode on a
group uploaded alone; the pair count exactly.  As in test_gpu_fof.py, a comparison of groups first asserts that the
input has no pair on the link criterion."""
import ctypes as C
import functools

import numpy as np
import pytest

import fof_ref as fr
import halo_ref as hr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

N = 20000
CV = float(np.float32(np.float64(np.float32(8.317e7) / np.float32(10.0)) / (5.0 / 3.0 - 1.0)))
BOXES = {"periodic": (fr.PERIODIC, 0), "open": (fr.OPEN, 16), "mixed": (fr.MIXED, 16)}
FOF_KEYS = ("label", "group_label", "count", "mass", "com", "vel")
ALL = ("moments", "thermal", "potential")


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def run(ctx, f, box, ell, ids=None, min_members=20, max_groups=4096, labels=True, std=False, edit=None, **kw):
    """(device result, halo stats) for the host columns f"""
    lim, bnd = box
    ds = sx.DeviceState(ctx, {k: np.asarray(v) for k, v in f.items()}, std=std)
    try:
        if edit:
            edit(ds.fields)
        dev_id = ctx.upload(np.ascontiguousarray(ids, dtype=np.uint64)) if ids is not None else None
        spec = sx.SxHalo(ell, min_members, max_groups, std=std, **kw)
        got = ctx.halos(ds.fields, sx.make_box(lim, bnd), spec, id=dev_id, labels=labels)
        return got, ctx.halo_stats()
    finally:
        ctx.free_all()


def run_fof(ctx, f, box, ell, ids=None, min_members=20):
    lim, bnd = box
    ds = sx.DeviceState(ctx, {k: np.asarray(v) for k, v in f.items()})
    try:
        dev_id = ctx.upload(np.ascontiguousarray(ids, dtype=np.uint64)) if ids is not None else None
        return ctx.fof(ds.fields, sx.make_box(lim, bnd), sx.SxFof(ell, min_members, 4096), id=dev_id)
    finally:
        ctx.free_all()


@functools.lru_cache(maxsize=None)
def clustered_case(name):
    """the clustered columns of test_gpu_fof.py in the box `name` with h and temp added, ids, the linking length"""
    box, outside = BOXES[name]
    f = fr.clustered(N, box=box, seed=7, outside=outside)
    rng = np.random.default_rng(17)
    f["h"] = rng.uniform(1e-4, 4e-3, N).astype(np.float32)
    f["temp"] = rng.uniform(0.5, 1.5, N) / CV
    ell = fr.mean_spacing_length(N, box)
    ids = np.random.default_rng(99).permutation(N).astype(np.uint64)
    return f, ids, ell


@functools.lru_cache(maxsize=None)
def clustered_oracle():
    """the oracle on the periodic case with ids, potential included; computed once and left unchanged"""
    f, ids, ell = clustered_case("periodic")
    return hr.halo(f, *fr.PERIODIC, ell, ids=ids, cv=CV)


@pytest.mark.parametrize("with_ids", [False, True], ids=["index", "id"])
@pytest.mark.parametrize("name", ["periodic", "open", "mixed"])
def test_without_a_cut_the_same_bits_as_fof(ctx, name, with_ids):
    box = BOXES[name][0]
    f, ids, ell = clustered_case(name)
    ids = ids if with_ids else None
    want = run_fof(ctx, f, box, ell, ids)
    assert want["num_groups"] >= 30
    got, _ = run(ctx, f, box, ell, ids, flags=ALL)
    for k in FOF_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert (got["num_groups"], got["num_all"]) == (want["num_groups"], want["num_all"])
    got, _ = run(ctx, f, box, ell, ids, flags=(), rho_min=-1.0)
    assert all(np.array_equal(got[k], want[k]) for k in FOF_KEYS) and got["epot"] is None and got["sigma"] is None


def test_moments_thermal_energy_and_potential(ctx):
    f, ids, ell = clustered_case("periodic")
    ref = clustered_oracle()
    assert ref["ties"] == 0, "the input has pairs on the criterion"
    assert ref["soft"].sum() > 1000 and ref["hard"].sum() > 1000, "both branches of r_eff occur inside groups"
    got, stats = run(ctx, f, fr.PERIODIC, ell, ids, flags=ALL)
    fr.assert_same(got, ref, fr.PERIODIC)
    about = hr.halo(f, *fr.PERIODIC, ell, ids=ids, cv=CV, about=got, potential=False)
    about["epot"] = ref["epot"]
    hr.assert_properties(got, about, thermal=True)
    assert stats["pair_terms"] == ref["pair_terms"] == int(np.sum(ref["count"].astype(np.int64) * (ref["count"].astype(np.int64) - 1) // 2))
    assert stats["with_epot"] == len(ref["count"]) and stats["over_cap"] == 0
    tiles = (ref["count"].astype(np.int64) + 255) // 256
    assert stats["pair_items"] == int(np.sum(tiles * (tiles + 1) // 2))
    # what Python derives
    assert np.array_equal(got["ekin"], 0.5 * got["mass"] * (got["sigma"][:, 0] + got["sigma"][:, 3] + got["sigma"][:, 5]))
    assert np.array_equal(got["alpha_vir"], 2.0 * got["ekin"] / np.abs(got["epot"]))
    assert np.array_equal(got["bound"], got["ekin"] + got["eint"] + got["epot"] < 0.0)
    assert got["axes"].shape == (len(ref["count"]), 3) and np.all(np.diff(got["axes"], axis=1) >= 0)
    assert np.allclose(got["axes"].sum(axis=1), got["shape"][:, [0, 3, 5]].sum(axis=1), rtol=1e-10)

    # the largest group uploaded alone (unwrapped about its centre): the direct sum in exact mode
    sel = np.flatnonzero(got["label"] == got["group_label"][0])
    assert len(sel) == got["count"][0] > 256
    alone = {k: f[k][sel] for k in ("m", "h")}
    for a, k in enumerate("xyz"):
        alone[k] = got["com"][0][a] + fr.min_image(f[k][sel] - got["com"][0][a], 1.0, True)
    ds = sx.DeviceState(ctx, alone)
    ctx.set_exact(True)
    try:
        n = len(sel)
        egrav, _ = ctx.gravity_direct(ds.fields, sx.SxGroups(firstBody=0, lastBody=n, numGroups=(n + 63) // 64), G=1.0)
    finally:
        ctx.set_exact(False)
        ctx.free_all()
    print("epot", got["epot"][0], "egrav", egrav, "relative", abs(got["epot"][0] - egrav) / abs(egrav))
    assert abs(got["epot"][0] - egrav) <= hr.CONTRACT * abs(egrav)


@functools.lru_cache(maxsize=None)
def tile_case():
    f, ell, sizes = hr.tile_edge_state()
    assert fr.near_ties([f[k] for k in "xyz"], *fr.PERIODIC, ell) == 0
    return f, ell, sizes, hr.halo(f, *fr.PERIODIC, ell, min_members=1)


def test_tile_edges(ctx):
    """groups of 1, 2, 255, 256, 257 and 513 members and one astride the corner of the periodic box"""
    f, ell, sizes, ref = tile_case()
    assert ref["count"].tolist() == sizes == [513, 257, 256, 255, 40, 2, 1]
    assert ref["soft"].sum() > 0 and ref["hard"].sum() > 0
    corner = 4
    assert np.ptp(f["x"][ref["label"] == ref["group_label"][corner]]) > 0.9, "the group of 40 wraps round the corner"
    got, stats = run(ctx, f, fr.PERIODIC, ell, min_members=1, flags=("moments", "potential"))
    fr.assert_same(got, ref, fr.PERIODIC)
    about = hr.halo(f, *fr.PERIODIC, ell, min_members=1, about=got, potential=False)
    about["epot"] = ref["epot"]
    hr.assert_properties(got, about)
    assert got["epot"][6] == 0.0 and got["epot"][5] < 0.0
    assert stats["pair_terms"] == sum(c * (c - 1) // 2 for c in sizes) == ref["pair_terms"]
    assert stats["pair_items"] == 6 + 3 + 1 + 1 + 1 + 1 + 1 and stats["with_epot"] == 7


def test_cap_on_the_pair_members(ctx):
    f, ell, sizes, ref = tile_case()
    free, _ = run(ctx, f, fr.PERIODIC, ell, min_members=1)
    got, stats = run(ctx, f, fr.PERIODIC, ell, min_members=1, max_pair_members=256)
    assert np.isnan(got["epot"][:2]).all() and stats["over_cap"] == 2 and stats["with_epot"] == 5
    assert np.array_equal(got["epot"][2:], free["epot"][2:]), "the others keep their bits"
    assert not np.isnan(got["epot"][2:]).any()
    for k in FOF_KEYS + ("sigma", "shape", "angmom", "rmax"):
        assert np.array_equal(got[k], free[k]), k
    assert stats["pair_terms"] == sum(c * (c - 1) // 2 for c in sizes[2:])
    capped = hr.halo(f, *fr.PERIODIC, ell, min_members=1, max_pair_members=256, potential=False)
    assert stats["pair_terms"] == capped["pair_terms"]


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_density_cut(ctx, std):
    f, ell, chain = hr.bridge_state(std=std)
    assert fr.near_ties([f[k] for k in "xyz"], *fr.OPEN, ell) == 0
    one, _ = run(ctx, f, fr.OPEN, ell, min_members=1, std=std)
    assert one["count"].tolist() == [141] and one["num_all"] == 1 and np.all(one["label"] == one["label"][0])
    ref = hr.halo(f, *fr.OPEN, ell, min_members=1, rho_min=5.0, std=std)
    got, stats = run(ctx, f, fr.OPEN, ell, min_members=1, rho_min=5.0, std=std)
    fr.assert_same(got, ref, fr.OPEN)
    assert got["count"].tolist() == [60, 60] and (got["num_groups"], got["num_all"]) == (2, 2)
    assert np.all(got["label"][chain] == hr.NONE) and np.all(got["label"][~chain] != hr.NONE)
    nan = np.isnan(hr.density(f, std))
    assert nan.sum() == 1 and got["label"][nan][0] == hr.NONE, "a NaN density is not selected"
    about = hr.halo(f, *fr.OPEN, ell, min_members=1, rho_min=5.0, std=std, about=got, potential=False)
    about["epot"] = ref["epot"]
    hr.assert_properties(got, about)
    assert stats["pair_terms"] == 2 * (60 * 59 // 2)
    # min_members counts selected particles only
    got, _ = run(ctx, f, fr.OPEN, ell, min_members=61, rho_min=5.0, std=std)
    assert (got["num_groups"], got["num_all"]) == (0, 2) and len(got["count"]) == 0

    # a cut above every density: no group, no launch over an empty catalogue
    got, stats = run(ctx, f, fr.OPEN, ell, min_members=1, rho_min=1e6, std=std)
    assert (got["num_groups"], got["num_all"]) == (0, 0) and len(got["count"]) == 0 and len(got["epot"]) == 0
    assert np.all(got["label"] == hr.NONE) and stats == dict(pair_terms=0, pair_items=0, with_epot=0, over_cap=0)


def test_missing_columns_are_refused(ctx):
    f, ell, _ = hr.bridge_state()

    def without(*names):
        def edit(fields):
            for k in names:
                setattr(fields, k, None)
        return edit

    with pytest.raises(sx.SxError, match="the density cut needs kx, xm and m, which this layout does not keep"):
        run(ctx, f, fr.OPEN, ell, rho_min=5.0, edit=without("kx"))
    with pytest.raises(sx.SxError, match="the density cut needs the rho column"):
        run(ctx, f, fr.OPEN, ell, rho_min=5.0, std=True, edit=without("rho"))
    with pytest.raises(sx.SxError, match="the thermal energy needs temp"):
        run(ctx, f, fr.OPEN, ell, flags=ALL, edit=without("temp"))
    with pytest.raises(sx.SxError, match="the potential needs h"):
        run(ctx, f, fr.OPEN, ell, edit=without("h"))
    with pytest.raises(sx.SxError, match="maxGroups is 0 with a catalogue array set"):
        run(ctx, f, fr.OPEN, ell, max_groups=0)
    with pytest.raises(sx.SxError, match="unknown flags 0x8"):
        run(ctx, f, fr.OPEN, ell, flags=8)
    # without a cut the density columns are not read
    got, _ = run(ctx, f, fr.OPEN, ell, min_members=1, edit=without("kx", "xm"))
    assert got["count"].tolist() == [141]


def bits(got):
    keys = ("group_label", "count", "mass", "com", "vel", "sigma", "shape", "angmom", "rmax", "eint", "epot")
    return [got[k].tobytes() for k in keys] + [got["num_groups"], got["num_all"]]


def test_same_bits_on_every_run_and_under_permutation(ctx):
    f, ids, ell = clustered_case("periodic")
    a, sa = run(ctx, f, fr.PERIODIC, ell, ids, flags=ALL)
    b, sb = run(ctx, f, fr.PERIODIC, ell, ids, flags=ALL)
    assert bits(a) == bits(b) and np.array_equal(a["label"], b["label"]) and sa == sb
    p = np.random.default_rng(5).permutation(N)
    c, sc = run(ctx, {k: v[p] for k, v in f.items()}, fr.PERIODIC, ell, ids[p], flags=ALL)
    assert bits(a) == bits(c), "with ids every array has the same bits under any permutation of the input"
    assert np.array_equal(a["label"][p], c["label"]) and sa == sc
    f, ell, _, _ = tile_case()
    n = len(f["x"])
    ids = np.random.default_rng(6).permutation(n).astype(np.uint64)
    a, _ = run(ctx, f, fr.PERIODIC, ell, ids, min_members=1)
    p = np.random.default_rng(7).permutation(n)
    c, _ = run(ctx, {k: v[p] for k, v in f.items()}, fr.PERIODIC, ell, ids[p], min_members=1)
    assert all(np.array_equal(a[k], c[k]) for k in ("count", "mass", "com", "vel", "sigma", "shape", "angmom", "rmax", "epot"))


def test_arrays_whose_flag_is_clear_or_pointer_null_are_not_written(ctx):
    f, ell, _, _ = tile_case()
    n, cap, mark = len(f["x"]), 16, -7.0
    ds = sx.DeviceState(ctx, f)
    try:
        names = {"groupSigma": 6, "groupShape": 6, "groupAngmom": 3, "groupRmax": 1, "groupEint": 1, "groupEpot": 1}
        flag = {"groupSigma": 1, "groupShape": 1, "groupAngmom": 1, "groupRmax": 1, "groupEint": 2, "groupEpot": 4}
        for flags, absent in ((4, ()), (1, ("groupShape",)), (0, ()), (2, ("groupEint",)), (7, ())):
            dev = {k: ctx.upload(np.full(cap * w, mark)) for k, w in names.items()}
            num = ctx.upload(np.zeros(2, np.uint64))
            res = sx.SxHaloResult(numGroups=num.ptr, **{k: d.ptr for k, d in dev.items() if k not in absent})
            spec = sx.SxHalo(ell, 1, cap, flags=flags)
            ctx.check(ctx.L.sx_halo_compute(ctx.h, C.byref(ds.fields), C.byref(sx.make_box(*fr.PERIODIC)), 0, n, None,
                                            C.byref(spec), C.byref(res)), "sx_halo_compute")
            assert num.get().tolist() == [7, 7]
            for k, d in dev.items():
                v = d.get()
                if flags & flag[k] and k not in absent:
                    assert np.all(v[:7 * names[k]] != mark) and np.all(v[7 * names[k]:] == mark), (flags, k)
                else:
                    assert np.all(v == mark), (flags, k)
    finally:
        ctx.free_all()


def test_fof_profile_and_halos_on_one_context_keep_apart(ctx):
    f, ids, ell = clustered_case("periodic")
    box = sx.make_box(*fr.PERIODIC)
    ds = sx.DeviceState(ctx, f)
    try:
        pspec = sx.SxProfile(edges=np.linspace(0.0, 0.5, 9), quantities=("vel",), center=(0.5, 0.5, 0.5))
        groups = ctx.fof(ds.fields, box, sx.SxFof(ell, 20, 4096))
        prof = ctx.profile(ds.fields, box, pspec)
        pstats = ctx.profile_stats()
        halos = ctx.halos(ds.fields, box, sx.SxHalo(ell, 20, 4096))
        hstats = ctx.halo_stats()
        assert all(np.array_equal(halos[k], groups[k]) for k in FOF_KEYS)
        assert ctx.profile_stats() == pstats
        # a smaller search in between reuses the search's buffers and leaves the properties' figures alone
        small = ctx.fof(ds.fields, box, sx.SxFof(0.5 * ell, 20, 4096))
        assert small["num_groups"] != groups["num_groups"] and ctx.halo_stats() == hstats
        prof2 = ctx.profile(ds.fields, box, pspec)
        assert all(np.array_equal(prof[k], prof2[k]) for k in prof)
        again = ctx.halos(ds.fields, box, sx.SxHalo(ell, 20, 4096))
        assert bits(dict(again, eint=np.zeros(0))) == bits(dict(halos, eint=np.zeros(0))) and ctx.halo_stats() == hstats
        assert all(np.array_equal(ctx.fof(ds.fields, box, sx.SxFof(ell, 20, 4096))[k], groups[k]) for k in FOF_KEYS)
    finally:
        ctx.free_all()
