"""The inputs of tests/gravity_cases.py have teeth, and the bounds the GPU tests hold the kernels to can be met:

* every case is pinned by its size and a few exact values;
* a float P2P whose displacements are formed in double and rounded once (sum in double) stays within 1e-5 S_i on every
  case (S_i: direct_ref.direct's sum of absolute terms of target i);
* the same P2P with both coordinates rounded relative to a far origin exceeds 1e-4 S_i on the clumps and stays under
  1e-6 S_i on the Evrard sphere -- the cases must not drift into something every scheme passes;
* the oracle's walk at theta = 0.5 is finite on every open case and agrees with the direct sum in the median to 1e-2,
  the figure of test_oracle_gravity.py.  On `massless` it is not finite for the one body at the
  origin (recorded below); the GPU tests compare that body with direct_ref alone.
"""
import numpy as np
import pytest

import gravity_cases as gc
import pyoracle as po
from sphexa_amd import ic

OPEN_CASES = list(gc.CASES)


def named(name):
    if name == "periodic":
        return gc.periodic()
    if name.startswith("picks"):
        return gc.picks(int(name[5:]))
    return gc.case(name)


def sample(name, n):
    """the bodies a case adds to its halo and every fourth of the others"""
    extra = gc.CASES.get(name, (None, gc.CLUMPS * gc.CLUMP_SIZE if name == "periodic" else 0))[1]
    return np.unique(np.concatenate([np.arange(0, n, 4), np.arange(n - min(extra, n), n)]))


def test_cases_are_pinned():
    sizes = {name: gc.case(name)[0]["x"].size for name in gc.CASES}
    assert sizes == {"halo_clumps_1e-2": 4288, "halo_clumps_1e-3": 4288, "halo_clumps_1e-4": 4288, "mass_ratio": 4096,
                     "massless": 4359, "coincident": 4096, "off_origin": 4288, "deep_uniform": 4096}
    for name in gc.CASES:
        f, lim, bnd = gc.case(name)
        assert f["x"].dtype == f["y"].dtype == f["z"].dtype == np.float64
        assert f["m"].dtype == f["h"].dtype == np.float32
        for a, c in enumerate("xyz"):
            assert np.all(f[c] >= lim[2 * a]) and np.all(f[c] < lim[2 * a + 1]), (name, c)
        assert np.all(f["h"] > 0) and np.all(f["m"] >= 0)
    f, lim, bnd = gc.case("halo_clumps_1e-3")
    assert f["m"][0] == np.float32(1.0 / 4096) and np.all(f["m"] == f["m"][0])
    assert np.all(f["h"][:4096] == np.float32(1.0 / 16)) and np.all(f["h"][4096:] == np.float32(1e-3 / 8))
    r = np.sqrt(f["x"] ** 2 + f["y"] ** 2 + f["z"] ** 2)
    assert np.min(r[4096:]) > np.sort(r[:4096])[-gc.OUTER] - 1e-2  # the clumps sit on the outermost bodies
    clump = np.stack([f[c][4096:].reshape(gc.CLUMPS, gc.CLUMP_SIZE) for c in "xyz"])
    assert 0.5e-3 < clump.std(axis=2).mean() < 1.5e-3
    f, lim, bnd = gc.case("mass_ratio")
    m = f["m"].astype(np.float64)
    assert abs(m.sum() - 1.0) < 1e-6 and m.max() == np.float32(0.9) and m[m > 0].min() < 2e-6 * 0.1
    big = int(np.argmax(m))
    assert 0.9 < np.sqrt(f["x"][big] ** 2 + f["y"][big] ** 2 + f["z"][big] ** 2) < 1.1
    f, lim, bnd = gc.case("massless")
    assert np.count_nonzero(f["m"] == 0) == gc.MASSLESS_GROUP
    assert (f["x"][-1], f["y"][-1], f["z"][-1]) == (0.0, 0.0, 0.0) and f["m"][-1] > 0
    f, lim, bnd = gc.case("coincident")
    for a, b in ((10, 11), (2000, 3000)):
        assert all(f[c][a] == f[c][b] for c in "xyz")
    u = (f["x"][100:116] - lim[0]) / (lim[1] - lim[0]) * 128
    assert np.all(u == np.round(u)) and f["x"][200] == lim[0] and f["y"][201] == lim[2] and f["z"][202] == lim[4]
    f, lim, bnd = gc.case("off_origin")
    g = gc.case("halo_clumps_1e-3")[0]
    assert np.array_equal(f["x"], g["x"] + 1024.0) and lim[:2] == [1012.0, 1036.0] and lim[2:4] == [-2060.0, -2036.0]
    f, lim, bnd = gc.periodic()
    assert bnd == [1, 1, 1] and lim == [0.0, 1.0] * 3 and f["x"].min() >= 0 and f["x"].max() < 1
    for n in gc.PICKS:
        assert gc.picks(n)[0]["x"].size == n


@pytest.mark.parametrize("name", OPEN_CASES + ["periodic", "picks129"])
def test_displacement_rounded_once_meets_the_bound(name):
    """here: at most 1.7e-7 S_i"""
    f, lim, bnd = named(name)
    t = sample(name, f["x"].size)
    ref, S = gc.direct(f, targets=t)
    err = np.max(np.abs(gc.displacement_rounded_once(f, t) - ref[:, 1:]) / (S[:, 1:] + 1e-300))
    print(name, "float displacements rounded once: max error / S_i =", err)
    assert err <= 1e-5


def test_origin_rounding_fails_on_the_clumps_and_passes_on_the_smooth_sphere():
    f, lim, bnd = gc.case("halo_clumps_1e-3")
    o = gc.morton_order(f, lim)
    pos = np.empty_like(o)
    pos[o] = np.arange(o.size)
    runs = np.unique(pos[4096:] // 64)  # the runs of 64 that hold a clump body
    t, a = gc.origin_rounded(f, o, runs)
    ref, S = gc.direct(f, targets=t)
    err = np.abs(a - ref[:, 1:]) / S[:, 1:]
    print("halo_clumps_1e-3, origin-rounded model: max error / S_i =", err.max(), "targets above 1e-5:",
          int((err.max(axis=1) > 1e-5).sum()), "of", t.size)
    assert err.max() > 1e-4

    arr, elim, ebnd, _ = ic.evrard(20)
    e = {k: np.asarray(arr[k]) for k in ("x", "y", "z", "m", "h")}
    o = gc.morton_order(e, elim)
    t, a = gc.origin_rounded(e, o, range(0, (o.size + 63) // 64, 3))
    ref, S = gc.direct(e, targets=t)
    err = np.max(np.abs(a - ref[:, 1:]) / S[:, 1:])
    print("evrard(20), origin-rounded model: max error / S_i =", err)
    assert err < 1e-6


@pytest.mark.parametrize("name", OPEN_CASES)
def test_oracle_walk_is_finite_and_close_to_the_direct_sum(name):
    ora = po.load_oracle()
    f, lim, bnd = gc.case(name)
    st, box = gc.oracle_state(f, lim, bnd, ora)
    eg, cen, mp = ora.gravity(st, box, ora.params(g=1.0, theta=0.5))
    a = np.column_stack([st.ax, st.ay, st.az]).astype(np.float64)
    assert np.all(np.isfinite(cen)) and np.all(np.isfinite(mp))
    bad = np.flatnonzero(~np.all(np.isfinite(a), axis=1))
    if name == "massless":
        # recorded: the oracle, like the reference it is pinned to, evaluates the M2P of the empty nodes, whose
        # expansion centre is (0, 0, 0): 0 * inf for the body that sits there.  Every other target is finite.  The GPU
        # tests therefore compare that body with direct_ref alone.
        assert list(st.order[bad]) == [st.n - 1] and not np.isfinite(eg)
    else:
        assert bad.size == 0 and np.isfinite(eg)
    t = np.setdiff1d(np.arange(0, st.n, 4), bad)
    ref, S = gc.direct(gc.fields_of(st), targets=t)
    norm = np.sqrt(np.sum(ref[:, 1:] ** 2, axis=1))
    rel = np.sqrt(np.sum((a[t] - ref[:, 1:]) ** 2, axis=1)) / np.where(norm > 0, norm, 1.0)
    print(name, "oracle walk, theta 0.5: median relative error", np.median(rel), "max", rel.max())
    assert np.median(rel) < 1e-2
