"""The profile oracle (tests/profile_ref.py) pinned to what the project already trusts (CPU): the binned means and
counts of oracle/trajectory.py, its analytic L1 against the Sedov table and the Noh closed form, and math.fsum.

Bounds.  trajectory.profiles sums a bin's n_b values of q with np.bincount, a sequential double sum whose error is at
most n_b 2^-53 sum |q|; the exact side adds less than one rounding.  Doubled for the final rounding of either side:
|S1 - bincount sum| <= n_b 2^-52 sum |q|.  analytic_l1 sums the N deviations with np.sum (pairwise, so the sequential
bound holds a fortiori): N 2^-52 sum |q - s| / N, plus 4 ulp of the larger of |s| and |q| per term for np.interp's
own rounding of s, which may differ from the header's bracketing.
"""
import math
import os

import numpy as np
import pytest

import profile_ref as pr
import pyoracle as po
import trajectory as tj

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -52


def state(which):
    st, box = (po.sedov_state if which == "sedov" else po.noh_state)(10)
    rng = np.random.default_rng(11)
    f = {k: v.copy() for k, v in st.arrays.items()}
    n = st.n
    for k in ("vx", "vy", "vz"):
        f[k] = (f[k] + 0.3 * rng.standard_normal(n)).astype(np.float32)
    f["temp"] = (f["temp"] + 1e-15) * rng.uniform(0.5, 2.0, n)
    # the EOS inputs of a state that has seen a density pass: kx m / xm about 1
    f["xm"] = (f["m"] * rng.uniform(0.8, 1.25, n)).astype(np.float32)
    f["kx"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    return f, list(box.lim), list(box.bnd)


@pytest.fixture(scope="module", params=["sedov", "noh"])
def case(request):
    f, lim, bnd = state(request.param)
    nbins, rmax = 7, 0.5
    edges, means, cnt = tj.profiles(f, rmax, nbins)
    res = pr.profile(f, lim, bnd, edges, ("rho", "p", "vel", "u"))
    return request.param, f, lim, bnd, edges, means, cnt, res


def test_radius_equals_trajectory_radii(case):
    _, f, lim, bnd, *_ = case
    c, *_ = pr.evaluate(f, lim, bnd, ())
    assert np.array_equal(c.view(np.uint64), tj.radii(f).view(np.uint64))  # centre 0: no min-image shift inside the box


def test_counts_and_means_equal_trajectory_profiles(case):
    _, f, lim, bnd, edges, means, cnt, res = case
    nb = len(edges) - 1
    assert np.array_equal(res["count"][:nb], cnt.astype(np.uint64))
    assert int(res["count"].sum()) + int(res["nonfinite"][0]) == f["x"].size and res["count"][nb] == 0
    rho, p = tj.eos_rho_p(f)
    r = tj.radii(f)
    b = np.searchsorted(edges, r, side="right") - 1
    qs = {"rho": rho.astype(np.float64), "p": p.astype(np.float64),
          "vel": np.sqrt(sum(np.asarray(f[k], np.float64) ** 2 for k in ("vx", "vy", "vz"))),
          "u": np.float64(po.ideal_gas_cv()) * f["temp"]}
    for k, name in enumerate(("rho", "p", "vel", "u")):
        for bin_ in range(nb):
            q = qs[name][b == bin_]
            seq = means[name][bin_] * cnt[bin_]  # the bincount sum back from the mean: one more rounding each way
            bound = q.size * U * np.sum(np.abs(q)) + 2 * U * abs(seq)
            assert abs(res["S1"][k][bin_] - seq) <= bound, (name, bin_)
            assert res["min"][k][bin_] == q.min(initial=np.inf) and res["max"][k][bin_] == q.max(initial=-np.inf)
            if cnt[bin_]:
                assert abs(res["S1"][k][bin_] / res["W"][bin_] - means[name][bin_]) <= bound / cnt[bin_]
    assert np.array_equal(res["W"][:nb], cnt)


def test_sedov_l1_equals_analytic_l1():
    f, lim, bnd = state("sedov")
    sol = np.load(os.path.join(GOLDEN, "traj_sedov50.npz"))["sol"]
    rho, _ = tj.eos_rho_p(f)
    for rscale in (1.0, 0.37):
        res = pr.profile(f, lim, bnd, np.linspace(0.0, 0.5, 6), ("rho",),
                         solutions={"rho": ("table", sol[:, 0], sol[:, 1], rscale)})
        ref = tj.analytic_l1(tj.radii(f) * rscale, rho.astype(np.float64), sol[:, 0], sol[:, 1])
        s = np.interp(tj.radii(f) * rscale, sol[:, 0], sol[:, 1])
        dev = np.abs(s - rho)
        bound = rho.size * U * dev.sum() / rho.size + 4 * U * np.sum(np.maximum(np.abs(s), rho)) / rho.size
        assert abs(pr.l1(res) - ref) <= bound, (pr.l1(res), ref, bound)
        assert pr.l1(res) > 0.1  # a real distance: the state is not the solution


def test_noh_l1_equals_noh_l1():
    f, lim, bnd = state("noh")
    rho, _ = tj.eos_rho_p(f)
    for t, rho0 in ((0.3, tj.NOH_RHO0_ATTR), (0.6, tj.NOH_RHO0_IC)):
        r = tj.radii(f)
        assert (r > 0.5 * (5.0 / 3.0 - 1) * t).any() and (r <= 0.5 * (5.0 / 3.0 - 1) * t).any()  # both sides of the front
        res = pr.profile(f, lim, bnd, np.linspace(0.0, 0.5, 6), ("rho",),
                         solutions={"rho": ("noh", dict(time=t, rho0=rho0))})
        ref = tj.noh_l1(f, t, rho0)
        s = tj.noh_rho(r, t, rho0=rho0)
        bound = rho.size * U * np.sum(np.abs(s - rho)) / rho.size + 4 * U * np.sum(np.maximum(np.abs(s), rho)) / rho.size
        assert abs(pr.l1(res) - ref) <= bound, (pr.l1(res), ref, bound)


def test_exact_sum_equals_fsum():
    rng = np.random.default_rng(3)
    t = rng.standard_normal(20000) * 10.0 ** rng.uniform(-12, 12, 20000)
    assert pr.exact_sum(t) == math.fsum(t)
    # the vectorised per-bin sums are the same integers
    bins = rng.integers(0, 5, t.size)
    E = pr.window(t)
    got = pr.exact_bin_sums(t, bins, 5)
    for b in range(5):
        assert got[b] == pr.from_fixed(sum(pr.to_fixed(v, E) for v in t[bins == b]), E)
