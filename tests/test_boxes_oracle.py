"""The oracle restatement against the live reference build (oracle/_ref) in the boxes of box_cases.py: non-cubic,
off-origin, and with periodic, open and fixed axes in one box.  test_oracle_vs_ref.py pins the oracle only in the cube
[-0.5, 0.5]^3; the per-axis arithmetic (keys normalised by each axis' own inverse length, node centres and sizes,
the minimum image, putInBox and the fixed-boundary skip) must agree bit for bit here as well.

Runs only where oracle/_ref/libsphexa_ref.so exists; tests/golden/boxes.npz (test_oracle_golden.py) carries two small
variants to the machines without it.
"""
import numpy as np
import pytest

import box_cases as bc
import pyoracle as po

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref not built")]

NAMES = list(bc.CASES)


@pytest.fixture(scope="module")
def ref():
    return po.load_ref()


@pytest.fixture(scope="module")
def ora():
    return po.load_oracle()


@pytest.mark.parametrize("name", NAMES)
def test_keys_tree_neighbors(ora, ref, name):
    """keys (with the limit particles), octree at buckets 64 and 1, node geometry, find_neighbors with and without
    the h iteration"""
    st, box = bc.state(name)
    full = bc.with_edges(st, box)
    keys = ref.sfc_keys(full, box).copy()
    assert np.array_equal(keys, ora.sfc_keys(full, box))
    # a particle on an upper limit lands in the last cell: the key of the particle a nextafter below it
    ek = keys[st.n:]
    for d in range(3):
        assert ek[3 * d + 1] == ek[3 * d + 2], (name, d)
    assert ek[10] == ek[11]
    skeys = np.sort(keys)
    for bucket in (64, 1):
        t1, t2 = ref.octree(skeys, bucket), ora.octree(skeys, bucket)
        for k in t1:
            assert np.array_equal(t1[k], t2[k]), (bucket, k)
        c1, s1 = ref.node_centers(t1["prefixes"], box)
        c2, s2 = ora.node_centers(t2["prefixes"], box)
        assert np.array_equal(c1, c2) and np.array_equal(s1, s2), bucket
    bc.sort_by_key(st, box, ref)
    h0 = st.h.copy()
    for it, hh in ((False, h0), (True, h0), (True, (h0 * np.float32(1.35)).astype(np.float32))):
        st.h[:] = hh
        n1, c1 = ref.find_neighbors(st, box, iterate_h=it)
        h1 = st.h.copy()
        st.h[:] = hh
        n2, c2 = ora.find_neighbors(st, box, iterate_h=it)
        assert np.array_equal(c1, c2) and np.array_equal(n1, n2) and np.array_equal(h1, st.h), it


STEP_RUNS = [(n, "ve") for n in NAMES] + [("mixed", "avclean"), ("windshock", "std")]


@pytest.mark.parametrize("name,prop", STEP_RUNS, ids=[f"{n}-{p}" for n, p in STEP_RUNS])
def test_two_steps(ora, ref, name, prop):
    st, box = bc.state(name)
    g = bc.CASES[name]["g"]
    kw = dict(av_clean=(prop == "avclean"), std=(prop == "std"), g=g)
    pr, pq = ref.params(**kw), ora.params(**kw)
    a, b = st.copy(), st.copy()
    for s in range(2):
        ref.step(a, box, params=pr)
        ora.step(b, box, params=pq)
        for k in a.arrays:
            assert np.array_equal(a.arrays[k], b.arrays[k]), (s, k)
        assert a.minDt == b.minDt and a.ttot == b.ttot
        if g:
            assert b.egrav == pytest.approx(a.egrav, rel=1e-12) and a.egrav < 0
    assert np.any(b.ax != 0) and not np.array_equal(b.x, st.x)
