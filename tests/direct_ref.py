"""The direct gravity sum restated in float64 numpy (ryoanji::directSum, nbody/traversal_cpu.hpp:234-270, with the P2P
of kernel.hpp:514-535), the inputs of the committed fixture tests/golden/direct_ref.npz and the bound for a re-ordered
sum.  tests/test_direct_ref.py pins the restatement and the fixture to the reference's own function; the GPU tests
import this module and need neither the reference nor a compiler.

Fixture inputs (fixed seeds): positions uniform in [-0.5, 0.5)^3 and deliberately not SFC-sorted, m = U(0.5, 1.5) / n
as float, h = k 2^-12 with an integer k in [64, 256] -- h_i + h_j is then exact in float, so the reference harness's
double h and the device's float h give the same R_eff^2 -- G = 1, L = 1.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "direct_ref.npz")
G, L = np.float32(1.0), 1.0
#: name -> (key of the inputs, n, seed, image shells)
CASES = {"n1000_s0": ("n1000", 1000, 20250101, 0), "n1000_s1": ("n1000", 1000, 20250101, 1),
         "n300_s2": ("n300", 300, 20250102, 2)}


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    f = {k: rng.uniform(-0.5, 0.5, n) for k in "xyz"}
    f["m"] = (rng.uniform(0.5, 1.5, n) / n).astype(np.float32)
    f["h"] = (rng.integers(64, 257, n).astype(np.float64) * 2.0 ** -12).astype(np.float32)
    return f


def case_inputs(case):
    key, n, seed, shells = CASES[case]
    return inputs(n, seed), shells


def direct(f, shells, G=G, L=L, targets=None):
    """(out4, scale): out4[i] = {G m_i phi_i, G ax, G ay, G az} of target i as the reference's CPU function returns
    them (zero-initialised outputs), summed per image with numpy's pairwise sums; scale[i] = {G m_i sum m_j R^2 /
    R_eff^3, S_i, S_i, S_i} with S_i = G sum_images sum_j m_j R / R_eff^3, the sums of the absolute terms"""
    x, y, z = (np.asarray(f[k], np.float64) for k in "xyz")
    m32, h32 = np.asarray(f["m"], np.float32), np.asarray(f["h"], np.float32)
    n = x.size
    t = np.arange(n) if targets is None else np.asarray(targets)
    acc, sabs = np.zeros((t.size, 4)), np.zeros((t.size, 2))
    hij = h32[t, None] + h32[None, :]                     # float, as the walk's p2p forms it
    hij2 = (hij * hij).astype(np.float64)
    md = m32.astype(np.float64)[None, :]
    for iz in range(-shells, shells + 1):
        for iy in range(-shells, shells + 1):
            for ix in range(-shells, shells + 1):
                dx = x[None, :] - (x[t] + ix * L)[:, None]
                dy = y[None, :] - (y[t] + iy * L)[:, None]
                dz = z[None, :] - (z[t] + iz * L)[:, None]
                r2 = dx * dx + (dy * dy + dz * dz)
                r2eff = np.where(r2 < hij2, hij2, r2)
                inv_r = 1.0 / np.sqrt(r2eff)
                inv_r3m = md * inv_r * (inv_r * inv_r)
                acc[:, 0] -= np.sum(inv_r3m * r2, axis=1)
                acc[:, 1] += np.sum(dx * inv_r3m, axis=1)
                acc[:, 2] += np.sum(dy * inv_r3m, axis=1)
                acc[:, 3] += np.sum(dz * inv_r3m, axis=1)
                sabs[:, 0] += np.sum(inv_r3m * r2, axis=1)
                sabs[:, 1] += np.sum(inv_r3m * np.sqrt(r2), axis=1)
    g = np.float64(np.float32(G))
    gm = (np.float32(G) * m32[t]).astype(np.float64)      # G * m[t] is a float product in the reference
    out4 = np.column_stack([gm * acc[:, 0], g * acc[:, 1], g * acc[:, 2], g * acc[:, 3]])
    scale = np.column_stack([gm * sabs[:, 0], g * sabs[:, 1], g * sabs[:, 1], g * sabs[:, 1]])
    return out4, scale


def reorder_bound(n, shells, scale):
    """two orders of the same n (2 shells + 1)^3 terms differ by at most 2 (N - 1) 2^-53 sum|term| <= N 2^-52 sum|term|
    (|a component's term| <= m_j R / R_eff^3); the output stage's one multiplication by G is common to both"""
    return n * (2 * shells + 1) ** 3 * 2.0 ** -52 * scale


def load_fixture():
    """{case: (inputs, shells, out4 of the reference)}"""
    out = {}
    with np.load(FIXTURE) as z:
        for case, (key, n, seed, shells) in CASES.items():
            f = {k: z[f"{key}_{k}"] for k in ("x", "y", "z", "m", "h")}
            out[case] = (f, shells, z[f"{case}_out4"])
    return out
