"""Oracle of the power spectra (sx_mesh_deposit, sx_fft3d, sx_shell_sums, sx_spectrum_compute): plain numpy in double.

Box and mesh: periodic cubic box of edge L, n^3 cells of size D = L / n, cell (ix, iy, iz) centred at
lim_lo + (i + 1/2) D per axis, arrays indexed [iz][iy][ix].
Deposit: S0(c) = sum_j m_j K W(r_jc / he_j) / he_j^3 with W(q) = sinc(pi q / 2)^6 evaluated with sin, r the minimum-image
distance to the cell centre, he_j = max(h_j, D / 2); S1_a(c) = sum_j w_jc a_j.
Field: W_a = S0^p S1_a / S0 (0 where S0 = 0).  Transform: What(n) = n^-3 sum_c W(c) exp(-2 pi i n.c / n) through
np.fft.fftn.  Shells: s = floor(|n| + 1/2) for n_i in [-n/2, n/2), numShells = floor(sqrt(3) n / 2 + 1/2) + 1,
power[s] = prefactor sum_a sum_{n in s} |What_a(n)|^2.
Nothing here shares code with the library: distances are minimum-image per cell and axis, whatever the block logic of the
kernels does, and the shell of a wave vector is decided in integers.
"""
import numpy as np

from map_ref import kernel_constant, kernel_w  # noqa: F401  (the same W and K as the maps' oracle)

VELOCITY, SCALAR = 0, 1
POWERS = {0: 0.0, 1: 0.5, 2: 1.0 / 3.0}


def mesh(pos, h, m, lim, n, K=None, a=None, clamp=True, scales=False):
    """pos: (np, 3); a: None or (np, k) columns.  Returns a dict: sum0 (n, n, n), sum1 and abs1 = sum |w a| (k, n, n, n),
    count (contributions per cell: particles whose support contains the cell centre), hits (np: the cells each particle
    contributes to) and, with scales=True, the first-order sensitivities to the distances dq0 = sum_j |d w_j / d q_j|
    (q the distance in units of he) and dq1 = sum_j |a_j d w_j / d q_j| (central differences of the same kernel)."""
    K = kernel_constant() if K is None else K
    pos = np.asarray(pos, np.float64)
    h = np.asarray(h, np.float64)
    m = np.asarray(m, np.float64)
    a = None if a is None else np.asarray(a, np.float64).reshape(len(h), -1)
    k = 0 if a is None else a.shape[1]
    L = lim[1] - lim[0]
    D = L / n
    centre = [lim[2 * ax] + (np.arange(n) + 0.5) * D for ax in range(3)]
    out = {"sum0": np.zeros((n, n, n)), "dq0": np.zeros((n, n, n)), "count": np.zeros((n, n, n), np.int64),
           "sum1": np.zeros((k, n, n, n)), "abs1": np.zeros((k, n, n, n)), "dq1": np.zeros((k, n, n, n)),
           "hits": np.zeros(len(h), np.int64)}
    for j in range(len(h)):
        he = max(h[j], 0.5 * D) if clamp else h[j]
        reach2 = 4.0 * he * he
        e = [pos[j, ax] - centre[ax] for ax in range(3)]
        e = [d - L * np.rint(d / L) for d in e]
        ix, iy, iz = (np.nonzero(d * d < reach2)[0] for d in e)
        if ix.size == 0 or iy.size == 0 or iz.size == 0:
            continue
        r2 = e[2][iz][:, None, None] ** 2 + e[1][iy][None, :, None] ** 2 + e[0][ix][None, None, :] ** 2
        t = r2 / (he * he)
        inside = t < 4.0
        q = np.sqrt(t)
        w = np.where(inside, m[j] * K * kernel_w(q) / he ** 3, 0.0)
        sl = np.ix_(iz, iy, ix)
        out["sum0"][sl] += w
        out["count"][sl] += inside
        out["hits"][j] = int(inside.sum())
        if scales:
            eps = 1e-5
            lo = np.maximum(q - eps, 0.0)
            dw = np.abs(m[j] * K * (kernel_w(q + eps) - kernel_w(lo)) / he ** 3) / (q + eps - lo)
            out["dq0"][sl] += dw
        for c in range(k):
            out["sum1"][c][sl] += w * a[j, c]
            out["abs1"][c][sl] += np.abs(w * a[j, c])
            if scales:
                out["dq1"][c][sl] += dw * abs(a[j, c])
    return out


def num_shells(n):
    return int(np.floor(np.sqrt(3.0) * n / 2 + 0.5)) + 1


def shell_index(n):
    """(n, n, n) integers [iz][iy][ix] in the transform's layout: index i is the wave number i for i < n / 2, i - n else"""
    k = np.where(np.arange(n) < n // 2, np.arange(n), np.arange(n) - n).astype(np.int64)
    k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, :] ** 2
    s = np.floor(np.sqrt(k2.astype(np.float64)) + 0.5).astype(np.int64)
    # in integers: s (s - 1) < k2 <= s (s + 1)
    s = np.where((s > 0) & (s * (s - 1) >= k2), s - 1, s)
    s = np.where(k2 > s * (s + 1), s + 1, s)
    assert ((s * (s - 1) < k2) | (k2 == 0)).all() and (k2 <= s * (s + 1)).all()
    return s


def shells(n):
    """(shell of every mode, modes per shell as uint64)"""
    s = shell_index(n)
    return s, np.bincount(s.ravel(), minlength=num_shells(n)).astype(np.uint64)


def field(s0, s1, weight):
    """W_a = S0^p S1_a / S0, 0 where S0 = 0"""
    p = POWERS[weight]
    ok = s0 > 0
    f = np.zeros_like(s0)
    f[ok] = s0[ok] ** p / s0[ok]
    return s1 * f


def spectrum(W, n, prefactor=1.0):
    """W: (A, n, n, n) real or complex fields.  Returns (power per shell, modes per shell)."""
    W = np.asarray(W).reshape(-1, n, n, n)
    s, modes = shells(n)
    p2 = np.zeros((n, n, n))
    for w in W:
        what = np.fft.fftn(w) / float(n) ** 3
        p2 += what.real ** 2 + what.imag ** 2
    return prefactor * np.bincount(s.ravel(), weights=p2.ravel(), minlength=modes.size), modes


def lattice(side, ng0=100, jitter=0.2, seed=3):
    """side^3 particles on a jittered lattice of the unit box with the h of ng0 neighbours and equal masses"""
    rng = np.random.default_rng(seed)
    g = (np.arange(side) + 0.5) / side
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = (pos + rng.uniform(-jitter, jitter, pos.shape) / side) % 1.0
    npart = side ** 3
    h = np.full(npart, 0.5 * (3.0 * ng0 / (4.0 * np.pi * npart)) ** (1.0 / 3.0), np.float32)
    h *= rng.uniform(0.95, 1.05, npart).astype(np.float32)
    m = np.full(npart, 1.0 / npart, np.float32)
    return pos, h, m


def shear_velocity(pos, L=1.0):
    """0.7 sin(2 pi 3 y / L) x^ + 0.35 cos(2 pi 2 x / L) z^: power in shells 3 and 2"""
    v = np.zeros_like(pos)
    v[:, 0] = 0.7 * np.sin(2 * np.pi * 3 * pos[:, 1] / L)
    v[:, 2] = 0.35 * np.cos(2 * np.pi * 2 * pos[:, 0] / L)
    return v
