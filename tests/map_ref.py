"""Oracle of the column-density and slice maps (sx_map_render): plain numpy in double, a loop over the particles and the
pixels each one reaches.

The line-of-sight kernel Y(q) = 2 int_0^sqrt(4 - q^2) W(sqrt(q^2 + s^2)) ds is a 200-node Gauss-Legendre quadrature and
W(q) = sinc(pi q / 2)^6 is evaluated with sin, so the device's polynomials are tested too.  Nothing here shares code with
the library: distances are minimum-image per pixel and axis, whatever the footprint logic of the kernels does.
"""
import numpy as np

_XG, _WG = np.polynomial.legendre.leggauss(200)
COLUMN, SLICE = 0, 1


def kernel_w(q):
    """W(q) = sinc(pi q / 2)^6, 0 for q >= 2"""
    q = np.asarray(q, np.float64)
    a = 0.5 * np.pi * q
    s = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return np.where(q < 2.0, s ** 6, 0.0)


def kernel_y(t):
    """Y as a function of t = q^2 (any shape), 0 for t >= 4"""
    t = np.asarray(t, np.float64)
    flat = t.reshape(-1)
    smax = np.sqrt(np.maximum(4.0 - flat, 0.0))
    s = 0.5 * smax[:, None] * (_XG[None, :] + 1.0)
    y = 2.0 * np.sum(0.5 * smax[:, None] * _WG[None, :] * kernel_w(np.sqrt(flat[:, None] + s * s)), axis=1)
    return y.reshape(t.shape)


def kernel_constant():
    """K with K int W 4 pi q^2 dq = 1 (Gauss-Legendre; the library's Simpson value agrees to 1e-9)"""
    xq, wq = np.polynomial.legendre.leggauss(400)
    q = 1.0 + xq
    return 1.0 / np.sum(wq * kernel_w(q) * 4.0 * np.pi * q * q)


def _min_image(d, L):
    return d - L * np.rint(d / L) if L > 0.0 else d


def render(pos, h, m, lim, bnd, kind, axis, center, width, npix, depth=0.0, K=None, a=None, clamp=True, scales=False):
    """pos: (n, 3).  Returns a dict of (npix[1], npix[0]) arrays: sum0, sum1 (zeros without a), count (contributions per
    pixel: particles whose support contains the pixel centre) and abs1 = sum |w_j a_j|; hits (n): the pixels each
    particle contributes to; and, with scales=True, the first-order sensitivities of the sums to the geometry:
    dq0 = sum_j |d w_j / d q_j| (q the distance in units of he, in the plane for a column, in space for a slice) and
    dq1 = sum_j |a_j d w_j / d q_j| (central differences of the same kernels)."""
    K = kernel_constant() if K is None else K
    pos = np.asarray(pos, np.float64)
    h = np.asarray(h, np.float64)
    m = np.asarray(m, np.float64)
    nx, ny = int(npix[0]), int(npix[1])
    au, av, an = (axis + 1) % 3, (axis + 2) % 3, axis
    L = [lim[2 * k + 1] - lim[2 * k] if bnd[k] == 1 else 0.0 for k in range(3)]
    du, dv = width[0] / nx, width[1] / ny
    pu = center[au] - 0.5 * width[0] + (np.arange(nx) + 0.5) * du
    pv = center[av] - 0.5 * width[1] + (np.arange(ny) + 0.5) * dv
    out = {k: np.zeros((ny, nx)) for k in ("sum0", "sum1", "abs1", "dq0", "dq1")}
    out["count"] = np.zeros((ny, nx), np.int64)
    out["hits"] = np.zeros(len(h), np.int64)
    hmin = 0.5 * max(du, dv) if (kind == COLUMN and clamp) else 0.0
    for j in range(len(h)):
        dn = _min_image(pos[j, an] - center[an], L[an])
        if kind == COLUMN:
            if depth > 0.0 and abs(dn) > 0.5 * depth:
                continue
            he = max(h[j], hmin)
            reach2 = 4.0 * he * he
        else:
            he = h[j]
            reach2 = 4.0 * he * he - dn * dn
            if reach2 <= 0.0:
                continue
        eu = _min_image(pos[j, au] - pu, L[au])
        ev = _min_image(pos[j, av] - pv, L[av])
        iu = np.nonzero(eu * eu < reach2)[0]
        iv = np.nonzero(ev * ev < reach2)[0]
        if iu.size == 0 or iv.size == 0:
            continue
        b2 = eu[iu][None, :] ** 2 + ev[iv][:, None] ** 2
        if kind == COLUMN:
            t = b2 / (he * he)
            w = m[j] * K * kernel_y(t) / (he * he)
        else:
            t = (b2 + dn * dn) / (he * he)
            w = m[j] * K * kernel_w(np.sqrt(t)) / he ** 3
        inside = t < 4.0
        w = np.where(inside, w, 0.0)
        sl = np.ix_(iv, iu)
        if scales:
            q, e = np.sqrt(t), 1e-5
            if kind == COLUMN:
                dw = m[j] * K * (kernel_y((q + e) ** 2) - kernel_y(np.maximum(q - e, 0.0) ** 2)) / (he * he)
            else:
                dw = m[j] * K * (kernel_w(q + e) - kernel_w(np.maximum(q - e, 0.0))) / he ** 3
            dw = np.abs(dw) / (q + e - np.maximum(q - e, 0.0))
            out["dq0"][sl] += dw
            if a is not None:
                out["dq1"][sl] += dw * abs(float(a[j]))
        out["sum0"][sl] += w
        out["count"][sl] += inside
        out["hits"][j] = int(inside.sum())
        if a is not None:
            out["sum1"][sl] += w * float(a[j])
            out["abs1"][sl] += np.abs(w * float(a[j]))
    return out
