"""numpy restatement of the reference's observables beyond the conserved quantities, term by term, with the types of
sph::SphTypes (x, y, z, temp float64; v, a, m, c, kx, xm float32) and the reference's operation order.  numpy keeps
float32 arithmetic in float32 and does not contract, so every term equals the reference's bit for bit up to the libm
behind exp/sin/cos.  (paths below main/src/observables of the reference)

  mach_rms      MachSquareSum            gpu_reductions.cu:98-107    norm2(V) / (c c) in float, widened
  kh_growth     localGrowthRate          time_energy_growth.hpp:57-63  Tc voli = xm / kx divides in float, rest double
  wind_bubble   Survivors                gpu_reductions.cu:132-151   float kx / xm * m >= 0.64 rhoBubble (double) and
                                                                     temp <= 0.9 tempWind
  grav_waves    d2QuadpoleMomentum       grav_waves_calculations.hpp:87-121  scalv2 and vel vel float, rest double;
                                                                     the diagonal times 2/3 after the sum (:108)
  conserved     localConservedQuantities conserved_quantities.hpp:49-101 (as oracle/pyoracle.py conserved_quantities)

terms(kind, f, ...) gives the per-particle float64 terms of every sum of the kind; sums(...) their sums and the sums of
their magnitudes, on which a summation-order tolerance is judged.  One deviation, shared with the kernel: a particle
at rest contributes 0 to the Mach sum whatever c holds.
"""
import numpy as np

KINDS = ["time_energy", "mach_rms", "kh_growth", "wind_bubble", "grav_waves"]
CONSERVED = ["ecin", "eint", "px", "py", "pz", "Lx", "Ly", "Lz", "totalNeighbors"]
EXTRA = {"time_energy": [], "mach_rms": ["machSquareSum"], "kh_growth": ["sumsi", "sumci", "sumdi"],
         "wind_bubble": ["survivors"], "grav_waves": ["d2xx", "d2yy", "d2zz", "d2xy", "d2xz", "d2yz"]}
F32 = ("vx", "vy", "vz", "ax", "ay", "az", "m", "c", "kx", "xm")
F64 = ("x", "y", "z", "temp")


def ideal_gas_cv(mui=np.float32(10.0), gamma=5.0 / 3.0):
    """idealGasCv<float, double> (sph/eos.hpp:13-18)"""
    R = np.float32(8.317e7)
    return np.float32(np.float64(R / np.float32(mui)) / (np.float64(gamma) - np.float64(np.float32(1.0))))


def _typed(f, s):
    out = {}
    for k in F32:
        if k in f:
            out[k] = np.ascontiguousarray(f[k], dtype=np.float32)[s]
    for k in F64:
        if k in f:
            out[k] = np.ascontiguousarray(f[k], dtype=np.float64)[s]
    if "nc" in f:
        out["nc"] = np.asarray(f["nc"])[s]
    return out


def conserved_terms(p, mui=np.float32(10.0), gamma=5.0 / 3.0):
    m = p["m"].astype(np.float64)
    V = [p[k].astype(np.float64) for k in ("vx", "vy", "vz")]
    X = [p[k] for k in ("x", "y", "z")]
    t = {"ecin": m * (V[0] * V[0] + V[1] * V[1] + V[2] * V[2]),  # halved after the sum
         "eint": np.float64(ideal_gas_cv(mui, gamma)) * p["temp"] * m,
         "px": m * V[0], "py": m * V[1], "pz": m * V[2],
         "Lx": m * (X[1] * V[2] - X[2] * V[1]),
         "Ly": m * (X[2] * V[0] - X[0] * V[2]),
         "Lz": m * (X[0] * V[1] - X[1] * V[0])}
    t["totalNeighbors"] = p["nc"].astype(np.float64) if "nc" in p else np.zeros(m.size)
    return t


def mach_terms(p):
    vx, vy, vz, c = p["vx"], p["vy"], p["vz"], p["c"]
    v2 = vx * vx + vy * vy + vz * vz  # float32
    assert v2.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (v2 / (c * c)).astype(np.float64)
    return {"machSquareSum": np.where(v2 == 0, 0.0, q)}


def kh_terms(p, ybox):
    x, y = p["x"], p["y"]
    voli = (p["xm"] / p["kx"]).astype(np.float64)  # the float quotient, widened
    four_pi = 4.0 * np.pi
    aux = np.where(y < ybox * 0.5, np.exp(-four_pi * np.abs(y - 0.25)), np.exp(-four_pi * np.abs(ybox - y - 0.25)))
    vyv = p["vy"].astype(np.float64) * voli
    return {"sumsi": vyv * np.sin(four_pi * x) * aux, "sumci": vyv * np.cos(four_pi * x) * aux, "sumdi": voli * aux}


def wind_rho(p):
    """rhoi = kx / xm * m in float (gpu_reductions.cu:143)"""
    r = p["kx"] / p["xm"] * p["m"]
    assert r.dtype == np.float32
    return r


def wind_terms(p, rho_bubble, temp_wind):
    cloud = (wind_rho(p).astype(np.float64) >= 0.64 * rho_bubble) & (p["temp"] <= 0.9 * temp_wind)
    return {"survivors": cloud.astype(np.float64)}


def grav_terms(p):
    """the terms of the six sums BEFORE the diagonal's 2/3"""
    X = [p[k] for k in ("x", "y", "z")]
    v = [p[k] for k in ("vx", "vy", "vz")]
    A = [p[k].astype(np.float64) for k in ("ax", "ay", "az")]
    m = p["m"].astype(np.float64)
    scalv2 = (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]).astype(np.float64)  # float sum, widened
    cda = X[0] * A[0] + X[1] * A[1] + X[2] * A[2]
    t = {}
    for name, d in (("d2xx", 0), ("d2yy", 1), ("d2zz", 2)):
        t[name] = (3.0 * ((v[d] * v[d]).astype(np.float64) + X[d] * A[d]) - scalv2 - cda) * m
    V = [c.astype(np.float64) for c in v]
    for name, (a, b) in (("d2xy", (0, 1)), ("d2xz", (0, 2)), ("d2yz", (1, 2))):
        t[name] = (2.0 * V[a] * V[b] + A[a] * X[b] + X[a] * A[b]) * m
    return t


def terms(kind, f, first=0, last=None, ybox=1.0, rho_bubble=1.0, temp_wind=1.0, conserved=True):
    n = len(f["x"] if "x" in f else f["vx"])
    p = _typed(f, slice(first, n if last is None else last))
    t = conserved_terms(p) if conserved else {}
    if kind == "mach_rms":
        t.update(mach_terms(p))
    elif kind == "kh_growth":
        t.update(kh_terms(p, ybox))
    elif kind == "wind_bubble":
        t.update(wind_terms(p, rho_bubble, temp_wind))
    elif kind == "grav_waves":
        t.update(grav_terms(p))
    elif kind != "time_energy":
        raise ValueError(kind)
    return t


def sums(kind, f, **kw):
    """({name: sum}, {name: sum of |term|}) with ecin halved and the gravitational-wave diagonal times 2/3, both after
    the sum, as the reference does"""
    t = terms(kind, f, **kw)
    s = {k: float(np.sum(v)) for k, v in t.items()}
    a = {k: float(np.sum(np.abs(v))) for k, v in t.items()}
    if "ecin" in s:
        s["ecin"], a["ecin"] = 0.5 * s["ecin"], 0.5 * a["ecin"]
    for k in ("d2xx", "d2yy", "d2zz"):
        if k in s:
            s[k], a[k] = s[k] * 2.0 / 3.0, a[k] * 2.0 / 3.0
    return s, a


GWUNITS = 6.6726e-8 / 2.997924562e10 ** 4 / 3.08568025e22  # computeHtt's unit (grav_waves_calculations.hpp:53-55)


def htt(q, theta, phi):
    """computeHtt (grav_waves_calculations.hpp:50-84) in float64, for bounds and closed forms (the bit-exact
    comparison is tests/test_observables_ref.py's)"""
    xx, yy, zz, xy, xz, yz = [float(v) for v in q]
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    s2t, s2p, c2p = np.sin(2.0 * theta), np.sin(2.0 * phi), np.cos(2.0 * phi)
    tt = (xx * cp * cp + yy * sp * sp + xy * s2p) * ct * ct + zz * st * st - (xz * cp + yz * sp) * s2t
    pp = xx * sp * sp + yy * cp * cp - xy * s2p
    tp = 0.5 * (yy - xx) * ct * s2p + xy * ct * c2p + (xz * sp - yz * cp) * st
    return (tt - pp) * GWUNITS, 2.0 * tp * GWUNITS


def htt_bound(err_q, theta, phi):
    """h+ and hx are linear in the six components: errors of at most err_q[k] in them move h+ and hx by at most
    sum_k |coefficient_k| err_q[k] (the coefficients carry GWUNITS)"""
    coef = np.array([htt(np.eye(6)[k], theta, phi) for k in range(6)])  # [k] = (d h+ / d q_k, d hx / d q_k)
    e = np.asarray(err_q, dtype=np.float64)
    return float(np.sum(np.abs(coef[:, 0]) * e)), float(np.sum(np.abs(coef[:, 1]) * e))
