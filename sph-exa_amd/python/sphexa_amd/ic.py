"""Initial conditions of the BASELINE configurations other than the device-generated Sedov lattice
(sx_sim_init_sedov): host numpy arrays in the layout sx_sim_set_state takes.

The reference builds Noh and Evrard from a glass block (main/src/init/{noh,evrard}_init.hpp, --glass) that is not
available offline; both use a cell-centred lattice instead, with the reference's field values.
"""
import math

import numpy as np

R_GAS = np.float32(8.317e7)


def ideal_gas_cv(mui=np.float32(10.0), gamma=5.0 / 3.0):
    """idealGasCv<float, double> (sph/eos.hpp:13-18)"""
    return np.float32(np.float64(R_GAS / np.float32(mui)) / (gamma - 1.0))


def _lattice(side, r):
    step = (2.0 * r) / side
    c = -r + 0.5 * step + np.arange(side, dtype=np.float64) * step
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    return xx.ravel(), yy.ravel(), zz.ravel()


def _fields(n):
    f = {k: np.zeros(n, np.float32) for k in ("h", "m", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "du_m1", "alpha")}
    f["alpha"][:] = np.float32(0.05)  # alphamin
    f["id"] = np.arange(n, dtype=np.uint64)
    return f


def noh(side):
    """Noh implosion (noh_init.hpp:46-100 field values): lattice cut to r <= 0.5, v = -r_hat, x_m1 = v dt0,
    T = 1e-20/cv, dt0 = 1e-4,
    open box.  Returns (arrays, box limits, boundary, dt0)."""
    r = 0.5
    x, y, z = _lattice(side, r)
    rad = np.sqrt(x * x + y * y + z * z)
    keep = rad <= r
    x, y, z, rad = x[keep], y[keep], z[keep], rad[keep]
    n = x.size
    f = _fields(n)
    f["x"], f["y"], f["z"] = x, y, z
    vol = 4.0 / 3.0 * math.pi * r ** 3
    f["h"][:] = np.float32(np.cbrt(3.0 / (4 * math.pi) * 100 * vol / n) * 0.5)
    f["m"][:] = np.float32(1.0 / n)
    inv = np.where(rad > 0, 1.0 / np.maximum(rad, 1e-300), 0.0)
    f["vx"][:], f["vy"][:], f["vz"][:] = -x * inv, -y * inv, -z * inv
    # the integrator's previous displacement x_m1 = v * minDt (noh_init.hpp:96-98): the first positionUpdate takes
    # the velocity from dX_n / dt_m1 (positions.hpp:77-88), so x_m1 = 0 would stop the inflow
    for d in ("x", "y", "z"):
        f[d + "_m1"][:] = (f["v" + d].astype(np.float64) * 1e-4).astype(np.float32)
    f["temp"] = np.full(n, 1e-20 / np.float64(ideal_gas_cv()))
    lo, hi = -0.5 - 1e-3, 0.5 + 1e-3
    return f, [lo, hi, lo, hi, lo, hi], [0, 0, 0], 1e-4


#: TurbulenceConstants() (main/src/init/turbulence_init.hpp:48-71): the entries that are parameters of a Sim
TURBULENCE_CONSTANTS = dict(gamma=1.001, muiConst=0.62, Kcour=0.4, ng0=100, ngmax=150)


def turbulence_params(params):
    """`params` (an SxParams) with TURBULENCE_CONSTANTS applied, as the reference's settings set the ParticlesData
    attributes of a turbulence run"""
    for k, v in TURBULENCE_CONSTANTS.items():
        setattr(params, k, v)
    return params


def turbulence(side, Lbox=1.0, mTotal=1.0, u0=1000.0):
    """Subsonic driven turbulence (turbulence_init.hpp:75-97 field values, initTurbulenceHydroFields): side^3 particles
    at rest in the periodic cube [-L/2, L/2)^3, m = mTotal/N, T = u0/cv with gamma = 1.001 and mui = 0.62, alpha =
    alphamin, h from ng0 = 100, dt0 = 1e-4.  The reference replicates a glass block (TurbulenceGlass, --glass) that is
    not available offline; a cell-centred lattice stands in for it.  Run with turbulence_params(default_params()) and
    Sim.set_turbulence(Lbox=Lbox).  Returns (arrays, box limits, boundary, dt0)."""
    r = 0.5 * Lbox
    x, y, z = _lattice(side, r)
    n = x.size
    f = _fields(n)
    f["x"], f["y"], f["z"] = x, y, z
    f["m"][:] = np.float32(mTotal / n)
    f["h"][:] = np.float32(np.cbrt(3.0 / (4.0 * math.pi) * TURBULENCE_CONSTANTS["ng0"] * Lbox ** 3 / n) * 0.5)
    cv = ideal_gas_cv(np.float32(TURBULENCE_CONSTANTS["muiConst"]), TURBULENCE_CONSTANTS["gamma"])
    f["temp"] = np.full(n, u0 / np.float64(cv))
    return f, [-r, r, -r, r, -r, r], [1, 1, 1], 1e-4


def evrard(side):
    """Evrard collapse (evrard_init.hpp:50-108 field values): lattice in [-1,1]^3 cut to 0 < r <= 1 and contracted by
    sqrt(r) to a 1/r density profile; m = 1/N, u0 = 0.05, h from the 1/r concentration, G = 1, dt0 = 1e-4; open box
    [-1.25, 1.25]^3 (the reference re-fits open boxes to the particles every sync)."""
    r = 1.0
    x, y, z = _lattice(side, r)
    rad0 = np.sqrt(x * x + y * y + z * z)
    keep = (rad0 <= r) & (rad0 > 1e-9 * r)
    x, y, z, rad0 = x[keep], y[keep], z[keep], rad0[keep]
    con = np.sqrt(rad0)
    x, y, z = x * con, y * con, z * con
    n = x.size
    f = _fields(n)
    f["x"], f["y"], f["z"] = x, y, z
    f["m"][:] = np.float32(1.0 / n)
    f["temp"] = np.full(n, 0.05 / np.float64(ideal_gas_cv()))
    c0 = 2.0 / 3.0 * n / (4.0 * math.pi / 3.0 * r ** 3)
    radius = np.sqrt(x * x + y * y + z * z)
    f["h"][:] = (np.cbrt(3.0 / (4.0 * math.pi) * 100 / (c0 / np.maximum(radius, 1e-12))) * 0.5).astype(np.float32)
    lo, hi = -1.25 * r, 1.25 * r
    return f, [lo, hi, lo, hi, lo, hi], [0, 0, 0], 1e-4


def plummer(n, seed=0, a=1.0, rmax=8.0, dt0=1e-4):
    """Plummer sphere in virial equilibrium for the gravity-only propagator (propagator 3), G = 1, total mass 1, scale
    radius a: the sampling of Aarseth, Henon & Wielen (1974) -- radii from the inverted mass profile
    r = a / sqrt(u^(-2/3) - 1), redrawn beyond rmax * a, isotropic speeds q * v_esc(r) with q from q^2 (1 - q^2)^(7/2)
    by rejection -- then shifted to zero centre of mass and zero total momentum.  Equal masses 1/n, h a constant
    softening a / n^(1/3), x_m1 = v * dt0.  No thermal field.  Open box [-1.5 rmax a, 1.5 rmax a]^3.
    Returns (arrays, box limits, boundary, dt0)."""
    rng = np.random.default_rng(seed)
    r = np.empty(0)
    while r.size < n:
        u = rng.uniform(0.0, 1.0, 2 * n)
        u = u[u > 0.0]
        c = 1.0 / np.sqrt(u ** (-2.0 / 3.0) - 1.0)
        r = np.concatenate([r, c[c <= rmax]])
    r = r[:n]

    def directions(k):
        cz = rng.uniform(-1.0, 1.0, k)
        ph = rng.uniform(0.0, 2.0 * math.pi, k)
        s = np.sqrt(1.0 - cz * cz)
        return s * np.cos(ph), s * np.sin(ph), cz

    q = np.empty(0)
    while q.size < n:
        cand = rng.uniform(0.0, 1.0, 4 * n)
        y = rng.uniform(0.0, 0.1, 4 * n)  # max of q^2 (1 - q^2)^3.5 is 0.0925
        q = np.concatenate([q, cand[y < cand * cand * (1.0 - cand * cand) ** 3.5]])
    q = q[:n]
    speed = q * math.sqrt(2.0) * (1.0 + r * r) ** -0.25 / math.sqrt(a)
    dx, dy, dz = directions(n)
    ux, uy, uz = directions(n)
    pos = [a * r * dx, a * r * dy, a * r * dz]
    vel = [speed * ux, speed * uy, speed * uz]
    f = {}
    for k, p, v in zip("xyz", pos, vel):
        f[k] = p - p.mean()  # equal masses: the centre of mass is the mean
        v32 = (v - v.mean()).astype(np.float32)
        v32 = (v32 - np.float32(v32.astype(np.float64).mean())).astype(np.float32)  # the float rounding's residue
        f["v" + k] = v32
        f[k + "_m1"] = (v32.astype(np.float64) * dt0).astype(np.float32)
    f["m"] = np.full(n, np.float32(1.0 / n))
    f["h"] = np.full(n, np.float32(a / np.cbrt(n)))
    f["id"] = np.arange(n, dtype=np.uint64)
    lim = 1.5 * rmax * a
    return f, [-lim, lim, -lim, lim, -lim, lim], [0, 0, 0], dt0
