"""Optically thin radiative cooling (sx_cooling_*, sx_cool, sx_sim_set_cooling): a tabulated cooling function in code
units, integrated exactly over the step for every particle (Townsend 2009, ApJS 181, 391).

The table is a list of nodes T_1 < ... < T_N with values L_k > 0; between two nodes the cooling function is the power
law through them, above T_N the last segment's law continues, and below T_1 -- the temperature floor -- nothing cools.
The model is dT/dt = -rho L(T) / cv at the rho of the step, with T the sim's temp column (u / cv): du/dt = -rho L.

No astrophysical table ships with the package: build one with from_samples from the curve of your choice and bring it
to code units with to_code_units.
"""
import ctypes as C

import numpy as np

from . import SX_OK, SxError, lib

#: the proton mass in g (CODATA 2018): the m_H of to_code_units
M_H = 1.67262192369e-24


class Cooling:
    """the host table (sx_cooling_create): nodes T (strictly increasing, positive) and values lam (positive), 2 to 256
    of them.  rate and integrate evaluate on the host the arithmetic the kernels run."""

    def __init__(self, T, lam):
        self.L = lib()
        T = np.ascontiguousarray(T, dtype=np.float64)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if T.ndim != 1 or T.shape != lam.shape:
            raise ValueError("Cooling: T and lam must be one-dimensional and of one length")
        self.h = C.c_void_p()
        rc = self.L.sx_cooling_create(C.byref(self.h), T.ctypes.data, lam.ctypes.data, T.size)
        if rc != SX_OK:
            self.h = None
            raise SxError(f"sx_cooling_create: code {rc}: needs 2 to 256 nodes, T strictly increasing, every entry "
                          "finite and positive, and exponents that double can hold")

    def close(self):
        if self.h:
            self.L.sx_cooling_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_nodes(self):
        return int(self.L.sx_cooling_num_nodes(self.h))

    def table(self):
        """dict of T, lam, alpha (the exponent of each segment; the last entry repeats the one before: the law above
        T_N) and Y (Townsend's temporal evolution function at the nodes, normalised by lam_N / T_N, 0 at T_N)"""
        n = self.num_nodes
        out = {k: np.empty(n, np.float64) for k in ("T", "lam", "alpha", "Y")}
        self.L.sx_cooling_get_table(self.h, *[out[k].ctypes.data for k in ("T", "lam", "alpha", "Y")])
        return out

    def rate(self, T):
        """L(T), 0 below the floor (sx_cooling_rate_host)"""
        f = np.vectorize(lambda t: self.L.sx_cooling_rate_host(self.h, float(t)), otypes=[np.float64])
        return f(np.asarray(T, dtype=np.float64))

    def integrate(self, T0, s):
        """T after s = rho dt / cv from T0 (sx_cooling_integrate_host)"""
        f = np.vectorize(lambda t, x: self.L.sx_cooling_integrate_host(self.h, float(t), float(x)),
                         otypes=[np.float64])
        return f(np.asarray(T0, dtype=np.float64), np.asarray(s, dtype=np.float64))


def power_law(L0, alpha, T0, Tmin, Tmax):
    """L(T) = L0 (T / T0)^alpha from the floor Tmin on (one segment, whose law continues above Tmax)"""
    T = np.array([Tmin, Tmax], dtype=np.float64)
    return Cooling(T, L0 * (T / T0) ** alpha)


def from_samples(T, Lambda):
    """power-law segments through the samples of any curve (sorted by T here)"""
    T = np.asarray(T, dtype=np.float64)
    Lambda = np.asarray(Lambda, dtype=np.float64)
    order = np.argsort(T, kind="stable")
    return Cooling(T[order], Lambda[order])


def to_code_units(T_K, Lambda_cgs, unit_mass, unit_length, unit_time, X=0.76):
    """nodes in K and a cooling function Lambda in erg cm^3 / s (the loss per volume being n_H^2 Lambda) to the code
    units of a sim whose unit mass, length and time are given in g, cm and s.  Returns (T, lam) for Cooling.

    With a hydrogen mass fraction X, n_H = X rho / m_H, so du/dt = -rho Lhat in erg / g / s for rho in g / cm^3 with

        Lhat_cgs = (X / m_H)^2 Lambda,

    and in code units, where du/dt = -rho Lhat holds between code quantities,

        Lhat = Lhat_cgs * unit_density * unit_time / unit_specific_energy,
        unit_density = unit_mass / unit_length^3,  unit_specific_energy = (unit_length / unit_time)^2.

    The sim's temp is u / cv with the cgs gas constant in cv (ic.ideal_gas_cv), so a code temp is the temperature in K
    over unit_specific_energy:

        T = T_K / unit_specific_energy.
    """
    unit_density = unit_mass / unit_length ** 3
    unit_specific_energy = (unit_length / unit_time) ** 2
    lam_cgs = (X / M_H) ** 2 * np.asarray(Lambda_cgs, dtype=np.float64)
    lam = lam_cgs * unit_density * unit_time / unit_specific_energy
    return np.asarray(T_K, dtype=np.float64) / unit_specific_energy, lam


def cool(ctx, cooling, rho, m, temp, cv, dt):
    """sx_cool on device columns (DeviceArray: rho, m float32, temp float64, updated in place): dict of the energy
    radiated, the particles that ended on the floor and the particles that were on or above it"""
    out = (C.c_double * 3)()
    ctx.check(ctx.L.sx_cool(ctx.h, cooling.h, int(temp.n), rho.ptr, m.ptr, temp.ptr, float(cv), float(dt), out),
              "sx_cool")
    return dict(radiated=out[0], on_floor=int(out[1]), cooled=int(out[2]))


def set_timing(ctx, on=True):
    """sx_set_cooling_timing: cool and cooling_time record device events round their kernels"""
    ctx.check(ctx.L.sx_set_cooling_timing(ctx.h, int(bool(on))), "sx_set_cooling_timing")


def kernel_times(ctx):
    """sx_cooling_times: device ms of the kernels of the last cool and the last cooling_time (zeros without timing)"""
    out = (C.c_double * 2)()
    ctx.check(ctx.L.sx_cooling_times(ctx.h, out), "sx_cooling_times")
    return dict(cool=out[0], coolingTime=out[1])


def cooling_time(ctx, cooling, rho, temp, cv):
    """sx_cooling_time on device columns: min over the particles of cv T / (rho L(T)), inf where nothing cools"""
    out = C.c_double()
    ctx.check(ctx.L.sx_cooling_time(ctx.h, cooling.h, int(temp.n), rho.ptr, temp.ptr, float(cv), C.byref(out)),
              "sx_cooling_time")
    return out.value
