"""numpy restatement of the reference's unsplit diffusive fluxes and time-step limits (test infrastructure, like
amr_oracle.py): the reference of record for apk_calc_diff_fluxes / apk_estimate_diffusion_timestep.

Every expression follows the operation order of the reference's loops, so that a build without FMA contraction matches
bit for bit:
  ThermalFluxIsoFixed        src/hydro/diffusion/conduction.cpp:189-259
  ThermalFluxGeneral         conduction.cpp:265-471 (anisotropic, fixed coefficient; lim4 of diffusion.hpp:20-68)
  MomentumDiffFluxIsoFixed   src/hydro/diffusion/viscosity.cpp:94-289
  OhmicDiffFluxIsoFixed      src/hydro/diffusion/resistivity.cpp:91-230 (Xf(k+1) - Xf(k-1) taken as 2 dx)
  Estimate*Timestep          conduction.cpp:44-184, viscosity.cpp:34-89, resistivity.cpp:33-86
Arrays are [nblocks][nvar][Nk][Nj][Ni]; flux[d] holds the flux through the lower d-face of a cell.  A transverse
direction that is collapsed contributes nothing (the reference's x1 anisotropic sweep would read j +- 1 in 1-D).
"""
import numpy as np

TINY = 1.0e-20
IDN, IV1, IV2, IV3, IPR, IB1, IB2, IB3 = 0, 1, 2, 3, 4, 5, 6, 7
IM1, IM2, IM3, IEN = 1, 2, 3, 4


def _minmod(a, b):
    return np.where(a * b > 0.0, np.where(a > 0.0, np.where(b < a, b, a), np.where(a < b, b, a)), 0.0)


def _mc(a, b):
    return _minmod(2.0 * _minmod(a, b), (a + b) / 2.0)


def lim4(a, b, c, d):
    return _mc(_mc(a, b), _mc(c, d))


class _Faces:
    """the faces of direction d over the interior extent: S(v, o) = prim(v) at R + o, o a 3-vector (i, j, k)"""

    def __init__(self, prim, nx, ng, d):
        self.prim = prim
        self.lo = [ng if n > 1 else 0 for n in nx]
        self.hi = [self.lo[a] + nx[a] + (1 if a == d else 0) for a in range(3)]
        self.d = d

    def sl(self, o=(0, 0, 0)):
        (i0, j0, k0), (i1, j1, k1) = self.lo, self.hi
        return (slice(k0 + o[2], k1 + o[2]), slice(j0 + o[1], j1 + o[1]), slice(i0 + o[0], i1 + o[0]))

    def S(self, v, o=(0, 0, 0)):
        return self.prim[(slice(None), v) + self.sl(o)]


def _e(a, s=1):
    o = [0, 0, 0]
    o[a] = s
    return o


def _add(*os):
    return tuple(sum(x) for x in zip(*os))


def diff_fluxes(prim, flux, nx, ng, dx, conduction="none", kappa=0.0, sat_prefac=1.5, viscosity="none", nu=0.0,
                resistivity="none", eta=0.0):
    """CalcDiffFluxes: returns copies of flux[0..ndim-1] with every enabled process added (conduction, viscosity,
    resistivity: the reference's order)"""
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    out = [np.array(f, copy=True) if f is not None else None for f in flux]
    for d in range(ndim):
        F = _Faces(prim, nx, ng, d)
        S = F.S
        L = tuple(_e(d, -1))
        ta, tb = (1, 2) if d == 0 else ((0, 2) if d == 1 else (0, 1))
        act = {ta: ta < ndim, tb: tb < ndim}
        dxn = dx[d]
        fl = out[d]
        sl = (slice(None),)

        def fv_(v):
            return fl[sl + (v,) + F.sl()]

        if conduction == "isotropic":
            tR = S(IPR) / S(IDN)
            tL = S(IPR, L) / S(IDN, L)
            dTdn = (tR - tL) / dxn
            denf = 0.5 * (S(IDN) + S(IDN, L))
            fv_(IEN)[...] = fv_(IEN) - kappa * denf * dTdn
        elif conduction == "anisotropic":
            def T(o=(0, 0, 0)):
                return S(IPR, o) / S(IDN, o)
            g = [None, None, None]
            g[d] = (T() - T(L)) / dxn
            for t in (ta, tb):
                if act[t]:
                    p, m = tuple(_e(t)), tuple(_e(t, -1))
                    g[t] = lim4(T(p) - T(), T() - T(m), T(_add(L, p)) - T(L), T(L) - T(_add(L, m))) / dx[t]
                else:
                    g[t] = 0.0
            denf = 0.5 * (S(IDN) + S(IDN, L))
            tdf = 0.5 * (kappa + kappa)
            bx = 0.5 * (S(IB1, L) + S(IB1))
            by = 0.5 * (S(IB2, L) + S(IB2))
            bz = 0.5 * (S(IB3, L) + S(IB3)) if ndim >= 3 else 0.0
            bmag = np.sqrt(bx * bx + by * by + bz * bz)
            bmag = np.where(bmag < TINY, TINY, bmag)
            bn = (bx, by, bz)[d] / bmag
            bdg = (bx * g[0] + by * g[1] + bz * g[2]) / bmag
            fc = -tdf * denf * bdg * bn
            fcm = np.abs(tdf * denf * bdg)
            pL, pR = S(IPR, L), S(IPR)
            presf = 0.5 * (pR + pL)
            with np.errstate(invalid="ignore"):
                fsat = np.where(fc > 0.0, sat_prefac * np.sqrt(pL / denf) * pL,
                                np.where(fc < 0.0, sat_prefac * np.sqrt(pR / denf) * pR,
                                         sat_prefac * np.sqrt(presf / denf) * presf))
            fv_(IEN)[...] = fv_(IEN) + (fsat / (fsat + fcm)) * fc
        if viscosity == "isotropic":
            vn, va, vb = IV1 + d, IV1 + ta, IV1 + tb

            def tsum(v, o):
                mo = tuple(-x for x in o)
                return (S(v, o) + S(v, _add(o, L))) - (S(v, mo) + S(v, _add(mo, L)))
            fv = [None, None, None]
            fv[d] = 4.0 * (S(vn) - S(vn, L)) / (3.0 * dxn)
            fv[ta] = (S(va) - S(va, L)) / dxn
            fv[tb] = (S(vb) - S(vb, L)) / dxn
            for t, vt in ((ta, va), (tb, vb)):
                if act[t]:
                    o = tuple(_e(t))
                    fv[d] = fv[d] - tsum(vt, o) / (6.0 * dx[t])
                    fv[t] = fv[t] + tsum(vn, o) / (4.0 * dx[t])
            nud = 0.5 * nu * (S(IDN) + S(IDN, L))
            fv_(IM1)[...] = fv_(IM1) - nud * fv[0]
            fv_(IM2)[...] = fv_(IM2) - nud * fv[1]
            fv_(IM3)[...] = fv_(IM3) - nud * fv[2]
            fv_(IEN)[...] = fv_(IEN) - 0.5 * nud * ((S(IV1, L) + S(IV1)) * fv[0] + (S(IV2, L) + S(IV2)) * fv[1] +
                                                    (S(IV3, L) + S(IV3)) * fv[2])
        if resistivity == "ohmic":
            def dn(v):
                return (S(v) - S(v, L)) / dxn

            def dt(v, t):
                if not act[t]:
                    return 0.0
                p, m = tuple(_e(t)), tuple(_e(t, -1))
                return (0.5 * (S(v, _add(p, L)) + S(v, p)) - 0.5 * (S(v, _add(m, L)) + S(v, m))) / (2.0 * dx[t])

            def bs(v):
                return S(v, L) + S(v)
            if d == 0:
                j2 = dt(IB1, 2) - dn(IB3)
                j3 = dn(IB2) - dt(IB1, 1)
                fv_(IB2)[...] = fv_(IB2) + -eta * j3
                fv_(IB3)[...] = fv_(IB3) + eta * j2
                fv_(IEN)[...] = fv_(IEN) + 0.5 * eta * (bs(IB3) * j2 - bs(IB2) * j3)
            elif d == 1:
                j3 = dt(IB2, 0) - dn(IB1)
                j1 = dn(IB3) - dt(IB2, 2)
                fv_(IB1)[...] = fv_(IB1) + eta * j3
                fv_(IB3)[...] = fv_(IB3) + -eta * j1
                fv_(IEN)[...] = fv_(IEN) + 0.5 * eta * (bs(IB1) * j3 - bs(IB3) * j1)
            else:
                j1 = dt(IB3, 1) - dn(IB2)
                j2 = dn(IB1) - dt(IB3, 0)
                fv_(IB1)[...] = fv_(IB1) + -eta * j2
                fv_(IB2)[...] = fv_(IB2) + eta * j1
                fv_(IEN)[...] = fv_(IEN) + 0.5 * eta * (bs(IB2) * j1 - bs(IB1) * j2)
    return out


def diffusion_timestep(prim, nx, ng, dx, cfl_diff, conduction="none", kappa=0.0, sat_prefac=1.5, viscosity="none",
                       nu=0.0, resistivity="none", eta=0.0):
    """min over the enabled processes of cfl_diff * fac * min(...) (hydro.cpp:935-949)"""
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    fac = 0.5 if ndim == 1 else (0.25 if ndim == 2 else 1.0 / 6.0)
    huge = np.finfo(np.float64).max

    def iso(coeff):
        m = huge
        for a in range(ndim):
            m = min(m, dx[a] * dx[a] / (coeff + TINY))
        return cfl_diff * fac * m
    dt = huge
    if conduction == "isotropic":
        dt = min(dt, iso(kappa))
    elif conduction == "anisotropic":
        lo = [ng if n > 1 else 0 for n in nx]
        hi = [lo[a] + nx[a] for a in range(3)]

        def S(v, o=(0, 0, 0)):
            return prim[:, v, lo[2] + o[2]:hi[2] + o[2], lo[1] + o[1]:hi[1] + o[1], lo[0] + o[0]:hi[0] + o[0]]

        def T(o=(0, 0, 0)):
            return S(IPR, o) / S(IDN, o)
        rho, p = S(IDN), S(IPR)
        dTdx = 0.5 * (T((1, 0, 0)) - T((-1, 0, 0))) / dx[0]
        dTdy = 0.5 * (T((0, 1, 0)) - T((0, -1, 0))) / dx[1] if ndim >= 2 else 0.0
        dTdz = 0.5 * (T((0, 0, 1)) - T((0, 0, -1))) / dx[2] if ndim >= 3 else 0.0
        gradTmag = np.sqrt(dTdx * dTdx + dTdy * dTdy + dTdz * dTdz)
        bx, by, bz = S(IB1), S(IB2), S(IB3)
        bmag = np.sqrt(bx * bx + by * by + bz * bz)
        flux_sat = sat_prefac * np.sqrt(p / rho) * p
        flux_classic = kappa * rho * gradTmag
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (gradTmag != 0.0) & (bmag != 0.0) & ~(flux_classic / flux_sat > 100.0)
            costheta = np.abs(bx * dTdx + by * dTdy + bz * dTdz) / (bmag * gradTmag)
            m = np.where(ok, dx[0] * dx[0] / (kappa * np.abs(bx) / bmag * costheta + TINY), huge)
            if ndim >= 2:
                m = np.fmin(m, np.where(ok, dx[1] * dx[1] / (kappa * np.abs(by) / bmag * costheta + TINY), huge))
            if ndim >= 3:
                m = np.fmin(m, np.where(ok, dx[2] * dx[2] / (kappa * np.abs(bz) / bmag * costheta + TINY), huge))
        dt = min(dt, cfl_diff * fac * float(np.min(m)))
    if viscosity != "none":
        dt = min(dt, iso(nu))
    if resistivity != "none":
        dt = min(dt, iso(eta))
    return dt
