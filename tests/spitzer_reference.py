"""numpy restatement of the reference's general thermal conduction with a temperature-dependent (Spitzer) diffusivity
(test infrastructure, like diffusion_reference.py, whose calling convention this keeps): the reference of record for
apk_calc_diff_fluxes_v2 / apk_estimate_diffusion_timestep_v2.

Every expression follows the operation order of the reference's loops, so that a build without FMA contraction matches
bit for bit:
  ThermalDiffusivity::Get      src/hydro/diffusion/conduction.cpp:28-42
  ThermalFluxGeneral           conduction.cpp:265-471, both branches (anisotropic; isotropic :344-346)
  EstimateConductionTimestep   conduction.cpp:93-181, the general branch
The dispatch is CalcDiffFluxes' (diffusion.cpp:18-53): isotropic conduction with a fixed coefficient is
ThermalFluxIsoFixed, which diffusion_reference.py restates and this module hands over to; everything else takes the
general path here.  Viscosity and resistivity are diffusion_reference's.

One deliberate deviation from the reference, shared with the library: T^(5/2) is T * T * sqrt(T), three correctly
rounded operations, where the reference calls std::pow (whose last bit differs between libraries).  As in
diffusion_reference.py a collapsed transverse direction contributes nothing to a gradient.

`spitzer`: None for the fixed coefficient `kappa`, else (coeff_code, mbar, k_boltzmann) in code units.
"""
import numpy as np

import diffusion_reference as R
from diffusion_reference import IB1, IB2, IB3, IDN, IEN, IPR, TINY, lim4


def t_pow_5_2(t):
    """T^(5/2) as the library forms it"""
    return t * t * np.sqrt(t)


def chi(pres, rho, kappa=0.0, spitzer=None):
    """ThermalDiffusivity::Get (conduction.cpp:28-42)"""
    if spitzer is None:
        return np.full_like(np.asarray(pres, dtype=np.float64), kappa)
    coeff, mbar, kb = spitzer
    t_cgs = mbar / kb * pres / rho
    kappa_spitzer = coeff * t_pow_5_2(t_cgs)
    return kappa_spitzer * mbar / kb / rho


def conduction_faces(prim, nx, ng, dx, d, conduction, kappa=0.0, sat_prefac=1.5, spitzer=None):
    """ThermalFluxGeneral on the faces of direction d (interior extent, as diffusion_reference._Faces): a dict of the
    intermediate face quantities -- flux_classic `fc`, its magnitude `fcm`, the saturated flux `fsat`, the field strength
    before the TINY clamp `bmag` (anisotropic) -- and the flux added to IEN, `q`"""
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    F = R._Faces(prim, nx, ng, d)
    S = F.S
    L = tuple(R._e(d, -1))
    ta, tb = (1, 2) if d == 0 else ((0, 2) if d == 1 else (0, 1))
    act = {ta: ta < ndim, tb: tb < ndim}

    def T(o=(0, 0, 0)):
        return S(IPR, o) / S(IDN, o)
    g = [None, None, None]
    g[d] = (T() - T(L)) / dx[d]
    for t in (ta, tb):
        if act[t]:
            p, m = tuple(R._e(t)), tuple(R._e(t, -1))
            g[t] = lim4(T(p) - T(), T() - T(m), T(R._add(L, p)) - T(L), T(L) - T(R._add(L, m))) / dx[t]
        else:
            g[t] = 0.0
    denf = 0.5 * (S(IDN) + S(IDN, L))
    tdf = 0.5 * (chi(S(IPR), S(IDN), kappa, spitzer) + chi(S(IPR, L), S(IDN, L), kappa, spitzer))
    out = {}
    if conduction == "anisotropic":
        bx = 0.5 * (S(IB1, L) + S(IB1))
        by = 0.5 * (S(IB2, L) + S(IB2))
        bz = 0.5 * (S(IB3, L) + S(IB3)) if ndim >= 3 else 0.0
        bmag = np.sqrt(bx * bx + by * by + bz * bz)
        out["bmag"] = bmag
        bmag = np.where(bmag < TINY, TINY, bmag)
        bn = (bx, by, bz)[d] / bmag
        bdg = (bx * g[0] + by * g[1] + bz * g[2]) / bmag
        fc = -tdf * denf * bdg * bn
        fcm = np.abs(tdf * denf * bdg)
    elif conduction == "isotropic":
        gmag = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        fc = -tdf * denf * g[d]
        fcm = tdf * denf * gmag
    else:
        raise ValueError(conduction)
    pL, pR = S(IPR, L), S(IPR)
    presf = 0.5 * (pR + pL)
    with np.errstate(invalid="ignore"):
        fsat = np.where(fc > 0.0, sat_prefac * np.sqrt(pL / denf) * pL,
                        np.where(fc < 0.0, sat_prefac * np.sqrt(pR / denf) * pR,
                                 sat_prefac * np.sqrt(presf / denf) * presf))
    out.update(fc=fc, fcm=fcm, fsat=fsat, q=(fsat / (fsat + fcm)) * fc, sl=F.sl())
    return out


def _general(conduction, spitzer):
    return conduction == "anisotropic" or (conduction == "isotropic" and spitzer is not None)


def diff_fluxes(prim, flux, nx, ng, dx, conduction="none", kappa=0.0, sat_prefac=1.5, viscosity="none", nu=0.0,
                resistivity="none", eta=0.0, spitzer=None):
    """CalcDiffFluxes: returns copies of flux[0..ndim-1] with every enabled process added (conduction, viscosity,
    resistivity: the reference's order, per face)"""
    if not _general(conduction, spitzer):
        return R.diff_fluxes(prim, flux, nx, ng, dx, conduction=conduction, kappa=kappa, sat_prefac=sat_prefac,
                             viscosity=viscosity, nu=nu, resistivity=resistivity, eta=eta)
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    out = [np.array(f, copy=True) if f is not None else None for f in flux]
    for d in range(ndim):
        c = conduction_faces(prim, nx, ng, dx, d, conduction, kappa, sat_prefac, spitzer)
        fe = out[d][(slice(None), IEN) + c["sl"]]
        fe[...] = fe + c["q"]
    # (each face's energy flux is a chain of sums in process order, so the other processes are added onto the result)
    return R.diff_fluxes(prim, out, nx, ng, dx, conduction="none", viscosity=viscosity, nu=nu, resistivity=resistivity,
                         eta=eta)


def cond_dt_cells(prim, nx, ng, dx, conduction, kappa=0.0, sat_prefac=1.5, spitzer=None):
    """the general branch of EstimateConductionTimestep per interior cell: a dict of `gradTmag`, `bmag`, the saturation
    ratio flux_classic / flux_sat `ratio` (anisotropic) and the cell's limit `m` (DBL_MAX where it sets none)"""
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    huge = np.finfo(np.float64).max
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
    c = chi(p, rho, kappa, spitzer)
    out = {"gradTmag": gradTmag}
    with np.errstate(invalid="ignore", divide="ignore"):
        if conduction == "isotropic":
            ok = gradTmag != 0.0
            m = np.where(ok, dx[0] * dx[0] / c, huge)
            if ndim >= 2:
                m = np.fmin(m, np.where(ok, dx[1] * dx[1] / c, huge))
            if ndim >= 3:
                m = np.fmin(m, np.where(ok, dx[2] * dx[2] / c, huge))
        else:
            bx, by, bz = S(IB1), S(IB2), S(IB3)
            bmag = np.sqrt(bx * bx + by * by + bz * bz)
            flux_sat = sat_prefac * np.sqrt(p / rho) * p
            flux_classic = c * rho * gradTmag
            ratio = flux_classic / flux_sat
            ok = (gradTmag != 0.0) & (bmag != 0.0) & ~(ratio > 100.0)
            costheta = np.abs(bx * dTdx + by * dTdy + bz * dTdz) / (bmag * gradTmag)
            m = np.where(ok, dx[0] * dx[0] / (c * np.abs(bx) / bmag * costheta + TINY), huge)
            if ndim >= 2:
                m = np.fmin(m, np.where(ok, dx[1] * dx[1] / (c * np.abs(by) / bmag * costheta + TINY), huge))
            if ndim >= 3:
                m = np.fmin(m, np.where(ok, dx[2] * dx[2] / (c * np.abs(bz) / bmag * costheta + TINY), huge))
            out.update(bmag=bmag, ratio=ratio)
    out["m"] = m
    return out


def diffusion_timestep(prim, nx, ng, dx, cfl_diff, conduction="none", kappa=0.0, sat_prefac=1.5, viscosity="none",
                       nu=0.0, resistivity="none", eta=0.0, spitzer=None):
    """min over the enabled processes of cfl_diff * fac * min(...) (hydro.cpp:935-949)"""
    if not _general(conduction, spitzer):
        return R.diffusion_timestep(prim, nx, ng, dx, cfl_diff, conduction=conduction, kappa=kappa, sat_prefac=sat_prefac,
                                    viscosity=viscosity, nu=nu, resistivity=resistivity, eta=eta)
    ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)
    fac = 0.5 if ndim == 1 else (0.25 if ndim == 2 else 1.0 / 6.0)
    m = cond_dt_cells(prim, nx, ng, dx, conduction, kappa, sat_prefac, spitzer)["m"]
    dt = cfl_diff * fac * float(np.min(m))
    return min(dt, R.diffusion_timestep(prim, nx, ng, dx, cfl_diff, conduction="none", viscosity=viscosity, nu=nu,
                                        resistivity=resistivity, eta=eta))
