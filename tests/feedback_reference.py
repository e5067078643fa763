"""numpy restatement of the cluster problem's fixed-power AGN feedback, in the operation order of the code under test:
the precessing jet frame, AGNFeedback's derived jet numbers and per-stage numbers, the loop of its source term (thermal
sphere, jet cylinders, ceilings, ConsToPrim), the magnetic tower's potential, field, density, central-difference curl,
source, power contributions and power scaling.  The yardstick of tests/test_cluster_feedback_host.py and
tests/test_gpu_cluster_feedback.py, in the manner of cluster_reference.py: written from the formulas, one numpy (or
math) call per libm call of the C++.

Scalars computed once on the host (cos, sin, pow, sqrt of parameters) go through `math`, which calls the same libm as
the C++; per-cell arithmetic is numpy float64, nothing fused or reassociated.  Squares of positions are products, as in
the code under test (the reference writes pow(x, 2) there).  exp is the one per-cell call that is not correctly rounded:
comparisons of anything behind an exp carry a bound instead of asking for equal bits.
"""
import math
from types import SimpleNamespace

import numpy as np

F = np.float64
EPS = np.finfo(np.float64).eps
C_CGS = 2.99792458e10  # src/units.hpp
LI, DONUT = 1, 2


# ---- the jet frame (jet_coords.hpp) ---------------------------------------------------------------------------------
def jet_coords(theta, phi_dot, phi0, time):
    phi = F(phi0) + F(time) * F(phi_dot)
    return SimpleNamespace(cos_theta=F(math.cos(theta)), sin_theta=F(math.sin(theta)), cos_phi=F(math.cos(phi)),
                           sin_phi=F(math.sin(phi)))


def sim_cart_to_jet_cyl(jc, x, y, z):
    """(r, cos_theta, sin_theta, h) of the positions in the jet's cylindrical coordinates"""
    x_jet = x * jc.cos_phi * jc.cos_theta + y * jc.sin_phi * jc.cos_theta - z * jc.sin_theta
    y_jet = -x * jc.sin_phi + y * jc.cos_phi
    z_jet = x * jc.sin_theta * jc.cos_phi + y * jc.sin_phi * jc.sin_theta + z * jc.cos_theta
    r = np.sqrt(np.abs(x_jet) * np.abs(x_jet) + np.abs(y_jet) * np.abs(y_jet))
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_t = np.where(r != 0, x_jet / r, F(0.0))
        sin_t = np.where(r != 0, y_jet / r, F(0.0))
    return r, cos_t, sin_t, z_jet


def jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, v_r, v_theta, v_h):
    v_x_jet = v_r * cos_t - v_theta * sin_t
    v_y_jet = v_r * sin_t + v_theta * cos_t
    v_z_jet = v_h
    v_x = v_x_jet * jc.cos_phi * jc.cos_theta - v_y_jet * jc.sin_phi + v_z_jet * jc.sin_theta * jc.cos_phi
    v_y = v_x_jet * jc.sin_phi * jc.cos_theta + v_y_jet * jc.cos_phi + v_z_jet * jc.sin_phi * jc.sin_theta
    v_z = -v_x_jet * jc.sin_theta + v_z_jet * jc.cos_theta
    return v_x, v_y, v_z


def grid(x1, x2, x3):
    """[k][j][i] coordinate arrays of the cell centres"""
    shape = (len(x3), len(x2), len(x1))
    return (np.broadcast_to(x1[None, None, :], shape), np.broadcast_to(x2[None, :, None], shape),
            np.broadcast_to(x3[:, None, None], shape))


# ---- AGNFeedback's constructor and per-stage numbers (agn_feedback.cpp:34-160, 187-212, 263-303) -----------------------
class RequirementError(Exception):
    pass


def agn_model(speed_of_light, mbar_gm1_over_kb, fixed_power=0.0, efficiency=1e-3, thermal_fraction=0.0, kinetic_fraction=0.0,
              magnetic_fraction=0.0, enable_magnetic_tower_mass_injection=True, thermal_radius=0.01, kinetic_jet_radius=0.01,
              kinetic_jet_thickness=0.02, kinetic_jet_offset=0.02, kinetic_jet_velocity=None, kinetic_jet_temperature=None,
              vceil=math.inf, Tceil=math.inf):
    m = SimpleNamespace(fixed_power=fixed_power, efficiency=efficiency, thermal_radius=thermal_radius,
                        kinetic_jet_radius=kinetic_jet_radius, kinetic_jet_thickness=kinetic_jet_thickness,
                        kinetic_jet_offset=kinetic_jet_offset, vceil=vceil, speed_of_light=speed_of_light)
    tf, kf, mf = thermal_fraction, kinetic_fraction, magnetic_fraction
    total = tf + kf + mf
    if total > 0:
        tf, kf, mf = tf / total, kf / total, mf / total
    if not (tf >= 0 and kf >= 0 and mf >= 0):
        raise RequirementError("AGN feedback energy fractions must be non-negative.")
    m.thermal_fraction, m.kinetic_fraction, m.magnetic_fraction = tf, kf, mf
    if enable_magnetic_tower_mass_injection:
        m.thermal_mass_fraction, m.kinetic_mass_fraction, m.magnetic_mass_fraction = tf, kf, mf
    else:
        tm = tf + kf
        m.thermal_mass_fraction = tf / tm if tm != 0 else math.nan
        m.kinetic_mass_fraction = kf / tm if tm != 0 else math.nan
        m.magnetic_mass_fraction = 0.0
    c, eff = speed_of_light, efficiency
    v, T = kinetic_jet_velocity, kinetic_jet_temperature
    e = None if T is None else T / mbar_gm1_over_kb
    if v is None and T is None:
        v, T, e = c * math.sqrt(2 * eff), 0.0, 0.0
    elif v is None:
        arg = 2 * (eff * (c * c) - (1.0 - eff) * e)
        v = math.sqrt(arg) if arg >= 0 else math.nan
    elif T is None:
        e = (eff * (c * c) - 0.5 * (v * v)) / (1 - eff)
        T = mbar_gm1_over_kb * e
    arg = 2 * (eff * (c * c) - (1 - eff) * e)
    v_of_e = math.sqrt(arg) if arg >= 0 else math.nan
    if not (abs(v - v_of_e) < 10 * EPS):
        raise RequirementError("Specified kinetic jet velocity and temperature are incompatible with mass to energy "
                               "conversion efficiency. Either the specified velocity, temperature, or efficiency are "
                               "incompatible")
    if not (v <= c * math.sqrt(2 * eff)):
        raise RequirementError("Kinetic jet velocity implies negative temperature of the jet")
    if not (e <= (c * c) * eff / (1 - eff)):
        raise RequirementError("Kinetic jet temperature implies negative kinetic energy of the jet")
    if not (v >= 0):
        raise RequirementError("Kinetic jet velocity must be non-negative")
    if not (T >= 0):
        raise RequirementError("Kinetic jet temperature must be non-negative")
    m.kinetic_jet_velocity, m.kinetic_jet_temperature, m.kinetic_jet_e = v, T, e
    m.eceil = Tceil / mbar_gm1_over_kb
    m.power = fixed_power
    m.mass_rate = fixed_power / (eff * math.pow(c, 2))
    return m


def stage_numbers(m, beta_dt):
    """the numbers of agn_feedback.cpp:263-303 for one stage"""
    c = SimpleNamespace()
    thermal_scaling_factor = 1 / (4. / 3. * math.pi * math.pow(m.thermal_radius, 3))
    c.thermal_feedback = m.thermal_fraction * m.power * thermal_scaling_factor * beta_dt
    c.thermal_density = m.thermal_mass_fraction * m.mass_rate * thermal_scaling_factor * beta_dt
    c.thermal_radius = m.thermal_radius
    kinetic_scaling_factor = 1 / (2 * m.kinetic_jet_thickness * math.pi * math.pow(m.kinetic_jet_radius, 2))
    c.jet_density = m.kinetic_mass_fraction * m.mass_rate * kinetic_scaling_factor * beta_dt
    c.jet_momentum = c.jet_density * m.kinetic_jet_velocity
    c.jet_feedback = m.kinetic_fraction * m.power * kinetic_scaling_factor * beta_dt
    c.kinetic_jet_radius, c.kinetic_jet_thickness = m.kinetic_jet_radius, m.kinetic_jet_thickness
    c.kinetic_jet_offset = m.kinetic_jet_offset
    c.vceil, c.eceil = m.vceil, m.eceil
    return c


# ---- ConsToPrim without floors or ceilings (adiabatic_hydro.hpp:52-142, adiabatic_glmmhd.hpp:62-167) ----------------------
def cons_to_prim(u, gamma):
    """[nvar][...] conserved -> primitive, the equation of state's defaults: no floor and no ceiling acts"""
    gm1 = F(gamma) - 1.0
    w = np.empty_like(u)
    w[0] = u[0]
    di = 1.0 / u[0]
    w[1], w[2], w[3] = u[1] * di, u[2] * di, u[3] * di
    e_k = 0.5 * di * (u[1] * u[1] + u[2] * u[2] + u[3] * u[3])
    if u.shape[0] >= 9:
        w[5:9] = u[5:9]
        e_B = 0.5 * (u[5] * u[5] + u[6] * u[6] + u[7] * u[7])
        w[4] = gm1 * (u[4] - e_k - e_B)
    else:
        w[4] = gm1 * (u[4] - e_k)
    return w


# ---- the loop of AGNFeedback::FeedbackSrcTerm (agn_feedback.cpp:314-409) --------------------------------------------------
def agn_feedback_src(u, w, x1, x2, x3, c, jc, gamma):
    """interior cells of one block: conserved u and stored primitives w, [nvar][k][j][i], with the cell centres x1, x2,
    x3.  Returns the new (u, w) and the masks of what acted where."""
    u, w = np.array(u, dtype=F), np.array(w, dtype=F)
    X, Y, Z = grid(x1, x2, x3)
    gm1 = F(gamma) - 1.0
    info = SimpleNamespace(sphere=np.zeros(X.shape, bool), on_sphere=np.zeros(X.shape, bool), jet=np.zeros(X.shape, bool),
                           on_axis=np.zeros(X.shape, bool), vceil=np.zeros(X.shape, bool), eceil=np.zeros(X.shape, bool))
    if c.thermal_feedback > 0 or c.thermal_density > 0:
        r2 = X * X + Y * Y + Z * Z
        R2 = F(c.thermal_radius) * F(c.thermal_radius)
        s = r2 <= R2
        info.sphere, info.on_sphere = s, r2 == R2
        if c.thermal_feedback > 0:
            u[4] = np.where(s, u[4] + F(c.thermal_feedback), u[4])
        if c.thermal_density > 0:
            d = F(c.thermal_density)
            add = [d, d * w[1], d * w[2], d * w[3], d * (0.5 * (w[1] * w[1] + w[2] * w[2] + w[3] * w[3]))]
            for n in range(5):
                u[n] = np.where(s, u[n] + add[n], u[n])
    if c.jet_density > 0:
        r, cos_t, sin_t, h = sim_cart_to_jet_cyl(jc, X, Y, Z)
        jet = (r < c.kinetic_jet_radius) & (np.abs(h) >= c.kinetic_jet_offset) & \
              (np.abs(h) <= F(c.kinetic_jet_offset) + F(c.kinetic_jet_thickness))
        info.jet, info.on_axis, info.r, info.h = jet, jet & (r == 0), r, h
        ax, ay, az = jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, F(0.0), F(0.0), F(1.0))
        sign = np.where(h > 0, F(1.0), F(-1.0))
        uj = u.copy()
        uj[0] = uj[0] + F(c.jet_density)
        uj[1] = uj[1] + F(c.jet_momentum) * sign * ax
        uj[2] = uj[2] + F(c.jet_momentum) * sign * ay
        uj[3] = uj[3] + F(c.jet_momentum) * sign * az
        uj[4] = uj[4] + F(c.jet_feedback)
        with np.errstate(all="ignore"):
            wj = cons_to_prim(uj, gamma)
        u = np.where(jet[None], uj, u)
        w = np.where(jet[None], wj, w)
        if math.isfinite(c.vceil) or math.isfinite(c.eceil):
            vceil, eceil = F(c.vceil), F(c.eceil)
            vceil2 = vceil * vceil
            v2 = w[1] * w[1] + w[2] * w[2] + w[3] * w[3]
            m = (vceil2 > 0) & (v2 > vceil2)
            info.vceil = m
            with np.errstate(all="ignore"):
                v = np.sqrt(v2)
                f = vceil / v
                for n in (1, 2, 3):
                    u[n] = np.where(m, u[n] * f, u[n])
                    w[n] = np.where(m, w[n] * f, w[n])
                u[4] = np.where(m, u[4] - 0.5 * w[0] * (v2 - vceil2), u[4])
                internal_e = w[4] / (gm1 * w[0])
                m2 = (eceil > 0) & (internal_e > eceil)
                info.eceil = m2
                u[4] = np.where(m2, u[4] - w[0] * (internal_e - eceil), u[4])
                w[4] = np.where(m2, gm1 * w[0] * eceil, w[4])
    with np.errstate(all="ignore"):
        w = cons_to_prim(u, gamma)
    return u, w, info


# ---- the magnetic tower (magnetic_tower.hpp:60-158, magnetic_tower.cpp:29-140, 146-202, 258-292) ----------------------------
def tower(potential, l_scale, li_alpha=0.0, donut_offset=0.0, donut_thickness=0.0, l_mass_scale=0.0):
    return SimpleNamespace(potential={"li": LI, "donut": DONUT}.get(potential, potential), l_scale=F(l_scale),
                           li_alpha=F(li_alpha), donut_offset=F(donut_offset), donut_thickness=F(donut_thickness),
                           l_mass_scale=F(l_mass_scale))


def tower_potential(t, jc, field, x, y, z):
    field = F(field)
    r, cos_t, sin_t, h = sim_cart_to_jet_cyl(jc, x, y, z)
    if t.potential == DONUT:
        rl = r / t.l_scale
        e = np.exp(-(rl * rl))
        inside = (np.abs(h) >= t.donut_offset) & (np.abs(h) <= t.donut_offset + t.donut_thickness)
        a_theta = np.zeros_like(r)
        a_h = np.where(inside, field * t.l_scale * e, F(0.0))
    else:
        rl, hl = r / t.l_scale, h / t.l_scale
        e = np.exp(-(rl * rl) - hl * hl)
        a_theta = field * t.l_scale * (r / t.l_scale) * e
        a_h = field * t.l_scale * t.li_alpha / 2.0 * e
    return jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, F(0.0), a_theta, a_h)


def tower_field(t, jc, field, x, y, z):
    field = F(field)
    r, cos_t, sin_t, h = sim_cart_to_jet_cyl(jc, x, y, z)
    if t.potential == DONUT:
        rl = r / t.l_scale
        e = np.exp(-(rl * rl))
        inside = (np.abs(h) >= t.donut_offset) & (np.abs(h) <= t.donut_offset + t.donut_thickness)
        b_r, b_h = np.zeros_like(r), np.zeros_like(r)
        b_theta = np.where(inside, 2.0 * field * r / t.l_scale * e, F(0.0))
    else:
        rl, hl = r / t.l_scale, h / t.l_scale
        e = np.exp(-(rl * rl) - hl * hl)
        b_r = field * 2 * (h / t.l_scale) * (r / t.l_scale) * e
        b_theta = field * t.li_alpha * (r / t.l_scale) * e
        b_h = field * 2 * (1 - rl * rl) * e
    return jet_cyl_to_sim_cart_vector(jc, cos_t, sin_t, b_r, b_theta, b_h)


def tower_density(t, jc, density, x, y, z):
    r, _, _, h = sim_cart_to_jet_cyl(jc, x, y, z)
    return F(density) * np.exp(-(r * r + h * h) / (t.l_mass_scale * t.l_mass_scale))


def density_to_add(mass_to_add, l_mass_scale):
    return mass_to_add / (math.pow(l_mass_scale, 3) * math.pow(math.pi, 3. / 2.)) if mass_to_add > 0.0 else 0.0


def curl(a, dx):
    """central-difference curl in the reference's association (/ dx / 2.0) of a = (a_x, a_y, a_z) given on [k][j][i]
    arrays one cell larger on every side than the result.  Returns (b, size): b[3][k][j][i], and size[3] = the sum over a
    component's two difference terms of (|A+| + |A-|) / (2 dx_d), what its rounding bound scales with."""
    c = slice(1, -1)
    dx1, dx2, dx3 = (F(v) for v in dx)

    def d(n, axis):
        lo = [c, c, c]
        hi = [c, c, c]
        lo[axis], hi[axis] = slice(0, -2), slice(2, None)
        return a[n][tuple(hi)], a[n][tuple(lo)]

    def term(n, axis, h):
        p, m = d(n, axis)
        return (p - m) / h / 2.0, (np.abs(p) + np.abs(m)) / (2 * h)

    # axis 0 = k (x3), 1 = j (x2), 2 = i (x1)
    t_zy, s_zy = term(2, 1, dx2)
    t_yz, s_yz = term(1, 0, dx3)
    t_xz, s_xz = term(0, 0, dx3)
    t_zx, s_zx = term(2, 2, dx1)
    t_yx, s_yx = term(1, 2, dx1)
    t_xy, s_xy = term(0, 1, dx2)
    b = np.stack([t_zy - t_yz, t_xz - t_zx, t_yx - t_xy])
    size = np.stack([s_zy + s_yz, s_xz + s_zx, s_yx + s_xy])
    return b, size


def extended(x, dx):
    """cell centres one cell beyond both ends: the centres the neighbouring blocks (or the ghost cells) have.  x must
    come from cluster_reference.cell_centres, whose formula continues: pass the extended array from there instead where
    bits matter."""
    return np.concatenate([[x[0] - F(dx)], x, [x[-1] + F(dx)]])


def tower_curl_field(t, jc, field, x1e, x2e, x3e, dx):
    """the discrete field of the potential at strength `field`: x*e are the centres of the interior plus one cell"""
    X, Y, Z = grid(x1e, x2e, x3e)
    a = tower_potential(t, jc, field, X, Y, Z)
    b, size = curl(a, dx)
    return b, size, a


def tol_b(b, size):
    """8 eps sum_terms (|A+| + |A-|) / (2 dx_d) + 2 eps |B|: exp within 1 ulp on either side, the IEEE operations after it
    the same"""
    return 8 * EPS * size + 2 * EPS * np.abs(b)


def tower_src(u, w, x1e, x2e, x3e, dx, t, jc, field, mass):
    """MagneticTower::AddSrcTerm on the interior cells of one GLM-MHD block: new u, the added field b, its bound"""
    u = np.array(u, dtype=F)
    if field == 0 and mass == 0:
        return u, np.zeros((3,) + u.shape[1:]), np.zeros((3,) + u.shape[1:])
    b, size, _ = tower_curl_field(t, jc, field, x1e, x2e, x3e, dx)
    u[5], u[6], u[7] = u[5] + b[0], u[6] + b[1], u[7] + b[2]
    u[4] = u[4] + (w[5] * b[0] + w[6] * b[1] + w[7] * b[2] + 0.5 * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]))
    rho_add = density_to_add(mass, float(t.l_mass_scale))
    if rho_add > 0.0:
        X, Y, Z = grid(x1e[1:-1], x2e[1:-1], x3e[1:-1])
        u[0] = u[0] + tower_density(t, jc, rho_add, X, Y, Z)
    return u, b, tol_b(b, size)


def tower_contribs(wB, x1, x2, x3, dx, t, jc):
    """(lin, quad, sum |lin terms|, sum |quad terms|): the power scaling's two sums over one block's interior cells, the
    terms added with math.fsum"""
    X, Y, Z = grid(x1, x2, x3)
    b = tower_field(t, jc, 1.0, X, Y, Z)
    vol = F(dx[0]) * F(dx[1]) * F(dx[2])
    lin = (wB[0] * b[0] + wB[1] * b[1] + wB[2] * b[2]) * vol
    quad = 0.5 * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]) * vol
    return (math.fsum(lin.ravel()), math.fsum(quad.ravel()), math.fsum(np.abs(lin).ravel()), math.fsum(np.abs(quad).ravel()))


def field_to_add(lin, quad, beta_dt, power):
    if lin == 0 and quad == 0:
        raise RequirementError("MagneticTowerModel::PowerSrcTerm mt_linear_contrib and mt_quadratic_contrib are both zero.")
    disc = lin * lin + 4 * quad * beta_dt * power
    if disc < 0 or quad == 0:
        raise RequirementError("MagneticTowerModel::PowerSrcTerm No field rate is viable")
    return (-lin + math.sqrt(disc)) / (2 * quad)
