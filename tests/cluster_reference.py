"""numpy restatement of the cluster problem's model, in the operation order of the code under test: the units of
src/units.hpp, the constants ClusterGravity's constructor rolls together, g_from_r, the ACCEPT-like entropy profile,
the hydrostatic-equilibrium sphere (RK4 pressure profile on a linear radial mesh, per meshblock), the problem generator
and the gravitational source term.  The yardstick of tests/test_cluster_host.py and tests/test_gpu_cluster.py, in the
manner of cooling_reference.py: written from the formulas, one numpy call per libm call of the C++.

Every function works on numpy float64 scalars or arrays; nothing here is fused or reassociated.
"""
import numpy as np

F = np.float64

# src/units.hpp, CGS
KEV_CGS = 1.60218e-9
KM_S_CGS = 1e5
KPC_CGS = 3.0856775809623245e+21
MPC_CGS = 3.0856775809623245e+24
MSUN_CGS = 1.98841586e+33
AMU_CGS = 1.660538921e-24
MH_CGS = 1.007947 * AMU_CGS
KB_CGS = 1.3806488e-16
G_CGS = 6.67408e-08


class Units:
    def __init__(self, length=1.0, mass=1.0, time=1.0):
        self.l, self.m, self.t = F(length), F(mass), F(time)

    def energy(self):
        return self.m * self.l * self.l / (self.t * self.t)

    def k_boltzmann(self):
        return F(KB_CGS) / self.energy()

    def gravitational_constant(self):
        return F(G_CGS) / (np.power(self.l, 3) / (self.m * np.power(self.t, 2)))

    def kev(self):
        return F(KEV_CGS) / self.energy()

    def g(self):
        return F(1.0) / self.m

    def cm(self):
        return F(1.0) / self.l

    def km_s(self):
        return F(KM_S_CGS) / (self.l / self.t)

    def kpc(self):
        return F(KPC_CGS) / self.l

    def mpc(self):
        return F(MPC_CGS) / self.l

    def msun(self):
        return F(MSUN_CGS) / self.m

    def mh(self):
        return F(MH_CGS) / self.m


def composition(He):
    """mu, mu_e (hydro.cpp:482-503)"""
    He = F(He)
    mu = 1 / (He * 3. / 4. + (1 - He) * 2)
    mu_e = 1 / (He * 2. / 4. + (1 - He))
    return F(mu), F(mu_e)


def defaults(u):
    """the reference's defaults of the keys read here, in the units u"""
    return dict(hubble_parameter=70 * u.km_s() / u.mpc(), m_nfw_200=8.5e14 * u.msun(), c_nfw=F(6.81), alpha_bcg_s=F(0.1),
                beta_bcg_s=F(1.43), m_bcg_s=7.5e10 * u.msun(), r_bcg_s=4 * u.kpc(), m_smbh=3.4e8 * u.msun(),
                g_smoothing_radius=F(0.0), k_0=20 * u.kev() * u.cm() * u.cm(), k_100=120 * u.kev() * u.cm() * u.cm(),
                r_k=100 * u.kpc(), alpha_k=F(1.75), r_fix=1953.9724519818478 * u.kpc(),
                rho_fix=8.607065015897638e-30 * u.g() / np.power(u.kpc(), 3), r_sampling=F(4.0))


class Gravity:
    """ClusterGravity: the constants of its constructor and g_from_r"""

    def __init__(self, G, hubble_parameter, include_nfw, which_bcg, include_smbh, m_nfw_200, c_nfw, m_bcg_s, r_bcg_s, m_smbh,
                 smoothing_r):
        G, H, c, m = F(G), F(hubble_parameter), F(c_nfw), F(m_nfw_200)
        self.include_nfw, self.which_bcg, self.include_smbh = bool(include_nfw), which_bcg, bool(include_smbh)
        rho_crit = 3 * H * H / (8 * np.pi * G)
        rho_nfw_0 = 200 / 3. * rho_crit * np.power(c, 3.) / (np.log(1 + c) - c / (1 + c))
        self.r_nfw_s = np.power(m / (4 * np.pi * rho_nfw_0 * (np.log(1 + c) - c / (1 + c))), F(1. / 3.))
        self.g_const_nfw = G * m / (np.log(1 + c) - c / (1 + c))
        self.r_bcg_s = F(r_bcg_s)
        self.g_const_bcg = G * F(m_bcg_s) / (self.r_bcg_s * self.r_bcg_s) if which_bcg == "HERNQUIST" else F(0.0)
        self.g_const_smbh = G * F(m_smbh)
        self.smoothing_r = F(smoothing_r)

    def nfw_terms(self, r_in):
        """L = log(1 + r / r_s) and q = r / (r + r_s) at the smoothed radius"""
        r = np.maximum(np.asarray(r_in, dtype=F), self.smoothing_r)
        return np.log(1 + r / self.r_nfw_s), r / (r + self.r_nfw_s)

    def g_from_r(self, r_in):
        r = np.maximum(np.asarray(r_in, dtype=F), self.smoothing_r)
        r2 = r * r
        g_r = np.zeros_like(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.include_nfw:
                g_r = g_r + self.g_const_nfw * (np.log(1 + r / self.r_nfw_s) - r / (r + self.r_nfw_s)) / r2
            if self.which_bcg == "HERNQUIST":
                g_r = g_r + self.g_const_bcg / ((1 + r / self.r_bcg_s) * (1 + r / self.r_bcg_s))
            if self.include_smbh:
                g_r = g_r + self.g_const_smbh / r2
        return g_r


class Sphere:
    """HydrostaticEquilibriumSphere<ClusterGravity, ACCEPTEntropyProfile>"""
    R_TOL = 1e-15

    def __init__(self, gravity, k_0, k_100, r_k, alpha_k, mh, k_boltzmann, mu, mu_e, r_fix, rho_fix, r_sampling=4.0):
        self.gravity = gravity
        self.k_0, self.k_100, self.r_k, self.alpha_k = F(k_0), F(k_100), F(r_k), F(alpha_k)
        self.mh, self.kb, self.mu, self.mu_e = F(mh), F(k_boltzmann), F(mu), F(mu_e)
        self.r_fix, self.rho_fix, self.r_sampling = F(r_fix), F(rho_fix), F(r_sampling)

    def K_from_r(self, r):
        return self.k_0 + self.k_100 * np.power(r / self.r_k, self.alpha_k)

    def P_from_rho_K(self, rho, k):
        return k * np.power(rho / self.mh, F(5. / 3.)) / (self.mu * np.power(self.mu_e, F(2. / 3.)))

    def rho_from_P_K(self, p, k):
        return np.power(self.mu * p / k, F(3. / 5.)) * self.mh * np.power(self.mu_e, F(2. / 5))

    def n_from_rho(self, rho):
        return rho / (self.mu * self.mh)

    def ne_from_rho(self, rho):
        return self.mu / self.mu_e * self.n_from_rho(rho)

    def T_from_rho_P(self, rho, p):
        return p / (self.n_from_rho(rho) * self.kb)

    def dP_dr(self, r, p):
        g = self.gravity.g_from_r(r)
        k = self.K_from_r(r)
        rho = self.rho_from_P_K(p, k)
        return -rho * g

    def step_rk4(self, t0, t1, y0):
        f = self.dP_dr
        h = t1 - t0
        k1 = f(t0, y0)
        k2 = f(t0 + h / 2., y0 + h / 2. * k1)
        k3 = f(t0 + h / 2., y0 + h / 2. * k2)
        k4 = f(t0 + h, y0 + h * k3)
        return y0 + h / 6. * (k1 + 2 * k2 + 2 * k3 + k4)

    def profile(self, r_start, r_end, n_r):
        """generate_P_rho_profile(r_start, r_end, n_r): (r, P)"""
        r_start, r_end, n_r = F(r_start), F(r_end), int(n_r)
        dr = (r_end - r_start) / (n_r - 1.0)
        r = r_start + np.arange(n_r, dtype=F) * dr
        p = np.zeros(n_r)
        k_fix = self.K_from_r(self.r_fix)
        p_fix = self.P_from_rho_K(self.rho_fix, k_fix)
        i_fix = int(np.floor((n_r - 1) / (r_end - r_start) * (self.r_fix - r_start)))
        if not (0 <= i_fix <= n_r - 2) or self.r_fix < r[i_fix] - self.R_TOL or self.r_fix > r[i_fix + 1] + self.R_TOL:
            raise ValueError("r(i_fix) to r_(i_fix+1) does not contain r_fix_")
        r_i, p_i = self.r_fix, p_fix
        for i in range(i_fix + 1, 0, -1):
            p[i - 1] = self.step_rk4(r_i, r[i - 1], p_i)
            r_i, p_i = r[i - 1], p[i - 1]
        r_i, p_i = self.r_fix, p_fix
        for i in range(i_fix, n_r - 1):
            p[i + 1] = self.step_rk4(r_i, r[i + 1], p_i)
            r_i, p_i = r[i + 1], p[i + 1]
        return r, p

    def block_mesh(self, x1, x2, x3, dx):
        """(r_start, r_end, n_r) of generate_P_rho_profile(ib, jb, kb, coords) for the block's cell centres"""
        dr = min(min(F(dx[0]), min(F(dx[1]), F(dx[2]))) / self.r_sampling, self.r_k / self.r_sampling)
        r = np.sqrt(x1[None, None, :] * x1[None, None, :] + x2[None, :, None] * x2[None, :, None] +
                    x3[:, None, None] * x3[:, None, None])
        r_start = min(F(r.min()), self.r_fix)
        r_end = max(F(r.max()), self.r_fix)
        r_start = max(F(0.0), r_start - self.r_sampling * dr)
        r_end = r_end + self.r_sampling * dr
        n_r = int(np.ceil((r_end - r_start) / dr))
        r_end = r_start + dr * (n_r - 1)
        return r_start, r_end, n_r

    def block_profile(self, x1, x2, x3, dx):
        return self.profile(*self.block_mesh(x1, x2, x3, dx))

    def columns(self, r, p):
        """PRhoProfile::write_to_ostream's columns"""
        k = self.K_from_r(r)
        rho = self.rho_from_P_K(p, k)
        return dict(r=r, P=p, K=k, rho=rho, n=self.n_from_rho(rho), ne=self.ne_from_rho(rho), T=self.T_from_rho_P(rho, p),
                    g=self.gravity.g_from_r(r), dP_dr=self.dP_dr(r, p))

    def P_from_r(self, prof, rr):
        r, p = prof
        n_r = r.size
        rr = np.asarray(rr, dtype=F)
        i_r = np.floor((n_r - 1) / (r[-1] - r[0]) * (rr - r[0])).astype(np.int64)
        if np.any(i_r < 0) or np.any(i_r > n_r - 2) or np.any(rr < r[i_r] - self.R_TOL) or np.any(rr > r[i_r + 1] + self.R_TOL):
            raise ValueError("PRhoProfile::P_from_r R(i_r) to R_(i_r+1) does not contain r")
        return (p[i_r] * (r[i_r + 1] - rr) + p[i_r + 1] * (rr - r[i_r])) / (r[i_r + 1] - r[i_r])

    def rho_from_r(self, prof, rr):
        p_r = self.P_from_r(prof, rr)
        return self.rho_from_P_K(p_r, self.K_from_r(np.asarray(rr, dtype=F)))


def cell_centres(xmin, dx, g0, n):
    """xc() of the host: xmin + ((g0 + i) + 1/2) dx for the n cells from global index g0"""
    return F(xmin) + ((F(g0) + np.arange(n, dtype=F)) + 0.5) * F(dx)


def radius(x1, x2, x3):
    """[k][j][i] radii of the cell centres"""
    X, Y, Z = x1[None, None, :], x2[None, :, None], x3[:, None, None]
    return np.sqrt(X * X + Y * Y + Z * Z)


def pgen_sphere(sphere, x1, x2, x3, dx, gamma, b=None):
    """the hydrostatic sphere's conserved state of one block from its own radial mesh: [5 or 8][k][j][i] (no psi)"""
    prof = sphere.block_profile(x1, x2, x3, dx)
    r = radius(x1, x2, x3)
    gm1 = F(gamma) - 1.0
    u = np.zeros((5 if b is None else 8,) + r.shape)
    u[0] = sphere.rho_from_r(prof, r)
    u[4] = sphere.P_from_r(prof, r) / gm1
    if b is not None:
        add_uniform_field(u, b)
    return u


def pgen_uniform(shape, rho, ux, uy, uz, pres, gamma, b=None):
    rho, ux, uy, uz, pres = F(rho), F(ux), F(uy), F(uz), F(pres)
    gm1 = F(gamma) - 1.0
    u = np.zeros((5 if b is None else 8,) + tuple(shape))
    u[0], u[1], u[2], u[3] = rho, rho * ux, rho * uy, rho * uz
    u[4] = rho * (0.5 * (ux * ux + uy * uy + uz * uz) + pres / (gm1 * rho))
    if b is not None:
        add_uniform_field(u, b)
    return u


def add_uniform_field(u, b):
    bx, by, bz = (F(v) for v in b)
    u[5], u[6], u[7] = bx, by, bz
    u[4] += 0.5 * (bx * bx + by * by + bz * bz)


def gravity_src(gravity, x1, x2, x3, rho, v1, v2, v3, beta_dt):
    """GravitationalFieldSrcTerm on [k][j][i] arrays: (src, dM1, dM2, dM3, dE), the amounts SUBTRACTED from the
    conserved momentum and energy (M -= dM, E -= dE)"""
    X = np.broadcast_to(x1[None, None, :], rho.shape)
    Y = np.broadcast_to(x2[None, :, None], rho.shape)
    Z = np.broadcast_to(x3[:, None, None], rho.shape)
    r = np.sqrt(X * X + Y * Y + Z * Z)
    g_r = gravity.g_from_r(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        src = np.where(r == 0, F(0.0), F(beta_dt) * rho * g_r / r)
    return src, src * X, src * Y, src * Z, src * (X * v1 + Y * v2 + Z * v3)


# ---- the physical parameters of inputs/cluster_hse.in, converted here with the constants above --------------------
DECK_UNITS = Units(MPC_CGS, 1.98841586e+47, 3.15576e+16)  # 1 Mpc, 1e14 Msun, 1 Gyr
DECK_HE, DECK_GAMMA = 0.25, 1.6666666666666667


def deck_parameters(u=DECK_UNITS):
    return dict(hubble_parameter=70 * u.km_s() / u.mpc(), m_nfw_200=1e15 * u.msun(), c_nfw=F(6.0),
                m_bcg_s=1e11 * u.msun(), r_bcg_s=4 * u.kpc(), m_smbh=1e8 * u.msun(), g_smoothing_radius=F(1e-6),
                k_0=10 * u.kev() * u.cm() * u.cm(), k_100=150 * u.kev() * u.cm() * u.cm(), r_k=100 * u.kpc(),
                alpha_k=F(1.1), r_fix=2 * u.mpc(), rho_fix=1e-28 * u.g() / np.power(u.cm(), 3), r_sampling=F(4.0))


def deck_model(nfw=True, bcg="HERNQUIST", smbh=True, u=DECK_UNITS):
    """(Gravity, Sphere) of inputs/cluster_hse.in, or of a variant with other components of the field"""
    q = deck_parameters(u)
    mu, mu_e = composition(DECK_HE)
    grav = Gravity(u.gravitational_constant(), q["hubble_parameter"], nfw, bcg, smbh, q["m_nfw_200"], q["c_nfw"],
                   q["m_bcg_s"], q["r_bcg_s"], q["m_smbh"], q["g_smoothing_radius"])
    sph = Sphere(grav, q["k_0"], q["k_100"], q["r_k"], q["alpha_k"], u.mh(), u.k_boltzmann(), mu, mu_e, q["r_fix"],
                 q["rho_fix"], q["r_sampling"])
    return grav, sph
