"""numpy restatement of the reference's tabular cooling (src/hydro/srcterms/tabular_cooling.{hpp,cpp}) and of Units
(src/units.hpp), for the tests: the table set-up, CoolingTableObj::DeDt, SubcyclingFixedIntSrcTerm<RK12|RK45>,
TownsendSrcTerm and EstimateTimeStep, in the reference's expression order, one cell at a time."""
import math

import numpy as np

# Units (src/units.hpp), cgs
ATOMIC_MASS_UNIT_CGS = 1.660538921e-24
MH_CGS = 1.007947 * ATOMIC_MASS_UNIT_CGS
K_BOLTZMANN_CGS = 1.3806488e-16
MPC_CGS, MSUN_CGS, GYR_CGS = 3.085677580962325e+24, 1.98841586e+33, 3.15576e+16
KEPSILON = 1e-12


class Units:
    def __init__(self, length=1.0, mass=1.0, time=1.0):
        self.length, self.mass, self.time = float(length), float(mass), float(time)
        self.energy = self.mass * self.length * self.length / (self.time * self.time)
        self.mh = MH_CGS / self.mass
        self.k_boltzmann = K_BOLTZMANN_CGS / self.energy
        self.atomic_mass_unit = ATOMIC_MASS_UNIT_CGS / self.mass
        self.erg = 1.0 / self.energy
        self.cm = 1.0 / self.length
        self.s = 1.0 / self.time

    def lambda_units(self, lambda_units_cgs=1.0):
        """lambda_units_cgs / (erg cm^3 / s in code units) (tabular_cooling.cpp:48-51)"""
        return lambda_units_cgs / (self.erg * math.pow(self.cm, 3) / self.s)


CLUSTER_UNITS = Units(MPC_CGS, 1e14 * MSUN_CGS, GYR_CGS)


def composition(units, He):
    """mu, mu_e, mbar, mbar_over_kb (hydro.cpp:486-502)"""
    mu = 1 / (He * 3. / 4. + (1 - He) * 2)
    mu_e = 1 / (He * 2. / 4. + (1 - He))
    return mu, mu_e, mu * units.atomic_mass_unit, mu * units.mh / units.k_boltzmann


def read_table(path):
    rows = []
    with open(path) as f:
        for line in f:
            s = line.strip()
            if s and not s.startswith("#"):
                rows.append([float(v) for v in s.split()])
    a = np.array(rows)
    return a[:, 0], a[:, 1]


class Table:
    """TabularCooling's table state (tabular_cooling.cpp:190-276) and CoolingTableObj's scalars"""

    def __init__(self, log_temps, log_lambdas_cgs, lambda_units, gamma, mbar_over_kb, He, mh, T_floor=-1.0,
                 d_e_tol=1e-8, max_iter=100, cfl=0.1, townsend=False):
        lt = [float(v) for v in log_temps]
        shift = math.log10(lambda_units)
        ll = [float(v) - shift for v in log_lambdas_cgs]
        self.n = n = len(lt)
        self.log_temps, self.log_lambdas = lt, ll
        self.log_temp_start, self.log_temp_final = lt[0], lt[n - 1]
        self.d_log_temp = lt[1] - lt[0]
        self.lambda_final = math.pow(10.0, ll[n - 1])
        self.gm1 = gamma - 1.0
        self.mbar_gm1_over_kb = mbar_over_kb * self.gm1
        xh = 1.0 - He
        self.x_H_over_m_h2 = (xh / mh) * (xh / mh)
        self.X_by_mh2 = math.pow((1 - He) / mh, 2)
        self.T_floor, self.d_e_tol, self.max_iter, self.cfl = T_floor, d_e_tol, max_iter, cfl
        self._noise = None  # (rate_noise)
        self.temp_cool_floor = math.pow(10.0, self.log_temp_start)
        self.temp_final = math.pow(10.0, self.log_temp_final)
        temp_floor = T_floor if T_floor > self.temp_cool_floor else self.temp_cool_floor
        self.e_floor_sub = temp_floor / self.mbar_gm1_over_kb
        self.e_floor_town = T_floor / self.mbar_gm1_over_kb
        if townsend:
            self.lambdas = [math.pow(10.0, v) for v in ll]
            self.temps = [math.pow(10.0, v) for v in lt]
            nb = n - 1
            self.alpha_k = [(math.log10(self.lambdas[i + 1]) - math.log10(self.lambdas[i])) / (lt[i + 1] - lt[i])
                            for i in range(nb)]
            Y = [0.0] * nb
            for i in range(nb - 2, -1, -1):
                am1 = self.alpha_k[i] - 1.0
                step = ((self.lambdas[nb] / self.lambdas[i]) * (self.temps[i] / self.temps[nb]) *
                        (math.pow(self.temps[i] / self.temps[i + 1], am1) - 1.0) / am1)
                Y[i] = Y[i + 1] - step
            self.Y_k = Y

    def log_lambda(self, e):
        """the log10 lambda DeDt interpolates at e (None where DeDt returns 0 before it)"""
        if e < 0 or math.isnan(e):
            return None
        log_temp = math.log10(self.mbar_gm1_over_kb * e)
        if log_temp < self.log_temp_start:
            return None
        if log_temp > self.log_temp_final:
            return 0.5 * log_temp - 0.5 * self.log_temp_final + self.log_lambdas[self.n - 1]
        i = int((log_temp - self.log_temp_start) / self.d_log_temp)
        i = min(i, self.n - 2)
        lti = self.log_temp_start + self.d_log_temp * i
        li, lip1 = self.log_lambdas[i], self.log_lambdas[i + 1]
        return li + (log_temp - lti) * (lip1 - li) / self.d_log_temp

    def dedt(self, e, rho):
        """CoolingTableObj::DeDt -> (de_dt, valid)"""
        if e < 0 or math.isnan(e):
            return 0.0, False
        ll = self.log_lambda(e)
        if ll is None:
            return 0.0, True
        lam = math.pow(10., ll)
        d = -lam * self.x_H_over_m_h2 * rho
        if self._noise is not None:
            delta, rng = self._noise
            d *= 1.0 + delta * rng.uniform(-1.0, 1.0)
        return d, True

    def rate_noise(self, delta=0.0, seed=0):
        """every non-zero DeDt from now on is multiplied by 1 + delta * xi, xi uniform in [-1, 1] from a generator
        seeded with `seed` (delta = 0: off, DeDt as the reference computes it).  A probe of how far a last-bit
        difference in log10 / pow moves a result."""
        self._noise = (float(delta), np.random.default_rng(seed)) if delta else None
        return self


def _rk12(h, y0, f):
    f0, v0 = f(y0)
    y1_l = y0 + h * f0
    f1, v1 = f(y1_l)
    return y0 + h / 2. * (f0 + f1), y1_l, v0 and v1


def _rk45(h, y0, f):
    valid = True

    def F(y):
        nonlocal valid
        r, v = f(y)
        valid = valid and v
        return r
    k1 = h * F(y0)
    k2 = h * F(y0 + 1. / 4. * k1)
    k3 = h * F(y0 + 3. / 32. * k1 + 9. / 32. * k2)
    k4 = h * F(y0 + 1932. / 2197. * k1 - 7200. / 2197. * k2 + 7296. / 2197. * k3)
    k5 = h * F(y0 + 439. / 216. * k1 - 8. * k2 + 3680. / 513. * k3 - 845. / 4104. * k4)
    k6 = h * F(y0 - 8. / 27. * k1 + 2. * k2 - 3544. / 2565. * k3 + 1859. / 4104. * k4 - 11. / 40. * k5)
    y1_l = y0 + 25. / 216. * k1 + 1408. / 2565. * k3 + 2197. / 4104. * k4 - 1. / 5. * k5
    y1_h = y0 + 16. / 135. * k1 + 6656. / 12825. * k3 + 28561. / 56430. * k4 - 9. / 50. * k5 + 2. / 55. * k6
    return y1_h, y1_l, valid


STEPPERS = {"rk12": (_rk12, 2), "rk45": (_rk45, 5)}


def optimal_step(order, h, err, tol):
    """RK12Stepper / RK45Stepper::OptimalStep.  pow(tol / err, 2) is the correctly rounded square: compiled from the
    reference's own header (oracle/ref, g++ -O2) a pow with the constant exponent 2 is the product, which is also what the
    product build's kernel writes, while libm's pow, which math.pow calls, is one ulp off it on about one ratio in a
    thousand (tests/test_reference_physics.py holds this function to the compiled header).  The fifth power stays libm's."""
    r = tol / err
    return 0.95 * h * (r * r if order == 2 else math.pow(r, order))


EVENTS = ("reject", "clamp_min", "accept_over_tol", "invalid_retry", "to_floor", "err_zero", "grow", "end_at_floor")


def subcycle_cell(T, integrator, rho, e0, dt, counts=None, events=None):
    """SubcyclingFixedIntSrcTerm for one cell: the final specific internal energy (counts: a list the number of
    accepted substeps is appended to; events: a dict whose EVENTS counters are incremented, one per branch taken:
    reject         d_e_err >= d_e_tol with sub_dt > min_sub_dt
    clamp_min      a rejected step whose new sub_dt is clamped to min_sub_dt
    accept_over_tol  a step accepted (at the minimum substep) with d_e_err >= d_e_tol
    invalid_retry  an invalid step (a stage's energy negative) retried at the minimum substep
    to_floor       an invalid step at the minimum substep: to the floor and the end of dt
    err_zero       an accepted step with d_e_err == 0 (a step to the floor before any valid attempt set it is one):
                   the next substep is the rest of dt
    grow           an accepted step whose next sub_dt is larger than the one just taken
    end_at_floor   a cell whose final energy is clamped to the floor)"""
    step, order = STEPPERS[integrator]
    f = lambda e: T.dedt(e, rho)  # noqa: E731
    opt = lambda h, err, tol: optimal_step(order, h, err, tol)  # noqa: E731
    max_iter, d_e_tol, floor = T.max_iter, T.d_e_tol, T.e_floor_sub
    min_sub_dt = dt / max_iter

    def ev(name):
        if events is not None:
            events[name] = events.get(name, 0) + 1
    e = e0
    d0, _ = f(e0)
    if d0 == 0.0 or e0 <= floor:
        if counts is not None:
            counts.append(0)
        return e0
    sub_t, sub_dt = 0.0, (min_sub_dt if d_e_tol == 0 else dt)
    sub_iter = 0
    while sub_t * (1 + KEPSILON) < dt and f(e)[0] != 0.0:
        assert sub_iter <= max_iter
        attempt, d_e_err = 0, 0.0
        while True:
            e_h, e_l, valid = step(sub_dt, e, f)
            attempt += 1
            again = False
            if not valid:
                if sub_dt == min_sub_dt:
                    ev("to_floor")
                    sub_dt = dt - sub_t
                    e_h = floor
                else:
                    ev("invalid_retry")
                    again, sub_dt = True, min_sub_dt
            else:
                if e_h != 0:
                    d_e_err = abs((e_h - e_l) / e_h)
                else:  # (IEEE: 0 / 0 is NaN, x / 0 infinite)
                    d_e_err = float("nan") if e_h == e_l else math.inf
                if math.isnan(d_e_err):
                    again, sub_dt = True, min_sub_dt
                elif d_e_err >= d_e_tol and sub_dt > min_sub_dt:
                    ev("reject")
                    again = True
                    sub_dt = min_sub_dt if d_e_tol == 0 else opt(sub_dt, d_e_err, d_e_tol)
                    if sub_dt < min_sub_dt or attempt >= max_iter:
                        ev("clamp_min")
                        sub_dt = min_sub_dt
                elif d_e_err >= d_e_tol:
                    ev("accept_over_tol")
            if not again:
                break
        sub_t += sub_dt
        e = e_h
        taken = sub_dt
        if d_e_err == 0:
            ev("err_zero")
        sub_dt = dt - sub_t if d_e_err == 0 else opt(sub_dt, d_e_err, d_e_tol)
        if d_e_tol == 0:
            sub_dt = min_sub_dt
        sub_dt = min_sub_dt if sub_dt < min_sub_dt else sub_dt
        sub_dt = (dt - sub_t) if (dt - sub_t) < sub_dt else sub_dt
        if sub_dt > taken:
            ev("grow")
        sub_iter += 1
    if counts is not None:
        counts.append(sub_iter)
    if not e > floor:
        ev("end_at_floor")
    return e if e > floor else floor


def townsend_cell(T, rho, e, dt, crossed=None):
    """TownsendSrcTerm for one cell: the final specific internal energy (crossed: a list the number of temperature
    bins the cell moved down is appended to; 0 for a cell that is not cooled)"""
    e1, bins = _townsend(T, rho, e, dt)
    if crossed is not None:
        crossed.append(bins)
    return e1


def _townsend(T, rho, e, dt):
    if e <= T.e_floor_town:
        return T.e_floor_town, 0
    temp = T.mbar_gm1_over_kb * e
    if temp < T.temp_cool_floor:
        return e, 0
    n_h2_by_rho = rho * T.X_by_mh2
    nb = T.n - 1
    idx = 0
    while idx < nb - 1 and T.temps[idx + 1] < temp:
        idx += 1
    am1 = T.alpha_k[idx] - 1.0
    tef = T.Y_k[idx] + (T.lambda_final / T.lambdas[idx]) * (T.temps[idx] / T.temp_final) * \
        (math.pow(T.temps[idx] / temp, am1) - 1.0) / am1
    tef_adj = tef + T.lambda_final * dt / T.temp_final * T.mbar_gm1_over_kb * n_h2_by_rho
    idx0 = idx
    while idx > 0 and tef_adj > T.Y_k[idx]:
        idx -= 1
    a = T.alpha_k[idx]
    temp_new = T.temps[idx] * math.pow(1 - (1.0 - a) * (T.lambdas[idx] / T.lambda_final) *
                                       (T.temp_final / T.temps[idx]) * (tef_adj - T.Y_k[idx]), 1.0 / (1.0 - a))
    e1 = temp_new / T.mbar_gm1_over_kb if temp_new > T.temp_cool_floor else T.temp_cool_floor / T.mbar_gm1_over_kb
    return e1, idx0 - idx


def specific_internal_e(u, mhd):
    """(rho, e) per cell of conserved arrays [nvar, ...] as the source terms compute them"""
    rho = u[0]
    e = u[4] - 0.5 * (u[1] * u[1] + u[2] * u[2] + u[3] * u[3]) / rho
    if mhd:
        e = e - 0.5 * (u[5] * u[5] + u[6] * u[6] + u[7] * u[7])
    return rho, e / rho


def src_term(T, integrator, cons, mhd, dt, interior):
    """SrcTerm on the cells selected by `interior` (a boolean mask over cons[0]'s shape): the new cons"""
    out = cons.copy()
    rho, e = specific_internal_e(cons, mhd)
    for idx in zip(*np.nonzero(interior)):
        r, e0 = float(rho[idx]), float(e[idx])
        if integrator == "townsend":
            e1 = townsend_cell(T, r, e0, dt)
        else:
            e1 = subcycle_cell(T, integrator, r, e0, dt)
        out[(4,) + idx] = cons[(4,) + idx] + r * (e1 - e0)
    return out


def cooling_timestep(T, prim, interior):
    """EstimateTimeStep: cfl * min |e / DeDt| over the cells of `interior`"""
    if T.cfl <= 0.0:
        return np.finfo(np.float64).max
    if math.isnan(T.cfl) or math.isinf(T.cfl):
        return math.inf
    m = math.inf
    for idx in zip(*np.nonzero(interior)):
        rho, pres = float(prim[(0,) + idx]), float(prim[(4,) + idx])
        e = pres / (rho * T.gm1)
        d, _ = T.dedt(e, rho)
        t = math.inf if (d == 0 or e < T.e_floor_sub) else abs(e / d)
        m = min(t, m)
    return T.cfl * m


def analytic_e(units, He, gamma, log_temps01, log_lambdas01, e0, t):
    """the power-law cooling's closed form of the cluster_tabular_cooling test (code units in and out)"""
    mu = 1 / (He * 3.0 / 4.0 + (1 - He) * 2)
    (lt0, lt1), (ll0, ll1) = log_temps01, log_lambdas01
    m = (ll1 - ll0) / (lt1 - lt0)
    b = ll1 - lt1 * m
    # in cgs: rho [g/cm^3], e [erg/g], t [s]
    e_cgs = e0 * units.energy / units.mass
    t_cgs = t * units.time
    return lambda rho: _analytic(rho * units.mass / units.length ** 3, e_cgs, t_cgs, mu, gamma, m, b, He) \
        / (units.energy / units.mass)


def _analytic(rho, e0, t, mu, gamma, m, b, He):
    n_h = rho * (1.0 - He) / MH_CGS
    X = mu * MH_CGS * (gamma - 1) / K_BOLTZMANN_CGS
    Y = 10 ** b * n_h ** 2 / rho
    return (e0 ** (1 - m) - Y * t * (1 - m) * X ** m) ** (1.0 / (1 - m))
