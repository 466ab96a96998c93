"""Numpy restatement of the multi-start L-BFGS state machine of include/gpk.h (gpk_fit_init / gpk_fit_step), the
analytic objectives the fitter tests use, and a driver that runs any (init, step) pair to completion.

The restatement follows the header's text, one member at a time, in plain float64 numpy: it is the specification
the device kernel is compared with (same decisions, values to rounding), not a bitwise twin of it."""
import numpy as np

RUNNING, CONVERGED_G, CONVERGED_F, MAX_ITER, STALLED, BAD_START = 0, 1, 2, 3, 4, 5
EPS_PAIR = 2.2e-16
U = 2.0 ** -53  # unit roundoff of float64


class Opts:
    def __init__(self, m=8, max_iter=200, max_backtracks=20, c1=1e-4, gtol=1e-5, ftol=1e-9):
        self.m, self.max_iter, self.max_backtracks = int(m), int(max_iter), int(max_backtracks)
        self.c1, self.gtol, self.ftol = float(c1), float(gtol), float(ftol)


def free_set(x, g, lo, hi):
    return (lo < hi) & ~((x == lo) & (g > 0)) & ~((x == hi) & (g < 0))


def two_loop(q, pairs):
    """H q for ``pairs`` = [(s, y), ...] oldest first; gamma = s^T y / y^T y of the newest pair."""
    if not pairs:
        return q.copy()
    q = q.copy()
    al = []
    for s, y in reversed(pairs):
        a = (1.0 / np.dot(s, y)) * np.dot(s, q)
        al.append(a)
        q = q - a * y
    s, y = pairs[-1]
    r = (np.dot(s, y) / np.dot(y, y)) * q
    for (s, y), a in zip(pairs, reversed(al)):
        beta = (1.0 / np.dot(s, y)) * np.dot(y, r)
        r = r + (a - beta) * s
    return r


def direction(g, mask, pairs):
    """(d, pairs kept, steepest descent?) of the header's `direction` rule."""
    r = two_loop(np.where(mask, g, 0.0), pairs)
    d = np.where(mask, -r, 0.0)
    sd = not pairs
    if not (np.dot(d, g) < 0.0):
        pairs, sd = [], True
    if sd:
        d = np.where(mask, -g, 0.0)
    return d, pairs, sd


def _sd_step(d):
    with np.errstate(divide="ignore"):
        return min(1.0, 1.0 / np.sqrt(np.dot(d, d)))


class Member:
    """One restart: the state of include/gpk.h with the ring as a list (oldest first)."""

    def __init__(self, x0, lo, hi, opts):
        self.o = opts
        self.lo, self.hi = np.asarray(lo, float).copy(), np.asarray(hi, float).copy()
        self.x = np.minimum(np.maximum(np.asarray(x0, float), self.lo), self.hi)
        self.x_trial = self.x.copy()
        self.phase, self.status, self.iters, self.nback, self.evals = 0, RUNNING, 0, 0, 0
        self.f = self.f_prev = 0.0
        self.t = 0.0
        self.sd = False
        self.g = np.zeros_like(self.x)
        self.d = np.zeros_like(self.x)
        self.pairs = []

    def _trial(self):
        self.x_trial = np.minimum(np.maximum(self.x + self.t * self.d, self.lo), self.hi)

    def step(self, f_t, g_t, info_t=0):
        if self.status != RUNNING:
            return self.status
        o = self.o
        g_t = np.asarray(g_t, float)
        self.evals += 1
        bad = info_t != 0 or not np.isfinite(f_t) or not np.all(np.isfinite(g_t))
        if self.phase == 0:
            self.phase = 1
            if bad:
                self.status = BAD_START
                return self.status
            self.x, self.f, self.f_prev, self.g = self.x_trial.copy(), float(f_t), float(f_t), g_t.copy()
            self.d = np.where(free_set(self.x, self.g, self.lo, self.hi), -self.g, 0.0)
            self.sd, self.nback, self.t = True, 0, _sd_step(self.d)
            self._trial()
            return self.status
        s = self.x_trial - self.x
        gts = np.dot(self.g, s)
        if not bad and gts <= 0.0 and f_t <= self.f + o.c1 * gts:
            y = g_t - self.g
            sy = np.dot(s, y)
            if sy > EPS_PAIR * (np.sqrt(np.dot(s, s)) * np.sqrt(np.dot(y, y))):
                self.pairs = (self.pairs + [(s.copy(), y.copy())])[-o.m:]
            else:
                self.pairs = []      # a rejected pair: the history no longer describes the curvature here
            self.f_prev, self.x, self.f, self.g = self.f, self.x_trial.copy(), float(f_t), g_t.copy()
            self.iters += 1
            mask = free_set(self.x, self.g, self.lo, self.hi)
            pgn = float(np.max(np.abs(self.g) * mask)) if mask.size else 0.0
            if pgn <= o.gtol:
                self.status = CONVERGED_G
            elif self.f_prev - self.f <= o.ftol * max(1.0, abs(self.f), abs(self.f_prev)):
                self.status = CONVERGED_F
            elif self.iters >= o.max_iter:
                self.status = MAX_ITER
            else:
                self.d, self.pairs, self.sd = direction(self.g, mask, self.pairs)
                self.t = _sd_step(self.d) if self.sd else 1.0
                self.nback = 0
        else:
            self.nback += 1
            if self.nback > o.max_backtracks:
                if self.sd:
                    self.status = STALLED
                else:
                    self.pairs = []
                    self.d = np.where(free_set(self.x, self.g, self.lo, self.hi), -self.g, 0.0)
                    self.sd, self.nback, self.t = True, 0, _sd_step(self.d)
            else:
                self.t *= 0.5
        if self.status == RUNNING:
            self._trial()
        else:
            self.x_trial = self.x.copy()
        return self.status


class NumpyFitter:
    """(init, step) over a batch of members, the shape of engine.LbfgsState."""

    def __init__(self, x0, lo, hi, opts=None):
        self.o = opts or Opts()
        self.members = [Member(row, lo, hi, self.o) for row in np.atleast_2d(np.asarray(x0, float))]

    @property
    def x_trial(self):
        return np.stack([m.x_trial for m in self.members])

    def step(self, f, g, info=None):
        for b, mem in enumerate(self.members):
            mem.step(float(f[b]), g[b], 0 if info is None else int(info[b]))
        return self.status

    @property
    def status(self):
        return np.array([m.status for m in self.members], dtype=np.int32)

    def current(self):
        return (np.stack([m.x for m in self.members]), np.array([m.f for m in self.members]),
                np.stack([m.g for m in self.members]), np.array([m.iters for m in self.members], dtype=np.int32))


def drive(fitter, objective, max_steps=5000, on_step=None):
    """Run ``fitter`` (x_trial, step(f, g, info) -> status) until no member is RUNNING; ``objective(X [B, P])`` ->
    (f [B], g [B, P], info [B] or None).  ``on_step(k, fitter)`` is called after every step.  Returns the steps."""
    for k in range(max_steps):
        f, g, info = objective(fitter.x_trial)
        status = fitter.step(f, g, info)
        if on_step is not None:
            on_step(k, fitter)
        if not np.any(np.asarray(status) == RUNNING):
            return k + 1
    raise AssertionError("the fitter did not finish in %d steps" % max_steps)


# ------------------------------------------------------------------------------------------ objectives (numpy)
def quadratic(A, xstar, c=0.0):
    """f = 1/2 (x - x*)^T A (x - x*) + c for a symmetric A [P, P]."""
    A, xstar = np.asarray(A, float), np.asarray(xstar, float)

    def fn(X):
        E = np.atleast_2d(X) - xstar
        G = E @ A
        return 0.5 * np.sum(G * E, axis=1) + c, G, None
    return fn


def diag_quadratic(h, xstar):
    """f = 1/2 sum_j h_j (x_j - x*_j)^2 (Hessian diag(h))."""
    h, xstar = np.asarray(h, float), np.asarray(xstar, float)

    def fn(X):
        E = np.atleast_2d(X) - xstar
        return 0.5 * np.sum(h * E * E, axis=1), h * E, None
    return fn


def rosenbrock(X):
    X = np.atleast_2d(X)
    x, y = X[:, 0], X[:, 1]
    f = (1 - x) ** 2 + 100 * (y - x * x) ** 2
    g = np.stack([-2 * (1 - x) - 400 * x * (y - x * x), 200 * (y - x * x)], axis=1)
    return f, g, None


def log_spaced(cond, n):
    """n Hessian eigenvalues from 1 to cond, log-spaced."""
    return np.exp(np.linspace(0.0, np.log(cond), n)) if n > 1 else np.ones(1)


def two_loop_rounding_bound(n_par, m, pairs, g):
    """A bound on |fl(H g) - H g|_inf for the two-loop recursion, by running the recursion on magnitudes.

    Every inner product of length n fl-evaluated in any order satisfies |fl(u.v) - u.v| <= gamma_n |u|.|v| with
    gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, (3.5)); the recursion has 2 m of them that feed the
    result linearly (each followed by a product with rho and an axpy: 3 more roundings, so gamma_{n + 3}) plus the two of
    gamma and the m of rho = 1 / s.y -- 4 m + 2 inner products counting those that form rho and gamma.  Propagating
    them to first order through a recursion whose every intermediate is replaced by its magnitude bounds the error of
    every component by gamma_{n + 3} (4 m + 2) R, with R = the result of the magnitude recursion (all signs made
    positive: |rho| |s|.|q|, q + |alpha| |y|, ...)."""
    n = n_par
    gam = (n + 3) * U / (1 - (n + 3) * U)
    q = np.abs(g).astype(float)
    al = []
    for s, y in reversed(pairs):
        kap = np.dot(np.abs(s), np.abs(y)) / abs(np.dot(s, y))   # (rho's own relative error: gamma_n kap)
        a = kap * abs(1.0 / np.dot(s, y)) * np.dot(np.abs(s), q)
        al.append(a)
        q = q + a * np.abs(y)
    s, y = pairs[-1]
    r = (np.dot(np.abs(s), np.abs(y)) / np.dot(y, y)) * q
    for (s, y), a in zip(pairs, reversed(al)):
        kap = np.dot(np.abs(s), np.abs(y)) / abs(np.dot(s, y))
        beta = kap * abs(1.0 / np.dot(s, y)) * np.dot(np.abs(y), r)
        r = r + (a + beta) * np.abs(s)
    return gam * (4 * m + 2) * r


def pseudo_huber(xstar):
    """f = sum_j (sqrt(1 + (x_j - x*_j)^2) - 1): unit Hessian at x*, curvature (1 + e^2)^-3/2 -> 0 far away, so the
    first quasi-Newton steps of a far start (gamma = s^T y / y^T y ~ 1 / curvature) overshoot x* by a wide margin."""
    xstar = np.asarray(xstar, float)

    def fn(X):
        E = np.atleast_2d(X) - xstar
        r = np.sqrt(1.0 + E * E)
        return np.sum(r - 1.0, axis=1), E / r, None
    return fn
