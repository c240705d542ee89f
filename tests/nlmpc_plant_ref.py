"""The plant step of the NLMPC closed loop (include/mpcx/nlmpc_loop.hpp) restated in numpy float64, with the round-off bound the tests hold
the kernel to.  Shared by test_emu_nlmpc_loop.py and test_nlmpc_loop_gpu.py.

Formulas: the state functions of include/mpcx/nlmpc_models.hpp (= the reference examples'), x <- f(x, u, p) for the discrete UGV and
`substeps` forward-Euler steps x <- x + (Ts / substeps) f(x, u, p) for the continuous systems, then x += w.

Bound.  Two correct evaluations of one formula differ by the order of the roundings and by which multiply-add pairs the compiler fuses.  With
u = 2^-52 (twice the unit round-off, which also covers a fused against an unfused pair), a component computed by c floating-point operations
from terms t_1 .. t_n is off by at most c u sum |t_j| to first order: every partial sum is at most sum |t_j| in magnitude and every operation
adds a relative error of at most u / 2 on each side.  `C[model]` is that operation count along the longest path to a component, counted next to
each model below, including the Euler update (h = Ts / substeps: 1, h * dx: 1, x + ...: 1) and the noise (1).  Across Euler sub-steps the error
already made is carried through the next step's Jacobian (first order; the squares are 1e-32): e <- e + h |J_f| e + c u sum |t_j|."""
import numpy as np

U = 2.0 ** -52


def _vdp(x, u, p):
    """dx0 = ((1 - x1 x1) x0) - x1 + u: mul, sub, mul, sub, add = 5 operations; dx1 = x0: none"""
    x0, x1 = x[:, 0], x[:, 1]
    dx = np.stack([((1.0 - (x1 * x1)) * x0) - x1 + u[:, 0], x0], axis=1)
    T = np.stack([np.abs(x0) + np.abs(x1 * x1 * x0) + np.abs(x1) + np.abs(u[:, 0]), np.abs(x0)], axis=1)
    J = np.zeros((x.shape[0], 2, 2))
    J[:, 0, 0] = np.abs(1.0 - x1 * x1); J[:, 0, 1] = np.abs(2.0 * x1 * x0 + 1.0); J[:, 1, 0] = 1.0
    return dx, T, J


def _ugv(x, u, p):
    """xn0 = x0 + Ts x2 + 0.5 Ts Ts u0: mul, add, mul, mul, mul, add = 6 operations; xn2 = x2 + Ts u0: 2"""
    Ts = p[:, 8]
    xn = np.stack([x[:, 0] + Ts * x[:, 2] + 0.5 * Ts * Ts * u[:, 0], x[:, 1] + Ts * x[:, 3] + 0.5 * Ts * Ts * u[:, 1],
                   x[:, 2] + Ts * u[:, 0], x[:, 3] + Ts * u[:, 1]], axis=1)
    T = np.stack([np.abs(x[:, 0]) + np.abs(Ts * x[:, 2]) + np.abs(0.5 * Ts * Ts * u[:, 0]), np.abs(x[:, 1]) + np.abs(Ts * x[:, 3]) + np.abs(0.5 * Ts * Ts * u[:, 1]),
                  np.abs(x[:, 2]) + np.abs(Ts * u[:, 0]), np.abs(x[:, 3]) + np.abs(Ts * u[:, 1])], axis=1)
    return xn, T, None


def _osc(N):
    def f(x, u, p):
        """a_i = mu (1 - q_i q_i) v_i - q_i + u_i + sum_{j != i} k (q_j - q_i): mul, sub, mul, mul, sub, add = 6, then (sub, mul, add) for each of the
        N - 1 neighbours; dq_i = v_i: none"""
        mu, k = p[:, 0:1], p[:, 1:2]
        q, v = x[:, 0::2], x[:, 1::2]
        a = mu * (1 - q * q) * v - q + u
        T = np.abs(mu * v) + np.abs(mu * q * q * v) + np.abs(q) + np.abs(u)
        for i in range(N):
            for j in range(N):
                if i != j:
                    a[:, i] += k[:, 0] * (q[:, j] - q[:, i])
                    T[:, i] += np.abs(k[:, 0]) * (np.abs(q[:, j]) + np.abs(q[:, i]))
        dx = np.empty_like(x); dx[:, 0::2] = v; dx[:, 1::2] = a
        Tt = np.empty_like(x); Tt[:, 0::2] = np.abs(v); Tt[:, 1::2] = T
        J = np.zeros((x.shape[0], 2 * N, 2 * N))
        for i in range(N):
            J[:, 2 * i, 2 * i + 1] = 1.0
            J[:, 2 * i + 1, 2 * i + 1] = np.abs(mu[:, 0] * (1 - q[:, i] ** 2))
            J[:, 2 * i + 1, 2 * i] = np.abs(2 * mu[:, 0] * q[:, i] * v[:, i]) + 1.0 + (N - 1) * np.abs(k[:, 0])
            for j in range(N):
                if j != i:
                    J[:, 2 * i + 1, 2 * j] = np.abs(k[:, 0])
        return dx, Tt, J
    return f


MODELS = {"vanderpol": (_vdp, True), "ugv": (_ugv, False), "osc6": (_osc(6), True)}
# operations along the longest path to a component of the new state: inside f (see each function), + 3 for the Euler update of a continuous
# system, + 1 for the noise
C = {"vanderpol": 5 + 3 + 1, "ugv": 6 + 1, "osc6": 6 + 3 * 5 + 3 + 1}
DEFAULT_PARAMS = {"vanderpol": [0.0], "ugv": [0.7071067811865476, 0.7071067811865476, 2.0, 1.0, 0.3, 1.0, 1.0, 0.3, 0.1], "osc6": [1.0, 0.1]}


def step(model, x, u, p, Ts, substeps=1, w=None):
    """(x_next, bound): numpy float64 arrays [B, nx]; p [B, n_params] (a single row is broadcast)"""
    f, continuous = MODELS[model]
    x = np.array(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    p = np.broadcast_to(np.atleast_2d(np.asarray(p, dtype=np.float64)), (x.shape[0], np.atleast_2d(p).shape[1]))
    c = C[model]
    e = np.zeros_like(x)
    wa = np.zeros_like(x) if w is None else np.abs(w)
    if continuous:
        h = Ts / substeps
        for s in range(substeps):
            dx, T, J = f(x, u, p)
            last = s == substeps - 1
            e = e + h * np.einsum("bij,bj->bi", J, e) + c * U * (np.abs(x) + h * T + (wa if last else 0.0))
            x = x + h * dx
    else:
        x, T, _ = f(x, u, p)
        e = c * U * (T + wa)
    if w is not None:
        x = x + w
    return x, e
