"""Restatement (numpy) of the stochastic pendulum's solve (include/lde.h: "the stochastic pendulum"): StochasticDiffEq's EM() and EulerHeun()
at a fixed step on dual numbers — values and the six partials ∂(x, v)/∂(x₀, v₀, L) — along the path the library's counter layout draws
(tests/philox_ref.py). float64 by default; `dtype=np.float32` runs the same formulas in f32. Test infrastructure only, pinned by
tests/test_sde_host.py (its partials against finite differences of its own values, its noise against the definition's statistics)."""
import math

import numpy as np

from tests import philox_ref as P

EM, EULER_HEUN = 2, 3
SIGMA = 0.01
G = 10.0


def plan(ts, dt):
    """[(n_j, h_j)] for j = 1 … T−1: n_j = max(1, ceil(D_j/dt − 1e-9)) substeps of h_j = D_j/n_j (f64)."""
    out = []
    for j in range(1, len(ts)):
        D = float(ts[j]) - float(ts[j - 1])
        n = max(1, int(math.ceil(D / dt - 1e-9)))
        out.append((n, D / n))
    return out


def xi(B, s, seed=0, off=0, first=0, dtype=np.float64):
    """(ξ_x, ξ_v) of trajectories first … first + B − 1 at substep s: the Box–Muller pair of words 0 and 1 of the block with counter
    (first + b, s, off lo, off hi) and key (seed lo, seed hi)."""
    off &= 0xFFFFFFFFFFFFFFFF
    b = (np.arange(B, dtype=np.uint64) + np.uint64(first & 0xFFFFFFFFFFFFFFFF)) & P.MASK
    w = P.philox4x32_10(b, s & 0xFFFFFFFF, off & 0xFFFFFFFF, off >> 32, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1 = ((w[0] >> np.uint64(8)).astype(dtype) + dtype(0.5)) * dtype(1.0 / 16777216.0)
    u2 = ((w[1] >> np.uint64(8)).astype(dtype) + dtype(0.5)) * dtype(1.0 / 16777216.0)
    r = np.sqrt(dtype(-2.0) * np.log(u1))
    a = dtype(2.0 * np.pi) * u2
    return r * np.cos(a), r * np.sin(a)


def _f(y, L):
    """The drift on duals: y [B, 8] = [x, v, ∂x/∂(x₀, v₀, L), ∂v/∂(x₀, v₀, L)]; ∂f/∂L = [0, (G/L²) sin x]."""
    dt_ = y.dtype.type
    s, c = np.sin(y[:, 0]), np.cos(y[:, 0])
    ngl = dt_(-G) / L
    dy = np.empty_like(y)
    dy[:, 0] = y[:, 1]
    dy[:, 1] = ngl * s
    dy[:, 2:5] = y[:, 5:8]
    dy[:, 5:8] = (ngl * c)[:, None] * y[:, 2:5]
    dy[:, 7] += dt_(G) / (L * L) * s
    return dy


def solve(z0, L, ts, dt, solver=EULER_HEUN, seed=0, offset=0, epoch=0, first=0, sigma=SIGMA, maxiters=100000, dtype=np.float64):
    """z0 [B, 2], L [B] or [B, 1], ts [T] → ẑ [T, B, 2], J [T, B, 2, 3] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(x₀, v₀, L)_q), ret [B].
    `sigma=0` gives the deterministic scheme on the same substeps."""
    z0 = np.asarray(z0, dtype)
    L = np.asarray(L, dtype).reshape(-1)
    B, T = z0.shape[0], len(ts)
    y = np.zeros((B, 8), dtype)
    y[:, 0:2] = z0
    y[:, 2] = 1
    y[:, 6] = 1
    z = np.empty((T, B, 2), dtype)
    J = np.empty((T, B, 2, 3), dtype)

    def save(j):
        z[j] = y[:, 0:2]
        J[j] = y[:, 2:8].reshape(B, 2, 3)

    save(0)
    pl = plan(ts, dt)
    if sum(n for n, _ in pl) > maxiters:
        z[:], J[:] = np.nan, 0
        return z, J, np.full(B, 1, np.int32)
    off = int(offset) + int(epoch)
    s = 0
    with np.errstate(over="ignore"):
        for j, (n, hd) in enumerate(pl, start=1):
            h = dtype(np.float32(hd))          # the state advances by the f32 of the f64 quotient, whatever the arithmetic
            sw = dtype(sigma) * np.sqrt(h)
            for _ in range(n):
                xx, xv = xi(B, s, seed, off, first, dtype)
                dW = np.zeros((B, 8), dtype)
                dW[:, 0], dW[:, 1] = sw * xx, sw * xv
                k0 = _f(y, L)
                if solver == EM:
                    y = y + h * k0 + dW
                else:
                    k1 = _f(y + h * k0 + dW, L)
                    y = y + (dtype(0.5) * h) * (k0 + k1) + dW
                s += 1
            save(j)
    return z, J, np.zeros(B, np.int32)


def pullback(J, dz):
    """dz0 [B, 2], dL [B, 1] from J [T, B, 2, 3] and the cotangent dz [T, B, 2]."""
    g = np.einsum("tbiq,tbi->bq", np.asarray(J, np.float64), np.asarray(dz, np.float64))
    return g[:, 0:2], g[:, 2:3]


def inputs(B, seed=0):
    """x₀, v₀ ~ U(−1.5, 1.5), L ~ U(0.8, 2) as float32 arrays z0 [B, 2], L [B, 1]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 1.5, (B, 2)).astype(np.float32), rng.uniform(0.8, 2.0, (B, 1)).astype(np.float32)


def cotangent(T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, 2)) / (B * T)).astype(np.float32)


def ragged_grid(seed=3):
    """Nine save times whose eight intervals are drawn from U(0.01, 0.13): 1 to 3 unequal substeps each at dt = 0.05."""
    return np.concatenate([[0.0], np.cumsum(np.random.default_rng(seed).uniform(0.01, 0.13, 8))])


def noise_statistics(v_end, v0, t_end, B):
    """(mean of v(T) − v₀ in standard errors, relative deviation of its variance from σ²·t_end in units of √(2/B))."""
    d = np.asarray(v_end, np.float64) - v0
    var = SIGMA ** 2 * t_end
    return d.mean() / np.sqrt(var / B), (d.var() / var - 1.0) / np.sqrt(2.0 / B)


# the statistics case of tests/test_sde_host.py and tests/test_gpu_sde.py: L = 1e30 switches the drift in v off
STAT = dict(seed=12, B=4096, L=1e30, v0=0.3, ts=0.05 * np.arange(21), dt=0.05)


# the parity cases of tests/test_gpu_sde.py (and of the f32-against-f64 check in tests/test_sde_host.py)
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]
