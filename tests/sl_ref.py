"""The Stuart–Landau network (include/lde.h: "the Stuart–Landau network"; LDE_RHS_STUART_LANDAU, LDE_SENSE_FORWARD_DUAL) for the numpy
restatement of the solve on dual numbers, tests/dual_ref.py: N = 1 … 3 Hopf normal-form oscillators with uniform all-to-all diffusive coupling,
z = (x₁ … x_N, y₁ … y_N), θ = (a₁ … a_N, ω₁ … ω_N, G), carried as values and NP = 4N + 1 partials per component, ∂z/∂(ẑ₀ (2N), a (N), ω (N), G).
The form is recalled from the literature (Deco et al.'s whole-brain Hopf model with uniform coupling), unpinned (include/lde.h says so):
include/lde.h's text is the contract, and `rhs_plain` is that text.

Two solves:
  * deterministic — `solve` / `pullback` are tests/dual_ref.py's on `system(N)`;
  * stochastic — `sde_solve`: StochasticDiffEq's EM() and EulerHeun() at a fixed step on duals, dz = f(z) dt + σ dW with diagonal additive noise
    of one σ, along the path the library's counter layout draws (`xi`): component c takes word c mod 4 of Philox block ⌊c/4⌋ of (trajectory,
    substep); words (0, 1) and (2, 3) are Box–Muller pairs by lde_randn's map; block 0 has the stochastic pendulum's counter and key
    (tests/sde_ref.py: xi), block 1 the same counter and the key with the top bit of its high word flipped (seed xor 2⁶³). The tangents get
    no noise. float64 by default; `dtype=np.float32` runs the same formulas in f32.

Test infrastructure only, pinned on the CPU by tests/test_sl_host.py (its values against `rhs_plain`, its J against central differences of its
own values, its stochastic partials against central differences with the noise held fixed, the closed form of the uncoupled a < 0 radius,
RK4's order, the noise against the definition, and every f32-against-f64 floor under the GPU bounds)."""
import numpy as np

from tests import dual_ref
from tests import philox_ref as P
from tests import sde_ref
from tests.dual_ref import RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, grid  # noqa: F401

KIND = 13
EM, EULER_HEUN = 2, 3
SIGMA = 0.01
NS = (1, 2, 3)
GROUP = {1: 8, 2: 16, 3: 16}      # lanes of a trajectory in the lane-per-direction kernels: 3, 7 and 3 of them pad lanes


def dims(N):
    """(D, P, NP) = (2N, 2N + 1, 4N + 1)."""
    return 2 * N, 2 * N + 1, 4 * N + 1


def _rhs(N):
    D, _, NP = dims(N)

    def rhs(u, th):
        """f on duals: u [n, D + D·NP] = [z (D), ∂z_i/∂q row by row], th [n, 2N + 1] = (a, ω, G) → du of the same shape."""
        n = u.shape[0]
        dtype = u.dtype.type
        z, Pz = u[:, :D], u[:, D:].reshape(n, D, NP)
        x, y, vx, vy = z[:, :N], z[:, N:], Pz[:, :N], Pz[:, N:]
        a, om, g = th[:, :N], th[:, N:2 * N], th[:, 2 * N]
        iN = dtype(1.0 / N)
        xm, ym = x.sum(axis=1) * iN, y.sum(axis=1) * iN
        vxm, vym = vx.sum(axis=1) * iN, vy.sum(axis=1) * iN                         # [n, NP]
        c = a - (x * x + y * y)
        dxm, dym = xm[:, None] - x, ym[:, None] - y
        du = np.empty_like(u)
        du[:, :N] = c * x - om * y + g[:, None] * dxm
        du[:, N:D] = c * y + om * x + g[:, None] * dym
        s2 = dtype(2) * (x[..., None] * vx + y[..., None] * vy)                      # [n, N, NP]
        fx, fy = np.zeros((n, N, NP), u.dtype), np.zeros((n, N, NP), u.dtype)      # the forcing columns ∂f/∂(a, ω, G)
        for j in range(N):
            fx[:, j, 2 * N + j], fy[:, j, 2 * N + j] = x[:, j], y[:, j]
            fx[:, j, 3 * N + j], fy[:, j, 3 * N + j] = -y[:, j], x[:, j]
            fx[:, j, 4 * N], fy[:, j, 4 * N] = dxm[:, j], dym[:, j]
        g3, c3, om3 = g[:, None, None], c[..., None], om[..., None]
        dvx = c3 * vx - s2 * x[..., None] - om3 * vy + g3 * (vxm[:, None, :] - vx) + fx
        dvy = c3 * vy - s2 * y[..., None] + om3 * vx + g3 * (vym[:, None, :] - vy) + fy
        du[:, D:] = np.concatenate([dvx, dvy], axis=1).reshape(n, D * NP)
        return du

    return rhs


_SYSTEMS = {N: dual_ref.System(2 * N, 4 * N + 1, _rhs(N)) for N in NS}


def system(N):
    return _SYSTEMS[N]


def rhs_plain(z, th):
    """The right-hand side as include/lde.h states it, values only, oscillator by oscillator: z [n, 2N], th [n, 2N + 1] → dz [n, 2N]."""
    N = z.shape[1] // 2
    x, y = z[:, :N], z[:, N:]
    a, om, G = th[:, :N], th[:, N:2 * N], th[:, 2 * N]
    xbar, ybar = x.mean(axis=1), y.mean(axis=1)
    dz = np.empty_like(z)
    for j in range(N):
        r2 = x[:, j] ** 2 + y[:, j] ** 2
        dz[:, j] = (a[:, j] - r2) * x[:, j] - om[:, j] * y[:, j] + G * (xbar - x[:, j])
        dz[:, N + j] = (a[:, j] - r2) * y[:, j] + om[:, j] * x[:, j] + G * (ybar - y[:, j])
    return dz


def jacobian_plain(z, th):
    """∂f/∂z [2N, 2N] and ∂f/∂θ [2N, 2N + 1] of ONE state, entry by entry as include/lde.h states them."""
    N = len(z) // 2
    x, y = z[:N], z[N:]
    a, om, G = th[:N], th[N:2 * N], th[2 * N]
    Jz, Jt = np.zeros((2 * N, 2 * N)), np.zeros((2 * N, 2 * N + 1))
    for j in range(N):
        r2 = x[j] ** 2 + y[j] ** 2
        for i in range(N):
            Jz[j, i] = Jz[N + j, N + i] = G / N
        Jz[j, j] = a[j] - r2 - 2 * x[j] ** 2 - G * (1 - 1 / N)
        Jz[N + j, N + j] = a[j] - r2 - 2 * y[j] ** 2 - G * (1 - 1 / N)
        Jz[j, N + j] = -2 * x[j] * y[j] - om[j]
        Jz[N + j, j] = -2 * x[j] * y[j] + om[j]
        Jt[j, j], Jt[N + j, j] = x[j], y[j]
        Jt[j, N + j], Jt[N + j, N + j] = -y[j], x[j]
        Jt[j, 2 * N], Jt[N + j, 2 * N] = x.mean() - x[j], y.mean() - y[j]
    return Jz, Jt


def solve(N, z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, 2N], theta [B, 2N + 1], ts [T] → ẑ [T, B, 2N], J [T, B, 2N, 4N + 1] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(ẑ₀, θ)_q), ret [B], info:
    tests/dual_ref.py's solve on this system."""
    return dual_ref.solve(system(N), z0, theta, ts, solver, adaptive, dt, steps, dtype, **opts)


def pullback(N, J, dz):
    """dz0 [B, 2N], dθ [B, 2N + 1] from J [T, B, 2N, 4N + 1] and the cotangent dz [T, B, 2N] (f64)."""
    return dual_ref.pullback(system(N), J, dz)


def xi(B, s, D, seed=0, off=0, first=0, dtype=np.float64):
    """ξ [B, D] of trajectories first … first + B − 1 at substep s, by the counter layout of include/lde.h ("the Stuart–Landau network")."""
    off &= 0xFFFFFFFFFFFFFFFF
    b = (np.arange(B, dtype=np.uint64) + np.uint64(first & 0xFFFFFFFFFFFFFFFF)) & P.MASK
    out = np.empty((B, D), dtype)
    for m in range((D + 3) // 4):
        k_hi = ((seed >> 32) & 0xFFFFFFFF) ^ (0x80000000 if m else 0)
        w = P.philox4x32_10(b, s & 0xFFFFFFFF, off & 0xFFFFFFFF, off >> 32, seed & 0xFFFFFFFF, k_hi)
        for p in range(2):
            c = 4 * m + 2 * p
            if c < D:
                u1 = ((w[2 * p] >> np.uint64(8)).astype(dtype) + dtype(0.5)) * dtype(1.0 / 16777216.0)
                u2 = ((w[2 * p + 1] >> np.uint64(8)).astype(dtype) + dtype(0.5)) * dtype(1.0 / 16777216.0)
                r = np.sqrt(dtype(-2.0) * np.log(u1))
                ang = dtype(2.0 * np.pi) * u2
                out[:, c], out[:, c + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


plan = sde_ref.plan


def sde_solve(N, z0, theta, ts, dt, solver=EULER_HEUN, seed=0, offset=0, epoch=0, first=0, sigma=SIGMA, maxiters=100000, dtype=np.float64):
    """z0 [B, 2N], theta [B, 2N + 1], ts [T] → ẑ [T, B, 2N], J [T, B, 2N, 4N + 1], ret [B]. `sigma=0` gives the deterministic scheme on the
    same substeps."""
    D, _, NP = dims(N)
    sys = system(N)
    z0 = np.asarray(z0, dtype)
    B, T = z0.shape[0], len(ts)
    th = np.asarray(theta, dtype).reshape(B, -1)
    y = np.zeros((B, D + D * NP), dtype)
    y[:, :D] = z0
    for i in range(D):
        y[:, D + NP * i + i] = 1
    z, J = np.empty((T, B, D), dtype), np.empty((T, B, D, NP), dtype)

    def save(j):
        z[j] = y[:, :D]
        J[j] = y[:, D:].reshape(B, D, NP)

    save(0)
    pl = plan(ts, dt)
    if sum(n for n, _ in pl) > maxiters:
        z[:], J[:] = np.nan, 0
        return z, J, np.full(B, RET_MAXITERS, np.int32)
    off = int(offset) + int(epoch)
    s = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for j, (n, hd) in enumerate(pl, start=1):
            h = dtype(np.float32(hd))          # the state advances by the f32 of the f64 quotient, whatever the arithmetic
            sw = dtype(sigma) * np.sqrt(h)
            for _ in range(n):
                dW = np.zeros_like(y)
                dW[:, :D] = sw * xi(B, s, D, seed, off, first, dtype)
                k0 = sys.rhs(y, th)
                if solver == EM:
                    y = y + h * k0 + dW
                else:
                    k1 = sys.rhs(y + h * k0 + dW, th)
                    y = y + (dtype(0.5) * h) * (k0 + k1) + dW
                s += 1
            save(j)
    ret = np.zeros(B, np.int32)
    bad = ~np.isfinite(z).all(axis=(0, 2)) | ~np.isfinite(J).all(axis=(0, 2, 3))
    if bad.any():
        z[:, bad], J[:, bad], ret[bad] = np.nan, 0, RET_NONFINITE
    return z, J, ret


def inputs(N, B, seed=0):
    """x₀, y₀ ~ U(−1, 1), a ~ U(−0.5, 1), ω ~ U(0.5, 3), G ~ U(0, 1) as float32 arrays z0 [B, 2N], theta [B, 2N + 1]: both sides of the
    bifurcation."""
    rng = np.random.default_rng(seed)
    z0 = rng.uniform(-1.0, 1.0, (B, 2 * N))
    th = np.concatenate([rng.uniform(-0.5, 1.0, (B, N)), rng.uniform(0.5, 3.0, (B, N)), rng.uniform(0.0, 1.0, (B, 1))], axis=1)
    return z0.astype(np.float32), th.astype(np.float32)


def cotangent(N, T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, 2 * N)) / (B * T)).astype(np.float32)


def radius_closed_form(a, r0, t):
    """r(t) of one uncoupled oscillator, from r' = (a − r²) r: r² = a / (1 − (1 − a/r₀²)·e^(−2at)) (a ≠ 0)."""
    return np.sqrt(a / (1.0 - (1.0 - a / r0 ** 2) * np.exp(-2.0 * a * t)))


def ragged_grid():
    """tests/dual_ref.py's nine ragged save times: the system's first accepted steps are tenths (tests/test_sl_host.py checks on the reference's
    own steps that a step holds two save times and that one holds none)."""
    return dual_ref.ragged_grid()


sde_ragged_grid = sde_ref.ragged_grid          # nine save times, 1 to 3 unequal substeps per interval at dt = 0.05


def noise_statistics(z_end, t_end, B, sigma=SIGMA):
    """Per component of z(t_end) [B, D] started at 0 with θ = 0: (mean in standard errors, relative deviation of the variance from σ²·t_end in
    units of √(2/B)) — tests/sde_ref.py's statistics, component by component."""
    d = np.asarray(z_end, np.float64)
    var = sigma ** 2 * t_end
    return d.mean(axis=0) / np.sqrt(var / B), (d.var(axis=0) / var - 1.0) / np.sqrt(2.0 / B)


# the parity cases of tests/test_gpu_sl.py and tests/test_gpu_sl_sde.py (and of the f32-against-f64 floors in tests/test_sl_host.py): one
# trajectory, a last workgroup of partial waves, several workgroups
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]
PARITY_SEED = {1: 1, 2: 2, 50: 5}                     # by T, the seed of the fixed-step parity inputs
ADAPTIVE_SEED, RAGGED_SEED, LONG_SEED, SDE_RAGGED_SEED = 7, 8, 9, 10
ADAPTIVE_SHAPE = (50, 37)
NOISE_SEED = 5                                        # the Philox seed of the stochastic parity cases

# the statistics case of tests/test_sl_host.py and tests/test_gpu_sl_sde.py: ẑ₀ = 0 and θ = 0 — the drift is −r²·z, cubic in a state of size
# σ√t = 0.01, so z(t_end) is the noise sum to about 1e-4 relative. The seed is one at which this reference sits inside the gates (|mean| ≤ 4
# standard errors, |variance − σ²t| ≤ 4·√(2/B)·σ²t: tests/test_gpu_sde.py's) for every N and both solvers, checked on the CPU.
STAT = dict(seed=12, B=4096, ts=0.05 * np.arange(21), dt=0.05)

# The GPU tests' bounds (ẑ, J, dz0, dθ; each relative to the largest entry of the reference array): the project's standing ones. Every case's
# f32-against-f64 floor is measured and asserted to be within a quarter of them by tests/test_sl_host.py — none comes from a kernel's output.
# Measured floors (ẑ / J / dz0 / dθ), the worst over N = 1, 2, 3, (2, 37) and (50, 256), dt = 0.05 and 0.0125:
#   Tsit5 fixed-step      7.4e-7 / 8.2e-7 / 6.5e-7 / 6.8e-7        RK4            5.3e-7 / 6.2e-7 / 7.7e-7 / 4.7e-7
#   EM                    6.1e-7 / 7.0e-7 / 5.1e-7 / 3.8e-7        EulerHeun      6.8e-7 / 8.6e-7 / 3.0e-7 / 2.7e-7
#   the stochastic ragged grid (256 trajectories) at most 2.5e-7 / 3.0e-7 / 1.5e-7 / 1.3e-7
# — all within a twentieth of the bounds, so none is widened: the resulting bounds are the standing ones for every case, deterministic and
# stochastic. (|ẑ| ≤ 1.2 and |J| ≤ 6.4 on these inputs.)
BOUNDS = (2e-5, 1e-4, 1e-4, 1e-4)


def bounds(*_):
    return BOUNDS


# "The noise is there": per trajectory the stochastic solve leaves the σ = 0 scheme by more than this somewhere — two thirds of the smallest
# departure of this reference over N = 1, 2, 3 × both solvers × seeds 5 and 6 on the (50, 256) parity inputs at dt = 0.05 (measured on the CPU
# by tests/test_sl_host.py::test_reference_departure_from_the_deterministic_scheme, which asserts the factor). Measured: the smallest is
# 7.9e-3 (N = 1, EulerHeun, seed 5); N = 3's smallest is 1.18e-2.
MIN_DEPARTURE = 5.2e-3
