"""The Lotka–Volterra system (include/lde.h: "the Lotka–Volterra system"; LDE_SENSE_FORWARD_DUAL) for the numpy restatement of the solve on
dual numbers, tests/dual_ref.py: dx = αx − βxy, dy = −γy + δxy carried as values and NP = 6 partials per component,
∂(x, y)/∂(x₀, y₀, α, β, γ, δ). This module holds the right-hand side on duals, the inputs and the conserved quantity; `solve` and `pullback`
are tests/dual_ref.py's on this system (the solvers, the step control, the three ways to choose the steps: see there).

Test infrastructure only, pinned on the CPU by tests/test_lv_host.py (its J against central differences of its own values, the closed form
at β = δ = 0, the conserved quantity)."""
import numpy as np

from tests import dual_ref
from tests.dual_ref import A, BT, R, R1, RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, _lincomb, _opts, grid, ragged_grid  # noqa: F401

NP, DN = 6, 14          # partials per component; floats of a dual state [x, y, ∂x/∂q (6), ∂y/∂q (6)]


def rhs(u, th):
    """f on duals: u [G, 14], th [G, 4] → du [G, 14]. ∂f/∂u = [[α − βy, −βx], [δy, −γ + δx]], ∂f/∂θ = [[x, −xy, 0, 0], [0, 0, −y, xy]]."""
    al, be, ga, de = th[:, 0], th[:, 1], th[:, 2], th[:, 3]
    x, y = u[:, 0], u[:, 1]
    xy = x * y
    du = np.empty_like(u)
    du[:, 0] = al * x - be * xy
    du[:, 1] = de * xy - ga * y
    px, py = u[:, 2:2 + NP], u[:, 2 + NP:]
    du[:, 2:2 + NP] = (al - be * y)[:, None] * px + (-be * x)[:, None] * py
    du[:, 2 + NP:] = (de * y)[:, None] * px + (de * x - ga)[:, None] * py
    du[:, 2 + 2] += x
    du[:, 2 + 3] -= xy
    du[:, 2 + NP + 4] -= y
    du[:, 2 + NP + 5] += xy
    return du


SYSTEM = dual_ref.System(2, NP, rhs)


def solve(z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, 2], theta [B, 4] = (α, β, γ, δ), ts [T] → ẑ [T, B, 2], J [T, B, 2, 6] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(x₀, y₀, α, β, γ, δ)_q), ret [B], info:
    tests/dual_ref.py's solve on this system."""
    return dual_ref.solve(SYSTEM, z0, theta, ts, solver, adaptive, dt, steps, dtype, **opts)


def pullback(J, dz):
    """dz0 [B, 2], dθ [B, 4] from J [T, B, 2, 6] and the cotangent dz [T, B, 2] (f64)."""
    return dual_ref.pullback(SYSTEM, J, dz)


def inputs(B, seed=0):
    """x₀, y₀ ~ U(0.5, 2), α, β, γ, δ ~ U(0.5, 1.5) as float32 arrays z0 [B, 2], theta [B, 4]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, (B, 2)).astype(np.float32), rng.uniform(0.5, 1.5, (B, 4)).astype(np.float32)


def cotangent(T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, 2)) / (B * T)).astype(np.float32)


def invariant(z, theta):
    """V = δx − γ ln x + βy − α ln y along ẑ [T, B, 2]."""
    al, be, ga, de = (np.asarray(theta, np.float64)[:, i] for i in range(4))
    x, y = z[..., 0].astype(np.float64), z[..., 1].astype(np.float64)
    return de * x - ga * np.log(x) + be * y - al * np.log(y)


# the parity cases of tests/test_gpu_lv.py (and of the f32-against-f64 floor in tests/test_lv_host.py)
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]
