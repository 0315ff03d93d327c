"""The cardiovascular system (include/lde.h: "the cardiovascular system"; LDE_RHS_CVS, LDE_SENSE_FORWARD_DUAL) for the numpy restatement of the
solve on dual numbers, tests/dual_ref.py: z = (p_a/100, p_v/10, s, sv/100), θ = (i_ext, r_mod), carried as values and NP = 6 partials per
component, ∂z/∂(ẑ₀ (4), i_ext, r_mod). This module holds the right-hand side on duals, the blood volume, the inputs and the GPU tests' bounds;
`solve` and `pullback` are tests/dual_ref.py's on this system. The form of the system is the GOKU-net authors' data generator's as recalled,
unpinned (include/lde.h says so): include/lde.h's text is the contract, and `rhs_plain` is that text.

The right-hand side, as csrc/lde_cvs_dualrhs.h evaluates it, in the scaled state with the constants folded:
    f_hr  = s·(F_MAX − F_MIN) + F_MIN,   r_tpr = s·(R_MAX − R_MIN) + (R_MIN − r_mod),   dva = 100·z₃·f_hr − (100·z₀ − 10·z₁)/r_tpr
    z₀' = dva/400,   z₁' = (i_ext − dva)/1110,   z₂' = (w − s)/TAU,   z₃' = i_ext·SV_MOD
with w = 1 − σ(K_W·(p_a − P_SET)) = 1/(1 + eˣ) and its partial −K_W·w·(1 − w)·∂p_a written out: finite where eˣ is inf or 0.

Test infrastructure only, pinned on the CPU by tests/test_cvs_host.py (its values against `rhs_plain`, its J against central differences of
its own values, the exact fourth row, the blood volume, RK4's order, the saturated baroreflex, and every f32-against-f64 floor under the GPU
bounds)."""
import numpy as np

from tests import dual_ref
from tests.dpend_ref import Dual
from tests.dual_ref import RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, grid  # noqa: F401

D, P, NP, G = 4, 2, 6, 8        # components, parameters, partial directions, lanes of a trajectory in k_forward_dual_dir (lanes 6, 7: pad)
F_MAX, F_MIN, R_MAX, R_MIN, C_A, C_V = 3.0, 2.0 / 3.0, 2.134, 0.5335, 4.0, 111.0
K_W, P_SET, TAU, SV_MOD = 0.1838, 70.0, 20.0, 0.001


def rhs(u, th):
    """f on duals: u [n, 4 + 4·6] = [z (4), ∂z_i/∂q row by row], th [n, 2] = (i_ext, r_mod) → du of the same shape."""
    n = u.shape[0]
    dtype = u.dtype.type
    z, Pz = u[:, :D], u[:, D:].reshape(n, D, NP)

    def par(v, q, dv):
        d = np.zeros((n, NP), u.dtype)
        d[:, q] = dv
        return Dual(v, d)

    ie, rm = th[:, 0], th[:, 1]
    iext, rbase = par(ie, 4, dtype(1)), par(dtype(R_MIN) - rm, 5, dtype(-1))
    dz3 = par(ie * dtype(SV_MOD), 4, dtype(SV_MOD))
    Z0, Z1, S, Z3 = (Dual(z[:, i], Pz[:, i]) for i in range(4))
    fhr = S * (F_MAX - F_MIN) + F_MIN
    rr = (S * (R_MAX - R_MIN) + rbase).rcp()
    dva = Z3 * 100.0 * fhr - (Z0 * 100.0 - Z1 * 10.0) * rr
    r0, r1 = dva * (1.0 / (C_A * 100.0)), (iext - dva) * (1.0 / (C_V * 10.0))
    with np.errstate(over="ignore"):
        e = np.exp(z[:, 0] * dtype(K_W * 100.0) - dtype(K_W * P_SET))
    w = dtype(1) / (dtype(1) + e)
    W = Dual(w, (dtype(-K_W * 100.0) * (w * (dtype(1) - w)))[:, None] * Pz[:, 0])
    r2 = (W - S) * (1.0 / TAU)
    du = np.empty_like(u)
    du[:, 0], du[:, 1], du[:, 2], du[:, 3] = r0.v, r1.v, r2.v, dz3.v
    du[:, D:] = np.stack([r0.d, r1.d, r2.d, dz3.d], axis=1).reshape(n, D * NP)
    return du


def rhs_plain(z, th):
    """The right-hand side as include/lde.h states it, values only: z [n, 4], th [n, 2] → dz [n, 4]."""
    p_a, p_v, s, sv = 100.0 * z[:, 0], 10.0 * z[:, 1], z[:, 2], 100.0 * z[:, 3]
    i_ext, r_mod = th[:, 0], th[:, 1]
    f_hr = s * (F_MAX - F_MIN) + F_MIN
    r_tpr = s * (R_MAX - R_MIN) + R_MIN - r_mod
    dva = -(p_a - p_v) / r_tpr + sv * f_hr
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-K_W * (p_a - P_SET)))
    return np.stack([dva / (C_A * 100.0), (-dva + i_ext) / (C_V * 10.0), (1.0 - sig - s) / TAU, i_ext * SV_MOD], axis=1)


def volume(z, th, t):
    """400·z₀ + 1110·z₁ − i_ext·t of z [T, B, 4] with th [B, 2] and t [T]: the blood volume less what flowed in, constant along a solution."""
    return 400.0 * z[..., 0] + 1110.0 * z[..., 1] - th[None, :, 0] * np.asarray(t, np.float64)[:, None]


SYSTEM = dual_ref.System(D, NP, rhs)


def solve(z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, 4], theta [B, 2] = (i_ext, r_mod), ts [T] → ẑ [T, B, 4], J [T, B, 4, 6] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(ẑ₀, θ)_q), ret [B], info:
    tests/dual_ref.py's solve on this system."""
    return dual_ref.solve(SYSTEM, z0, theta, ts, solver, adaptive, dt, steps, dtype, **opts)


def pullback(J, dz):
    """dz0 [B, 4], dθ [B, 2] from J [T, B, 4, 6] and the cotangent dz [T, B, 4] (f64)."""
    return dual_ref.pullback(SYSTEM, J, dz)


def inputs(B, seed=0):
    """z₀ ~ U(0.75, 0.85), z₁ ~ U(0.5, 0.9), z₂ ~ U(0.15, 0.25), z₃ ~ U(0.9, 1.0), i_ext ~ U(−2, 0), r_mod ~ U(0, 0.3) as float32 arrays z0 [B, 4],
    theta [B, 2]: pressures around the set point, a bleeding patient, a lowered resistance."""
    rng = np.random.default_rng(seed)
    z0 = np.stack([rng.uniform(0.75, 0.85, B), rng.uniform(0.5, 0.9, B), rng.uniform(0.15, 0.25, B), rng.uniform(0.9, 1.0, B)], axis=1)
    th = np.stack([rng.uniform(-2.0, 0.0, B), rng.uniform(0.0, 0.3, B)], axis=1)
    return z0.astype(np.float32), th.astype(np.float32)


def saturated_inputs(B, p_a, seed=31):      # (SATURATED_SEED)
    """`inputs` with the arterial pressure p_a (2000 or 0: z₀ = 20 or 0) on every trajectory: the baroreflex's eˣ is inf or ≈ 0."""
    z0, th = inputs(B, seed=seed)
    z0[:, 0] = np.float32(p_a / 100.0)
    return z0, th


def cotangent(T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, D)) / (B * T)).astype(np.float32)


def volume_cotangent(T, B, ts, seed=5):
    """The cotangent c_j·(400, 1110, 0, 0) [T, B, 4] (f32) with the pullback the volume's tangent gives it exactly: dz0 = (400 Σc, 1110 Σc, 0, 0)
    [B, 4] and dθ = (Σ_j c_j t_j, 0) [B, 2] (f64, from the f32 c)."""
    c = (np.random.default_rng(seed).standard_normal((T, B)) / (B * T)).astype(np.float32)
    dz = np.zeros((T, B, D), np.float32)
    dz[:, :, 0], dz[:, :, 1] = np.float32(400.0) * c, np.float32(1110.0) * c
    c64 = c.astype(np.float64)
    want0, wantth = np.zeros((B, D)), np.zeros((B, P))
    want0[:, 0], want0[:, 1] = 400.0 * c64.sum(axis=0), 1110.0 * c64.sum(axis=0)
    wantth[:, 0] = np.einsum("t,tb->b", np.asarray(ts, np.float64), c64)
    return dz, want0, wantth


def slow_grid(T):
    """1.0·j: the system's own time scale (TAU = 20) and the paper's Δt = 1."""
    return 1.0 * np.arange(T)


RAGGED_STRETCH = 20.0


def ragged_grid():
    """tests/dual_ref.py's nine ragged save times stretched by a constant: this system's first accepted steps are seconds long, not hundredths
    (tests/test_cvs_host.py checks on the reference's own steps that a step holds two save times and that one holds none)."""
    return RAGGED_STRETCH * dual_ref.ragged_grid()


# the parity cases of tests/test_gpu_cvs.py (and of the f32-against-f64 floor in tests/test_cvs_host.py): one trajectory, a last workgroup of
# partial waves, several workgroups
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]
SLOW_DT, SLOW_SHAPE = 0.25, (50, 37)

# The GPU tests' inputs and bounds (ẑ, J, dz0, dθ; each relative to the largest entry of the reference array). The bounds are the dual tests'
# (tests/test_gpu_lv.py) wherever this reference's own f32 mode stays within a quarter of them on the test's inputs; where it does not, the
# case's bound is 4 × that floor, rounded up. Every floor is measured and asserted on the CPU by tests/test_cvs_host.py — none comes from a
# kernel's output; the seeds were fixed there too.
#
# Measured floors (ẑ / J / dz0 / dθ) and the largest |J|:
#   (50, 256) on `grid`, dt = 0.05, Tsit5 and RK4     1.5e-6 / 9.7e-7 / 3.1e-7 / 3.5e-7     1.77      the standing bounds
#   (50, 256) on `grid`, dt = 0.0125, both            5.8e-6 / 2.9e-6 / 1.3e-6 / 8.0e-7     1.77      ẑ over a quarter of 2e-5: 4 × 5.8e-6 → 2.5e-5
#   (50, 37) on `slow_grid`, dt = 0.25, both          5.6e-6 / 2.8e-6 / 1.2e-6 / 1.4e-6     2.24      ẑ likewise → 2.5e-5
#   adaptive 1e-6 / 1e-3 on `slow_grid`, replayed     1.9e-6 / 2.2e-6 / 6.9e-7 / 8.8e-7     2.35      the standing bounds
#   ragged grid 8.6e-7 / 1.0e-6 / 7.5e-7 / 1.3e-6; T = 6001 2.2e-6 / 2.3e-6 / 4.0e-7 / 1.7e-7; p_a(0) = 2000 and 0 at most 5.6e-7 / 2.3e-7 / 1.2e-7 / 6.7e-7
# (the ẑ floor of the long fixed-step solves is the rounding of 196 f32 state updates, not the system: it is smooth and not stiff)
BOUNDS = (2e-5, 1e-4, 1e-4, 1e-4)
FINE_BOUNDS = (2.5e-5, 1e-4, 1e-4, 1e-4)              # dt = 0.0125 on (50, 256), and dt = 0.25 on `slow_grid` (50, 37)
PARITY_SEED = {1: 1, 2: 2, 50: 5}                     # by T, the seed of the fixed-step parity inputs
SLOW_SEED, ADAPTIVE_SEED, RAGGED_SEED, LONG_SEED, SATURATED_SEED = 6, 7, 8, 9, 31


def bounds(solver, dt, T=50):
    return FINE_BOUNDS if (dt == 0.0125 and T == 50) else BOUNDS


def volume_bounds(solver, dt):
    """(drift of the volume, dz0, dθ) of the blood-volume test on (50, 256): the case's ẑ, dz0 and dθ bounds, but for dθ at dt = 0.0125. There
    the reference's f32 mode is 4.2e-5 (Tsit5) / 5.0e-5 (RK4) from (Σ c_j t_j, 0) — the cotangent weighs J[1, i_ext] ≈ t/1110 with 1110, so
    an f32 rounding of J (1e-6 of its largest entry, 1.77) is 2e-3 against t ≤ 2.45 — over a quarter of 1e-4: 4 × 5.0e-5, rounded up.
    (dt = 0.05: 2.2e-5, within a quarter.)"""
    b = bounds(solver, dt, 50)
    return b[0], b[2], 2.1e-4 if dt == 0.0125 else b[3]
