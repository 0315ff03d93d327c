"""The Kuramoto system (include/lde.h: "the Kuramoto system"; LDE_SENSE_FORWARD_DUAL) for the numpy restatement of the solve on dual
numbers, tests/dual_ref.py: N phase oscillators dφ_i = ω_i + (K/N) Σ_j sin(φ_j − φ_i) carried as values and NP = 2N + 1 partials per component,
∂φ/∂(φ₀ (N), ω (N), K). This module holds the right-hand side on duals and the inputs; `solve` and `pullback` are tests/dual_ref.py's on this
system (the solvers, the step control on N components, the three ways to choose the steps: see there).

The right-hand side in mean-field form: s = sin φ, c = cos φ, S = Σ s, C = Σ c, f_i = ω_i + (K/N)(c_i S − s_i C); ∂f_i/∂φ_j = (K/N)(c_i c_j +
s_i s_j) for j ≠ i, ∂f_i/∂φ_i = −(K/N)(c_i C + s_i S − 1), ∂f_i/∂ω_j = δ_ij, ∂f_i/∂K = (c_i S − s_i C)/N.

Test infrastructure only, pinned on the CPU by tests/test_kuramoto_host.py (its J against central differences of its own values, the
uncoupled closed form, the conserved phase sum, the two-oscillator closed form)."""
import numpy as np

from tests import dual_ref
from tests.dual_ref import A, BT, R, R1, RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, _lincomb, _opts, grid, ragged_grid  # noqa: F401


def n_partials(N):
    return 2 * N + 1


def group_width(N):
    """Lanes of a trajectory in k_forward_dual_dir (csrc/lde_host.h: dir_group_width)."""
    return 8 if N <= 3 else 16


def rhs(u, th, N):
    """f on duals: u [G, N + N·NP] = [φ (N), ∂φ_i/∂q row by row], th [G, N + 1] → du of the same shape."""
    NP = n_partials(N)
    G = u.shape[0]
    dtype = u.dtype.type
    om, kn = th[:, :N], th[:, N] * dtype(1.0 / N)
    phi, P = u[:, :N], u[:, N:].reshape(G, N, NP)
    s, c = np.sin(phi), np.cos(phi)
    S, C = s.sum(axis=1, keepdims=True), c.sum(axis=1, keepdims=True)
    g = c * S - s * C                                        # Σ_j sin(φ_j − φ_i)
    du = np.empty_like(u)
    du[:, :N] = om + kn[:, None] * g
    jac = c[:, :, None] * c[:, None, :] + s[:, :, None] * s[:, None, :]     # cos(φ_j − φ_i)
    idx = np.arange(N)
    jac[:, idx, idx] = -(c * C + s * S - dtype(1))
    jac = kn[:, None, None] * jac
    dP = np.einsum("gij,gjq->giq", jac, P).astype(u.dtype)
    dP[:, idx, N + idx] += dtype(1)
    dP[:, :, 2 * N] += g * dtype(1.0 / N)
    du[:, N:] = dP.reshape(G, N * NP)
    return du


def system(N):
    return dual_ref.System(N, n_partials(N), lambda u, th: rhs(u, th, N))


def solve(z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, N], theta [B, N + 1] = (ω₁ … ω_N, K), ts [T] → ẑ [T, B, N], J [T, B, N, 2N + 1] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(φ₀, ω, K)_q), ret [B],
    info: tests/dual_ref.py's solve on this system."""
    return dual_ref.solve(system(np.shape(z0)[1]), z0, theta, ts, solver, adaptive, dt, steps, dtype, **opts)


def pullback(J, dz):
    """dz0 [B, N], dθ [B, N + 1] from J [T, B, N, 2N + 1] and the cotangent dz [T, B, N] (f64)."""
    return dual_ref.pullback(system(J.shape[2]), J, dz)


def inputs(B, N, seed=0):
    """φ₀ ~ U(−π, π), ω ~ U(0.5, 2), K ~ U(0.5, 2) as float32 arrays z0 [B, N], theta [B, N + 1]."""
    rng = np.random.default_rng(seed)
    z0 = rng.uniform(-np.pi, np.pi, (B, N)).astype(np.float32)
    th = np.concatenate([rng.uniform(0.5, 2.0, (B, N)), rng.uniform(0.5, 2.0, (B, 1))], axis=1).astype(np.float32)
    return z0, th


def turn_inputs(B, N):
    """The inputs of the tests of phases past 256 turns: seed 23 with TURNS whole turns added in f64, then rounded to f32 once."""
    z0, th = inputs(B, N, seed=23)
    return (z0.astype(np.float64) + 2 * np.pi * TURNS).astype(np.float32), th


def cotangent(T, B, N, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, N)) / (B * T)).astype(np.float32)


# the parity cases of tests/test_gpu_kuramoto.py (and of the f32-against-f64 floor in tests/test_kuramoto_host.py): G = 8 with 3 pad lanes and
# with 1, G = 16 with 7 and with 1; one trajectory, a last workgroup of partial groups, several workgroups
NS = [2, 3, 4, 7]
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]
TURNS = 300                 # the whole turns added to φ₀ in the test of phases past the hardware sine's 256
