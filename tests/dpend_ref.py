"""The double pendulum (include/lde.h: "the double pendulum"; LDE_SENSE_FORWARD_DUAL) for the numpy restatement of the solve on dual numbers,
tests/dual_ref.py: z = (θ₁, θ₂, ω₁, ω₂), θ = (L₁, L₂, m₁, m₂), g = 10, carried as values and NP = 8 partials per component,
∂z/∂(ẑ₀ (4), L₁, L₂, m₁, m₂). This module holds the right-hand side on duals, the energy, the inputs and the GPU tests' bounds; `solve` and
`pullback` are tests/dual_ref.py's on this system (the solvers, the step control on four components, the three ways to choose the steps:
see there).

The right-hand side, as csrc/lde_dpend_dualrhs.h evaluates it: in the mass ratio μ = m₂/m₁ (the system is homogeneous of degree 0 in the
masses), Δ = θ₁ − θ₂, den = 2 + μ − μ cos 2Δ,
    ω₁' = [ −g(2 + μ) sin θ₁ − μ g sin(θ₁ − 2θ₂) − 2 sinΔ · μ (ω₂² L₂ + ω₁² L₁ cosΔ) ] / (L₁ · den)
    ω₂' = [ 2 sinΔ ( (1 + μ)(ω₁² L₁ + g cos θ₁) + ω₂² L₂ μ cosΔ ) ] / (L₂ · den)
with sin Δ, cos Δ, cos 2Δ and sin(θ₁ − 2θ₂) from the sines and cosines of θ₁ and θ₂ by the angle-sum identities, on numbers that carry
their eight partials (`Dual`). `rhs_plain` is the form of include/lde.h in the masses themselves, values only: what `rhs` is checked against.

Test infrastructure only, pinned on the CPU by tests/test_dpend_host.py (its J against central differences of its own values, the m₂ = 0
limit, the mass homogeneity, the energy drift under RK4)."""
import numpy as np

from tests import dual_ref
from tests.dual_ref import A, BT, R, R1, RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, _lincomb, _opts, grid, ragged_grid  # noqa: F401

D, P, NP, G = 4, 4, 8, 8        # components, parameters, partial directions, lanes of a trajectory in k_forward_dual_dir (no pad lane)
GRAV = 10.0
TURNS = 300                     # the whole turns added to θ₁, θ₂ in the test of angles past the hardware sine's 256


class Dual:
    """v [G] with its partials d [G, NP]."""

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def _lift(o, like):
        return o if isinstance(o, Dual) else Dual(like.v.dtype.type(o) + np.zeros_like(like.v), np.zeros_like(like.d))

    def __add__(self, o):
        o = Dual._lift(o, self)
        return Dual(self.v + o.v, self.d + o.d)

    def __sub__(self, o):
        o = Dual._lift(o, self)
        return Dual(self.v - o.v, self.d - o.d)

    def __mul__(self, o):
        if not isinstance(o, Dual):
            c = self.v.dtype.type(o)
            return Dual(self.v * c, self.d * c)
        return Dual(self.v * o.v, self.d * o.v[:, None] + self.v[:, None] * o.d)

    def rcp(self):
        r = self.v.dtype.type(1) / self.v
        return Dual(r, -self.d * (r * r)[:, None])


def rhs(u, th):
    """f on duals: u [G, 4 + 4·8] = [z (4), ∂z_i/∂q row by row], th [G, 4] = (L₁, L₂, m₁, m₂) → du of the same shape."""
    n = u.shape[0]
    dtype = u.dtype.type
    z, Pz = u[:, :D], u[:, D:].reshape(n, D, NP)

    def par(v, q, dv):
        d = np.zeros((n, NP), u.dtype)
        d[:, q] = dv
        return Dual(v, d)

    L1, L2, m1, m2 = (th[:, i] for i in range(4))
    one = dtype(1)
    l1, l2 = par(L1, 4, one), par(L2, 5, one)
    il1, il2 = par(one / L1, 4, -(one / L1) * (one / L1)), par(one / L2, 5, -(one / L2) * (one / L2))
    im = one / m1
    mu = par(m2 * im, 6, -(m2 * im) * im)
    mu.d[:, 7] = im
    s1, c1, s2, c2 = np.sin(z[:, 0]), np.cos(z[:, 0]), np.sin(z[:, 1]), np.cos(z[:, 1])
    S1, C1 = Dual(s1, c1[:, None] * Pz[:, 0]), Dual(c1, -s1[:, None] * Pz[:, 0])
    S2, C2 = Dual(s2, c2[:, None] * Pz[:, 1]), Dual(c2, -s2[:, None] * Pz[:, 1])
    W1, W2 = Dual(z[:, 2], Pz[:, 2]), Dual(z[:, 3], Pz[:, 3])
    sd, cd = S1 * C2 - C1 * S2, C1 * C2 + S1 * S2
    c2d = cd * cd - sd * sd
    s12 = sd * C2 - cd * S2
    rden = ((mu + 2.0) - mu * c2d).rcp()
    a, b = W1 * W1 * l1, W2 * W2 * l2
    num1 = ((mu + 2.0) * S1 + mu * s12) * (-GRAV) - sd * mu * (b + a * cd) * 2.0
    num2 = sd * ((mu + 1.0) * (a + C1 * GRAV) + b * mu * cd) * 2.0
    r1, r2 = num1 * il1 * rden, num2 * il2 * rden
    du = np.empty_like(u)
    du[:, 0], du[:, 1], du[:, 2], du[:, 3] = z[:, 2], z[:, 3], r1.v, r2.v
    dP = np.stack([Pz[:, 2], Pz[:, 3], r1.d, r2.d], axis=1)
    du[:, D:] = dP.reshape(n, D * NP)
    return du


def rhs_plain(z, th):
    """The right-hand side as include/lde.h states it, in (m₁, m₂), values only: z [n, 4], th [n, 4] → dz [n, 4]."""
    t1, t2, w1, w2 = (z[:, i] for i in range(4))
    L1, L2, m1, m2 = (th[:, i] for i in range(4))
    dl = t1 - t2
    den = 2 * m1 + m2 - m2 * np.cos(2 * dl)
    a1 = (-GRAV * (2 * m1 + m2) * np.sin(t1) - m2 * GRAV * np.sin(t1 - 2 * t2)
          - 2 * np.sin(dl) * m2 * (w2 * w2 * L2 + w1 * w1 * L1 * np.cos(dl))) / (L1 * den)
    a2 = (2 * np.sin(dl) * (w1 * w1 * L1 * (m1 + m2) + GRAV * (m1 + m2) * np.cos(t1) + w2 * w2 * L2 * m2 * np.cos(dl))) / (L2 * den)
    return np.stack([w1, w2, a1, a2], axis=1)


def energy(z, th):
    """½m₁L₁²ω₁² + ½m₂(L₁²ω₁² + L₂²ω₂² + 2L₁L₂ω₁ω₂ cosΔ) − (m₁+m₂)gL₁cos θ₁ − m₂gL₂cos θ₂ of z [..., 4] with th [n, 4] on the last batch axis."""
    t1, t2, w1, w2 = (z[..., i] for i in range(4))
    L1, L2, m1, m2 = (th[:, i] for i in range(4))
    return (0.5 * m1 * L1 ** 2 * w1 ** 2 + 0.5 * m2 * (L1 ** 2 * w1 ** 2 + L2 ** 2 * w2 ** 2 + 2 * L1 * L2 * w1 * w2 * np.cos(t1 - t2))
            - (m1 + m2) * GRAV * L1 * np.cos(t1) - m2 * GRAV * L2 * np.cos(t2))


SYSTEM = dual_ref.System(D, NP, rhs)


def solve(z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, 4], theta [B, 4] = (L₁, L₂, m₁, m₂), ts [T] → ẑ [T, B, 4], J [T, B, 4, 8] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(ẑ₀, θ)_q), ret [B], info:
    tests/dual_ref.py's solve on this system."""
    return dual_ref.solve(SYSTEM, z0, theta, ts, solver, adaptive, dt, steps, dtype, **opts)


def pullback(J, dz):
    """dz0 [B, 4], dθ [B, 4] from J [T, B, 4, 8] and the cotangent dz [T, B, 4] (f64)."""
    return dual_ref.pullback(SYSTEM, J, dz)


def inputs(B, seed=0):
    """θ₁, θ₂ ~ U(−1, 1), ω₁, ω₂ ~ U(−1, 1), L₁, L₂ ~ U(0.8, 1.6), m₁, m₂ ~ U(0.5, 2) as float32 arrays z0 [B, 4], theta [B, 4]. The ranges are on
    purpose: over t ≤ 2.45 the motion is regular (largest |J| ≈ 70); at |θ| ≤ 2 it is already chaotic (|J| 2e4, f32 1e-3 from f64) — an input
    that would test the number format, not the kernel."""
    rng = np.random.default_rng(seed)
    z0 = rng.uniform(-1.0, 1.0, (B, 4)).astype(np.float32)
    th = np.concatenate([rng.uniform(0.8, 1.6, (B, 2)), rng.uniform(0.5, 2.0, (B, 2))], axis=1).astype(np.float32)
    return z0, th


def turn_inputs(B):
    """The inputs of the tests of angles past 256 turns: seed 23 with TURNS whole turns added to θ₁ and θ₂ in f64, then rounded to f32 once."""
    z0, th = inputs(B, seed=23)
    z = z0.astype(np.float64)
    z[:, :2] += 2 * np.pi * TURNS
    return z.astype(np.float32), th


def cotangent(T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, D)) / (B * T)).astype(np.float32)


# the parity cases of tests/test_gpu_dpend.py (and of the f32-against-f64 floor in tests/test_dpend_host.py): one trajectory, a last workgroup
# of partial waves, several workgroups
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]

# The GPU tests' inputs and bounds (ẑ, J, dz0, dθ; each relative to the largest entry of the reference array). The bounds are the dual tests'
# (tests/test_gpu_lv.py) wherever this reference's own f32 mode stays within a quarter of them on the test's inputs; where it does not, the
# case's bound is 4 × that floor, rounded up. Every floor is measured and asserted on the CPU by tests/test_dpend_host.py — none comes from a
# kernel's output. The seeds were chosen there too (the smallest floor of a handful): the system is sensitive, and an input on which f32 is
# far from f64 would test the number format, not the kernel.
BOUNDS = (2e-5, 1e-4, 1e-4, 1e-4)
TSIT5_DT05_BOUNDS = (2.5e-5, 1.5e-4, 1e-4, 1e-4)      # Tsit5 at dt = 0.05 on (50, 256): floor 6.3e-6 / 3.6e-5 / 1.4e-5 / 1.9e-5
ADAPTIVE_BOUNDS = (3.5e-5, 1.6e-4, 1e-4, 1e-4)        # Tsit5 at 1e-6 / 1e-3 on (50, 37), the steps replayed: floor 8.5e-6 / 3.9e-5 / 9.1e-6 / 6.5e-6
TURN_BOUNDS = (2e-5, 1.4e-3, 1.1e-3, 8.5e-4)          # θ + 2π·300 on (5, 37): floor 7.1e-7 / 3.5e-4 / 2.7e-4 / 2.2e-4 (the format at |θ| ≈ 1 885)
PARITY_SEED = {1: 1, 2: 2, 50: 54}                    # by T, the seed of the fixed-step parity inputs
ADAPTIVE_SEED, RAGGED_SEED, LONG_SEED = 54, 18, 14


def bounds(solver, dt, T=50):
    return TSIT5_DT05_BOUNDS if (solver == TSIT5 and dt == 0.05 and T == 50) else BOUNDS
