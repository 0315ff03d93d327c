"""Restatement (numpy) of the double-pendulum solve on dual numbers (include/lde.h: "the double pendulum"; LDE_SENSE_FORWARD_DUAL):
z = (θ₁, θ₂, ω₁, ω₂), θ = (L₁, L₂, m₁, m₂), g = 10, carried as values and NP = 8 partials per component, ∂z/∂(ẑ₀ (4), L₁, L₂, m₁, m₂), through
Tsit5 with its free interpolant or RK4 with the cubic Hermite, with the step control of csrc/lde_dual_dir.hip on four components: the
dual-aware norm ‖u_i‖ = sqrt(v² + Σ_q p_q²) in the Hairer initial step, in the scale and in EEst, squares and ratios in the working precision,
the sum over the components and the root in f64, and the PI controller. The structure is tests/kuramoto_ref.py's; the tableau, the
controller's options, the interpolants and the three ways to choose the steps are tests/lv_ref.py's (imported where they do not depend on
the system). The partials' squares are summed in index order — the kernel sums them across lanes in a butterfly, which is one of the things
the GPU tests' tolerance is for. float64 by default; `dtype=np.float32` runs the same formulas in f32.

The right-hand side, as csrc/lde_dpend_dualrhs.h evaluates it: in the mass ratio μ = m₂/m₁ (the system is homogeneous of degree 0 in the
masses), Δ = θ₁ − θ₂, den = 2 + μ − μ cos 2Δ,
    ω₁' = [ −g(2 + μ) sin θ₁ − μ g sin(θ₁ − 2θ₂) − 2 sinΔ · μ (ω₂² L₂ + ω₁² L₁ cosΔ) ] / (L₁ · den)
    ω₂' = [ 2 sinΔ ( (1 + μ)(ω₁² L₁ + g cos θ₁) + ω₂² L₂ μ cosΔ ) ] / (L₂ · den)
with sin Δ, cos Δ, cos 2Δ and sin(θ₁ − 2θ₂) from the sines and cosines of θ₁ and θ₂ by the angle-sum identities, on numbers that carry
their eight partials (`Dual`). `rhs_plain` is the form of include/lde.h in the masses themselves, values only: what `rhs` is checked against.

Test infrastructure only, pinned on the CPU by tests/test_dpend_host.py (its J against central differences of its own values, the m₂ = 0
limit, the mass homogeneity, the energy drift under RK4)."""
import numpy as np

from tests.lv_ref import A, BT, R, R1, RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, _lincomb, _opts, grid, ragged_grid  # noqa: F401

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


def dual_abs(u):
    """‖u_i‖ [G, 4]: sqrt(v² + Σ_q p_q²), the squares added in index order."""
    out = []
    for i in range(D):
        s2 = u[:, i] * u[:, i]
        for q in range(NP):
            p = u[:, D + NP * i + q]
            s2 = s2 + p * p
        out.append(np.sqrt(s2))
    return np.stack(out, axis=1)


def dual_rms(e, sk):
    """RMS over the four components of ‖e_i‖ / sk_i: ratio and square in the working precision, sum and root in f64 → [G] float64."""
    r = dual_abs(e) / sk
    r2 = (r * r).astype(np.float64)
    s2 = np.zeros(r2.shape[0])
    for i in range(D):
        s2 = s2 + r2[:, i]
    return np.sqrt(s2 / float(D))


def init_dt(y, f0, th, dtmax, o, dtype):
    """Hairer–Nørsett–Wanner with every norm the dual norm (one trajectory) → float."""
    at, rt = dtype(o["abstol"]), dtype(o["reltol"])
    sk = at + dual_abs(y) * rt
    d0, d1 = float(dual_rms(y, sk)[0]), float(dual_rms(f0, sk)[0])
    dt0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    dt0 = min(dt0, dtmax)
    h = dtype(np.float32(dt0))
    f1 = rhs(y + h * f0, th) - f0
    d2 = float(dual_rms(f1, sk)[0]) / dt0
    dm = max(d1, d2)
    dt1 = max(1e-6, dt0 * 1e-3) if dm <= 1e-15 else 10.0 ** (-(2.0 + np.log10(dm)) / 5.0)
    return min(min(100.0 * dt0, dt1), dtmax)


def _group(y, th, ts, solver, adaptive, dt_fixed, steps, o, dtype):
    """One group of trajectories that share their step sequence (a fixed-step batch, or ONE trajectory under the controller / a replay).
    y [n, 4 + 4·8] start state; returns z [T, n, 4], J [T, n, 4, 8], retcode, statistics with the accepted steps."""
    n, T = y.shape[0], len(ts)
    z, J = np.empty((T, n, D), dtype), np.empty((T, n, D, NP), dtype)

    def f(u):
        return rhs(u, th)

    def save(j, u):
        z[j] = u[:, :D]
        J[j] = u[:, D:].reshape(n, D, NP)

    save(0, y)
    st = dict(nfe=0, naccept=0, nreject=0, t=[], dt=[])
    ret = RET_SUCCESS
    if T > 1:
        t, tend = float(ts[0]), float(ts[-1])
        dtmax = tend - t
        dtmin = o["dtmin"] if o["dtmin"] > 0 else 1e-12 * abs(tend - t)
        at, rt = dtype(o["abstol"]), dtype(o["reltol"])
        q_lo, q_hi, inv_gamma = dtype(1.0 / o["qmax"]), dtype(1.0 / o["qmin"]), dtype(1.0 / o["gamma"])
        b1, b2 = dtype(o["beta1"]), dtype(o["beta2"])
        k = [None] * 7
        k[0] = f(y)
        st["nfe"] = 1
        presc = steps is not None
        controlled = adaptive and not presc
        if presc:
            dt = 0.0
        elif not adaptive:
            dt = float(dt_fixed)
        elif dt_fixed and dt_fixed > 0:
            dt = min(float(dt_fixed), dtmax)
        else:
            dt = init_dt(y, k[0], th, dtmax, o, dtype)
            st["nfe"] += 1
        qold = dtype(1e-4)
        iters, j, ntr = 0, 1, 0
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            while t < tend:
                if iters >= o["maxiters"]:
                    ret = RET_MAXITERS
                    break
                iters += 1
                dtp, last = dt, False
                if presc:
                    if ntr >= len(steps[0]):
                        ret = RET_MAXITERS
                        break
                    t, dt, last = float(steps[0][ntr]), float(steps[1][ntr]), ntr == len(steps[0]) - 1
                elif t + dt >= tend - 1e-12 * abs(tend):
                    dt, last = tend - t, True
                h = dtype(np.float32(dt))          # the state advances by the f32 of the f64 step, whatever the arithmetic
                EEst = dtype(0)
                if solver == TSIT5:
                    for s in range(1, 6):
                        k[s] = f(y + h * _lincomb(A[s], k, dtype))
                    yn = y + h * _lincomb(A[6], k, dtype)
                    k[6] = f(yn)
                    st["nfe"] += 6
                    if adaptive:
                        e = _lincomb(BT, k, dtype) * h
                        sk = at + np.maximum(dual_abs(y), dual_abs(yn)) * rt
                        EEst = dtype(dual_rms(e, sk)[0])
                    FS = 6
                else:
                    hh, h6 = dtype(0.5) * h, h * dtype(1.0 / 6.0)
                    k[1] = f(y + hh * k[0])
                    k[2] = f(y + hh * k[1])
                    k[3] = f(y + h * k[2])
                    yn = y + h6 * (k[0] + dtype(2) * (k[1] + k[2]) + k[3])
                    k[4] = f(yn)
                    st["nfe"] += 4
                    FS = 4
                if not np.isfinite(yn).all() or not (EEst == EEst):
                    if controlled and dt > dtmin:
                        st["nreject"] += 1
                        dt = dt * float(dtype(o["qmin"]))
                        continue
                    ret = RET_NONFINITE
                    break
                if controlled:
                    if EEst == 0:
                        q11, q = dtype(0), q_lo
                    else:
                        q11 = EEst ** b1
                        q = max(q_lo, min(q_hi, q11 * qold ** (-b2) * inv_gamma))
                    if EEst > 1:
                        st["nreject"] += 1
                        dt = dt / float(min(q_hi, q11 * inv_gamma))
                        if dt < dtmin:
                            ret = RET_DTMIN
                            break
                        continue
                    qold = max(EEst, dtype(1e-4))
                    dtp = min(dt / float(q), dtmax)
                st["t"].append(t)
                st["dt"].append(dt)
                st["naccept"] += 1
                ntr += 1
                tnew = tend if last else (float(steps[0][ntr]) if presc else t + dt)
                while j < T and ts[j] <= tnew:
                    tj = float(ts[j])
                    if tj >= tnew or (j == T - 1 and last):
                        u = yn
                    else:
                        thd = (tj - t) / dt
                        if solver == TSIT5:       # u(t + Θh) = y + h Σ_i b_i(Θ) k_i: csrc/lde_device.h tsit5_interp_weights
                            th_ = dtype(thd)
                            bw = [th_ * (dtype(1) + th_ * (dtype(R1[0]) + th_ * (dtype(R1[1]) + th_ * dtype(R1[2]))))]
                            bw += [th_ * th_ * (dtype(R[i][0]) + th_ * (dtype(R[i][1]) + th_ * dtype(R[i][2]))) for i in range(6)]
                            acc = bw[0] * k[0]
                            for i in range(1, 7):
                                acc = acc + bw[i] * k[i]
                            u = y + h * acc
                        else:                     # cubic Hermite between (y, k₁) and (y_new, f(y_new)), coefficients formed in f64
                            om = 1.0 - thd
                            h00, h10 = dtype((1.0 + 2.0 * thd) * om * om), dtype(thd * om * om * dt)
                            h01, h11 = dtype(thd * thd * (3.0 - 2.0 * thd)), dtype(thd * thd * (thd - 1.0) * dt)
                            u = h00 * y + h10 * k[0] + h01 * yn + h11 * k[4]
                    save(j, u)
                    j += 1
                y = yn
                k[0] = k[FS]
                t = tnew
                dt = dtp if adaptive else float(dt_fixed)
    if ret != RET_SUCCESS:
        z[:], J[:] = np.nan, 0
    return z, J, ret, st


def solve(z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, 4], theta [B, 4] = (L₁, L₂, m₁, m₂), ts [T] → ẑ [T, B, 4], J [T, B, 4, 8] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(ẑ₀, θ)_q), ret [B], info
    (nfe, naccept, nreject summed; `t`, `dt`: per trajectory the accepted steps). `steps`: (t [B][n_b], dt [B][n_b]) — replay, no controller."""
    o = _opts(**opts)
    ts = np.asarray(ts, np.float64)
    z0 = np.asarray(z0, dtype)
    B = z0.shape[0]
    theta = np.asarray(theta, dtype).reshape(B, P)
    T = len(ts)
    y = np.zeros((B, D + D * NP), dtype)
    y[:, :D] = z0
    for i in range(D):
        y[:, D + NP * i + i] = 1
    z, J = np.empty((T, B, D), dtype), np.empty((T, B, D, NP), dtype)
    ret = np.zeros(B, np.int32)
    info = dict(nfe=0, naccept=0, nreject=0, t=[None] * B, dt=[None] * B)
    shared = steps is None and not adaptive
    groups = [slice(0, B)] if shared else [slice(b, b + 1) for b in range(B)]
    for g in groups:
        sg = None if steps is None else (steps[0][g.start], steps[1][g.start])
        zg, Jg, rg, st = _group(y[g], theta[g], ts, solver, adaptive, dt, sg, o, dtype)
        z[:, g], J[:, g], ret[g] = zg, Jg, rg
        n = g.stop - g.start
        for key in ("nfe", "naccept", "nreject"):
            info[key] += st[key] * n
        for b in range(g.start, g.stop):
            info["t"][b], info["dt"][b] = np.array(st["t"]), np.array(st["dt"])
    return z, J, ret, info


def pullback(J, dz):
    """dz0 [B, 4], dθ [B, 4] from J [T, B, 4, 8] and the cotangent dz [T, B, 4] (f64)."""
    g = np.einsum("tbiq,tbi->bq", np.asarray(J, np.float64), np.asarray(dz, np.float64))
    return g[:, :D], g[:, D:]


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
