"""Restatement (numpy) of the Kuramoto solve on dual numbers (include/lde.h: "the Kuramoto system"; LDE_SENSE_FORWARD_DUAL): N phase
oscillators dφ_i = ω_i + (K/N) Σ_j sin(φ_j − φ_i) carried as values and NP = 2N + 1 partials per component, ∂φ/∂(φ₀ (N), ω (N), K), through
Tsit5 with its free interpolant or RK4 with the cubic Hermite, with the step control of csrc/lde_dual_dir.hip — csrc/lde_dual.h's from 2 to N
components: the dual-aware norm ‖u_i‖ = sqrt(v² + Σ_q p_q²) in the Hairer initial step, in the scale and in EEst, squares and ratios in the
working precision, the sum over the N components and the root in f64, and the PI controller. The structure, the tableau, the controller, the
interpolants and the three ways to choose the steps are tests/lv_ref.py's (imported where they do not depend on the system); what differs
is the N-component norms and the right-hand side. The partials' squares are summed in index order — the kernel sums them across lanes in a
butterfly, which is one of the things the GPU tests' tolerance is for. float64 by default; `dtype=np.float32` runs the same formulas in f32.

The right-hand side in mean-field form: s = sin φ, c = cos φ, S = Σ s, C = Σ c, f_i = ω_i + (K/N)(c_i S − s_i C); ∂f_i/∂φ_j = (K/N)(c_i c_j +
s_i s_j) for j ≠ i, ∂f_i/∂φ_i = −(K/N)(c_i C + s_i S − 1), ∂f_i/∂ω_j = δ_ij, ∂f_i/∂K = (c_i S − s_i C)/N.

Test infrastructure only, pinned on the CPU by tests/test_kuramoto_host.py (its J against central differences of its own values, the
uncoupled closed form, the conserved phase sum, the two-oscillator closed form)."""
import numpy as np

from tests.lv_ref import A, BT, R, R1, RET_DTMIN, RET_MAXITERS, RET_NONFINITE, RET_SUCCESS, RK4, TSIT5, _lincomb, _opts, grid, ragged_grid  # noqa: F401


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


def dual_abs(u, N):
    """‖u_i‖ [G, N]: sqrt(v² + Σ_q p_q²), the squares added in index order."""
    NP = n_partials(N)
    out = []
    for i in range(N):
        s2 = u[:, i] * u[:, i]
        for q in range(NP):
            p = u[:, N + NP * i + q]
            s2 = s2 + p * p
        out.append(np.sqrt(s2))
    return np.stack(out, axis=1)


def dual_rms(e, sk, N):
    """RMS over the N components of ‖e_i‖ / sk_i: ratio and square in the working precision, sum and root in f64 → [G] float64."""
    r = dual_abs(e, N) / sk
    r2 = (r * r).astype(np.float64)
    s2 = np.zeros(r2.shape[0])
    for i in range(N):
        s2 = s2 + r2[:, i]
    return np.sqrt(s2 / float(N))


def init_dt(y, f0, th, N, dtmax, o, dtype):
    """Hairer–Nørsett–Wanner with every norm the dual norm (one trajectory: G = 1) → float."""
    at, rt = dtype(o["abstol"]), dtype(o["reltol"])
    sk = at + dual_abs(y, N) * rt
    d0, d1 = float(dual_rms(y, sk, N)[0]), float(dual_rms(f0, sk, N)[0])
    dt0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    dt0 = min(dt0, dtmax)
    h = dtype(np.float32(dt0))
    f1 = rhs(y + h * f0, th, N) - f0
    d2 = float(dual_rms(f1, sk, N)[0]) / dt0
    dm = max(d1, d2)
    dt1 = max(1e-6, dt0 * 1e-3) if dm <= 1e-15 else 10.0 ** (-(2.0 + np.log10(dm)) / 5.0)
    return min(min(100.0 * dt0, dt1), dtmax)


def _group(y, th, N, ts, solver, adaptive, dt_fixed, steps, o, dtype):
    """One group of trajectories that share their step sequence (a fixed-step batch, or ONE trajectory under the controller / a replay).
    y [G, N + N·NP] start state; returns z [T, G, N], J [T, G, N, NP], retcode, statistics with the accepted steps."""
    NP = n_partials(N)
    G, T = y.shape[0], len(ts)
    z, J = np.empty((T, G, N), dtype), np.empty((T, G, N, NP), dtype)

    def f(u):
        return rhs(u, th, N)

    def save(j, u):
        z[j] = u[:, :N]
        J[j] = u[:, N:].reshape(G, N, NP)

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
            dt = init_dt(y, k[0], th, N, dtmax, o, dtype)
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
                        sk = at + np.maximum(dual_abs(y, N), dual_abs(yn, N)) * rt
                        EEst = dtype(dual_rms(e, sk, N)[0])
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
    """z0 [B, N], theta [B, N + 1] = (ω₁ … ω_N, K), ts [T] → ẑ [T, B, N], J [T, B, N, 2N + 1] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(φ₀, ω, K)_q), ret [B],
    info (nfe, naccept, nreject summed; `t`, `dt`: per trajectory the accepted steps). `steps`: (t [B][n_b], dt [B][n_b]) — replay, no
    controller."""
    o = _opts(**opts)
    ts = np.asarray(ts, np.float64)
    z0 = np.asarray(z0, dtype)
    B, N = z0.shape
    NP = n_partials(N)
    theta = np.asarray(theta, dtype).reshape(B, N + 1)
    T = len(ts)
    y = np.zeros((B, N + N * NP), dtype)
    y[:, :N] = z0
    for i in range(N):
        y[:, N + NP * i + i] = 1
    z, J = np.empty((T, B, N), dtype), np.empty((T, B, N, NP), dtype)
    ret = np.zeros(B, np.int32)
    info = dict(nfe=0, naccept=0, nreject=0, t=[None] * B, dt=[None] * B)
    shared = steps is None and not adaptive
    groups = [slice(0, B)] if shared else [slice(b, b + 1) for b in range(B)]
    for g in groups:
        sg = None if steps is None else (steps[0][g.start], steps[1][g.start])
        zg, Jg, rg, st = _group(y[g], theta[g], N, ts, solver, adaptive, dt, sg, o, dtype)
        z[:, g], J[:, g], ret[g] = zg, Jg, rg
        n = g.stop - g.start
        for key in ("nfe", "naccept", "nreject"):
            info[key] += st[key] * n
        for b in range(g.start, g.stop):
            info["t"][b], info["dt"][b] = np.array(st["t"]), np.array(st["dt"])
    return z, J, ret, info


def pullback(J, dz):
    """dz0 [B, N], dθ [B, N + 1] from J [T, B, N, 2N + 1] and the cotangent dz [T, B, N] (f64)."""
    N = J.shape[2]
    g = np.einsum("tbiq,tbi->bq", np.asarray(J, np.float64), np.asarray(dz, np.float64))
    return g[:, :N], g[:, N:]


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
