"""Restatement (numpy) of THE dual-number solve (LDE_SENSE_FORWARD_DUAL: k_forward_dual, k_forward_dual_dir), over a system description:
a state of D components carried as values and NP partials per component, u = [z (D), ∂z_i/∂q row by row (D·NP)], through Tsit5 with its free
interpolant or RK4 with the cubic Hermite, with the step control of csrc/lde_dual.h — the dual-aware norm ‖u_i‖ = sqrt(v² + Σ_q p_q²) in the
Hairer initial step, in the scale and in EEst, squares and ratios in the working precision, the sum over the components and the root in
f64, and the PI controller. The partials' squares are summed in index order (the lane-per-direction kernel sums them across lanes in a
butterfly, which is one of the things the GPU tests' tolerance is for). The tableau is csrc/lde_device.h's (namespace ts5), digit for
digit. float64 by default; `dtype=np.float32` runs the same formulas in f32.

A system is `System(D, NP, rhs)`: `rhs(u [n, D + D·NP], th [n, P]) → du`; the seed is the identity in the first D directions (∂z(t₀)/∂ẑ₀ = I,
∂/∂θ = 0). tests/lv_ref.py, tests/kuramoto_ref.py and tests/dpend_ref.py hold the systems and thin `solve` / `pullback` wrappers.

Three ways to choose the steps: `adaptive=True` (the controller, per trajectory), `adaptive=False, dt=h` (fixed steps, the batch at once), and
`steps=[(t_n, dt_n) arrays per trajectory]` — the replay mode: the accepted steps of another solve (the kernel's "step_trace") are taken as
they are and no controller runs. Test infrastructure only; its bits are pinned by tests/test_dual_ref_bits.py."""
import collections

import numpy as np

TSIT5, RK4 = 0, 1
RET_SUCCESS, RET_MAXITERS, RET_DTMIN, RET_NONFINITE = 0, 1, 2, 3

System = collections.namedtuple("System", "D NP rhs")

# csrc/lde_device.h: namespace ts5
A = [[],
     [0.161],
     [-0.008480655492356989, 0.335480655492357],
     [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
     [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
     [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
     [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]]
BT = [-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552,
      -0.45808210592918697, 0.015151515151515152]
R1 = [-2.763706197274826, 2.9132554618219126, -1.0530884977290216]
R = [[0.13169999999999998, -0.2234, 0.1017],
     [3.9302962368947516, -5.941033872131505, 2.490627285651253],
     [-12.411077166933676, 30.33818863028232, -16.548102889244902],
     [37.50931341651104, -88.1789048947664, 47.37952196281928],
     [-27.896526289197286, 65.09189467479366, -34.87065786149661],
     [1.5, -4.0, 2.5]]


def dual_abs(sys, u):
    """‖u_i‖ [n, D]: sqrt(v² + Σ_q p_q²), the squares added in index order."""
    out = []
    for i in range(sys.D):
        s2 = u[:, i] * u[:, i]
        for q in range(sys.NP):
            p = u[:, sys.D + sys.NP * i + q]
            s2 = s2 + p * p
        out.append(np.sqrt(s2))
    return np.stack(out, axis=1)


def dual_rms(sys, e, sk):
    """RMS over the D components of ‖e_i‖ / sk_i: ratio and square in the working precision, sum and root in f64 → [n] float64."""
    r = dual_abs(sys, e) / sk
    r2 = (r * r).astype(np.float64)
    s2 = np.zeros(r2.shape[0])
    for i in range(sys.D):
        s2 = s2 + r2[:, i]
    return np.sqrt(s2 / float(sys.D))


def _lincomb(coef, k, dtype):
    acc = dtype(coef[0]) * k[0]
    for j in range(1, len(coef)):
        acc = acc + dtype(coef[j]) * k[j]
    return acc


def _opts(**kw):
    o = dict(abstol=1e-6, reltol=1e-3, qmin=0.2, qmax=10.0, gamma=0.9, beta1=7.0 / 50.0, beta2=2.0 / 25.0, dtmin=0.0, maxiters=100000)
    o.update(kw)
    return o


def init_dt(sys, y, f0, th, dtmax, o, dtype):
    """Hairer–Nørsett–Wanner with every norm the dual norm (one trajectory) → float."""
    at, rt = dtype(o["abstol"]), dtype(o["reltol"])
    sk = at + dual_abs(sys, y) * rt
    d0, d1 = float(dual_rms(sys, y, sk)[0]), float(dual_rms(sys, f0, sk)[0])
    dt0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    dt0 = min(dt0, dtmax)
    h = dtype(np.float32(dt0))
    f1 = sys.rhs(y + h * f0, th) - f0
    d2 = float(dual_rms(sys, f1, sk)[0]) / dt0
    dm = max(d1, d2)
    dt1 = max(1e-6, dt0 * 1e-3) if dm <= 1e-15 else 10.0 ** (-(2.0 + np.log10(dm)) / 5.0)
    return min(min(100.0 * dt0, dt1), dtmax)


def _group(sys, y, th, ts, solver, adaptive, dt_fixed, steps, o, dtype):
    """One group of trajectories that share their step sequence (a fixed-step batch, or ONE trajectory under the controller / a replay).
    y [n, D + D·NP] start state; returns z [T, n, D], J [T, n, D, NP], retcode, statistics with the accepted steps."""
    D, NP = sys.D, sys.NP
    n, T = y.shape[0], len(ts)
    z, J = np.empty((T, n, D), dtype), np.empty((T, n, D, NP), dtype)

    def f(u):
        return sys.rhs(u, th)

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
            dt = init_dt(sys, y, k[0], th, dtmax, o, dtype)
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
                elif t + dt >= tend - 1e-12 * max(abs(tend), dtmax):
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
                        sk = at + np.maximum(dual_abs(sys, y), dual_abs(sys, yn)) * rt
                        EEst = dtype(dual_rms(sys, e, sk)[0])
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


def solve(sys, z0, theta, ts, solver=TSIT5, adaptive=True, dt=0.0, steps=None, dtype=np.float64, **opts):
    """z0 [B, D], theta [B, P], ts [T] → ẑ [T, B, D], J [T, B, D, NP] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(ẑ₀, θ)_q), ret [B], info (nfe, naccept, nreject
    summed; `t`, `dt`: per trajectory the accepted steps). `steps`: (t [B][n_b], dt [B][n_b]) — replay, no controller."""
    D, NP = sys.D, sys.NP
    o = _opts(**opts)
    ts = np.asarray(ts, np.float64)
    z0 = np.asarray(z0, dtype)
    B, T = z0.shape[0], len(ts)
    theta = np.asarray(theta, dtype).reshape(B, -1)
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
        zg, Jg, rg, st = _group(sys, y[g], theta[g], ts, solver, adaptive, dt, sg, o, dtype)
        z[:, g], J[:, g], ret[g] = zg, Jg, rg
        n = g.stop - g.start
        for key in ("nfe", "naccept", "nreject"):
            info[key] += st[key] * n
        for b in range(g.start, g.stop):
            info["t"][b], info["dt"][b] = np.array(st["t"]), np.array(st["dt"])
    return z, J, ret, info


def pullback(sys, J, dz):
    """dz0 [B, D], dθ [B, NP − D] from J [T, B, D, NP] and the cotangent dz [T, B, D] (f64)."""
    g = np.einsum("tbiq,tbi->bq", np.asarray(J, np.float64), np.asarray(dz, np.float64))
    return g[:, :sys.D], g[:, sys.D:]


def grid(T):
    return 0.05 * np.arange(T)


def ragged_grid():
    """Nine save times: several inside one step of the default tolerances, and gaps that several steps cross without a save."""
    return np.array([0.0, 0.01, 0.02, 0.025, 0.9, 0.91, 0.915, 2.2, 2.45])
