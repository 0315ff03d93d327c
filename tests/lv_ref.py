"""Restatement (numpy) of the Lotka–Volterra solve on dual numbers (include/lde.h: "the Lotka–Volterra system"; LDE_SENSE_FORWARD_DUAL):
dx = αx − βxy, dy = −γy + δxy carried as values and NP = 6 partials per component, ∂(x, y)/∂(x₀, y₀, α, β, γ, δ), through Tsit5 with its free
interpolant or RK4 with the cubic Hermite, with the step control of csrc/lde_dual.h — the dual-aware norm ‖u_i‖ = sqrt(v² + Σ_q p_q²) in the
Hairer initial step, in the scale and in EEst, squares and ratios in the working precision, sum and root in f64, and the PI controller. The
tableau is csrc/lde_device.h's (namespace ts5), digit for digit. float64 by default; `dtype=np.float32` runs the same formulas in f32.

Three ways to choose the steps: `adaptive=True` (the controller, per trajectory), `adaptive=False, dt=h` (fixed steps, the batch at once), and
`steps=[(t_n, dt_n) arrays per trajectory]` — the replay mode: the accepted steps of another solve (the kernel's "step_trace") are taken as
they are and no controller runs. Test infrastructure only, pinned on the CPU by tests/test_lv_host.py (its J against central differences of
its own values, the closed form at β = δ = 0, the conserved quantity)."""
import numpy as np

TSIT5, RK4 = 0, 1
NP, DN = 6, 14          # partials per component; floats of a dual state [x, y, ∂x/∂q (6), ∂y/∂q (6)]
RET_SUCCESS, RET_MAXITERS, RET_DTMIN, RET_NONFINITE = 0, 1, 2, 3

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


def dual_abs(u):
    """‖u_i‖ [G, 2]: sqrt(v² + Σ_q p_q²), the squares added in order."""
    out = []
    for i in range(2):
        s2 = u[:, i] * u[:, i]
        for q in range(NP):
            p = u[:, 2 + NP * i + q]
            s2 = s2 + p * p
        out.append(np.sqrt(s2))
    return np.stack(out, axis=1)


def dual_rms(e, sk):
    """RMS over the two components of ‖e_i‖ / sk_i: ratio and square in the working precision, sum and root in f64 → [G] float64."""
    r = dual_abs(e) / sk
    r2 = (r * r).astype(np.float64)
    return np.sqrt((r2[:, 0] + r2[:, 1]) / 2.0)


def _lincomb(coef, k, dtype):
    acc = dtype(coef[0]) * k[0]
    for j in range(1, len(coef)):
        acc = acc + dtype(coef[j]) * k[j]
    return acc


def _opts(**kw):
    o = dict(abstol=1e-6, reltol=1e-3, qmin=0.2, qmax=10.0, gamma=0.9, beta1=7.0 / 50.0, beta2=2.0 / 25.0, dtmin=0.0, maxiters=100000)
    o.update(kw)
    return o


def init_dt(y, f0, th, dtmax, o, dtype):
    """Hairer–Nørsett–Wanner with every norm the dual norm (one trajectory: G = 1) → float."""
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
    y [G, 14] start state; returns z [T, G, 2], J [T, G, 2, 6], retcode, statistics, the accepted steps."""
    G, T = y.shape[0], len(ts)
    z, J = np.empty((T, G, 2), dtype), np.empty((T, G, 2, NP), dtype)

    def save(j, u):
        z[j] = u[:, 0:2]
        J[j] = u[:, 2:].reshape(G, 2, NP)

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
        k[0] = rhs(y, th)
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
                        k[s] = rhs(y + h * _lincomb(A[s], k, dtype), th)
                    yn = y + h * _lincomb(A[6], k, dtype)
                    k[6] = rhs(yn, th)
                    st["nfe"] += 6
                    if adaptive:
                        e = _lincomb(BT, k, dtype) * h
                        sk = at + np.maximum(dual_abs(y), dual_abs(yn)) * rt
                        EEst = dtype(dual_rms(e, sk)[0])
                    FS = 6
                else:
                    hh, h6 = dtype(0.5) * h, h * dtype(1.0 / 6.0)
                    k[1] = rhs(y + hh * k[0], th)
                    k[2] = rhs(y + hh * k[1], th)
                    k[3] = rhs(y + h * k[2], th)
                    yn = y + h6 * (k[0] + dtype(2) * (k[1] + k[2]) + k[3])
                    k[4] = rhs(yn, th)
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
    """z0 [B, 2], theta [B, 4] = (α, β, γ, δ), ts [T] → ẑ [T, B, 2], J [T, B, 2, 6] (J[j, b, i, q] = ∂ẑ_i(t_j)/∂(x₀, y₀, α, β, γ, δ)_q), ret [B], info
    (nfe, naccept, nreject summed; `t`, `dt`: per trajectory the accepted steps). `steps`: (t [B][n_b], dt [B][n_b]) — replay, no controller."""
    o = _opts(**opts)
    ts = np.asarray(ts, np.float64)
    z0, theta = np.asarray(z0, dtype), np.asarray(theta, dtype).reshape(-1, 4)
    B, T = z0.shape[0], len(ts)
    y = np.zeros((B, DN), dtype)
    y[:, 0:2] = z0
    y[:, 2] = 1
    y[:, 2 + NP + 1] = 1
    z, J = np.empty((T, B, 2), dtype), np.empty((T, B, 2, NP), dtype)
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
    """dz0 [B, 2], dθ [B, 4] from J [T, B, 2, 6] and the cotangent dz [T, B, 2] (f64)."""
    g = np.einsum("tbiq,tbi->bq", np.asarray(J, np.float64), np.asarray(dz, np.float64))
    return g[:, 0:2], g[:, 2:6]


def inputs(B, seed=0):
    """x₀, y₀ ~ U(0.5, 2), α, β, γ, δ ~ U(0.5, 1.5) as float32 arrays z0 [B, 2], theta [B, 4]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, (B, 2)).astype(np.float32), rng.uniform(0.5, 1.5, (B, 4)).astype(np.float32)


def cotangent(T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, 2)) / (B * T)).astype(np.float32)


def grid(T):
    return 0.05 * np.arange(T)


def ragged_grid():
    """Nine save times: several inside one step of the default tolerances, and gaps that several steps cross without a save."""
    return np.array([0.0, 0.01, 0.02, 0.025, 0.9, 0.91, 0.915, 2.2, 2.45])


def invariant(z, theta):
    """V = δx − γ ln x + βy − α ln y along ẑ [T, B, 2]."""
    al, be, ga, de = (np.asarray(theta, np.float64)[:, i] for i in range(4))
    x, y = z[..., 0].astype(np.float64), z[..., 1].astype(np.float64)
    return de * x - ga * np.log(x) + be * y - al * np.log(y)


# the parity cases of tests/test_gpu_lv.py (and of the f32-against-f64 floor in tests/test_lv_host.py)
SHAPES = [(1, 1), (2, 37), (50, 256)]
DTS = [0.05, 0.0125]
