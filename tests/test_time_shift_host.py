"""CPU: the time-translation known answer on the checkers themselves (tests/time_shift.py; the kernels: tests/test_gpu_time_shift.py).

Every right-hand side here is autonomous, so a solve on `ts + c` is the solve on `ts`. On the dyadic grids of `shifted_grids` (base =
(0 … 32)/16; c = ±1024, +2²⁰, −base[−1], −base[16]) with dt ∈ {1/32, 3/64} every time the stepping loops form is exact, and the f32 and f64
oracle, tests/dual_ref.py on every system module and the stochastic schemes of tests/sde_ref.py / tests/sl_ref.py must return the SAME BITS
on every grid (Part A). Part C is the grid 0.05·j − 2.45, which ends at 0 and is not dyadic: the end-of-solve guard
`t + dt ≥ tend − 1e-12·max(|tend|, |tend − t₀|)` is scaled by the span as dtmin is, so a grid that ends at 0 keeps it — with the guard scaled
by |tend| alone it vanished there and every trajectory took one more step of ≈ 1e-16 (measured on the oracle before the rule changed, f32
and f64, B = 37: 37 more accepted steps than on 0.05·j for Tsit5 at the fixed step 0.05).

Part B's yardstick — the oracle's own deviation under the shifts at Tsit5 adaptive, B = 37, T = 33, as fractions of each array's largest
entry — is printed by test_oracle_adaptive_deviation_under_the_shifts; measured (f32 oracle, both right-hand sides, both tolerances): ẑ ≤ 1.4e-7,
the discrete sweep's gradients ≤ 3.1e-6 (dz0 2.8e-6, dθ 3.1e-6: the frictionless pendulum at 1e-6/1e-3), the continuous adjoints' ≤ 8.5e-7, the
dual solve's ẑ, J and gradients ≤ 1.4e-7; the accepted steps of the forward, dual and time-parallel adjoint solves unchanged under every shift.
The MLP right-hand sides' yardstick (test_oracle_mlp_deviation_under_the_shifts): ẑ ≤ 7.8e-8, gradients ≤ 4.4e-7."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sde_ref, sl_ref
from tests import dual_ref
from tests import time_shift as TS

B = 37
KINDS = [O.RHS_PENDULUM, O.RHS_PENDULUM_FRICTION]
FIXED = [(O.SOLVER_RK4, dt) for dt in TS.DTS] + [(O.SOLVER_TSIT5, dt) for dt in TS.DTS]


def _oracle_all(orc, kind, kw, ts, c, B=B):
    """Everything the oracle returns for one solve configuration: the forward solve with its statistics and accepted dt's, the three
    continuous adjoints, the recorded steps (start times with c taken off) and the discrete sweep on them, the dual solve."""
    z0, L = O.pendulum_inputs(B, seed=3)
    dz = O.cotangent(len(ts), B, 2)
    out = {}
    z, ret, info = orc.forward(O.make_desc(rhs_kind=kind, **kw), z0, L, ts)
    out.update(z=z, ret=ret, stats=np.array([info[k] for k in ("nfe", "naccept", "nreject", "nfailed", "max_steps")]), dt_trace=info["dt_trace"])
    for sense in (O.SENSE_BACKSOLVE_CHECKPOINTED, O.SENSE_BACKSOLVE, O.SENSE_PARALLEL_CHECKPOINTED):
        g0, gL, _, ai = orc.adjoint(O.make_desc(rhs_kind=kind, sensealg=sense, **kw), z, L, ts, dz)
        out[f"adj{sense}_dz0"], out[f"adj{sense}_dtheta"] = g0, gL
        out[f"adj{sense}_stats"] = np.array([ai[k] for k in ("nfe", "naccept", "nreject", "nfailed")])
    dd = O.make_desc(rhs_kind=kind, sensealg=O.SENSE_DISCRETE, **kw)
    zs, rets, rec, _ = orc.forward_steps(dd, z0, L, ts)
    out["rec_t"], out["rec_dt"] = TS.masked_steps(rec["t"], rec["dt"], rec["n"], c)
    out.update(steps_z=zs, steps_ret=rets, rec_n=rec["n"])
    out["disc_dz0"], out["disc_dtheta"], _, _ = orc.adjoint_discrete(dd, zs, L, ts, dz, rec)
    zd, J, (q0, qL), retd, recd, di = orc.forward_dual(O.make_desc(rhs_kind=kind, sensealg=4, **kw), z0, L, ts, dz_out=dz, dual_norm=True)
    out["dual_t"], out["dual_dt"] = TS.masked_steps(recd["t"], recd["dt"], recd["n"], c)
    out.update(dual_z=zd, dual_J=J, dual_dz0=q0, dual_dtheta=qL, dual_ret=retd, dual_n=recd["n"], dual_stats=np.array([di["nfe"], di["naccept"], di["nreject"]]))
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_fixed_step_solves_keep_their_bits_under_a_time_shift(prec, kind):
    orc = O.Oracle(prec)
    base, shifts = TS.grids()
    for solver, dt in FIXED:
        kw = dict(solver=solver, adaptive=False, dt=dt)
        ref = _oracle_all(orc, kind, kw, base, 0.0)
        assert (ref["ret"] == 0).all() and np.isfinite(ref["z"]).all()
        for name, ts, c in shifts[:-1]:
            TS.same(f"{prec} kind {kind} solver {solver} dt {dt} {name}", _oracle_all(orc, kind, kw, ts, c), ref)


def _dual_ref_all(sys, z0, th, dz, ts, c, **kw):
    z, J, ret, info = dual_ref.solve(sys, z0, th, ts, **kw)
    g0, gth = dual_ref.pullback(sys, J, dz)
    t = np.stack([np.asarray(a) - c for a in info["t"]])
    return dict(z=z, J=J, ret=ret, dz0=g0, dtheta=gth, stats=np.array([info["nfe"], info["naccept"], info["nreject"]]), t=t, dt=np.stack(info["dt"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(TS.dual_systems()))
def test_dual_ref_fixed_step_solves_keep_their_bits_under_a_time_shift(name, dtype):
    s = TS.dual_systems()[name]
    z0, th = s["inputs"](B)
    dz = TS.dual_cotangent(s["sys"].D, TS.T, B)
    base, shifts = TS.grids()
    for solver in (dual_ref.RK4, dual_ref.TSIT5):
        for dt in TS.DTS:
            kw = dict(solver=solver, adaptive=False, dt=dt, dtype=dtype)
            ref = _dual_ref_all(s["sys"], z0, th, dz, base, 0.0, **kw)
            assert (ref["ret"] == 0).all() and np.isfinite(ref["J"]).all()
            for sname, ts, c in shifts[:-1]:
                TS.same(f"{name} solver {solver} dt {dt} {sname}", _dual_ref_all(s["sys"], z0, th, dz, ts, c, **kw), ref)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("solver", [sde_ref.EM, sde_ref.EULER_HEUN])
def test_stochastic_references_keep_their_path_under_a_time_shift(solver, dtype):
    """The noise is indexed by substep, not by time: the same seed gives the same path. dt = 0.05 splits an interval of 1/16 into two
    substeps of 1/32 (the substep rule divides the interval evenly)."""
    base, shifts = TS.grids()
    z0, L = sde_ref.inputs(B, seed=3)
    runs = [("spendulum", lambda ts, dt: sde_ref.solve(z0, L, ts, dt, solver, seed=5, dtype=dtype))]
    for N in (1, 3):
        y0, th = sl_ref.inputs(N, B, seed=3)
        runs.append((f"sl{N}", lambda ts, dt, N=N, y0=y0, th=th: sl_ref.sde_solve(N, y0, th, ts, dt, solver, seed=5, dtype=dtype)))
    for tag, run in runs:
        for dt in TS.DTS + (0.05,):
            assert sde_ref.plan(base, dt) == [(2, 1.0 / 32.0)] * (TS.T - 1)
            z, J, ret = run(base, dt)
            assert (ret == 0).all() and np.isfinite(J).all()
            for name, ts, _ in shifts[:-1]:
                zs, Js, rets = run(ts, dt)
                TS.same(f"{tag} solver {solver} dt {dt} {name}", dict(z=zs, J=Js, ret=rets), dict(z=z, J=J, ret=ret))


# ---- Part C: 0.05·j − 2.45 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("solve", sorted(TS.PART_C_SOLVES))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_on_a_grid_that_ends_at_zero(prec, kind, solve):
    """Per trajectory the accepted steps of 0.05·j − 2.45 are those of 0.05·j (no step of 1e-16 at the end), with the same step sizes up to
    the round-off of the times; ẑ and every gradient agree to the bar of tests/test_oracle_kat.py's `ts + 3.0` assertion (1e-5; gradients:
    1e-5 of the largest entry)."""
    orc = O.Oracle(prec)
    t0, tz = TS.part_c_grids()
    assert tz[-1] == 0.0
    kw = TS.PART_C_SOLVES[solve]
    a, b = _oracle_all(orc, kind, kw, t0, 0.0), _oracle_all(orc, kind, kw, tz, 0.0)
    assert (b["ret"] == 0).all() and (b["dual_ret"] == 0).all() and all(np.isfinite(v).all() for v in b.values())
    assert np.array_equal(b["rec_n"], a["rec_n"]) and np.array_equal(b["dual_n"], a["dual_n"]), (b["rec_n"] - a["rec_n"], b["dual_n"] - a["dual_n"])
    assert b["stats"][1] == a["stats"][1] and np.array_equal(b["stats"], a["stats"])
    for s in (0, 1, 2):
        assert np.array_equal(b[f"adj{s}_stats"], a[f"adj{s}_stats"]), s
    assert b["rec_dt"][b["rec_dt"] > 0].min() > 1e-9, "no step of round-off size"
    assert np.abs(b["rec_dt"] - a["rec_dt"]).max() <= 1e-14
    for k in ("z", "steps_z", "dual_z"):
        assert np.abs(b[k] - a[k]).max() <= 1e-5, k
    for k in [k_ for k_ in a if k_.endswith(("dz0", "dtheta", "_J"))]:
        assert np.abs(b[k] - a[k]).max() <= 1e-5 * np.abs(a[k]).max(), k


@pytest.mark.parametrize("name", sorted(TS.dual_systems()))
def test_dual_ref_on_a_grid_that_ends_at_zero(name):
    """The numpy dual solve, every system: the same accepted steps per trajectory on both grids (five trajectories under the controller —
    the step sequence is per trajectory, so a smaller batch checks the same thing), f32 and f64."""
    s = TS.dual_systems()[name]
    nb = 5
    z0, th = s["inputs"](nb)
    t0, tz = TS.part_c_grids()
    for dtype in (np.float32, np.float64):
        for solve, kw in TS.PART_C_SOLVES.items():
            kw = dict(solver=kw["solver"], adaptive=bool(kw.get("adaptive", 1)), dt=kw.get("dt", 0.0), dtype=dtype)
            za, Ja, ra, ia = dual_ref.solve(s["sys"], z0, th, t0, **kw)
            zb, Jb, rb, ib = dual_ref.solve(s["sys"], z0, th, tz, **kw)
            assert (ra == 0).all() and (rb == 0).all() and np.isfinite(Jb).all()
            assert [len(x) for x in ib["dt"]] == [len(x) for x in ia["dt"]], (name, solve)
            assert min(x.min() for x in ib["dt"]) > 1e-9
            assert ib["nfe"] == ia["nfe"] and ib["nreject"] == ia["nreject"]
            tol = 2e-5 if dtype == np.float32 else 1e-9
            assert np.abs(zb - za).max() <= tol * max(1.0, np.abs(za).max()), (name, solve, np.abs(zb - za).max())


# ---- Part B's yardstick ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_adaptive_deviation_under_the_shifts(kind, tol):
    """The controller never sees t: under a shift only the last step's h = (real)(tend − t) and the dense-output Θ can move, by an ulp. The
    f32 oracle's deviations (printed: the numbers the GPU tests' sharp gate multiplies by 8) stay at round-off — far below the parity gates
    of the solve (1e-5 for ẑ at the tight tolerance, 1e-4 of the largest entry for a gradient) — the accepted steps of the forward, dual and
    time-parallel adjoint solves do not change (those of the sequential reverse-time adjoints may: tests/time_shift.py), and the f64 oracle
    moves by the round-off of its times at 2²⁰ with every count unchanged."""
    dev, mag, changed = TS.oracle_shift_deviation("f32", kind, tol, B)
    print(f"f32 oracle, kind {kind}, tol {tol}: " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert changed <= {"adj0", "adj1"}, f"a time shift changed the accepted steps of {sorted(changed)}"
    assert max(dev.values()) <= 1e-5 and dev["z"] * mag["z"] <= 1e-5, dev
    dev64, _, changed64 = TS.oracle_shift_deviation("f64", kind, tol, B)
    # f64: with an adaptive (not dyadic) dt the sums t + dt round at 2²⁰ to 2.3e-10 each; ≲ 50 steps put the step ends — and with them the
    # last h and every Θ·h — off by ≤ 1.2e-8, and the state moves by |ż|·δt with |ż| ≤ G/L·1 + |ω| ≲ 12: 1.5e-7, of a largest entry ≳ 1
    assert not changed64 and max(dev64.values()) <= 1.5e-7, (changed64, dev64)


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("case", sorted(TS.MLP_CASES))
def test_oracle_mlp_deviation_under_the_shifts(case, tol):
    """Part B's yardstick for the MLP right-hand sides (tanh units; tests/time_shift.py: mlp_adaptive_case): the f32 oracle's forward solve
    keeps its accepted steps under every shift, and ẑ, the discrete sweep's and the continuous adjoint's dz0 and dW move by round-off —
    far below the solves' parity gates (1e-4 for ẑ, 1e-4 / 2e-3 of the largest entry for the gradients)."""
    dev, unchanged = TS.oracle_mlp_shift_deviation(case, tol)
    print(f"f32 oracle, {case}, tol {tol}: " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert unchanged and max(dev.values()) <= 1e-5, dev


@pytest.mark.parametrize("name", sorted(TS.dual_systems()))
def test_part_c_dual_bounds_stand_on_the_f32_floor(name):
    """The GPU tests' Part C bounds for the dual systems are constants (tests/time_shift.py: part_c_dual_bounds). Each is the standing bound,
    or — the double pendulum — 4 × the measured floor rounded up: here the numpy reference's own f32 mode against its f64 mode, on the same
    inputs, grid and solves, stays within a quarter of every one of them (and a widened bound is not wider than 2 × the standing one)."""
    bounds = TS.part_c_dual_bounds(name)
    assert all(b <= 2 * s for b, s in zip(bounds, TS.DUAL_STANDING_BOUNDS))
    for solve in TS.PART_C_SOLVES:
        floor = TS.part_c_dual_floor(name, solve)
        print(f"{name} {solve}: f32 floor " + " ".join(f"{x:.1e}" for x in floor))
        assert all(4 * f <= b for f, b in zip(floor, bounds)), (solve, floor, bounds)
