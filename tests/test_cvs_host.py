"""CPU: the cardiovascular system (LDE_RHS_CVS, include/lde.h) without a GPU — (1) which descriptions the built library serves and which it
refuses, with what status and text, including that rhs_kind = 6, 8, 10 and 12 are unknown; (2) the numpy restatement the GPU tests compare
against (tests/cvs_ref.py) pinned before it is trusted: its right-hand side against the form of include/lde.h, its J against central
differences of its own values, the exact fourth row, the blood volume and its tangent, RK4's order, the saturated baroreflex, and its f32
mode against its f64 mode on every GPU case's own inputs (the floor under the GPU bounds); (3) the Python plug-in: its fields and the head
widths default_layers builds from it; (4) csrc/lde_host.h's part under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/cvs_host_driver.cpp, run as a program).

Every test here that creates a description of rhs_kind = 11 (or asks for la.CVS) fails before this right-hand side existed, where lde_create
returns LDE_ERR_INVALID_ARG ("unknown rhs_kind")."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cvs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    base = dict(rhs_kind=L.RHS_CVS, state_dim=4, param_dim=2, sensealg=L.SENSE_FORWARD_DUAL)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return lib, d


def test_served_and_refused_descriptions_through_the_c_abi():
    from latentdiffeq_amd import _lib as L
    assert L.RHS_CVS == 11 and L.RHS_DOUBLE_PENDULUM == 9 and L.RHS_KURAMOTO == 7 and L.RHS_LOTKA_VOLTERRA == 5
    assert L.load().lde_abi_version() == 1                 # lde_problem_desc did not change
    for kw in (dict(), dict(adaptive=0, dt=0.05), dict(solver=L.SOLVER_RK4, adaptive=0, dt=0.0125), dict(dt=0.01)):
        lib, d = _desc(**kw)
        assert lib.lde_desc_error(C.byref(d)) == b"", kw
        assert lib.lde_num_weights(C.byref(d)) == 0
        h = C.c_void_p()
        rc = lib.lde_create(C.byref(d), C.byref(h))
        assert rc in (0, -3), rc                           # LDE_OK with a GPU, LDE_ERR_NO_DEVICE without: never an argument error
        if rc == 0:
            assert lib.lde_set_noise(h, 1, 0, 0, None) == -2 and b"LDE_RHS_SPENDULUM only" in lib.lde_last_error(h)
            lib.lde_destroy(h)
    dims = "LDE_RHS_CVS needs state_dim=4, param_dim=2, augment_dim=0"
    refused = [
        (dict(state_dim=2), -1, dims),
        (dict(state_dim=5, param_dim=3), -1, dims),
        (dict(param_dim=4), -1, dims),
        (dict(param_dim=1), -1, dims),
        (dict(augment_dim=2), -1, dims),
        (dict(n_layers=1), -1, "LDE_RHS_CVS is analytic: n_layers must be 0"),
        (dict(rhs_kind=6), -1, "unknown rhs_kind"),                                        # 6, 8 and 10 are still no right-hand sides
        (dict(rhs_kind=8), -1, "unknown rhs_kind"),
        (dict(rhs_kind=10), -1, "unknown rhs_kind"),
        (dict(rhs_kind=12), -1, "unknown rhs_kind"),
        (dict(rhs_kind=-1), -1, "unknown rhs_kind"),
        (dict(param_dim=1, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -1, dims),    # the dims come before the solver
        (dict(sensealg=L.SENSE_DISCRETE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_PARALLEL_CHECKPOINTED), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE_CHECKPOINTED), -2, "LDE_RHS_CVS: only the solve on dual numbers exists"),
        (dict(batching=L.BATCH_COUPLED), -2, "LDE_RHS_CVS: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"),
        (dict(solver=L.SOLVER_EM, adaptive=0, dt=0.05), -2, "LDE_RHS_SPENDULUM only"),
        (dict(solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -2, "LDE_RHS_SPENDULUM only"),
        (dict(solver=L.SOLVER_RK4), -2, "RK4 is fixed-step only"),
    ]
    for kw, status, needle in refused:
        lib, d = _desc(**kw)
        h = C.c_void_p()
        assert lib.lde_create(C.byref(d), C.byref(h)) == status and not h.value, kw
        assert needle in lib.lde_desc_error(C.byref(d)).decode(), (kw, lib.lde_desc_error(C.byref(d)))
        assert lib.lde_num_weights(C.byref(d)) == 0
    # the feature is additive: the defaults are what they were
    lib, _ = _desc()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    assert (d.abi_version, d.rhs_kind, d.state_dim, d.param_dim, d.augment_dim, d.n_layers) == (1, 0, 2, 1, 0, 0)
    assert (d.solver, d.batching, d.sensealg, d.adaptive, d.maxiters, d.dt, d.abstol, d.reltol) == (0, 0, 3, 1, 100000, 0.0, 1e-6, 1e-3)


def test_python_plug_in_fields_and_default_layers():
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    cv = la.CVS()
    assert isinstance(cv.solver, la.Tsit5) and cv.sensealg.code == L.SENSE_FORWARD_DUAL and cv._rhs_kind == 11
    assert len(cv.prob.u0) == 4 and len(cv.prob.p) == 2 and cv.flat_weights() is None
    assert la.CVS(sensalg=la.BacksolveAdjoint()).sensealg.code == L.SENSE_BACKSOLVE_CHECKPOINTED   # (refused at the first solve)
    assert la.CVS(solver=la.RK4(), adaptive=False, dt=0.05).kwargs == dict(adaptive=False, dt=0.05)
    x = torch.linspace(-7.0, 7.0, 24, dtype=torch.float32).reshape(4, 2, 3)
    assert la.transform_after_diffeq(x, cv) is x                                   # the identity
    _, dec = TR.default_layers(la.GOKU_basic(), 784, cv, z0_activation="sigmoid", theta_activation="identity")
    lo_z0, lo_th = dec[0]
    assert tuple(lo_z0.sizes) == (16, 200, 4) and tuple(lo_th.sizes) == (16, 200, 2) and dec[1] is cv
    assert lo_z0.acts[-1] == L.CACT_SIGMOID and lo_th.acts[-1] == L.CACT_IDENTITY
    _, dflt = TR.default_layers(la.GOKU_basic(), 784, cv)
    assert dflt[0][0].acts[-1] == L.CACT_IDENTITY and dflt[0][1].acts[-1] == L.CACT_SOFTPLUS   # (the defaults: not the heads for this system)


def test_reference_right_hand_side_is_the_stated_form():
    """The reference evaluates the system with folded constants and 1 − σ(x) as 1/(1 + eˣ); include/lde.h states it in pressures with σ: the
    same numbers to rounding (1e-13 of the largest entry), on the inputs' ranges and well outside them."""
    rng = np.random.default_rng(2)
    for lo, hi in ((0.1, 1.0), (0.0, 3.0)):
        z = rng.uniform(lo, hi, (200, 4))
        th = np.stack([rng.uniform(-2, 2, 200), rng.uniform(0, 0.3, 200)], axis=1)
        u = np.zeros((200, R.D + R.D * R.NP))
        u[:, :4] = z
        want = R.rhs_plain(z, th)
        assert np.abs(R.rhs(u, th)[:, :4] - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("mode", ["tsit5-fixed", "rk4-fixed", "tsit5-steps"])
def test_reference_partials_are_the_central_differences_of_its_values(mode, eps):
    """ẑ₀, i_ext, r_mod perturbed on FIXED steps (a fixed dt, or the accepted steps of the unperturbed adaptive solve replayed): central
    differences in f64, at two difference steps, against the carried partials, to 1e-6 of J's largest entry. Measured: at most 3.3e-9."""
    B, T = 6, 20
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=4))
    ts = R.slow_grid(T)
    if mode == "tsit5-steps":
        _, _, ret, info = R.solve(z0, th, ts)
        assert (ret == 0).all()
        kw = dict(steps=(info["t"], info["dt"]))
    else:
        kw = dict(solver=R.TSIT5 if mode == "tsit5-fixed" else R.RK4, adaptive=False, dt=0.3)      # (0.3: save times inside the steps)
    _, J, ret, _ = R.solve(z0, th, ts, **kw)
    assert (ret == 0).all() and J.shape == (T, B, 4, 6)
    worst = 0.0
    for q in range(6):
        dz0, dth = np.zeros_like(z0), np.zeros_like(th)
        if q < 4:
            dz0[:, q] = eps
        else:
            dth[:, q - 4] = eps
        zp = R.solve(z0 + dz0, th + dth, ts, **kw)[0]
        zm = R.solve(z0 - dz0, th - dth, ts, **kw)[0]
        fd = (zp - zm) / (2 * eps)
        err = np.abs(fd - J[..., q]).max() / np.abs(J).max()
        worst = max(worst, err)
        assert err <= 1e-6, (q, err)
        assert np.abs(J[..., q]).max() > 1e-3, q              # (every direction moves something)
    print(f"{mode}, eps {eps}: central differences within {worst:.2e} of J's largest entry")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ["tsit5-adaptive", "tsit5-fixed", "rk4-grid"])
def test_reference_fourth_row_is_exact(mode, dtype):
    """z₃' = i_ext·SV_MOD depends on i_ext alone: row 3 of J is exactly (0, 0, 0, 1, ·, 0) in both precisions — zeros and a one, not residue —
    J[3, 4] = SV_MOD·t and z₃ = z₃(0) + i_ext·SV_MOD·t to rounding. (RK4 with save times on its steps' ends: the cubic Hermite's weights
    h00 + h01 are 1 only in exact arithmetic, so a save time inside an RK4 step may round the 1.)"""
    B, T = 5, 20
    z0, th = R.inputs(B, seed=5)
    ts = R.slow_grid(T) if mode != "rk4-grid" else R.grid(T)
    kw = dict() if mode == "tsit5-adaptive" else dict(solver=R.TSIT5, adaptive=False, dt=0.3) if mode == "tsit5-fixed" else dict(solver=R.RK4, adaptive=False, dt=0.05)
    z, J, ret, _ = R.solve(z0, th, ts, dtype=dtype, **kw)
    assert (ret == 0).all()
    assert (J[:, :, 3, [0, 1, 2, 5]] == 0).all() and (J[:, :, 3, 3] == 1).all()
    tol = 1e-7 if dtype == np.float64 else 2e-6      # (the state advances by the f32 of the f64 step in either mode: 2⁻²⁴ = 6e-8 per step)
    want = R.SV_MOD * ts[:, None] * np.ones(B)
    assert np.abs(J[:, :, 3, 4] - want).max() <= tol * np.abs(want).max()
    z3 = z0[None, :, 3].astype(np.float64) + th[None, :, 0].astype(np.float64) * R.SV_MOD * ts[:, None]
    assert np.abs(z[:, :, 3] - z3).max() <= tol * np.abs(z3).max()


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_conserves_the_blood_volume(solver):
    """400·z₀ + 1110·z₁ − i_ext·t is constant along a solve (a linear invariant: every Runge–Kutta method keeps it to rounding), and its
    tangent: 400·J[0, q] + 1110·J[1, q] = (400, 1110, 0, 0, t, 0) — to 1e-12 of the largest entry in f64."""
    B, T = 16, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=7))
    ts = R.slow_grid(T)
    z, J, ret, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=0.25)
    assert (ret == 0).all()
    V = R.volume(z, th, ts)
    assert np.abs(V - V[0]).max() <= 1e-12 * np.abs(V).max(), np.abs(V - V[0]).max()
    assert np.abs(z[-1] - z[0]).max() > 1e-2                                        # (the state itself moves)
    want = np.zeros((T, B, 6))
    want[..., 0], want[..., 1], want[..., 4] = 400.0, 1110.0, ts[:, None]
    got = 400.0 * J[:, :, 0] + 1110.0 * J[:, :, 1]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want).max()


def test_reference_rk4_error_falls_with_the_fourth_power_of_the_step():
    """RK4's global error at t = 49 against a fine solve (dt = 1/16) falls about 16× per halving of dt, from dt = 2 to 1 to 0.5: at least 12×
    (order 4 gives 16) and less than 32× (what a pure fifth-order term would give — the next term of the expansion raises the ratio above 16
    at these large steps). Measured: 1.01e-6, 4.94e-8, 2.75e-9 — ratios 20.5 and 18.0, falling towards 16. (All three steps are exact in f32.)"""
    B, T = 8, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=8))
    ts = R.slow_grid(T)
    fine = R.solve(z0, th, ts, R.RK4, adaptive=False, dt=0.0625)[0]
    err = []
    for dt in (2.0, 1.0, 0.5):
        z, _, ret, _ = R.solve(z0, th, ts, R.RK4, adaptive=False, dt=dt)
        assert (ret == 0).all()
        err.append(np.abs(z[-1] - fine[-1]).max())
    print(f"RK4 global error at dt = 2, 1, 0.5: {err[0]:.2e}, {err[1]:.2e}, {err[2]:.2e}: ratios {err[0] / err[1]:.1f}, {err[1] / err[2]:.1f}")
    assert 12 <= err[0] / err[1] < 32 and 12 <= err[1] / err[2] < 32, err
    assert err[1] / err[2] < err[0] / err[1]                                       # (towards 16 as the step shrinks)


def _floor(z0, th, ts, dz, **kw):
    z64, J64, r64, _ = R.solve(z0, th, ts, **kw)
    z32, J32, r32, _ = R.solve(z0, th, ts, dtype=np.float32, **kw)
    assert z32.dtype == np.float32 and J32.dtype == np.float32 and (r64 == 0).all() and (r32 == 0).all()
    assert np.isfinite(z64).all() and np.isfinite(J64).all() and np.isfinite(z32).all() and np.isfinite(J32).all()
    g64, g32 = R.pullback(J64, dz), R.pullback(J32, dz)
    return tuple(np.abs(a - b).max() / np.abs(b).max() for a, b in ((z32, z64), (J32, J64), (g32[0], g64[0]), (g32[1], g64[1])))


def _within_a_quarter(tag, floor, bounds):
    print(f"f32 against f64 floor, {tag}: z {floor[0]:.2e}, J {floor[1]:.2e}, dz0 {floor[2]:.2e}, dtheta {floor[3]:.2e}; bounds {bounds}")
    for f, b in zip(floor, bounds):
        assert f <= b / 4, (tag, floor, bounds)


@pytest.mark.parametrize("pa", [2000.0, 0.0])
def test_reference_saturated_baroreflex_stays_finite(pa):
    """p_a(0) = 2000 (eˣ overflows f32: w = 0) and p_a(0) = 0 (eˣ ≈ 3e-6: w ≈ 1): values and tangents are finite in both precisions — w·(1 − w)
    is 0 or tiny, never inf·0 — and the f32 mode stays within a quarter of the standing bounds (tests/test_gpu_cvs.py's case: (20, 37), RK4
    at 0.05)."""
    T, B = 20, 37
    z0, th = R.saturated_inputs(B, pa)
    u = np.zeros((B, R.D + R.D * R.NP), np.float32)
    u[:, :4] = z0
    u[:, 4:] = 1.0
    du = R.rhs(u, th)
    assert np.isfinite(du).all()
    if pa == 2000.0:
        assert (du[:, 4 + 2 * R.NP:4 + 3 * R.NP] == -np.float32(1.0 / R.TAU)).all()      # w and ∂w are exact zeros: row 2's tangent is −v₂/TAU alone
    _within_a_quarter(f"p_a(0) = {pa}", _floor(z0, th, R.grid(T), R.cotangent(T, B), solver=R.RK4, adaptive=False, dt=0.05), R.BOUNDS)


@pytest.mark.parametrize("T,B", R.SHAPES[1:])
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_f32_floor_under_the_gpu_bounds(solver, dt, T, B):
    """The f32 restatement against the f64 one on tests/test_gpu_cvs.py's own fixed-step inputs, relative to the largest entry: the floor under
    the GPU bounds, which must stay within a quarter of them. Measured on (50, 256) (ẑ / J / dz0 / dθ): dt = 0.05 1.5e-6 / 9.7e-7 / 3.1e-7 /
    3.5e-7 — the dual tests' 2e-5 and 1e-4 stand; dt = 0.0125 5.8e-6 / 2.9e-6 / 1.3e-6 / 8.0e-7 with either solver — ẑ does not fit a quarter
    of 2e-5 (196 f32 updates of a state whose increments are 1e-4 of it), so by the project's rule that case's ẑ bound is 4 × its floor,
    rounded up: 2.5e-5 (tests/cvs_ref.py: FINE_BOUNDS). (2, 37) fits the standing bounds at both steps."""
    z0, th = R.inputs(B, seed=R.PARITY_SEED[T])
    floor = _floor(z0, th, R.grid(T), R.cotangent(T, B), solver=solver, adaptive=False, dt=dt)
    _within_a_quarter(f"solver {solver} dt {dt} ({T}, {B})", floor, R.bounds(solver, dt, T))


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_f32_floor_of_the_blood_volume(solver, dt):
    """tests/test_gpu_cvs.py::test_blood_volume on the reference's own f32 mode, (50, 256): the volume's drift relative to its largest entry
    and the pullback of the cotangent c_j·(400, 1110, 0, 0) against (400 Σc, 1110 Σc, 0, 0) and (Σ c_j t_j, 0), each within a quarter of the
    case's bound. Measured (drift / dz0 / dθ): dt = 0.05 3.1e-7 / 1.2e-7 / 2.2e-5; dt = 0.0125 9.9e-7 / 3.7e-7 / 5.0e-5 — dθ does not fit a
    quarter of 1e-4 there, so that case's dθ bound is 4 × its floor, rounded up: 2.1e-4 (tests/cvs_ref.py: volume_bounds)."""
    T, B = 50, 256
    z0, th = R.inputs(B, seed=R.PARITY_SEED[T])
    ts = R.grid(T)
    dz, want0, wantth = R.volume_cotangent(T, B, ts)
    z, J, ret, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=dt, dtype=np.float32)
    assert (ret == 0).all()
    V = R.volume(z.astype(np.float64), th.astype(np.float64), ts)
    g0, gth = R.pullback(J, dz)
    floor = (np.abs(V - V[0]).max() / np.abs(V).max(), np.abs(g0 - want0).max() / np.abs(want0).max(), np.abs(gth - wantth).max() / np.abs(wantth).max())
    b = R.volume_bounds(solver, dt)
    print(f"solver {solver} dt {dt}: f32 volume drift {floor[0]:.2e}, dz0 {floor[1]:.2e}, dtheta {floor[2]:.2e} (bounds {b})")
    assert floor[0] <= b[0] / 4 and floor[1] <= b[1] / 4 and floor[2] <= b[2] / 4, floor


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_f32_floor_on_the_slow_grid(solver):
    """(50, 37) on ts = 1.0·j at dt = 0.25. Measured: 5.6e-6 / 2.8e-6 / 1.2e-6 / 1.4e-6 — ẑ over a quarter of 2e-5 again: 2.5e-5 (FINE_BOUNDS)."""
    T, B = R.SLOW_SHAPE
    z0, th = R.inputs(B, seed=R.SLOW_SEED)
    floor = _floor(z0, th, R.slow_grid(T), R.cotangent(T, B), solver=solver, adaptive=False, dt=R.SLOW_DT)
    _within_a_quarter(f"slow grid, solver {solver}", floor, R.FINE_BOUNDS)
    assert floor[0] > R.BOUNDS[0] / 4                                              # (why this case has a bound of its own)


def test_reference_f32_floor_of_the_adaptive_case():
    """The inputs of the GPU test of the adaptive solve, (50, 37) on ts = 1.0·j at 1e-6 / 1e-3: the reference's own accepted steps replayed in
    both modes. Measured: 1.9e-6 / 2.2e-6 / 6.9e-7 / 8.8e-7, within a quarter of the standing bounds; 22.1 accepted steps per trajectory, none
    rejected. And the first accepted step: the f32 mode's equals the f64 mode's to 1e-4 for all 37 (measured 6.5e-8)."""
    T, B = R.SLOW_SHAPE
    z0, th = R.inputs(B, seed=R.ADAPTIVE_SEED)
    _, _, ret, info = R.solve(z0, th, R.slow_grid(T))
    assert (ret == 0).all()
    print(f"accepted steps per trajectory {info['naccept'] / B:.1f}, rejected {info['nreject']}")
    floor = _floor(z0, th, R.slow_grid(T), R.cotangent(T, B), steps=(info["t"], info["dt"]))
    _within_a_quarter("adaptive, own steps replayed", floor, R.BOUNDS)
    d64 = np.array([d[0] for d in info["dt"]])
    d32 = np.array([d[0] for d in R.solve(z0, th, R.slow_grid(T), dtype=np.float32)[3]["dt"]])
    print(f"first accepted step, f32 against f64: largest relative difference {np.abs(d32 / d64 - 1).max():.2e}")
    assert (np.abs(d32 - d64) <= 1e-4 * d64).all()


def test_reference_f32_floor_of_the_ragged_and_the_long_grid():
    """The inputs of the GPU tests on the ragged nine-point grid (B = 3, the reference's own steps replayed) and on T = 6001 save times (B = 3,
    Tsit5 at dt = 0.0125, t ≤ 6): both within a quarter of the standing bounds. The ragged grid is tests/dual_ref.py's stretched 20×: on the
    reference's own steps every trajectory has a step with at least two save times and a step with none."""
    ts = R.ragged_grid()
    assert len(ts) == 9 and ts[-1] == 49.0
    z0, th = R.inputs(3, seed=R.RAGGED_SEED)
    _, _, ret, info = R.solve(z0, th, ts)
    assert (ret == 0).all()
    for b in range(3):
        per_step = np.histogram(ts[1:], bins=np.append(info["t"][b], ts[-1] + 1e-9))[0]
        assert per_step.max() >= 2 and (per_step == 0).sum() >= 1, per_step
    _within_a_quarter("ragged grid", _floor(z0, th, ts, R.cotangent(len(ts), 3), steps=(info["t"], info["dt"])), R.BOUNDS)
    T = 6001
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(3, seed=R.LONG_SEED)
    _within_a_quarter("T = 6001", _floor(z0, th, ts, R.cotangent(T, 3), solver=R.TSIT5, adaptive=False, dt=0.0125), R.BOUNDS)


def test_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "cvs_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "cvs_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "cardiovascular system host logic under ASan + UBSan" in r.stdout
