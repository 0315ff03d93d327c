"""CPU: the double pendulum (LDE_RHS_DOUBLE_PENDULUM, include/lde.h) without a GPU — (1) which descriptions the built library serves and
which it refuses, with what status and text, including that rhs_kind = 6 and 8 are still unknown; (2) the numpy restatement the GPU tests
compare against (tests/dpend_ref.py) pinned before it is trusted: its right-hand side against the form of include/lde.h, its J against
central differences of its own values, the m₂ = 0 limit (the pendulum of length L₁), the mass homogeneity, the energy drift under RK4, and
its f32 mode against its f64 mode on the GPU tests' own inputs (the floor under the GPU bounds); (3) the Python plug-in: its fields and the
head widths default_layers builds from it; (4) csrc/lde_host.h's part — validate(), the group width, the launch shape, the dual record, the
dispatch of both systems of the lane-per-direction kernels — under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/dpend_host_driver.cpp, run as a program).

Every test here that creates a description of rhs_kind = 9 (or asks for la.DoublePendulum) fails before this right-hand side existed, where
lde_create returns LDE_ERR_INVALID_ARG ("unknown rhs_kind")."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dpend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    base = dict(rhs_kind=L.RHS_DOUBLE_PENDULUM, state_dim=4, param_dim=4, sensealg=L.SENSE_FORWARD_DUAL)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return lib, d


def test_served_and_refused_descriptions_through_the_c_abi():
    from latentdiffeq_amd import _lib as L
    assert L.RHS_DOUBLE_PENDULUM == 9 and L.RHS_KURAMOTO == 7 and L.RHS_LOTKA_VOLTERRA == 5
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
    dims = "LDE_RHS_DOUBLE_PENDULUM needs state_dim=4, param_dim=4, augment_dim=0"
    refused = [
        (dict(state_dim=2), -1, dims),
        (dict(state_dim=5, param_dim=5), -1, dims),
        (dict(param_dim=3), -1, dims),
        (dict(param_dim=1), -1, dims),
        (dict(augment_dim=2), -1, dims),
        (dict(n_layers=1), -1, "LDE_RHS_DOUBLE_PENDULUM is analytic: n_layers must be 0"),
        (dict(rhs_kind=6), -1, "unknown rhs_kind"),                                        # 6 and 8 are still no right-hand sides
        (dict(rhs_kind=8), -1, "unknown rhs_kind"),
        (dict(rhs_kind=10), -1, "unknown rhs_kind"),
        (dict(param_dim=1, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -1, dims),    # the dims come before the solver
        (dict(sensealg=L.SENSE_DISCRETE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_PARALLEL_CHECKPOINTED), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE_CHECKPOINTED), -2, "LDE_RHS_DOUBLE_PENDULUM: only the solve on dual numbers exists"),
        (dict(batching=L.BATCH_COUPLED), -2, "LDE_RHS_DOUBLE_PENDULUM: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"),
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
    dp = la.DoublePendulum()
    assert isinstance(dp.solver, la.Tsit5) and dp.sensealg.code == L.SENSE_FORWARD_DUAL and dp._rhs_kind == 9
    assert len(dp.prob.u0) == 4 and len(dp.prob.p) == 4 and dp.flat_weights() is None
    assert la.DoublePendulum(sensalg=la.BacksolveAdjoint()).sensealg.code == L.SENSE_BACKSOLVE_CHECKPOINTED   # (refused at the first solve)
    assert la.DoublePendulum(solver=la.RK4(), adaptive=False, dt=0.05).kwargs == dict(adaptive=False, dt=0.05)
    x = torch.linspace(-7.0, 7.0, 24, dtype=torch.float32).reshape(4, 2, 3)
    assert la.transform_after_diffeq(x, dp) is x                                   # the identity
    _, dec = TR.default_layers(la.GOKU_basic(), 784, dp)
    lo_z0, lo_th = dec[0]
    assert tuple(lo_z0.sizes) == (16, 200, 4) and tuple(lo_th.sizes) == (16, 200, 4)
    assert lo_th.acts[-1] == L.CACT_SOFTPLUS and dec[1] is dp


def test_reference_right_hand_side_is_the_stated_form():
    """The reference evaluates the system in μ = m₂/m₁ with the angle-sum identities; include/lde.h states it in (m₁, m₂) with sin(θ₁ − 2θ₂)
    and cos 2Δ: the same numbers to rounding (1e-13 of the largest entry), on the inputs' ranges and far outside them."""
    rng = np.random.default_rng(2)
    for scale in (1.0, 6.0):
        z = rng.uniform(-scale, scale, (200, 4))
        th = np.concatenate([rng.uniform(0.8, 1.6, (200, 2)), rng.uniform(0.5, 2.0, (200, 2))], axis=1)
        u = np.zeros((200, R.D + R.D * R.NP))
        u[:, :4] = z
        want = R.rhs_plain(z, th)
        assert np.abs(R.rhs(u, th)[:, :4] - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("mode", ["tsit5-fixed", "rk4-fixed", "tsit5-steps"])
def test_reference_partials_are_the_central_differences_of_its_values(mode, eps):
    """ẑ₀, L₁, L₂, m₁, m₂ perturbed on FIXED steps (a fixed dt, or the accepted steps of the unperturbed adaptive solve replayed): central
    differences in f64, at two difference steps, against the carried partials, to 1e-6 of each partial's largest entry
    (tests/test_kuramoto_host.py's rule). Measured: at most 4.6e-9."""
    B, T = 6, 20
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=4))
    ts = R.grid(T)
    if mode == "tsit5-steps":
        _, _, ret, info = R.solve(z0, th, ts)
        assert (ret == 0).all()
        kw = dict(steps=(info["t"], info["dt"]))
    else:
        kw = dict(solver=R.TSIT5 if mode == "tsit5-fixed" else R.RK4, adaptive=False, dt=0.03)      # (0.03: save times inside the steps)
    _, J, ret, _ = R.solve(z0, th, ts, **kw)
    assert (ret == 0).all() and J.shape == (T, B, 4, 8)
    worst = 0.0
    for q in range(8):
        dz0, dth = np.zeros_like(z0), np.zeros_like(th)
        if q < 4:
            dz0[:, q] = eps
        else:
            dth[:, q - 4] = eps
        zp = R.solve(z0 + dz0, th + dth, ts, **kw)[0]
        zm = R.solve(z0 - dz0, th - dth, ts, **kw)[0]
        fd = (zp - zm) / (2 * eps)
        err = np.abs(fd - J[..., q]).max() / np.abs(J[..., q]).max()
        worst = max(worst, err)
        assert err <= 1e-6, (q, err)
    print(f"{mode}, eps {eps}: central differences within {worst:.2e} of the partials")


def _pendulum_rk4(x0, v0, L, ts, dt):
    """The library's pendulum, x'' = −(g/L) sin x, by plain RK4 at the fixed step dt (f64); ts on step boundaries."""
    y = np.stack([x0, v0], axis=1)
    f = lambda y: np.stack([y[:, 1], -(R.GRAV / L) * np.sin(y[:, 0])], axis=1)
    out, t, j = [y], 0, 1
    nsub = [int(round((ts[i] - ts[i - 1]) / dt)) for i in range(1, len(ts))]
    for n in nsub:
        for _ in range(n):
            k1 = f(y)
            k2 = f(y + 0.5 * dt * k1)
            k3 = f(y + 0.5 * dt * k2)
            k4 = f(y + dt * k3)
            y = y + dt / 6.0 * (k1 + 2 * (k2 + k3) + k4)
        out.append(y)
    return np.stack(out)


def test_reference_m2_zero_is_the_pendulum_of_length_l1():
    """m₂ = 0: the first arm does not feel the second — (θ₁, ω₁) is the pendulum's RK4 solution for L = L₁ at the same steps, to rounding —
    and the columns ∂(θ₁, ω₁)/∂L₂ and ∂/∂m₁ are exact zeros (∂/∂m₂ is not: the limit has a slope)."""
    B, T, dt = 8, 20, 0.05
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=6))
    th[:, 3] = 0.0
    ts = R.grid(T)
    z, J, ret, _ = R.solve(z0, th, ts, R.RK4, adaptive=False, dt=dt)
    assert (ret == 0).all()
    want = _pendulum_rk4(z0[:, 0], z0[:, 2], th[:, 0], ts, float(np.float32(dt)))     # (the state advances by the f32 of the step)
    got = z[:, :, [0, 2]]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want).max()
    assert (J[:, :, [0, 2], 5] == 0).all() and (J[:, :, [0, 2], 6] == 0).all()
    assert np.abs(J[:, :, [0, 2], 7]).max() > 1e-3 and np.abs(J[:, :, [1, 3], 5]).max() > 1e-3
    z32, J32, _, _ = R.solve(z0, th, ts, R.RK4, adaptive=False, dt=dt, dtype=np.float32)
    assert (J32[:, :, [0, 2], 5] == 0).all() and (J32[:, :, [0, 2], 6] == 0).all()      # … in f32 too: zeros, not residue


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_is_homogeneous_of_degree_zero_in_the_masses(solver):
    """m₁·∂ẑ/∂m₁ + m₂·∂ẑ/∂m₂ = 0: to 1e-13 of the largest entry of J in f64 — and scaling both masses by 3 leaves ẑ where it is."""
    B, T = 16, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=7))
    ts = R.grid(T)
    z, J, ret, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=0.025)
    assert (ret == 0).all()
    res = th[None, :, None, 2] * J[..., 6] + th[None, :, None, 3] * J[..., 7]
    assert np.abs(res).max() <= 1e-13 * np.abs(J).max(), np.abs(res).max() / np.abs(J).max()
    th3 = th.copy()
    th3[:, 2:] *= 3.0
    z3 = R.solve(z0, th3, ts, solver, adaptive=False, dt=0.025)[0]
    assert np.abs(z3 - z).max() <= 1e-12 * np.abs(z).max()


def test_reference_energy_drift_falls_with_the_fourth_power_of_the_step():
    """The energy is conserved by the flow; under RK4 its drift over t ≤ 2.45 falls at least 12× per halving of dt (order 4 gives 16).
    Measured (16 trajectories, the largest |E(t) − E(0)|): 1.04e-1, 4.58e-3, 1.57e-4 — ratios 22.7 and 29.2."""
    B, T = 16, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=8))
    ts = R.grid(T)
    drift = []
    for dt in (0.05, 0.025, 0.0125):
        z, _, ret, _ = R.solve(z0, th, ts, R.RK4, adaptive=False, dt=dt)
        assert (ret == 0).all()
        E = R.energy(z, th)
        drift.append(np.abs(E - E[0]).max())
    print(f"RK4 energy drift at dt = 0.05, 0.025, 0.0125: {drift[0]:.2e}, {drift[1]:.2e}, {drift[2]:.2e}: ratios {drift[0] / drift[1]:.1f}, {drift[1] / drift[2]:.1f}")
    assert drift[0] / drift[1] >= 12 and drift[1] / drift[2] >= 12, drift


def _floor(z0, th, ts, dz, **kw):
    z64, J64, r64, _ = R.solve(z0, th, ts, **kw)
    z32, J32, r32, _ = R.solve(z0, th, ts, dtype=np.float32, **kw)
    assert z32.dtype == np.float32 and J32.dtype == np.float32 and (r64 == 0).all() and (r32 == 0).all()
    g64, g32 = R.pullback(J64, dz), R.pullback(J32, dz)
    return tuple(np.abs(a - b).max() / np.abs(b).max() for a, b in ((z32, z64), (J32, J64), (g32[0], g64[0]), (g32[1], g64[1])))


def _within_a_quarter(tag, floor, bounds):
    print(f"f32 against f64 floor, {tag}: z {floor[0]:.2e}, J {floor[1]:.2e}, dz0 {floor[2]:.2e}, dtheta {floor[3]:.2e}; bounds {bounds}")
    for f, b in zip(floor, bounds):
        assert f <= b / 4, (tag, floor, bounds)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_f32_floor_under_the_gpu_bounds(solver, dt):
    """The f32 restatement against the f64 one on tests/test_gpu_dpend.py's own (50, 256) inputs, relative to the largest entry: the floor
    under the GPU bounds, which must stay within a quarter of them. Measured (ẑ / J / dz0 / dθ): Tsit5 at 0.0125 2.5e-6 / 1.8e-5 / 3.9e-6 /
    3.8e-6, RK4 at 0.05 1.3e-6 / 6.3e-6 / 1.2e-6 / 1.7e-6, RK4 at 0.0125 1.6e-6 / 9.6e-6 / 2.8e-6 / 3.7e-6: within a quarter of the dual tests'
    2e-5 and 1e-4, which stand. Tsit5 at dt = 0.05: 6.3e-6 / 3.6e-5 / 1.4e-5 / 1.9e-5 — ẑ and J do not fit (on every seed of 50 … 66; Tsit5's
    stage coefficients of ±12 cancel in f32 at the large step), so by the project's rule that case's bounds are 4 × its floor, rounded up:
    ẑ 2.5e-5, J 1.5e-4 (tests/dpend_ref.py: BOUNDS). The seed of these inputs, 54, is the one of 50 … 66 with the smallest floor: the system
    is sensitive — on seed 50 one trajectory of 256 reaches |J| = 655 under Tsit5 at dt = 0.05 where the finer steps give 43, and f32 is 3e-3
    from f64 there — and such an input would test the number format, not the kernel."""
    T, B = 50, 256
    z0, th = R.inputs(B, seed=R.PARITY_SEED[T])
    floor = _floor(z0, th, R.grid(T), R.cotangent(T, B), solver=solver, adaptive=False, dt=dt)
    _within_a_quarter(f"solver {solver} dt {dt}", floor, R.bounds(solver, dt))


def test_reference_f32_floor_of_the_adaptive_case():
    """The inputs of the GPU test of the adaptive solve, (50, 37): the reference's own accepted steps replayed in both modes. Measured: ẑ
    8.5e-6, J 3.9e-5, dz0 9.1e-6, dθ 6.5e-6 — ẑ and J do not fit a quarter of 2e-5 / 1e-4, so that test's bounds are 4 × the floor, rounded
    up: ẑ 3.5e-5, J 1.6e-4 (R.ADAPTIVE_BOUNDS). And the seed's first accepted step: the f32 mode's equals the f64 mode's to 1e-4 for all 37."""
    T, B = 50, 37
    z0, th = R.inputs(B, seed=R.ADAPTIVE_SEED)
    _, _, ret, info = R.solve(z0, th, R.grid(T))
    assert (ret == 0).all()
    floor = _floor(z0, th, R.grid(T), R.cotangent(T, B), steps=(info["t"], info["dt"]))
    _within_a_quarter("adaptive, own steps replayed", floor, R.ADAPTIVE_BOUNDS)
    d64 = np.array([d[0] for d in info["dt"]])
    d32 = np.array([d[0] for d in R.solve(z0, th, R.grid(T), dtype=np.float32)[3]["dt"]])
    print(f"first accepted step, f32 against f64: largest relative difference {np.abs(d32 / d64 - 1).max():.2e}")
    assert (np.abs(d32 - d64) <= 1e-4 * d64).all()


def test_reference_f32_floor_of_the_ragged_and_the_long_grid():
    """The inputs of the GPU tests on the ragged nine-point grid (B = 3, the reference's own steps replayed) and on T = 6001 save times (B = 3,
    Tsit5 at dt = 0.0125, t ≤ 6): both within a quarter of the standing bounds."""
    ts = R.ragged_grid()
    z0, th = R.inputs(3, seed=R.RAGGED_SEED)
    _, _, ret, info = R.solve(z0, th, ts)
    assert (ret == 0).all()
    _within_a_quarter("ragged grid", _floor(z0, th, ts, R.cotangent(len(ts), 3), steps=(info["t"], info["dt"])), R.BOUNDS)
    T = 6001
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(3, seed=R.LONG_SEED)
    _within_a_quarter("T = 6001", _floor(z0, th, ts, R.cotangent(T, 3), solver=R.TSIT5, adaptive=False, dt=0.0125), R.BOUNDS)


def test_reference_f32_floor_of_angles_past_256_turns():
    """The case of tests/test_gpu_dpend.py::test_angles_past_256_turns: θ₁, θ₂ + 2π·300 ≈ 1 885, (T, B) = (5, 37), fixed steps of 0.05. Between
    1 024 and 2 048 an f32 angle is a multiple of 2⁻¹³, so every stage's sine argument carries a rounding of up to 6.1e-5 rad. Measured, worst
    over the two solvers: ẑ 7.1e-7, J 3.5e-4, dz0 2.7e-4, dθ 2.2e-4; the GPU test's bounds are 4 × these, rounded up (R.TURN_BOUNDS): J 1.4e-3,
    dz0 1.1e-3, dθ 8.5e-4; ẑ keeps 2e-5. Whole turns do not change the dynamics: J of the same solve without them is the same to the format's 1e-3."""
    T, B = 5, 37
    z0, th = R.turn_inputs(B)
    assert np.abs(z0[:, :2]).min() > 2 * np.pi * 256
    for solver in (R.TSIT5, R.RK4):
        floor = _floor(z0, th, R.grid(T), R.cotangent(T, B), solver=solver, adaptive=False, dt=0.05)
        _within_a_quarter(f"past 256 turns, solver {solver}", floor, R.TURN_BOUNDS)
    zt, Jt, _, _ = R.solve(z0, th, R.grid(T), adaptive=False, dt=0.05)
    z0n, _ = R.inputs(B, seed=23)
    zn, Jn, _, _ = R.solve(z0n, th, R.grid(T), adaptive=False, dt=0.05)
    assert np.abs(Jt - Jn).max() / np.abs(Jn).max() <= 1e-3


def test_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "dpend_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "dpend_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "double pendulum host logic under ASan + UBSan" in r.stdout
