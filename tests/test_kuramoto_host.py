"""CPU: the Kuramoto right-hand side (LDE_RHS_KURAMOTO, include/lde.h) without a GPU — (1) which descriptions the built library serves and
which it refuses, with what status and text, including that rhs_kind = 6 is still unknown; (2) the numpy restatement the GPU tests compare
against (tests/kuramoto_ref.py) pinned before it is trusted: its J against central differences of its own values, the uncoupled closed form,
the conserved phase sum, the two-oscillator closed form, its f32 mode against its f64 mode (the floor under the GPU bounds) and the seed of
the first-step test; (3) the Python plug-in: its fields, its hook, the head widths default_layers builds from it; (4) csrc/lde_host.h's part —
the group width, the launch shape, the dual record of every N, the dispatch, validate() — under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/kuramoto_host_driver.cpp, run as a program).

Every test here that creates a description of rhs_kind = 7 (or asks for la.Kuramoto) fails before this right-hand side existed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import kuramoto_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the bounds of tests/test_gpu_kuramoto.py, relative to the largest entry of the reference array
Z_BOUND, J_BOUND = 2e-5, 1e-4
TURN_J_BOUND, TURN_G0_BOUND, TURN_GTH_BOUND = 1.6e-4, 1e-4, 8e-4
FIRST_STEP_SEED = 50        # tests/test_gpu_kuramoto.py: the inputs of the adaptive tests


def _desc(N=3, **kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    base = dict(rhs_kind=L.RHS_KURAMOTO, state_dim=N, param_dim=N + 1, sensealg=L.SENSE_FORWARD_DUAL)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return lib, d


def test_served_and_refused_descriptions_through_the_c_abi():
    from latentdiffeq_amd import _lib as L
    assert L.RHS_KURAMOTO == 7 and L.RHS_LOTKA_VOLTERRA == 5
    assert L.load().lde_abi_version() == 1                 # lde_problem_desc did not change: N is state_dim
    for N in range(2, 8):
        for kw in (dict(), dict(adaptive=0, dt=0.05), dict(solver=L.SOLVER_RK4, adaptive=0, dt=0.0125), dict(dt=0.01)):
            lib, d = _desc(N, **kw)
            assert lib.lde_desc_error(C.byref(d)) == b"", (N, kw)
            assert lib.lde_num_weights(C.byref(d)) == 0
            h = C.c_void_p()
            rc = lib.lde_create(C.byref(d), C.byref(h))
            assert rc in (0, -3), rc                       # LDE_OK with a GPU, LDE_ERR_NO_DEVICE without: never an argument error
            if rc == 0:
                lib.lde_destroy(h)
    dims = "LDE_RHS_KURAMOTO needs state_dim=N with 2 <= N <= 7, param_dim=N+1, augment_dim=0"
    refused = [
        (dict(state_dim=1, param_dim=2), -1, dims),
        (dict(state_dim=8, param_dim=9), -1, dims),
        (dict(param_dim=3), -1, dims),
        (dict(param_dim=1), -1, dims),
        (dict(augment_dim=2), -1, dims),
        (dict(n_layers=1), -1, "LDE_RHS_KURAMOTO is analytic: n_layers must be 0"),
        (dict(rhs_kind=6), -1, "unknown rhs_kind"),                                        # 6 is still no right-hand side
        (dict(rhs_kind=8), -1, "unknown rhs_kind"),
        (dict(param_dim=1, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -1, dims),    # the dims come before the solver
        (dict(sensealg=L.SENSE_DISCRETE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_PARALLEL_CHECKPOINTED), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE_CHECKPOINTED), -2, "LDE_RHS_KURAMOTO: only the solve on dual numbers exists"),
        (dict(batching=L.BATCH_COUPLED), -2, "LDE_RHS_KURAMOTO: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"),
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


def test_python_plug_in_fields_hook_and_default_layers():
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    ku = la.Kuramoto()
    assert ku.N == 3 and isinstance(ku.solver, la.Tsit5) and ku.sensealg.code == L.SENSE_FORWARD_DUAL and ku._rhs_kind == 7
    assert len(ku.prob.u0) == 3 and len(ku.prob.p) == 4
    assert la.Kuramoto(5, sensalg=la.BacksolveAdjoint()).sensealg.code == L.SENSE_BACKSOLVE_CHECKPOINTED   # (refused at the first solve)
    assert la.Kuramoto(N=4, solver=la.RK4(), adaptive=False, dt=0.05).kwargs == dict(adaptive=False, dt=0.05)
    # the hook is the sine, through the module-level dispatch diffeq_layer uses, and autograd sees through it
    x = torch.linspace(-7.0, 7.0, 24, dtype=torch.float32).reshape(3, 2, 4).requires_grad_()
    y = la.transform_after_diffeq(x, ku)
    assert torch.equal(y, torch.sin(x))
    y.sum().backward()
    assert torch.equal(x.grad, torch.cos(x.detach()))
    assert la.transform_after_diffeq(x, la.LotkaVolterra()) is x                  # the other plug-ins keep the identity
    for N in (2, 3, 7):
        k = la.Kuramoto(N)
        assert len(k.prob.u0) == N and len(k.prob.p) == N + 1
        _, dec = TR.default_layers(la.GOKU_basic(), 784, k)
        lo_z0, lo_th = dec[0]
        assert tuple(lo_z0.sizes) == (16, 200, N) and tuple(lo_th.sizes) == (16, 200, N + 1)
        assert lo_th.acts[-1] == L.CACT_SOFTPLUS and dec[1] is k


@pytest.mark.parametrize("N", [2, 3, 7])
@pytest.mark.parametrize("mode", ["tsit5-fixed", "rk4-fixed", "tsit5-steps"])
def test_reference_partials_are_the_central_differences_of_its_values(mode, N):
    """φ₀, ω, K perturbed on FIXED steps (a fixed dt, or the accepted steps of the unperturbed adaptive solve replayed): central differences
    in f64 against the carried partials, to 1e-6 of each partial's largest entry."""
    B, T = 6, 20
    z0, th = (a.astype(np.float64) for a in R.inputs(B, N, seed=4))
    ts = R.grid(T)
    if mode == "tsit5-steps":
        _, _, ret, info = R.solve(z0, th, ts)
        assert (ret == 0).all()
        kw = dict(steps=(info["t"], info["dt"]))
    else:
        kw = dict(solver=R.TSIT5 if mode == "tsit5-fixed" else R.RK4, adaptive=False, dt=0.03)      # (0.03: save times inside the steps)
    _, J, ret, _ = R.solve(z0, th, ts, **kw)
    assert (ret == 0).all() and J.shape == (T, B, N, 2 * N + 1)
    eps = 1e-6
    for q in range(2 * N + 1):
        dz0, dth = np.zeros_like(z0), np.zeros_like(th)
        if q < N:
            dz0[:, q] = eps
        else:
            dth[:, q - N] = eps
        zp = R.solve(z0 + dz0, th + dth, ts, **kw)[0]
        zm = R.solve(z0 - dz0, th - dth, ts, **kw)[0]
        fd = (zp - zm) / (2 * eps)
        err = np.abs(fd - J[..., q]).max() / np.abs(J[..., q]).max()
        assert err <= 1e-6, (q, err)


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_reproduces_the_uncoupled_closed_form(solver):
    """K = 0: φ_i(t) = φ_i0 + ω_i t, ∂φ_i/∂φ_j0 = δ_ij, ∂φ_i/∂ω_j = δ_ij t (the K column is NOT zero at K = 0 and is not looked at)."""
    N, B, T = 4, 8, 20
    z0, th = (a.astype(np.float64) for a in R.inputs(B, N, seed=6))
    th[:, N] = 0.0
    ts = R.grid(T)
    kw = dict(abstol=1e-10, reltol=1e-10) if solver == R.TSIT5 else dict(adaptive=False, dt=0.0025)
    z, J, ret, _ = R.solve(z0, th, ts, solver, **kw)
    assert (ret == 0).all()
    t = ts[:, None, None]
    zc = z0[None] + th[None, :, :N] * t
    eye = np.eye(N)[None, None]
    # the state advances by (float)dt while t advances by dt (include/lde.h): the solve sees a time that is off by up to 2⁻²⁴ relative
    tol = np.abs(th[:, :N]).max() * ts[-1] * 2.0 ** -24 + 1e-9
    assert np.abs(z - zc).max() <= tol, np.abs(z - zc).max()
    assert np.abs(J[..., :N] - eye).max() <= 1e-9
    assert np.abs(J[..., N:2 * N] - eye * ts[:, None, None, None]).max() <= ts[-1] * 2.0 ** -24 + 1e-9
    assert np.abs(J[..., 2 * N]).max() > 1e-3                        # ∂φ/∂K ≠ 0 at K = 0


@pytest.mark.parametrize("N", [2, 5, 7])
def test_reference_conserves_the_phase_sum(N):
    """Σ_i φ_i(t) = Σ φ_i0 + t Σ ω_i for any K (the coupling is antisymmetric) — and so do the partials: Σ_i ∂φ_i/∂φ_j0 = 1, Σ_i ∂φ_i/∂ω_j = t,
    Σ_i ∂φ_i/∂K = 0. Runge–Kutta methods keep linear invariants: to rounding, at the default tolerances."""
    B, T = 16, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, N, seed=7))
    ts = R.grid(T)
    z, J, ret, _ = R.solve(z0, th, ts)
    assert (ret == 0).all()
    want = z0.sum(axis=1)[None] + ts[:, None] * th[:, :N].sum(axis=1)[None]
    assert np.abs(z.sum(axis=2) - want).max() <= 1e-6 * np.abs(want).max() + ts[-1] * N * 2 * 2.0 ** -24
    Js = J.sum(axis=2)                                               # [T, B, NP]
    assert np.abs(Js[..., :N] - 1).max() <= 1e-12
    assert np.abs(Js[..., N:2 * N] - ts[:, None, None]).max() <= ts[-1] * 2.0 ** -23
    assert np.abs(Js[..., 2 * N]).max() <= 1e-12


def test_reference_reproduces_the_two_oscillator_closed_form():
    """N = 2 with ω₁ = ω₂: ψ = φ₂ − φ₁ obeys ψ' = −K sin ψ, so tan(ψ/2) = tan(ψ₀/2)·e^{−Kt}."""
    B, T = 16, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, 2, seed=8))
    th[:, 1] = th[:, 0]
    ts = R.grid(T)
    z, _, ret, _ = R.solve(z0, th, ts, abstol=1e-10, reltol=1e-10)
    assert (ret == 0).all()
    psi = z[..., 1] - z[..., 0]
    want = np.tan((z0[:, 1] - z0[:, 0]) / 2)[None] * np.exp(-th[:, 2][None] * ts[:, None])
    err = np.abs(np.tan(psi / 2) - want).max() / np.abs(want).max()
    assert err <= 1e-6, err


def _floor(z0, th, ts, dz, worst, cases):
    for solver, dt in cases:
        z64, J64, r64, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=dt)
        z32, J32, r32, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=dt, dtype=np.float32)
        assert z32.dtype == np.float32 and J32.dtype == np.float32 and (r64 == 0).all() and (r32 == 0).all()
        g64, g32 = R.pullback(J64, dz), R.pullback(J32, dz)
        for key, a, b in (("z", z32, z64), ("J", J32, J64), ("g0", g32[0], g64[0]), ("gth", g32[1], g64[1])):
            worst[key] = max(worst[key], np.abs(a - b).max() / np.abs(b).max())


def test_reference_f32_floor_under_the_gpu_bounds():
    """The f32 restatement against the f64 one on the largest GPU case of each N — (T, B) = (50, 256), both solvers, both step sizes —
    relative to the largest entry: the floor under the bounds of tests/test_gpu_kuramoto.py. Measured, worst over N ∈ {2, 3, 4, 7}: ẑ 2.0e-6,
    J 1.8e-5 (N = 4; 2.3e-6 to 4.1e-6 at the other N), dz0 6.3e-6, dθ 6.2e-6 — all within a quarter of the bounds (5e-6 / 2.5e-5), which
    therefore stay the dual tests' 2e-5 and 1e-4."""
    T, B = 50, 256
    worst = dict(z=0.0, J=0.0, g0=0.0, gth=0.0)
    for N in R.NS:
        z0, th = R.inputs(B, N, seed=T)
        _floor(z0, th, R.grid(T), R.cotangent(T, B, N), worst, [(s, dt) for s in (R.TSIT5, R.RK4) for dt in R.DTS])
    print("f32 against f64 floors: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["z"] <= Z_BOUND / 4 and max(worst["J"], worst["g0"], worst["gth"]) <= J_BOUND / 4, worst


def test_reference_f32_floor_of_phases_past_256_turns():
    """The same floor for the case of tests/test_gpu_kuramoto.py::test_phases_past_256_turns: φ₀ + 2π·300 ≈ 1 885, (T, B) = (5, 37), fixed
    steps of 0.05. There the number format sets the floor, not the summation order: between 1 024 and 2 048 an f32 phase is a multiple of
    2⁻¹³, so every stage's sine argument carries a rounding of up to 6.1e-5 rad — an error of that size in each sin(φ_j − φ_i), hence in
    every Jacobian entry and in the K column's forcing — while ẑ, relative to 1 885, does not notice. Measured, worst over N and the two
    solvers: ẑ 1.2e-7, J 3.4e-5, dz0 1.5e-5, dθ 1.9e-4. J and dθ do not fit a quarter of 1e-4, so by the project's rule their bounds in that
    test are 4 × the floor, rounded up: J 1.6e-4, dθ 8e-4; dz0 keeps 1e-4, ẑ 2e-5. (A sine that returns 0 past 256 turns moves J by 0.15
    to 0.22 of its largest entry on these inputs: a thousand times the bound.)"""
    T, B = 5, 37
    worst = dict(z=0.0, J=0.0, g0=0.0, gth=0.0)
    for N in R.NS:
        z0, th = R.turn_inputs(B, N)
        _floor(z0, th, R.grid(T), R.cotangent(T, B, N), worst, [(R.TSIT5, 0.05), (R.RK4, 0.05)])
    print("f32 against f64 floors past 256 turns: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["z"] <= Z_BOUND / 4 and worst["g0"] <= TURN_G0_BOUND / 4, worst
    assert worst["J"] <= TURN_J_BOUND / 4 and worst["gth"] <= TURN_GTH_BOUND / 4, worst
    # … and what the test is there to catch is far above the bounds: the uncoupled solve (a sine that returns 0 out there) against the real one
    N = 3
    z0, th = R.turn_inputs(B, N)
    th0 = th.copy()
    th0[:, N] = 0
    Jr = R.solve(z0, th, R.grid(T), adaptive=False, dt=0.05)[1]
    J0 = R.solve(z0, th0, R.grid(T), adaptive=False, dt=0.05)[1]
    assert np.abs(J0[..., :2 * N] - Jr[..., :2 * N]).max() / np.abs(Jr).max() >= 100 * TURN_J_BOUND


def test_first_step_seed_meets_the_share_between_the_two_modes():
    """The seed of tests/test_gpu_kuramoto.py's adaptive tests: with it the f32 mode's first accepted step equals the f64 mode's (to 1e-4
    relative) for every one of the 37 trajectories, at every N. Reached: 100 % (largest relative difference 1.2e-6)."""
    B, T = 37, 50
    for N in R.NS:
        z0, th = R.inputs(B, N, seed=FIRST_STEP_SEED)
        d64 = np.array([d[0] for d in R.solve(z0, th, R.grid(T))[3]["dt"]])
        d32 = np.array([d[0] for d in R.solve(z0, th, R.grid(T), dtype=np.float32)[3]["dt"]])
        share = (np.abs(d32 - d64) <= 1e-4 * d64).mean()
        print(f"N = {N}: first accepted step, f32 against f64: share {share:.4f}, largest relative difference {np.abs(d32 / d64 - 1).max():.2e}")
        assert share == 1.0, (N, share)


def test_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "kuramoto_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "kuramoto_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "kuramoto host logic under ASan + UBSan" in r.stdout
