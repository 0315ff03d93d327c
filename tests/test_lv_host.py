"""CPU: the Lotka–Volterra right-hand side (LDE_RHS_LOTKA_VOLTERRA, include/lde.h) without a GPU — (1) which descriptions the built library
serves and which it refuses, with what status and text; (2) the numpy restatement the GPU tests compare against (tests/lv_ref.py) pinned
before it is trusted: its J against central differences of its own values, the closed form at β = δ = 0, the conserved quantity, its f32
mode against its f64 mode (the floor under the GPU bounds) and the seed of the first-step test; (3) csrc/lde_host.h's part — validate(),
the dual record over NP partials per component, the kernels' dispatch — under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/lv_host_driver.cpp, run as a program)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the bounds of tests/test_gpu_lv.py (the pendulum dual tests'), relative to the largest entry of the reference array
Z_BOUND, J_BOUND = 2e-5, 1e-4
FIRST_STEP_SEED = 50        # tests/test_gpu_lv.py: the inputs of the first-step test


def _desc(**kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    base = dict(rhs_kind=L.RHS_LOTKA_VOLTERRA, param_dim=4, sensealg=L.SENSE_FORWARD_DUAL)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return lib, d


def test_served_and_refused_descriptions_through_the_c_abi():
    from latentdiffeq_amd import _lib as L
    assert L.RHS_LOTKA_VOLTERRA == 5
    for kw in (dict(), dict(adaptive=0, dt=0.05), dict(solver=L.SOLVER_RK4, adaptive=0, dt=0.0125), dict(dt=0.01)):
        lib, d = _desc(**kw)
        assert lib.lde_desc_error(C.byref(d)) == b"", kw
        assert lib.lde_num_weights(C.byref(d)) == 0
        h = C.c_void_p()
        rc = lib.lde_create(C.byref(d), C.byref(h))
        assert rc in (0, -3), rc                           # LDE_OK with a GPU, LDE_ERR_NO_DEVICE without: never an argument error
        if rc == 0:
            lib.lde_destroy(h)
    refused = [
        (dict(param_dim=1), -1, "LDE_RHS_LOTKA_VOLTERRA needs state_dim=2, param_dim=4, augment_dim=0"),
        (dict(state_dim=3), -1, "state_dim=2, param_dim=4"),
        (dict(augment_dim=2), -1, "augment_dim=0"),
        (dict(n_layers=1), -1, "n_layers must be 0"),
        (dict(param_dim=1, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -1, "param_dim=4"),   # the dims come before the solver
        (dict(sensealg=L.SENSE_DISCRETE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_PARALLEL_CHECKPOINTED), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(batching=L.BATCH_COUPLED), -2, "LDE_BATCH_PER_TRAJECTORY only"),
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


def test_python_plug_in_sizes_the_default_layers():
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    lv = la.LotkaVolterra()
    assert isinstance(lv.solver, la.Tsit5) and lv.sensealg.code == L.SENSE_FORWARD_DUAL and lv._rhs_kind == 5
    assert len(lv.prob.u0) == 2 and len(lv.prob.p) == 4
    assert la.LotkaVolterra(sensalg=la.BacksolveAdjoint()).sensealg.code == L.SENSE_BACKSOLVE_CHECKPOINTED   # (refused at the first solve)
    assert la.LotkaVolterra(solver=la.RK4(), adaptive=False, dt=0.05).kwargs == dict(adaptive=False, dt=0.05)
    from latentdiffeq_amd import train as TR
    _, dec = TR.default_layers(la.GOKU_basic(), 784, lv)
    lo_z0, lo_th = dec[0]
    assert tuple(lo_th.sizes) == (16, 200, 4) and tuple(lo_z0.sizes) == (16, 200, 2)
    assert lo_th.acts[-1] == L.CACT_SOFTPLUS and dec[1] is lv


@pytest.mark.parametrize("mode", ["tsit5-fixed", "rk4-fixed", "tsit5-steps"])
def test_reference_partials_are_the_central_differences_of_its_values(mode):
    """x₀, y₀, α, β, γ, δ perturbed on FIXED steps (a fixed dt, or the accepted steps of the unperturbed adaptive solve replayed): central
    differences in f64 against the carried partials, to 1e-6 of each partial's largest entry."""
    B, T = 16, 20
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=4))
    ts = R.grid(T)
    if mode == "tsit5-steps":
        _, _, ret, info = R.solve(z0, th, ts)
        assert (ret == 0).all()
        kw = dict(steps=(info["t"], info["dt"]))
    else:
        kw = dict(solver=R.TSIT5 if mode == "tsit5-fixed" else R.RK4, adaptive=False, dt=0.03)      # (0.03: save times inside the steps)
    _, J, ret, _ = R.solve(z0, th, ts, **kw)
    assert (ret == 0).all()
    eps = 1e-6
    for q in range(6):
        dz0, dth = np.zeros_like(z0), np.zeros_like(th)
        if q < 2:
            dz0[:, q] = eps
        else:
            dth[:, q - 2] = eps
        zp = R.solve(z0 + dz0, th + dth, ts, **kw)[0]
        zm = R.solve(z0 - dz0, th - dth, ts, **kw)[0]
        fd = (zp - zm) / (2 * eps)
        err = np.abs(fd - J[..., q]).max() / np.abs(J[..., q]).max()
        print(f"{mode} partial {q}: {err:.2e}")
        assert err <= 1e-6, (q, err)


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_reference_reproduces_the_closed_form_without_interaction(solver):
    """β = δ = 0: x = x₀e^{αt}, y = y₀e^{−γt}; ∂x/∂x₀ = e^{αt}, ∂x/∂α = t·x, ∂y/∂y₀ = e^{−γt}, ∂y/∂γ = −t·y, every other partial zero — the
    β and δ columns are NOT zero (∂x/∂β = −∫…), so they are checked against their own closed forms: ∂x/∂β = −x·y₀(1 − e^{−γt})/γ,
    ∂y/∂δ = y·x₀(e^{αt} − 1)/α."""
    B, T = 8, 20
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=6))
    th[:, 1] = th[:, 3] = 0.0
    ts = R.grid(T)
    kw = dict(abstol=1e-10, reltol=1e-10) if solver == R.TSIT5 else dict(adaptive=False, dt=0.0025)
    z, J, ret, _ = R.solve(z0, th, ts, solver, **kw)
    assert (ret == 0).all()
    x0, y0, al, ga = z0[:, 0], z0[:, 1], th[:, 0], th[:, 2]

    def closed(t):
        t = t[:, None]
        x, y = x0 * np.exp(al * t), y0 * np.exp(-ga * t)
        Jc = np.zeros((T, B, 2, 6))
        Jc[:, :, 0, 0], Jc[:, :, 0, 2], Jc[:, :, 0, 3] = np.exp(al * t), t * x, -x * y0 * (1 - np.exp(-ga * t)) / ga
        Jc[:, :, 1, 1], Jc[:, :, 1, 4], Jc[:, :, 1, 5] = np.exp(-ga * t), -t * y, y * x0 * (np.exp(al * t) - 1) / al
        return np.stack([x, y], axis=-1), Jc

    zc, Jc = closed(ts)
    # the state advances by (float)dt while t advances by dt (include/lde.h): the solve sees a time that is off by up to 2⁻²⁴ relative —
    # the bound is what that moves the closed form by, plus 1e-9 for the solve itself
    zs, Js = closed(ts * (1 + 2.0 ** -24))
    tz, tJ = np.abs(zs - zc).max() + 1e-9, np.abs(Js - Jc).max() + 1e-9
    ez, eJ = np.abs(z - zc).max(), np.abs(J - Jc).max()
    print(f"solver {solver}: |z - closed form| {ez:.2e} (bound {tz:.2e}), |J - closed form| {eJ:.2e} (bound {tJ:.2e})")
    assert ez <= tz and eJ <= tJ, (ez, tz, eJ, tJ)


def test_reference_conserves_the_invariant():
    """V = δx − γ ln x + βy − α ln y along the solve at abstol = reltol = 1e-9: constant to 1e-7 of |V| (a hundred times the tolerance; the
    error estimate is per step and the dual norm's partials only tighten it)."""
    B, T = 32, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(B, seed=7))
    z, _, ret, _ = R.solve(z0, th, R.grid(T), abstol=1e-9, reltol=1e-9)
    V = R.invariant(z, th)
    drift = np.abs(V - V[0]).max() / np.abs(V[0]).min()
    print(f"invariant drift {drift:.2e}")
    assert (ret == 0).all() and drift <= 1e-7, drift


def test_reference_f32_floor_under_the_gpu_bounds():
    """The f32 restatement against the f64 one on the (50, 256) parity cases of tests/test_gpu_lv.py, relative to the largest entry: the floor
    under its bounds. Measured: ẑ 5.0e-7, J 5.9e-7, dz0 8.7e-7, dθ 5.7e-7 — all below a quarter of the bounds (5e-6 / 2.5e-5), which therefore
    stay the pendulum dual tests' 2e-5 and 1e-4."""
    T, B = 50, 256
    ts, dz = R.grid(T), R.cotangent(T, B)
    z0, th = R.inputs(B, seed=T)
    worst = dict(z=0.0, J=0.0, g0=0.0, gth=0.0)
    for solver in (R.TSIT5, R.RK4):
        for dt in R.DTS:
            z64, J64, _, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=dt)
            z32, J32, _, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=dt, dtype=np.float32)
            assert z32.dtype == np.float32
            g64, g32 = R.pullback(J64, dz), R.pullback(J32, dz)
            for key, a, b in (("z", z32, z64), ("J", J32, J64), ("g0", g32[0], g64[0]), ("gth", g32[1], g64[1])):
                worst[key] = max(worst[key], np.abs(a - b).max() / np.abs(b).max())
    print("f32 against f64 floors: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["z"] <= Z_BOUND / 4 and max(worst["J"], worst["g0"], worst["gth"]) <= J_BOUND / 4, worst


def test_first_step_seed_meets_the_share_between_the_two_modes():
    """The seed of tests/test_gpu_lv.py's first-step test: with it the f32 mode's first accepted step equals the f64 mode's (to 1e-4 relative)
    for at least 99 % of the 256 trajectories. Reached: 100 % (largest relative difference 1.2e-6)."""
    B, T = 256, 50
    z0, th = R.inputs(B, seed=FIRST_STEP_SEED)
    d64 = np.array([d[0] for d in R.solve(z0, th, R.grid(T))[3]["dt"]])
    d32 = np.array([d[0] for d in R.solve(z0, th, R.grid(T), dtype=np.float32)[3]["dt"]])
    share = (np.abs(d32 - d64) <= 1e-4 * d64).mean()
    print(f"first accepted step, f32 against f64: share {share:.4f}, largest relative difference {np.abs(d32 / d64 - 1).max():.2e}")
    assert share >= 0.99, share


def test_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "lv_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "lv_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "lotka-volterra host logic under ASan + UBSan" in r.stdout
