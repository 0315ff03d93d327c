"""CPU: the stochastic pendulum (LDE_RHS_SPENDULUM, include/lde.h) without a GPU — (1) which descriptions the built library serves and
which it refuses, with what text; (2) the numpy restatement the GPU tests compare against (tests/sde_ref.py): its partials against central
finite differences of its own values, its f32 mode against its f64 mode; (3) the statistics of the noise as the header defines it; (4) the
substep plan of csrc/lde_host.h under AddressSanitizer + UndefinedBehaviorSanitizer (tests/sde_host_driver.cpp, run as a program)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sde_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    base = dict(rhs_kind=L.RHS_SPENDULUM, solver=L.SOLVER_EULER_HEUN, sensealg=L.SENSE_FORWARD_DUAL, adaptive=0, dt=0.05)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return lib, d


def test_served_and_unserved_descriptions():
    from latentdiffeq_amd import _lib as L
    h = C.c_void_p()
    for solver in (L.SOLVER_EM, L.SOLVER_EULER_HEUN):
        for dt in (0.05, 0.0125, 1e-30, 7.0):
            lib, d = _desc(solver=solver, dt=dt)
            assert lib.lde_desc_error(C.byref(d)) == b""
            rc = lib.lde_create(C.byref(d), C.byref(h))
            assert rc in (0, -3), rc                       # LDE_OK with a GPU, LDE_ERR_NO_DEVICE without: never an argument error
            if rc == 0:
                lib.lde_destroy(h)
    unserved = [
        (dict(adaptive=1), "adaptive"),
        (dict(dt=0.0), "dt"),
        (dict(batching=L.BATCH_COUPLED), "LDE_BATCH_PER_TRAJECTORY"),
        (dict(sensealg=L.SENSE_DISCRETE), "use LDE_SENSE_FORWARD_DUAL"),
        (dict(rhs_kind=L.RHS_PENDULUM, solver=L.SOLVER_EM), "LDE_RHS_SPENDULUM"),
        (dict(solver=L.SOLVER_TSIT5), "LDE_SOLVER_EM"),
    ]
    for kw, needle in unserved:
        lib, d = _desc(**kw)
        h = C.c_void_p()
        assert lib.lde_create(C.byref(d), C.byref(h)) == -2 and not h.value, kw      # LDE_ERR_UNSUPPORTED
        assert needle in lib.lde_desc_error(C.byref(d)).decode(), (kw, lib.lde_desc_error(C.byref(d)))
    # the feature is additive: the struct and its defaults are what they were
    lib, _ = _desc()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    assert C.sizeof(d) == 4 * 18 + 8 + 9 * 8
    assert (d.abi_version, d.rhs_kind, d.state_dim, d.param_dim, d.augment_dim, d.n_layers) == (1, 0, 2, 1, 0, 0)
    assert (d.solver, d.batching, d.sensealg, d.activation, d.adaptive, d.maxiters, d.dt) == (0, 0, 3, 0, 1, 100000, 0.0)
    assert (d.abstol, d.reltol, d.dtmin, d.qmin, d.qmax, d.gamma, d.beta1, d.beta2) == (1e-6, 1e-3, 0.0, 0.2, 10.0, 0.9, 7.0 / 50.0, 2.0 / 25.0)
    assert lib.lde_set_noise(None, 0, 0, 0, None) == -1
    # the Python mirror: EulerHeun at dt = 0.05, any ForwardDiffSensitivity = the dual-number solve, the offset moves with every forward
    import latentdiffeq_amd as la
    sp = la.SPendulum()
    assert isinstance(sp.solver, la.EulerHeun) and isinstance(sp.sensealg, la.ForwardDiffSensitivity)
    assert (la.EM.code, la.EulerHeun.code) == (2, 3) and sp.kwargs["dt"] == 0.05 and sp.kwargs["adaptive"] is False
    assert [sp._next_noise()[:3] for _ in range(2)] == [(0, 0, 0), (0, 1, 0)]
    sp.reseed(9)
    assert sp._next_noise()[:3] == (9, 0, 0)
    assert len(sp.prob.u0) == 2 and len(sp.prob.p) == 1


@pytest.mark.parametrize("solver", [S.EM, S.EULER_HEUN])
def test_reference_partials_are_the_finite_differences_of_its_values(solver):
    """x₀, v₀ and L perturbed with the noise held fixed (same seed and offset): central differences in f64 against the carried partials, to
    1e-6 of each partial's largest entry."""
    B, T, dt = 64, 50, 0.05
    z0, L = S.inputs(B, seed=4)
    z0, L = z0.astype(np.float64), L.astype(np.float64)
    ts = 0.05 * np.arange(T)
    kw = dict(dt=dt, solver=solver, seed=7, offset=3)
    _, J, _ = S.solve(z0, L, ts, **kw)
    eps = 1e-5
    for q in range(3):
        dz0, dL = np.zeros_like(z0), np.zeros_like(L)
        if q < 2:
            dz0[:, q] = eps
        else:
            dL[:] = eps
        zp, _, _ = S.solve(z0 + dz0, L + dL, ts, **kw)
        zm, _, _ = S.solve(z0 - dz0, L - dL, ts, **kw)
        fd = (zp - zm) / (2 * eps)
        err = np.abs(fd - J[..., q]).max() / np.abs(J[..., q]).max()
        print(f"solver {solver} partial {q}: {err:.2e}")
        assert err <= 1e-6, (q, err)


def test_reference_f32_mode_stays_close_to_f64():
    """The f32 restatement on the GPU parity cases: within 2e-5 of f64 (measured: 4.7e-6 at worst, T = 50, B = 256)."""
    worst = 0.0
    cases = [(0.05 * np.arange(T), B, dt) for T, B in S.SHAPES for dt in S.DTS] + [(S.ragged_grid(), 256, 0.05)]
    for ts, B, dt in cases:
        z0, L = S.inputs(B, seed=len(ts))
        for solver in (S.EM, S.EULER_HEUN):
            z64, _, _ = S.solve(z0, L, ts, dt, solver, seed=5)
            z32, _, _ = S.solve(z0, L, ts, dt, solver, seed=5, dtype=np.float32)
            assert z32.dtype == np.float32
            worst = max(worst, np.abs(z32 - z64).max())
    print(f"f32 against f64: {worst:.2e}")
    assert worst <= 2e-5, worst


STAT, noise_statistics = S.STAT, S.noise_statistics


@pytest.mark.parametrize("solver", [S.EM, S.EULER_HEUN])
def test_noise_statistics_of_the_definition(solver):
    """L = 1e30: the drift in v vanishes and v(T) − v₀ = Σ ΔW_v ~ N(0, σ²·t_end)."""
    B = STAT["B"]
    z0 = np.zeros((B, 2))
    z0[:, 1] = STAT["v0"]
    z, _, ret = S.solve(z0, np.full(B, STAT["L"]), STAT["ts"], STAT["dt"], solver, seed=STAT["seed"])
    m, v = noise_statistics(z[-1, :, 1], STAT["v0"], STAT["ts"][-1], B)
    print(f"solver {solver}: mean {m:+.2f} standard errors, variance {v:+.2f} units of sqrt(2/B)")
    assert (ret == 0).all() and abs(m) <= 4 and abs(v) <= 4, (m, v)


def test_substep_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "sde_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "sde_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "sde substep plan under ASan + UBSan" in r.stdout
    # the plan in numpy (what tests/sde_ref.py steps by) is the same rule
    assert [n for n, _ in S.plan([0.0, 0.01, 0.14, 0.22, 0.27, 0.3701], 0.05)] == [1, 3, 2, 1, 3]
    assert sum(n for n, _ in S.plan(0.05 * np.arange(50), 0.0125)) == 196
