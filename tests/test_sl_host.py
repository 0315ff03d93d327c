"""CPU: the Stuart–Landau network (LDE_RHS_STUART_LANDAU, include/lde.h) without a GPU — (1) which descriptions the built library serves and
which it refuses, with what status and text: the deterministic and the stochastic solves, every other kind still refusing the stochastic steppers
with its old text, rhs_kind = 6, 8, 10 and 12 still unknown; (2) the numpy restatement the GPU tests compare against (tests/sl_ref.py) pinned
before it is trusted: its right-hand side and Jacobian against the form of include/lde.h, its J against central differences of its own values,
its stochastic partials against central differences with the noise held fixed, the closed form of the uncoupled radius, RK4's order, its noise
against the definition, and its f32 mode against its f64 mode on every GPU case's own inputs (the floor under the GPU bounds); (3) the Python
plug-in: its fields and the head widths default_layers builds from it; (4) csrc/lde_host.h's part under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/sl_host_driver.cpp, run as a program).

Every test here that creates a description of rhs_kind = 13 (or asks for la.StuartLandau) fails before this right-hand side existed, where
lde_create returns LDE_ERR_INVALID_ARG ("unknown rhs_kind")."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import philox_ref as P
from tests import sde_ref
from tests import sl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_TEXT = "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"


def _desc(N=2, **kw):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    base = dict(rhs_kind=L.RHS_STUART_LANDAU, state_dim=2 * N, param_dim=2 * N + 1, sensealg=L.SENSE_FORWARD_DUAL)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return lib, d


@pytest.mark.parametrize("N", R.NS)
def test_served_and_refused_descriptions_through_the_c_abi(N):
    from latentdiffeq_amd import _lib as L
    assert L.RHS_STUART_LANDAU == 13 and L.RHS_CVS == 11 and L.RHS_DOUBLE_PENDULUM == 9 and L.RHS_KURAMOTO == 7 and L.RHS_LOTKA_VOLTERRA == 5
    assert L.load().lde_abi_version() == 1                 # lde_problem_desc did not change
    served = (dict(), dict(adaptive=0, dt=0.05), dict(solver=L.SOLVER_RK4, adaptive=0, dt=0.0125), dict(dt=0.01),
              dict(solver=L.SOLVER_EM, adaptive=0, dt=0.05), dict(solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.0125))
    for kw in served:
        lib, d = _desc(N, **kw)
        assert lib.lde_desc_error(C.byref(d)) == b"", kw
        assert lib.lde_num_weights(C.byref(d)) == 0
        h = C.c_void_p()
        rc = lib.lde_create(C.byref(d), C.byref(h))
        assert rc in (0, -3), rc                           # LDE_OK with a GPU, LDE_ERR_NO_DEVICE without: never an argument error
        if rc == 0:
            _noise_sigma_rules(lib, h)
            lib.lde_destroy(h)
    dims = "LDE_RHS_STUART_LANDAU needs state_dim=2N with 1 <= N <= 3, param_dim=2N+1, augment_dim=0"
    refused = [
        (dict(state_dim=3, param_dim=4), -1, dims),
        (dict(state_dim=8, param_dim=9), -1, dims),
        (dict(param_dim=2 * N), -1, dims),
        (dict(param_dim=2 * N + 2), -1, dims),
        (dict(augment_dim=2), -1, dims),
        (dict(n_layers=1), -1, "LDE_RHS_STUART_LANDAU is analytic: n_layers must be 0"),
        (dict(rhs_kind=6), -1, "unknown rhs_kind"),                                        # 6, 8, 10 and 12 are still no right-hand sides
        (dict(rhs_kind=8), -1, "unknown rhs_kind"),
        (dict(rhs_kind=10), -1, "unknown rhs_kind"),
        (dict(rhs_kind=12), -1, "unknown rhs_kind"),
        (dict(rhs_kind=-1), -1, "unknown rhs_kind"),
        (dict(param_dim=1, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -1, dims),    # the dims come before the solver
        (dict(sensealg=L.SENSE_DISCRETE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_PARALLEL_CHECKPOINTED), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(sensealg=L.SENSE_BACKSOLVE_CHECKPOINTED), -2, "LDE_RHS_STUART_LANDAU: only the solve on dual numbers exists"),
        (dict(sensealg=L.SENSE_DISCRETE, solver=L.SOLVER_EM, adaptive=0, dt=0.05), -2, "use LDE_SENSE_FORWARD_DUAL"),
        (dict(batching=L.BATCH_COUPLED), -2, "LDE_RHS_STUART_LANDAU: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"),
        (dict(batching=L.BATCH_COUPLED, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05), -2, "LDE_RHS_STUART_LANDAU: no coupled solve"),
        (dict(solver=L.SOLVER_RK4), -2, "RK4 is fixed-step only"),
        (dict(solver=L.SOLVER_EM), -2, "LDE_RHS_STUART_LANDAU: no adaptive stochastic stepping"),          # adaptive = 1, the default
        (dict(solver=L.SOLVER_EULER_HEUN, adaptive=1, dt=0.05), -2, "LDE_RHS_STUART_LANDAU: no adaptive stochastic stepping"),
        (dict(solver=L.SOLVER_EM, adaptive=0, dt=0.0), -2, "pass a finite dt > 0"),
        (dict(solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=float("inf")), -2, "pass a finite dt > 0"),
        (dict(solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=float("nan")), -2, "pass a finite dt > 0"),
    ]
    for kw, status, needle in refused:
        lib, d = _desc(N, **kw)
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


def _noise_sigma_rules(lib, h):
    """(with a device only) "noise_sigma" on a handle of this kind: default 0.01, finite and ≥ 0; lde_set_noise is accepted."""
    v = C.c_double(-1.0)
    assert lib.lde_get_option(h, b"noise_sigma", C.byref(v)) == 0 and v.value == 0.01
    for ok in (0.0, 0.5, 1e-3):
        assert lib.lde_set_option(h, b"noise_sigma", C.c_double(ok)) == 0
        assert lib.lde_get_option(h, b"noise_sigma", C.byref(v)) == 0 and v.value == ok
    for bad in (-1e-9, float("inf"), float("-inf"), float("nan")):
        assert lib.lde_set_option(h, b"noise_sigma", C.c_double(bad)) == -1
        assert lib.lde_get_option(h, b"noise_sigma", C.byref(v)) == 0 and v.value == 1e-3
    assert lib.lde_set_noise(h, 1, 0, 0, None) == 0


def test_every_other_kind_still_refuses_the_stochastic_steppers_with_its_old_text():
    """… and "noise_sigma" / lde_set_noise on a handle of another kind keep today's status (with a device only)."""
    from latentdiffeq_amd import _lib as L
    others = [(L.RHS_PENDULUM, 2, 1, L.SENSE_DISCRETE), (L.RHS_PENDULUM_FRICTION, 2, 1, L.SENSE_DISCRETE), (L.RHS_LOTKA_VOLTERRA, 2, 4, L.SENSE_FORWARD_DUAL),
              (L.RHS_KURAMOTO, 3, 4, L.SENSE_FORWARD_DUAL), (L.RHS_DOUBLE_PENDULUM, 4, 4, L.SENSE_FORWARD_DUAL), (L.RHS_CVS, 4, 2, L.SENSE_FORWARD_DUAL)]
    for kind, D, Pn, sa in others:
        for solver in (L.SOLVER_EM, L.SOLVER_EULER_HEUN):
            lib, d = _desc(rhs_kind=kind, state_dim=D, param_dim=Pn, sensealg=sa, solver=solver, adaptive=0, dt=0.05)
            h = C.c_void_p()
            assert lib.lde_create(C.byref(d), C.byref(h)) == -2 and not h.value, kind
            assert lib.lde_desc_error(C.byref(d)).decode() == OLD_TEXT, kind
        lib, d = _desc(rhs_kind=kind, state_dim=D, param_dim=Pn, sensealg=sa)
        h = C.c_void_p()
        rc = lib.lde_create(C.byref(d), C.byref(h))
        assert rc in (0, -3), (kind, rc)
        if rc == 0:
            v = C.c_double(7.0)
            assert lib.lde_set_option(h, b"noise_sigma", C.c_double(0.02)) == -2 and lib.lde_get_option(h, b"noise_sigma", C.byref(v)) == -2
            assert lib.lde_set_noise(h, 1, 0, 0, None) == -2 and b"LDE_RHS_SPENDULUM only" in lib.lde_last_error(h)
            lib.lde_destroy(h)
    lib, d = _desc(rhs_kind=L.RHS_SPENDULUM, state_dim=2, param_dim=1, solver=L.SOLVER_EULER_HEUN, adaptive=0, dt=0.05)   # still served
    assert lib.lde_desc_error(C.byref(d)) == b""
    lib, d = _desc(rhs_kind=L.RHS_MLP, state_dim=2, param_dim=0, n_layers=1, solver=L.SOLVER_EM, adaptive=0, dt=0.05, sensealg=L.SENSE_DISCRETE)
    d.layer_sizes[0], d.layer_sizes[1] = 2, 2
    assert lib.lde_desc_error(C.byref(d)).decode() == OLD_TEXT


@pytest.mark.parametrize("N", R.NS)
def test_python_plug_in_fields_and_default_layers(N):
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    sl = la.StuartLandau(N)
    assert isinstance(sl.solver, la.Tsit5) and sl.sensealg.code == L.SENSE_FORWARD_DUAL and sl._rhs_kind == 13 and sl.N == N
    assert len(sl.prob.u0) == 2 * N and len(sl.prob.p) == 2 * N + 1 and sl.flat_weights() is None
    assert not sl.stochastic and sl._next_noise() is None and sl.offset == 0 and sl.kwargs == dict()
    assert la.StuartLandau().N == 2 and la.StuartLandau().sigma == 0.01
    assert la.StuartLandau(N, sensalg=la.BacksolveAdjoint()).sensealg.code == L.SENSE_BACKSOLVE_CHECKPOINTED   # (refused at the first solve)
    assert la.StuartLandau(N, solver=la.RK4(), adaptive=False, dt=0.05).kwargs == dict(adaptive=False, dt=0.05)
    st = la.StuartLandau(N, solver=la.EulerHeun(), sigma=0.02, dt=0.0125, seed=7)
    assert st.stochastic and st.kwargs == dict(adaptive=False, dt=0.0125) and st.sigma == 0.02 and st.first_trajectory == 0
    assert st._next_noise() == (7, 0, 0, None) and st._next_noise() == (7, 1, 0, None)        # the offset advances per forward call
    st.reseed(9)
    assert st._next_noise() == (9, 0, 0, None)
    assert la.StuartLandau(N, solver=la.EM()).stochastic and "theta_activation=\"identity\"" in la.StuartLandau.__doc__
    x = torch.linspace(-7.0, 7.0, 24, dtype=torch.float32).reshape(4, 2, 3)
    assert la.transform_after_diffeq(x, sl) is x                                   # the identity
    _, dec = TR.default_layers(la.GOKU_basic(), 784, sl, theta_activation="identity")
    lo_z0, lo_th = dec[0]
    assert tuple(lo_z0.sizes) == (16, 200, 2 * N) and tuple(lo_th.sizes) == (16, 200, 2 * N + 1) and dec[1] is sl
    assert lo_th.acts[-1] == L.CACT_IDENTITY
    _, dflt = TR.default_layers(la.GOKU_basic(), 784, sl)
    assert dflt[0][0].acts[-1] == L.CACT_IDENTITY and dflt[0][1].acts[-1] == L.CACT_SOFTPLUS   # (the default: not the head for this system)


def _seeded(N, B):
    D, _, NP = R.dims(N)
    u = np.zeros((B, D + D * NP))
    for i in range(D):
        u[:, D + NP * i + i] = 1
    return u


@pytest.mark.parametrize("N", R.NS)
def test_reference_right_hand_side_is_the_stated_form(N):
    """The reference evaluates the system in mean-field form on arrays; include/lde.h states it oscillator by oscillator, and its Jacobian and
    forcing columns entry by entry: the same numbers to rounding, on the inputs' ranges and well outside them — and against central
    differences of `rhs_plain`, to 1e-7."""
    D, Pn, NP = R.dims(N)
    rng = np.random.default_rng(2)
    for scale in (1.0, 3.0):
        B = 50
        z = rng.uniform(-scale, scale, (B, D))
        th = np.concatenate([rng.uniform(-2, 2, (B, N)), rng.uniform(-3, 3, (B, N)), rng.uniform(0, 2, (B, 1))], axis=1)
        u = _seeded(N, B)
        u[:, :D] = z
        du = R.system(N).rhs(u, th)
        want = R.rhs_plain(z, th)
        assert np.abs(du[:, :D] - want).max() <= 1e-13 * np.abs(want).max()
        for b in range(B):
            Jz, Jt = R.jacobian_plain(z[b], th[b])
            Jw = np.concatenate([Jz, Jt], axis=1)
            assert np.abs(du[b, D:].reshape(D, NP) - Jw).max() <= 1e-13 * max(np.abs(Jw).max(), 1.0)
        eps = 1e-6
        for q in range(NP):
            dz, dth = np.zeros_like(z), np.zeros_like(th)
            if q < D:
                dz[:, q] = eps
            else:
                dth[:, q - D] = eps
            fd = (R.rhs_plain(z + dz, th + dth) - R.rhs_plain(z - dz, th - dth)) / (2 * eps)
            got = du[:, D:].reshape(B, D, NP)[:, :, q]
            assert np.abs(fd - got).max() <= 1e-7 * max(np.abs(got).max(), 1.0), (q, np.abs(fd - got).max())


@pytest.mark.parametrize("mode", ["tsit5-fixed", "rk4-fixed", "tsit5-steps"])
@pytest.mark.parametrize("N", R.NS)
def test_reference_partials_are_the_central_differences_of_its_values(N, mode):
    """ẑ₀, a, ω, G perturbed on FIXED steps (a fixed dt, or the accepted steps of the unperturbed adaptive solve replayed): central differences
    in f64 against the carried partials, to 1e-6 of J's largest entry (measured: at most 1.4e-10)."""
    D, Pn, NP = R.dims(N)
    B, T, eps = 6, 20, 1e-5
    z0, th = (a.astype(np.float64) for a in R.inputs(N, B, seed=4))
    ts = R.grid(T)
    if mode == "tsit5-steps":
        _, _, ret, info = R.solve(N, z0, th, ts)
        assert (ret == 0).all()
        kw = dict(steps=(info["t"], info["dt"]))
    else:
        kw = dict(solver=R.TSIT5 if mode == "tsit5-fixed" else R.RK4, adaptive=False, dt=0.13)      # (0.13: save times inside the steps)
    _, J, ret, _ = R.solve(N, z0, th, ts, **kw)
    assert (ret == 0).all() and J.shape == (T, B, D, NP)
    worst = 0.0
    for q in range(NP):
        dz0, dth = np.zeros_like(z0), np.zeros_like(th)
        if q < D:
            dz0[:, q] = eps
        else:
            dth[:, q - D] = eps
        zp = R.solve(N, z0 + dz0, th + dth, ts, **kw)[0]
        zm = R.solve(N, z0 - dz0, th - dth, ts, **kw)[0]
        err = np.abs((zp - zm) / (2 * eps) - J[..., q]).max() / np.abs(J).max()
        worst = max(worst, err)
        assert err <= 1e-6, (q, err)
        assert np.abs(J[..., q]).max() > 1e-3 or (N == 1 and q == NP - 1), q   # (every direction moves something; N = 1 has no coupling: ∂/∂G = 0)
    if N == 1:
        assert (J[..., NP - 1] == 0).all()                                       # x̄ − x = 0 exactly for one oscillator
    print(f"N {N} {mode}: central differences within {worst:.2e} of J's largest entry")


@pytest.mark.parametrize("solver", [R.EM, R.EULER_HEUN])
@pytest.mark.parametrize("N", R.NS)
def test_reference_stochastic_partials_are_central_differences_with_the_noise_held_fixed(N, solver):
    """The same check along a drawn path: the noise is a function of the counter alone, so perturbing ẑ₀ or θ leaves it where it is, and the
    carried partials are the derivative of the scheme along that path. The ragged grid: 1 to 3 unequal substeps per interval."""
    D, Pn, NP = R.dims(N)
    B, eps = 6, 1e-5
    z0, th = (a.astype(np.float64) for a in R.inputs(N, B, seed=4))
    ts = R.sde_ragged_grid()
    ns = [n for n, _ in R.plan(ts, 0.05)]
    assert min(ns) == 1 and max(ns) == 3
    kw = dict(dt=0.05, solver=solver, seed=11, offset=2, first=5, sigma=0.05)
    _, J, ret = R.sde_solve(N, z0, th, ts, **kw)
    assert (ret == 0).all()
    for q in range(NP):
        dz0, dth = np.zeros_like(z0), np.zeros_like(th)
        if q < D:
            dz0[:, q] = eps
        else:
            dth[:, q - D] = eps
        zp = R.sde_solve(N, z0 + dz0, th + dth, ts, **kw)[0]
        zm = R.sde_solve(N, z0 - dz0, th - dth, ts, **kw)[0]
        err = np.abs((zp - zm) / (2 * eps) - J[..., q]).max() / np.abs(J).max()
        assert err <= 1e-6, (q, err)


def test_reference_follows_the_closed_form_of_the_uncoupled_radius():
    """N = 1 (no coupling), a < 0: r' = (a − r²)·r has r² = a / (1 − (1 − a/r₀²)·e^(−2at)), and the phase turns at ω. The adaptive solve at
    1e-10 / 1e-8 against it to 1e-7, the default tolerances to 1e-3 (measured: radius 2.9e-9 and 1.4e-5, phase 1.8e-8 and 9.5e-5)."""
    B, T = 8, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(1, B, seed=6))
    th[:, 0] = -np.linspace(0.05, 0.5, B)
    ts = R.grid(T)
    r0 = np.hypot(z0[:, 0], z0[:, 1])
    want = R.radius_closed_form(th[None, :, 0], r0[None, :], ts[:, None])
    phase0 = np.arctan2(z0[:, 1], z0[:, 0])
    for tol, bound in ((dict(abstol=1e-10, reltol=1e-8), 1e-7), (dict(), 1e-3)):
        z, _, ret, _ = R.solve(1, z0, th, ts, **tol)
        assert (ret == 0).all()
        r = np.hypot(z[..., 0], z[..., 1])
        err = np.abs(r - want).max()
        ph = np.angle(np.exp(1j * (np.arctan2(z[..., 1], z[..., 0]) - phase0[None] - th[None, :, 1] * ts[:, None])))
        print(f"tolerances {tol}: radius within {err:.2e}, phase within {np.abs(ph).max():.2e}")
        assert err <= bound and np.abs(ph).max() <= bound
    assert (want[-1] < want[0]).all()                                              # a < 0: the radius decays


def test_reference_rk4_error_falls_with_the_fourth_power_of_the_step():
    """RK4's global error at t = 2.45 against a fine solve (dt = 1/256) falls about 16× per halving of dt, from dt = 0.2 to 0.1 to 0.05 (N = 3):
    at least 12× and less than 24× (all steps taken as their f32 values in both solves). Measured: 3.66e-3, 2.32e-4, 1.46e-5 — ratios 15.8 and 15.9."""
    N, B, T = 3, 8, 50
    z0, th = (a.astype(np.float64) for a in R.inputs(N, B, seed=8))
    ts = R.grid(T)
    fine = R.solve(N, z0, th, ts, R.RK4, adaptive=False, dt=1.0 / 256)[0]
    err = []
    for dt in (0.2, 0.1, 0.05):
        z, _, ret, _ = R.solve(N, z0, th, ts, R.RK4, adaptive=False, dt=dt)
        assert (ret == 0).all()
        err.append(np.abs(z[-1] - fine[-1]).max())
    print(f"RK4 global error at dt = 0.2, 0.1, 0.05: {err[0]:.2e}, {err[1]:.2e}, {err[2]:.2e}: ratios {err[0] / err[1]:.1f}, {err[1] / err[2]:.1f}")
    assert 12 <= err[0] / err[1] < 24 and 12 <= err[1] / err[2] < 24, err


def _floor(N, dz, f64, f32):
    (z64, J64), (z32, J32) = f64[:2], f32[:2]
    assert z32.dtype == np.float32 and J32.dtype == np.float32 and (f64[2] == 0).all() and (f32[2] == 0).all()
    assert np.isfinite(z64).all() and np.isfinite(J64).all() and np.isfinite(z32).all() and np.isfinite(J32).all()
    g64, g32 = R.pullback(N, J64, dz), R.pullback(N, J32, dz)
    return tuple(np.abs(a - b).max() / np.abs(b).max() for a, b in ((z32, z64), (J32, J64), (g32[0], g64[0]), (g32[1], g64[1])))


def _within_a_quarter(tag, floor, bounds):
    print(f"f32 against f64 floor, {tag}: z {floor[0]:.2e}, J {floor[1]:.2e}, dz0 {floor[2]:.2e}, dtheta {floor[3]:.2e}; bounds {bounds}")
    for f, b in zip(floor, bounds):
        assert f <= b / 4, (tag, floor, bounds)


@pytest.mark.parametrize("T,B", R.SHAPES[1:])
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
@pytest.mark.parametrize("N", R.NS)
def test_reference_f32_floor_under_the_gpu_bounds(N, solver, dt, T, B):
    """The f32 restatement against the f64 one on tests/test_gpu_sl.py's own fixed-step inputs, relative to the largest entry: the floor under
    the GPU bounds, within a quarter of them. Measured, the worst of all cases (ẑ / J / dz0 / dθ): Tsit5 7.4e-7 / 8.2e-7 / 6.5e-7 / 6.8e-7, RK4
    5.3e-7 / 6.2e-7 / 7.7e-7 / 4.7e-7 — the standing 2e-5 and 1e-4 stand everywhere."""
    z0, th = R.inputs(N, B, seed=R.PARITY_SEED[T])
    ts, dz = R.grid(T), R.cotangent(N, T, B)
    floor = _floor(N, dz, R.solve(N, z0, th, ts, solver, adaptive=False, dt=dt), R.solve(N, z0, th, ts, solver, adaptive=False, dt=dt, dtype=np.float32))
    _within_a_quarter(f"N {N} solver {solver} dt {dt} ({T}, {B})", floor, R.bounds(solver, dt, T))


@pytest.mark.parametrize("grid,B,dt", [(T, B, dt) for T, B in R.SHAPES[1:] for dt in R.DTS] + [("ragged", 256, 0.05)])
@pytest.mark.parametrize("solver", [R.EM, R.EULER_HEUN])
@pytest.mark.parametrize("N", R.NS)
def test_reference_stochastic_f32_floor_under_the_gpu_bounds(N, solver, grid, B, dt):
    """The same for tests/test_gpu_sl_sde.py's parity cases, along the drawn path (the noise itself is formed in the working precision).
    Measured, the worst of all cases: EM 6.1e-7 / 7.0e-7 / 5.1e-7 / 3.8e-7, EulerHeun 6.8e-7 / 8.6e-7 / 3.0e-7 / 2.7e-7 — the standing bounds
    stand for the stochastic solve too."""
    ts = R.sde_ragged_grid() if grid == "ragged" else R.grid(grid)
    z0, th = R.inputs(N, B, seed=R.SDE_RAGGED_SEED if grid == "ragged" else R.PARITY_SEED[grid])
    dz = R.cotangent(N, len(ts), B)
    kw = dict(dt=dt, solver=solver, seed=R.NOISE_SEED)
    floor = _floor(N, dz, R.sde_solve(N, z0, th, ts, **kw), R.sde_solve(N, z0, th, ts, dtype=np.float32, **kw))
    _within_a_quarter(f"N {N} solver {solver} grid {grid} dt {dt} B {B}", floor, R.BOUNDS)


@pytest.mark.parametrize("N", R.NS)
def test_reference_f32_floor_of_the_adaptive_case(N):
    """The inputs of the GPU test of the adaptive solve, (50, 37) at 1e-6 / 1e-3: the reference's own accepted steps replayed in both modes,
    within a quarter of the standing bounds; 11.9 / 12.6 / 13.2 accepted steps per trajectory for N = 1 / 2 / 3, none rejected. And the first accepted step: the f32
    mode's equals the f64 mode's to 1e-4 for all 37 (measured 9.1e-7)."""
    T, B = R.ADAPTIVE_SHAPE
    z0, th = R.inputs(N, B, seed=R.ADAPTIVE_SEED)
    ts, dz = R.grid(T), R.cotangent(N, T, B)
    _, _, ret, info = R.solve(N, z0, th, ts)
    assert (ret == 0).all() and info["nreject"] == 0
    print(f"N {N}: accepted steps per trajectory {info['naccept'] / B:.1f}, rejected {info['nreject']}")
    kw = dict(steps=(info["t"], info["dt"]))
    _within_a_quarter(f"N {N} adaptive, own steps replayed", _floor(N, dz, R.solve(N, z0, th, ts, **kw), R.solve(N, z0, th, ts, dtype=np.float32, **kw)), R.BOUNDS)
    d64 = np.array([d[0] for d in info["dt"]])
    d32 = np.array([d[0] for d in R.solve(N, z0, th, ts, dtype=np.float32)[3]["dt"]])
    print(f"first accepted step, f32 against f64: largest relative difference {np.abs(d32 / d64 - 1).max():.2e}")
    assert (np.abs(d32 - d64) <= 1e-4 * d64).all()


@pytest.mark.parametrize("N", R.NS)
def test_reference_f32_floor_of_the_ragged_and_the_long_grid(N):
    """The inputs of the GPU tests on the ragged nine-point grid (B = 3, the reference's own steps replayed) and on T = 6001 save times (B = 3,
    Tsit5 at dt = 0.0125, t ≤ 6): both within a quarter of the standing bounds. On the reference's own steps every trajectory has a step with
    at least two save times and a step with none."""
    ts = R.ragged_grid()
    z0, th = R.inputs(N, 3, seed=R.RAGGED_SEED)
    _, _, ret, info = R.solve(N, z0, th, ts)
    assert (ret == 0).all()
    for b in range(3):
        per_step = np.histogram(ts[1:], bins=np.append(info["t"][b], ts[-1] + 1e-9))[0]
        assert per_step.max() >= 2 and (per_step == 0).sum() >= 1, per_step
    kw = dict(steps=(info["t"], info["dt"]))
    dz = R.cotangent(N, len(ts), 3)
    _within_a_quarter(f"N {N} ragged grid", _floor(N, dz, R.solve(N, z0, th, ts, **kw), R.solve(N, z0, th, ts, dtype=np.float32, **kw)), R.BOUNDS)
    T = 6001
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(N, 3, seed=R.LONG_SEED)
    dz = R.cotangent(N, T, 3)
    kw = dict(solver=R.TSIT5, adaptive=False, dt=0.0125)
    _within_a_quarter(f"N {N} T = 6001", _floor(N, dz, R.solve(N, z0, th, ts, **kw), R.solve(N, z0, th, ts, dtype=np.float32, **kw)), R.BOUNDS)


def test_noise_definition_components_and_blocks():
    """The counter layout of include/lde.h, restated with tests/philox_ref.py: for N = 1 the path's (ξ_x, ξ_y) are the stochastic pendulum's
    (ξ_x, ξ_v) (tests/sde_ref.py: xi) bit for bit; components 2 and 3 are the Box–Muller pair of words 2 and 3 of the same block; components 4
    and 5 that of words 0 and 1 of the block whose key has the top bit of its high word flipped — block 0 of seed xor 2⁶³ — and differ from
    block 0's."""
    B = 64
    for seed, off, first, s in ((0, 0, 0, 0), (5, 3, 17, 9), ((3 << 32) | 12345, (1 << 32) + 7, 1000, 195), ((1 << 63) | 77, 2, 5, 1)):
        x1 = R.xi(B, s, 2, seed, off, first)
        px, pv = sde_ref.xi(B, s, seed, off, first)
        assert np.array_equal(x1[:, 0], px) and np.array_equal(x1[:, 1], pv)
        x3 = R.xi(B, s, 6, seed, off, first)
        assert np.array_equal(x3[:, :2], x1) and np.array_equal(R.xi(B, s, 4, seed, off, first), x3[:, :4])
        b = (np.arange(B, dtype=np.uint64) + np.uint64(first)) & P.MASK
        w0 = P.philox4x32_10(b, s, off & 0xFFFFFFFF, off >> 32, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        w1 = P.philox4x32_10(b, s, off & 0xFFFFFFFF, off >> 32, seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ 0x80000000)
        for bb in range(0, B, 7):
            assert np.allclose(x3[bb, :4], P.normals([w0[i][bb] for i in range(4)]), rtol=0, atol=1e-12)
            assert np.allclose(x3[bb, 4:], P.normals([w1[0][bb], w1[1][bb]]), rtol=0, atol=1e-12)
        other = R.xi(B, s, 6, seed ^ (1 << 63), off, first)
        assert np.array_equal(other[:, :2], x3[:, 4:]), "block 1 of seed S is block 0 of seed S xor 2^63"
        assert np.abs(x3[:, 4:] - x3[:, :2]).min() > 0 and np.abs(x3[:, 4:] - x3[:, 2:4]).min() > 0, "block 1 differs from block 0"
    f32 = R.xi(B, 3, 6, 5, 0, 0, np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - R.xi(B, 3, 6, 5, 0, 0)).max() <= 2e-5


@pytest.mark.parametrize("N", R.NS)
def test_noise_definition_statistics(N):
    """(a) 2·10⁵ draws per component: mean, variance, and the correlations between components — those across the two blocks included — within
    4.5 standard errors. (b) The statistics case of tests/test_gpu_sl_sde.py on this reference: ẑ₀ = 0, θ = 0, B = 4096, 20 substeps; the
    drift is cubic in a state of size σ√t, so z(t_end) is the noise sum to 1e-3 relative, and the mean and variance of every component sit
    inside tests/test_gpu_sde.py's gates at R.STAT's seed, for both solvers."""
    D = 2 * N
    n = 200000
    x = np.concatenate([R.xi(20000, s, D, seed=3) for s in range(10)])
    se = 1.0 / np.sqrt(n)
    assert (np.abs(x.mean(axis=0)) <= 4.5 * se).all() and (np.abs(x.var(axis=0) - 1.0) <= 4.5 * np.sqrt(2.0) * se).all()
    c = np.corrcoef(x.T) - np.eye(D)
    assert np.abs(c).max() <= 4.5 * se, np.abs(c).max()
    B, ts = R.STAT["B"], R.STAT["ts"]
    sums = R.SIGMA * np.sqrt(np.float64(np.float32(0.05))) * sum(R.xi(B, s, D, seed=R.STAT["seed"]) for s in range(20))
    for solver in (R.EM, R.EULER_HEUN):
        z, _, ret = R.sde_solve(N, np.zeros((B, D)), np.zeros((B, D + 1)), ts, R.STAT["dt"], solver, seed=R.STAT["seed"])
        assert (ret == 0).all()
        assert np.abs(z[-1] - sums).max() <= 1e-3 * np.abs(sums).max()
        m, v = R.noise_statistics(z[-1], ts[-1], B)
        print(f"N {N} solver {solver}: means {np.round(m, 2)} standard errors, variances {np.round(v, 2)} units of sqrt(2/B)")
        assert (np.abs(m) <= 4).all() and (np.abs(v) <= 4).all(), (m, v)


def test_reference_departure_from_the_deterministic_scheme():
    """"The noise is there" (tests/test_gpu_sl_sde.py): on the (50, 256) parity inputs at dt = 0.05 every trajectory of this reference leaves the
    σ = 0 scheme by at least 7.9e-3 somewhere — N = 1, 2, 3 × both solvers × seeds 5 and 6 — and R.MIN_DEPARTURE is two thirds of that
    smallest departure, rounded down."""
    T, B = 50, 256
    smallest = np.inf
    for N in R.NS:
        z0, th = R.inputs(N, B, seed=R.PARITY_SEED[T])
        for solver in (R.EM, R.EULER_HEUN):
            zdet = R.sde_solve(N, z0, th, R.grid(T), 0.05, solver, sigma=0.0)[0]
            for seed in (R.NOISE_SEED, R.NOISE_SEED + 1):
                z = R.sde_solve(N, z0, th, R.grid(T), 0.05, solver, seed=seed)[0]
                smallest = min(smallest, np.abs(z - zdet).max(axis=(0, 2)).min())
    print(f"smallest per-trajectory departure from the deterministic scheme {smallest:.3e}; two thirds {2 * smallest / 3:.3e}")
    assert 0.95 * (2.0 / 3.0) * smallest <= R.MIN_DEPARTURE <= (2.0 / 3.0) * smallest


def test_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "sl_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "sl_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "Stuart-Landau host logic under ASan + UBSan" in r.stdout
