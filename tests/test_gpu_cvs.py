"""GPU: the cardiovascular system (LDE_RHS_CVS: CvsDir of csrc/lde_cvs_dualrhs.h on k_forward_dual_dir + k_adjoint_dual_dir of
csrc/lde_dual_dir.hip, a lane per trajectory and partial direction: 6 directions in one 8-lane group, lanes 6 and 7 pad lanes) against the
float64 numpy restatement of the solve on dual numbers (tests/cvs_ref.py, pinned on the CPU by tests/test_cvs_host.py).

Inputs: seeded, z₀ ~ U(0.75, 0.85), z₁ ~ U(0.5, 0.9), z₂ ~ U(0.15, 0.25), z₃ ~ U(0.9, 1.0), i_ext ~ U(−2, 0), r_mod ~ U(0, 0.3); ts = 0.05·j
(`grid`) or 1.0·j (`slow_grid`, the system's own time scale). Bounds: the dual tests' (tests/test_gpu_lv.py), each relative to the largest
entry of the reference array of the case — ẑ 2e-5, J / dz0 / dθ 1e-4, on the same steps — wherever the reference's own f32 mode stays within
a quarter of them on the case's inputs (tests/test_cvs_host.py asserts every floor on the CPU). Two cases do not fit in ẑ and have, by the
project's rule, 4 × their CPU floor, rounded up (tests/cvs_ref.py: FINE_BOUNDS): dt = 0.0125 on (50, 256) and dt = 0.25 on `slow_grid`
(50, 37), ẑ 2.5e-5. Worst measured on the MI355X: DESIGN.md §8.6.

Every test here creates a handle of rhs_kind = 11 (or la.CVS), which lde_create refuses with LDE_ERR_INVALID_ARG before this right-hand
side existed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cvs_ref as R

pytestmark = pytest.mark.gpu

D, P, G, NP = R.D, R.P, R.G, R.NP
DUAL_TS_LDS_MAX = 6000      # csrc/lde_dual.h


def _native(**kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=L.RHS_CVS, state_dim=D, param_dim=P, sensealg=L.SENSE_FORWARD_DUAL, **kw))


def _fixed(solver, dt, **kw):
    return _native(solver=solver, adaptive=0, dt=dt, **kw)


def _a256(x):
    return (x + 255) // 256 * 256


class _Record:
    """A dual record owned by the test (lde_set_step_record), so that J can be read back: n [B] | J [T][4][B][8] | (t, dt)."""

    def __init__(self, nat, B, T):
        import torch
        from latentdiffeq_amd import _lib as L
        self.nat, self.B, self.T = nat, B, T
        self.nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
        assert self.nbytes >= _a256(4 * B) + _a256(4 * T * D * B * G)
        self.buf = torch.zeros((self.nbytes,), device="cuda", dtype=torch.uint8)
        L.check(nat.lib.lde_set_step_record(nat.h, C.c_void_p(self.buf.data_ptr()), self.nbytes), nat.h, "lde_set_step_record")

    def n(self):
        import torch
        return self.buf[:4 * self.B].view(torch.int32).cpu().numpy()

    def J8(self):
        """[T, B, 4, 8]: the record's eight columns, the two pad lanes' included."""
        import torch
        off = _a256(4 * self.B)
        raw = self.buf[off:off + 4 * self.T * D * self.B * G].view(torch.float32).cpu().numpy()
        return raw.reshape(self.T, D, self.B, G).transpose(0, 2, 1, 3).copy()


def _rel(a, b):
    """max |a − b| relative to the largest entry of the reference array b (0 where both are all zero)."""
    m = np.abs(b).max()
    d = np.abs(np.asarray(a, np.float64) - b).max()
    return d / m if m > 0 else d


def _gates(tag, z, J, g0, gth, zr, Jr, r0, rth, bounds=R.BOUNDS):
    ez, eJ, e0, eth = _rel(z, zr), _rel(J, Jr), _rel(g0, r0), _rel(gth, rth)
    print(f"{tag}: z {ez:.2e}, J {eJ:.2e}, dz0 {e0:.2e}, dtheta {eth:.2e} of the reference's largest entry (bounds {bounds})")
    assert ez <= bounds[0], ez
    assert eJ <= bounds[1], eJ
    assert e0 <= bounds[2] and eth <= bounds[3], (e0, eth)


@functools.lru_cache(maxsize=None)
def _ref_fixed(solver, dt, T, B, slow=False):
    """(z0, θ, ts, dz, ẑ_ref, J_ref, dz0_ref, dθ_ref, info): computed once per case in f64, shared, never written."""
    ts = R.slow_grid(T) if slow else R.grid(T)
    z0, th = R.inputs(B, seed=R.SLOW_SEED if slow else R.PARITY_SEED[T])
    dz = R.cotangent(T, B)
    z, J, ret, info = R.solve(z0, th, ts, solver, adaptive=False, dt=dt)
    assert (ret == 0).all()
    g0, gth = R.pullback(J, dz)
    for a in (ts, z, J, g0, gth):
        a.setflags(write=False)
    return z0, th, ts, dz, z, J, g0, gth, info


def _steps_of(tr):
    """The kernel's accepted steps (Native.step_record) as the reference's replay argument."""
    return [tr["t"][b, :tr["n"][b]] for b in range(len(tr["n"]))], [tr["dt"][b, :tr["n"][b]] for b in range(len(tr["n"]))]


def _run(nat, z0, th, ts, dz):
    """forward into a test-owned record, J read back (the pad columns must be exact zeros), pullback."""
    B, T = z0.shape[0], len(ts)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J8 = rec.J8()
    assert (J8[..., NP:] == 0).all(), "the pad lanes' columns of the record are zero"
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert z.shape == (T, B, D) and g0.shape == (B, D) and gth.shape == (B, P)
    return dict(rec=rec, z=z, ret=ret, st=st, J=J8[..., :NP].copy(), g0=g0, gth=gth, sta=sta, n=rec.n())


def _parity(solver, dt, T, B, slow, bounds):
    z0, th, ts, dz, zr, Jr, r0, rth, info = _ref_fixed(solver, dt, T, B, slow)
    a = _run(_fixed(solver, dt), z0, th, ts, dz)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    if T == 1:      # (1, 1) is exact: ẑ₀ itself and the seeds
        assert np.array_equal(a["z"], zr.astype(np.float32)) and np.array_equal(a["J"], Jr.astype(np.float32))
        assert np.array_equal(a["g0"], r0.astype(np.float32)) and (a["gth"] == 0).all() and (rth == 0).all()
    _gates(f"solver {solver} dt {dt} T {T} B {B}{' slow grid' if slow else ''}", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth, bounds=bounds)
    assert a["st"] == dict(nfe=info["nfe"], naccept=info["naccept"], nreject=0, nfailed=0, max_steps=info["naccept"] // B)
    assert (a["n"] == info["naccept"] // B).all()
    assert a["sta"]["nfe"] == 0 and a["sta"]["naccept"] == 0 and a["sta"]["nfailed"] == 0
    return a


@pytest.mark.parametrize("T,B", R.SHAPES)
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_fixed_step_parity_with_the_f64_reference(solver, dt, T, B):
    _parity(solver, dt, T, B, False, R.bounds(solver, dt, T))


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_fixed_step_parity_on_the_slow_grid(solver):
    """ts = 1.0·j, dt = 0.25, (50, 37): the system's own time scale — t ≤ 49, where the baroreflex (TAU = 20) has moved."""
    _parity(solver, R.SLOW_DT, *R.SLOW_SHAPE, True, R.FINE_BOUNDS)


def test_last_kernel_labels():
    """lde_last_kernel returns the path's labels, the Kuramoto system's: the kernels are the same templates over another system."""
    z0, th, ts, dz, *_ = _ref_fixed(R.RK4, 0.05, 2, 37)
    nat = _fixed(R.RK4, 0.05)
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"" and nat.lib.lde_last_kernel(nat.h, 1) == b""
    _run(nat, z0, th, ts, dz)
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_forward_dual_dir" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_adjoint_dual_dir"
    assert nat.lib.lde_set_noise(nat.h, 1, 0, 0, None) == -2 and b"LDE_RHS_SPENDULUM only" in nat.lib.lde_last_error(nat.h)


@functools.lru_cache(maxsize=None)
def _adaptive_run():
    """Tsit5 at 1e-6 / 1e-3 on `slow_grid`, (T, B) = (50, 37), with the step trace: one solve for the tests that look at it."""
    T, B = R.SLOW_SHAPE
    nat = _native()
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, th = R.inputs(B, seed=R.ADAPTIVE_SEED)
    ts, dz = R.slow_grid(T), R.cotangent(T, B)
    a = _run(nat, z0, th, ts, dz)
    a.update(nat=nat, z0=z0, th=th, ts=ts, dz=dz, tr=nat.step_record(0, B, cap=512))
    return a


def test_adaptive_solve_on_the_kernels_own_steps():
    a = _adaptive_run()
    (T, B), tr = R.SLOW_SHAPE, a["tr"]
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], a["z0"])
    assert np.array_equal(tr["n"], a["n"]) and a["st"]["naccept"] == tr["n"].sum()
    assert a["st"]["nfe"] == 6 * (a["st"]["naccept"] + a["st"]["nreject"]) + 2 * B
    assert a["sta"]["nfe"] == 0 and a["sta"]["nfailed"] == 0
    zr, Jr, retr, _ = R.solve(a["z0"], a["th"], a["ts"], steps=_steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, a["dz"])
    _gates("adaptive, the kernel's steps replayed", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    nmax, cap = C.c_int32(0), C.c_int32(0)
    nat = a["nat"]
    assert nat.lib.lde_step_record_status(nat.h, C.c_void_p(a["rec"].buf.data_ptr()), B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value == tr["n"].max() <= cap.value == 100000


def test_first_accepted_step_is_the_dual_norm_controllers():
    """The kernel's first accepted step equals the f64 reference's (Hairer initial step and PI controller on the four-component dual-aware
    norm, whose sum over the partials the kernel forms across a group's lanes, pad lanes adding zeros) to 1e-4 relative for every one of the
    37 trajectories. The reference's own f32 mode differs from its f64 mode by 6.5e-8 there
    (tests/test_cvs_host.py::test_reference_f32_floor_of_the_adaptive_case)."""
    a = _adaptive_run()
    _, _, ret, info = R.solve(a["z0"], a["th"], a["ts"])
    assert (ret == 0).all()
    d1 = np.array([d[0] for d in info["dt"]])
    k1 = a["tr"]["dt"][:, 0]
    same = np.abs(k1 - d1) <= 1e-4 * d1
    print(f"first accepted step: share {same.mean():.4f}, largest relative difference {np.abs(k1 / d1 - 1).max():.2e}; "
          f"accepted steps {a['st']['naccept']} (reference {info['naccept']}), rejected {a['st']['nreject']} ({info['nreject']})")
    assert same.all(), same.mean()


def test_ragged_grid():
    """Nine save times (tests/dual_ref.py's, stretched 20× for this slower system): three inside one step, gaps that several steps cross
    without a save. B = 3; the kernel's steps replayed."""
    B = 3
    ts = R.ragged_grid()
    T = len(ts)
    z0, th = R.inputs(B, seed=R.RAGGED_SEED)
    dz = R.cotangent(T, B)
    nat = _native()
    nat.set_option("step_trace", 1)
    a = _run(nat, z0, th, ts, dz)
    tr = nat.step_record(0, B, cap=256)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    for b in range(B):   # the grid is what it claims to be: a step with several save times, and steps with none
        t0 = tr["t"][b, :tr["n"][b]]
        per_step = np.histogram(ts[1:], bins=np.append(t0, ts[-1] + 1e-9))[0]
        assert per_step.max() >= 2 and (per_step == 0).sum() >= 1, per_step
    zr, Jr, retr, _ = R.solve(z0, th, ts, steps=_steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, dz)
    _gates("ragged grid", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)


def test_save_grid_outside_lds():
    """T = DUAL_TS_LDS_MAX + 1 save times 1e-3 apart (the grid is read from global memory), B = 3, Tsit5 at the fixed step 0.0125: against the
    reference; and the first 88 save points — those before the T = 100 solve's clipped last step, which starts at 0.0875 — are the bits of
    the T = 100 solve, whose grid is in LDS."""
    T, B, dt = DUAL_TS_LDS_MAX + 1, 3, 0.0125
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(B, seed=R.LONG_SEED)
    dz = R.cotangent(T, B)
    nat = _fixed(R.TSIT5, dt)
    a = _run(nat, z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    zr, Jr, retr, info = R.solve(z0, th, ts, R.TSIT5, adaptive=False, dt=dt)
    r0, rth = R.pullback(Jr, dz)
    _gates("T = 6001 (grid in global memory)", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    assert a["st"]["naccept"] == info["naccept"]
    rec100 = _Record(nat, B, 100)
    z100, ret100, _ = nat.forward(z0, th, ts[:100])
    J100 = rec100.J8()[..., :NP]
    assert (ret100 == 0).all()
    assert np.array_equal(z100[:88], a["z"][:88]) and np.array_equal(J100[:88], a["J"][:88])
    assert _rel(z100, zr[:100]) <= R.BOUNDS[0] and _rel(J100, Jr[:100]) <= R.BOUNDS[1]


def _bits_of_shards(T, cuts, seed, ts, **kw):
    """One call over [0, cuts[-1]) against the calls over the shards between the cuts: every output bit for bit."""
    Btot = cuts[-1]
    dz = R.cotangent(T, Btot)
    z0, th = R.inputs(Btot, seed=seed)
    nat = _native(**kw)
    whole = _run(nat, z0, th, ts, dz)
    assert (whole["ret"] == 0).all() and np.isfinite(whole["J"]).all()
    for lo, hi in zip([0] + list(cuts[:-1]), cuts):
        part = _run(nat, z0[lo:hi], th[lo:hi], ts, dz[:, lo:hi])
        assert np.array_equal(part["z"], whole["z"][:, lo:hi]) and np.array_equal(part["J"], whole["J"][:, lo:hi]), (lo, hi)
        assert np.array_equal(part["g0"], whole["g0"][lo:hi]) and np.array_equal(part["gth"], whole["gth"][lo:hi]), (lo, hi)
        assert np.array_equal(part["n"], whole["n"][lo:hi]) and np.array_equal(part["ret"], whole["ret"][lo:hi])


def test_shards_are_the_bits_of_the_whole_batch():
    """B = 37 as one call against 18 + 19: the second shard's groups sit at other positions of their waves (and in other waves) than in the
    whole batch. The adaptive solve: step control included."""
    _bits_of_shards(20, [18, 37], seed=11, ts=R.slow_grid(20))


def test_batch_across_the_lane_threshold():
    """B·8 = 4 096 lanes run in 64-lane workgroups, one trajectory more in 256-lane ones: the first 512 trajectories are the same bits, and the
    last one — alone in the last workgroup's first group — is the bits of its own one-trajectory solve."""
    _bits_of_shards(9, [512, 513], seed=12, ts=R.slow_grid(9))


def test_a_failing_neighbour_leaves_its_wave_alone():
    """One trajectory of 37 gets a NaN in its ẑ₀: it returns LDE_RET_NONFINITE, a NaN block, zero J and a zero gradient (whatever its
    cotangent holds) — and every other trajectory, those of its wave included, is the run without it, bit for bit."""
    B, T, bad = 37, 20, 5
    ts, dz = R.slow_grid(T), np.array(R.cotangent(T, B))
    z0, th = R.inputs(B, seed=19)
    nat = _native()
    good = _run(nat, z0, th, ts, dz)
    assert (good["ret"] == 0).all()
    z0b = z0.copy()
    z0b[bad, 2] = np.nan
    dzb = dz.copy()
    dzb[:, bad] = np.nan                                              # (what a loss of a NaN block hands back)
    a = _run(nat, z0b, th, ts, dzb)
    others = np.arange(B) != bad
    assert a["ret"][bad] == R.RET_NONFINITE and (a["ret"][others] == 0).all() and a["st"]["nfailed"] == 1 and a["sta"]["nfailed"] == 1
    assert np.isnan(a["z"][:, bad]).all() and (a["J"][:, bad] == 0).all() and a["n"][bad] == -R.RET_NONFINITE
    assert (a["g0"][bad] == 0).all() and (a["gth"][bad] == 0).all()
    for key in ("z", "J"):
        assert np.array_equal(a[key][:, others], good[key][:, others]), key
    for key in ("g0", "gth", "n"):
        assert np.array_equal(a[key][others], good[key][others]), key


@pytest.mark.parametrize("mode", ["tsit5-adaptive", "tsit5-fixed", "rk4-fixed"])
def test_fourth_row_is_exact(mode):
    """z₃' = i_ext·SV_MOD depends on i_ext alone: J[3, (0, 1, 2, 5)] are exact zeros and J[3, 3] an exact one at every save time — adaptive
    (`slow_grid`) and fixed-step (`grid` at dt = 0.05: save times on the steps' ends, see
    tests/test_cvs_host.py::test_reference_fourth_row_is_exact) — and a cotangent on row 3 alone gives dz0[:, 0:3] = 0 and dθ[:, r_mod] = 0
    exactly, with dθ[:, i_ext] = SV_MOD·Σ_j t_j·c_j not zero."""
    T, B = 20, 37
    z0, th = R.inputs(B, seed=13)
    dz = np.array(R.cotangent(T, B))
    dz[:, :, :3] = 0.0
    if mode == "tsit5-adaptive":
        nat, ts = _native(), R.slow_grid(T)
    else:
        nat, ts = _fixed(R.TSIT5 if mode == "tsit5-fixed" else R.RK4, 0.05), R.grid(T)
    a = _run(nat, z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    assert (a["J"][:, :, 3, [0, 1, 2, 5]] == 0).all() and (a["J"][:, :, 3, 3] == 1).all()
    assert (a["g0"][:, 0:3] == 0).all() and (a["gth"][:, 1] == 0).all()
    assert np.abs(a["gth"][:, 0]).min() > 0
    want = R.SV_MOD * np.einsum("t,tb->b", ts, dz[:, :, 3].astype(np.float64))
    assert _rel(a["gth"][:, 0], want) <= R.BOUNDS[3]
    assert _rel(a["g0"][:, 3], dz[:, :, 3].astype(np.float64).sum(axis=0)) <= R.BOUNDS[2]


@pytest.mark.parametrize("solver,dt", [(R.TSIT5, 0.05), (R.TSIT5, 0.0125), (R.RK4, 0.05), (R.RK4, 0.0125)])
def test_blood_volume(solver, dt):
    """On the (50, 256) parity cases: 400·ẑ₀ + 1110·ẑ₁ − i_ext·t is constant along the solve, to the case's ẑ bound relative to the largest
    entry of the volume; and with the cotangent c_j·(400, 1110, 0, 0) the pullback is dz0 = (400 Σc, 1110 Σc, 0, 0), dθ = (Σ c_j t_j, 0), each
    to the case's bound relative to the largest entry (dθ at dt = 0.0125: 2.1e-4, 4 × the reference's own f32 floor —
    tests/test_cvs_host.py::test_reference_f32_floor_of_the_blood_volume)."""
    T, B = 50, 256
    z0, th, ts, _, zr, Jr, _, _, _ = _ref_fixed(solver, dt, T, B)
    bounds = R.volume_bounds(solver, dt)
    dz, want0, wantth = R.volume_cotangent(T, B, ts)
    a = _run(_fixed(solver, dt), z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    V = R.volume(a["z"].astype(np.float64), th.astype(np.float64), ts)
    drift = np.abs(V - V[0]).max() / np.abs(V).max()
    e0, eth = _rel(a["g0"], want0), _rel(a["gth"], wantth)
    print(f"solver {solver} dt {dt}: volume drift {drift:.2e}, dz0 {e0:.2e}, dtheta {eth:.2e} of the largest entry (bounds {bounds})")
    assert drift <= bounds[0], drift
    assert e0 <= bounds[1] and eth <= bounds[2], (e0, eth)


@pytest.mark.parametrize("pa", [2000.0, 0.0])
def test_saturated_baroreflex(pa):
    """p_a(0) = 2000 (eˣ = inf, w = 0) and p_a(0) = 0 (w ≈ 1), (20, 37), RK4 at 0.05: everything is finite, every return code 0, and parity
    holds at the standing bounds (floor: tests/test_cvs_host.py::test_reference_saturated_baroreflex_stays_finite)."""
    T, B = 20, 37
    z0, th = R.saturated_inputs(B, pa)
    ts, dz = R.grid(T), R.cotangent(T, B)
    a = _run(_fixed(R.RK4, 0.05), z0, th, ts, dz)
    assert (a["ret"] == 0).all() and a["st"]["nfailed"] == 0
    for key in ("z", "J", "g0", "gth"):
        assert np.isfinite(a[key]).all(), key
    zr, Jr, retr, _ = R.solve(z0, th, ts, R.RK4, adaptive=False, dt=0.05)
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, dz)
    _gates(f"p_a(0) = {pa}", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)


def test_captured_pair_replays_bit_for_bit():
    """lde_reserve, an eager forward + pullback, then the pair captured on one stream: the replay writes the eager bits."""
    import torch
    from latentdiffeq_amd import _lib as L
    B, T = 300, 20
    nat = _native()
    lib = nat.lib
    L.check(lib.lde_reserve(nat.h, B, T), nat.h, "lde_reserve")
    ts = R.slow_grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = R.inputs(B, seed=3)
    z0d, thd, dzd = (torch.from_numpy(a).to("cuda") for a in (z0, th, R.cotangent(T, B)))
    rec = _Record(nat, B, T)
    out = torch.empty((T, B, D), device="cuda")
    g0, gth = torch.empty((B, D), device="cuda"), torch.empty((B, P), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def step():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.lde_forward(nat.h, p(z0d), p(thd), tsp, T, B, p(out), None, s), nat.h, "fwd")
        L.check(lib.lde_adjoint(nat.h, p(out), p(thd), tsp, T, B, p(dzd), p(g0), p(gth), None, s), nat.h, "adj")

    def snap():
        torch.cuda.synchronize()
        return [x.clone() for x in (out, g0, gth, rec.buf)]

    def clobber():
        for x in (out, g0, gth):
            x.fill_(7.0)
        rec.buf.zero_()
        torch.cuda.synchronize()

    step()
    a = snap()
    assert torch.isfinite(a[0]).all() and a[2].abs().max() > 0
    clobber()
    step()
    for x, y in zip(a, snap()):
        assert torch.equal(x, y), "two runs must be bit-identical"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    clobber()
    graph.replay()
    for x, y in zip(a, snap()):
        assert torch.equal(x, y), "the replayed graph must equal the eager result bit for bit"


def test_torch_autograd_equals_the_c_abi():
    """CVS() through autograd: ẑ₀ [4, B] and θ̂ [2, B] in, gradients of those shapes out; ẑ, dz0 and dθ are the C ABI's bit for bit
    (transform_after_diffeq is the identity); another sensealg is refused with the library's text."""
    import torch
    import latentdiffeq_amd as la
    B, T = 75, 20
    ts = R.slow_grid(T)
    cv = la.CVS()
    dec = la.Decoder(la.GOKU_basic(), (None, cv, None))
    z0, th = R.inputs(B, seed=1)
    dz = R.cotangent(T, B, seed=11)
    dzt = torch.tensor(dz, device="cuda")
    nat = _native()
    zc, ret, _ = nat.forward(z0, th, ts)
    assert (ret == 0).all()
    g0, gth, _, _ = nat.adjoint(zc, th, ts, dz)
    z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
    tht = torch.tensor(th.T.copy(), device="cuda", requires_grad=True)
    assert z0t.shape == (D, B) and tht.shape == (P, B)
    zhat = la.diffeq_layer(dec, (z0t, tht), ts)                       # [4, B, T]
    assert zhat.shape == (D, B, T)
    assert np.array_equal(zhat.detach().permute(2, 1, 0).cpu().numpy(), zc)
    (zhat * dzt.permute(2, 1, 0)).sum().backward()
    torch.cuda.synchronize()
    assert z0t.grad.shape == (D, B) and tht.grad.shape == (P, B)
    assert np.array_equal(z0t.grad.cpu().numpy().T, g0) and np.array_equal(tht.grad.cpu().numpy().T, gth) and np.abs(gth).max() > 0
    h = cv._native()
    assert h.lib.lde_last_kernel(h.ptr, 0) == b"k_forward_dual_dir" and h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
    for other in (la.BacksolveAdjoint(), la.ForwardDiffSensitivity(), la.ParallelAdjoint()):
        with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
            la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.CVS(sensealg=other), None)), (z0t, tht), ts)


def test_loss_batch_trains_end_to_end():
    """A LatentDiffEqModel with the plug-in and the heads its docstring names: 28×28 input, B = 8, T = 10; loss_batch forward and backward
    leave a finite gradient of its parameter's shape on every parameter, lo_z₀ is the four-wide sigmoid head and lo_θ the two-wide identity
    head, lo_θ's gradient is not zero, and a gradient step moves lo_θ."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    torch.manual_seed(0)
    B, T = 8, 10
    mt, cv = la.GOKU_basic(), la.CVS()
    enc, dec = TR.default_layers(mt, 784, cv, device="cuda", z0_activation="sigmoid", theta_activation="identity")
    assert tuple(dec[0][0].sizes) == (16, 200, 4) and tuple(dec[0][1].sizes) == (16, 200, 2)
    assert dec[0][0].acts[-1] == L.CACT_SIGMOID and dec[0][1].acts[-1] == L.CACT_IDENTITY
    model = TR.LatentDiffEqModel(mt, enc, dec)
    x = torch.rand(T, B, 784, device="cuda").permute(2, 1, 0)
    for variational in (False, True):
        for prm in model.parameters():
            prm.grad = None
        loss = TR.loss_batch(model, x, R.slow_grid(T), 1e-3, variational)
        loss.backward()
        L.join_weight_gradients()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        params = model.parameters()
        assert len(params) > 0
        for prm in params:
            assert prm.grad is not None and prm.grad.shape == prm.shape and torch.isfinite(prm.grad).all()
        assert dec[0][1].theta.grad.abs().max() > 0, "the gradient must reach lo_θ through dθ̂"
    before = dec[0][1].theta.detach().clone()
    with torch.no_grad():                                             # a plain gradient step on every parameter
        for prm in model.parameters():
            prm -= 1e-2 * prm.grad
    torch.cuda.synchronize()
    assert torch.isfinite(dec[0][1].theta).all() and not torch.equal(dec[0][1].theta.detach(), before)
    h = cv._native()
    assert h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
