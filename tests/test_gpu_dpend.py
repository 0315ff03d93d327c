"""GPU: the double pendulum (LDE_RHS_DOUBLE_PENDULUM: DoublePendDir of csrc/lde_dpend_dualrhs.h on k_forward_dual_dir + k_adjoint_dual_dir of
csrc/lde_dual_dir.hip, a lane per trajectory and partial direction: 8 directions in one 8-lane group, no pad lane) against the float64 numpy
restatement of the solve on dual numbers (tests/dpend_ref.py, pinned on the CPU by tests/test_dpend_host.py).

Inputs: seeded, θ₁, θ₂, ω₁, ω₂ ~ U(−1, 1), L ~ U(0.8, 1.6), m ~ U(0.5, 2), ts = 0.05·j. Bounds: the dual tests' (tests/test_gpu_lv.py), each
relative to the largest entry of the reference array of the case — ẑ 2e-5, J / dz0 / dθ 1e-4, on the same steps — wherever the reference's
own f32 mode stays within a quarter of them on the case's inputs (tests/test_dpend_host.py asserts every floor on the CPU). Three cases do
not fit and have, by the project's rule, 4 × their CPU floor, rounded up (tests/dpend_ref.py: the table at its end): Tsit5 at dt = 0.05 on
(50, 256) ẑ 2.5e-5, J 1.5e-4; the adaptive solve on (50, 37) ẑ 3.5e-5, J 1.6e-4; angles past 256 turns J 1.4e-3, dz0 1.1e-3, dθ 8.5e-4.
Worst measured on the MI355X: DESIGN.md §8.4.

Every test here creates a handle of rhs_kind = 9, which lde_create refuses with LDE_ERR_INVALID_ARG before this right-hand side existed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import dpend_ref as R

pytestmark = pytest.mark.gpu

D, P, G, NP = R.D, R.P, R.G, R.NP
DUAL_TS_LDS_MAX = 6000      # csrc/lde_dual.h


def _native(**kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=L.RHS_DOUBLE_PENDULUM, state_dim=D, param_dim=P, sensealg=L.SENSE_FORWARD_DUAL, **kw))


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

    def J(self):
        """[T, B, 4, 8] (the reference's J layout)."""
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
def _ref_fixed(solver, dt, T, B):
    """(z0, θ, ts, dz, ẑ_ref, J_ref, dz0_ref, dθ_ref, info): computed once per case in f64, shared, never written."""
    ts = R.grid(T)
    z0, th = R.inputs(B, seed=R.PARITY_SEED[T])
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
    """forward into a test-owned record, J read back, pullback."""
    B, T = z0.shape[0], len(ts)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J = rec.J()
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert z.shape == (T, B, D) and g0.shape == (B, D) and gth.shape == (B, P)
    return dict(rec=rec, z=z, ret=ret, st=st, J=J, g0=g0, gth=gth, sta=sta, n=rec.n())


@pytest.mark.parametrize("T,B", R.SHAPES)
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_fixed_step_parity_with_the_f64_reference(solver, dt, T, B):
    z0, th, ts, dz, zr, Jr, r0, rth, info = _ref_fixed(solver, dt, T, B)
    nat = _fixed(solver, dt)
    a = _run(nat, z0, th, ts, dz)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    if T == 1:      # (1, 1) is exact: ẑ₀ itself and the seeds
        assert np.array_equal(a["z"], zr.astype(np.float32)) and np.array_equal(a["J"], Jr.astype(np.float32))
        assert np.array_equal(a["g0"], r0.astype(np.float32)) and (a["gth"] == 0).all() and (rth == 0).all()
    _gates(f"solver {solver} dt {dt} T {T} B {B}", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth, bounds=R.bounds(solver, dt, T))
    assert a["st"] == dict(nfe=info["nfe"], naccept=info["naccept"], nreject=0, nfailed=0, max_steps=info["naccept"] // B)
    assert (a["n"] == info["naccept"] // B).all()
    assert a["sta"]["nfe"] == 0 and a["sta"]["naccept"] == 0 and a["sta"]["nfailed"] == 0


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
    """Tsit5 at 1e-6 / 1e-3 on (T, B) = (50, 37) with the step trace: one solve for the two tests that look at it."""
    B, T = 37, 50
    nat = _native()
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, th = R.inputs(B, seed=R.ADAPTIVE_SEED)
    ts, dz = R.grid(T), R.cotangent(T, B)
    a = _run(nat, z0, th, ts, dz)
    a.update(nat=nat, z0=z0, th=th, ts=ts, dz=dz, tr=nat.step_record(0, B, cap=512))
    return a


def test_adaptive_solve_on_the_kernels_own_steps():
    a = _adaptive_run()
    B, T, tr = 37, 50, a["tr"]
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], a["z0"])
    assert np.array_equal(tr["n"], a["n"]) and a["st"]["naccept"] == tr["n"].sum()
    assert a["st"]["nfe"] == 6 * (a["st"]["naccept"] + a["st"]["nreject"]) + 2 * B
    assert a["sta"]["nfe"] == 0 and a["sta"]["nfailed"] == 0
    zr, Jr, retr, _ = R.solve(a["z0"], a["th"], a["ts"], steps=_steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, a["dz"])
    _gates("adaptive, the kernel's steps replayed", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth, bounds=R.ADAPTIVE_BOUNDS)
    nmax, cap = C.c_int32(0), C.c_int32(0)
    nat = a["nat"]
    assert nat.lib.lde_step_record_status(nat.h, C.c_void_p(a["rec"].buf.data_ptr()), B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value == tr["n"].max() <= cap.value == 100000


def test_first_accepted_step_is_the_dual_norm_controllers():
    """The kernel's first accepted step equals the f64 reference's (Hairer initial step and PI controller on the four-component dual-aware
    norm, whose sum over the eight partials the kernel forms across a group's lanes) to 1e-4 relative for every one of the 37 trajectories.
    With these inputs the reference's own f32 mode meets its f64 mode for all 37 on the CPU (largest relative difference 2.3e-5:
    tests/test_dpend_host.py::test_reference_f32_floor_of_the_adaptive_case)."""
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
    """Nine save times: three inside the first step(s), a gap of 0.875 that several steps cross without a save, three close together, a gap
    again. B = 3; the kernel's steps replayed."""
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
    J100 = rec100.J()
    assert (ret100 == 0).all()
    assert np.array_equal(z100[:88], a["z"][:88]) and np.array_equal(J100[:88], a["J"][:88])
    assert _rel(z100, zr[:100]) <= R.BOUNDS[0] and _rel(J100, Jr[:100]) <= R.BOUNDS[1]


def _bits_of_shards(T, cuts, seed, **kw):
    """One call over [0, cuts[-1]) against the calls over the shards between the cuts: every output bit for bit."""
    Btot = cuts[-1]
    ts, dz = R.grid(T), R.cotangent(T, Btot)
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
    _bits_of_shards(20, [18, 37], seed=11)


def test_batch_across_the_lane_threshold():
    """B·8 = 4 096 lanes run in 64-lane workgroups, one trajectory more in 256-lane ones: the first 512 trajectories are the same bits, and the
    last one — alone in the last workgroup's first group — is the bits of its own one-trajectory solve."""
    _bits_of_shards(9, [512, 513], seed=12)


def test_a_failing_neighbour_leaves_its_wave_alone():
    """One trajectory of 37 gets a NaN in its ẑ₀: it returns LDE_RET_NONFINITE, a NaN block, zero J and a zero gradient (whatever its
    cotangent holds) — and every other trajectory, those of its wave included, is the run without it, bit for bit."""
    B, T, bad = 37, 20, 5
    ts, dz = R.grid(T), np.array(R.cotangent(T, B))
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


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_m2_zero_is_the_librarys_pendulum(solver):
    """m₂ = 0: (θ₁, ω₁) is within 2e-5 (of the largest entry) of the library's own pendulum kernel for L = L₁ under the same solver at the same
    fixed steps, and for a cotangent on those two rows alone the dθ columns L₂ and m₁ are exact zeros (dθ[L₁] and dθ[m₂] are not)."""
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    B, T, dt = 37, 20, 0.05
    ts = R.grid(T)
    z0, th = R.inputs(B, seed=21)
    th[:, 3] = 0.0
    dz = np.array(R.cotangent(T, B))
    dz[:, :, [1, 3]] = 0.0
    a = _run(_fixed(solver, dt), z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    pend = Native(make_desc(rhs_kind=L.RHS_PENDULUM, sensealg=L.SENSE_FORWARD_DUAL, solver=solver, adaptive=0, dt=dt))
    zp, retp, _ = pend.forward(z0[:, [0, 2]], th[:, :1], ts)
    assert (retp == 0).all()
    err = _rel(a["z"][:, :, [0, 2]], zp.astype(np.float64))
    print(f"solver {solver}, m2 = 0: (theta1, omega1) within {err:.2e} of the pendulum kernel's")
    assert err <= R.BOUNDS[0], err
    assert (a["gth"][:, 1] == 0).all() and (a["gth"][:, 2] == 0).all()
    assert (a["J"][:, :, [0, 2], 5] == 0).all() and (a["J"][:, :, [0, 2], 6] == 0).all()
    assert np.abs(a["gth"][:, 0]).min() > 0 and np.abs(a["gth"][:, 3]).max() > 0
    g0p, gLp, _, _ = pend.adjoint(zp, th[:, :1], ts, dz[:, :, [0, 2]])
    assert _rel(a["g0"][:, [0, 2]], g0p.astype(np.float64)) <= R.BOUNDS[2] and _rel(a["gth"][:, :1], gLp.astype(np.float64)) <= R.BOUNDS[3]


@pytest.mark.parametrize("solver,dt", [(R.TSIT5, 0.0125), (R.RK4, 0.05)])
def test_mass_homogeneity_of_the_gradient(solver, dt):
    """m₁·dθ[m₁] + m₂·dθ[m₂] is within the dθ bound (of dθ's largest entry) of 0: the right-hand side is homogeneous of degree 0 in the masses."""
    z0, th, ts, dz, zr, Jr, r0, rth, _ = _ref_fixed(solver, dt, 50, 256)
    a = _run(_fixed(solver, dt), z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    res = th[:, 2].astype(np.float64) * a["gth"][:, 2] + th[:, 3].astype(np.float64) * a["gth"][:, 3]
    rel = np.abs(res).max() / np.abs(rth).max()
    print(f"solver {solver} dt {dt}: m1 dtheta[m1] + m2 dtheta[m2] is {rel:.2e} of dtheta's largest entry")
    assert rel <= R.BOUNDS[3], rel
    assert np.abs(a["gth"][:, 2:]).max() > 100 * R.BOUNDS[3] * np.abs(rth).max()      # (neither column is small by itself)


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_angles_past_256_turns(solver):
    """θ₁, θ₂ + 2π·300: past the 256 turns up to which the hardware sine is defined. (T, B) = (5, 37), fixed steps of 0.05, against the f64
    reference on the same f32 inputs. The bounds are 4 × the f32 format's floor at this magnitude
    (tests/test_dpend_host.py::test_reference_f32_floor_of_angles_past_256_turns)."""
    T, B = 5, 37
    z0, th = R.turn_inputs(B)
    assert np.abs(z0[:, :2]).min() > 2 * np.pi * 256
    ts, dz = R.grid(T), R.cotangent(T, B)
    a = _run(_fixed(solver, 0.05), z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    zr, Jr, retr, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=0.05)
    r0, rth = R.pullback(Jr, dz)
    _gates(f"solver {solver} past 256 turns", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth, bounds=R.TURN_BOUNDS)


def test_captured_pair_replays_bit_for_bit():
    """lde_reserve, an eager forward + pullback, then the pair captured on one stream: the replay writes the eager bits."""
    import torch
    from latentdiffeq_amd import _lib as L
    B, T = 300, 20
    nat = _native()
    lib = nat.lib
    L.check(lib.lde_reserve(nat.h, B, T), nat.h, "lde_reserve")
    ts = R.grid(T)
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
    """DoublePendulum() through autograd: ẑ₀ [4, B] and θ̂ [4, B] in, gradients of those shapes out; ẑ, dz0 and dθ are the C ABI's bit for
    bit (transform_after_diffeq is the identity); another sensealg is refused with the library's text."""
    import torch
    import latentdiffeq_amd as la
    B, T = 75, 20
    ts = R.grid(T)
    dp = la.DoublePendulum()
    dec = la.Decoder(la.GOKU_basic(), (None, dp, None))
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
    h = dp._native()
    assert h.lib.lde_last_kernel(h.ptr, 0) == b"k_forward_dual_dir" and h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
    for other in (la.BacksolveAdjoint(), la.ForwardDiffSensitivity(), la.ParallelAdjoint()):
        with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
            la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.DoublePendulum(sensealg=other), None)), (z0t, tht), ts)


def test_loss_batch_trains_end_to_end():
    """A LatentDiffEqModel with the plug-in: 28×28 input, B = 8, T = 10; loss_batch forward and backward leave a finite gradient of its
    parameter's shape on every parameter, lo_z₀ is four wide and lo_θ the four-wide softplus head, and a gradient step moves lo_θ."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    torch.manual_seed(0)
    B, T = 8, 10
    mt, dp = la.GOKU_basic(), la.DoublePendulum()
    enc, dec = TR.default_layers(mt, 784, dp, device="cuda")
    assert tuple(dec[0][0].sizes) == (16, 200, 4) and tuple(dec[0][1].sizes) == (16, 200, 4) and dec[0][1].acts[-1] == L.CACT_SOFTPLUS
    model = TR.LatentDiffEqModel(mt, enc, dec)
    x = torch.rand(T, B, 784, device="cuda").permute(2, 1, 0)
    for variational in (False, True):
        for prm in model.parameters():
            prm.grad = None
        loss = TR.loss_batch(model, x, R.grid(T), 1e-3, variational)
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
    h = dp._native()
    assert h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
