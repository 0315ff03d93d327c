"""GPU: the Kuramoto right-hand side (LDE_RHS_KURAMOTO: k_forward_dual_dir + k_adjoint_dual_dir of csrc/lde_dual_dir.hip, a lane per trajectory
and partial direction) against the float64 numpy restatement of the solve on dual numbers (tests/kuramoto_ref.py, pinned on the CPU by
tests/test_kuramoto_host.py).

Inputs: seeded, φ₀ ~ U(−π, π), ω, K ~ U(0.5, 2), ts = 0.05·j. N ∈ {2, 3, 4, 7}: groups of 8 lanes with 3 and 1 pad lanes, of 16 with 7 and 1.
Bounds: the dual tests' (tests/test_gpu_lv.py), each relative to the largest entry of the reference array of the case — ẑ 2e-5, J / dz0 / dθ
1e-4, on the same steps. The floor under them, the reference's f32 mode against its f64 mode on the (50, 256) cases
(tests/test_kuramoto_host.py::test_reference_f32_floor_under_the_gpu_bounds): ẑ 2.0e-6, J 1.8e-5, dz0 6.3e-6, dθ 6.2e-6 — within a quarter of
the bounds, which therefore stand as they are. Phases past 256 turns have bounds of their own, from the f32 format at |φ| ≈ 1 885 (same file,
test_reference_f32_floor_of_phases_past_256_turns): J 1.6e-4, dθ 8e-4.
Worst measured on the MI355X, ẑ / J / dz0 / dθ: fixed steps 2.0e-6 / 1.3e-5 / 7.8e-6 / 5.8e-6; the kernel's own adaptive steps
replayed 2.3e-6 / 2.7e-5 / 1.8e-5 / 1.4e-5 (N = 2; ≤ 4.8e-6 at the other N); T = 6001 7.1e-7 / 3.0e-6 / 5.2e-6 / 4.5e-6; the ragged grid 5.0e-7 /
1.3e-6 / 7.3e-7 / 4.9e-7; past 256 turns 1.2e-7 / 3.4e-5 / 1.6e-5 / 1.9e-4 (the f32 floor itself). First accepted step: 37 of 37 trajectories
within 1e-4 of the reference's at every N (largest relative difference 1.8e-6).

Every test here creates a handle of rhs_kind = 7, which lde_create refuses with LDE_ERR_INVALID_ARG before this right-hand side existed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import kuramoto_ref as R
from tests.lv_ref import ragged_grid

pytestmark = pytest.mark.gpu

Z_BOUND, J_BOUND = 2e-5, 1e-4
TURN_J_BOUND, TURN_G0_BOUND, TURN_GTH_BOUND = 1.6e-4, 1e-4, 8e-4      # tests/test_kuramoto_host.py: 4 × the f32 floor where it exceeds a quarter of 1e-4
FIRST_STEP_SEED = 50        # chosen on the CPU (tests/test_kuramoto_host.py): the reference's f32 mode meets its f64 mode's first step for all 37, every N
DUAL_TS_LDS_MAX = 6000      # csrc/lde_dual.h


def _native(N, **kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=L.RHS_KURAMOTO, state_dim=N, param_dim=N + 1, sensealg=L.SENSE_FORWARD_DUAL, **kw))


def _fixed(N, solver, dt, **kw):
    return _native(N, solver=solver, adaptive=0, dt=dt, **kw)


def _a256(x):
    return (x + 255) // 256 * 256


class _Record:
    """A dual record owned by the test (lde_set_step_record), so that J can be read back: n [B] | J [T][N][B][G] | (t, dt)."""

    def __init__(self, nat, N, B, T, hand_over=True):
        import torch
        self.nat, self.N, self.B, self.T, self.G = nat, N, B, T, R.group_width(N)
        self.nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
        assert self.nbytes >= _a256(4 * B) + _a256(4 * T * N * B * self.G)
        self.buf = torch.zeros((self.nbytes,), device="cuda", dtype=torch.uint8)
        if hand_over:
            self.hand_over()

    def hand_over(self):
        from latentdiffeq_amd import _lib as L
        L.check(self.nat.lib.lde_set_step_record(self.nat.h, C.c_void_p(self.buf.data_ptr()), self.nbytes), self.nat.h, "lde_set_step_record")

    def n(self):
        import torch
        return self.buf[:4 * self.B].view(torch.int32).cpu().numpy()

    def J(self):
        """[T, B, N, 2N + 1] (the reference's J layout); the pad lanes' columns must be zero."""
        import torch
        off = _a256(4 * self.B)
        raw = self.buf[off:off + 4 * self.T * self.N * self.B * self.G].view(torch.float32).cpu().numpy()
        full = raw.reshape(self.T, self.N, self.B, self.G).transpose(0, 2, 1, 3)
        NP = R.n_partials(self.N)
        assert (full[..., NP:] == 0).all(), "a pad lane's tangent must stay zero"
        return full[..., :NP].copy()


def _rel(a, b):
    """max |a − b| relative to the largest entry of the reference array b (0 where both are all zero)."""
    m = np.abs(b).max()
    d = np.abs(np.asarray(a, np.float64) - b).max()
    return d / m if m > 0 else d


def _gates(tag, z, J, g0, gth, zr, Jr, r0, rth, bounds=(Z_BOUND, J_BOUND, J_BOUND, J_BOUND)):
    ez, eJ, e0, eth = _rel(z, zr), _rel(J, Jr), _rel(g0, r0), _rel(gth, rth)
    print(f"{tag}: z {ez:.2e}, J {eJ:.2e}, dz0 {e0:.2e}, dtheta {eth:.2e} of the reference's largest entry")
    assert ez <= bounds[0], ez
    assert eJ <= bounds[1], eJ
    assert e0 <= bounds[2] and eth <= bounds[3], (e0, eth)


@functools.lru_cache(maxsize=None)
def _ref_fixed(N, solver, dt, T, B):
    """(z0, θ, ts, dz, ẑ_ref, J_ref, dz0_ref, dθ_ref, info): computed once per case in f64, shared, never written."""
    ts = R.grid(T)
    z0, th = R.inputs(B, N, seed=T)
    dz = R.cotangent(T, B, N)
    z, J, ret, info = R.solve(z0, th, ts, solver, adaptive=False, dt=dt)
    assert (ret == 0).all()
    g0, gth = R.pullback(J, dz)
    for a in (ts, z, J, g0, gth):
        a.setflags(write=False)
    return z0, th, ts, dz, z, J, g0, gth, info


def _steps_of(tr):
    """The kernel's accepted steps (Native.step_record) as the reference's replay argument."""
    return [tr["t"][b, :tr["n"][b]] for b in range(len(tr["n"]))], [tr["dt"][b, :tr["n"][b]] for b in range(len(tr["n"]))]


def _run(nat, N, z0, th, ts, dz):
    """forward into a test-owned record, J read back, pullback."""
    B, T = z0.shape[0], len(ts)
    rec = _Record(nat, N, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J = rec.J()
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert z.shape == (T, B, N) and g0.shape == (B, N) and gth.shape == (B, N + 1)
    return dict(rec=rec, z=z, ret=ret, st=st, J=J, g0=g0, gth=gth, sta=sta, n=rec.n())


@pytest.mark.parametrize("T,B", R.SHAPES)
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
@pytest.mark.parametrize("N", R.NS)
def test_fixed_step_parity_with_the_f64_reference(N, solver, dt, T, B):
    z0, th, ts, dz, zr, Jr, r0, rth, info = _ref_fixed(N, solver, dt, T, B)
    nat = _fixed(N, solver, dt)
    a = _run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    _gates(f"N {N} solver {solver} dt {dt} T {T} B {B}", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    assert a["st"] == dict(nfe=info["nfe"], naccept=info["naccept"], nreject=0, nfailed=0, max_steps=info["naccept"] // B)
    assert (a["n"] == info["naccept"] // B).all()
    assert a["sta"]["nfe"] == 0 and a["sta"]["naccept"] == 0 and a["sta"]["nfailed"] == 0
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_forward_dual_dir" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_adjoint_dual_dir"


@functools.lru_cache(maxsize=None)
def _adaptive_run(N):
    """Tsit5 at 1e-6 / 1e-3 on (T, B) = (50, 37) with the step trace: one solve per N for the two tests that look at it."""
    B, T = 37, 50
    nat = _native(N)
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, th = R.inputs(B, N, seed=FIRST_STEP_SEED)
    ts, dz = R.grid(T), R.cotangent(T, B, N)
    a = _run(nat, N, z0, th, ts, dz)
    a.update(nat=nat, z0=z0, th=th, ts=ts, dz=dz, tr=nat.step_record(0, B, cap=512))
    return a


@pytest.mark.parametrize("N", R.NS)
def test_adaptive_solve_on_the_kernels_own_steps(N):
    a = _adaptive_run(N)
    B, T, tr = 37, 50, a["tr"]
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], a["z0"])
    assert np.array_equal(tr["n"], a["n"]) and a["st"]["naccept"] == tr["n"].sum()
    assert a["st"]["nfe"] == 6 * (a["st"]["naccept"] + a["st"]["nreject"]) + 2 * B
    assert a["sta"]["nfe"] == 0 and a["sta"]["nfailed"] == 0
    zr, Jr, retr, _ = R.solve(a["z0"], a["th"], a["ts"], steps=_steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, a["dz"])
    _gates(f"N {N} adaptive, the kernel's steps replayed", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    # the record never overflows: its capacity is maxiters
    nmax, cap = C.c_int32(0), C.c_int32(0)
    nat = a["nat"]
    assert nat.lib.lde_step_record_status(nat.h, C.c_void_p(a["rec"].buf.data_ptr()), B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value == tr["n"].max() <= cap.value == 100000


@pytest.mark.parametrize("N", R.NS)
def test_first_accepted_step_is_the_dual_norm_controllers(N):
    """The kernel's first accepted step equals the f64 reference's (Hairer initial step and PI controller on the N-component dual-aware
    norm, whose sum over the partials the kernel forms across a group's lanes) to 1e-4 relative for every one of the 37 trajectories. Inputs:
    seed 50, with which the reference's own f32 mode reaches 100 % against its f64 mode on the CPU
    (tests/test_kuramoto_host.py::test_first_step_seed_meets_the_share_between_the_two_modes)."""
    a = _adaptive_run(N)
    _, _, ret, info = R.solve(a["z0"], a["th"], a["ts"])
    assert (ret == 0).all()
    d1 = np.array([d[0] for d in info["dt"]])
    k1 = a["tr"]["dt"][:, 0]
    same = np.abs(k1 - d1) <= 1e-4 * d1
    print(f"N {N} first accepted step: share {same.mean():.4f}, largest relative difference {np.abs(k1 / d1 - 1).max():.2e}; "
          f"accepted steps {a['st']['naccept']} (reference {info['naccept']})")
    assert same.all(), same.mean()


def test_ragged_grid():
    """Nine save times: three inside the first step(s), a gap of 0.875 that several steps cross without a save, three close together, a gap
    again. B = 3, N = 4; the kernel's steps replayed."""
    N, B = 4, 3
    ts = ragged_grid()
    T = len(ts)
    z0, th = R.inputs(B, N, seed=17)
    dz = R.cotangent(T, B, N)
    nat = _native(N)
    nat.set_option("step_trace", 1)
    a = _run(nat, N, z0, th, ts, dz)
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
    """T = DUAL_TS_LDS_MAX + 1 save times 1e-3 apart (the grid is read from global memory), B = 3, N = 4, Tsit5 at the fixed step 0.0125:
    against the reference; and the first 88 save points — those before the T = 100 solve's clipped last step, which starts at 0.0875 — are
    the bits of the T = 100 solve, whose grid is in LDS."""
    N, T, B, dt = 4, DUAL_TS_LDS_MAX + 1, 3, 0.0125
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(B, N, seed=13)
    dz = R.cotangent(T, B, N)
    nat = _fixed(N, R.TSIT5, dt)
    a = _run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    zr, Jr, retr, info = R.solve(z0, th, ts, R.TSIT5, adaptive=False, dt=dt)
    r0, rth = R.pullback(Jr, dz)
    _gates("T = 6001 (grid in global memory)", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    assert a["st"]["naccept"] == info["naccept"]
    rec100 = _Record(nat, N, B, 100)
    z100, ret100, _ = nat.forward(z0, th, ts[:100])
    J100 = rec100.J()
    assert (ret100 == 0).all()
    assert np.array_equal(z100[:88], a["z"][:88]) and np.array_equal(J100[:88], a["J"][:88])
    assert _rel(z100, zr[:100]) <= Z_BOUND and _rel(J100, Jr[:100]) <= J_BOUND


def _bits_of_shards(N, T, cuts, seed, **kw):
    """One call over [0, cuts[-1]) against the calls over the shards between the cuts: every output bit for bit."""
    Btot = cuts[-1]
    ts, dz = R.grid(T), R.cotangent(T, Btot, N)
    z0, th = R.inputs(Btot, N, seed=seed)
    nat = _native(N, **kw)
    whole = _run(nat, N, z0, th, ts, dz)
    assert (whole["ret"] == 0).all() and np.isfinite(whole["J"]).all()
    for lo, hi in zip([0] + list(cuts[:-1]), cuts):
        part = _run(nat, N, z0[lo:hi], th[lo:hi], ts, dz[:, lo:hi])
        assert np.array_equal(part["z"], whole["z"][:, lo:hi]) and np.array_equal(part["J"], whole["J"][:, lo:hi]), (lo, hi)
        assert np.array_equal(part["g0"], whole["g0"][lo:hi]) and np.array_equal(part["gth"], whole["gth"][lo:hi]), (lo, hi)
        assert np.array_equal(part["n"], whole["n"][lo:hi]) and np.array_equal(part["ret"], whole["ret"][lo:hi])


@pytest.mark.parametrize("N", R.NS)
def test_shards_are_the_bits_of_the_whole_batch(N):
    """B = 37 as one call against 18 + 19: the second shard's groups sit at other positions of their waves (and in other waves) than in the
    whole batch. The adaptive solve: step control included."""
    _bits_of_shards(N, 20, [18, 37], seed=11)


@pytest.mark.parametrize("N", [3, 4])
def test_batch_across_the_lane_threshold(N):
    """B·G = 4 096 lanes run in 64-lane workgroups, one trajectory more in 256-lane ones: the first 4096 / G trajectories are the same bits,
    and the last one — alone in the last workgroup's first group — is the bits of its own one-trajectory solve."""
    Bt = 4096 // R.group_width(N)
    _bits_of_shards(N, 9, [Bt, Bt + 1], seed=12)


@pytest.mark.parametrize("N", [3, 7])
def test_a_failing_neighbour_leaves_its_wave_alone(N):
    """One trajectory of 37 gets a NaN θ: it returns LDE_RET_NONFINITE, a NaN block, zero J and a zero gradient (whatever its cotangent
    holds) — and every other trajectory, those of its wave included, is the run without it, bit for bit."""
    B, T, bad = 37, 20, 5
    ts, dz = R.grid(T), np.array(R.cotangent(T, B, N))
    z0, th = R.inputs(B, N, seed=19)
    nat = _native(N)
    good = _run(nat, N, z0, th, ts, dz)
    assert (good["ret"] == 0).all()
    thb = th.copy()
    thb[bad, N // 2] = np.nan
    dzb = dz.copy()
    dzb[:, bad] = np.nan                                              # (what a loss of a NaN block hands back)
    a = _run(nat, N, z0, thb, ts, dzb)
    others = np.arange(B) != bad
    assert a["ret"][bad] == R.RET_NONFINITE and (a["ret"][others] == 0).all() and a["st"]["nfailed"] == 1 and a["sta"]["nfailed"] == 1
    assert np.isnan(a["z"][:, bad]).all() and (a["J"][:, bad] == 0).all() and a["n"][bad] == -R.RET_NONFINITE
    assert (a["g0"][bad] == 0).all() and (a["gth"][bad] == 0).all()
    for key in ("z", "J"):
        assert np.array_equal(a[key][:, others], good[key][:, others]), key
    for key in ("g0", "gth", "n"):
        assert np.array_equal(a[key][others], good[key][others]), key


@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
@pytest.mark.parametrize("N", R.NS)
def test_phases_past_256_turns(N, solver):
    """φ₀ + 2π·300: past the 256 turns up to which the hardware sine is defined. (T, B) = (5, 37), fixed steps of 0.05, against the f64
    reference on the same f32 inputs. A sine that returns 0 out there loses the coupling and moves J by 0.15 to 0.22 of its largest entry;
    the bounds are the f32 format's at this magnitude (tests/test_kuramoto_host.py::test_reference_f32_floor_of_phases_past_256_turns)."""
    T, B = 5, 37
    z0, th = R.turn_inputs(B, N)
    assert np.abs(z0).min() > 2 * np.pi * 256
    ts, dz = R.grid(T), R.cotangent(T, B, N)
    nat = _fixed(N, solver, 0.05)
    a = _run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    zr, Jr, retr, _ = R.solve(z0, th, ts, solver, adaptive=False, dt=0.05)
    r0, rth = R.pullback(Jr, dz)
    _gates(f"N {N} solver {solver} past 256 turns", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth,
           bounds=(Z_BOUND, TURN_J_BOUND, TURN_G0_BOUND, TURN_GTH_BOUND))


def test_captured_pair_replays_bit_for_bit():
    """lde_reserve, an eager forward + pullback, then the pair captured on one stream: the replay writes the eager bits."""
    import torch
    from latentdiffeq_amd import _lib as L
    N, B, T = 4, 300, 20
    nat = _native(N)
    lib = nat.lib
    L.check(lib.lde_reserve(nat.h, B, T), nat.h, "lde_reserve")
    ts = R.grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = R.inputs(B, N, seed=3)
    z0d, thd, dzd = (torch.from_numpy(a).to("cuda") for a in (z0, th, R.cotangent(T, B, N)))
    rec = _Record(nat, N, B, T)
    out = torch.empty((T, B, N), device="cuda")
    g0, gth = torch.empty((B, N), device="cuda"), torch.empty((B, N + 1), device="cuda")
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
    """Kuramoto(3) through autograd: ẑ₀ [3, B] and θ̂ [4, B] in, gradients of those shapes out. Before the hook (solve_batch, what
    diffeq_layer calls) ẑ, dz0 and dθ are the C ABI's bit for bit; diffeq_layer's output is the sine of that ẑ and its gradients are the C
    ABI's pullback of the cotangent times cos ẑ; another sensealg is refused with the library's text."""
    import torch
    import latentdiffeq_amd as la
    N, B, T = 3, 75, 20
    ts = R.grid(T)
    ku = la.Kuramoto(N)
    dec = la.Decoder(la.GOKU_basic(), (None, ku, None))
    z0, th = R.inputs(B, N, seed=1)
    dz = R.cotangent(T, B, N, seed=11)
    dzt = torch.tensor(dz, device="cuda")
    nat = _native(N)
    zc, ret, _ = nat.forward(z0, th, ts)
    assert (ret == 0).all()
    # before the hook
    z0b = torch.tensor(z0, device="cuda", requires_grad=True)
    thb = torch.tensor(th, device="cuda", requires_grad=True)
    zb, _ = la.solve_batch(ku, z0b, thb, ts)                          # (T, B, N)
    (zb * dzt).sum().backward()
    torch.cuda.synchronize()
    g0, gth, _, _ = nat.adjoint(zc, th, ts, dz)
    assert np.array_equal(zb.detach().cpu().numpy(), zc)
    assert np.array_equal(z0b.grad.cpu().numpy(), g0) and np.array_equal(thb.grad.cpu().numpy(), gth) and np.abs(gth).max() > 0
    h = ku._native()
    assert h.lib.lde_last_kernel(h.ptr, 0) == b"k_forward_dual_dir" and h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
    # with the hook, in the reference's layout
    z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
    tht = torch.tensor(th.T.copy(), device="cuda", requires_grad=True)
    assert z0t.shape == (N, B) and tht.shape == (N + 1, B)
    zhat = la.diffeq_layer(dec, (z0t, tht), ts)                       # [N, B, T]
    assert zhat.shape == (N, B, T)
    zct = torch.tensor(zc, device="cuda")
    assert torch.equal(zhat.detach().permute(2, 1, 0), torch.sin(zct))
    (zhat * dzt.permute(2, 1, 0)).sum().backward()
    torch.cuda.synchronize()
    h0, hth, _, _ = nat.adjoint(zc, th, ts, (dzt * torch.cos(zct)).cpu().numpy())
    assert z0t.grad.shape == (N, B) and tht.grad.shape == (N + 1, B)
    assert np.array_equal(z0t.grad.cpu().numpy().T, h0) and np.array_equal(tht.grad.cpu().numpy().T, hth)
    for other in (la.BacksolveAdjoint(), la.ForwardDiffSensitivity(), la.ParallelAdjoint()):
        with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
            la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.Kuramoto(N, sensealg=other), None)), (z0t, tht), ts)


def test_loss_batch_trains_end_to_end():
    """A LatentDiffEqModel with the plug-in: 28×28 input, B = 8, T = 10, N = 3; loss_batch forward and backward leave a finite gradient on
    every parameter, lo_z₀ is three wide and lo_θ the four-wide softplus head."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    torch.manual_seed(0)
    B, T = 8, 10
    mt, ku = la.GOKU_basic(), la.Kuramoto(3)
    enc, dec = TR.default_layers(mt, 784, ku, device="cuda")
    assert tuple(dec[0][0].sizes) == (16, 200, 3) and tuple(dec[0][1].sizes) == (16, 200, 4) and dec[0][1].acts[-1] == L.CACT_SOFTPLUS
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
            assert prm.grad is not None and torch.isfinite(prm.grad).all()
        assert dec[0][1].theta.grad.abs().max() > 0, "the gradient must reach lo_θ through dθ̂"
    h = ku._native()
    assert h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
