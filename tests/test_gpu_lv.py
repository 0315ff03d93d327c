"""GPU: the Lotka–Volterra right-hand side (LDE_RHS_LOTKA_VOLTERRA: the k_lv_forward_dual + k_lv_adjoint_dual path of csrc/lde_dual.hip) against the
float64 numpy restatement of the solve on dual numbers (tests/lv_ref.py, pinned on the CPU by tests/test_lv_host.py).

Inputs: seeded, x₀, y₀ ∈ [0.5, 2], α, β, γ, δ ∈ [0.5, 1.5], ts = 0.05·j. Bounds: the pendulum dual tests' (tests/test_gpu_forward_dual.py), each
relative to the largest entry of the reference array of the case — ẑ 2e-5, J / dz0 / dθ 1e-4, on the same steps. The floor under them, the
reference's f32 mode against its f64 mode on the (50, 256) cases (tests/test_lv_host.py::test_reference_f32_floor_under_the_gpu_bounds):
ẑ 5.0e-7, J 5.9e-7, dz0 8.7e-7, dθ 5.7e-7 — below a quarter of the bounds, which therefore stand as they are.
Worst measured on the MI355X, ẑ / J / dz0 / dθ: fixed steps 6.9e-7 / 4.7e-7 / 7.6e-7 / 7.1e-7; the kernel's own adaptive steps
replayed 1.1e-6 / 1.3e-6 / 1.3e-6 / 1.2e-6; T = 6001 7.7e-7 / 1.8e-6 / 3.4e-6 / 1.8e-6; the ragged grid 1.1e-6 / 6.2e-7 / 2.9e-6 / 3.3e-7. First
accepted step: 256 of 256 trajectories within 1e-4 of the reference's (largest relative difference 1.2e-6).

Every test here creates a handle of rhs_kind = 5, which lde_create refuses with LDE_ERR_INVALID_ARG before this right-hand side existed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import lv_ref as R

pytestmark = pytest.mark.gpu

Z_BOUND, J_BOUND = 2e-5, 1e-4
FIRST_STEP_SEED = 50        # chosen on the CPU (tests/test_lv_host.py): the reference's f32 mode meets its f64 mode's first step for 100 % of 256
DUAL_TS_LDS_MAX = 6000      # csrc/lde_dual.h


def _native(**kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=L.RHS_LOTKA_VOLTERRA, param_dim=4, sensealg=L.SENSE_FORWARD_DUAL, **kw))


def _fixed(solver, dt, **kw):
    return _native(solver=solver, adaptive=0, dt=dt, **kw)


def _a256(x):
    return (x + 255) // 256 * 256


class _Record:
    """A dual record owned by the test (lde_set_step_record), so that J can be read back: n [B] | J [T][2][6][B] | (t, dt)."""

    def __init__(self, nat, B, T, hand_over=True):
        import torch
        self.nat, self.B, self.T = nat, B, T
        self.nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
        assert self.nbytes >= _a256(4 * B) + _a256(48 * T * B)
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
        """[T, B, 2, 6] (the reference's J layout)."""
        import torch
        off = _a256(4 * self.B)
        raw = self.buf[off:off + 48 * self.T * self.B].view(torch.float32).cpu().numpy()
        return raw.reshape(self.T, 2, R.NP, self.B).transpose(0, 3, 1, 2).copy()


def _rel(a, b):
    """max |a − b| relative to the largest entry of the reference array b (0 where both are all zero)."""
    m = np.abs(b).max()
    d = np.abs(np.asarray(a, np.float64) - b).max()
    return d / m if m > 0 else d


def _gates(tag, z, J, g0, gth, zr, Jr, r0, rth):
    ez, eJ, e0, eth = _rel(z, zr), _rel(J, Jr), _rel(g0, r0), _rel(gth, rth)
    print(f"{tag}: z {ez:.2e}, J {eJ:.2e}, dz0 {e0:.2e}, dtheta {eth:.2e} of the reference's largest entry")
    assert ez <= Z_BOUND, ez
    assert eJ <= J_BOUND, eJ
    assert e0 <= J_BOUND and eth <= J_BOUND, (e0, eth)


@functools.lru_cache(maxsize=None)
def _ref_fixed(solver, dt, T, B):
    """(z0, θ, ts, dz, ẑ_ref, J_ref, dz0_ref, dθ_ref, info): computed once per case in f64, shared, never written."""
    ts = R.grid(T)
    z0, th = R.inputs(B, seed=T)
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


@pytest.mark.parametrize("T,B", R.SHAPES)
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
def test_fixed_step_parity_with_the_f64_reference(solver, dt, T, B):
    z0, th, ts, dz, zr, Jr, r0, rth, info = _ref_fixed(solver, dt, T, B)
    nat = _fixed(solver, dt)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J = rec.J()
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert (ret == 0).all() and np.array_equal(z[0], z0) and gth.shape == (B, 4)
    _gates(f"solver {solver} dt {dt} T {T} B {B}", z, J, g0, gth, zr, Jr, r0, rth)
    assert st == dict(nfe=info["nfe"], naccept=info["naccept"], nreject=0, nfailed=0, max_steps=info["naccept"] // B)
    assert (rec.n() == info["naccept"] // B).all()
    assert sta["nfe"] == 0 and sta["naccept"] == 0 and sta["nfailed"] == 0
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_lv_forward_dual" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_lv_adjoint_dual"


@pytest.fixture(scope="module")
def adaptive_run():
    """Tsit5 at 1e-6 / 1e-3 on B = 256, T = 50 with the step trace: one solve for the two tests that look at it."""
    B, T = 256, 50
    nat = _native()
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, th = R.inputs(B, seed=FIRST_STEP_SEED)
    ts, dz = R.grid(T), R.cotangent(T, B)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J = rec.J()
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    tr = nat.step_record(0, B, cap=512)
    return dict(nat=nat, rec=rec, z0=z0, th=th, ts=ts, dz=dz, z=z, ret=ret, st=st, J=J, g0=g0, gth=gth, sta=sta, tr=tr)


def test_adaptive_solve_on_the_kernels_own_steps(adaptive_run):
    a = adaptive_run
    B, T, tr = 256, 50, a["tr"]
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], a["z0"])
    assert np.array_equal(tr["n"], a["rec"].n()) and a["st"]["naccept"] == tr["n"].sum()
    assert a["st"]["nfe"] == 6 * (a["st"]["naccept"] + a["st"]["nreject"]) + 2 * B
    assert a["sta"]["nfe"] == 0 and a["sta"]["nfailed"] == 0
    zr, Jr, retr, _ = R.solve(a["z0"], a["th"], a["ts"], steps=_steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, a["dz"])
    _gates("adaptive, the kernel's steps replayed", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    # the record never overflows: its capacity is maxiters
    nmax, cap = C.c_int32(0), C.c_int32(0)
    nat = a["nat"]
    assert nat.lib.lde_step_record_status(nat.h, C.c_void_p(a["rec"].buf.data_ptr()), B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value == tr["n"].max() <= cap.value == 100000


@functools.lru_cache(maxsize=None)
def _ref_first_steps():
    z0, th = R.inputs(256, seed=FIRST_STEP_SEED)
    _, _, ret, info = R.solve(z0, th, R.grid(50))
    assert (ret == 0).all()
    return np.array([d[0] for d in info["dt"]]), info["naccept"]


def test_first_accepted_step_is_the_dual_norm_controllers(adaptive_run):
    """The kernel's first accepted step equals the f64 reference's (Hairer initial step and PI controller on the dual-aware norm) to 1e-4
    relative for at least 99 % of the 256 trajectories. Inputs: seed 50, with which the reference's own f32 mode reaches 100 % against its
    f64 mode on the CPU (tests/test_lv_host.py::test_first_step_seed_meets_the_share_between_the_two_modes)."""
    d1, nacc = _ref_first_steps()
    k1 = adaptive_run["tr"]["dt"][:, 0]
    same = np.abs(k1 - d1) <= 1e-4 * d1
    print(f"first accepted step: share {same.mean():.4f}, largest relative difference {np.abs(k1 / d1 - 1).max():.2e}; "
          f"accepted steps {adaptive_run['st']['naccept']} (reference {nacc})")
    assert same.mean() >= 0.99, same.mean()


def test_batch_across_the_lane_threshold():
    """B = 4097 runs in 256-lane workgroups, B = 4096 in 64-lane ones: the first 4096 columns are the same bits, and the last trajectory — alone
    in the seventeenth workgroup's first lane — is the bits of its own one-trajectory solve."""
    T = 9
    ts, dz = R.grid(T), R.cotangent(T, 4097)
    z0, th = R.inputs(4097, seed=11)
    nat = _native()
    out = []
    for lo, hi in ((0, 4097), (0, 4096), (4096, 4097)):
        B = hi - lo
        rec = _Record(nat, B, T)
        z, ret, _ = nat.forward(z0[lo:hi], th[lo:hi], ts)
        J = rec.J()
        g0, gth, _, _ = nat.adjoint(z, th[lo:hi], ts, dz[:, lo:hi])
        assert (ret == 0).all() and np.isfinite(J).all()
        out.append((z, J, g0, gth, rec.n()))
    whole, first, last = out
    for w, f, l in zip(whole, first, last):
        w = np.moveaxis(w, 1, 0) if w.ndim >= 3 else w            # trajectory first
        f = np.moveaxis(f, 1, 0) if f.ndim >= 3 else f
        l = np.moveaxis(l, 1, 0) if l.ndim >= 3 else l
        assert np.array_equal(w[:4096], f) and np.array_equal(w[4096:], l)


def test_save_grid_outside_lds():
    """T = DUAL_TS_LDS_MAX + 1 save times 1e-3 apart (the grid is read from global memory), B = 3, Tsit5 at the fixed step 0.0125 so that the
    T = 100 solve (grid in LDS) takes the same steps: against the reference; the first 88 save points — those before the T = 100 solve's
    clipped last step, which starts at 0.0875 — are the LDS variant's bits, and the other twelve, reached through last steps of 0.0115 and
    0.0125, agree to 8 roundings of f32 (1e-6 of the largest entry: both steps' truncation errors, ≈ h⁵, are far below one rounding)."""
    T, B, dt = DUAL_TS_LDS_MAX + 1, 3, 0.0125
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(B, seed=13)
    dz = R.cotangent(T, B)
    nat = _fixed(R.TSIT5, dt)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J = rec.J()
    g0, gth, _, _ = nat.adjoint(z, th, ts, dz)
    assert (ret == 0).all()
    zr, Jr, retr, info = R.solve(z0, th, ts, R.TSIT5, adaptive=False, dt=dt)
    r0, rth = R.pullback(Jr, dz)
    _gates("T = 6001 (grid in global memory)", z, J, g0, gth, zr, Jr, r0, rth)
    assert st["naccept"] == info["naccept"]
    rec100 = _Record(nat, B, 100)
    z100, ret100, _ = nat.forward(z0, th, ts[:100])
    J100 = rec100.J()
    assert (ret100 == 0).all()
    assert np.array_equal(z100[:88], z[:88]) and np.array_equal(J100[:88], J[:88])
    assert _rel(z100, zr[:100]) <= Z_BOUND and _rel(J100, Jr[:100]) <= J_BOUND
    assert np.abs(z100 - z[:100]).max() <= 1e-6 * np.abs(zr[:100]).max() and np.abs(J100 - J[:100]).max() <= 1e-6 * np.abs(Jr[:100]).max()


def test_ragged_grid():
    """Nine save times: three inside the first step(s), a gap of 0.875 that several steps cross without a save, three close together, a gap
    again. The kernel's steps replayed."""
    ts = R.ragged_grid()
    T, B = len(ts), 37
    z0, th = R.inputs(B, seed=17)
    dz = R.cotangent(T, B)
    nat = _native()
    nat.set_option("step_trace", 1)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    J = rec.J()
    g0, gth, _, _ = nat.adjoint(z, th, ts, dz)
    tr = nat.step_record(0, B, cap=256)
    assert (ret == 0).all() and np.array_equal(z[0], z0)
    # the grid is what it claims to be, for every trajectory: a step with several save times, and steps with none
    for b in range(B):
        t0 = tr["t"][b, :tr["n"][b]]
        per_step = np.histogram(ts[1:], bins=np.append(t0, ts[-1] + 1e-9))[0]
        assert per_step.max() >= 2 and (per_step == 0).sum() >= 1, per_step
    zr, Jr, retr, _ = R.solve(z0, th, ts, steps=_steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(Jr, dz)
    _gates("ragged grid", z, J, g0, gth, zr, Jr, r0, rth)


def test_two_forwards_in_flight_with_caller_owned_records():
    """Two forwards of different shapes, each into a record the caller owns, then their pullbacks in reverse order: each pullback contracts
    its own J."""
    import torch
    from latentdiffeq_amd import _lib as L
    nat = _fixed(R.TSIT5, 0.05)
    cases = [_ref_fixed(R.TSIT5, 0.05, 50, 256), _ref_fixed(R.TSIT5, 0.05, 2, 37)]
    flights = []
    for z0, th, ts, dz, zr, Jr, r0, rth, _ in cases:
        rec = _Record(nat, z0.shape[0], len(ts))
        z, ret, _ = nat.forward(z0, th, ts)
        assert (ret == 0).all()
        flights.append((rec, z))
    for (z0, th, ts, dz, zr, Jr, r0, rth, _), (rec, z) in reversed(list(zip(cases, flights))):
        rec.hand_over()
        g0, gth, _, _ = nat.adjoint(z, th, ts, dz)
        _gates(f"in flight, B {z0.shape[0]}", z, rec.J(), g0, gth, zr, Jr, r0, rth)
    # without the caller's record the handle has none of that shape: refused, not a wrong J
    L.check(nat.lib.lde_set_step_record(nat.h, None, 0), nat.h, "lde_set_step_record")
    with pytest.raises(Exception, match="no dual record"):
        nat.adjoint(flights[0][1], cases[0][1], cases[0][2], cases[0][3])
    torch.cuda.synchronize()


def test_failed_trajectory_gives_nan_block_and_zero_gradient():
    B, T = 8, 50                                                     # (the reference needs 8 to 10 accepted steps here)
    nat = _native(maxiters=3)
    z0, th = R.inputs(B, seed=2)
    ts = R.grid(T)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, th, ts)                             # (the call itself returns LDE_OK: Native.forward checks it)
    assert (ret == R.RET_MAXITERS).all() and np.isnan(z).all() and st["nfailed"] == B
    assert (rec.J() == 0).all() and (rec.n() == -R.RET_MAXITERS).all()
    dz = np.array(R.cotangent(T, B))
    dz[:, :3] = np.nan                                               # (what a loss of a NaN block hands back)
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert (g0 == 0).all() and (gth == 0).all() and sta["nfailed"] == B and sta["nfe"] == 0
    with pytest.raises(Exception, match="LDE_ERR_UNSUPPORTED"):      # a deterministic handle takes no noise
        from latentdiffeq_amd import _lib as L
        L.check(nat.lib.lde_set_noise(nat.h, 1, 0, 0, None), nat.h, "lde_set_noise")


def test_captured_pair_replays_bit_for_bit():
    """lde_reserve, an eager forward + pullback, then the pair captured on one stream: the replay writes the eager bits."""
    import torch
    from latentdiffeq_amd import _lib as L
    B, T = 512, 50
    nat = _native()
    lib = nat.lib
    L.check(lib.lde_reserve(nat.h, B, T), nat.h, "lde_reserve")
    ts = R.grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = R.inputs(B, seed=3)
    z0d, thd, dzd = (torch.from_numpy(a).to("cuda") for a in (z0, th, R.cotangent(T, B)))
    rec = _Record(nat, B, T)
    out = torch.empty((T, B, 2), device="cuda")
    g0, gth = torch.empty((B, 2), device="cuda"), torch.empty((B, 4), device="cuda")
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
    """diffeq_layer with LotkaVolterra(): θ̂ [4, B] in, dθ̂ [4, B] out through autograd — the C ABI's ẑ, dz0, dθ bit for bit; two forwards in
    flight before their pullbacks each keep their own J; another sensealg is refused with the library's text."""
    import torch
    import latentdiffeq_amd as la
    B, T = 75, 20
    ts = R.grid(T)
    lv = la.LotkaVolterra()
    dec = la.Decoder(la.GOKU_basic(), (None, lv, None))
    cases = []
    for seed in (1, 2):
        z0, th = R.inputs(B, seed=seed)
        z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
        tht = torch.tensor(th.T.copy(), device="cuda", requires_grad=True)
        assert tht.shape == (4, B)
        zhat = la.diffeq_layer(dec, (z0t, tht), ts)                   # [2, B, T]
        assert zhat.shape == (2, B, T)
        cases.append((z0, th, R.cotangent(T, B, seed=10 + seed), z0t, tht, zhat))
    for z0, th, dz, z0t, tht, zhat in reversed(cases):                # pullbacks in the other order
        (zhat * torch.tensor(dz, device="cuda").permute(2, 1, 0)).sum().backward()
    torch.cuda.synchronize()
    h = lv._native()
    assert h.lib.lde_last_kernel(h.ptr, 0) == b"k_lv_forward_dual" and h.lib.lde_last_kernel(h.ptr, 1) == b"k_lv_adjoint_dual"
    nat = _native()
    for z0, th, dz, z0t, tht, zhat in cases:
        zc, ret, _ = nat.forward(z0, th, ts)
        g0, gth, _, _ = nat.adjoint(zc, th, ts, dz)
        assert (ret == 0).all() and tht.grad.shape == (4, B)
        assert np.array_equal(zhat.detach().permute(2, 1, 0).cpu().numpy(), zc)
        assert np.array_equal(z0t.grad.cpu().numpy().T, g0) and np.array_equal(tht.grad.cpu().numpy().T, gth)
        assert np.abs(gth).max() > 0
    for other in (la.BacksolveAdjoint(), la.ForwardDiffSensitivity(), la.ParallelAdjoint()):
        with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
            la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.LotkaVolterra(sensealg=other), None)), (cases[0][3], cases[0][4]), ts)


def test_loss_batch_trains_end_to_end():
    """A LatentDiffEqModel with the plug-in: 28×28 input, B = 8, T = 10; loss_batch forward and backward leave a finite gradient on every
    parameter, and lo_θ is the four-wide softplus head."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    torch.manual_seed(0)
    B, T = 8, 10
    mt, lv = la.GOKU_basic(), la.LotkaVolterra()
    enc, dec = TR.default_layers(mt, 784, lv, device="cuda")
    assert tuple(dec[0][1].sizes) == (16, 200, 4) and dec[0][1].acts[-1] == L.CACT_SOFTPLUS
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
    h = lv._native()
    assert h.lib.lde_last_kernel(h.ptr, 1) == b"k_lv_adjoint_dual"
