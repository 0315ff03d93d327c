"""GPU: the deterministic Stuart–Landau network (LDE_RHS_STUART_LANDAU: StuartLandauDir<N> of csrc/lde_sl_dualrhs.h on k_forward_dual_dir +
k_adjoint_dual_dir of csrc/lde_dual_dir.hip, a lane per trajectory and partial direction: N = 1 — 5 directions in an 8-lane group, three pad
lanes; N = 2 — 9 in 16, seven pad lanes; N = 3 — 13 in 16, three pad lanes, and D = 6 components) against the float64 numpy restatement of the
solve on dual numbers (tests/sl_ref.py, pinned on the CPU by tests/test_sl_host.py).

Inputs: seeded, x₀, y₀ ~ U(−1, 1), a ~ U(−0.5, 1), ω ~ U(0.5, 3), G ~ U(0, 1); ts = 0.05·j. Bounds: the project's standing ones, each relative to
the largest entry of the reference array of the case — ẑ 2e-5, J / dz0 / dθ 1e-4, on the same steps; the reference's own f32 mode stays within a
twentieth of them on every case's inputs (tests/test_sl_host.py asserts a quarter). Worst measured on the MI355X: DESIGN.md §8.7.

Every test here creates a handle of rhs_kind = 13 (or la.StuartLandau), which lde_create refuses with LDE_ERR_INVALID_ARG ("unknown rhs_kind")
before this right-hand side existed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sl_gpu as U
from tests import sl_ref as R

pytestmark = pytest.mark.gpu

DUAL_TS_LDS_MAX = 6000      # csrc/lde_dual.h
NS = R.NS


@functools.lru_cache(maxsize=None)
def _ref_fixed(N, solver, dt, T, B):
    """(z0, θ, ts, dz, ẑ_ref, J_ref, dz0_ref, dθ_ref, info): computed once per case in f64, shared, never written."""
    ts = R.grid(T)
    z0, th = R.inputs(N, B, seed=R.PARITY_SEED[T])
    dz = R.cotangent(N, T, B)
    z, J, ret, info = R.solve(N, z0, th, ts, solver, adaptive=False, dt=dt)
    assert (ret == 0).all()
    g0, gth = R.pullback(N, J, dz)
    for a in (ts, z, J, g0, gth):
        a.setflags(write=False)
    return z0, th, ts, dz, z, J, g0, gth, info


@pytest.mark.parametrize("T,B", R.SHAPES)
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("solver", [R.TSIT5, R.RK4])
@pytest.mark.parametrize("N", NS)
def test_fixed_step_parity_with_the_f64_reference(N, solver, dt, T, B):
    z0, th, ts, dz, zr, Jr, r0, rth, info = _ref_fixed(N, solver, dt, T, B)
    nat = U.fixed(N, solver, dt)
    assert nat.lib.lde_last_kernel(nat.h, 0) == b""
    a = U.run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    if T == 1:      # (1, 1) is exact: ẑ₀ itself and the seeds
        assert np.array_equal(a["z"], zr.astype(np.float32)) and np.array_equal(a["J"], Jr.astype(np.float32))
        assert np.array_equal(a["g0"], r0.astype(np.float32)) and (a["gth"] == 0).all() and (rth == 0).all()
    U.gates(f"N {N} solver {solver} dt {dt} T {T} B {B}", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth, bounds=R.bounds(solver, dt, T))
    assert a["st"] == dict(nfe=info["nfe"], naccept=info["naccept"], nreject=0, nfailed=0, max_steps=info["naccept"] // B)
    assert (a["n"] == info["naccept"] // B).all()
    assert a["sta"]["nfe"] == 0 and a["sta"]["naccept"] == 0 and a["sta"]["nfailed"] == 0
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_forward_dual_dir" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_adjoint_dual_dir"


@functools.lru_cache(maxsize=None)
def _adaptive_run(N):
    """Tsit5 at 1e-6 / 1e-3 on ts = 0.05·j, (T, B) = (50, 37), with the step trace: one solve per N for the tests that look at it."""
    T, B = R.ADAPTIVE_SHAPE
    nat = U.native(N)
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, th = R.inputs(N, B, seed=R.ADAPTIVE_SEED)
    ts, dz = R.grid(T), R.cotangent(N, T, B)
    a = U.run(nat, N, z0, th, ts, dz)
    a.update(nat=nat, z0=z0, th=th, ts=ts, dz=dz, tr=nat.step_record(0, B, cap=512))
    return a


@pytest.mark.parametrize("N", NS)
def test_adaptive_solve_on_the_kernels_own_steps(N):
    a = _adaptive_run(N)
    (T, B), tr = R.ADAPTIVE_SHAPE, a["tr"]
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], a["z0"])
    assert np.array_equal(tr["n"], a["n"]) and a["st"]["naccept"] == tr["n"].sum()
    assert a["st"]["nfe"] == 6 * (a["st"]["naccept"] + a["st"]["nreject"]) + 2 * B
    assert a["sta"]["nfe"] == 0 and a["sta"]["nfailed"] == 0
    zr, Jr, retr, _ = R.solve(N, a["z0"], a["th"], a["ts"], steps=U.steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(N, Jr, a["dz"])
    U.gates(f"N {N} adaptive, the kernel's steps replayed", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    nmax, cap = C.c_int32(0), C.c_int32(0)
    nat = a["nat"]
    assert nat.lib.lde_step_record_status(nat.h, C.c_void_p(a["rec"].buf.data_ptr()), B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value == tr["n"].max() <= cap.value == 100000


@pytest.mark.parametrize("N", NS)
def test_first_accepted_step_is_the_dual_norm_controllers(N):
    """The kernel's first accepted step equals the f64 reference's (Hairer initial step and PI controller on the 2N-component dual-aware
    norm, whose sum over the partials the kernel forms across a group's lanes, pad lanes adding zeros) to 1e-4 relative for every one of the
    37 trajectories (the reference's own f32 mode against its f64 mode: tests/test_sl_host.py::test_reference_f32_floor_of_the_adaptive_case)."""
    a = _adaptive_run(N)
    _, _, ret, info = R.solve(N, a["z0"], a["th"], a["ts"])
    assert (ret == 0).all()
    d1 = np.array([d[0] for d in info["dt"]])
    k1 = a["tr"]["dt"][:, 0]
    same = np.abs(k1 - d1) <= 1e-4 * d1
    print(f"N {N} first accepted step: share {same.mean():.4f}, largest relative difference {np.abs(k1 / d1 - 1).max():.2e}; "
          f"accepted steps {a['st']['naccept']} (reference {info['naccept']}), rejected {a['st']['nreject']} ({info['nreject']})")
    assert same.all(), same.mean()


@pytest.mark.parametrize("N", NS)
def test_ragged_grid(N):
    """Nine save times (tests/dual_ref.py's): three inside one step, gaps that several steps cross without a save. B = 3; the kernel's steps
    replayed."""
    B = 3
    ts = R.ragged_grid()
    T = len(ts)
    z0, th = R.inputs(N, B, seed=R.RAGGED_SEED)
    dz = R.cotangent(N, T, B)
    nat = U.native(N)
    nat.set_option("step_trace", 1)
    a = U.run(nat, N, z0, th, ts, dz)
    tr = nat.step_record(0, B, cap=256)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    for b in range(B):   # the grid is what it claims to be: a step with several save times, and steps with none
        t0 = tr["t"][b, :tr["n"][b]]
        per_step = np.histogram(ts[1:], bins=np.append(t0, ts[-1] + 1e-9))[0]
        assert per_step.max() >= 2 and (per_step == 0).sum() >= 1, per_step
    zr, Jr, retr, _ = R.solve(N, z0, th, ts, steps=U.steps_of(tr))
    assert (retr == 0).all()
    r0, rth = R.pullback(N, Jr, dz)
    U.gates(f"N {N} ragged grid", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)


@pytest.mark.parametrize("N", NS)
def test_save_grid_outside_lds(N):
    """T = DUAL_TS_LDS_MAX + 1 save times 1e-3 apart (the grid is read from global memory), B = 3, Tsit5 at the fixed step 0.0125: against the
    reference; and the first 88 save points — those before the T = 100 solve's clipped last step, which starts at 0.0875 — are the bits of
    the T = 100 solve, whose grid is in LDS."""
    T, B, dt = DUAL_TS_LDS_MAX + 1, 3, 0.0125
    NP = R.dims(N)[2]
    ts = 1e-3 * np.arange(T)
    z0, th = R.inputs(N, B, seed=R.LONG_SEED)
    dz = R.cotangent(N, T, B)
    nat = U.fixed(N, R.TSIT5, dt)
    a = U.run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    zr, Jr, retr, info = R.solve(N, z0, th, ts, R.TSIT5, adaptive=False, dt=dt)
    r0, rth = R.pullback(N, Jr, dz)
    U.gates(f"N {N} T = 6001 (grid in global memory)", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    assert a["st"]["naccept"] == info["naccept"]
    rec100 = U.Record(nat, N, B, 100)
    z100, ret100, _ = nat.forward(z0, th, ts[:100])
    J100 = rec100.JG()[..., :NP]
    assert (ret100 == 0).all()
    assert np.array_equal(z100[:88], a["z"][:88]) and np.array_equal(J100[:88], a["J"][:88])
    assert U.rel(z100, zr[:100]) <= R.BOUNDS[0] and U.rel(J100, Jr[:100]) <= R.BOUNDS[1]


def _bits_of_shards(N, T, cuts, seed):
    """One call over [0, cuts[-1]) against the calls over the shards between the cuts: every output bit for bit. The adaptive solve: step
    control included."""
    Btot = cuts[-1]
    ts = R.grid(T)
    dz = R.cotangent(N, T, Btot)
    z0, th = R.inputs(N, Btot, seed=seed)
    nat = U.native(N)
    whole = U.run(nat, N, z0, th, ts, dz)
    assert (whole["ret"] == 0).all() and np.isfinite(whole["J"]).all()
    for lo, hi in zip([0] + list(cuts[:-1]), cuts):
        part = U.run(nat, N, z0[lo:hi], th[lo:hi], ts, dz[:, lo:hi])
        assert np.array_equal(part["z"], whole["z"][:, lo:hi]) and np.array_equal(part["J"], whole["J"][:, lo:hi]), (lo, hi)
        assert np.array_equal(part["g0"], whole["g0"][lo:hi]) and np.array_equal(part["gth"], whole["gth"][lo:hi]), (lo, hi)
        assert np.array_equal(part["n"], whole["n"][lo:hi]) and np.array_equal(part["ret"], whole["ret"][lo:hi])


@pytest.mark.parametrize("N", NS)
def test_shards_are_the_bits_of_the_whole_batch(N):
    """B = 37 as one call against 18 + 19: the second shard's groups sit at other positions of their waves (and in other waves) than in the
    whole batch."""
    _bits_of_shards(N, 20, [18, 37], seed=11)


@pytest.mark.parametrize("N", NS)
def test_batch_across_the_lane_threshold(N):
    """B·G = 4 096 lanes (B = 512 at N = 1, 256 at N = 2, 3) run in 64-lane workgroups, one trajectory more in 256-lane ones: the first B
    trajectories are the same bits, and the last one — alone in the last workgroup's first group — is the bits of its own one-trajectory solve."""
    B = 4096 // R.GROUP[N]
    _bits_of_shards(N, 9, [B, B + 1], seed=12)


@pytest.mark.parametrize("N", NS)
def test_a_failing_neighbour_leaves_its_wave_alone(N):
    """One trajectory of 37 gets a NaN in its θ (its coupling G): it returns LDE_RET_NONFINITE, a NaN block, zero J and a zero gradient
    (whatever its cotangent holds) — and every other trajectory, those of its wave included, is the run without it, bit for bit."""
    B, T, bad = 37, 20, 5
    ts, dz = R.grid(T), np.array(R.cotangent(N, T, B))
    z0, th = R.inputs(N, B, seed=19)
    nat = U.native(N)
    good = U.run(nat, N, z0, th, ts, dz)
    assert (good["ret"] == 0).all()
    thb = th.copy()
    thb[bad, 2 * N] = np.nan
    dzb = dz.copy()
    dzb[1:, bad] = np.nan                                             # (what a loss of a NaN block hands back)
    a = U.run(nat, N, z0, thb, ts, dzb)
    others = np.arange(B) != bad
    assert a["ret"][bad] == R.RET_NONFINITE and (a["ret"][others] == 0).all() and a["st"]["nfailed"] == 1 and a["sta"]["nfailed"] == 1
    assert np.isnan(a["z"][:, bad]).all() and (a["J"][:, bad] == 0).all() and a["n"][bad] == -R.RET_NONFINITE
    assert (a["g0"][bad] == 0).all() and (a["gth"][bad] == 0).all()
    for key in ("z", "J"):
        assert np.array_equal(a[key][:, others], good[key][:, others]), key
    for key in ("g0", "gth", "n"):
        assert np.array_equal(a[key][others], good[key][others]), key


@pytest.mark.parametrize("N", NS)
def test_captured_pair_replays_bit_for_bit(N):
    """lde_reserve, an eager forward + pullback, then the pair captured on one stream: the replay writes the eager bits."""
    import torch
    from latentdiffeq_amd import _lib as L
    D, P, _ = R.dims(N)
    B, T = 300, 20
    nat = U.native(N)
    lib = nat.lib
    L.check(lib.lde_reserve(nat.h, B, T), nat.h, "lde_reserve")
    ts = R.grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = R.inputs(N, B, seed=3)
    z0d, thd, dzd = (torch.from_numpy(a).to("cuda") for a in (z0, th, R.cotangent(N, T, B)))
    rec = U.Record(nat, N, B, T)
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


@pytest.mark.parametrize("N", NS)
def test_torch_autograd_equals_the_c_abi(N):
    """StuartLandau(N) through autograd: ẑ₀ [2N, B] and θ̂ [2N + 1, B] in, gradients of those shapes out; ẑ, dz0 and dθ are the C ABI's bit for
    bit (transform_after_diffeq is the identity); another sensealg is refused with the library's text."""
    import torch
    import latentdiffeq_amd as la
    D, P, _ = R.dims(N)
    B, T = 75, 20
    ts = R.grid(T)
    sl = la.StuartLandau(N)
    dec = la.Decoder(la.GOKU_basic(), (None, sl, None))
    z0, th = R.inputs(N, B, seed=1)
    dz = R.cotangent(N, T, B, seed=11)
    dzt = torch.tensor(dz, device="cuda")
    nat = U.native(N)
    zc, ret, _ = nat.forward(z0, th, ts)
    assert (ret == 0).all()
    g0, gth, _, _ = nat.adjoint(zc, th, ts, dz)
    z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
    tht = torch.tensor(th.T.copy(), device="cuda", requires_grad=True)
    assert z0t.shape == (D, B) and tht.shape == (P, B)
    zhat = la.diffeq_layer(dec, (z0t, tht), ts)                       # [2N, B, T]
    assert zhat.shape == (D, B, T)
    assert np.array_equal(zhat.detach().permute(2, 1, 0).cpu().numpy(), zc)
    (zhat * dzt.permute(2, 1, 0)).sum().backward()
    torch.cuda.synchronize()
    assert z0t.grad.shape == (D, B) and tht.grad.shape == (P, B)
    assert np.array_equal(z0t.grad.cpu().numpy().T, g0) and np.array_equal(tht.grad.cpu().numpy().T, gth) and np.abs(gth).max() > 0
    h = sl._native()
    assert h.lib.lde_last_kernel(h.ptr, 0) == b"k_forward_dual_dir" and h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
    for other in (la.BacksolveAdjoint(), la.ForwardDiffSensitivity(), la.ParallelAdjoint()):
        with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
            la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.StuartLandau(N, sensealg=other), None)), (z0t, tht), ts)


@pytest.mark.parametrize("N", NS)
def test_loss_batch_trains_end_to_end(N):
    """A LatentDiffEqModel with the plug-in and the head its docstring names: 28×28 input, B = 8, T = 10; loss_batch forward and backward
    leave a finite gradient of its parameter's shape on every parameter, lo_z₀ is 2N wide and lo_θ the (2N+1)-wide identity head, lo_θ's
    gradient is not zero, and a gradient step moves lo_θ."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import train as TR
    torch.manual_seed(0)
    D, P, _ = R.dims(N)
    B, T = 8, 10
    mt, sl = la.GOKU_basic(), la.StuartLandau(N)
    enc, dec = TR.default_layers(mt, 784, sl, device="cuda", theta_activation="identity")
    assert tuple(dec[0][0].sizes) == (16, 200, D) and tuple(dec[0][1].sizes) == (16, 200, P)
    assert dec[0][1].acts[-1] == L.CACT_IDENTITY
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
    h = sl._native()
    assert h.lib.lde_last_kernel(h.ptr, 1) == b"k_adjoint_dual_dir"
