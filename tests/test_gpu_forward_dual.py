"""GPU parity of LDE_SENSE_FORWARD_DUAL (k_pend_forward_dual / k_pend_adjoint_dual) against the oracle's dual solve with the dual-aware
norm (oracle_forward_dual, dual_norm = 1) — ForwardDiffSensitivity as the reference executes it during training
[REF examples/pendulum_friction-less/pendulum.jl:8-11], [REF src/models/GOKU.jl:107, :121].

  * same steps: the kernel's accepted steps (option "step_trace") replayed in the f32 and f64 oracles: ẑ within 2e-5, J within 1e-4 of each
    column's largest |J|, dz0 / dθ within 1e-4 of their largest entry;
  * it is the dual-norm controller: the first accepted dt is the dual-norm oracle's (≥ 99 % of trajectories to 1e-4 relative) and differs
    from the primal controller's wherever the two oracle runs do; free-running, the gates of test_gpu_pendulum.py::test_forward_matches_oracle
    against the dual-norm oracle;
  * failure semantics, determinism, graph capture, the torch path.
The J of a solve is read from a dual record the test hands over (include/lde.h: the layout)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _native(**kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc, copy_desc_to_oracle
    kw.setdefault("sensealg", L.SENSE_FORWARD_DUAL)
    d = make_desc(**kw)
    return Native(d), copy_desc_to_oracle(d)


def _a256(x):
    return (x + 255) // 256 * 256


class _Record:
    """A dual record owned by the test (lde_set_step_record), so that J can be read back: n [B] | J [T][2][3][B] | (t, dt)."""

    def __init__(self, nat, B, T):
        import torch
        from latentdiffeq_amd import _lib as L
        self.B, self.T = B, T
        nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
        assert nbytes >= _a256(4 * B) + 24 * T * B
        self.buf = torch.zeros((nbytes,), device="cuda", dtype=torch.uint8)
        L.check(nat.lib.lde_set_step_record(nat.h, C.c_void_p(self.buf.data_ptr()), nbytes), nat.h, "lde_set_step_record")

    def n(self):
        import torch
        return self.buf[:4 * self.B].view(torch.int32).cpu().numpy()

    def J(self):
        """[T, B, 2, 3] (the oracle's J layout)."""
        import torch
        off = _a256(4 * self.B)
        raw = self.buf[off:off + 24 * self.T * self.B].view(torch.float32).cpu().numpy()
        return raw.reshape(self.T, 2, 3, self.B).transpose(0, 3, 1, 2).copy()


def _case(case):
    return {"metric": {}, "friction": dict(rhs_kind=O.RHS_PENDULUM_FRICTION),
            "rk4": dict(solver=O.SOLVER_RK4, adaptive=0, dt=0.013)}[case]


def _col_err(a, b):
    return [np.abs(a[..., q] - b[..., q]).max() / max(np.abs(b[..., q]).max(), 1e-30) for q in range(b.shape[-1])]


def _replay_gates(od, o32, o64, z0, L, ts, dz, z, J, g0, gL, tr, idx=None):
    """The kernel's steps replayed in both oracles (on the trajectories `idx`)."""
    if idx is not None:
        z0, L, dz, z, J, g0, gL = z0[idx], L[idx], dz[:, idx], z[:, idx], J[:, idx], g0[idx], gL[idx]
        tr = dict(t=tr["t"][idx], dt=tr["dt"][idx], n=tr["n"][idx])
    for orc in (o32, o64):
        zr, Jr, (r0, rL), retr, _, _ = orc.forward_dual(od, z0, L, ts, dz_out=dz, dual_norm=True, rec=tr)
        assert (retr == 0).all()
        print(f"replay {orc.dtype.__name__}: |z - ref| {np.abs(z - zr).max():.2e}, J columns {max(_col_err(J, Jr)):.2e}, "
              f"dz0 {np.abs(g0 - r0).max() / np.abs(r0).max():.2e}, dtheta {np.abs(gL - rL).max() / np.abs(rL).max():.2e}")
        assert np.abs(z - zr).max() <= 2e-5, np.abs(z - zr).max()
        assert max(_col_err(J, Jr)) <= 1e-4, _col_err(J, Jr)
        assert np.abs(g0 - r0).max() <= 1e-4 * np.abs(r0).max()
        assert np.abs(gL - rL).max() <= 1e-4 * np.abs(rL).max()


@pytest.mark.parametrize("case", ["metric", "friction", "rk4"])
def test_same_steps_as_the_dual_oracle(o32, o64, case):
    B, T = 256, 50
    nat, od = _native(**_case(case))
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, L = O.pendulum_inputs(B)
    ts = O.time_grid(T)
    dz = O.cotangent(T, B, 2)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, L, ts)
    assert (ret == 0).all() and np.array_equal(z[0], z0)
    J = rec.J()
    g0, gL, _, sta = nat.adjoint(z, L, ts, dz)
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_pend_forward_dual" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_pend_adjoint_dual"
    tr = nat.step_record(0, B, cap=512)
    assert np.array_equal(tr["n"], rec.n()) and st["naccept"] == tr["n"].sum()
    assert sta["nfe"] == 0 and sta["naccept"] == 0 and sta["nfailed"] == 0
    _replay_gates(od, o32, o64, z0, L, ts, dz, z, J, g0, gL, tr)
    # the record never overflows: its capacity is maxiters
    nmax, cap = C.c_int32(0), C.c_int32(0)
    assert nat.lib.lde_step_record_status(nat.h, C.c_void_p(rec.buf.data_ptr()), B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value == tr["n"].max() <= cap.value == 100000


def test_it_is_the_dual_norm_controller(o32, o64):
    """Metric configuration: B = 256, T = 50, Tsit5 1e-6 / 1e-3. The dual-aware initial step sees the seeds, so its first dt differs from the
    primal controller's for most trajectories — and the kernel's is the dual one."""
    B, T = 256, 50
    nat, od = _native()
    nat.set_option("step_trace", 1)
    z0, L = O.pendulum_inputs(B)
    ts = O.time_grid(T)
    z, ret, st = nat.forward(z0, L, ts)
    tr = nat.step_record(0, B, cap=512)
    zd, _, _, retd, recd, infod = o32.forward_dual(od, z0, L, ts, dual_norm=True)
    _, _, _, _, recp, _ = o32.forward_dual(od, z0, L, ts, dual_norm=False)
    assert (ret == 0).all() and (retd == 0).all()
    k1, d1, p1 = tr["dt"][:, 0], recd["dt"][:, 0], recp["dt"][:, 0]
    same = np.abs(k1 - d1) <= 1e-4 * d1
    assert same.mean() >= 0.99, same.mean()
    # the seeds enter the initial step's norms: the two oracle runs' first steps differ beyond the gate above for (nearly) every trajectory
    # (measured: all 256 by > 1e-4, 95 % by > 1e-3, 45 % by > 1e-2) — and wherever they differ by more than 1e-2 the kernel's is not the primal one
    assert (np.abs(d1 - p1) > 1e-4 * d1).mean() >= 0.9
    differ = np.abs(d1 - p1) > 1e-2 * d1
    assert differ.mean() >= 0.25, differ.mean()
    assert (np.abs(k1 - p1)[differ & same] > 5e-3 * p1[differ & same]).all()
    assert (np.abs(k1 - d1) < np.abs(k1 - p1)).mean() >= 0.99
    # free-running: the gates of test_forward_matches_oracle against the dual-norm oracle
    assert abs(st["naccept"] - infod["naccept"]) <= 0.02 * infod["naccept"] + 1
    assert st["nfe"] == 6 * (st["naccept"] + st["nreject"]) + 2 * B
    per_traj = np.abs(z - zd).max(axis=(0, 2))
    assert per_traj.max() <= 3e-4 and np.quantile(per_traj, 0.99) <= 1e-4, (per_traj.max(), np.quantile(per_traj, 0.99))
    zt, _, _ = o64.forward(O.make_desc(abstol=1e-10, reltol=1e-10), z0, L, ts)
    e_k, e_o = np.abs(z - zt).max(), np.abs(zd - zt).max()
    assert e_k <= min(5e-4, 1.5 * e_o + 1e-5), (e_k, e_o)


@pytest.mark.parametrize("B", [1, 7, 1024, 65536])
def test_batch_sizes(o32, o64, B):
    T = 50
    nat, od = _native()
    nat.set_option("step_trace", 1)
    z0, L = O.pendulum_inputs(B, seed=5)
    ts = O.time_grid(T)
    dz = O.cotangent(T, B, 2)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, L, ts)
    assert (ret == 0).all() and np.array_equal(z[0], z0)
    J = rec.J()
    g0, gL, _, _ = nat.adjoint(z, L, ts, dz)
    tr = nat.step_record(0, B, cap=256)
    idx = None if B <= 1024 else np.random.default_rng(0).choice(B, 1024, replace=False)
    _replay_gates(od, o32, o64, z0, L, ts, dz, z, J, g0, gL, tr, idx)
    zs, Ls = (z0, L) if idx is None else (z0[idx], L[idx])
    zd, _, _, _, _, infod = o32.forward_dual(od, zs, Ls, ts, dual_norm=True)
    per_traj = np.abs((z if idx is None else z[:, idx]) - zd).max(axis=(0, 2))
    assert per_traj.max() <= 3e-4 and np.quantile(per_traj, 0.99) <= 1e-4
    nk = tr["n"].sum() if idx is None else tr["n"][idx].sum()
    assert abs(nk - infod["naccept"]) <= 0.02 * infod["naccept"] + 1


def test_save_grid_outside_lds(o32, o64):
    """The pendulum twin of test_gpu_lv.py::test_save_grid_outside_lds: T = DUAL_TS_LDS_MAX + 1 = 6001 save times 1e-3 apart (the kernel reads
    the grid from global memory), B = 3, Tsit5 at the fixed step 0.0125 — 480 steps, a dozen save times inside each — replayed in the f32 and
    f64 oracles through _replay_gates. The first 88 save points — those before the T = 100 solve's clipped last step, which starts at 0.0875
    — are the bits of the solve with the grid in LDS.
    Measured on the MI355X, on the per-system kernels before csrc/lde_dual.hip and again on it (the same figures), f32 / f64 replay:
    |ẑ − ref| 1.2e-6 / 1.3e-6, J columns 1.0e-6 / 9.0e-7, dz0 5.7e-7 / 2.3e-6, dθ 9.6e-7 / 4.7e-7 of the largest entry."""
    T, B, dt = 6001, 3, 0.0125
    ts = 1e-3 * np.arange(T)
    nat, od = _native(adaptive=0, dt=dt)
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    z0, L = O.pendulum_inputs(B, seed=13)
    dz = O.cotangent(T, B, 2)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, L, ts)
    J = rec.J()
    g0, gL, _, _ = nat.adjoint(z, L, ts, dz)
    tr = nat.step_record(0, B, cap=512)
    assert (ret == 0).all() and np.array_equal(z[0], z0)
    assert (tr["n"] == 480).all() and st["naccept"] == 480 * B and st["nfe"] == (6 * 480 + 1) * B
    _replay_gates(od, o32, o64, z0, L, ts, dz, z, J, g0, gL, tr)
    rec100 = _Record(nat, B, 100)
    z100, ret100, _ = nat.forward(z0, L, ts[:100])
    assert (ret100 == 0).all()
    assert np.array_equal(z100[:88], z[:88]) and np.array_equal(rec100.J()[:88], J[:88])


def test_failed_trajectory_gives_nan_block_and_zero_gradient():
    B, T = 8, 20
    nat, _ = _native(maxiters=3)
    z0, L = O.pendulum_inputs(B, seed=2)
    ts = O.time_grid(T)
    rec = _Record(nat, B, T)
    z, ret, st = nat.forward(z0, L, ts)
    assert (ret != 0).all() and np.isnan(z).all() and st["nfailed"] == B
    assert (rec.J() == 0).all() and (rec.n() < 0).all()
    dz = O.cotangent(T, B, 2)
    dz[:, :3] = np.nan                                               # (what a loss of a NaN block hands back)
    g0, gL, _, sta = nat.adjoint(z, L, ts, dz)
    assert (g0 == 0).all() and (gL == 0).all() and sta["nfailed"] == B and sta["nfe"] == 0


def test_deterministic_and_graph_capturable():
    import torch
    from latentdiffeq_amd import _lib as L
    B, T = 512, 50
    nat, _ = _native()
    lib = nat.lib
    ts = O.time_grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, Lp = O.pendulum_inputs(B, seed=3)
    z0d, thd, dzd = (torch.from_numpy(a).to("cuda") for a in (z0, Lp, O.cotangent(T, B, 2)))
    rec = _Record(nat, B, T)
    out = torch.empty((T, B, 2), device="cuda")
    g0, gL = torch.empty((B, 2), device="cuda"), torch.empty((B, 1), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def step():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.lde_forward(nat.h, p(z0d), p(thd), tsp, T, B, p(out), None, s), nat.h, "fwd")
        L.check(lib.lde_adjoint(nat.h, p(out), p(thd), tsp, T, B, p(dzd), p(g0), p(gL), None, s), nat.h, "adj")

    def snap():
        torch.cuda.synchronize()
        return [x.clone() for x in (out, g0, gL, rec.buf)]

    def clobber():
        for x in (out, g0, gL):
            x.fill_(7.0)
        rec.buf.zero_()
        torch.cuda.synchronize()

    step()
    a = snap()
    clobber()
    step()
    b = snap()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs must be bit-identical"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    clobber()
    graph.replay()
    c = snap()
    for x, y in zip(a, c):
        assert torch.equal(x, y), "the replayed graph must equal the eager result bit for bit"


def test_torch_autograd_path(o32):
    """diffeq_layer with Pendulum(sensealg=ForwardDiffSensitivity(dual_norm=True)) returns the dual-norm oracle's (dz0, dθ); two forwards in
    flight before their pullbacks each keep their own J."""
    import torch
    import latentdiffeq_amd as la
    B, T = 64, 50
    ts = O.time_grid(T)
    pend = la.Pendulum(sensealg=la.ForwardDiffSensitivity(dual_norm=True))
    dec = la.Decoder(la.GOKU_basic(), (None, pend, None))
    od = O.make_desc(sensealg=4)
    cases = []
    for seed in (1, 2):
        z0, L = O.pendulum_inputs(B, seed=seed)
        z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
        tht = torch.tensor(L.T.copy(), device="cuda", requires_grad=True)
        zhat = la.diffeq_layer(dec, (z0t, tht), ts)                   # [2, B, T]
        dz = O.cotangent(T, B, 2, seed=10 + seed)
        cases.append((z0, L, dz, z0t, tht, zhat))
    for z0, L, dz, z0t, tht, zhat in reversed(cases):                 # pullbacks in the other order
        (zhat * torch.tensor(dz, device="cuda").permute(2, 1, 0)).sum().backward()
    torch.cuda.synchronize()
    h = pend._native()
    assert h.lib.lde_last_kernel(h.ptr, 1) == b"k_pend_adjoint_dual"
    for z0, L, dz, z0t, tht, zhat in cases:
        zr, _, (r0, rL), _, _, _ = o32.forward_dual(od, z0, L, ts, dz_out=dz, dual_norm=True)
        per_traj = np.abs(zhat.detach().permute(2, 1, 0).cpu().numpy() - zr).max(axis=(0, 2))
        assert np.quantile(per_traj, 0.99) <= 1e-4 and per_traj.max() <= 3e-4
        assert np.abs(z0t.grad.cpu().numpy().T - r0).max() <= 5e-4 * np.abs(r0).max()
        assert np.abs(tht.grad.cpu().numpy().T - rL).max() <= 5e-4 * np.abs(rL).max()
