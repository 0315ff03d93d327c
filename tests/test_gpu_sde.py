"""GPU: the stochastic pendulum (LDE_RHS_SPENDULUM: k_pend_forward_sde + k_pend_adjoint_dual) against the float64 numpy restatement of its
two schemes on dual numbers (tests/sde_ref.py, pinned by tests/test_sde_host.py).

  * parity: |ẑ − ẑ_ref| ≤ 1e-4 (the project's parity bar), dz0 / dθ of a seeded cotangent within 1e-4 of the reference's largest entry (the
    bound of the other pendulum gradients) — both solvers × (T, B) ∈ {(1, 1), (2, 37), (50, 256)} × dt ∈ {0.05, 0.0125}, and a ragged grid;
  * the noise is there and is indexed as include/lde.h says: seed, offset, the device epoch word, first_trajectory; bit-reproducible;
  * the statistics of v(T) − v₀ with the drift switched off; the failure semantics; the Python mirror; graph capture with a device epoch."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sde_ref as S

pytestmark = pytest.mark.gpu

STAT, noise_statistics = S.STAT, S.noise_statistics

NFE = {S.EM: 1, S.EULER_HEUN: 2}


def _native(solver=S.EULER_HEUN, dt=0.05, **kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=L.RHS_SPENDULUM, solver=solver, sensealg=L.SENSE_FORWARD_DUAL, adaptive=0, dt=dt, **kw))


def _set_noise(nat, seed=0, offset=0, first=0, epoch=None):
    from latentdiffeq_amd import _lib as L
    L.check(nat.lib.lde_set_noise(nat.h, seed, offset, first, C.c_void_p(epoch.data_ptr()) if epoch is not None else None), nat.h, "lde_set_noise")


def _grid(name):
    return S.ragged_grid() if name == "ragged" else 0.05 * np.arange(name)


@functools.lru_cache(maxsize=None)
def _ref(solver, grid, B, dt, seed=5, off=0, sigma=S.SIGMA):
    """(z0, L, ts, dz, ẑ_ref, dz0_ref, dθ_ref): computed once per case, shared, never written."""
    ts = _grid(grid)
    z0, L = S.inputs(B, seed=len(ts))
    dz = S.cotangent(len(ts), B)
    z, J, ret = S.solve(z0, L, ts, dt, solver, seed=seed, offset=off, sigma=sigma)
    assert (ret == 0).all()
    g0, gL = S.pullback(J, dz)
    out = (z0, L, ts, dz, z, g0, gL)
    for a in (ts, z, g0, gL):          # (the f32 inputs go through torch.from_numpy, which wants writable arrays; nothing writes them)
        a.setflags(write=False)
    return out


CASES = [(T, B, dt) for T, B in S.SHAPES for dt in S.DTS] + [("ragged", 256, 0.05)]


@pytest.mark.parametrize("grid,B,dt", CASES)
@pytest.mark.parametrize("solver", [S.EM, S.EULER_HEUN])
def test_parity_with_the_f64_reference(solver, grid, B, dt):
    """Worst measured values: DESIGN.md §8.1."""
    z0, L, ts, dz, zr, r0, rL = _ref(solver, grid, B, dt)
    T = len(ts)
    nat = _native(solver, dt)
    _set_noise(nat, seed=5)
    z, ret, st = nat.forward(z0, L, ts)
    g0, gL, _, sta = nat.adjoint(z, L, ts, dz)
    ez = np.abs(z - zr).max()
    e0 = np.abs(g0 - r0).max() / max(np.abs(r0).max(), 1e-300)
    eL = np.abs(gL - rL).max() / max(np.abs(rL).max(), 1e-300)
    print(f"solver {solver} grid {grid} B {B} dt {dt}: |z - ref| {ez:.2e}, dz0 {e0:.2e}, dtheta {eL:.2e} of the largest entry")
    assert (ret == 0).all() and np.array_equal(z[0], z0)
    assert ez <= 1e-4, ez
    assert np.abs(g0 - r0).max() <= 1e-4 * np.abs(r0).max(), e0
    assert np.abs(gL - rL).max() <= 1e-4 * np.abs(rL).max(), eL
    N = sum(n for n, _ in S.plan(ts, dt))
    assert st == dict(nfe=NFE[solver] * N * B, naccept=N * B, nreject=0, nfailed=0, max_steps=N)
    assert sta["nfe"] == 0 and sta["nfailed"] == 0
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_pend_forward_sde" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_pend_adjoint_dual"


@pytest.mark.parametrize("solver", [S.EM, S.EULER_HEUN])
def test_the_noise_is_there(solver):
    """Per trajectory the solve leaves the σ = 0 scheme by more than 5e-3 somewhere (reference on these inputs: ≥ 7.5e-3) — with the seed of
    the parity case and with another one, and the two seeds' paths differ as much."""
    B, dt = 256, 0.05
    z0, L, ts, _, _, _, _ = _ref(solver, 50, B, dt)
    zdet = _ref(solver, 50, B, dt, sigma=0.0)[4]
    nat = _native(solver, dt)
    zs = []
    for seed in (5, 6):
        _set_noise(nat, seed=seed)
        z, ret, _ = nat.forward(z0, L, ts)
        per_traj = np.abs(z - zdet).max(axis=(0, 2))
        print(f"solver {solver} seed {seed}: smallest per-trajectory distance to the deterministic scheme {per_traj.min():.2e}")
        assert (ret == 0).all() and per_traj.min() > 5e-3, per_traj.min()
        zs.append(z)
    assert np.abs(zs[0] - zs[1]).max(axis=(0, 2)).min() > 5e-3


def test_noise_indexing_seed_offset_and_epoch():
    import torch
    B, dt, solver = 256, 0.05, S.EULER_HEUN
    z0, L, ts, _, z_off0, _, _ = _ref(solver, 50, B, dt)
    nat = _native(solver, dt)
    _set_noise(nat, seed=5, offset=0)
    a, _, _ = nat.forward(z0, L, ts)
    b, _, _ = nat.forward(z0, L, ts)
    assert np.array_equal(a, b), "the same (seed, offset) must give the same bits"
    assert np.abs(a - z_off0).max() <= 1e-4
    # another offset: the reference's path for that off, and not the first one
    z_off5 = _ref(solver, 50, B, dt, off=5)[4]
    _set_noise(nat, seed=5, offset=5)
    c, _, _ = nat.forward(z0, L, ts)
    assert np.abs(c - z_off5).max() <= 1e-4 and np.abs(c - a).max(axis=(0, 2)).min() > 5e-3
    # the device epoch word adds to the offset at run time: offset 2 + epoch 3 is offset 5, bit for bit
    ep = torch.tensor([3], device="cuda", dtype=torch.int64)
    _set_noise(nat, seed=5, offset=2, epoch=ep)
    d, _, _ = nat.forward(z0, L, ts)
    assert np.array_equal(d, c)
    ep.fill_(0)
    torch.cuda.synchronize()
    e, _, _ = nat.forward(z0, L, ts)
    assert np.abs(e - _ref(solver, 50, B, dt, off=2)[4]).max() <= 1e-4 and not np.array_equal(e, c)
    # a 64-bit seed and an offset beyond 2³²: both key words and both offset words enter
    seed, off = (3 << 32) | 12345, (1 << 32) + 7
    _set_noise(nat, seed=seed, offset=off)
    f, _, _ = nat.forward(z0, L, ts)
    assert np.abs(f - _ref(solver, 50, B, dt, seed=seed, off=off)[4]).max() <= 1e-4
    with pytest.raises(Exception, match="LDE_ERR_UNSUPPORTED"):   # a deterministic handle takes no noise
        from tests.gpu_util import make_desc, Native
        _set_noise(Native(make_desc()), seed=1)


@pytest.mark.parametrize("B,T", [(74, 9), (8192, 6)])
def test_two_halves_with_first_trajectory_equal_the_whole(B, T):
    """Nothing depends on the launch geometry: 8192 trajectories run in 256-lane workgroups, their halves in 64-lane ones."""
    ts = 0.05 * np.arange(T)
    z0, L = S.inputs(B, seed=B)
    dz = S.cotangent(T, B)
    nat = _native(S.EULER_HEUN, 0.0125)
    _set_noise(nat, seed=9, offset=1)
    z, ret, _ = nat.forward(z0, L, ts)
    g0, gL, _, _ = nat.adjoint(z, L, ts, dz)
    assert (ret == 0).all()
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        _set_noise(nat, seed=9, offset=1, first=lo)
        zh, _, _ = nat.forward(z0[lo:hi], L[lo:hi], ts)
        h0, hL, _, _ = nat.adjoint(zh, L[lo:hi], ts, dz[:, lo:hi])
        assert np.array_equal(zh, z[:, lo:hi]) and np.array_equal(h0, g0[lo:hi]) and np.array_equal(hL, gL[lo:hi])
    _set_noise(nat, seed=9, offset=1, first=0)
    zw, _, _ = nat.forward(z0[h:], L[h:], ts)
    assert not np.array_equal(zw, z[:, h:]), "first_trajectory must enter the counter"


@pytest.mark.parametrize("solver", [S.EM, S.EULER_HEUN])
def test_noise_statistics_on_the_gpu(solver):
    """tests/test_sde_host.py's case 3 with the kernel's f32 path: the same bounds."""
    B = STAT["B"]
    z0 = np.zeros((B, 2), np.float32)
    z0[:, 1] = STAT["v0"]
    nat = _native(solver, STAT["dt"])
    _set_noise(nat, seed=STAT["seed"])
    z, ret, _ = nat.forward(z0, np.full((B, 1), STAT["L"], np.float32), STAT["ts"])
    m, v = noise_statistics(z[-1, :, 1], np.float64(np.float32(STAT["v0"])), STAT["ts"][-1], B)
    print(f"solver {solver}: mean {m:+.2f} standard errors, variance {v:+.2f} units of sqrt(2/B)")
    assert (ret == 0).all() and abs(m) <= 4 and abs(v) <= 4, (m, v)


def test_maxiters_gives_nan_blocks_and_zero_gradients():
    B, T = 37, 50
    ts = 0.05 * np.arange(T)                                         # 49 substeps against maxiters = 10
    z0, L = S.inputs(B, seed=2)
    nat = _native(S.EULER_HEUN, 0.05, maxiters=10)
    z, ret, st = nat.forward(z0, L, ts)
    assert (ret == 1).all() and np.isnan(z).all() and st["nfailed"] == B      # LDE_RET_MAXITERS
    dz = np.array(S.cotangent(T, B))
    dz[:, :3] = np.nan                                               # (what a loss of a NaN block hands back)
    g0, gL, _, sta = nat.adjoint(z, L, ts, dz)
    assert (g0 == 0).all() and (gL == 0).all() and sta["nfailed"] == B
    nmax, cap = C.c_int32(-1), C.c_int32(-1)
    assert nat.lib.lde_step_record_status(nat.h, None, B, T, C.byref(nmax), C.byref(cap), None) == 0
    assert nmax.value <= cap.value == 10                             # a dual record never reports an overflow
    nat49 = _native(S.EULER_HEUN, 0.05, maxiters=49)                 # exactly maxiters substeps are a solve
    z, ret, st = nat49.forward(z0, L, ts)
    assert (ret == 0).all() and np.isfinite(z).all() and st["naccept"] == 49 * B


def test_python_mirror_matches_the_c_abi_and_draws_fresh_noise():
    import torch
    import latentdiffeq_amd as la
    B, T = 75, 20
    ts = 0.05 * np.arange(T)
    z0, L = S.inputs(B, seed=8)
    dz = S.cotangent(T, B)
    sp = la.SPendulum(seed=4)
    dec = la.Decoder(la.GOKU_basic(), (None, sp, None))
    z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
    tht = torch.tensor(L.T.copy(), device="cuda", requires_grad=True)
    dzt = torch.tensor(dz, device="cuda").permute(2, 1, 0)
    z1 = la.diffeq_layer(dec, (z0t, tht), ts)                        # [2, B, T], offset 0
    z2 = la.diffeq_layer(dec, (z0t, tht), ts)                        # offset 1: fresh noise
    (z1 * dzt).sum().backward()                                      # the pullback of the FIRST forward, after the second one ran
    torch.cuda.synchronize()
    nat = _native(S.EULER_HEUN, 0.05)
    _set_noise(nat, seed=4, offset=0)
    zc, ret, _ = nat.forward(z0, L, ts)
    g0, gL, _, _ = nat.adjoint(zc, L, ts, dz)
    assert np.array_equal(z1.detach().permute(2, 1, 0).cpu().numpy(), zc)
    assert np.array_equal(z0t.grad.cpu().numpy().T, g0) and np.array_equal(tht.grad.cpu().numpy().T, gL)
    assert (z1 - z2).detach().abs().amax(dim=(0, 2)).min().item() > 1e-3, "two consecutive forward calls must differ"
    sp.reseed(4)
    z3 = la.diffeq_layer(dec, (z0t, tht), ts)
    z4 = la.diffeq_layer(dec, (z0t, tht), ts)
    assert torch.equal(z3, z1) and torch.equal(z4, z2), "after reseed the sequence repeats"
    # sharded by trajectory: each shard passes its first global index, the shards draw the whole batch's path
    from latentdiffeq_amd import dist
    parts = []
    for rank in range(2):
        dr = la.Decoder(la.GOKU_basic(), (None, la.SPendulum(seed=4), None))
        parts.append(dist.diffeq_layer_sharded(dr, (z0t, tht), ts, rank=rank, world=2))
        assert dr.diffeq.first_trajectory == (0, 38)[rank]
    assert torch.equal(torch.cat(parts, dim=1), z1)
    # another sensealg is refused with the library's advice
    with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
        la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.SPendulum(sensealg=la.BacksolveAdjoint()), None)), (z0t, tht), ts)


def test_captured_pair_replays_each_epochs_path():
    """lde_reserve, then a forward + pullback pair captured on one stream: every replay reads the device epoch word and draws the reference's
    path for that offset — bit for bit what the eager pair gives at that epoch."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    B, dt, solver = 256, 0.05, S.EULER_HEUN
    z0, Lp, ts, dz, _, _, _ = _ref(solver, 50, B, dt)
    T = len(ts)
    ep = torch.zeros(1, device="cuda", dtype=torch.int64)
    sp = la.SPendulum(seed=5, epoch=ep)
    h = sp._native()
    lib = h.lib
    L.check(lib.lde_reserve(h.ptr, B, T), h.ptr, "lde_reserve")
    L.check(lib.lde_set_noise(h.ptr, 5, 0, 0, C.c_void_p(ep.data_ptr())), h.ptr, "lde_set_noise")
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0d, thd, dzd = (torch.from_numpy(np.array(a)).to("cuda") for a in (z0, Lp, dz))
    out = torch.empty((T, B, 2), device="cuda")
    g0, gL = torch.empty((B, 2), device="cuda"), torch.empty((B, 1), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def step():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.lde_forward(h.ptr, p(z0d), p(thd), tsp, T, B, p(out), None, s), h.ptr, "fwd")
        L.check(lib.lde_adjoint(h.ptr, p(out), p(thd), tsp, T, B, p(dzd), p(g0), p(gL), None, s), h.ptr, "adj")

    def snap():
        torch.cuda.synchronize()
        return [x.clone() for x in (out, g0, gL)]

    eager = []
    for e in range(3):
        ep.fill_(e)
        step()
        eager.append(snap())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for e in (2, 0, 1):
        ep.fill_(e)
        for x in (out, g0, gL):
            x.fill_(7.0)
        graph.replay()
        got = snap()
        for x, y in zip(got, eager[e]):
            assert torch.equal(x, y), "a replay must equal the eager pair at that epoch bit for bit"
        zr, r0 = _ref(solver, 50, B, dt, off=e)[4:6]
        assert np.abs(got[0].cpu().numpy() - zr).max() <= 1e-4
        assert np.abs(got[1].cpu().numpy() - r0).max() <= 1e-4 * np.abs(r0).max()
