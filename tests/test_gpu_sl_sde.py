"""GPU: the stochastic Stuart–Landau network (LDE_RHS_STUART_LANDAU under LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN: k_forward_sde_dir of
csrc/lde_dual_dir.hip — the stochastic pendulum's stepper in the lane-per-direction frame, every lane of a group drawing the same ΔW from the
same counter — and k_adjoint_dual_dir on the record it leaves) against the float64 numpy restatement of the two schemes on dual numbers along
the path of the counter layout (tests/sl_ref.py: sde_solve, pinned on the CPU by tests/test_sl_host.py).

  * parity of ẑ, J, dz0 and dθ at the project's standing bounds (ẑ 2e-5, J / dz0 / dθ 1e-4 of the reference's largest entry; the reference's own
    f32 mode stays within a twentieth of them: tests/sl_ref.py) — both solvers × N ∈ {1, 2, 3} × (T, B) ∈ {(1, 1), (2, 37), (50, 256)} ×
    dt ∈ {0.05, 0.0125}, and a ragged grid; parity of J is also what catches lanes of a group that drew different noise: the values a lane
    differentiates would not be the values lane 0 saved;
  * σ = 0 is the deterministic scheme; the noise is there and is indexed as include/lde.h says: seed, offset, the device epoch word,
    first_trajectory; bit-reproducible; the second Philox block of N = 3;
  * the statistics of z(t_end) with the drift all but switched off; the failure semantics; the Python mirror; graph capture with a device epoch.
Worst measured on the MI355X: DESIGN.md §8.7.

Every test here creates a handle of rhs_kind = 13 (or la.StuartLandau), which lde_create refuses with LDE_ERR_INVALID_ARG ("unknown rhs_kind")
before this right-hand side existed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sl_gpu as U
from tests import sl_ref as R

pytestmark = pytest.mark.gpu

NS = R.NS
SOLVERS = [R.EM, R.EULER_HEUN]
NFE = {R.EM: 1, R.EULER_HEUN: 2}
SEED = R.NOISE_SEED


def _grid(name):
    return R.sde_ragged_grid() if name == "ragged" else R.grid(name)


@functools.lru_cache(maxsize=None)
def _ref(N, solver, grid, B, dt, seed=SEED, off=0, sigma=R.SIGMA):
    """(z0, θ, ts, dz, ẑ_ref, J_ref, dz0_ref, dθ_ref): computed once per case in f64, shared, never written."""
    ts = _grid(grid)
    z0, th = R.inputs(N, B, seed=R.SDE_RAGGED_SEED if grid == "ragged" else R.PARITY_SEED[grid])
    dz = R.cotangent(N, len(ts), B)
    z, J, ret = R.sde_solve(N, z0, th, ts, dt, solver, seed=seed, offset=off, sigma=sigma)
    assert (ret == 0).all()
    g0, gth = R.pullback(N, J, dz)
    for a in (ts, z, J, g0, gth):
        a.setflags(write=False)
    return z0, th, ts, dz, z, J, g0, gth


CASES = [(T, B, dt) for T, B in R.SHAPES for dt in R.DTS] + [("ragged", 256, 0.05)]


@pytest.mark.parametrize("grid,B,dt", CASES)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("N", NS)
def test_parity_with_the_f64_reference(N, solver, grid, B, dt):
    z0, th, ts, dz, zr, Jr, r0, rth = _ref(N, solver, grid, B, dt)
    T = len(ts)
    nat = U.fixed(N, solver, dt)
    U.set_noise(nat, seed=SEED)
    a = U.run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all() and np.array_equal(a["z"][0], z0)
    if T == 1:      # (1, 1) is exact: ẑ₀ itself and the seeds
        assert np.array_equal(a["z"], zr.astype(np.float32)) and np.array_equal(a["J"], Jr.astype(np.float32))
        assert np.array_equal(a["g0"], r0.astype(np.float32)) and (a["gth"] == 0).all() and (rth == 0).all()
    U.gates(f"N {N} solver {solver} grid {grid} B {B} dt {dt}", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    if grid == "ragged":
        ns = [n for n, _ in R.plan(ts, dt)]
        assert min(ns) == 1 and max(ns) == 3, ns
    Nsub = sum(n for n, _ in R.plan(ts, dt))
    assert a["st"] == dict(nfe=NFE[solver] * Nsub * B, naccept=Nsub * B, nreject=0, nfailed=0, max_steps=Nsub)
    assert (a["n"] == Nsub).all() and a["sta"]["nfe"] == 0 and a["sta"]["nfailed"] == 0
    assert nat.lib.lde_last_kernel(nat.h, 0) == b"k_forward_sde_dir" and nat.lib.lde_last_kernel(nat.h, 1) == b"k_adjoint_dual_dir"


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("N", NS)
def test_sigma_zero_is_the_deterministic_scheme(N, solver):
    """Option "noise_sigma" = 0: the reference's deterministic scheme on the same substeps, whatever the seed; the option reads back, and its
    default is the pendulum's 0.01."""
    z0, th, ts, dz, zr, Jr, r0, rth = _ref(N, solver, 50, 256, 0.05, sigma=0.0)
    nat = U.fixed(N, solver, 0.05)
    v = C.c_double(-1.0)
    assert nat.lib.lde_get_option(nat.h, b"noise_sigma", C.byref(v)) == 0 and v.value == 0.01
    nat.set_option("noise_sigma", 0.0)
    assert nat.lib.lde_get_option(nat.h, b"noise_sigma", C.byref(v)) == 0 and v.value == 0.0
    U.set_noise(nat, seed=SEED)
    a = U.run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == 0).all()
    U.gates(f"N {N} solver {solver} sigma 0", a["z"], a["J"], a["g0"], a["gth"], zr, Jr, r0, rth)
    U.set_noise(nat, seed=SEED + 1, offset=3)
    b, _, _ = nat.forward(z0, th, ts)
    assert np.array_equal(b, a["z"]), "without noise the seed does not enter"
    nat.set_option("noise_sigma", 0.02)                               # another σ: the reference's path for it
    U.set_noise(nat, seed=SEED)
    c, _, _ = nat.forward(z0, th, ts)
    assert U.rel(c, _ref(N, solver, 50, 256, 0.05, sigma=0.02)[4]) <= R.BOUNDS[0]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("N", NS)
def test_the_noise_is_there(N, solver):
    """Per trajectory the solve leaves the σ = 0 scheme by more than R.MIN_DEPARTURE somewhere (two thirds of the reference's smallest
    departure on these inputs, measured on the CPU) — with the seed of the parity case and with another one, and the two seeds' paths differ
    as much."""
    B, dt = 256, 0.05
    z0, th, ts = _ref(N, solver, 50, B, dt)[:3]
    zdet = _ref(N, solver, 50, B, dt, sigma=0.0)[4]
    nat = U.fixed(N, solver, dt)
    zs = []
    for seed in (SEED, SEED + 1):
        U.set_noise(nat, seed=seed)
        z, ret, _ = nat.forward(z0, th, ts)
        per_traj = np.abs(z - zdet).max(axis=(0, 2))
        print(f"N {N} solver {solver} seed {seed}: smallest per-trajectory distance to the deterministic scheme {per_traj.min():.2e}")
        assert (ret == 0).all() and per_traj.min() > R.MIN_DEPARTURE, per_traj.min()
        zs.append(z)
    assert np.abs(zs[0] - zs[1]).max(axis=(0, 2)).min() > R.MIN_DEPARTURE


@pytest.mark.parametrize("N", NS)
def test_noise_indexing_seed_offset_and_epoch(N):
    import torch
    B, dt, solver = 256, 0.05, R.EULER_HEUN
    z0, th, ts, _, z_off0 = _ref(N, solver, 50, B, dt)[:5]
    tol = R.BOUNDS[0]
    nat = U.fixed(N, solver, dt)
    U.set_noise(nat, seed=SEED, offset=0)
    a, _, _ = nat.forward(z0, th, ts)
    b, _, _ = nat.forward(z0, th, ts)
    assert np.array_equal(a, b), "the same (seed, offset) must give the same bits"
    assert U.rel(a, z_off0) <= tol
    # another offset: the reference's path for that off, and not the first one
    z_off5 = _ref(N, solver, 50, B, dt, off=5)[4]
    U.set_noise(nat, seed=SEED, offset=5)
    c, _, _ = nat.forward(z0, th, ts)
    assert U.rel(c, z_off5) <= tol and np.abs(c - a).max(axis=(0, 2)).min() > R.MIN_DEPARTURE
    # the device epoch word adds to the offset at run time: offset 2 + epoch 3 is offset 5, bit for bit
    ep = torch.tensor([3], device="cuda", dtype=torch.int64)
    U.set_noise(nat, seed=SEED, offset=2, epoch=ep)
    d, _, _ = nat.forward(z0, th, ts)
    assert np.array_equal(d, c)
    ep.fill_(0)
    torch.cuda.synchronize()
    e, _, _ = nat.forward(z0, th, ts)
    assert U.rel(e, _ref(N, solver, 50, B, dt, off=2)[4]) <= tol and not np.array_equal(e, c)
    # a 64-bit seed and an offset beyond 2³²: both key words and both offset words enter (N = 3: block 1's key flips the seed's top bit)
    for seed, off in (((3 << 32) | 12345, (1 << 32) + 7), ((1 << 63) | (5 << 32) | 99, (7 << 32) + 1)):
        U.set_noise(nat, seed=seed, offset=off)
        f, _, _ = nat.forward(z0, th, ts)
        assert U.rel(f, _ref(N, solver, 50, B, dt, seed=seed, off=off)[4]) <= tol
    # a deterministic handle of this kind takes lde_set_noise and ignores it
    det = U.native(N)
    U.set_noise(det, seed=1)


@pytest.mark.parametrize("N,B,T", [(1, 74, 9), (1, 1024, 6), (2, 74, 9), (2, 512, 6), (3, 74, 9), (3, 512, 6)])
def test_two_halves_with_first_trajectory_equal_the_whole(N, B, T):
    """Nothing depends on the launch geometry: B·G > 4 096 lanes run in 256-lane workgroups, their halves in 64-lane ones."""
    ts = R.grid(T)
    z0, th = R.inputs(N, B, seed=B)
    dz = R.cotangent(N, T, B)
    nat = U.fixed(N, R.EULER_HEUN, 0.0125)
    if B > 74:
        assert B * R.GROUP[N] > 4096 >= B // 2 * R.GROUP[N]
    U.set_noise(nat, seed=9, offset=1)
    w = U.run(nat, N, z0, th, ts, dz)
    assert (w["ret"] == 0).all()
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        U.set_noise(nat, seed=9, offset=1, first=lo)
        p = U.run(nat, N, z0[lo:hi], th[lo:hi], ts, dz[:, lo:hi])
        assert np.array_equal(p["z"], w["z"][:, lo:hi]) and np.array_equal(p["J"], w["J"][:, lo:hi])
        assert np.array_equal(p["g0"], w["g0"][lo:hi]) and np.array_equal(p["gth"], w["gth"][lo:hi])
    U.set_noise(nat, seed=9, offset=1, first=0)
    zw, _, _ = nat.forward(z0[h:], th[h:], ts)
    assert not np.array_equal(zw, w["z"][:, h:]), "first_trajectory must enter the counter"


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("N", NS)
def test_noise_statistics_on_the_gpu(N, solver):
    """tests/test_sl_host.py's statistics case with the kernel's f32 path: ẑ₀ = 0 and θ = 0, so z(t_end) is the noise sum to about 1e-4
    relative; mean and variance of every component within tests/test_gpu_sde.py's gates."""
    B, ts = R.STAT["B"], R.STAT["ts"]
    nat = U.fixed(N, solver, R.STAT["dt"])
    U.set_noise(nat, seed=R.STAT["seed"])
    z, ret, _ = nat.forward(np.zeros((B, 2 * N), np.float32), np.zeros((B, 2 * N + 1), np.float32), ts)
    m, v = R.noise_statistics(z[-1], ts[-1], B)
    print(f"N {N} solver {solver}: means {np.round(m, 2)} standard errors, variances {np.round(v, 2)} units of sqrt(2/B)")
    assert (ret == 0).all() and (np.abs(m) <= 4).all() and (np.abs(v) <= 4).all(), (m, v)


@pytest.mark.parametrize("N", NS)
def test_maxiters_gives_nan_blocks_and_zero_gradients(N):
    B, T = 37, 50
    ts = R.grid(T)                                                   # 49 substeps against maxiters = 10
    z0, th = R.inputs(N, B, seed=2)
    nat = U.fixed(N, R.EULER_HEUN, 0.05, maxiters=10)
    dz = np.array(R.cotangent(N, T, B))
    dz[:, :3] = np.nan                                               # (what a loss of a NaN block hands back)
    a = U.run(nat, N, z0, th, ts, dz)
    assert (a["ret"] == R.RET_MAXITERS).all() and np.isnan(a["z"]).all() and a["st"]["nfailed"] == B
    assert (a["J"] == 0).all() and (a["n"] == -R.RET_MAXITERS).all()
    assert (a["g0"] == 0).all() and (a["gth"] == 0).all() and a["sta"]["nfailed"] == B
    nat49 = U.fixed(N, R.EULER_HEUN, 0.05, maxiters=49)              # exactly maxiters substeps are a solve
    z, ret, st = nat49.forward(z0, th, ts)
    assert (ret == 0).all() and np.isfinite(z).all() and st["naccept"] == 49 * B


@pytest.mark.parametrize("N", NS)
def test_python_mirror_matches_the_c_abi_and_draws_fresh_noise(N):
    import torch
    import latentdiffeq_amd as la
    B, T = 75, 20
    ts = R.grid(T)
    z0, th = R.inputs(N, B, seed=8)
    dz = R.cotangent(N, T, B)
    sp = la.StuartLandau(N, solver=la.EulerHeun(), seed=4)
    dec = la.Decoder(la.GOKU_basic(), (None, sp, None))
    z0t = torch.tensor(z0.T.copy(), device="cuda", requires_grad=True)
    tht = torch.tensor(th.T.copy(), device="cuda", requires_grad=True)
    dzt = torch.tensor(dz, device="cuda").permute(2, 1, 0)
    z1 = la.diffeq_layer(dec, (z0t, tht), ts)                        # [2N, B, T], offset 0
    z2 = la.diffeq_layer(dec, (z0t, tht), ts)                        # offset 1: fresh noise
    (z1 * dzt).sum().backward()                                      # the pullback of the FIRST forward, after the second one ran
    torch.cuda.synchronize()
    nat = U.fixed(N, R.EULER_HEUN, 0.05)
    U.set_noise(nat, seed=4, offset=0)
    zc, ret, _ = nat.forward(z0, th, ts)
    g0, gth, _, _ = nat.adjoint(zc, th, ts, dz)
    assert np.array_equal(z1.detach().permute(2, 1, 0).cpu().numpy(), zc)
    assert np.array_equal(z0t.grad.cpu().numpy().T, g0) and np.array_equal(tht.grad.cpu().numpy().T, gth)
    assert (z1 - z2).detach().abs().amax(dim=(0, 2)).min().item() > 1e-3, "two consecutive forward calls must differ"
    sp.reseed(4)
    z3 = la.diffeq_layer(dec, (z0t, tht), ts)
    z4 = la.diffeq_layer(dec, (z0t, tht), ts)
    assert torch.equal(z3, z1) and torch.equal(z4, z2), "after reseed the sequence repeats"
    h = sp._native()
    assert h.lib.lde_last_kernel(h.ptr, 0) == b"k_forward_sde_dir"
    # `sigma` reaches the handle: another σ is another path, σ = 0 none
    zs = la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.StuartLandau(N, solver=la.EulerHeun(), seed=4, sigma=0.0), None)), (z0t, tht), ts)
    nat.set_option("noise_sigma", 0.0)
    zc0, _, _ = nat.forward(z0, th, ts)
    assert np.array_equal(zs.detach().permute(2, 1, 0).cpu().numpy(), zc0) and not torch.equal(zs, z1)
    # sharded by trajectory: each shard passes its first global index, the shards draw the whole batch's path
    from latentdiffeq_amd import dist
    parts = []
    for rank in range(2):
        dr = la.Decoder(la.GOKU_basic(), (None, la.StuartLandau(N, solver=la.EulerHeun(), seed=4), None))
        parts.append(dist.diffeq_layer_sharded(dr, (z0t, tht), ts, rank=rank, world=2))
        assert dr.diffeq.first_trajectory == (0, 38)[rank]
    assert torch.equal(torch.cat(parts, dim=1), z1)
    # another sensealg is refused with the library's advice
    with pytest.raises(Exception, match="use LDE_SENSE_FORWARD_DUAL"):
        la.diffeq_layer(la.Decoder(la.GOKU_basic(), (None, la.StuartLandau(N, solver=la.EM(), sensealg=la.BacksolveAdjoint()), None)), (z0t, tht), ts)


@pytest.mark.parametrize("N", NS)
def test_captured_pair_replays_each_epochs_path(N):
    """lde_reserve, then a forward + pullback pair captured on one stream: every replay reads the device epoch word and draws the reference's
    path for that offset — bit for bit what the eager pair gives at that epoch."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import _lib as L
    D, P, _ = R.dims(N)
    B, dt, solver = 256, 0.05, R.EULER_HEUN
    z0, th, ts, dz = _ref(N, solver, 50, B, dt)[:4]
    T = len(ts)
    ep = torch.zeros(1, device="cuda", dtype=torch.int64)
    sp = la.StuartLandau(N, solver=la.EulerHeun(), seed=SEED, epoch=ep)
    h = sp._native()
    lib = h.lib
    L.check(lib.lde_reserve(h.ptr, B, T), h.ptr, "lde_reserve")
    L.check(lib.lde_set_noise(h.ptr, SEED, 0, 0, C.c_void_p(ep.data_ptr())), h.ptr, "lde_set_noise")
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0d, thd, dzd = (torch.from_numpy(np.array(a)).to("cuda") for a in (z0, th, dz))
    out = torch.empty((T, B, D), device="cuda")
    g0, gth = torch.empty((B, D), device="cuda"), torch.empty((B, P), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def step():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.lde_forward(h.ptr, p(z0d), p(thd), tsp, T, B, p(out), None, s), h.ptr, "fwd")
        L.check(lib.lde_adjoint(h.ptr, p(out), p(thd), tsp, T, B, p(dzd), p(g0), p(gth), None, s), h.ptr, "adj")

    def snap():
        torch.cuda.synchronize()
        return [x.clone() for x in (out, g0, gth)]

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
        for x in (out, g0, gth):
            x.fill_(7.0)
        graph.replay()
        got = snap()
        for x, y in zip(got, eager[e]):
            assert torch.equal(x, y), "a replay must equal the eager pair at that epoch bit for bit"
        zr, r0, rth = (_ref(N, solver, 50, B, dt, off=e)[i] for i in (4, 6, 7))
        assert U.rel(got[0].cpu().numpy(), zr) <= R.BOUNDS[0]
        assert U.rel(got[1].cpu().numpy(), r0) <= R.BOUNDS[2] and U.rel(got[2].cpu().numpy(), rth) <= R.BOUNDS[3]
