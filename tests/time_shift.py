"""What tests/test_time_shift_host.py and tests/test_gpu_time_shift.py share: the shifted save grids (latentdiffeq_amd.synthetic.shifted_grids),
the table of dual-number systems with their numpy references, and the CPU oracle's own deviation under a time shift — the number the GPU
tests' sharp gate is built from. Test infrastructure only.

Every right-hand side of the library is autonomous, so the solution on `ts + c` is the solution on `ts`. On the grids of `shifted_grids` all
time arithmetic is exact (dyadic times, dyadic dt), so a fixed-step solve must return the SAME BITS on every grid; an adaptive solve may move
by an ulp-sized perturbation of the last step's h = (float)(tend − t) and of the dense-output Θ, amplified by the solve."""
import functools

import numpy as np

from oracle import oracle as O
from tests import cvs_ref, dpend_ref, kuramoto_ref, lv_ref, sl_ref

T = 33
DTS = (1.0 / 32.0, 3.0 / 64.0)
BATCHES = (37, 130)              # a partial wave; three waves with a ragged last workgroup for the 64-lane mappings
TOLS = ((1e-6, 1e-3), (1e-6, 1e-6))
ORDER = ("plus_1024", "minus_1024", "plus_2p20", "ends_at_0", "contains_0", "base")   # after a first run on "base": ONE handle, in this order


def grids(T=T, spacing=1.0 / 16.0):
    """(base, [(name, grid, c)] in ORDER — ending with the base grid again, so that a stale save-time cache also shows)."""
    g = O.shifted_grids(T, spacing)
    return g["base"], [(name, g[name], float(g[name][0] - g["base"][0])) for name in ORDER]


def part_c_grids():
    """Part C: the reference's own grid and its translate that ends at 0 — not dyadic; (0.05·j, 0.05·j − 2.45)."""
    return O.time_grid(50), O.time_grid(50) - 2.45


PART_C_SOLVES = {"tsit5_fixed_0.05": dict(solver=O.SOLVER_TSIT5, adaptive=0, dt=0.05), "rk4_0.05": dict(solver=O.SOLVER_RK4, adaptive=0, dt=0.05),
                 "rk4_0.13": dict(solver=O.SOLVER_RK4, adaptive=0, dt=0.13), "tsit5_adaptive": dict(solver=O.SOLVER_TSIT5)}


def same(tag, got, want):
    """Bit equality of two dicts of arrays (NaN patterns included), with the worst entry in the message."""
    assert got.keys() == want.keys(), (tag, sorted(got), sorted(want))
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            raise AssertionError(f"{tag}: `{k}` differs in {int((a != b).sum())} of {a.size} entries, largest |difference| {np.nanmax(d):.3e}")


def masked_steps(t, dt, n, c=0.0):
    """A step record [nseq, cap] reduced to what it holds: entries at and past n are zeroed; the start times have the shift c taken off
    (exact on the dyadic grids)."""
    t, dt, n = np.array(t, np.float64), np.array(dt, np.float64), np.asarray(n)
    live = np.arange(t.shape[1])[None, :] < n[:, None]
    return np.where(live, t - c, 0.0), np.where(live, dt, 0.0)


# ---- the dual-number systems beyond the pendulums: descriptor, inputs, numpy reference ------------------------------------------------------
def dual_systems():
    from latentdiffeq_amd import _lib as L
    S = {"lv": dict(desc=dict(rhs_kind=L.RHS_LOTKA_VOLTERRA, param_dim=4), sys=lv_ref.SYSTEM, inputs=lambda B: lv_ref.inputs(B, seed=3),
                    kernels=(b"k_lv_forward_dual", b"k_lv_adjoint_dual")),
         "dpend": dict(desc=dict(rhs_kind=L.RHS_DOUBLE_PENDULUM, state_dim=dpend_ref.D, param_dim=dpend_ref.P), sys=dpend_ref.SYSTEM,
                       inputs=lambda B: dpend_ref.inputs(B, seed=3)),
         "cvs": dict(desc=dict(rhs_kind=L.RHS_CVS, state_dim=cvs_ref.D, param_dim=cvs_ref.P), sys=cvs_ref.SYSTEM, inputs=lambda B: cvs_ref.inputs(B, seed=3))}
    for N in (3, 4):                      # 8 and 16 lanes per trajectory
        S[f"kuramoto{N}"] = dict(desc=dict(rhs_kind=L.RHS_KURAMOTO, state_dim=N, param_dim=N + 1), sys=kuramoto_ref.system(N),
                                 inputs=lambda B, N=N: kuramoto_ref.inputs(B, N, seed=3))
    for N in sl_ref.NS:
        S[f"sl{N}"] = dict(desc=dict(rhs_kind=L.RHS_STUART_LANDAU, state_dim=2 * N, param_dim=2 * N + 1), sys=sl_ref.system(N),
                           inputs=lambda B, N=N: sl_ref.inputs(N, B, seed=3))
    # lanes of a trajectory in the lane-per-direction kernels (0: k_forward_dual, whose record is J [T][2][NP][B])
    lanes = dict(lv=0, dpend=dpend_ref.G, cvs=cvs_ref.G, kuramoto3=kuramoto_ref.group_width(3), kuramoto4=kuramoto_ref.group_width(4),
                 **{f"sl{N}": sl_ref.GROUP[N] for N in sl_ref.NS})
    for name, s in S.items():
        s.setdefault("kernels", (b"k_forward_dual_dir", b"k_adjoint_dual_dir"))
        s["G"] = lanes[name]
    return S


def record_J(head, B, T, D, NP, G):
    """J [T, B, D, NP] out of a dual record's bytes n | J (include/lde.h: J [T][2][NP][B] of k_forward_dual, G = 0; J [T][D][B][G] of the
    lane-per-direction kernels, whose pad lanes' columns must be zero)."""
    off = (4 * B + 255) // 256 * 256
    if G == 0:
        return head[off:off + 4 * T * D * NP * B].view(np.float32).reshape(T, D, NP, B).transpose(0, 3, 1, 2).copy()
    full = head[off:off + 4 * T * D * B * G].view(np.float32).reshape(T, D, B, G).transpose(0, 2, 1, 3)
    assert (full[..., NP:] == 0).all(), "a pad lane's tangent must stay zero"
    return full[..., :NP].copy()


def dual_cotangent(D, T, B, seed=1):
    return (np.random.default_rng(seed).standard_normal((T, B, D)) / (B * T)).astype(np.float32)


# ---- the oracle's own deviation under the shifts (Part B's yardstick) ------------------------------------------------------------------------
def _oracle_adaptive(orc, kind, tol, ts, B):
    """Every quantity the pendulum paths return, from the oracle at Tsit5 adaptive: ẑ, the three continuous adjoints on it, the discrete sweep
    on its own steps, the dual solve's ẑ, J and gradients; and the accepted steps per trajectory."""
    z0, L = O.pendulum_inputs(B, seed=3)
    dz = O.cotangent(len(ts), B, 2)
    kw = dict(rhs_kind=kind, abstol=tol[0], reltol=tol[1])
    out, nacc = {}, {}
    zs, ret, rec, _ = orc.forward_steps(O.make_desc(sensealg=O.SENSE_DISCRETE, **kw), z0, L, ts)
    assert (ret == 0).all()
    out["z"], nacc["forward"] = zs, rec["n"].copy()
    d0, dL, _, _ = orc.adjoint_discrete(O.make_desc(sensealg=O.SENSE_DISCRETE, **kw), zs, L, ts, dz, rec)
    out["disc_dz0"], out["disc_dtheta"] = d0, dL
    for sense in (O.SENSE_BACKSOLVE_CHECKPOINTED, O.SENSE_BACKSOLVE, O.SENSE_PARALLEL_CHECKPOINTED):
        g0, gL, _, info = orc.adjoint(O.make_desc(sensealg=sense, **kw), zs, L, ts, dz)
        out[f"adj{sense}_dz0"], out[f"adj{sense}_dtheta"] = g0, gL
        nacc[f"adj{sense}"] = np.array([info["naccept"]])
    zd, J, (q0, qL), retd, recd, _ = orc.forward_dual(O.make_desc(sensealg=4, **kw), z0, L, ts, dz_out=dz, dual_norm=True)
    assert (retd == 0).all()
    out["dual_z"], out["dual_J"], out["dual_dz0"], out["dual_dtheta"] = zd, J, q0, qL
    nacc["dual"] = recd["n"].copy()
    return out, nacc


@functools.lru_cache(maxsize=None)
def oracle_shift_deviation(prec, kind, tol, B, T=T, spacing=1.0 / 16.0):
    """{quantity: largest |shifted − unshifted| over the shifts, as a fraction of the unshifted array's largest magnitude}, {quantity: that
    magnitude}, and the solves whose accepted-step counts a shift changed — the f32 (or f64) oracle on the inputs the GPU tests use. (The
    forward, dual and time-parallel adjoint solves keep theirs; the sequential reverse-time adjoints — "adj0", "adj1" — clip a step at each
    of the T − 1 save times, and at 1e-6 in f32, where the error estimate is round-off, an ulp in those h moves a few accept decisions.)"""
    orc = O.Oracle(prec)
    base, sh = grids(T, spacing)
    ref, nref = _oracle_adaptive(orc, kind, tol, base, B)
    dev = {k: 0.0 for k in ref}
    changed = set()
    for name, ts, c in sh[:-1]:
        out, nacc = _oracle_adaptive(orc, kind, tol, ts, B)
        for k in ref:
            dev[k] = max(dev[k], float(np.abs(out[k].astype(np.float64) - ref[k]).max() / np.abs(ref[k]).max()))
        changed |= {k for k in nref if not np.array_equal(nacc[k], nref[k])}
    return dev, {k: float(np.abs(v).max()) for k, v in ref.items()}, frozenset(changed)


F32_ULP = float(np.finfo(np.float32).eps)


def sharp_bound(dev_rel):
    """Part B's gate against the same kernel on the base grid, as a fraction of the array's largest magnitude: 8 × the reference's own
    deviation (both sides are f32 evaluations of the same formulas that differ in contraction only, so the ulp-sized perturbation of the last
    step and of Θ is amplified alike), floored at 4 f32 ulps of the largest magnitude."""
    return max(8.0 * dev_rel, 4.0 * F32_ULP)


# ---- the MLP right-hand sides: shapes, inputs and the oracle's deviation under the shifts ----------------------------------------------------
# the smallest shapes of tests/test_gpu_mlp.py::test_kernel_families_agree that reach each kernel family, and the family each leg's CONTINUOUS
# adjoint runs (option "adjoint_family") as recorded there — the mapping does not read the solver
MLP_CASES = {
    "per_traj_3_20_64_3": dict(layers=(3, 20, 64, 3), B=19, kw=dict(rhs_kind=O.RHS_MLP, state_dim=3, param_dim=0, activation=O.ACT_TANH),
                               legs=dict(new=1, tiles=6, mlpv=5)),
    "coupled_8_200_200_8": dict(layers=(8, 200, 200, 8), B=48, kw=dict(rhs_kind=O.RHS_MLP, state_dim=8, param_dim=0, batching=O.BATCH_COUPLED),
                                legs=dict(new=2, mlpw=4, tiles=0, mlpv=5)),
    "coupled_32_128_128_32": dict(layers=(32, 128, 128, 32), B=40, kw=dict(rhs_kind=O.RHS_MLP, state_dim=32, param_dim=0, batching=O.BATCH_COUPLED),
                                  legs=dict(new=3)),
}
MLP_ADAPTIVE_B = 8      # trajectories of the coupled cases under the controller: the oracle's 200-wide replay is what a case costs


def mlp_inputs(case, T, B=None):
    cfg = MLP_CASES[case]
    D = cfg["kw"]["state_dim"]
    B = B or cfg["B"]
    z0 = (0.5 * np.random.default_rng(4).standard_normal((cfg["B"], D))).astype(np.float32)[:B]
    return cfg, O.mlp_weights(cfg["layers"], seed=8), z0, O.cotangent(T, cfg["B"], D)[:, :B]


def mlp_adaptive_case(case, tol):
    """Part B on an MLP right-hand side: the case's shape with tanh units (smooth: an ulp in the last step's h cannot flip a relu unit, which
    would move a gradient by a finite amount in the kernel and in the oracle alike and make the sharp gate a test of luck), Tsit5 adaptive at
    `tol`; eight trajectories where the batch is coupled. → (descriptor keywords, W, z0, dz, B)."""
    cfg = MLP_CASES[case]
    B = MLP_ADAPTIVE_B if cfg["kw"].get("batching") == O.BATCH_COUPLED else cfg["B"]
    _, W, z0, dz = mlp_inputs(case, T, B)
    kw = dict(cfg["kw"], layers=cfg["layers"], activation=O.ACT_TANH, solver=O.SOLVER_TSIT5, abstol=tol[0], reltol=tol[1])
    return kw, W, z0, dz, B


def _oracle_mlp_adaptive(orc, kw, W, z0, dz, ts, nthreads):
    out = {}
    dd = O.make_desc(sensealg=O.SENSE_DISCRETE, **kw)
    zs, ret, rec, _ = orc.forward_steps(dd, z0, None, ts, W=W, nthreads=nthreads)
    assert (ret == 0).all()
    out["z"] = zs
    out["disc_dz0"], _, out["disc_dW"], _ = orc.adjoint_discrete(dd, zs, None, ts, dz, rec, W=W, nthreads=nthreads)
    out["adj_dz0"], _, out["adj_dW"], _ = orc.adjoint(O.make_desc(sensealg=O.SENSE_PARALLEL_CHECKPOINTED, **kw), zs, None, ts, dz, W=W, nthreads=nthreads)   # (tests/gpu_util.py's default: the GPU test's descriptor)
    return out, rec["n"].copy()


@functools.lru_cache(maxsize=None)
def oracle_mlp_shift_deviation(case, tol, nthreads=8):
    """The f32 oracle's own deviation under the shifts on an MLP case's inputs: {z, disc_dz0, disc_dW, adj_dz0, adj_dW: fraction of the base
    array's largest entry}, and whether its forward solve kept its accepted steps."""
    kw, W, z0, dz, B = mlp_adaptive_case(case, tol)
    orc = O.Oracle("f32")
    base, sh = grids(T)
    ref, nref = _oracle_mlp_adaptive(orc, kw, W, z0, dz, base, nthreads)
    dev, unchanged = {k: 0.0 for k in ref}, True
    for name, ts, c in sh[:-1]:
        out, n = _oracle_mlp_adaptive(orc, kw, W, z0, dz, ts, nthreads)
        for k in ref:
            dev[k] = max(dev[k], float(np.abs(out[k].astype(np.float64) - ref[k]).max() / np.abs(ref[k]).max()))
        unchanged &= bool(np.array_equal(n, nref))
    return dev, unchanged


# ---- Part C on the dual systems: bounds (ẑ, J, dz0, dθ; each relative to the reference array's largest entry) -----------------------------------
# The project's rule (tests/dpend_ref.py, tests/cvs_ref.py): the standing bounds wherever the numpy reference's own f32 mode stays within a
# quarter of them on the case's inputs and steps, else 4 × that floor, rounded up — constants, every floor measured and asserted on the CPU by
# tests/test_time_shift_host.py::test_part_c_dual_bounds_stand_on_the_f32_floor, none taken from a kernel. Only the double pendulum (a
# sensitive system; seed 3 is not one of its hand-picked seeds) needs more than the standing ones. Floors measured on 0.05·j − 2.45, B = 37,
# worst of the four solves: 6.4e-6 / 3.2e-5 / 2.3e-5 / 3.2e-5.
DUAL_STANDING_BOUNDS = (2e-5, 1e-4, 1e-4, 1e-4)
PART_C_DUAL_BOUNDS = {"dpend": (2.7e-5, 1.4e-4, 1e-4, 1.3e-4)}
PART_C_DUAL_B = 37


def part_c_dual_bounds(name):
    return PART_C_DUAL_BOUNDS.get(name, DUAL_STANDING_BOUNDS)


def rel(a, b):
    """max |a − b| relative to the largest entry of the reference array b."""
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def part_c_dual_floor(name, solve):
    """The f32 numpy reference against the f64 one on 0.05·j − 2.45, on the f64 solve's own steps: (ẑ, J, dz0, dθ)."""
    from tests import dual_ref
    s, kw = dual_systems()[name], PART_C_SOLVES[solve]
    z0, th = s["inputs"](PART_C_DUAL_B)
    dz = dual_cotangent(s["sys"].D, 50, PART_C_DUAL_B)
    tz = part_c_grids()[1]
    if kw.get("adaptive", 1):
        z, J, ret, info = dual_ref.solve(s["sys"], z0, th, tz, kw["solver"])
        zf, Jf, retf, _ = dual_ref.solve(s["sys"], z0, th, tz, kw["solver"], steps=(info["t"], info["dt"]), dtype=np.float32)
    else:
        z, J, ret, _ = dual_ref.solve(s["sys"], z0, th, tz, kw["solver"], adaptive=False, dt=kw["dt"])
        zf, Jf, retf, _ = dual_ref.solve(s["sys"], z0, th, tz, kw["solver"], adaptive=False, dt=kw["dt"], dtype=np.float32)
    assert (ret == 0).all() and (retf == 0).all()
    g, gf = dual_ref.pullback(s["sys"], J, dz), dual_ref.pullback(s["sys"], Jf, dz)
    return rel(zf, z), rel(Jf, J), rel(gf[0], g[0]), rel(gf[1], g[1])
