"""GPU: the dual-number solve kernels (csrc/lde_dual.hip: k_forward_dual / k_adjoint_dual over the system; csrc/lde_pend_sde.hip) write the
BITS that the per-system kernels they replaced wrote — k_pend_forward_dual / k_pend_adjoint_dual, k_lv_forward_dual / k_lv_adjoint_dual and
k_pend_forward_sde before its prologue and epilogue moved into csrc/lde_dual.h.

tests/golden/dual_parent_bits.npz was recorded on an MI355X from a build of the commit named in its `parent_commit` entry (the last one with
the three copies), by `record()` below; `hipcc_version` is the compiler of that build. Every array is compared as raw bytes — a NaN block is
its bit pattern, −0.0 is not 0.0 — no tolerance: ẑ, J, rec.n, the return codes, the four statistics of the forward and of the pullback, dz0,
dθ, and the step trace where a case takes one. A difference is a finding about the kernels' arithmetic (how a state is seeded, an expression
regrouped, a multiply-add fused differently), not a reason for a bound.

Cases (inputs from the neighbouring tests' generators; B = 67 is a full wave plus three lanes, the last workgroup ragged; the nine save times
are tests/lv_ref.py's ragged grid: three inside the first step, a gap of 0.875 that several steps cross, three close together, a gap again):
  * the two pendulums and Lotka–Volterra × {Tsit5 adaptive 1e-6 / 1e-3, Tsit5 at dt = 0.05, RK4 at dt = 0.05};
  * the stochastic pendulum, EM and Euler–Heun at dt = 0.05, seed 5, offset 2, a device epoch word of 3;
  * one failing solve per system (maxiters = 3 ⇒ LDE_RET_MAXITERS): a NaN block, zero J, zero gradient;
  * the frictionless pendulum with option "step_trace": the t and dt arrays;
  * the save grid outside LDS: T = 6001, B = 3, Tsit5 at dt = 0.0125, pendulum and Lotka–Volterra — rows 0, 1, 3000, 6000 of ẑ and J and
    the whole gradients (which sum over every row)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dual_parent_bits.npz")
B_RAGGED = 67
LONG_ROWS = [0, 1, 3000, 6000]
RET_MAXITERS = 1

SYSTEMS = ("pend", "friction", "lv")
SOLVES = {"tsit5_adaptive": dict(), "tsit5_fixed": dict(adaptive=0, dt=0.05), "rk4_fixed": dict(solver=1, adaptive=0, dt=0.05)}
CASES = ([f"{s}-{v}" for s in SYSTEMS for v in SOLVES] + ["sde-em", "sde-euler_heun"] + [f"{s}-fails" for s in ("pend", "lv", "sde")]
         + ["pend-step_trace", "pend-long_grid", "lv-long_grid"])


def _a256(x):
    return (x + 255) // 256 * 256


def _system(name, B, T, **kw):
    """(handle, z0, θ, dz_out, partials per component) of a system on B trajectories."""
    from latentdiffeq_amd import _lib as L
    from oracle import oracle as O
    from tests import lv_ref, sde_ref
    from tests.gpu_util import Native, make_desc
    kw.setdefault("sensealg", L.SENSE_FORWARD_DUAL)
    if name == "lv":
        z0, th = lv_ref.inputs(B, seed=T)
        return Native(make_desc(rhs_kind=L.RHS_LOTKA_VOLTERRA, param_dim=4, **kw)), z0, th, lv_ref.cotangent(T, B), 6
    if name == "sde":
        z0, th = sde_ref.inputs(B, seed=T)
        kw.setdefault("solver", sde_ref.EULER_HEUN)
        nat = Native(make_desc(rhs_kind=L.RHS_SPENDULUM, adaptive=0, dt=0.05, **kw))
        return nat, z0, th, sde_ref.cotangent(T, B), 3
    z0, th = O.pendulum_inputs(B, seed=T)
    kind = L.RHS_PENDULUM_FRICTION if name == "friction" else L.RHS_PENDULUM
    return Native(make_desc(rhs_kind=kind, **kw)), z0, th, O.cotangent(T, B, 2), 3


def _solve(nat, z0, th, ts, dz, NP, rows=None, trace=False):
    """One lde_forward into a record this test owns and its lde_adjoint: everything the two launches wrote, as numpy arrays."""
    import torch
    from latentdiffeq_amd import _lib as L
    B, T = z0.shape[0], len(ts)
    if trace:
        nat.set_option("step_trace", 1)
        nat.set_option("record_capacity", 256)
    nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
    assert nbytes >= _a256(4 * B) + 8 * NP * T * B
    buf = torch.zeros((nbytes,), device="cuda", dtype=torch.uint8)
    L.check(nat.lib.lde_set_step_record(nat.h, C.c_void_p(buf.data_ptr()), nbytes), nat.h, "lde_set_step_record")
    z, ret, st = nat.forward(z0, th, ts)
    n = buf[:4 * B].view(torch.int32).cpu().numpy()
    off = _a256(4 * B)
    J = buf[off:off + 8 * NP * T * B].view(torch.float32).cpu().numpy().reshape(T, 2, NP, B)
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    keys = ("nfe", "naccept", "nreject", "nfailed")
    out = dict(z=z if rows is None else z[rows], J=J if rows is None else J[rows], n=n, retcode=ret, dz0=g0, dtheta=gth,
               forward_stats=np.array([st[k] for k in keys], np.int64), pullback_stats=np.array([sta[k] for k in keys], np.int64))
    if trace:
        tr = nat.step_record(0, B, cap=256)
        out.update(trace_t=tr["t"], trace_dt=tr["dt"], trace_n=tr["n"])
    return out


def compute(case):
    """The arrays of one case, from whatever build of the library is loaded."""
    import torch
    from latentdiffeq_amd import _lib as L
    from tests import lv_ref, sde_ref
    name, what = case.split("-")
    if what == "long_grid":            # T = DUAL_TS_LDS_MAX + 1: the kernels read the grid from global memory
        T, B = 6001, 3
        ts = 1e-3 * np.arange(T)
        nat, z0, th, dz, NP = _system(name, B, T, adaptive=0, dt=0.0125)
        return _solve(nat, z0, th, ts, dz, NP, rows=LONG_ROWS)
    ts = lv_ref.ragged_grid()
    B, T = B_RAGGED, len(ts)
    if name == "sde":
        kw = dict(maxiters=3) if what == "fails" else dict(solver={"em": sde_ref.EM, "euler_heun": sde_ref.EULER_HEUN}[what])
        nat, z0, th, dz, NP = _system(name, B, T, **kw)
        epoch = torch.tensor([3], device="cuda", dtype=torch.int64)
        L.check(nat.lib.lde_set_noise(nat.h, 5, 2, 0, C.c_void_p(epoch.data_ptr())), nat.h, "lde_set_noise")
        return _solve(nat, z0, th, ts, dz, NP)
    kw = dict(maxiters=3) if what == "fails" else {} if what == "step_trace" else SOLVES[what]
    nat, z0, th, dz, NP = _system(name, B, T, **kw)
    if what == "fails":
        dz = np.array(dz)
        dz[:, :3] = np.nan             # (what a loss of a NaN block hands back)
    return _solve(nat, z0, th, ts, dz, NP, trace=what == "step_trace")


def record(path, parent_commit, hipcc_version):
    """Write the golden file from the loaded build (run once, on the build of the commit before the kernels were merged)."""
    arrays = {"parent_commit": np.array(parent_commit), "hipcc_version": np.array(hipcc_version)}
    for case in CASES:
        for k, v in compute(case).items():
            arrays[f"{case}/{k}"] = v
    np.savez_compressed(path, **arrays)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_grid_is_what_the_cases_need():
    """The nine save times against the fixed step 0.05 of the cases: an interval shorter than a step, and one that several steps cross."""
    from tests import lv_ref
    d = np.diff(lv_ref.ragged_grid())
    assert len(d) == 8 and d.min() < 0.05 and d.max() > 3 * 0.05


@pytest.mark.parametrize("case", CASES)
def test_the_parents_bits(case):
    gold = _golden()
    got = compute(case)
    want = {k.split("/", 1)[1]: v for k, v in gold.items() if k.startswith(case + "/")}
    assert set(want) == set(got) and len(want) >= 8
    name, what = case.split("-")
    if what == "fails":
        assert (got["retcode"] == RET_MAXITERS).all() and (got["n"] == -RET_MAXITERS).all()
        assert np.isnan(got["z"]).all() and (got["J"] == 0).all() and (got["dz0"] == 0).all() and (got["dtheta"] == 0).all()
    else:
        assert (got["retcode"] == 0).all() and np.isfinite(got["z"]).all() and np.abs(got["J"]).max() > 0
        assert np.abs(got["dtheta"]).max() > 0
    if what == "step_trace":
        assert np.array_equal(got["trace_n"], got["n"]) and got["trace_n"].min() >= 2
    bad = [k for k in sorted(want) if not _same_bytes(want[k], got[k])]
    assert not bad, f"{case}: {bad} differ from the bits of {gold['parent_commit']}"
