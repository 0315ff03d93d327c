"""GPU: the lane-per-direction kernels over a system (csrc/lde_dual_dir.hip: k_forward_dual_dir<SYS, …> / k_adjoint_dual_dir<D, NP, G>) write,
for each of their systems, the BITS that an earlier build wrote: for Kuramoto the kernels hard-wired to KuramotoDir<N>, before the double
pendulum became their second system; for the double pendulum the kernels of the commit that added it — the pin that any later change to
the stepping loop these kernels share with k_forward_dual has to keep.

tests/golden/dual_parent_bits_kuramoto.npz and tests/golden/dual_parent_bits_dpend.npz were each recorded on an MI355X from a build of the
commit named in the file's `parent_commit` entry, by `record()` below; `hipcc_version` is the compiler of that build. Every array is compared
as raw bytes — a NaN block is its bit pattern, −0.0 is not 0.0 — no tolerance: ẑ, J (the record's own layout [T][D][B][G], pad lanes
included), rec.n, the return codes, the four statistics of the forward and of the pullback, dz0, dθ, and the step trace where a case takes
one. A difference is a finding about the change to the kernels (a multiply-add fused differently, a seed formed differently), not a reason
for a bound.

Cases (the nine save times are tests/lv_ref.py's ragged grid; B = 19 ends in a ragged last wave at both group widths: 152 lanes at G = 8,
304 at G = 16). A case is "<system>-<what>"; the system is n<N> (Kuramoto, inputs from tests/kuramoto_ref.py) or dp (the double pendulum,
G = 8, inputs from tests/dpend_ref.py at its own seeds for this grid and for the long one):
  * N ∈ {2, 3, 4, 7} and dp × {Tsit5 adaptive 1e-6 / 1e-3, Tsit5 at dt = 0.05, RK4 at dt = 0.05}; at N = 4 and 7 the file keeps the rows of
    J named in the case's `J_rows` entry (the file has a size limit) — the gradients, which sum over every row, are whole;
  * one failing solve (maxiters = 3 ⇒ LDE_RET_MAXITERS) at N = 3, at N = 7 and at dp: a NaN block, zero J, zero gradient;
  * N = 3 and dp with option "step_trace": the t and dt arrays;
  * the save grid outside LDS: T = 6001, B = 3, N = 4 and dp, Tsit5 at dt = 0.0125 — rows 0, 1, 3000, 6000 of ẑ and J and the whole
    gradients."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = {"n": os.path.join(GOLDEN_DIR, "dual_parent_bits_kuramoto.npz"), "dp": os.path.join(GOLDEN_DIR, "dual_parent_bits_dpend.npz")}
B_RAGGED = 19
LONG_ROWS = [0, 1, 3000, 6000]
WIDE_J_ROWS = {"n4": [1, 5, 8], "n7": [1, 8]}     # of the nine: inside the first step, among the three close together, the last
RET_MAXITERS = 1
SIZE_LIMIT = 300_000

NS = (2, 3, 4, 7)
SOLVES = {"tsit5_adaptive": dict(), "tsit5_fixed": dict(adaptive=0, dt=0.05), "rk4_fixed": dict(solver=1, adaptive=0, dt=0.05)}
CASES = {"n": [f"n{N}-{v}" for N in NS for v in SOLVES] + ["n3-fails", "n7-fails", "n3-step_trace", "n4-long_grid"],
         "dp": [f"dp-{v}" for v in SOLVES] + ["dp-fails", "dp-step_trace", "dp-long_grid"]}


def _a256(x):
    return (x + 255) // 256 * 256


def _system(name):
    """What a case's system is to this test: its rhs_kind, D, P and G, its inputs and cotangent, its seeds of the ragged and the long grid."""
    if name == "dp":
        from tests import dpend_ref as R
        return dict(kind="RHS_DOUBLE_PENDULUM", D=R.D, P=R.P, G=R.G, inputs=R.inputs, cotangent=R.cotangent, seeds=(R.RAGGED_SEED, R.LONG_SEED))
    from tests import kuramoto_ref as R
    N = int(name[1:])
    return dict(kind="RHS_KURAMOTO", D=N, P=N + 1, G=R.group_width(N), inputs=lambda B, seed: R.inputs(B, N, seed=seed),
                cotangent=lambda T, B: R.cotangent(T, B, N), seeds=(9 + N, 6001))


def _native(s, **kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=getattr(L, s["kind"]), state_dim=s["D"], param_dim=s["P"], sensealg=L.SENSE_FORWARD_DUAL, **kw))


def _solve(nat, s, z0, th, ts, dz, rows=None, J_rows=None, trace=False):
    """One lde_forward into a record this test owns and its lde_adjoint: everything the two launches wrote, as numpy arrays."""
    import torch
    from latentdiffeq_amd import _lib as L
    B, T, D, G = z0.shape[0], len(ts), s["D"], s["G"]
    if trace:
        nat.set_option("step_trace", 1)
        nat.set_option("record_capacity", 256)
    nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
    assert nbytes >= _a256(4 * B) + 4 * T * D * B * G
    buf = torch.zeros((nbytes,), device="cuda", dtype=torch.uint8)
    L.check(nat.lib.lde_set_step_record(nat.h, C.c_void_p(buf.data_ptr()), nbytes), nat.h, "lde_set_step_record")
    z, ret, st = nat.forward(z0, th, ts)
    n = buf[:4 * B].view(torch.int32).cpu().numpy()
    off = _a256(4 * B)
    J = buf[off:off + 4 * T * D * B * G].view(torch.float32).cpu().numpy().reshape(T, D, B, G)
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    keys = ("nfe", "naccept", "nreject", "nfailed")
    J_rows = rows if rows is not None else J_rows
    out = dict(z=z if rows is None else z[rows], J=J if J_rows is None else J[J_rows], n=n, retcode=ret, dz0=g0, dtheta=gth,
               forward_stats=np.array([st[k] for k in keys], np.int64), pullback_stats=np.array([sta[k] for k in keys], np.int64))
    if J_rows is not None:
        out["J_rows"] = np.array(J_rows, np.int64)
    if trace:
        tr = nat.step_record(0, B, cap=256)
        out.update(trace_t=tr["t"], trace_dt=tr["dt"], trace_n=tr["n"])
    return out


def compute(case):
    """The arrays of one case, from whatever build of the library is loaded."""
    from tests.lv_ref import ragged_grid
    name, what = case.split("-")
    s = _system(name)
    if what == "long_grid":            # T = DUAL_TS_LDS_MAX + 1: the kernels read the grid from global memory
        T, B = 6001, 3
        ts = 1e-3 * np.arange(T)
        z0, th = s["inputs"](B, seed=s["seeds"][1])
        return _solve(_native(s, adaptive=0, dt=0.0125), s, z0, th, ts, s["cotangent"](T, B), rows=LONG_ROWS)
    ts = ragged_grid()
    B, T = B_RAGGED, len(ts)
    kw = dict(maxiters=3) if what == "fails" else {} if what == "step_trace" else SOLVES[what]
    z0, th = s["inputs"](B, seed=s["seeds"][0])
    dz = s["cotangent"](T, B)
    if what == "fails":
        dz = np.array(dz)
        dz[:, :3] = np.nan             # (what a loss of a NaN block hands back)
    return _solve(_native(s, **kw), s, z0, th, ts, dz, J_rows=WIDE_J_ROWS.get(name), trace=what == "step_trace")


def record(system, parent_commit, hipcc_version):
    """Write the golden file of `system` ("n" or "dp") from the loaded build (run once, on the build of the commit before the kernels change).
    Every case is computed twice and nothing is written if the two differ: the system may be chaotic, the kernel is not."""
    arrays = {"parent_commit": np.array(parent_commit), "hipcc_version": np.array(hipcc_version)}
    for case in CASES[system]:
        first, again = compute(case), compute(case)
        bad = [k for k in first if not _same_bytes(first[k], again[k])]
        assert not bad, f"{case}: {bad} differ between two runs of one build"
        for k, v in first.items():
            arrays[f"{case}/{k}"] = v
    np.savez_compressed(GOLDEN[system], **arrays)
    assert os.path.getsize(GOLDEN[system]) <= SIZE_LIMIT, os.path.getsize(GOLDEN[system])


@functools.lru_cache(maxsize=None)
def _golden(system):
    with np.load(GOLDEN[system]) as f:
        return {k: f[k] for k in f.files}


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_cases_are_what_they_claim():
    """The nine save times against the fixed step 0.05; 19 trajectories leave the last wave ragged at both group widths; the files' sizes."""
    from tests import dpend_ref, kuramoto_ref as R
    d = np.diff(R.ragged_grid())
    assert len(d) == 8 and d.min() < 0.05 and d.max() > 3 * 0.05
    assert [B_RAGGED * R.group_width(N) for N in NS] == [152, 152, 304, 304] and 152 % 64 and 304 % 64
    assert B_RAGGED * dpend_ref.G == 152
    for system in GOLDEN:
        assert os.path.getsize(GOLDEN[system]) <= SIZE_LIMIT
        assert str(_golden(system)["parent_commit"]) and str(_golden(system)["hipcc_version"])


@pytest.mark.parametrize("case", CASES["n"] + CASES["dp"])
def test_the_parents_bits(case):
    name, what = case.split("-")
    gold = _golden("dp" if name == "dp" else "n")
    got = compute(case)
    want = {k.split("/", 1)[1]: v for k, v in gold.items() if k.startswith(case + "/")}
    assert set(want) == set(got) and len(want) >= 8
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
