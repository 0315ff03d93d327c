"""The Stuart–Landau network's cost (LDE_RHS_STUART_LANDAU: StuartLandauDir<N> on k_forward_dual_dir / k_forward_sde_dir / k_adjoint_dual_dir;
N = 1: five directions in an 8-lane group, N = 2 and 3: nine and thirteen in a 16-lane group) beside the Kuramoto system's at N = 3 and the
cardiovascular system's — the same kernels over other systems — on the same box in the same run, alternating: forward and pullback through
the C ABI at T = 50 on ts = 0.05·j, caller-owned records, HIP events around `--iters` back-to-back calls after a warm-up
(abl/kuramoto_time.py's and abl/cvs_time.py's runners, which this reuses for those two systems). Three solves per N: Tsit5 at the default
tolerances (1e-6 / 1e-3), and the two stochastic steppers EM() and EulerHeun() at dt = 0.05 (49 substeps, σ = 0.01). One JSON line per
(right-hand side, solver, B) with the step attempts (substeps) per trajectory and forward_us_per_attempt. Recorded in DESIGN.md §8.7, not gated.

    python abl/sl_time.py [--B 256 65536] [--T 50] [--iters 200] [--rounds 2] [--N 1 2 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cvs_time  # noqa: E402
import kuramoto_time  # noqa: E402
from latentdiffeq_amd import _lib as L  # noqa: E402

SOLVERS = {"tsit5": L.SOLVER_TSIT5, "em": L.SOLVER_EM, "euler_heun": L.SOLVER_EULER_HEUN}


def sl_inputs(N, B, seed=0):
    """x₀, y₀ ~ U(−1, 1), a ~ U(−0.5, 1), ω ~ U(0.5, 3), G ~ U(0, 1): the ranges of tests/test_gpu_sl.py."""
    rng = np.random.default_rng(seed)
    z0 = rng.uniform(-1.0, 1.0, (B, 2 * N))
    th = np.concatenate([rng.uniform(-0.5, 1.0, (B, N)), rng.uniform(0.5, 3.0, (B, N)), rng.uniform(0.0, 1.0, (B, 1))], axis=1)
    return z0.astype(np.float32), th.astype(np.float32)


def run(N, solver, B, T, iters):
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    D, P, G = 2 * N, 2 * N + 1, 8 if N == 1 else 16
    d.rhs_kind, d.state_dim, d.param_dim, d.sensealg, d.solver = L.RHS_STUART_LANDAU, D, P, L.SENSE_FORWARD_DUAL, SOLVERS[solver]
    if solver != "tsit5":
        d.adaptive, d.dt = 0, 0.05
    h = C.c_void_p()
    L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
    ts = 0.05 * np.arange(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = sl_inputs(N, B)
    dz = (np.random.default_rng(1).standard_normal((T, B, D)) / (B * T)).astype(np.float32)
    z0d, thd, dzd = (torch.from_numpy(a).cuda() for a in (z0, th, dz))
    out = torch.empty((T, B, D), device="cuda")
    g0, gth = torch.empty((B, D), device="cuda"), torch.empty((B, P), device="cuda")
    nbytes = int(lib.lde_step_record_bytes(h, B, T))
    rec = torch.empty((nbytes,), device="cuda", dtype=torch.uint8)
    L.check(lib.lde_set_step_record(h, C.c_void_p(rec.data_ptr()), nbytes), h, "lde_set_step_record")
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        L.check(lib.lde_forward(h, p(z0d), p(thd), tsp, T, B, p(out), None, s), h, "lde_forward")

    def adj():
        L.check(lib.lde_adjoint(h, p(out), p(thd), tsp, T, B, p(dzd), p(g0), p(gth), None, s), h, "lde_adjoint")

    for _ in range(10):
        fwd()
        adj()
    torch.cuda.synchronize()
    res = {}
    for what, f in (("forward", fwd), ("pullback", adj)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        res[what + "_us"] = round(e0.elapsed_time(e1) * 1e3 / iters, 2)
    st = L.Stats()
    L.check(lib.lde_get_stats(h, 0, C.byref(st), s), h, "lde_get_stats")
    kern = (lib.lde_last_kernel(h, 0).decode(), lib.lde_last_kernel(h, 1).decode())
    lib.lde_set_step_record(h, C.c_void_p(), 0)
    lib.lde_destroy(h)
    jrow = D * G
    io = dict(forward_read=4 * (D + P), forward_written=4 * T * (D + jrow) + 4, pullback_read=4 * T * (D + jrow) + 4, pullback_written=4 * (D + P))
    return dict(rhs=f"stuart_landau N={N}", solver=solver, B=B, T=T, kernels=kern, record_bytes=nbytes, bytes_per_trajectory=io, nfailed=st.nfailed,
                steps_per_trajectory=round((st.naccept + st.nreject) / B, 2), max_steps=st.max_steps, **res)


def per_attempt(row):
    row["forward_us_per_attempt"] = round(row["forward_us"] / row["steps_per_trajectory"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2, help="passes over the configurations (the systems alternate within a pass)")
    ap.add_argument("--N", type=int, nargs="+", default=[1, 2, 3])
    a = ap.parse_args()
    for _ in range(a.rounds):
        for B in a.B:
            for N in a.N:
                for solver in SOLVERS:
                    print(json.dumps(per_attempt(run(N, solver, B, a.T, a.iters))), flush=True)
            print(json.dumps(per_attempt(kuramoto_time.run(3, B, a.T, a.iters))), flush=True)
            print(json.dumps(per_attempt(cvs_time.run(B, a.T, a.iters))), flush=True)


if __name__ == "__main__":
    main()
