"""The stochastic pendulum's cost (LDE_RHS_SPENDULUM: EM and EulerHeun, LDE_SENSE_FORWARD_DUAL) beside the dual-number solve of the
deterministic pendulum with fixed-step RK4 at the same dt, on the same box: forward and pullback through the C ABI at T = 50, caller-owned
records, HIP events around `--iters` back-to-back calls after a warm-up (as abl/dual_time.py). One JSON line per (solver, B).

    python abl/sde_time.py [--B 256 65536] [--dt 0.05] [--iters 200]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from latentdiffeq_amd import _lib as L  # noqa: E402
from latentdiffeq_amd.synthetic import cotangent, pendulum_inputs, time_grid  # noqa: E402

CONFIGS = {"RK4 (deterministic, dual)": (L.RHS_PENDULUM, L.SOLVER_RK4), "EM": (L.RHS_SPENDULUM, L.SOLVER_EM),
           "EulerHeun": (L.RHS_SPENDULUM, L.SOLVER_EULER_HEUN)}


def run(name, B, T, dt, iters):
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    d.rhs_kind, d.solver = CONFIGS[name]
    d.sensealg, d.adaptive, d.dt = L.SENSE_FORWARD_DUAL, 0, dt
    h = C.c_void_p()
    L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
    ts = time_grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = pendulum_inputs(B)
    z0d, thd, dzd = (torch.from_numpy(a).cuda() for a in (z0, th, cotangent(T, B, 2)))
    out = torch.empty((T, B, 2), device="cuda")
    g0, gL = torch.empty((B, 2), device="cuda"), torch.empty((B, 1), device="cuda")
    nbytes = int(lib.lde_step_record_bytes(h, B, T))
    rec = torch.empty((nbytes,), device="cuda", dtype=torch.uint8)
    L.check(lib.lde_set_step_record(h, C.c_void_p(rec.data_ptr()), nbytes), h, "lde_set_step_record")
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        L.check(lib.lde_forward(h, p(z0d), p(thd), tsp, T, B, p(out), None, s), h, "lde_forward")

    def adj():
        L.check(lib.lde_adjoint(h, p(out), p(thd), tsp, T, B, p(dzd), p(g0), p(gL), None, s), h, "lde_adjoint")

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
    return dict(solver=name, B=B, T=T, dt=dt, kernels=kern, nfe_per_trajectory=st.nfe // B, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    for B in a.B:
        for name in CONFIGS:
            print(json.dumps(run(name, B, a.T, a.dt, a.iters)), flush=True)


if __name__ == "__main__":
    main()
