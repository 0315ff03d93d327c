"""The double pendulum's cost (LDE_RHS_DOUBLE_PENDULUM: DoublePendDir on k_forward_dual_dir / k_adjoint_dual_dir, eight directions in one
8-lane group with no pad lane) beside the Kuramoto system's at N = 3 (8 lanes, one pad lane) and N = 4 (16 lanes, seven pad lanes) — the same
kernels over another system — and Lotka–Volterra's (k_lv_forward_dual / k_lv_adjoint_dual, a lane per trajectory), on the same box in the
same run, alternating: forward and pullback through the C ABI at T = 50, Tsit5 at the default tolerances (1e-6 / 1e-3), caller-owned
records, HIP events around `--iters` back-to-back calls after a warm-up (as abl/kuramoto_time.py, whose inputs and runner this reuses). One
JSON line per (right-hand side, B), with the unique bytes a trajectory reads and writes and the step attempts per trajectory. Recorded in
DESIGN.md §8.4, not gated.

    python abl/dpend_time.py [--B 256 65536] [--T 50] [--iters 200] [--rounds 2]
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

import kuramoto_time  # noqa: E402
from latentdiffeq_amd import _lib as L  # noqa: E402
from latentdiffeq_amd.synthetic import time_grid  # noqa: E402


def dpend_inputs(B, seed=0):
    """θ₁, θ₂, ω₁, ω₂ ~ U(−1, 1), L ~ U(0.8, 1.6), m ~ U(0.5, 2): the ranges of tests/test_gpu_dpend.py."""
    rng = np.random.default_rng(seed)
    z0 = rng.uniform(-1.0, 1.0, (B, 4)).astype(np.float32)
    th = np.concatenate([rng.uniform(0.8, 1.6, (B, 2)), rng.uniform(0.5, 2.0, (B, 2))], axis=1).astype(np.float32)
    return z0, th


def run(B, T, iters):
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    d.rhs_kind, d.state_dim, d.param_dim, d.sensealg = L.RHS_DOUBLE_PENDULUM, 4, 4, L.SENSE_FORWARD_DUAL
    D, P, G = 4, 4, 8
    h = C.c_void_p()
    L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
    ts = time_grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = dpend_inputs(B)
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
    return dict(rhs="double pendulum", B=B, T=T, kernels=kern, record_bytes=nbytes, bytes_per_trajectory=io,
                steps_per_trajectory=round((st.naccept + st.nreject) / B, 2), max_steps=st.max_steps, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2, help="passes over the configurations (the systems alternate within a pass)")
    a = ap.parse_args()
    for _ in range(a.rounds):
        for B in a.B:
            print(json.dumps(kuramoto_time.run(0, B, a.T, a.iters)), flush=True)      # Lotka–Volterra
            print(json.dumps(run(B, a.T, a.iters)), flush=True)
            for N in (3, 4):
                print(json.dumps(kuramoto_time.run(N, B, a.T, a.iters)), flush=True)


if __name__ == "__main__":
    main()
