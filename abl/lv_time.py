"""The Lotka–Volterra solve's cost (LDE_RHS_LOTKA_VOLTERRA: k_lv_forward_dual / k_lv_adjoint_dual, six partials per component) beside the
pendulum's dual-number solve (k_pend_forward_dual / k_pend_adjoint_dual, three) on the same box in the same run: forward and pullback
through the C ABI at T = 50, Tsit5 at the default tolerances (1e-6 / 1e-3), caller-owned records, HIP events around `--iters` back-to-back
calls after a warm-up (as abl/dual_time.py, abl/sde_time.py). One JSON line per (right-hand side, B). Recorded in DESIGN.md §8.2, not gated.

    python abl/lv_time.py [--B 256 65536] [--T 50] [--iters 200]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from latentdiffeq_amd import _lib as L  # noqa: E402
from latentdiffeq_amd.synthetic import cotangent, pendulum_inputs, time_grid  # noqa: E402

CONFIGS = {"pendulum": (L.RHS_PENDULUM, 1), "lotka-volterra": (L.RHS_LOTKA_VOLTERRA, 4)}


def lv_inputs(B, seed=0):
    """x₀, y₀ ~ U(0.5, 2), α, β, γ, δ ~ U(0.5, 1.5): the ranges of tests/test_gpu_lv.py."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, (B, 2)).astype(np.float32), rng.uniform(0.5, 1.5, (B, 4)).astype(np.float32)


def run(name, B, T, iters):
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    d.rhs_kind, d.param_dim = CONFIGS[name]
    d.sensealg = L.SENSE_FORWARD_DUAL
    h = C.c_void_p()
    L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
    ts = time_grid(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = pendulum_inputs(B) if name == "pendulum" else lv_inputs(B)
    z0d, thd, dzd = (torch.from_numpy(a).cuda() for a in (z0, th, cotangent(T, B, 2)))
    out = torch.empty((T, B, 2), device="cuda")
    g0, gth = torch.empty((B, 2), device="cuda"), torch.empty((B, d.param_dim), device="cuda")
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
    return dict(rhs=name, B=B, T=T, kernels=kern, record_bytes=nbytes, steps_per_trajectory=round((st.naccept + st.nreject) / B, 2),
                max_steps=st.max_steps, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    for B in a.B:
        for name in CONFIGS:
            print(json.dumps(run(name, B, a.T, a.iters)), flush=True)


if __name__ == "__main__":
    main()
