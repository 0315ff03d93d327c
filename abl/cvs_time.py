"""The cardiovascular system's cost (LDE_RHS_CVS: CvsDir on k_forward_dual_dir / k_adjoint_dual_dir, six directions in one 8-lane group, two
pad lanes) beside the Kuramoto system's at N = 3 (8 lanes, one pad lane) and the double pendulum's (8 lanes, none) — the same kernels over
other systems — on the same box in the same run, alternating: forward and pullback through the C ABI at T = 50, Tsit5 at the default
tolerances (1e-6 / 1e-3), caller-owned records, HIP events around `--iters` back-to-back calls after a warm-up (abl/dpend_time.py's and
abl/kuramoto_time.py's runners, which this reuses for those two systems). CVS runs on ts = 1.0·j, its own time scale (TAU = 20 s; the
GOKU-net paper's Δt = 1); the other two on their scripts' 0.05·j, so that their rows are the ones DESIGN.md §8.3 / §8.4 already hold. What
compares across the three is therefore the time per step attempt: one JSON line per (right-hand side, B) with the step attempts per
trajectory and forward_us_per_attempt = forward_us / steps_per_trajectory. Recorded in DESIGN.md §8.6, not gated.

    python abl/cvs_time.py [--B 256 65536] [--T 50] [--iters 200] [--rounds 2]
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

import dpend_time  # noqa: E402
import kuramoto_time  # noqa: E402
from latentdiffeq_amd import _lib as L  # noqa: E402


def cvs_inputs(B, seed=0):
    """z₀ ~ U(0.75, 0.85), z₁ ~ U(0.5, 0.9), z₂ ~ U(0.15, 0.25), z₃ ~ U(0.9, 1.0), i_ext ~ U(−2, 0), r_mod ~ U(0, 0.3): the ranges of
    tests/test_gpu_cvs.py."""
    rng = np.random.default_rng(seed)
    z0 = np.stack([rng.uniform(0.75, 0.85, B), rng.uniform(0.5, 0.9, B), rng.uniform(0.15, 0.25, B), rng.uniform(0.9, 1.0, B)], axis=1)
    th = np.stack([rng.uniform(-2.0, 0.0, B), rng.uniform(0.0, 0.3, B)], axis=1)
    return z0.astype(np.float32), th.astype(np.float32)


def run(B, T, iters):
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    d.rhs_kind, d.state_dim, d.param_dim, d.sensealg = L.RHS_CVS, 4, 2, L.SENSE_FORWARD_DUAL
    D, P, G = 4, 2, 8
    h = C.c_void_p()
    L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
    ts = 1.0 * np.arange(T)
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    z0, th = cvs_inputs(B)
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
    return dict(rhs="cvs", B=B, T=T, kernels=kern, record_bytes=nbytes, bytes_per_trajectory=io, nfailed=st.nfailed,
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
    a = ap.parse_args()
    for _ in range(a.rounds):
        for B in a.B:
            print(json.dumps(per_attempt(run(B, a.T, a.iters))), flush=True)
            print(json.dumps(per_attempt(kuramoto_time.run(3, B, a.T, a.iters))), flush=True)
            print(json.dumps(per_attempt(dpend_time.run(B, a.T, a.iters))), flush=True)


if __name__ == "__main__":
    main()
