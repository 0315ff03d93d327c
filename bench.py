#!/usr/bin/env python3
"""bench.py — trajectories/sec (forward solve + adjoint) of the latent-ODE hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload goku_pendulum|c2|c3|c4|latentode_ref|goku_decoder|goku_step] [--batch B]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one lde_forward + one lde_adjoint over one batch of synthetic trajectories whose inputs are
already resident in HBM. Default workload = BASELINE.json's metric config: GOKU pendulum (D=2, P=1, T=50,
t=0:0.05:2.45, Tsit5 abstol=1e-6 reltol=1e-3), batch 256 PER GPU (weak scaling: the batch shards by
trajectory with no data-path collective; a collective exists only for workloads with shared RHS-MLP
weights, whose dW is all-reduced once per step).

Prints ONE JSON line on rank 0 (the driver's contract). A plain run sets up, warms up, times the K steps and
prints the headline (metric, value, unit, higher_is_better, dtype, ms_per_step, …). `--full` adds what takes runs of
its own, as before:
  "roofline":     dominant kernel's algorithmic bytes / its average launch duration (HIP events on the launch stream)
  "cpu_baseline": the CPU oracle (a port of the same algorithm, OpenMP over trajectories like the reference's
                  EnsembleThreads [REF src/models/GOKU.jl:121]) timed on this box's host cores, bounded sample
  and the per-kernel / per-call figures, the other definition of the gradient, the strong-scaling rider (N > 1) and
  `--sweep`'s large batches (which implies --full).
`--dump-outputs DIR` writes what the timed path computed in its last step as DIR/<name>.npy (see dump_outputs).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: peak FP32 vector == matrix (f32-in MFMA)
BF16_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA peak (no sparsity)

WORKLOADS = {
    # name: dict(describing BASELINE.json configs; SURVEY.md §8d inputs)
    "goku_pendulum": dict(desc="GOKU pendulum D=2 P=1 T=50 Tsit5 abstol=1e-6 reltol=1e-3, per-trajectory", B=256,
                          rhs="pendulum", D=2, P=1, T=50, layers=(), solver="tsit5", batching="per_trajectory"),
    "c2": dict(desc="LatentODE D=8 8-200-200-8 relu, RK4 fixed dt=0.05, coupled", B=256, rhs="mlp", D=8, P=0, T=50,
               layers=(8, 200, 200, 8), solver="rk4", batching="coupled", dt=0.05),
    "c3": dict(desc="GOKU pendulum + 2-64-64-2 MLP, Tsit5, per-trajectory", B=1024, rhs="pendulum_plus_mlp", D=2, P=1,
               T=50, layers=(2, 64, 64, 2), solver="tsit5", batching="per_trajectory"),
    "c4": dict(desc="LatentODE D=32 32-128-128-32 relu, Tsit5, coupled (512 per GPU)", B=512, rhs="mlp", D=32, P=0,
               T=50, layers=(32, 128, 128, 32), solver="tsit5", batching="coupled"),
    # the reference's own LatentODE example [REF examples/pendulum_friction-less/model_train_LatentODE.jl:37, :42], [REF nODE.jl:11-16]
    "latentode_ref": dict(desc="LatentODE reference example: NODE(16) 16-200-200-16 relu, Tsit5, coupled, batch 64", B=64, rhs="mlp",
                          D=16, P=0, T=50, layers=(16, 200, 200, 16), solver="tsit5", batching="coupled"),
}


# The reference's default definition of the gradient, per workload: the GOKU path carries ForwardDiffSensitivity() — the exact derivative of
# the discrete solve [REF examples/pendulum_friction-less/pendulum.jl:8-11], [REF src/models/GOKU.jl:107, :121] = LDE_SENSE_DISCRETE; a
# NeuralODE carries DiffEqFlux's InterpolatingAdjoint [REF src/models/LatentODE.jl:67-70] = the continuous adjoint.
REF_SENSEALG = {"goku_pendulum": "discrete", "c3": "discrete", "goku_decoder": "discrete", "goku_step": "discrete",
                "c2": "continuous", "c4": "continuous", "latentode_ref": "continuous"}


def resolve_sensealg(workload, arg):
    return REF_SENSEALG[workload] if arg == "default" else arg


def build_problem(w, B, seed_shift=0, sensealg="discrete"):
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import synthetic as O
    lib = L.load()
    d = L.ProblemDesc()
    lib.lde_problem_desc_default(C.byref(d))
    d.rhs_kind = {"pendulum": L.RHS_PENDULUM, "mlp": L.RHS_MLP, "pendulum_plus_mlp": L.RHS_PENDULUM_PLUS_MLP}[w["rhs"]]
    d.state_dim, d.param_dim = w["D"], w["P"]
    d.n_layers = max(len(w["layers"]) - 1, 0)
    for i, s in enumerate(w["layers"]):
        d.layer_sizes[i] = s
    d.solver = L.SOLVER_TSIT5 if w["solver"] == "tsit5" else L.SOLVER_RK4
    d.batching = L.BATCH_COUPLED if w["batching"] == "coupled" else L.BATCH_PER_TRAJECTORY
    if w["solver"] == "rk4":
        d.adaptive, d.dt = 0, w["dt"]
    # LDE_SENSE_DISCRETE: what the reference's GOKU default ForwardDiffSensitivity() differentiates [REF pendulum.jl:11]; continuous: the
    # time-parallel checkpointed adjoint on the GOKU path, the sequential checkpointed one for MLP right-hand sides (lde_create's mapping)
    assert sensealg in ("discrete", "continuous"), sensealg
    d.sensealg = L.SENSE_DISCRETE if sensealg == "discrete" else L.SENSE_PARALLEL_CHECKPOINTED
    T, D = w["T"], w["D"]
    ts = O.time_grid(T)
    if w["rhs"] == "mlp":
        rng = np.random.default_rng(1 + seed_shift)
        z0 = (0.5 * rng.standard_normal((B, D))).astype(np.float32)
        theta = None
    else:
        z0, theta = O.pendulum_inputs(B, seed=1 + seed_shift)
    W = O.mlp_weights(w["layers"], seed=3, scale=1.0) if w["layers"] else None
    dz = O.cotangent(T, B, D, seed=2 + seed_shift)
    return d, ts, z0, theta, W, dz


def alg_bytes_per_traj(w):
    """fwd reads 4(D+P), writes 4·D'·T; adjoint reads 4·D'·T, writes 4(D+P)."""
    D, P, T = w["D"], w["P"], w["T"]
    fwd = 4 * (D + P) + 4 * D * T
    bwd = 4 * D * T + 4 * (D + P)
    return fwd, bwd


def flops_per_eval(w):
    return 2 * sum(a * b for a, b in zip(w["layers"][:-1], w["layers"][1:])) if w["layers"] else 0


def cpu_baseline(w, d_native, ts, z0, theta, W, dz, budget_s=12.0):
    """Time the CPU oracle (same algorithm, -O3 -march=native build, OpenMP over trajectories) on a bounded sample.

    GOKU workloads with the reference's default gradient (LDE_SENSE_DISCRETE): `value` is the algorithm the reference's CPU path RUNS —
    the solve on dual numbers, D + P partials through every stage, then Σ_j J_jᵀΔ_j (oracle_forward_dual: ForwardDiffSensitivity as
    SciMLSensitivity executes it, dual-aware error norm included [REF src/models/GOKU.jl:107, :121]); `reverse_sweep` beside it is the same
    derivative taken the cheaper way on the CPU too (record the steps, sweep them in reverse: what the kernels do). Both ratios are the
    bench line's to print. Median of three samples at the fastest thread count (the figure moved ±12 % run to run as one long sample)."""
    from oracle import oracle as O
    try:
        orc = O.Oracle("f32", native=True)
    except Exception:
        orc = O.Oracle("f32")
    od = O.Desc()
    C.memmove(C.byref(od), C.byref(d_native), C.sizeof(od))
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    B = z0.shape[0]
    # bounded sample: the same workload, at most `cap` trajectories per pass
    cap = B if w["batching"] == "per_trajectory" else min(B, 64)
    z0s, ths, dzs = z0[:cap], (None if theta is None else theta[:cap]), dz[:, :cap]
    disc = od.sensealg == O.SENSE_DISCRETE
    dual = disc and w["rhs"] == "pendulum"       # (the analytic GOKU path: what the reference differentiates by dual numbers)

    def reverse(nt):
        z, _, rec, _ = orc.forward_steps(od, z0s, ths, ts, W=W, cap=1024, nthreads=nt)
        orc.adjoint_discrete(od, z, ths, ts, dzs, rec, W=W, nthreads=nt)

    def one(nt):
        if dual:      # forward solve on duals (the Jacobians stay in the solve's buffers) + the pullback's contraction
            orc.forward_dual(od, z0s, ths, ts, dz_out=dzs, dual_norm=True, cap=1024, nthreads=nt, keep_jac=False)
        elif disc:    # the same definition of the gradient on the CPU: record the steps, sweep them in reverse
            reverse(nt)
        else:
            z, _, _ = orc.forward(oc_seq, z0s, ths, ts, W=W, nthreads=nt)
            orc.adjoint(oc_seq, z, ths, ts, dzs, W=W, nthreads=nt)

    # the continuous adjoint on the CPU: the sequential checkpointed form whatever form the GPU runs (the time-parallel one restarts the solver
    # in each of the T − 1 intervals — what pays on a GPU costs a CPU a factor two: 0.47 M against 0.88 M trajectories/s at the metric shape)
    oc_seq = O.Desc()
    C.memmove(C.byref(oc_seq), C.byref(od), C.sizeof(oc_seq))
    if not disc and od.sensealg == O.SENSE_PARALLEL_CHECKPOINTED:
        oc_seq.sensealg = O.SENSE_BACKSOLVE_CHECKPOINTED

    def rate(fn, nt, budget):
        fn(nt)  # warm-up (thread pool, page faults)
        n, t0 = 0, time.perf_counter()
        while True:
            fn(nt)
            n += 1
            el = time.perf_counter() - t0
            if el > budget:
                return n, el

    # EnsembleThreads analogue (per-trajectory mode: OpenMP over trajectories; coupled mode: OpenMP over the columns of every
    # stage evaluation, the role OpenBLAS threads play under the reference's per-stage sgemms): pick the thread count that is
    # fastest on this box (more threads than work only adds fork/join cost), then time that one.
    cands = sorted({1, 8, 16, 32, 64, min(avail, 128), avail} & set(range(1, avail + 1)))
    best, best_r = 1, 0.0
    for nt in cands:
        n, el = rate(one, nt, 0.6)
        if n * cap / el > best_r:
            best, best_r = nt, n * cap / el
    nthreads = best
    samples = []
    for _ in range(3):
        n, el = rate(one, nthreads, budget_s / 4.0)
        samples.append((n * cap / el, n, el))
    samples.sort()
    val, n, el = samples[1]
    out = dict(value=val, unit="trajectories/s", cores=nthreads, kind="port",
               sample=f"median of 3 samples ({samples[0][0]:.0f} / {samples[1][0]:.0f} / {samples[2][0]:.0f}); the median one: {n} passes of fwd+adjoint over "
                      f"{cap} trajectories of the same workload, {el:.1f} s wall, {nthreads} OpenMP thread(s) (fastest of {cands} on {avail} "
                      f"available cores; {cpu_model()})",
               algorithm=("the solve on dual numbers (D + P = 3 partials per state component, dual-aware error norm) + the pullback's contraction: "
                          "ForwardDiffSensitivity as the reference's CPU path executes it" if dual else
                          "forward solve recording its steps + reverse sweep over them (LDE_SENSE_DISCRETE on the CPU)" if disc else
                          "forward solve + reverse-time continuous adjoint (sequential, checkpointed at the save times: the faster form on a CPU)"))
    if dual:
        def best_of(fn):   # (its own fastest thread count: the three algorithms parallelise differently)
            r = []
            for nt in cands:
                n_, el_ = rate(fn, nt, 0.5)
                r.append((n_ * cap / el_, nt))
            nt = max(r)[1]
            rs = sorted(rate(fn, nt, budget_s / 10.0) for _ in range(3))
            return rs[1][0] * cap / rs[1][1], nt

        def continuous(nt):
            oc = O.Desc()
            C.memmove(C.byref(oc), C.byref(od), C.sizeof(oc))
            oc.sensealg = O.SENSE_BACKSOLVE_CHECKPOINTED
            z, _, _ = orc.forward(oc, z0s, ths, ts, W=W, nthreads=nt)
            orc.adjoint(oc, z, ths, ts, dzs, W=W, nthreads=nt)
        v, nt = best_of(reverse)
        out["reverse_sweep"] = dict(value=v, unit="trajectories/s", cores=nt,
                                    what="the same derivative by recording the steps and sweeping them in reverse on the CPU (what the kernels do)")
        v, nt = best_of(continuous)
        out["continuous_adjoint"] = dict(value=v, unit="trajectories/s", cores=nt,
                                         what="forward solve + reverse-time continuous adjoint on the CPU: rounds 1-5's denominator (418-517 k)")
    return out


DUMP_BUDGET_BYTES = 60 << 20     # (under 64 MB however a megabyte is counted, .npy headers included)


def dump_outputs(dirname, arrays):
    """--dump-outputs: the arrays a caller of the timed path receives from its last step, as DIR/<name>.npy — float64 stays
    float64, everything else (f32, bf16, int32 return codes) is written as float32. At most DUMP_BUDGET_BYTES in all: an array
    that does not fit its share is replaced by a fixed sample of its elements (seeded by its name, flat order kept), so that two
    builds run with the same arguments compare element for element."""
    import zlib

    import torch
    os.makedirs(dirname, exist_ok=True)
    host = {}
    for name, a in arrays.items():
        if a is None:
            continue
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu()
            a = (a if a.dtype == torch.float64 else a.float()).numpy()
        a = np.asarray(a)
        host[name] = np.ascontiguousarray(a if a.dtype == np.float64 else a.astype(np.float32))
    left, n_left = DUMP_BUDGET_BYTES, len(host)
    for name, a in sorted(host.items(), key=lambda kv: kv[1].nbytes):
        share = left // n_left
        if a.nbytes > share:
            k = share // a.itemsize
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)
        left -= a.nbytes
        n_left -= 1


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            names = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")]
        return f"{names[0]}, {len(names)} logical CPUs" if names else "unknown CPU"
    except OSError:
        return "unknown CPU"


# ---- decoder path: apply_latent_out → diffeq_layer → apply_reconstructor and its pullback (scope row f-1) ----------
DECODER = dict(desc="GOKU decoder: latent_out (16-200-2, 16-200-1 softplus) -> pendulum solve (Tsit5) -> reconstructor "
                    "(2-200-200-200-784, skips, sigmoid), forward + pullback", B=256, T=50, input_dim=784, latent=16)


def run_decoder(args, torch, dist, world, rank, local):
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd import synthetic as S
    lib = L.load()
    w = WORKLOADS["goku_pendulum"]
    B = args.batch or DECODER["B"]
    T, D, P, NI, NL = DECODER["T"], 2, 1, DECODER["input_dim"], DECODER["latent"]
    N = B * T
    dev = torch.device("cuda", local)
    d, ts, _, _, _, _ = build_problem(w, B, seed_shift=rank, sensealg=resolve_sensealg("goku_decoder", args.sensealg))
    h = C.c_void_p()
    L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
    L.check(lib.lde_reserve(h, B, T), h, "lde_reserve")
    specs = {  # [REF src/models/GOKU.jl:252-269]
        "lo_z0": ((NL, 200, D), (L.CACT_RELU, L.CACT_IDENTITY), (0, 0)),
        "lo_th": ((NL, 200, P), (L.CACT_RELU, L.CACT_SOFTPLUS), (0, 0)),
        "rec": ((D, 200, 200, 200, NI), (L.CACT_RELU, L.CACT_RELU, L.CACT_RELU, L.CACT_SIGMOID), (0, 1, 1, 0)),
    }
    chains, weights = {}, {}
    for i, (name, (sizes, acts, skips)) in enumerate(specs.items()):
        cdsc = L.ChainDesc()
        cdsc.abi_version, cdsc.n_layers = L.LDE_ABI_VERSION, len(sizes) - 1
        for k, v in enumerate(sizes):
            cdsc.sizes[k] = v
        for k, (a_, s_) in enumerate(zip(acts, skips)):
            cdsc.activation[k], cdsc.skip[k] = a_, s_
        ch = C.c_void_p()
        L.check(lib.lde_chain_create(C.byref(cdsc), C.byref(ch)), ch if ch else None, "lde_chain_create", chain=True)
        Wc = S.mlp_weights(sizes, seed=20 + i, scale=0.5 if name != "rec" else 1.0)
        if name == "lo_th":   # keep the pendulum length L = softplus(·) in the data range U(1,2)
            Wc[-1] = 1.0
        L.check(lib.lde_chain_set_weights(ch, Wc.ctypes.data_as(C.c_void_p), Wc.size), ch, "lde_chain_set_weights", chain=True)
        L.check(lib.lde_chain_reserve(ch, N if name == "rec" else B), ch, "lde_chain_reserve", chain=True)
        if args.dtype == "mixed":
            L.check(lib.lde_chain_set_dtype(ch, L.DTYPE_BF16), ch, "lde_chain_set_dtype", chain=True)
        chains[name], weights[name] = (ch, sizes), Wc
    rng = np.random.default_rng(40 + rank)
    zt = torch.from_numpy((0.6 * rng.standard_normal((B, NL))).astype(np.float32)).to(dev)     # l̃ = (z̃₀, θ̃)
    tt = torch.from_numpy((0.6 * rng.standard_normal((B, NL))).astype(np.float32)).to(dev)
    dxh = torch.from_numpy((rng.standard_normal((N, NI)) / (N * NI)).astype(np.float32)).to(dev)  # ∂L/∂x̂ of an MSE
    z0 = torch.empty((B, D), device=dev); th = torch.empty((B, P), device=dev)
    zout = torch.empty((T, B, D), device=dev); ret = torch.empty((B,), device=dev, dtype=torch.int32)
    xhat = torch.empty((N, NI), device=dev)
    dz = torch.empty((T, B, D), device=dev); dz0 = torch.empty((B, D), device=dev); dth = torch.empty((B, P), device=dev)
    dzt = torch.empty((B, NL), device=dev); dtt = torch.empty((B, NL), device=dev)
    nWs = {k: int(v.size) for k, v in weights.items()}
    flat = torch.zeros((sum(nWs.values()),), device=dev)      # ONE flat gradient buffer ⇒ one all-reduce
    offs, o = {}, 0
    for k in specs:
        offs[k] = o
        o += nWs[k]
    gW = {k: flat[offs[k]:offs[k] + nWs[k]] for k in specs}
    tsp = ts.ctypes.data_as(C.POINTER(C.c_double))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    ck = lambda rc, ch, what: L.check(rc, ch, what, chain=True)
    # the training variant of the chains: the forward call keeps the hidden activations for the pullback
    saved = {k: torch.empty((int(lib.lde_chain_saved_floats(chains[k][0], N if k == "rec" else B)),), device=dev) for k in specs}

    # apply_latent_out's two chains act on B columns only: one grouped call each way (lde_chain_group_*: one launch per stage)
    arr2 = lambda a, b: (C.c_void_p * 2)(a, b)
    lo_h = arr2(chains["lo_z0"][0].value, chains["lo_th"][0].value)
    lo_N = (C.c_int64 * 2)(B, B)
    lo_x, lo_y = arr2(zt.data_ptr(), tt.data_ptr()), arr2(z0.data_ptr(), th.data_ptr())
    lo_sv = arr2(saved["lo_z0"].data_ptr(), saved["lo_th"].data_ptr())
    lo_dy, lo_dx = arr2(dz0.data_ptr(), dth.data_ptr()), arr2(dzt.data_ptr(), dtt.data_ptr())
    lo_dW = arr2(gW["lo_z0"].data_ptr(), gW["lo_th"].data_ptr())

    def fwd():
        ck(lib.lde_chain_group_forward_save(2, lo_h, lo_x, lo_N, lo_y, lo_sv, sp), chains["lo_z0"][0], "latent_out fwd")
        L.check(lib.lde_forward(h, p(z0), p(th), tsp, T, B, p(zout), p(ret), sp), h, "lde_forward")
        ck(lib.lde_chain_forward_save(chains["rec"][0], p(zout), N, p(xhat), p(saved["rec"]), sp), chains["rec"][0], "rec fwd")

    def bwd():
        flat.zero_()
        ck(lib.lde_chain_backward_saved(chains["rec"][0], p(zout), p(xhat), p(dxh), p(saved["rec"]), N, p(dz), p(gW["rec"]), sp),
           chains["rec"][0], "rec bwd")
        L.check(lib.lde_adjoint(h, p(zout), p(th), tsp, T, B, p(dz), p(dz0), p(dth), C.c_void_p(), sp), h, "lde_adjoint")
        ck(lib.lde_chain_group_backward_saved(2, lo_h, lo_x, lo_y, lo_dy, lo_sv, lo_N, lo_dx, lo_dW, sp), chains["lo_z0"][0], "latent_out bwd")
        if world > 1:
            dist.all_reduce(flat)     # the one collective: shared decoder parameters

    def step():
        fwd()
        bwd()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()          # this rank's K steps are done: its clock stops here; the closing barrier follows, and the MAX over
    el = time.perf_counter() - t0     # ranks (below) is the job's time — the barrier's own latency (an RCCL collective) is not a step
    if world > 1:
        dist.barrier()
    if world > 1:
        tmax = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        el = float(tmax.item())
    assert int(ret.abs().sum().item()) == 0 and bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0

    # the last timed step's results, before the --full probes below launch the same calls on these buffers again
    dumped = {k: v.clone() for k, v in dict(x_hat=xhat, z_hat=zout, retcode=ret, dW=flat, dl_z0=dzt, dl_theta=dtt).items()} if args.dump_outputs else None
    ms_per_step = el / args.steps * 1e3
    out = {
        "metric": "trajectories/sec (latent_out -> solve -> reconstructor, forward + pullback) goku_decoder",
        "value": B * world * args.steps / el, "unit": "trajectories/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.dtype == "f32" else "bf16 operands / f32 accumulate (dense chains), f32 solve", "data": "synthetic",
        "config": {"workload": f"goku_decoder: {DECODER['desc']}", "batch_per_gpu": B, "global_batch": B * world,
                   "save_points": T, "columns_through_the_reconstructor": N,
                   "parallelism": f"dp{world} (batch sharded by trajectory; one all-reduce of the flat decoder gradient per step)"},
        "roofline": None, "cpu_baseline": None,
    }
    if args.full:   # per-call HIP-event times, the MFMA roofline of the dominant chain kernel (+ its HBM view), the CPU baseline
        def ev_ms(fn, n):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for a, b in evs:
                a.record(stream); fn(); b.record(stream)
            torch.cuda.synchronize()
            return float(np.mean([a.elapsed_time(b) for a, b in evs]))

        n = min(args.steps, 50)
        parts = {
            "reconstructor_forward": ev_ms(lambda: ck(lib.lde_chain_forward_save(chains["rec"][0], p(zout), N, p(xhat), p(saved["rec"]), sp), chains["rec"][0], "f"), n),
            "reconstructor_backward": ev_ms(lambda: ck(lib.lde_chain_backward_saved(chains["rec"][0], p(zout), p(xhat), p(dxh), p(saved["rec"]), N, p(dz), p(gW["rec"]), sp), chains["rec"][0], "b"), n),
            "reconstructor_backward_recompute": ev_ms(lambda: ck(lib.lde_chain_backward(chains["rec"][0], p(zout), p(xhat), p(dxh), N, p(dz), p(gW["rec"]), sp), chains["rec"][0], "b"), n),
            "lde_forward": ev_ms(lambda: L.check(lib.lde_forward(h, p(z0), p(th), tsp, T, B, p(zout), p(ret), sp), h, "f"), n),
            "lde_adjoint": ev_ms(lambda: L.check(lib.lde_adjoint(h, p(zout), p(th), tsp, T, B, p(dz), p(dz0), p(dth), C.c_void_p(), sp), h, "a"), n),
            "latent_out_forward_x2": ev_ms(lambda: lib.lde_chain_group_forward_save(2, lo_h, lo_x, lo_N, lo_y, lo_sv, sp), n),
            "latent_out_backward_x2": ev_ms(lambda: lib.lde_chain_group_backward_saved(2, lo_h, lo_x, lo_y, lo_dy, lo_sv, lo_N, lo_dx, lo_dW, sp), n),
            "latent_out_forward_separate_calls": ev_ms(lambda: (lib.lde_chain_forward_save(chains["lo_z0"][0], p(zt), B, p(z0), p(saved["lo_z0"]), sp),
                                                                lib.lde_chain_forward_save(chains["lo_th"][0], p(tt), B, p(th), p(saved["lo_th"]), sp)), n),
            "latent_out_backward_separate_calls": ev_ms(lambda: (lib.lde_chain_backward_saved(chains["lo_z0"][0], p(zt), p(z0), p(dz0), p(saved["lo_z0"]), B, p(dzt), p(gW["lo_z0"]), sp),
                                                                 lib.lde_chain_backward_saved(chains["lo_th"][0], p(tt), p(th), p(dth), p(saved["lo_th"]), B, p(dtt), p(gW["lo_th"]), sp)), n),
        }
        mac = lambda sizes: sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
        F_rec = 2 * mac(specs["rec"][0]) * N
        F_lo = 2 * (mac(specs["lo_z0"][0]) + mac(specs["lo_th"][0])) * B
        # algorithmic flops of a step: forward F, pullback 2F (input + weight gradients); the solve's flops are negligible here
        flops = 3 * (F_rec + F_lo)
        dom = max(("reconstructor_forward", "reconstructor_backward"), key=lambda k: parts[k])
        dom_flops = F_rec if dom == "reconstructor_forward" else 2 * F_rec
        ach = dom_flops / (parts[dom] * 1e-3) / 1e12
        out["roofline"] = dict(bound="mfma", kernel=f"lde_chain {dom}", achieved=ach, peak=FP32_PEAK_TFLOPS if args.dtype == "f32" else BF16_PEAK_TFLOPS, unit="TFLOP/s",
                               frac=ach / (FP32_PEAK_TFLOPS if args.dtype == "f32" else BF16_PEAK_TFLOPS), traffic=None, alg_flops_per_launch=dom_flops, avg_launch_ms=parts[dom],
                               whole_step_TFLOPs=flops / (ms_per_step * 1e-3) / 1e12)
        out["kernel_ms"] = parts
        hv, tr, trk = chain_hbm_view("goku_decoder", args.dtype != "f32")
        if hv:   # the bf16 chain kernels move 2.4–4 TB/s of counter bytes: HBM-bound, not MFMA-bound — both views side by side
            out["roofline"]["traffic"] = tr
            out["roofline"]["traffic_kernel"] = trk
            out["roofline"]["hbm_view"] = hv
            if args.dtype != "f32":
                out["roofline"]["bound"] = "hbm (mixed: see hbm_view; the MFMA fraction is quoted beside it)"
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = decoder_cpu_baseline(specs, weights, d, ts, zt.cpu().numpy(), tt.cpu().numpy(), dxh.cpu().numpy(), B, T)
    for ch, _ in chains.values():
        lib.lde_chain_destroy(ch)
    lib.lde_destroy(h)
    if world > 1 or (dist.is_available() and dist.is_initialized()):
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        if dumped is not None:
            dump_outputs(args.dump_outputs, dumped)
        emit(out)


def decoder_cpu_baseline(specs, weights, d_native, ts, zt, tt, dxh, B, T, budget_s=12.0):
    """The same decoder step with the CPU oracle (OpenMP over columns / trajectories), bounded sample."""
    from oracle import oracle as O
    try:
        orc = O.Oracle("f32", native=True)
    except Exception:
        orc = O.Oracle("f32")
    od = O.Desc()
    C.memmove(C.byref(od), C.byref(d_native), C.sizeof(od))
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cd = {k: O.make_chain_desc(*v) for k, v in specs.items()}
    cap = min(B, 64)                         # bounded sample: 64 trajectories × T columns
    zs, tsm, dxs = zt[:cap], tt[:cap], dxh.reshape(T, B, -1)[:, :cap].reshape(T * cap, -1)

    def one(nt):
        z0 = orc.chain_forward(cd["lo_z0"], weights["lo_z0"], zs, nthreads=nt)
        th = orc.chain_forward(cd["lo_th"], weights["lo_th"], tsm, nthreads=nt)
        disc = od.sensealg == O.SENSE_DISCRETE
        if disc:
            z, _, rec, _ = orc.forward_steps(od, z0, th, ts, cap=1024, nthreads=nt)
        else:
            z, _, _ = orc.forward(od, z0, th, ts, nthreads=nt)
        zc = z.reshape(T * cap, -1)
        orc.chain_forward(cd["rec"], weights["rec"], zc, nthreads=nt)
        dz, _ = orc.chain_backward(cd["rec"], weights["rec"], zc, dxs, nthreads=nt)
        if disc:
            g0, gth, _, _ = orc.adjoint_discrete(od, z, th, ts, dz.reshape(T, cap, -1), rec, nthreads=nt)
        else:
            g0, gth, _, _ = orc.adjoint(od, z, th, ts, dz.reshape(T, cap, -1), nthreads=nt)
        orc.chain_backward(cd["lo_z0"], weights["lo_z0"], zs, g0, nthreads=nt)
        orc.chain_backward(cd["lo_th"], weights["lo_th"], tsm, gth, nthreads=nt)

    def rate(nt, budget):
        one(nt)
        n, t0 = 0, time.perf_counter()
        while True:
            one(nt)
            n += 1
            el = time.perf_counter() - t0
            if el > budget:
                return n, el

    cands = sorted({1, 8, 16, 32, 64, min(avail, 128), avail} & set(range(1, avail + 1)))
    best, best_r = 1, 0.0
    for nt in cands:
        n, el = rate(nt, 1.0)
        if n * cap / el > best_r:
            best, best_r = nt, n * cap / el
    n, el = rate(best, budget_s)
    return dict(value=n * cap / el, unit="trajectories/s", cores=best, kind="port",
                sample=f"{n} passes of the decoder step over {cap} trajectories ({cap * T} reconstructor columns), {el:.1f} s wall, "
                       f"{best} OpenMP thread(s) (fastest of {cands} on {avail} available cores; {cpu_model()})")


# ---- whole GOKU training step (BASELINE.json configs[4] shape, one GPU's share): encoder → sample → decoder → loss → pullback → AdamW
def run_goku_step(args, torch, dist, world, rank, local):
    import latentdiffeq_amd as M
    from latentdiffeq_amd import recurrent as _rec
    if os.environ.get("LDE_BENCH_GRAPH", "1") != "0":
        _rec._BRANCH_STREAMS = False   # the captured step runs on one stream (a module attribute of the host code: nothing reads the environment)
    from latentdiffeq_amd.chain import decode, decode_loss, default_decoder_layers
    from latentdiffeq_amd.dist import FlatGradAllReduce
    from latentdiffeq_amd.loss import reconstruction_loss, sample, sample_with_kl, vector_kl
    from latentdiffeq_amd.loss import backward as loss_backward     # loss.backward() seeded from a constant 1 (no fill launch per step)
    from latentdiffeq_amd.recurrent import Encoder, default_encoder_layers, encode
    from latentdiffeq_amd import _lib as L
    B = args.batch or 256
    T, NI = 50, 784
    dev = torch.device("cuda", local)
    torch.manual_seed(100)                  # the same initial weights on every rank (data parallel); the data differs per rank
    mt = M.GOKU_basic()
    # Pendulum() carries the reference's GOKU default, ForwardDiffSensitivity = LDE_SENSE_DISCRETE [REF pendulum.jl:8-11]; --sensealg continuous:
    # the time-parallel continuous adjoint instead
    diffeq = M.Pendulum() if resolve_sensealg("goku_step", args.sensealg) == "discrete" else M.Pendulum(sensealg=M.ParallelAdjoint())
    enc = Encoder(mt, default_encoder_layers(mt, NI, device=dev))
    dec = M.Decoder(mt, default_decoder_layers(mt, NI, diffeq, device=dev))
    lo_z0, lo_th = dec.latent_out
    with torch.no_grad():   # start inside the data range of the pendulum length, L ~ U(1,2) [REF create_data.jl:19-22]
        lo_th._dense[-1].bias.fill_(1.0)
    mods = [enc.feature_extractor, *enc.pattern_extractor, *enc.latent_in, lo_z0, lo_th, dec.reconstructor]
    if args.dtype == "mixed":   # BASELINE.json configs[4]: bf16 encoder-decoder (the dense chains), f32 solve; the recurrent stacks stay f32
        for m in (enc.feature_extractor, *enc.latent_in, lo_z0, lo_th, dec.reconstructor):
            m.set_dtype("bf16")
    params = [p for m in mods for p in m.parameters()]
    from latentdiffeq_amd.train import FluxADAMW, GraphedStep
    # one GPU: the whole step is captured in a hipGraph and replayed (train.GraphedStep; needs the encoder's branch streams off — read when
    # the package was imported); LDE_BENCH_GRAPH=0 or a process group: eager
    use_graph = os.environ.get("LDE_BENCH_GRAPH", "1") != "0" and not _rec._BRANCH_STREAMS
    unroll = 1
    split = use_graph and (world > 1 or os.environ.get("LDE_BENCH_FORCE_PG") == "1")
    if os.environ.get("LDE_BENCH_FORCE_PG") == "1":
        from latentdiffeq_amd import dist as _ldist
        _ldist.FORCE_ALLREDUCE = True   # (a one-rank RCCL group on a one-GPU box still runs the collective)   # several GPUs: graph · all-reduce (eager) · graph
    opt = FluxADAMW(params, lr=1e-3, decay=1e-10, capturable=use_graph)   # ADAMW(η, β, decay), Flux flavour [REF model_train.jl:138, :150]; one fused update kernel
    sync = FlatGradAllReduce(params)
    torch.manual_seed(1000 + rank)
    x = torch.rand(T, B, NI, device=dev).permute(2, 1, 0)                   # synthetic frames in [0, 1], this rank's shard: [pixels, B, T] in the
                                                                            # reference's column-major memory order (pixels fastest), like ẑ
    ts = np.arange(T) * 0.05
    Bg = B * world

    # default: on for the f32 step (1.036 → 0.998 ms), off for the mixed one (its bf16 weight-gradient kernel is HBM-bound and slows what it runs beside: 0.491 → 0.502 ms)
    async_dw = args.async_dw >= 1 or (args.async_dw == -1 and args.dtype == "f32" and use_graph and world == 1)
    if async_dw:
        # what has something to run beside: the reconstructor's weight gradient (the solve's adjoint, the small chains, the recurrent stacks'
        # pullback follow it) and the stacks' (the feature extractor's pullback follows); the feature extractor's own is the last kernel of the
        # pullback. (--async-dw 2: the stacks' only, 3: the reconstructor's only)
        L.set_async_weight_gradients(True, dev)
        off = [enc.feature_extractor, *enc.latent_in, lo_z0, lo_th] + ([dec.reconstructor] if args.async_dw == 2 else [])
        for m in off:
            L.check(L.load().lde_chain_set_option(m._native(), b"async_dw", 0.0), m._native(), "lde_chain_set_option", chain=True)
        if args.async_dw == 3:
            for m in enc.pattern_extractor:
                L.check(L.load().lde_rnn_set_option(m._native(), b"async_dw", 0.0), m._native(), "lde_rnn_set_option", rnn=True)
    fused_loss = True     # (False: separate sample / vector_kl / reconstruction_loss and torch additions — tests/test_gpu_loss.py compares the two)
    refresh = True   # one k_refresh_many launch re-packs every module's weights after the update (instead of an upload at each module's next call)

    def step():
        opt.zero_grad(set_to_none=True)
        mu, logvar = encode(enc, x)
        if fused_loss:   # sample and β·KL of the same (μ, logσ²) in one pass, the additions folded into the reductions (train.loss_batch)
            l_tilde, bkl = sample_with_kl(mu, logvar, 1e-3, Bg)
            loss, _ = decode_loss(dec, l_tilde, ts, x, Bg, plus=bkl, want_x_hat=False)   # Σ_pixels mean_{B,T} + β·KL  [REF model_train.jl:225-238]; the step keeps no x̂
        else:
            l_tilde = sample(mu, logvar)
            x_hat, z_hat, l_hat = decode(dec, l_tilde, ts)
            loss = reconstruction_loss(x, x_hat, Bg) + 1e-3 * vector_kl(mu, logvar, Bg)
        loss_backward(loss)
        L.join_weight_gradients()
        sync()
        opt.step()
        if refresh:
            L.refresh_weights(mods)         # the new weights of all eleven modules handed to the library in one launch
        return loss

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def step_a():        # zero_grad … backward
        opt.zero_grad(set_to_none=True)
        mu, logvar = encode(enc, x)
        l_tilde, bkl = sample_with_kl(mu, logvar, 1e-3, Bg)
        loss, _ = decode_loss(dec, l_tilde, ts, x, Bg, plus=bkl, want_x_hat=False)
        loss_backward(loss)
        return loss

    def step_b():        # update + weight hand-over
        opt.step()
        if refresh:
            L.refresh_weights(mods)

    if split:
        gs = GraphedStep(step_a, warmup=3, between=sync, fn2=step_b)
        run = gs.replay
    elif use_graph:
        gs = GraphedStep(step, warmup=3)
        run = gs.replay
    else:
        run = step
    n_rep = 1
    for _ in range(args.warmup // n_rep):
        run()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps // n_rep):
        loss = run()
    torch.cuda.synchronize()          # this rank's K steps are done: its clock stops here; the closing barrier follows, and the MAX over
    el = time.perf_counter() - t0     # ranks (below) is the job's time — the barrier's own latency (an RCCL collective) is not a step
    if world > 1:
        dist.barrier()
    if world > 1:
        tmax = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        el = float(tmax.item())
    assert bool(torch.isfinite(loss))
    if rank == 0 and args.dump_outputs:   # the loss of the last timed step, and the parameters and gradients that step left behind
        grads = [q.grad.reshape(-1).float() for q in params if q.grad is not None]
        dump_outputs(args.dump_outputs, dict(loss=loss.reshape(1), params=torch.cat([q.detach().reshape(-1).float() for q in params]),
                                             grads=torch.cat(grads) if grads else None))
    N = B * T
    mac = lambda sizes: sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
    F_dense = 2 * (mac(enc.feature_extractor.sizes) + mac(dec.reconstructor.sizes)) * N
    ms = el / args.steps * 1e3
    out = {
        "metric": "trajectories/sec, whole GOKU training step (encoder -> sample -> latent_out -> solve -> reconstructor, loss, pullback, AdamW) goku_step",
        "value": B * world * args.steps / el, "unit": "trajectories/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.dtype == "f32" else "mixed: bf16 operands / f32 accumulate in the dense chains, f32 solve and recurrent stacks", "data": "synthetic",
        "config": {"workload": "goku_step: GOKU_basic default layers (input 784, T=50), Pendulum Tsit5, MSE + 1e-3·KL, AdamW; "
                               "torch-level API over lde_chain_* / lde_rnn_* / lde_forward / lde_adjoint",
                   "batch_per_gpu": B, "global_batch": Bg, "save_points": T,
                   "parallelism": f"dp{world} (batch sharded by trajectory; one flat all-reduce of all parameter gradients per step)",
                   "submission": ("two hipGraph replays per step around the eager gradient all-reduce (train.GraphedStep)" if split else
                                  "one hipGraph replay per step (train.GraphedStep)") if use_graph else "eager (≈ 50 launches per step)",
                   "weight_gradient_branch": "the reconstructor's weight-gradient kernels run as a parallel branch of the captured step (lde_set_dw_stream)" if async_dw
                   else "off: every kernel on one stream"},
        "roofline": dict(bound="mfma", kernel="whole step (dense chains dominate the flops)", achieved=3 * F_dense / (ms * 1e-3) / 1e12,
                         peak=FP32_PEAK_TFLOPS if args.dtype == "f32" else BF16_PEAK_TFLOPS, unit="TFLOP/s",
                         frac=3 * F_dense / (ms * 1e-3) / 1e12 / (FP32_PEAK_TFLOPS if args.dtype == "f32" else BF16_PEAK_TFLOPS), traffic=None,
                         note=("one hipGraph replay of ≈ 30 kernels on one stream: the figure is the device's critical path (DESIGN.md §4.7)"
                               if use_graph else "eager: ≈ 50 launches per step, host enqueue time comparable to device time (DESIGN.md §4.7)")
                         + ("; mixed: the dense chains run on the bf16 matrix cores — the fraction is against the dense bf16 peak (2.5 PF), and "
                            "the chains' large kernels are HBM-bound (hbm_view)" if args.dtype != "f32" else "")),
        "loss": float(loss.detach()), "cpu_baseline": None,
    }
    hv, tr, trk = chain_hbm_view("goku_step", args.dtype != "f32")
    if hv:
        out["roofline"]["traffic"] = tr
        out["roofline"]["traffic_kernel"] = trk
        out["roofline"]["hbm_view"] = hv
        if args.dtype != "f32":
            out["roofline"]["bound"] = "hbm (mixed: see hbm_view; the MFMA fraction is quoted beside it)"
    if world > 1 or (dist.is_available() and dist.is_initialized()):
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(out)


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def attach_traffic(roof, workload, B, mlp, full_batch, dom=None, rounds=("r6", "r5", "r4", "r3", "r2", "r1"), launched=None):
    """roofline.traffic (+ rocprof_avg_launch_ms, whole_step.traffic) of the solve workloads from the newest committed PMC summary
    (profiles/collect.sh + profiles/summarize.py; FETCH_SIZE ×2 only for kernels that load 16 bytes per lane, WRITE_SIZE as is —
    MI355X_MICROARCH.md §HBM). Also called by profiles/refresh.py on the bench line it copies next to a fresh summary, so the
    committed line and its summary cannot disagree."""
    # `launched` = {"lde_forward": name, "lde_adjoint": name}: the kernels THIS run launched (lde_last_kernel). A summary that does not hold
    # the launched kernel is stale — a kernel change since it was collected — and is not attached (traffic stays null and the line says why).
    roof["traffic"] = None
    stale = []
    for rnd in rounds:
        prof = os.path.join(ROOT, "profiles", f"{rnd}_{workload}_b{B}_summary.json" if not mlp else f"{rnd}_{workload}_summary.json")
        if not os.path.exists(prof):
            continue
        kern = json.load(open(prof))["kernels"]

        def tb(kd):
            return kd.get("fetch_bytes", kd["fetch_bytes_x2_gfx950"]) + kd["write_bytes"]
        if not mlp:
            call = dom or ("lde_forward" if "lde_forward" in roof.get("kernel", "lde_forward") else "lde_adjoint")
            kn = (launched or {}).get(call) or {"lde_forward": "k_pend_forward", "lde_adjoint": "k_pend_adjoint"}[call]
            for name, kd in kern.items():
                if name.startswith(kn) and "write_bytes" in kd:
                    roof["traffic"] = tb(kd)
                    roof["traffic_kernel"] = name
                    roof["rocprof_avg_launch_ms"] = kd["avg_ns"] * 1e-6
            if roof["traffic"] is None:
                stale.append(f"{os.path.relpath(prof, ROOT)} holds no {kn}")
        elif full_batch:   # MLP workloads: the dominant kernel's own traffic; the whole step's beside it
            def is_adj_solve(name):   # the adjoint's solve kernels: k_mlp64_adj / k_mlp64_disc<…>, k_mlpb / k_mlpc / k_mlpw / k_mlpv<…, true…>, k_mlp_adjoint[_disc], k_mlp4_adjoint
                return name.startswith(("k_mlp64_adj", "k_mlp64_disc", "k_mlp_adjoint", "k_mlp4_adjoint")) or (name.startswith(("k_mlpb", "k_mlpc", "k_mlpw", "k_mlpv")) and "true" in name)
            want = (launched or {}).get("lde_adjoint") or "k_mlp"
            adj = [(kd.get("avg_ns", 0), tb(kd), name) for name, kd in kern.items() if is_adj_solve(name) and name.startswith(want) and "write_bytes" in kd]
            if not adj:
                stale.append(f"{os.path.relpath(prof, ROOT)} holds no {want} adjoint solve kernel")
            tr = [tb(kd) for name, kd in kern.items() if name.startswith(("k_mlp", "k_reduce", "k_sum")) and "write_bytes" in kd]
            if adj:
                roof["traffic"] = float(max(adj)[1])                 # the longest-running solve kernel of the step = the adjoint's
                roof["traffic_kernel"] = max(adj)[2]
                roof["rocprof_avg_launch_ms"] = max(adj)[0] * 1e-6
            if tr and "whole_step" in roof:
                roof["whole_step"]["traffic"] = float(sum(tr))
        if roof["traffic"] is not None:
            roof["traffic_source"] = os.path.relpath(prof, ROOT)
            break
    if roof["traffic"] is None and stale:
        roof["traffic_source"] = "none attached (stale summaries: " + "; ".join(stale[:3]) + ")"
    return roof



def chain_hbm_view(workload, mixed, rounds=("r4", "r3", "r2")):
    """The dense chains' large kernels against the HBM roof: counter bytes (FETCH_SIZE + WRITE_SIZE of the committed PMC passes,
    corrected as MI355X_MICROARCH.md §HBM prescribes) ÷ rocprofv3's average launch duration, per kernel, for the three kernels that
    carry the step's bytes. Returns (view, traffic of the slowest of them, its name) or (None, None, None) without a committed summary."""
    name = f"{workload}_mixed" if mixed else workload
    for rnd in rounds:
        prof = os.path.join(ROOT, "profiles", f"{rnd}_{name}_summary.json")
        if not os.path.exists(prof):
            continue
        kern = json.load(open(prof))["kernels"]
        rows = []
        for kn, kd in kern.items():
            if kn.startswith(("k_chain_forward", "k_chain_backward", "k_chain_dw")) and "_group" not in kn and "write_bytes" in kd:
                by = kd.get("fetch_bytes", kd["fetch_bytes_x2_gfx950"]) + kd["write_bytes"]
                gbs = by / (kd["avg_ns"] * 1e-9) / 1e9
                rows.append(dict(kernel=kn, avg_launch_us=kd["avg_ns"] * 1e-3, traffic=by, achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s",
                                 frac=gbs / HBM_PEAK_GBS))
        if rows:
            rows.sort(key=lambda r: -r["avg_launch_us"])
            return dict(bound="hbm", source=os.path.relpath(prof, ROOT), kernels=rows[:3]), rows[0]["traffic"], rows[0]["kernel"]
    return None, None, None


def emit(out):
    """Rank 0's ONE JSON line — and the LAST line of stdout: RCCL writes a version banner through C stdio, which sits in libc's buffer
    (stdout is a pipe under the driver) until the process exits, i.e. it would land BEHIND a line printed from Python. Flush libc first,
    print, flush Python."""
    try:
        C.CDLL(None).fflush(None)
    except Exception:   # noqa: BLE001
        pass
    sys.stdout.write(json.dumps(out) + "\n")
    sys.stdout.flush()


def count_gpus_sysfs():
    """GPUs of this node WITHOUT touching HIP/HSA (the launcher parent must stay GPU-free: it starts the ranks as children):
    KFD topology nodes with a non-zero simd_count, cut down by a *_VISIBLE_DEVICES list when one is set. None if sysfs has no KFD."""
    import glob
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    n = 0
    for f in nodes:
        try:
            with open(f) as fh:
                props = dict(ln.split()[:2] for ln in fh if len(ln.split()) >= 2)
            n += int(props.get("simd_count", "0")) > 0
        except (OSError, ValueError):
            return None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None and v.strip() != "":
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def launch_ranks(args, argv):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start the N ranks as CHILD processes
    (`python -m torch.distributed.run --nproc-per-node N bench.py …`, one rank per GPU) BEFORE this process touches a GPU
    — a process that has initialised HIP must never be replaced by another program —, relay rank 0's single JSON line and
    exit with the children's code."""
    import subprocess
    if not args.dry_launch and os.environ.get("LDE_BENCH_SHARE_GPU") != "1":
        have = count_gpus_sysfs()                 # from the KFD topology in sysfs: this process never opens the GPU driver
        if have is not None and have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible on this node")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC (RCCL needs it)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or len(lines) != 1:
        sys.stderr.write(r.stdout)
        raise SystemExit(r.returncode or 1)
    print(lines[0])
    raise SystemExit(0)


def dry_launch(args):
    """The launch path without GPUs (CPU test of the N-rank plumbing): gloo ranks, one all-reduce of ones, one JSON line."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    ranks = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        one = torch.ones(1)
        dist.all_reduce(one)
        ranks = int(one.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "trajectories/sec (fwd+adjoint) GOKU pendulum, batch=256, 1/2/4/8 GPU", "value": 0.0,
                          "unit": "trajectories/s", "n_gpus": world, "steps": 0, "warmup": 0, "ms_per_step": None,
                          "dry_launch": True, "collective_ranks": ranks, "config": {"workload": args.workload}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="goku_pendulum", choices=sorted(WORKLOADS) + ["goku_decoder", "goku_step"])
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the workload's)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: the workload's batch on EVERY GPU (default); strong: the workload's batch split over the GPUs")
    ap.add_argument("--dtype", default="f32", choices=["f32", "mixed"],
                    help="goku_step / goku_decoder: 'mixed' = bf16 dense chains (f32 accumulate, f32 master weights), f32 solve")
    ap.add_argument("--sensealg", default="default", choices=["default", "discrete", "continuous"],
                    help="default: the reference's own default for the workload — discrete (LDE_SENSE_DISCRETE: the exact derivative of the discrete "
                         "solve, the GOKU path's ForwardDiffSensitivity) for goku_pendulum / c3 / goku_decoder / goku_step, continuous (the reverse-time "
                         "adjoint: a NeuralODE's InterpolatingAdjoint) for c2 / c4 / latentode_ref; or force one of the two")
    ap.add_argument("--async-dw", type=int, default=-1, choices=[-1, 0, 1, 2, 3],
                    help="goku_step: the large chains' weight-gradient kernels on a stream of their own — a parallel branch of the captured step (-1: the workload's default)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-sensealg", action="store_true", help="skip the second measurement with the other definition of the gradient (profiling runs: one set of kernels per trace)")
    ap.add_argument("--sweep", action="store_true", help="also report a large-batch sweep (extra keys, rank 0)")
    ap.add_argument("--dry-launch", action="store_true", help="exercise the N-rank launch path without GPUs (gloo)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: per-kernel and per-call times, roofline, CPU baseline, the other definition of "
                         "the gradient, the strong-scaling rider (N > 1); without it a run times the K steps and prints the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()
    if args.sweep:   # (the large-batch sweep is one of the --full extras)
        args.full = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args, sys.argv[1:])
    if args.dry_launch:
        return dry_launch(args)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    # LDE_BENCH_SHARE_GPU=1 — a TEST switch (tests/test_gpu_bench_contract.py), never a measurement: the N ranks share the box's GPUs
    # (rank r on device r mod device_count) and meet over gloo, because RCCL refuses two ranks on one device. It runs every line of the
    # N > 1 path except RCCL itself on the one-GPU boxes the round's tests get; the line says so (`config.shared_gpu_test`).
    args.share_gpu = world > 1 and os.environ.get("LDE_BENCH_SHARE_GPU") == "1"
    if args.share_gpu:
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    args.rccl_ranks = 1
    if world > 1 or os.environ.get("LDE_BENCH_FORCE_PG") == "1":   # (the switch: a one-rank RCCL group on a one-GPU box — the capture below beside torch's collective watchdog)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if world == 1:
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if args.share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)                    # RCCL is up and spans every rank
        args.rccl_ranks = int(one.item())
        assert args.rccl_ranks == world
        C.CDLL(None).fflush(None)   # RCCL's version banner (C stdio, every rank) leaves NOW — not at exit, behind rank 0's JSON line

    if args.workload == "goku_decoder":
        return run_decoder(args, torch, dist, world, rank, local)
    if args.workload == "goku_step":
        return run_goku_step(args, torch, dist, world, rank, local)

    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd.dist import shard_bounds
    lib = L.load()
    w = WORKLOADS[args.workload]
    T, D, P = w["T"], w["D"], w["P"]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)

    # the one collective of the path (shared RHS-MLP gradient): through the C ABI (lde_comm_*) when RCCL binds, else torch's
    comm, comm_kind = None, "none"
    if world > 1 and args.workload != "goku_pendulum" and not args.share_gpu:   # (the metric's right-hand side has no weights: no collective, no communicator)
        try:
            from latentdiffeq_amd.dist import LdeComm
            comm, comm_kind = LdeComm(rank, world), "lde_comm_allreduce_f32 (C ABI over RCCL)"
        except Exception as e:                                                   # noqa: BLE001
            comm_kind = f"torch.distributed all_reduce (lde_comm unavailable: {e})"
        C.CDLL(None).fflush(None)
    elif world > 1 and args.share_gpu:
        comm_kind = "torch.distributed all_reduce over gloo (LDE_BENCH_SHARE_GPU test)"

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def kernel_ms(fn, n):
        """average duration of n launches: bracketed = an event pair around every launch; stream = one pair around n back-to-back"""
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in evs:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize()
        br = [a.elapsed_time(b) for a, b in evs]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(n):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        return float(np.mean(br)), float(np.median(br)), a.elapsed_time(b) / n

    def measure(B, seed_shift, detail, sensealg=None, keep=False):
        """W warm-up steps, then exactly K timed steps of lde_forward + lde_adjoint on B resident trajectories (detail: the --full
        probes after them; keep: a copy of the last timed step's outputs for --dump-outputs)."""
        d, ts, z0, theta, W, dz = build_problem(w, B, seed_shift=seed_shift, sensealg=sensealg or sense)
        h = C.c_void_p()
        L.check(lib.lde_create(C.byref(d), C.byref(h)), None, "lde_create")
        nW = int(lib.lde_num_weights(C.byref(d)))
        if nW:
            L.check(lib.lde_set_weights(h, W.ctypes.data_as(C.c_void_p), nW), h, "lde_set_weights")
        L.check(lib.lde_reserve(h, B, T), h, "lde_reserve")
        z0d = torch.from_numpy(z0).to(dev)
        thd = torch.from_numpy(theta).to(dev) if theta is not None else None
        dzd = torch.from_numpy(dz).to(dev)
        zout = torch.empty((T, B, D), device=dev)
        ret = torch.empty((B,), device=dev, dtype=torch.int32)
        dz0 = torch.empty((B, D), device=dev)
        dth = torch.empty((B, P), device=dev) if P else None
        dW = torch.zeros((nW,), device=dev) if nW else None
        tsp = ts.ctypes.data_as(C.POINTER(C.c_double))

        # the device pointers as ctypes objects, made once (a `ccall` host pays nothing per argument; ctypes re-wraps every int it is handed)
        pz0, pth, pzo, pret, pdz, pdz0, pdth, pdW = p(z0d), p(thd), p(zout), p(ret), p(dzd), p(dz0), p(dth), p(dW)

        def fwd(s=sp):
            L.check(lib.lde_forward(h, pz0, pth, tsp, T, B, pzo, pret, s), h, "lde_forward")

        def bwd(s=sp):
            if dW is not None:
                dW.zero_()
            L.check(lib.lde_adjoint(h, pzo, pth, tsp, T, B, pdz, pdz0, pdth, pdW, s), h, "lde_adjoint")
            if dW is not None and world > 1:  # the one collective of the path: shared RHS-MLP gradient
                if comm is not None:
                    comm.allreduce_(dW)
                else:
                    dist.all_reduce(dW)

        def step():
            fwd()
            bwd()

        # the same step as a training loop pays it (MLP right-hand sides): the weights are handed over before every forward solve
        # (lde_set_weights_device + the re-layout launches behind it: the optimiser has just changed them) and the pullback WRITES dW
        # (option "adjoint_overwrite": no zero fill by the caller)
        Wd = torch.from_numpy(W).to(dev) if nW else None

        def step_train():
            L.check(lib.lde_set_weights_device(h, p(Wd), nW, sp), h, "lde_set_weights_device")
            fwd()
            L.check(lib.lde_adjoint(h, p(zout), p(thd), tsp, T, B, p(dzd), p(dz0), p(dth), p(dW), sp), h, "lde_adjoint")
            if world > 1:
                if comm is not None:
                    comm.allreduce_(dW)
                else:
                    dist.all_reduce(dW)

        # The analytic-RHS step is two ≈ 5–11 µs kernels: a launch-bound inner loop, so the K timed steps are submitted as hipGraph
        # replays (chunks of ≤ 256 captured steps; every step still runs both kernels on the same buffers — abl/metric_graph.py:
        # 14.3 µs per step against 14.9–15.5 µs for 2·K stream launches, and the rate no longer depends on how fast this host thread
        # enqueues beside seven other ranks). LDE_BENCH_GRAPH=0 or a failed capture: plain stream launches.
        graphs = None
        if not nW and os.environ.get("LDE_BENCH_GRAPH", "1") != "0":
            try:
                gs = torch.cuda.Stream()
                gsp = C.c_void_p(gs.cuda_stream)
                gs.wait_stream(torch.cuda.current_stream())
                chunk = max(1, min(args.steps, 256))
                plan = [(chunk, args.steps // chunk)] + ([(args.steps % chunk, 1)] if args.steps % chunk else [])
                with torch.cuda.stream(gs):
                    fwd(gsp)
                    bwd(gsp)
                    torch.cuda.synchronize()
                    graphs = []
                    for n, reps in plan:
                        g = torch.cuda.CUDAGraph()
                        # thread_local: torch's collective watchdog (N > 1) may query its events from another thread while this one captures
                        with torch.cuda.graph(g, stream=gs, capture_error_mode="thread_local"):
                            for _ in range(n):
                                fwd(gsp)
                                bwd(gsp)
                        graphs.append((g, reps))
                    torch.cuda.synchronize()
                    for g, _ in graphs:      # first replay of a graph uploads it: part of the warm-up
                        g.replay()
                    torch.cuda.synchronize()
            except Exception as e:   # noqa: BLE001 — the measurement falls back to stream launches and says so
                sys.stderr.write(f"bench: hipGraph capture failed ({e}); timing stream launches\n")
                graphs = None
        for _ in range(args.warmup):
            step()
        fence()
        t0 = time.perf_counter()
        if graphs:
            for g, reps in graphs:
                for _ in range(reps):
                    g.replay()
        else:
            for _ in range(args.steps):
                step()
        torch.cuda.synchronize()          # this rank's K steps are done: its clock stops here; the closing barrier follows, and the MAX over
        el = time.perf_counter() - t0     # ranks (below) is the job's time — the barrier's own latency (an RCCL collective) is not a step
        if world > 1:
            dist.barrier()
        if world > 1:
            tmax = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el = float(tmax.item())
        res = dict(el=el, B=B, nW=nW, problem=(d, ts, z0, theta, W, dz), graphed=bool(graphs))
        if keep:   # the last timed step's results, before the probes below launch the same calls on these buffers again
            res["outputs"] = {k: v.clone() for k, v in dict(z_hat=zout, retcode=ret, dz0=dz0, dtheta=dth, dW=dW).items() if v is not None}
        if detail:
            nprobe = min(max(args.steps, 20), 200)
            fwd()
            res["fwd"] = kernel_ms(fwd, nprobe)
            res["bwd"] = kernel_ms(bwd, nprobe)
            res["step"] = kernel_ms(step, nprobe)
            # SURVEY.md §8(d)'s definition of the time: wall clock of lde_forward + lde_adjoint, device-synchronised per call, median of
            # ≥ 100 iterations after ≥ 10 warm-ups (the host's enqueue and the synchronisation's wake-up are inside every sample)
            nsync = max(100, min(args.steps, 1000))
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            samp = []
            for _ in range(nsync):
                t1 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                samp.append(time.perf_counter() - t1)
            res["sync_call"] = (float(np.median(samp)) * 1e3, float(np.mean(samp)) * 1e3, nsync)
            if nW:
                L.check(lib.lde_set_option(h, b"adjoint_overwrite", 1.0), h, "lde_set_option")
                step_train()
                res["step_train"] = kernel_ms(step_train, nprobe)
                L.check(lib.lde_set_option(h, b"adjoint_overwrite", 0.0), h, "lde_set_option")
                fam = C.c_double(-1.0)
                lib.lde_get_option(h, b"adjoint_family", C.byref(fam))
                res["adjoint_family"] = int(fam.value)
            if nW:   # the adjoint's two phases, from HIP events the library records on this stream (lde_set_phase_timing)
                lib.lde_set_phase_timing(h, 1)
                ph = []
                ms2 = (C.c_float * 2)()
                for _ in range(min(nprobe, 30)):
                    bwd()
                    if lib.lde_get_phase_ms(h, ms2) == 0:
                        ph.append((ms2[0], ms2[1]))
                lib.lde_set_phase_timing(h, 0)
                if ph:
                    res["phase_ms"] = (float(np.mean([a_ for a_, _ in ph])), float(np.mean([b_ for _, b_ in ph])))
            st = L.Stats()
            lib.lde_get_stats(h, 0, C.byref(st), sp)
            res["fstat"] = dict(nfe=st.nfe, naccept=st.naccept, nreject=st.nreject, nfailed=st.nfailed, max_steps=st.max_steps)
            lib.lde_get_stats(h, 1, C.byref(st), sp)
            res["bstat"] = dict(nfe=st.nfe, naccept=st.naccept, nreject=st.nreject, nfailed=st.nfailed, max_steps=st.max_steps)
        res["handle"] = h
        return res

    def full_figures(m, out):
        """--full: per-launch HIP-event times of lde_forward / lde_adjoint, the dominant kernel's roofline (+ counter bytes from the committed
        profiles), the per-step event figures, the solver statistics and the device-synchronised per-call time."""
        B, h = m["B"], m["handle"]
        disc = sense == "discrete"
        (fwd_ms, fwd_med, fwd_stream), (bwd_ms, bwd_med, bwd_stream) = m["fwd"], m["bwd"]
        fstat, bstat = m["fstat"], m["bstat"]

        fb, bb = alg_bytes_per_traj(w)
        dom, dom_ms, dom_stream, dom_bytes = ("lde_adjoint", bwd_ms, bwd_stream, bb) if bwd_ms >= fwd_ms else ("lde_forward", fwd_ms, fwd_stream, fb)
        Ff = flops_per_eval(w)
        # flops of the pullback per evaluation it reports: the continuous adjoint's evaluations are fused (forward + z-VJP + weight gradient:
        # 3·F_f); the discrete sweep reports 2S per accepted step — S forward-only (F_f) and S fused (3·F_f): 2·F_f on average
        adj_f = 2 if disc else 3
        if Ff and w["batching"] == "coupled":
            flops = (fstat["nfe"] * Ff + bstat["nfe"] * adj_f * Ff) * B
        else:
            flops = fstat["nfe"] * Ff + bstat["nfe"] * adj_f * Ff
        if Ff:  # MLP right-hand side: compute-bound on the f32 MFMA/VALU rate
            # the DOMINANT kernel = the adjoint's solve kernel: its flops are the recomputed forward pass and the z-VJP of every evaluation
            # (2·F_f each; the weight-gradient product, the third F_f, is counted where it runs — inside that kernel or in the tail)
            cols = B if w["batching"] == "coupled" else 1
            ph = m.get("phase_ms")
            # k_mlp64 / k_mlpb / k_mlpc fold gW inside the solve kernel (what follows it is the fixed-order row sum: a few µs); the tile
            # kernels and k_mlpw / k_mlpv stage (a_l, δ_l) for k_mlp_dw, whose product then is the tail's
            # which family ran: reported by the library (option "adjoint_family": 1 k_mlp64, 2 k_mlpb, 3 k_mlpc fold in the kernel), not guessed
            in_kernel_dw = m.get("adjoint_family", -1) in (1, 2, 3)
            dom_flops = bstat["nfe"] * ((2 if in_kernel_dw else 1.5) if disc else (3 if in_kernel_dw else 2)) * Ff * cols
            dom_ms_k = ph[0] if ph else bwd_stream
            ach = dom_flops / (dom_ms_k * 1e-3) / 1e12
            whole = flops / ((fwd_stream + bwd_stream) * 1e-3) / 1e12
            roof = dict(bound="mfma", kernel="lde_adjoint: solve kernel (HIP events of lde_set_phase_timing)", achieved=ach, peak=FP32_PEAK_TFLOPS,
                        unit="TFLOP/s", frac=ach / FP32_PEAK_TFLOPS, traffic=None, alg_flops_per_launch=dom_flops, avg_launch_ms=dom_ms_k,
                        tail=dict(what="weight-gradient product + fixed-order sums after the solve kernel", avg_launch_ms=ph[1] if ph else None,
                                  alg_flops=0 if in_kernel_dw else bstat["nfe"] * Ff * cols),
                        whole_step=dict(kernel="lde_forward+lde_adjoint", achieved=whole, frac=whole / FP32_PEAK_TFLOPS, alg_flops_per_step=flops,
                                        avg_launch_ms=fwd_stream + bwd_stream, avg_launch_ms_bracketed=fwd_ms + bwd_ms))
        else:
            # average launch duration of the dominant call over n back-to-back launches (HIP events on the launch stream); the
            # bracketed figure (an event pair around every single launch) carries the events' own ≈ 2.5 µs
            ach = dom_bytes * B / (dom_stream * 1e-3) / 1e9
            roof = dict(bound="hbm", kernel=dom, achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS,
                        traffic=None, alg_bytes_per_launch=dom_bytes * B, avg_launch_ms=dom_stream, avg_launch_ms_bracketed=dom_ms)

        # HBM traffic of the dominant kernel from the committed rocprofv3 PMC passes of this same command
        lib.lde_last_kernel.restype = C.c_char_p
        launched = {"lde_forward": (lib.lde_last_kernel(h, 0) or b"").decode(), "lde_adjoint": (lib.lde_last_kernel(h, 1) or b"").decode()}
        attach_traffic(roof, args.workload + ("_discrete" if disc else ""), B, mlp=bool(Ff), full_batch=(B == w["B"]), dom=None if Ff else dom, launched=launched)
        roof["launched_kernels"] = launched

        out.update({
            "roofline": roof,
            "kernel_ms": {"lde_forward": fwd_stream, "lde_adjoint": bwd_stream, "lde_forward_bracketed": fwd_ms, "lde_adjoint_bracketed": bwd_ms},
            # per-step figures from HIP events (an event pair around every step): the wall-clock mean above is K steps / elapsed
            "ms_per_step_events": {"median": m["step"][1], "mean": m["step"][0], "back_to_back": m["step"][2], "samples": min(max(args.steps, 20), 200)},
            "solver_stats": {"forward": fstat, "adjoint": bstat},
            # device-synchronised per call, median of ≥ 100 (host enqueue + wake-up included) — beside the pipelined figure above
            "per_call_synchronised": {"median_ms": m["sync_call"][0], "mean_ms": m["sync_call"][1], "samples": m["sync_call"][2],
                                      "value": B * world / (m["sync_call"][0] * 1e-3), "unit": "trajectories/s"},
        })

    sense = resolve_sensealg(args.workload, args.sensealg)
    Bw = args.batch or w["B"]
    if args.scaling == "strong":
        lo, hi = shard_bounds(Bw, rank, world)
        B = hi - lo
        global_batch = Bw
    else:
        B = Bw
        global_batch = Bw * world
    m = measure(B, rank, args.full, keep=bool(args.dump_outputs))
    el, nW, h = m["el"], m["nW"], m["handle"]
    d, ts, z0, theta, W, dz = m["problem"]
    ms_per_step = el / args.steps * 1e3
    value = global_batch * args.steps / el
    disc = sense == "discrete"
    out = {
        "metric": "trajectories/sec (fwd+adjoint) GOKU pendulum, batch=256, 1/2/4/8 GPU"
        if args.workload == "goku_pendulum" else f"trajectories/sec (fwd+adjoint) {args.workload}",
        "value": value, "unit": "trajectories/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.workload}: {w['desc']}", "batch_per_gpu": B, "global_batch": global_batch,
                   "save_points": T, "rccl_ranks": args.rccl_ranks, **({"shared_gpu_test": "ranks share a GPU and meet over gloo: plumbing test, not a measurement"} if args.share_gpu else {}),
                   "parallelism": f"dp{world} (batch sharded by trajectory, no data-path collective)"
                   if not nW else f"dp{world} (batch sharded; one all-reduce of dW per step: {comm_kind})",
                   "submission": "hipGraph replays of ≤ 256 captured steps (each step = lde_forward + lde_adjoint)" if m.get("graphed")
                   else "stream launches (two per step)"},
        "roofline": None,
        "sensealg": ("LDE_SENSE_DISCRETE (the exact derivative of the discrete solve on its accepted steps: the reference's ForwardDiffSensitivity)" if disc
                     else "continuous adjoint (reverse-time solve; time-parallel on the analytic GOKU path)")
        + (" — the reference's default for this workload" if sense == REF_SENSEALG[args.workload] else " — forced by --sensealg"),
    }
    if args.full:
        full_figures(m, out)

    # the same K steps with the other definition of the gradient, beside the headline (every rank takes part: the timing's barriers are collective)
    if args.full and not args.no_other_sensealg:
        other = "continuous" if disc else "discrete"
        mo = measure(B, rank, False, sensealg=other)
        out["other_sensealg"] = {"sensealg": other, "value": global_batch * args.steps / mo["el"], "unit": "trajectories/s",
                                 "ms_per_step": mo["el"] / args.steps * 1e3}
        lib.lde_destroy(mo["handle"])

    if "step_train" in m:
        # the MLP lines' step as a training loop pays it: lde_set_weights_device (+ its re-layout launches) before every forward solve, dW
        # written by the pullback (no zero fill) — beside the headline, whose weights are uploaded once
        st_ = m["step_train"]
        out["training_step"] = {"what": "lde_set_weights_device + lde_forward + lde_adjoint (option adjoint_overwrite: dW written, no fill launch)",
                                "ms_per_step": st_[2], "ms_per_step_bracketed": st_[0], "value": global_batch / (st_[2] * 1e-3),
                                "adjoint_family": m.get("adjoint_family")}
    if args.full and world > 1 and args.scaling == "weak" and args.workload == "goku_pendulum":
        # the same ranks on the GLOBAL batch of the metric (256 split over the GPUs): the strong-scaling figure beside the weak one
        lo, hi = shard_bounds(Bw, rank, world)
        try:   # (an extra: whatever happens here must not cost the line above)
            ms2 = measure(hi - lo, 100 + rank, False)
            out["strong_scaling"] = {"global_batch": Bw, "batch_per_gpu": hi - lo, "value": Bw * args.steps / ms2["el"],
                                     "ms_per_step": ms2["el"] / args.steps * 1e3}
            lib.lde_destroy(ms2["handle"])
        except Exception as e:   # noqa: BLE001
            out["strong_scaling"] = {"error": str(e)[:200]}

    if rank == 0 and args.sweep and not nW:
        sweep = {}
        fb, bb = alg_bytes_per_traj(w)
        for Bs in (1 << 12, 1 << 16, 1 << 20):
            d2, ts2, z02, th2, _, dz2 = build_problem(w, Bs)
            a = torch.from_numpy(z02).to(dev); b_ = torch.from_numpy(th2).to(dev); c = torch.from_numpy(dz2).to(dev)
            zo = torch.empty((T, Bs, D), device=dev); r = torch.empty((Bs,), device=dev, dtype=torch.int32)
            g0 = torch.empty((Bs, D), device=dev); gt = torch.empty((Bs, P), device=dev)
            lib.lde_reserve(h, Bs, T)
            tsp2 = ts2.ctypes.data_as(C.POINTER(C.c_double))

            def f2():
                L.check(lib.lde_forward(h, p(a), p(b_), tsp2, T, Bs, p(zo), p(r), sp), h, "fwd")

            def b2():
                L.check(lib.lde_adjoint(h, p(zo), p(b_), tsp2, T, Bs, p(c), p(g0), p(gt), C.c_void_p(), sp), h, "bwd")
            f2(); b2(); torch.cuda.synchronize()
            fm, bm = kernel_ms(f2, 10)[2], kernel_ms(b2, 10)[2]
            sweep[str(Bs)] = dict(traj_per_s=Bs / ((fm + bm) * 1e-3), fwd_ms=fm, bwd_ms=bm,
                                  fwd_GBs=fb * Bs / (fm * 1e-3) / 1e9, bwd_GBs=bb * Bs / (bm * 1e-3) / 1e9)
        out["batch_sweep"] = sweep

    lib.lde_destroy(h)
    if comm is not None:
        comm.close()
    if world > 1 or (dist.is_available() and dist.is_initialized()):
        dist.barrier()
        dist.destroy_process_group()
    # the CPU baseline is taken AFTER the timed region and after the process group is gone (the other ranks have exited or are
    # exiting: nothing competes for the host cores); on N > 1 too, with a shorter budget, so that every line carries it
    if rank == 0 and args.full and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(w, d, ts, z0, theta, W, dz, budget_s=12.0 if world == 1 else 6.0)
        except Exception as e:   # noqa: BLE001 — the GPU figure is measured; a broken CPU leg is reported, not fatal
            out["cpu_baseline"] = {"value": None, "unit": "trajectories/s", "cores": 0, "kind": "port", "sample": f"failed: {str(e)[:160]}"}
    elif rank == 0:
        out["cpu_baseline"] = None
    if rank == 0:
        cb = out.get("cpu_baseline")
        if cb and cb.get("value"):
            out["vs_cpu_baseline"] = {"ratio": out["value"] / cb["value"] / max(world, 1),
                                      "what": "one GPU's trajectories/s over the CPU baseline's (same gradient definition on both sides)"}
            for k_ in ("reverse_sweep", "continuous_adjoint"):
                if cb.get(k_):
                    out["vs_cpu_baseline"]["ratio_vs_" + k_] = out["value"] / cb[k_]["value"] / max(world, 1)
        if "outputs" in m:
            dump_outputs(args.dump_outputs, m["outputs"])
        emit(out)


if __name__ == "__main__":
    main()
