"""GPU: every solve on save grids that do not start at zero — the time-translation known answer (tests/time_shift.py; the checkers' own:
tests/test_time_shift_host.py).

Every right-hand side the library solves is autonomous: the solution on `ts + c` is the solution on `ts`. Absolute time is what the kernels
treat most differently from one another — t is carried in f64 and (float)(tj − t), (float)(tend − t), the save-time index guess of
k_pend_adjoint_disc_tp, the substep counts of the stochastic steppers and the MLP families' step-count hint are formed in different places
— and before this file one forward call of the suite left ts[0] = 0.

Part A (fixed steps, bit for bit). Grids: base = (0 … T−1)/16, T = 33 (97 too for k_pend_forward_tl's several-saves-per-lane form), shifted
by c ∈ {+1024, −1024, +2²⁰, −base[−1], −base[T//2]}; dt ∈ {1/32, 3/64}: all time arithmetic is exact, so ẑ, ret, the statistics, the J
record, the step record (n, dt, y; t = unshifted t + c exactly) and every gradient of a shifted solve are the unshifted solve's BITS. All
shifts of a case run on ONE handle in sequence and end with the base grid again (a stale save-time cache would show). B = 37 (a partial
wave) and 130 (three waves, a ragged last workgroup).
Part B (Tsit5 adaptive at 1e-6/1e-3 and 1e-6/1e-6; the analytic mappings, pullbacks and adjoints, the dual solves, the MLP families). Gate 1: the path's existing gate against the oracle / the numpy dual reference on the
SAME shifted grid. Gate 2, against the same kernel on the base grid: the controller never sees t, only the last step's h = (float)(tend − t)
and the dense-output Θ move, by an ulp — bound = 8 × the f32 reference's own largest deviation over these shifts on the same inputs, floored
at 4 f32 ulps of the array's largest magnitude (tests/time_shift.py: sharp_bound). A trajectory whose accepted-step count differs between
the two kernel runs is exempt from gate 2 (a borderline `last` decision), stays under gate 1, and at most 1 % of B may be.
Part C (0.05·j − 2.45: ends at 0, not dyadic). ret = 0, everything finite, per-trajectory accepted steps those of 0.05·j, the oracle gates on
the same grid. The end-of-solve guard is `t + dt ≥ tend − 1e-12·max(|tend|, tend − t₀)` in every kernel, the oracle and tests/dual_ref.py
(scaled by |tend| alone it vanished on this grid and the oracle took one more step of 1e-16 per trajectory: DESIGN.md §7).

Measured on the MI355X. Part A: bit for bit on every path, every shift, the closing base grid included — every gradient is run-to-run
reproducible. Part B, worst shifted-against-base deviation over every case, as a fraction of the array's largest entry, kernel / the f32
reference on the same inputs (the bound is 8 × the latter, per case):
    ẑ of the analytic forward mappings                1.7e-7 / 1.2e-6      discrete pullbacks dz0, dθ       1.0e-6, 6.7e-7 / 2.8e-6, 3.1e-6
    k_pend_adjoint (checkpointed) dz0, dθ              4.1e-7, 4.2e-7 / 7.7e-7, 8.5e-7
    k_pend_adjoint (no reset)     dz0, dθ              6.2e-7, 7.2e-7 / 6.2e-7, 7.1e-7
    k_pend_adjoint_fused          dz0, dθ              0 (bit-identical: every interval's solve starts from the interval's length) / 2.1e-7, 1.2e-7
    dual pendulums ẑ, J, dz0, dθ                       8.6e-8, 9.0e-8, 1.0e-7, 7.1e-8 / 1.5e-7, 1.2e-7, 1.4e-7, 1.1e-7
    Lotka–Volterra … Stuart–Landau ẑ, J, dz0, dθ       1.7e-7, 1.7e-7, 8.5e-8, 1.1e-7 / 1.2e-6, 8.5e-7, 4.3e-7, 1.6e-7 (numpy f32 reference, B = 37)
    MLP families 0 – 6 (tanh) ẑ                        7.8e-8 / 7.8e-8      continuous adjoint dz0, dW       5.7e-7, 1.1e-6 / 4.4e-7, 2.7e-7
                              discrete sweep dz0, dW   1.8e-7, 3.6e-7 / 2.9e-7, 1.5e-7      (the bound's floor, 4 ulp = 4.8e-7, is what most MLP cases stand on;
                                                                                              the worst, dW 1.1e-6 of the k_mlp4_adjoint leg, against 8 × 2.1e-7)
No trajectory of any kernel run changed its accepted-step count under a shift (nor did the references' forward and dual solves; the
oracle's sequential reverse-time adjoints move theirs by a few per cent at 1e-6: tests/time_shift.py). Part C: every case takes the
accepted steps of 0.05·j.
Not covered: k_pend_adjoint_stream (B > 24 576 or T − 1 > 1024 only, no option forces it); the systems' adaptive solves at B = 130 (their
reference's controller runs in Python). lde_last_kernel cannot tell the 8-row ring from k_pend_forward_tl proper (one label), nor an MLP
forward's family from its adjoint's (it reports the adjoint's): those legs rest on the options the older tests force them with.
The coupled MLP cases of Parts B and C take 7 – 13 s each on the GPU box: the CPU oracle's f32 and f64 replays inside `_check`."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import dpend_ref, dual_ref, sde_ref, sl_ref
from tests import time_shift as TS

pytestmark = pytest.mark.gpu

STAT_KEYS = ("nfe", "naccept", "nreject", "nfailed", "max_steps")
KINDS = [O.RHS_PENDULUM, O.RHS_PENDULUM_FRICTION]
FIXED = [(O.SOLVER_RK4, dt) for dt in TS.DTS] + [(O.SOLVER_TSIT5, dt) for dt in TS.DTS]

# the forward mappings of the analytic right-hand sides, forced as tests/test_gpu_pendulum.py and tests/test_gpu_discrete.py force them:
# options, the label lde_last_kernel returns, whether the mapping writes step records
_RING = dict(pend_tl_max_b=0, pend_sh_max_b=0, pend_ws=0, pend_lb_min_b=0)
MAPPINGS = {
    "lane": (dict(pend_ws=0, pend_tl_max_b=0, pend_sh_max_b=0), b"k_pend_forward<", True),
    "ws": (dict(pend_tl_max_b=0, pend_sh_max_b=0), b"k_pend_forward_ws", True),
    "tl": (dict(pend_tl_max_b=1024, pend_sh_max_b=0), b"k_pend_forward_tl", False),
    "sh": (dict(pend_sh_max_b=1000000, pend_lp=0), b"k_pend_forward_sh", True),
    "ring8": (dict(_RING, pend_lb=8), b"k_pend_forward_tl", False),        # (a recording forward always has the 16-row ring; the ring forms share tl's label)
    "ring16": (dict(_RING, pend_lb=16), b"k_pend_forward_tl", True),
    "lp": (dict(pend_sh_max_b=1000000), b"k_pend_forward_lp", True),       # frictionless Tsit5 adaptive only: Parts B and C
}
PULLBACKS = ((1 << 20, b"k_pend_adjoint_disc_tp"), (0, b"k_pend_adjoint_disc<"))


def _a256(x):
    return (x + 255) // 256 * 256


def _stats(st):
    return np.array([st[k] for k in STAT_KEYS], np.int64)


def _handle(options=(), W=None, **kw):
    from tests.gpu_util import Native, copy_desc_to_oracle, make_desc
    d = make_desc(**kw)
    nat = Native(d)
    for k, v in dict(options).items():
        nat.set_option(k, v)
    if W is not None:
        nat.set_weights(W)
    return nat, copy_desc_to_oracle(d)


class _Raw:
    """A step record owned by the test (lde_set_step_record), read back as bytes: whatever its layout, a shifted solve must leave the
    unshifted solve's bits in it. Zeroed before every forward, so nothing of an earlier solve is compared."""

    def __init__(self, nat, B, T):
        import torch
        from latentdiffeq_amd import _lib as L
        self.B, self.T = B, T
        self.nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
        assert self.nbytes >= _a256(4 * B)
        self.buf = torch.zeros((self.nbytes,), device="cuda", dtype=torch.uint8)
        L.check(nat.lib.lde_set_step_record(nat.h, C.c_void_p(self.buf.data_ptr()), self.nbytes), nat.h, "lde_set_step_record")

    def clear(self):
        self.buf.zero_()

    def raw(self, nbytes=None):
        return self.buf[:nbytes or self.nbytes].cpu().numpy()

    def n(self):
        return self.raw(4 * self.B).view(np.int32).copy()

    def forward_record(self, cap, c):
        """A forward step record of a two-state solve (include/lde.h: n [B] | t [cap][B] | dt [cap][B] | y [cap][B][2]) reduced to its live
        entries: n, t − c, dt, y."""
        B, raw = self.B, self.raw()
        n = raw[:4 * B].view(np.int32).copy()
        o = _a256(4 * B)
        t = raw[o:o + 8 * cap * B].view(np.float64).reshape(cap, B).T
        o += _a256(8 * cap * B)
        dt = raw[o:o + 8 * cap * B].view(np.float64).reshape(cap, B).T
        o += _a256(8 * cap * B)
        y = raw[o:o + 8 * cap * B].view(np.float32).reshape(cap, B, 2).transpose(1, 0, 2)
        assert o + 8 * cap * B <= raw.size and int(n.max()) <= cap
        tm, dtm = TS.masked_steps(t, dt, n, c)
        live = np.arange(cap)[None, :] < n[:, None]
        return dict(rec_n=n, rec_t=tm, rec_dt=dtm, rec_y=np.where(live[..., None], y, np.float32(0)))


def _sweep(tag, run, T=TS.T):
    """run(ts, c) → dict of arrays, on the base grid, every shifted grid and the base grid again: all bit-identical to the first."""
    base, shifts = TS.grids(T)
    ref = run(base, 0.0)
    for name, ts, c in shifts:
        TS.same(f"{tag} {name}", run(ts, c), ref)
    return ref


def _kernel(nat, which):
    return nat.lib.lde_last_kernel(nat.h, which)


# =================================================================================================================== Part A: fixed steps
def _pend_run(nat, rec, cap, label, z0, L, dz, ts, c):
    """One forward of an analytic right-hand side on the forced mapping, and — a recording handle — its step record and both discrete pullbacks."""
    if rec is not None:
        rec.clear()
    z, ret, st = nat.forward(z0, L, ts)
    assert _kernel(nat, 0) == label, _kernel(nat, 0)
    out = dict(z=z, ret=ret, stats=_stats(st))
    if rec is not None:
        out.update(rec.forward_record(cap, c))
        assert out["rec_n"].sum() == st["naccept"]
        for tp, name in PULLBACKS:
            nat.set_option("pend_disc_tp_max_b", tp)
            g0, gL, _, sb = nat.adjoint(z, L, ts, dz)
            assert _kernel(nat, 1) == name, _kernel(nat, 1)
            k = name.decode().rstrip("<")
            out[k + "_dz0"], out[k + "_dtheta"], out[k + "_stats"] = g0, gL, _stats(sb)
    return out


@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("mapping", ["lane", "ws", "tl", "sh", "ring8", "ring16"])
def test_pendulum_fixed_step_forward_mappings_and_discrete_pullbacks_keep_their_bits(mapping, B):
    """Both right-hand sides × {RK4, Tsit5 at a fixed step} × dt ∈ {1/32, 3/64}, the non-recording forward and — where the mapping writes
    step records — the recording one with its record and k_pend_adjoint_disc_tp / k_pend_adjoint_disc on it. Run-to-run reproducible on
    one grid: every path (the sweep ends with the base grid again)."""
    options, label, records = MAPPINGS[mapping]
    z0, L = O.pendulum_inputs(B, seed=3)
    for T in (TS.T, 97) if mapping == "tl" else (TS.T,):
        dz = O.cotangent(T, B, 2)
        for kind in KINDS:
            for solver, dt in FIXED:
                for recording in (False, True) if records else (False,):
                    sense = O.SENSE_DISCRETE if recording else O.SENSE_PARALLEL_CHECKPOINTED
                    nat, _ = _handle(options, rhs_kind=kind, solver=solver, adaptive=0, dt=dt, sensealg=sense)
                    rec = cap = None
                    if recording:
                        nat.set_option("record_capacity", 128)       # 64 steps at dt = 1/32
                        rec, cap = _Raw(nat, B, T), 128
                        assert nat.lib.lde_step_record_capacity(nat.h, T) == cap
                    ref = _sweep(f"{mapping} T {T} kind {kind} solver {solver} dt {dt} recording {recording}",
                                 lambda ts, c: _pend_run(nat, rec, cap, label, z0, L, dz, ts, c), T)
                    assert (ref["ret"] == 0).all() and np.isfinite(ref["z"]).all()
                    nsteps = int(np.ceil((T - 1) / 16.0 / dt))
                    assert ref["stats"][1] == nsteps * B and ref["stats"][2] == 0
                    if recording:
                        assert (ref["rec_n"] == nsteps).all() and np.isfinite(ref["k_pend_adjoint_disc_tp_dz0"]).all()
                        assert np.array_equal(ref["rec_t"][:, :nsteps], np.broadcast_to(dt * np.arange(nsteps), (B, nsteps)))


@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("sense,label", [(O.SENSE_PARALLEL_CHECKPOINTED, b"k_pend_adjoint_fused"), (O.SENSE_BACKSOLVE_CHECKPOINTED, b"k_pend_adjoint<"),
                                         (O.SENSE_BACKSOLVE, b"k_pend_adjoint<")])
def test_pendulum_fixed_step_continuous_adjoints_keep_their_bits(sense, label, B):
    """The three continuous sensealgs (k_pend_adjoint_fused; k_pend_adjoint with and without the reset at the save times) on the default
    forward. k_pend_adjoint_stream serves B > 24 576 or T − 1 > 1024 only and no option forces it: out of this file's shapes."""
    z0, L = O.pendulum_inputs(B, seed=3)
    dz = O.cotangent(TS.T, B, 2)
    for kind in KINDS:
        for solver, dt in FIXED:
            nat, _ = _handle(rhs_kind=kind, solver=solver, adaptive=0, dt=dt, sensealg=sense)

            def run(ts, c):
                z, ret, st = nat.forward(z0, L, ts)
                g0, gL, _, sb = nat.adjoint(z, L, ts, dz)
                assert _kernel(nat, 1) == label, _kernel(nat, 1)
                return dict(z=z, ret=ret, stats=_stats(st), dz0=g0, dtheta=gL, adj_stats=_stats(sb))

            ref = _sweep(f"sense {sense} kind {kind} solver {solver} dt {dt}", run)
            assert (ref["ret"] == 0).all() and np.isfinite(ref["dz0"]).all() and ref["adj_stats"][3] == 0


def _dual_handle(name, **kw):
    """(handle, inputs(B), D, labels) of a LDE_SENSE_FORWARD_DUAL system: the two pendulums, and tests/time_shift.py's table."""
    from latentdiffeq_amd import _lib as L
    if name in ("pendulum", "friction"):
        desc = dict(rhs_kind=L.RHS_PENDULUM if name == "pendulum" else L.RHS_PENDULUM_FRICTION)
        inputs, D, labels = (lambda B: O.pendulum_inputs(B, seed=3)), 2, (b"k_pend_forward_dual", b"k_pend_adjoint_dual")
    else:
        s = TS.dual_systems()[name]
        desc, inputs, D, labels = s["desc"], s["inputs"], s["sys"].D, s["kernels"]
    nat, _ = _handle(sensealg=L.SENSE_FORWARD_DUAL, **desc, **kw)
    return nat, inputs, D, labels


def _dual_run(nat, rec, head, labels, cap, z0, th, dz, ts, c):
    """forward into the test's record (n | J as bytes; the traced steps through lde_get_step_record), pullback."""
    B = z0.shape[0]
    rec.clear()
    z, ret, st = nat.forward(z0, th, ts)
    record = rec.raw(head)
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert (_kernel(nat, 0), _kernel(nat, 1)) == labels, (_kernel(nat, 0), _kernel(nat, 1))
    out = dict(z=z, ret=ret, stats=_stats(st), record=record, dz0=g0, dtheta=gth, adj_stats=_stats(sta))
    if cap:
        tr = nat.step_record(0, B, cap=cap)
        t, dt = np.zeros((B, cap)), np.zeros((B, cap))
        t[:, :tr["t"].shape[1]], dt[:, :tr["dt"].shape[1]] = tr["t"], tr["dt"]
        out["rec_t"], out["rec_dt"] = TS.masked_steps(t, dt, tr["n"], c)
        out["rec_n"] = tr["n"]
    return out


def _traced(nat, B, T, cap):
    """The test's record with the step trace switched on; `head` = the bytes of n | J (the record's size without the trace)."""
    head = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", cap)
    rec = _Raw(nat, B, T)
    assert rec.nbytes > head
    return rec, head


DUAL_NAMES = ["pendulum", "friction", "lv", "kuramoto3", "kuramoto4", "dpend", "cvs", "sl1", "sl2", "sl3"]


@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("name", DUAL_NAMES)
def test_dual_fixed_step_solves_keep_their_bits(name, B):
    """LDE_SENSE_FORWARD_DUAL, forward and pullback: k_forward_dual (the pendulums, Lotka–Volterra) and k_forward_dual_dir (Kuramoto on 8
    and 16 lanes, the double pendulum, CVS, Stuart–Landau N = 1, 2, 3) with k_pend_adjoint_dual / k_adjoint_dual_dir; RK4 and Tsit5 fixed."""
    for solver, dt in FIXED:
        nat, inputs, D, labels = _dual_handle(name, solver=solver, adaptive=0, dt=dt)
        z0, th = inputs(B)
        dz = TS.dual_cotangent(D, TS.T, B)
        rec, head = _traced(nat, B, TS.T, 128)
        ref = _sweep(f"{name} solver {solver} dt {dt}", lambda ts, c: _dual_run(nat, rec, head, labels, 128, z0, th, dz, ts, c))
        assert (ref["ret"] == 0).all() and np.isfinite(ref["dz0"]).all() and np.isfinite(ref["dtheta"]).all()
        assert (ref["rec_n"] == int(np.ceil(2.0 / dt))).all() and ref["record"][_a256(4 * B):].any()


@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("solver", [sde_ref.EM, sde_ref.EULER_HEUN])
@pytest.mark.parametrize("name", ["spendulum", "sl1", "sl3"])
def test_stochastic_solves_keep_their_path(name, solver, B):
    """k_pend_forward_sde and k_forward_sde_dir (N = 1, 3), EM and EulerHeun, dt ∈ {1/32, 3/64, 0.05}: the substep plan comes from
    ts[j] − ts[j−1] (two substeps of 1/32 per interval for each dt — an interval is divided evenly) and the noise is indexed by substep,
    not by time: the same seed gives the same path, bit for bit."""
    from latentdiffeq_amd import _lib as L
    from tests import sl_gpu
    for dt in TS.DTS + (0.05,):
        if name == "spendulum":
            nat, _ = _handle(rhs_kind=L.RHS_SPENDULUM, solver=solver, sensealg=L.SENSE_FORWARD_DUAL, adaptive=0, dt=dt)
            (z0, th), D, labels = sde_ref.inputs(B, seed=3), 2, (b"k_pend_forward_sde", b"k_pend_adjoint_dual")
        else:
            N = int(name[2:])
            nat = sl_gpu.fixed(N, solver, dt)
            (z0, th), D, labels = sl_ref.inputs(N, B, seed=3), 2 * N, (b"k_forward_sde_dir", b"k_adjoint_dual_dir")
        sl_gpu.set_noise(nat, seed=5)
        dz = TS.dual_cotangent(D, TS.T, B)
        rec, head = _traced(nat, B, TS.T, 128)
        ref = _sweep(f"{name} solver {solver} dt {dt}", lambda ts, c: _dual_run(nat, rec, head, labels, 128, z0, th, dz, ts, c))
        assert (ref["ret"] == 0).all() and np.isfinite(ref["dz0"]).all() and (ref["rec_n"] == 2 * (TS.T - 1)).all()
        assert ref["stats"][1] == 2 * (TS.T - 1) * B


# tests/time_shift.py: the smallest shapes of tests/test_gpu_mlp.py::test_kernel_families_agree that reach each family; the legs force them as
# that test does
MLP_CASES, _mlp_inputs = TS.MLP_CASES, TS.mlp_inputs
MLP_LEGS = dict(new={}, mlpw={"mlpb": 0}, tiles={"mlpv": 0, "mlp64": 0, "mlpw": 0}, mlpv={"mlp64": 0, "mlpw": 0})
MLP_LEG_CASES = [(c, l) for c, v in MLP_CASES.items() for l in v["legs"]]


@pytest.mark.parametrize("case,leg", MLP_LEG_CASES)
def test_mlp_fixed_step_solves_keep_their_bits(case, leg):
    """RK4 at dt = 1/32, coupled and per-trajectory, every kernel family (0 tiles, 1 k_mlp64, 2 k_mlpb, 3 k_mlpc, 4 k_mlpw, 5 k_mlpv,
    6 k_mlp4_adjoint), forward + adjoint for both definitions of the gradient: the continuous adjoint (whose family is asserted) and
    LDE_SENSE_DISCRETE on the forward's step record (legs "new" and "tiles": a recording forward runs on neither k_mlpw nor k_mlpv).
    (The library reports the ADJOINT's family only — lde_last_kernel answers with it for either call; the forward's family follows from the
    same `*_serves` predicates of csrc/lde_host.h at these batches, and is not observable from here.)"""
    cfg, W, z0, dz = _mlp_inputs(case, TS.T)
    B = cfg["B"]
    for sense in (None, O.SENSE_DISCRETE):
        if sense == O.SENSE_DISCRETE and leg not in ("new", "tiles"):
            continue
        skw = dict(sensealg=sense) if sense == O.SENSE_DISCRETE else {}       # (the continuous adjoint: tests/gpu_util.py's default, as that test)
        nat, _ = _handle(MLP_LEGS[leg], W, layers=cfg["layers"], solver=O.SOLVER_RK4, adaptive=0, dt=1.0 / 32.0, **skw, **cfg["kw"])

        def run(ts, c):
            z, ret, st = nat.forward(z0, None, ts)
            g0, _, gW, sb = nat.adjoint(z, None, ts, dz)
            out = dict(z=z, ret=ret, stats=_stats(st), dz0=g0, dW=gW, adj_stats=_stats(sb), family=np.array(nat.adjoint_family()))
            if sense == O.SENSE_DISCRETE:
                tr = nat.step_record(0, B, cap=128)
                t, dt = np.zeros((len(tr["n"]), 128)), np.zeros((len(tr["n"]), 128))
                t[:, :tr["t"].shape[1]], dt[:, :tr["dt"].shape[1]] = tr["t"], tr["dt"]
                out["rec_t"], out["rec_dt"] = TS.masked_steps(t, dt, tr["n"], c)
                out["rec_n"] = tr["n"]
            return out

        ref = _sweep(f"{case} {leg} sense {sense}", run)
        assert (ref["ret"] == 0).all() and np.isfinite(ref["dW"]).all() and ref["adj_stats"][3] == 0
        assert ref["stats"][1] == 64 * (1 if cfg["kw"].get("batching") == O.BATCH_COUPLED else B)
        if sense != O.SENSE_DISCRETE:
            assert int(ref["family"]) == cfg["legs"][leg], (leg, int(ref["family"]))
        else:
            assert (ref["rec_n"] == 64).all()


# ================================================================================================================ Part B: Tsit5 adaptive
def _exempt(n_shift, n_base, B):
    """Trajectories whose accepted-step count moved: exempt from the sharp gate, at most 1 % of B."""
    ex = np.asarray(n_shift) != np.asarray(n_base)
    assert ex.sum() <= B // 100, f"{int(ex.sum())} of {B} trajectories changed their accepted-step count under a time shift"
    return ex


def _sharp(tag, a, b, dev_rel, exempt=None, axis_b=None, worst=None):
    """|a − b| ≤ sharp_bound(dev_rel)·max|b| outside the exempt trajectories (axis_b: the trajectory axis of the arrays)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    if exempt is not None and exempt.any():
        d = np.delete(d, np.nonzero(exempt)[0], axis=axis_b)
    rel = float(d.max() / np.abs(b).max())
    if worst is not None:
        worst[tag.split()[-1]] = max(worst.get(tag.split()[-1], 0.0), rel)
    assert rel <= TS.sharp_bound(dev_rel), f"{tag}: {rel:.2e} of the largest entry against a bound of {TS.sharp_bound(dev_rel):.2e} (the f32 oracle's own: {dev_rel:.2e})"


def _forward_gate(z, zr, tol):
    """tests/test_gpu_pendulum.py::test_forward_matches_oracle's gates against the f32 oracle on the same grid."""
    per_traj = np.abs(z - zr).max(axis=(0, 2))
    if tol[1] > 1e-4:
        assert per_traj.max() <= 3e-4 and np.quantile(per_traj, 0.99) <= 1e-4, (per_traj.max(), np.quantile(per_traj, 0.99))
    else:
        assert per_traj.max() <= 1e-5, per_traj.max()


def _mapping_cases():
    """(mapping, right-hand side): k_pend_forward_lp serves the frictionless pendulum only."""
    return [(m, k) for m in MAPPINGS for k in KINDS if not (m == "lp" and k != O.RHS_PENDULUM)]


def _part_c_mapping_cases():
    """… and Tsit5 adaptive solves only."""
    return [(m, k, s) for m, k in _mapping_cases() for s in sorted(TS.PART_C_SOLVES) if m != "lp" or "adaptive" in s]


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("mapping,kind", _mapping_cases())
def test_pendulum_adaptive_forward_mappings_and_discrete_pullbacks_under_a_time_shift(o32, o64, mapping, kind, B, tol):
    """Every forward mapping (k_pend_forward_lp included: frictionless only) at Tsit5 adaptive. Recording mappings: `_check` of
    tests/test_gpu_discrete.py on the kernel's own record, with both pullbacks, on every shifted grid (gate 1), and ẑ and the gradients
    against the base grid's (gate 2; exemptions by the record's per-trajectory counts). Mappings that write no record (and the
    non-recording instantiation of the others): ẑ against the oracle on the same grid and against the base grid's; without per-trajectory
    counts the exemption is by the launch's accepted-step total — unchanged total, nothing exempt."""
    from tests.test_gpu_discrete import _check
    options, label, records = MAPPINGS[mapping]
    dev, _, changed = TS.oracle_shift_deviation("f32", kind, tol, B)
    assert "forward" not in changed
    z0, L = O.pendulum_inputs(B, seed=3)
    dz = O.cotangent(TS.T, B, 2)
    base, shifts = TS.grids()
    worst = {}
    # the non-recording instantiation
    nat, od = _handle(options, rhs_kind=kind, abstol=tol[0], reltol=tol[1])
    zb, retb, stb = nat.forward(z0, L, base)
    assert _kernel(nat, 0) == label and (retb == 0).all()
    for name, ts, c in shifts:
        z, ret, st = nat.forward(z0, L, ts)
        zr, retr, _ = o32.forward(od, z0, L, ts)
        assert (ret == 0).all() and (retr == 0).all() and np.array_equal(z[0], z0)
        _forward_gate(z, zr, tol)
        if st["naccept"] == stb["naccept"]:
            _sharp(f"{mapping} {name} z", z, zb, dev["z"], worst=worst)
        else:       # some trajectory took another number of steps: at most 1 % of B may then leave the sharp bound
            per = np.abs(z.astype(np.float64) - zb).max(axis=(0, 2)) / np.abs(zb).max()
            _exempt(per > TS.sharp_bound(dev["z"]), np.zeros(B, bool), B)
    if records:
        nat, od = _handle(options, rhs_kind=kind, abstol=tol[0], reltol=tol[1], sensealg=O.SENSE_DISCRETE)
        ref = {}
        for name, ts, c in [("base0", base, 0.0)] + shifts:
            for tp, pull in PULLBACKS:
                nat.set_option("pend_disc_tp_max_b", tp)
                z, rec, (g0, gL, _), st, sb = _check(nat, od, o32, o64, z0, L, ts, dz, None)
                assert _kernel(nat, 0) == label and _kernel(nat, 1) == pull
                if name == "base0":
                    ref[tp] = (z, rec["n"].copy(), g0, gL)
                    continue
                zb_, nb, g0b, gLb = ref[tp]
                ex = _exempt(rec["n"], nb, B)
                _sharp(f"{mapping} recording {name} z", z, zb_, dev["z"], ex, 1, worst)
                _sharp(f"{mapping} {pull.decode()} {name} disc_dz0", g0, g0b, dev["disc_dz0"], ex, 0, worst)
                _sharp(f"{mapping} {pull.decode()} {name} disc_dtheta", gL, gLb, dev["disc_dtheta"], ex, 0, worst)
    print(f"{mapping} kind {kind} B {B} tol {tol}: worst shifted-against-base, kernel / f32 oracle: " +
          ", ".join(f"{k} {v:.1e} / {dev[k]:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_pendulum_adaptive_tl_with_several_saves_per_lane_under_a_time_shift(o32, kind, B, tol):
    """k_pend_forward_tl's other instantiation (T − 1 > 64: a lane serves several save times and fetches the next inside the stepping
    loop) at Tsit5 adaptive, T = 97. Its existing gate is tests/test_gpu_pendulum.py::test_small_batch_forward_over_save_grid_lengths':
    worst entry within 3e-4 of the f32 oracle at the default tolerance, 1e-5 at 1e-6/1e-6 — stated for grids of 2.5 time units (at reltol
    1e-3 two correct f32 solves drift apart with the length of the solve: on 97 points 1/16 apart, 6 time units, the kernel sits 3.06e-4
    from the oracle on the UNSHIFTED grid too, measured). So Part B runs here on (0 … 96)/64 and its shifts — 1.5 time units, several save
    times inside every step — and Part C on 0.025·j − 2.4 (97 points, ends at 0, not dyadic): the accepted-step total and the same gate."""
    T, spacing = 97, 1.0 / 64.0
    gate = 3e-4 if tol[1] > 1e-4 else 1e-5
    options, label, _ = MAPPINGS["tl"]
    dev, _, changed = TS.oracle_shift_deviation("f32", kind, tol, B, T, spacing)
    assert "forward" not in changed
    z0, L = O.pendulum_inputs(B, seed=3)
    base, shifts = TS.grids(T, spacing)
    worst = {}
    nat, od = _handle(options, rhs_kind=kind, abstol=tol[0], reltol=tol[1])
    zb, retb, stb = nat.forward(z0, L, base)
    assert _kernel(nat, 0) == label and (retb == 0).all()
    for name, ts, c in shifts:
        z, ret, st = nat.forward(z0, L, ts)
        zr, retr, _ = o32.forward(od, z0, L, ts)
        assert (ret == 0).all() and (retr == 0).all() and np.array_equal(z[0], z0)
        assert np.abs(z - zr).max() <= gate, (name, np.abs(z - zr).max())
        assert st["naccept"] == stb["naccept"], "the accepted-step total moved under a time shift"
        _sharp(f"tl97 {name} z", z, zb, dev["z"], worst=worst)
    t0 = O.time_grid(T, 0.025)
    tz = t0 - t0[-1]
    assert tz[-1] == 0.0
    za, reta, sta = nat.forward(z0, L, t0)
    zc, retc, stc = nat.forward(z0, L, tz)
    assert (reta == 0).all() and (retc == 0).all() and np.isfinite(zc).all() and stc["naccept"] == sta["naccept"]
    ec = np.abs(zc - o32.forward(od, z0, L, tz)[0]).max()
    assert ec <= gate, ec
    print(f"tl T 97 kind {kind} B {B} tol {tol}: worst shifted-against-base, kernel / f32 oracle: z {worst['z']:.1e} / {dev['z']:.1e}")


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sense", [O.SENSE_PARALLEL_CHECKPOINTED, O.SENSE_BACKSOLVE_CHECKPOINTED, O.SENSE_BACKSOLVE])
def test_pendulum_adaptive_continuous_adjoints_under_a_time_shift(o32, sense, kind, B, tol):
    """Gate 1: tests/test_gpu_pendulum.py::test_adjoint_matches_oracle's (5e-4 of the largest entry at the default tolerance, 1e-4 at the
    tight one) against the f32 oracle's adjoint on the same grid and the same ẑ. Gate 2 against the base grid's gradients. (The forward is
    the default mapping's; its per-trajectory counts are not read — an unchanged accepted-step total exempts nothing.)"""
    dev, _, _ = TS.oracle_shift_deviation("f32", kind, tol, B)
    z0, L = O.pendulum_inputs(B, seed=3)
    dz = O.cotangent(TS.T, B, 2)
    base, shifts = TS.grids()
    nat, od = _handle(rhs_kind=kind, abstol=tol[0], reltol=tol[1], sensealg=sense)
    lim = 5e-4 if tol[1] > 1e-4 else 1e-4
    worst, ref = {}, None
    for name, ts, c in [("base0", base, 0.0)] + shifts:
        z, ret, st = nat.forward(z0, L, ts)
        g0, gL, _, sb = nat.adjoint(z, L, ts, dz)
        r0, rL, _, _ = o32.adjoint(od, z, L, ts, dz)
        assert (ret == 0).all() and sb["nfailed"] == 0
        assert np.abs(g0 - r0).max() <= lim * np.abs(r0).max() and np.abs(gL - rL).max() <= lim * np.abs(rL).max()
        if ref is None:
            ref = (g0, gL, st["naccept"])
            continue
        if st["naccept"] == ref[2]:
            _sharp(f"sense {sense} {name} adj{sense}_dz0", g0, ref[0], dev[f"adj{sense}_dz0"], worst=worst)
            _sharp(f"sense {sense} {name} adj{sense}_dtheta", gL, ref[1], dev[f"adj{sense}_dtheta"], worst=worst)
        else:
            per = np.maximum(np.abs(g0 - ref[0]).max(axis=1) / np.abs(ref[0]).max(), np.abs(gL - ref[1]).max(axis=1) / np.abs(ref[1]).max())
            _exempt(per > TS.sharp_bound(max(dev[f"adj{sense}_dz0"], dev[f"adj{sense}_dtheta"])), np.zeros(B, bool), B)
    print(f"sense {sense} kind {kind} B {B} tol {tol}: worst shifted-against-base, kernel / f32 oracle: " +
          ", ".join(f"{k} {v:.1e} / {dev[k]:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("B", TS.BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_pendulum_adaptive_dual_solve_under_a_time_shift(o32, o64, kind, B, tol):
    """k_forward_dual / k_pend_adjoint_dual on the pendulums. Gate 1: tests/test_gpu_forward_dual.py's — the kernel's steps replayed in the
    f32 and f64 oracles (_replay_gates) and, free-running at the default tolerance, the dual-norm oracle's ẑ. Gate 2 on ẑ, J and the gradients."""
    from tests.test_gpu_forward_dual import _Record, _native, _replay_gates
    dev, _, changed = TS.oracle_shift_deviation("f32", kind, tol, B)
    assert "dual" not in changed
    z0, L = O.pendulum_inputs(B, seed=3)
    dz = O.cotangent(TS.T, B, 2)
    base, shifts = TS.grids()
    nat, od = _native(rhs_kind=kind, abstol=tol[0], reltol=tol[1])
    nat.set_option("step_trace", 1)
    nat.set_option("record_capacity", 512)
    rec = _Record(nat, B, TS.T)
    worst, ref = {}, None
    for name, ts, c in [("base0", base, 0.0)] + shifts:
        z, ret, st = nat.forward(z0, L, ts)
        J = rec.J()
        g0, gL, _, _ = nat.adjoint(z, L, ts, dz)
        tr = nat.step_record(0, B, cap=512)
        assert (ret == 0).all() and np.array_equal(z[0], z0) and np.array_equal(tr["n"], rec.n())
        _replay_gates(od, o32, o64, z0, L, ts, dz, z, J, g0, gL, tr)
        if tol[1] > 1e-4:      # (free-running, test_it_is_the_dual_norm_controller gates the default tolerance only)
            zd, _, _, retd, _, _ = o32.forward_dual(od, z0, L, ts, dual_norm=True)
            _forward_gate(z, zd, tol)
        if ref is None:
            ref = (z, J, g0, gL, tr["n"].copy())
            continue
        ex = _exempt(tr["n"], ref[4], B)
        _sharp(f"dual {name} dual_z", z, ref[0], dev["dual_z"], ex, 1, worst)
        _sharp(f"dual {name} dual_J", J, ref[1], dev["dual_J"], ex, 1, worst)
        _sharp(f"dual {name} dual_dz0", g0, ref[2], dev["dual_dz0"], ex, 0, worst)
        _sharp(f"dual {name} dual_dtheta", gL, ref[3], dev["dual_dtheta"], ex, 0, worst)
    print(f"dual kind {kind} B {B} tol {tol}: worst shifted-against-base, kernel / f32 oracle: " +
          ", ".join(f"{k} {v:.1e} / {dev[k]:.1e}" for k, v in worst.items()))


_DUAL_REF_DEV = {}


def _ref_idx(name, B):
    """The trajectories the numpy reference runs: all, but every ninth of the double pendulum's (its solve takes 70 steps a trajectory at
    1e-6 and the reference's controller runs in Python; trajectories are independent). Gate 1 — the replay — and the yardstick look at
    these; gate 2, kernel against kernel, at every trajectory."""
    return np.arange(0, B, 9) if name == "dpend" else np.arange(B)


def _dual_ref_deviation(name, tol, B):
    """The f32 numpy reference's own deviation under the shifts on the inputs of the kernel's case: {z, J, dz0, dtheta: fraction of the base
    array's largest entry}, and whether its per-trajectory accepted steps stayed. Computed once per case."""
    key = (name, tol, B)
    if key not in _DUAL_REF_DEV:
        s = TS.dual_systems()[name]
        idx = _ref_idx(name, B)
        z0, th = s["inputs"](B)
        dz = TS.dual_cotangent(s["sys"].D, TS.T, B)[:, idx]
        z0, th = z0[idx], th[idx]
        base, shifts = TS.grids()
        outs = []
        for ts in [base] + [g for _, g, _ in shifts[:-1]]:
            z, J, ret, info = dual_ref.solve(s["sys"], z0, th, ts, dtype=np.float32, abstol=tol[0], reltol=tol[1])
            assert (ret == 0).all()
            g0, gth = dual_ref.pullback(s["sys"], J, dz)
            outs.append((z, J, g0, gth, [len(x) for x in info["dt"]]))
        dev = {k: max(float(np.abs(o[i].astype(np.float64) - outs[0][i]).max() / np.abs(outs[0][i]).max()) for o in outs[1:])
               for i, k in enumerate(("z", "J", "dz0", "dtheta"))}
        _DUAL_REF_DEV[key] = (dev, all(o[4] == outs[0][4] for o in outs[1:]))
    return _DUAL_REF_DEV[key]


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("name", DUAL_NAMES[2:])
def test_dual_adaptive_solves_under_a_time_shift(name, tol):
    """k_forward_dual on Lotka–Volterra and k_forward_dual_dir on every system, B = 37 (the batch of the systems' own adaptive tests: the
    reference's controller runs a trajectory at a time in numpy, and the yardstick needs it on the same inputs under every shift).
    Gate 1: the kernel's steps replayed in the f64 reference — ẑ, J, dz0, dθ within the bounds of the systems' own adaptive tests
    ((2e-5, 1e-4, 1e-4, 1e-4) of the largest entry; the double pendulum's ADAPTIVE_BOUNDS). Gate 2 on ẑ, J, dz0, dθ of every trajectory with
    the f32 numpy reference's deviation on the same inputs."""
    B = 37
    s = TS.dual_systems()[name]
    sys_ = s["sys"]
    dev, ref_steps_unchanged = _dual_ref_deviation(name, tol, B)
    nat, inputs, D, labels = _dual_handle(name, abstol=tol[0], reltol=tol[1])
    z0, th = inputs(B)
    dz = TS.dual_cotangent(D, TS.T, B)
    idx = _ref_idx(name, B)
    rec, head = _traced(nat, B, TS.T, 512)
    bz, bJ, b0, bth = dpend_ref.ADAPTIVE_BOUNDS if name == "dpend" else TS.DUAL_STANDING_BOUNDS
    rel = TS.rel
    base, shifts = TS.grids()
    worst, ref = {}, None
    for gname, ts, c in [("base0", base, 0.0)] + shifts:
        a = _dual_run(nat, rec, head, labels, 512, z0, th, dz, ts, 0.0)
        z, g0, gth, n = a["z"], a["dz0"], a["dtheta"], a["rec_n"]
        J = TS.record_J(a["record"], B, TS.T, sys_.D, sys_.NP, s["G"])
        assert (a["ret"] == 0).all() and np.array_equal(z[0], z0) and np.array_equal(n, rec.n())
        steps = ([a["rec_t"][b, :n[b]] for b in idx], [a["rec_dt"][b, :n[b]] for b in idx])
        zr, Jr, retr, _ = dual_ref.solve(sys_, z0[idx], th[idx], ts, steps=steps)
        # (the pullback is per trajectory: the kernel's rows of these trajectories against the reference's on their cotangents)
        r0, rth = dual_ref.pullback(sys_, Jr, dz[:, idx])
        errs = (rel(z[:, idx], zr), rel(J[:, idx], Jr), rel(g0[idx], r0), rel(gth[idx], rth))
        assert (retr == 0).all() and all(e <= bd for e, bd in zip(errs, (bz, bJ, b0, bth))), (gname, errs)
        if ref is None:
            ref = (z, J, g0, gth, n.copy())
            continue
        ex = _exempt(n, ref[4], B)
        _sharp(f"{name} {gname} z", z, ref[0], dev["z"], ex, 1, worst)
        _sharp(f"{name} {gname} J", J, ref[1], dev["J"], ex, 1, worst)
        _sharp(f"{name} {gname} dz0", g0, ref[2], dev["dz0"], ex, 0, worst)
        _sharp(f"{name} {gname} dtheta", gth, ref[3], dev["dtheta"], ex, 0, worst)
    print(f"{name} tol {tol}: worst shifted-against-base, kernel / f32 numpy reference (its steps unchanged: {ref_steps_unchanged}): " +
          ", ".join(f"{k} {v:.1e} / {dev[k]:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("tol", TS.TOLS)
@pytest.mark.parametrize("case,leg", MLP_LEG_CASES)
def test_mlp_adaptive_solves_under_a_time_shift(o32, o64, case, leg, tol):
    """The MLP right-hand sides at Tsit5 adaptive, coupled and per-trajectory, every family leg, both definitions of the gradient; the
    shapes of Part A with tanh units and eight trajectories where the batch is coupled (tests/time_shift.py: mlp_adaptive_case).
    Gate 1 on every shifted grid. LDE_SENSE_DISCRETE (legs "new", "tiles"): `_check` of tests/test_gpu_discrete.py on the kernel's own
    record. The continuous adjoint: tests/test_gpu_mlp.py's gates against the f32 oracle on the same grid — ẑ within 1e-4·max(1, |ẑ|) and
    gradients within 2e-3 of the largest entry at 1e-6/1e-6 (test_one_mlp_handle_changing_shapes), 3e-4·max(1, |ẑ|) and 5e-3 at the default
    tolerance (_check_forward, test_tsit5_mlp_adjoint).
    Gate 2 against the base grid's ẑ, dz0 and dW, bound from the f32 oracle's deviation on the same inputs; exemptions by the record's
    counts (discrete) or, without per-trajectory counts, none while the launch's accepted-step total is unchanged."""
    from tests.test_gpu_discrete import _check
    kw, W, z0, dz, B = TS.mlp_adaptive_case(case, tol)
    dev, ref_unchanged = TS.oracle_mlp_shift_deviation(case, tol)
    assert ref_unchanged
    base, shifts = TS.grids()
    tight = tol[1] < 1e-4
    zlim, glim = (1e-4, 2e-3) if tight else (3e-4, 5e-3)
    worst = {}
    nat, od = _handle(MLP_LEGS[leg], W, **kw)
    ref = None
    for name, ts, c in [("base0", base, 0.0)] + shifts:
        z, ret, st = nat.forward(z0, None, ts)
        g0, _, gW, sb = nat.adjoint(z, None, ts, dz)
        assert (ret == 0).all() and sb["nfailed"] == 0 and nat.adjoint_family() == MLP_CASES[case]["legs"][leg]
        zr, _, _ = o32.forward(od, z0, None, ts, W=W)
        r0, _, rW, _ = o32.adjoint(od, z, None, ts, dz, W=W)
        assert np.abs(z - zr).max() <= zlim * max(1.0, np.abs(zr).max()), (name, np.abs(z - zr).max())
        assert TS.rel(g0, r0) <= glim and TS.rel(gW, rW) <= glim, (name, TS.rel(g0, r0), TS.rel(gW, rW))
        if ref is None:
            ref = (z, g0, gW, st["naccept"])
            continue
        assert st["naccept"] == ref[3], "the forward's accepted-step total moved under a time shift"
        _sharp(f"{case} {leg} {name} z", z, ref[0], dev["z"], worst=worst)
        _sharp(f"{case} {leg} {name} adj_dz0", g0, ref[1], dev["adj_dz0"], worst=worst)
        _sharp(f"{case} {leg} {name} adj_dW", gW, ref[2], dev["adj_dW"], worst=worst)
    if leg in ("new", "tiles"):
        nat, od = _handle(MLP_LEGS[leg], W, **dict(kw, sensealg=O.SENSE_DISCRETE))
        ref = None
        for name, ts, c in [("base0", base, 0.0)] + shifts:
            z, rec, (g0, _, gW), st, sb = _check(nat, od, o32, o64, z0, None, ts, dz, W)
            if ref is None:
                ref = (z, g0, gW, rec["n"].copy())
                continue
            ex = _exempt(rec["n"], ref[3], B)
            if len(ex) != B:          # a coupled solve is one step sequence: a changed count exempts nothing (_exempt has refused it)
                ex = None
            _sharp(f"{case} {leg} recording {name} z", z, ref[0], dev["z"], ex, 1, worst)
            _sharp(f"{case} {leg} {name} disc_dz0", g0, ref[1], dev["disc_dz0"], ex, 0, worst)
            _sharp(f"{case} {leg} {name} disc_dW", gW, ref[2], dev["disc_dW"], worst=worst)
    print(f"mlp {case} {leg} tol {tol}: worst shifted-against-base, kernel / f32 oracle: " + ", ".join(f"{k} {v:.1e} / {dev[k]:.1e}" for k, v in worst.items()))


# ======================================================================================================= Part C: 0.05·j − 2.45, ends at 0
@pytest.mark.parametrize("mapping,kind,solve", _part_c_mapping_cases())
def test_pendulum_mappings_on_a_grid_that_ends_at_zero(o32, o64, mapping, kind, solve):
    """Every forward mapping and both discrete pullbacks: ret = 0, finite, the accepted steps of 0.05·j per trajectory (the record's
    counts; the launch's total where the mapping writes none), and the oracle gates on the same grid — `_check` on the kernel's own
    record, and for ẑ of the non-recording instantiation test_forward_matches_oracle's (fixed steps: 1e-5, as test_rk4_fixed_step)."""
    from tests.test_gpu_discrete import _check
    kw = TS.PART_C_SOLVES[solve]
    adaptive = "adaptive" in solve
    # B = 64 and the default seed: the smallest case of test_forward_matches_oracle, whose gate — a statistic of the batch: worst trajectory
    # ≤ 3e-4, 99 % of them ≤ 1e-4 — is the adaptive solves' gate here, at that test's own batch, moved to this grid
    B = 64
    options, label, records = MAPPINGS[mapping]
    t0, tz = TS.part_c_grids()
    z0, L = O.pendulum_inputs(B)
    dz = O.cotangent(50, B, 2)
    nat, od = _handle(options, rhs_kind=kind, **kw)
    za, reta, sta = nat.forward(z0, L, t0)
    zb, retb, stb = nat.forward(z0, L, tz)
    assert _kernel(nat, 0) == label
    assert (reta == 0).all() and (retb == 0).all() and np.isfinite(zb).all()
    assert stb["naccept"] == sta["naccept"] and stb["max_steps"] == sta["max_steps"], (stb, sta)
    zr, _, info = o32.forward(od, z0, L, tz)
    if adaptive:
        _forward_gate(zb, zr, (1e-6, 1e-3))
    else:
        assert np.abs(zb - zr).max() <= 1e-5 and stb["naccept"] == info["naccept"]
    if records:
        nat, od = _handle(options, rhs_kind=kind, sensealg=O.SENSE_DISCRETE, **kw)
        for tp, pull in PULLBACKS:
            nat.set_option("pend_disc_tp_max_b", tp)
            _, ra, ga, _, _ = _check(nat, od, o32, o64, z0, L, t0, dz, None)
            _, rb, gb, _, sb = _check(nat, od, o32, o64, z0, L, tz, dz, None)
            assert _kernel(nat, 0) == label and _kernel(nat, 1) == pull
            assert np.array_equal(rb["n"], ra["n"]), np.nonzero(rb["n"] != ra["n"])[0]
            live = np.arange(rb["dt"].shape[1])[None, :] < rb["n"][:, None]
            assert rb["dt"][live].min() > 1e-9, "a step of round-off size"
            assert np.isfinite(gb[0]).all() and np.isfinite(gb[1]).all()


@pytest.mark.parametrize("solve", sorted(TS.PART_C_SOLVES))
@pytest.mark.parametrize("name", DUAL_NAMES)
def test_dual_solves_on_a_grid_that_ends_at_zero(o32, o64, name, solve):
    """The dual solves of Part A: the record's per-trajectory counts are those of 0.05·j, and the kernel's steps on the shifted grid
    replayed in the reference meet the path's bounds on ẑ, J, dz0 and dθ: tests/test_gpu_forward_dual.py's _replay_gates (f32 and f64
    oracle) for the pendulums, the f64 numpy reference with tests/time_shift.py's pinned bounds for the systems."""
    kw = TS.PART_C_SOLVES[solve]
    B = TS.PART_C_DUAL_B
    nat, inputs, D, labels = _dual_handle(name, **kw)
    z0, th = inputs(B)
    dz = TS.dual_cotangent(D, 50, B)
    t0, tz = TS.part_c_grids()
    rec, head = _traced(nat, B, 50, 512)
    a = _dual_run(nat, rec, head, labels, 512, z0, th, dz, t0, 0.0)
    b = _dual_run(nat, rec, head, labels, 512, z0, th, dz, tz, 0.0)
    assert (b["ret"] == 0).all() and np.isfinite(b["z"]).all() and np.isfinite(b["dz0"]).all() and np.isfinite(b["dtheta"]).all()
    assert np.array_equal(b["rec_n"], a["rec_n"]), np.nonzero(b["rec_n"] != a["rec_n"])[0]
    assert np.array_equal(b["stats"], a["stats"])
    assert b["rec_dt"][b["rec_dt"] > 0].min() > 1e-9, "a step of round-off size"
    n = b["rec_n"]
    tr = dict(t=b["rec_t"], dt=b["rec_dt"], n=n)
    rel = TS.rel
    if name in ("pendulum", "friction"):
        from tests.gpu_util import copy_desc_to_oracle
        from tests.test_gpu_forward_dual import _replay_gates
        J = TS.record_J(b["record"], B, 50, 2, 3, 0)
        _replay_gates(copy_desc_to_oracle(nat.d), o32, o64, z0, th, tz, dz, b["z"], J, b["dz0"], b["dtheta"], tr)
    else:
        s = TS.dual_systems()[name]
        J = TS.record_J(b["record"], B, 50, s["sys"].D, s["sys"].NP, s["G"])
        if kw.get("adaptive", 1):      # the kernel's accepted steps, replayed a trajectory at a time
            steps = ([tr["t"][i, :n[i]] for i in range(B)], [tr["dt"][i, :n[i]] for i in range(B)])
            zr, Jr, retr, info = dual_ref.solve(s["sys"], z0, th, tz, kw["solver"], steps=steps)
        else:                          # fixed steps: the reference's own — the kernel's record must hold exactly these times, bit for bit
            zr, Jr, retr, info = dual_ref.solve(s["sys"], z0, th, tz, kw["solver"], adaptive=False, dt=kw["dt"])
            k = len(info["t"][0])
            assert (n == k).all() and np.array_equal(tr["t"][:, :k], np.stack(info["t"])) and np.array_equal(tr["dt"][:, :k], np.stack(info["dt"]))
        r0, rth = dual_ref.pullback(s["sys"], Jr, dz)
        bounds = TS.part_c_dual_bounds(name)       # constants; the f32 reference's floor under them is asserted on the CPU
        errs = (rel(b["z"], zr), rel(J, Jr), rel(b["dz0"], r0), rel(b["dtheta"], rth))
        print(f"{name} {solve}: kernel against the f64 reference z {errs[0]:.1e} J {errs[1]:.1e} dz0 {errs[2]:.1e} dtheta {errs[3]:.1e} (bounds {bounds})")
        assert (retr == 0).all() and all(e <= bd for e, bd in zip(errs, bounds)), (errs, bounds)


@pytest.mark.parametrize("solve", sorted(TS.PART_C_SOLVES))
@pytest.mark.parametrize("case", ["per_traj_3_20_64_3", "coupled_8_200_200_8"])
def test_mlp_solves_on_a_grid_that_ends_at_zero(o32, o64, case, solve):
    """One per-trajectory and one coupled MLP right-hand side under LDE_SENSE_DISCRETE: the step record's counts are those of 0.05·j — the
    fixed-step families size their workspace from lde_host::fixed_step_count(ts), which a step of 1e-16 at the end would overrun by one —
    and `_check` of tests/test_gpu_discrete.py on the kernel's own record on the shifted grid."""
    from tests.test_gpu_discrete import _check
    kw = TS.PART_C_SOLVES[solve]
    cfg, W, z0, dz = _mlp_inputs(case, 50)
    nb = min(cfg["B"], 8) if cfg["kw"].get("batching") == O.BATCH_COUPLED else cfg["B"]     # (the oracle's 200-wide coupled replay, f32 and f64, is the cost)
    z0, dz = z0[:nb], dz[:, :nb]
    t0, tz = TS.part_c_grids()
    nat, od = _handle((), W, layers=cfg["layers"], sensealg=O.SENSE_DISCRETE, **cfg["kw"], **kw)
    za, reta, sta = nat.forward(z0, None, t0)
    ra = nat.step_record(0, nb)
    assert (reta == 0).all()
    zb, rb, gb, stb, _ = _check(nat, od, o32, o64, z0, None, tz, dz, W)
    assert np.array_equal(rb["n"], ra["n"]), (rb["n"], ra["n"])
    assert stb["naccept"] == sta["naccept"] and stb["nfe"] == sta["nfe"]
    live = np.arange(rb["dt"].shape[1])[None, :] < rb["n"][:, None]
    assert rb["dt"][live].min() > 1e-9, "a step of round-off size"
    assert np.isfinite(zb).all() and np.isfinite(gb[0]).all() and np.isfinite(gb[2]).all()
