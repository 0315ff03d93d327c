"""GPU: the AdaBelief step — lde_adabelief_flux_step / _dev / _guarded / _clipped (include/lde.h: "the AdaBelief step"),
`FluxAdaBelief`, `GraphedStep(guard=FluxAdaBelief(...))` and `train(optimiser="adabelief")`.

The reference is the f64 mode of tests/belief_ref.py on the f32 values the C ABI receives. The tolerance is measured, not chosen: the FLOOR
is the distance of the restatement's f32 mode (same operations, one rounding each, no fused multiply-add) from its f64 mode on the test's
own inputs, per quantity and per step, and the bound is 4 floors (belief_ref.BOUND_FACTOR): the kernel fuses a·b + c·d in three places and
so rounds at other places than numpy, each such difference a rounding of the floor's size. x is measured in units of 2⁻²⁴·(|x| + η), m and s
relative to the largest entry of the step. Floors on the two input sets (tests/belief_ref.py: inputs; measured by tests/test_belief_host.py),
steps 1 …:
    "paths"      x 2.95 4.02 3.14 3.75   m 4.57e-08 7.10e-08 8.53e-08 8.72e-08   s 1.03e-07 1.36e-07 1.55e-07 1.21e-07
    "49 arrays"  x 2.34 3.02 3.61        m 4.56e-08 6.96e-08 8.91e-08            s 1.18e-07 9.59e-08 1.03e-07
so the bounds are x ≤ 9.4 … 16.1 units, m ≤ 1.8e-7 … 3.6e-7, s ≤ 3.8e-7 … 6.2e-7. What one MI355X gave is recorded in DESIGN.md §4.6.
"paths": sizes [1, 0, 5, 2047, 2048, 2049, 8193, 3·2048 + 7] around the update's slice of 2048 elements per workgroup, and one array whose
p/g/m/v views start one float past a 16-byte boundary; "49 arrays": one more non-empty array than a launch's table holds, empty ones in
between — two launches, the count bumped once. A fresh Gaussian gradient at every step. Bit-for-bit comparisons wherever two forms must agree."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import belief_ref as R
from tests.test_gpu_guard import BAD, CLEAN_WORDS, new_words, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = R.HP
ADAMW_HP = (HP[0], HP[1], HP[2], 1e-8, HP[5])
MODES = sorted(R.C.MODES)
_FLOORS = {}


def floors(name):
    """(per-step floors, per-step f64 reference states) of a case: computed once, shared, not modified."""
    if name not in _FLOORS:
        sizes, _, ps, grads = R.inputs(name)
        _FLOORS[name] = R.floors(ps, grads, R.zeros(ps), R.zeros(ps), HP)
    return _FLOORS[name]


def within(err, floor, what):
    print(f"[belief] {what}: x {err[0]:.2f} (floor {floor[0]:.2f}) m {err[1]:.2e} ({floor[1]:.2e}) s {err[2]:.2e} ({floor[2]:.2e})")
    assert all(e <= R.BOUND_FACTOR * f for e, f in zip(err, floor)), (what, err, floor)


class Box:
    """x, g, m, s of several arrays as views into buffers of their own (an `unaligned` array starts one float past a 16-byte boundary),
    the device step count, guard words, and the clipped step's workspace and norms with a margin that is checked after every step."""

    def __init__(self, name=None, sizes=None, unaligned=(), ps=None):
        import torch
        from latentdiffeq_amd import _lib as L
        if name is not None:
            sizes, unaligned, ps, _ = R.inputs(name)
        self.sizes, self.unaligned = list(sizes), set(unaligned)
        self.p, self.g, self.m, self.v = [], [], [], []
        for i, n in enumerate(self.sizes):
            off = 1 if i in self.unaligned else 0
            for dst in (self.p, self.g, self.m, self.v):
                view = torch.zeros(n + 4, device="cuda")[off:off + n]
                assert view.data_ptr() % 16 == (4 if off else 0)
                dst.append(view)
            if ps is not None:
                self.p[i].copy_(torch.from_numpy(np.array(ps[i])))
        self.step = torch.zeros((), dtype=torch.int64, device="cuda")
        self.w = new_words()
        self.nbytes = int(L.load().lde_clip_ws_bytes(len(self.sizes), self.table()))
        self.ws = torch.full((self.nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.norms = torch.full((len(self.sizes) + 3,), -7.0, device="cuda")

    def copy(self):
        b = Box(sizes=self.sizes, unaligned=self.unaligned)
        for name in "pgmv":
            for d, s in zip(getattr(b, name), getattr(self, name)):
                d.copy_(s)
        b.step.copy_(self.step)
        b.w.copy_(self.w)
        return b

    def table(self):
        from latentdiffeq_amd import _lib as L
        tab = (L.AdamTensor * len(self.sizes))()
        for i in range(len(self.sizes)):
            t = tab[i]
            t.p, t.g, t.m, t.v, t.n = self.p[i].data_ptr(), self.g[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), self.sizes[i]
        return tab

    def set_grads(self, gs):
        import torch
        for d, g in zip(self.g, gs):
            d.copy_(torch.from_numpy(np.array(g)))

    def set_bits(self, i, e, bits):
        import torch
        self.g[i].view(torch.int32)[e:e + 1].copy_(torch.from_numpy(np.array([bits], np.uint32).view(np.int32)))

    def state(self):
        return [a.clone() for name in "pmv" for a in getattr(self, name)] + [self.step.clone()]

    def host(self):
        return tuple([x.cpu().numpy() for x in arr] for arr in (self.p, self.m, self.v))

    def call(self, name, *args):
        from latentdiffeq_amd import _lib as L
        rc = getattr(L.load(), name)(len(self.sizes), self.table(), *args, L.raw_stream())
        assert rc == 0, (name, rc)

    def host_counted(self, t):
        self.call("lde_adabelief_flux_step", *HP, t)

    def dev(self):
        from latentdiffeq_amd import _lib as L
        self.call("lde_adabelief_flux_step_dev", *HP, L.ptr(self.step))

    def guarded(self):
        from latentdiffeq_amd import _lib as L
        self.call("lde_adabelief_flux_step_guarded", *HP, L.ptr(self.step), L.ptr(self.w))

    def clipped(self, c, mode, rule="lde_adabelief_flux_step_clipped", hp=HP, check=True):
        from latentdiffeq_amd import _lib as L
        self.call(rule, *hp, c, R.C.MODES[mode], L.ptr(self.step), L.ptr(self.w), L.ptr(self.ws), L.ptr(self.norms))
        if check:                                       # (not inside a capture: a look at the margins is a synchronisation)
            self.check_margins()

    def check_margins(self):
        n = len(self.sizes)
        assert (self.ws[self.nbytes:] == 0xA5).all() and self.norms[n + 1:].tolist() == [-7.0, -7.0]

    def read_norms(self):
        w = self.norms[:len(self.sizes) + 1].tolist()
        return w[:-1], w[-1]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_host_counted_form_against_the_restatement(name):
    fl, ref = floors(name)
    _, _, _, grads = R.inputs(name)
    b = Box(name)
    for k, gs in enumerate(grads):
        b.set_grads(gs)
        b.host_counted(k + 1)
        within(R.errors(b.host(), ref[k], HP[0]), fl[k], f"host-counted {name!r} step {k + 1}")
    assert int(b.step) == 0 and b.w.tolist() == CLEAN_WORDS


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_device_counted_form(name):
    """Within the bound of the reference AND of the host-counted form at equal t (the two form 1/(1 − βᵗ) with different `pow`s); the count
    advances by exactly one per call — with 49 arrays that is two launches and ONE bump."""
    fl, ref = floors(name)
    _, _, _, grads = R.inputs(name)
    b, h = Box(name), Box(name)
    for k, gs in enumerate(grads):
        b.set_grads(gs)
        h.set_grads(gs)
        b.dev()
        h.host_counted(k + 1)
        assert int(b.step) == k + 1
        within(R.errors(b.host(), ref[k], HP[0]), fl[k], f"device-counted {name!r} step {k + 1}")
        within(R.errors(b.host(), h.host(), HP[0]), fl[k], f"device-counted against host-counted {name!r} step {k + 1}")


def test_a_step_over_empty_arrays_only_ticks_the_count():
    import torch
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    w = new_words()
    step = torch.zeros((), dtype=torch.int64, device="cuda")
    norms = torch.full((4,), -7.0, device="cuda")
    tab = (L.AdamTensor * 2)()
    s = L.raw_stream()
    assert lib.lde_adabelief_flux_step_dev(2, tab, *HP, L.ptr(step), s) == 0 and int(step) == 1
    assert lib.lde_adabelief_flux_step_dev(0, None, *HP, L.ptr(step), s) == 0 and int(step) == 2
    assert lib.lde_adabelief_flux_step_guarded(2, tab, *HP, L.ptr(step), L.ptr(w), s) == 0 and int(step) == 3
    assert lib.lde_adabelief_flux_step_clipped(2, tab, *HP, 1.0, 0, L.ptr(step), L.ptr(w), None, L.ptr(norms), s) == 0 and int(step) == 4
    assert norms.tolist() == [0.0, 0.0, 0.0, -7.0] and w.tolist() == CLEAN_WORDS
    assert lib.lde_adabelief_flux_step(2, tab, *HP, 1, s) == 0 and int(step) == 4          # host-counted: nothing to do


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_clean_guarded_step_is_the_device_counted_step(name):
    _, _, _, grads = R.inputs(name)
    a, b = Box(name), Box(name)
    for k, gs in enumerate(grads[:3]):
        a.set_grads(gs)
        b.set_grads(gs)
        a.guarded()
        b.dev()
        assert same(a.state(), b.state()), k
        assert a.w.tolist() == CLEAN_WORDS and int(a.step) == k + 1


@pytest.mark.parametrize("kind", ["+nan", "+inf", "-inf"])
def test_a_non_finite_gradient_withholds_the_whole_update(kind):
    """One bad value at the first element, the last element, or in a ragged tail (of the update's slice, of the scan's, of the unaligned
    array): x, m, s and the count stay bit for bit, the words are what include/lde.h states, word [0] is −1 afterwards; the next clean step
    applies — it equals the device-counted form on a copy — and clears the streak."""
    sizes, _, _, grads = R.inputs("paths")
    a = Box("paths")
    a.set_grads(grads[0])
    a.guarded()                                         # one applied step first: the count is 1, not 0
    assert int(a.step) == 1 and a.w.tolist() == CLEAN_WORDS
    a.set_grads(grads[1])
    places = [(0, 0), (8, 2050), (5, 2048), (6, 8192), (7, 3 * 2048 + 6), (8, 0), (3, 2046)]
    assert all(e < sizes[i] for i, e in places)
    for k, (i, e) in enumerate(places, 1):
        keep = a.g[i][e].clone()
        a.set_bits(i, e, BAD[kind])
        before = a.state()
        a.guarded()
        assert same(a.state(), before), (kind, i, e)
        assert a.w.tolist() == [-1, k, k, i] and int(a.step) == 1, (kind, i, e, a.w.tolist())
        a.g[i][e] = keep
    b = a.copy()
    a.guarded()
    b.dev()
    n = len(places)
    assert same(a.state(), b.state()) and not same(a.state(), before) and a.w.tolist() == [-1, n, 0, 3] and int(a.step) == 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_scale_one_is_the_guarded_step(name, mode):
    _, _, _, grads = R.inputs(name)
    a, b = Box(name), Box(name)
    for k, gs in enumerate(grads[:3]):
        a.set_grads(gs)
        b.set_grads(gs)
        per, total = R.C.norms(gs)
        a.clipped(1.5 * total if mode == "global" else 1.5 * max(per), mode)
        b.guarded()
        assert same(a.state(), b.state()), k
        assert a.w.tolist() == CLEAN_WORDS and int(a.step) == k + 1
        assert same(a.g, b.g)                                              # the gradients are not modified in memory


@pytest.mark.parametrize("mode", MODES)
def test_active_clipping_against_the_restatement(mode):
    """c = half the first step's total norm (global) or half its median non-empty per-array norm (per array: some arrays over c, some under).
    norms_dev must be, bit for bit, what lde_adamw_flux_step_clipped writes for the same gradients (the scan is the same code, and
    tests/test_gpu_clip.py holds THAT to 2e-6 of the f64 norm — repeated here); the reference then takes its scales from those f32 norms by
    tests/clip_ref.py's f32 rule, so that what is measured against the floor is this rule's update and not the norm's last bit (a scale
    that differs by one ulp moves m by 1.2e-7 of itself: as much as the floor)."""
    sizes, _, ps, grads = R.inputs("paths")
    per0, total0 = R.C.norms(grads[0])
    c = 0.5 * (total0 if mode == "global" else float(np.median([x for x in per0 if x > 0])))
    b, twin = Box("paths"), Box("paths")
    scales = []
    for k, gs in enumerate(grads):
        b.set_grads(gs)
        twin.set_grads(gs)
        b.clipped(c, mode)
        twin.clipped(c, mode, rule="lde_adamw_flux_step_clipped", hp=ADAMW_HP)
        n = len(sizes) + 1
        assert same([b.norms[:n]], [twin.norms[:n]]) and int(b.step) == k + 1 and b.w.tolist() == CLEAN_WORDS
        got, got_total = b.read_norms()
        per, total = R.C.norms(gs)
        assert abs(got_total - total) <= 2e-6 * total and all(abs(x - y) <= 2e-6 * y for x, y in zip(got, per))
        s = R.C.scales(got, got_total, c, R.C.MODES[mode])
        over = [i for i, x in enumerate(s) if float(x) != 1.0 and sizes[i]]
        assert over and (mode == "global" or len(over) < sum(1 for x in sizes if x)), (mode, s)
        scales.append(s)
    fl, ref = R.floors(ps, grads, R.zeros(ps), R.zeros(ps), HP, scales=scales)
    # the device states were overwritten step by step: run again on a fresh box, comparing as it goes
    b = Box("paths")
    for k, gs in enumerate(grads):
        b.set_grads(gs)
        b.clipped(c, mode)
        within(R.errors(b.host(), ref[k], HP[0]), fl[k], f"clipped ({mode}) step {k + 1}")


@pytest.mark.parametrize("mode", MODES)
def test_a_non_finite_norm_withholds_the_step(mode):
    import torch
    sizes, _, _, grads = R.inputs("paths")
    b = Box("paths")
    b.set_grads(grads[0])
    per, total = R.C.norms(grads[0])
    c = 0.5 * (total if mode == "global" else min(x for x in per if x > 0))
    b.clipped(c, mode)
    assert int(b.step) == 1 and b.w.tolist() == CLEAN_WORDS
    b.set_grads(grads[1])
    b.g[6].fill_(3e19)                                  # finite values whose squares overflow f32
    assert torch.isfinite(b.g[6]).all()
    before = b.state()
    b.clipped(c, mode)
    got, got_total = b.read_norms()
    assert same(b.state(), before) and b.w.tolist() == [-1, 1, 1, 6] and int(b.step) == 1
    assert not np.isfinite(got[6]) and not np.isfinite(got_total)
    b.set_bits(2, 4, BAD["-nan-payload"])               # and a NaN in a lower array: that one is reported
    b.clipped(c, mode)
    assert same(b.state(), before) and b.w.tolist() == [-1, 2, 2, 2]
    b.set_grads(grads[1])
    twin = b.copy()
    b.clipped(c, mode)
    twin.clipped(c, mode)
    assert not same(b.state(), before) and same(b.state(), twin.state()) and b.w.tolist() == [-1, 2, 0, 2] and int(b.step) == 2


def test_not_adamw_under_another_name():
    """The first step from a zero state moves x by η/β₁ here and by η in lde_adamw_flux_step (both against the gradient's sign), and s is
    β₁² of ADAMW's v: on the same inputs the two differ by more than 100 bounds in x and in s. (m is the same rule in both.)"""
    fl, ref = floors("paths")
    _, _, _, grads = R.inputs("paths")
    a, b = Box("paths"), Box("paths")
    a.set_grads(grads[0])
    b.set_grads(grads[0])
    a.host_counted(1)
    b.call("lde_adamw_flux_step", *ADAMW_HP, 1)
    ex, em, es = R.errors(b.host(), a.host(), HP[0])
    print(f"[belief] ADAMW against AdaBelief, first step: x {ex:.0f} units, m {em:.2e}, s {es:.2e}")
    assert ex > 100 * R.BOUND_FACTOR * fl[0][0] and es > 100 * R.BOUND_FACTOR * fl[0][2], (ex, es, fl[0])
    moved = np.concatenate([x - np.asarray(p0) for x, p0 in zip(a.host()[0], R.inputs("paths")[2])])
    x0 = np.concatenate([np.asarray(p0) for p0 in R.inputs("paths")[2]])
    g0 = np.concatenate(grads[0])
    want = -np.sign(g0) * (HP[0] / HP[1]) - HP[5] * x0                      # Δ = ±η/β₁ + decay·x …
    big = np.abs(g0) > 1e-3                                                 # … where ε_var = 1e-16 is negligible beside (1 − β₂)β₁²g² ≥ 8e-10
    assert big.sum() > 0.9 * big.size and np.abs(moved - want)[big].max() <= 1e-6 * HP[0] + 2.0 ** -22 * np.abs(x0).max()


def _run(tmp_path, name, text):
    f = tmp_path / name
    f.write_text(text)
    r = subprocess.run([sys.executable, str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, LDE_ROOT=ROOT))
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok " in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


REPLAY = r'''
import os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import numpy as np, torch
from tests import belief_ref as R
from tests.test_gpu_belief import Box, same
sizes, unaligned, ps, grads = R.inputs("paths")
grads = grads[:3]
for mode in sorted(R.C.MODES):
    a, b = Box("paths"), Box("paths")
    per, total = R.C.norms(grads[0])
    c = 0.4 * (total if mode == "global" else float(np.median([x for x in per if x > 0])))
    scratch = Box(sizes=[5, 2049])                      # the kernels are loaded before the capture, on arrays of no consequence
    scratch.clipped(1.0, mode)
    torch.cuda.synchronize()
    src = [torch.zeros_like(g) for g in a.g]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # ONE stream: the copies and the step
        for g, s in zip(a.g, src):
            g.copy_(s)
        a.clipped(c, mode, check=False)
    torch.cuda.synchronize()
    assert int(a.step) == 0 and a.w.tolist() == [-1, 0, 0, -1]      # a capture runs nothing
    for gs in grads:                                    # three replays, new gradient contents at the same addresses
        for s, g in zip(src, gs):
            s.copy_(torch.from_numpy(np.array(g)))
        graph.replay()
    for gs in grads:                                    # three eager steps
        b.set_grads(gs)
        b.clipped(c, mode)
    torch.cuda.synchronize()
    a.check_margins()
    n = len(sizes) + 1
    assert same(a.state(), b.state()) and int(a.step) == 3 and a.w.tolist() == [-1, 0, 0, -1]
    assert same([a.norms[:n]], [b.norms[:n]])
print("ok replay")
'''


def test_captured_clipped_step_equals_three_eager_steps(tmp_path):
    _run(tmp_path, "belief_replay.py", REPLAY)


def test_native_path_stays_within_the_bound_of_the_non_native_path():
    import torch
    from latentdiffeq_amd.train import FluxAdaBelief
    fl, _ = floors("paths")
    _, _, ps, grads = R.inputs("paths")
    pa = [torch.nn.Parameter(torch.from_numpy(np.array(p)).cuda()) for p in ps]
    pb = [torch.nn.Parameter(torch.from_numpy(np.array(p)).cuda()) for p in ps]
    oa = FluxAdaBelief(pa, decay=HP[5])
    ob = FluxAdaBelief(pb, decay=HP[5], native=False)
    assert oa.native and not ob.native
    for k, gs in enumerate(grads):
        for x, y, g in zip(pa, pb, gs):
            x.grad = torch.from_numpy(np.array(g)).cuda()
            y.grad = x.grad.clone()
        v0 = pa[0]._version
        oa.step()
        ob.step()
        assert pa[0]._version > v0                                          # the raw-pointer update is announced to torch
        host = lambda params, opt: ([p.detach().cpu().numpy() for p in params], [opt.state[p]["exp_avg"].cpu().numpy() for p in params],
                                    [opt.state[p]["exp_avg_var"].cpu().numpy() for p in params])
        within(R.errors(host(pa, oa), host(pb, ob), HP[0]), fl[k], f"native against non-native step {k + 1}")
        assert all(oa.state[p]["step"] == k + 1 and set(oa.state[p]) == {"step", "exp_avg", "exp_avg_var"} for p in pa if p.numel())


def test_capturable_state_dict_round_trip_continues_at_t():
    import copy
    import torch
    from latentdiffeq_amd.train import FluxAdaBelief
    torch.manual_seed(3)
    p = [torch.nn.Parameter(torch.randn(300, device="cuda")), torch.nn.Parameter(torch.randn(5, device="cuda"))]
    grads = [[torch.randn_like(x) * 0.1 for x in p] for _ in range(3)]
    opt = FluxAdaBelief(p, decay=1e-3, capturable=True)
    for gs in grads[:2]:
        for x, g in zip(p, gs):
            x.grad = g.clone()
        opt.step()
    assert int(opt._step_dev) == 2
    sd = copy.deepcopy(opt.state_dict())
    assert all(st["step"] == 2 and set(st) == {"step", "exp_avg", "exp_avg_var"} for st in sd["state"].values())
    q = [torch.nn.Parameter(x.detach().clone()) for x in p]
    twin = FluxAdaBelief(q, decay=1e-3, capturable=True)
    twin.load_state_dict(sd)
    assert int(twin._step_dev) == 2 and all("step" not in st for st in twin.state.values())
    for x, y, g in zip(p, q, grads[2]):
        x.grad, y.grad = g.clone(), g.clone()
    opt.step()
    twin.step()
    assert int(twin._step_dev) == 3
    assert same([x.detach() for x in p] + [opt.state[x][k] for x in p for k in ("exp_avg", "exp_avg_var")],
                [y.detach() for y in q] + [twin.state[y][k] for y in q for k in ("exp_avg", "exp_avg_var")])
    fresh = FluxAdaBelief([torch.nn.Parameter(x.detach().clone()) for x in p], decay=1e-3, capturable=True)   # … and not at t = 1
    for y, g in zip(fresh.param_groups[0]["params"], grads[2]):
        y.grad = g.clone()
    fresh.step()
    assert not torch.equal(fresh.param_groups[0]["params"][0].detach(), p[0].detach())


GRAPHED = r'''
import ctypes as C, os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import numpy as np, torch
import latentdiffeq_amd as M
from latentdiffeq_amd import _lib as L
from latentdiffeq_amd.train import FluxAdaBelief, GraphedStep
from tests import guard_ref as G
dev = torch.device("cuda", 0)
ts = G.grid()
inputs = {k: tuple(torch.from_numpy(a).to(dev) for a in G.inputs(k)) for k in ("mild", "harsh")}
ibits = lambda t: t.detach().view(torch.int32)
# the small model of tests/test_gpu_guard.py: B = 8 pendulums, T = 8, loss = mean(ẑ²), the leaves ẑ₀ and θ, a step record of 20 steps
pend = M.Pendulum()
dec = M.Decoder(M.GOKU_basic(), (None, pend, None))
h = pend._native()
L.call("lde_set_option", h.ptr, b"record_capacity", float(G.CAP))
z0 = torch.nn.Parameter(torch.zeros(G.B, 2, device=dev))
th = torch.nn.Parameter(torch.ones(G.B, 1, device=dev))
z0_in, th_in = (t.clone() for t in inputs["mild"])
opt = FluxAdaBelief([z0, th], lr=1e-3, decay=1e-10, capturable=True, guard=True)

def fn():
    opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        z0.copy_(z0_in)
        th.copy_(th_in)
    zhat = M.diffeq_layer(dec, (z0.t(), th.t()), ts)
    loss = (zhat ** 2).mean()
    loss.backward()
    opt.step()
    return loss

moments = lambda: [opt.state[p][k].clone() for p in (z0, th) for k in ("exp_avg", "exp_avg_var")]
W = 3
gs = GraphedStep(fn, static_inputs=[z0_in, th_in], warmup=W, guard=opt, check_every=1)
for k in range(2):
    loss = gs.replay(*inputs["mild"])
    assert torch.isfinite(loss) and not torch.equal(z0.detach(), inputs["mild"][0]) and not torch.equal(th.detach(), inputs["mild"][1])
assert int(opt._step_dev) == W + 2 and opt.guard_state() == dict(skipped=0, streak=0, last_bad_array=-1) and gs.recoveries == 0
m_before = moments()
gs.replay(*inputs["harsh"])                             # the record overflows: NaN gradients, the update withheld, then ONE recovery
assert torch.equal(ibits(z0), ibits(inputs["harsh"][0])) and torch.equal(ibits(th), ibits(inputs["harsh"][1]))
assert all(torch.equal(ibits(a), ibits(b)) for a, b in zip(moments(), m_before))
st = opt.guard_state()
assert st["skipped"] == 1 and st["streak"] == 1 and st["last_bad_array"] == 0, st
assert int(opt._step_dev) == W + 2 and gs.recoveries == 1
loss = gs.replay(*inputs["harsh"])                      # the new capture's record holds the solve: the step applies
assert torch.isfinite(loss) and torch.isfinite(z0.grad).all() and torch.isfinite(th.grad).all()
assert not torch.equal(z0.detach(), inputs["harsh"][0]) and not torch.equal(th.detach(), inputs["harsh"][1])
assert int(opt._step_dev) == W + 3 and gs.recoveries == 1 and opt.guard_state() == dict(skipped=1, streak=0, last_bad_array=0)
assert all(torch.isfinite(m).all() for m in moments())
print("ok graphed")
'''


def test_graphed_step_replays_withholds_and_recovers_with_adabelief(tmp_path):
    _run(tmp_path, "belief_graphed.py", GRAPHED)


def test_train_with_adabelief_on_a_tiny_goku_model():
    """train(optimiser="adabelief") on the default GOKU model (28×28 input, B = 8, T = 10), two epochs of one minibatch."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import train as TR
    torch.manual_seed(4)
    mt, diffeq = la.GOKU_basic(), la.Pendulum()
    enc, dec = TR.default_layers(mt, 784, diffeq, device="cuda")
    with torch.no_grad():
        dec[0][1]._dense[-1].bias.fill_(1.0)
    model = TR.LatentDiffEqModel(mt, enc, dec)
    before = [p.detach().clone() for p in model.parameters()]
    data = torch.rand(784, 16, 12, device="cuda")                       # 12 frames, windows of T = 10 (time_loader)
    hist, best = TR.train(model, [data[:, :8]], data[:, 8:, :10], dt=0.05, epochs=2, seq_len=10, full_seq_len=12, rng=np.random.default_rng(0),
                          optimiser="adabelief")
    assert len(hist) == 2 and all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in hist)
    assert best is not None and len(best) == len(before) and all(torch.isfinite(p).all() for p in best)
    assert all(torch.isfinite(p).all() for p in model.parameters()) and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    with pytest.raises(ValueError, match="optimiser"):
        TR.train(model, [data[:, :8]], data[:, 8:, :10], dt=0.05, epochs=1, seq_len=10, full_seq_len=12, optimiser="lion")
