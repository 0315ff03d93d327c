"""GPU: the guarded parameter update — lde_guard_init / lde_adamw_flux_step_guarded (include/lde.h: "the guarded step"),
`FluxADAMW(capturable=True, guard=True)` and `GraphedStep(guard=…)`. The reference everywhere is lde_adamw_flux_step_dev on a copy of the
same arrays, and every comparison is bit for bit: a clean guarded step IS the unguarded one, a withheld one moves nothing.
S = 8 192 is the scan's slice per workgroup (csrc/lde_host.h: GUARD_PER_WG), 2 048 the update's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8192
HP = (1e-3, 0.9, 0.999, 1e-8, 1e-3)          # η, β₁, β₂, ε, decay
BAD = {"+nan": 0x7FC00000, "-nan-payload": 0xFFC12345, "+inf": 0x7F800000, "-inf": 0xFF800000}
CLEAN_WORDS = [-1, 0, 0, -1]


class Arrays:
    """p, g, m, v of several arrays as views into buffers of their own; an `unaligned` array starts one float past a 16-byte boundary."""

    def __init__(self, sizes, unaligned=(), seed=0):
        import torch
        rng = np.random.default_rng(seed)
        self.sizes, self.unaligned = list(sizes), set(unaligned)
        self.p, self.g, self.m, self.v = [], [], [], []
        for i, n in enumerate(sizes):
            off = 1 if i in self.unaligned else 0
            for dst, a in ((self.p, rng.standard_normal(n)), (self.g, rng.standard_normal(n) * 0.1), (self.m, rng.standard_normal(n) * 0.01),
                           (self.v, rng.random(n) * 1e-3)):
                buf = torch.zeros(n + 4, device="cuda")
                view = buf[off:off + n]
                view.copy_(torch.from_numpy(a.astype(np.float32)))
                assert view.data_ptr() % 16 == (4 if off else 0)
                dst.append(view)
        self.step = torch.zeros((), dtype=torch.int64, device="cuda")

    def copy(self):
        import torch
        c = Arrays.__new__(Arrays)
        c.sizes, c.unaligned = self.sizes, self.unaligned
        for name in "pgmv":
            out = []
            for i, a in enumerate(getattr(self, name)):
                off = 1 if i in self.unaligned else 0
                buf = torch.zeros(a.numel() + 4, device="cuda")
                view = buf[off:off + a.numel()]
                view.copy_(a)
                out.append(view)
            setattr(c, name, out)
        c.step = self.step.clone()
        return c

    def table(self):
        from latentdiffeq_amd import _lib as L
        tab = (L.AdamTensor * len(self.sizes))()
        for i in range(len(self.sizes)):
            t = tab[i]
            t.p, t.g, t.m, t.v, t.n = self.p[i].data_ptr(), self.g[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), self.sizes[i]
        return tab

    def state(self):
        return [a.clone() for name in "pmv" for a in getattr(self, name)] + [self.step.clone()]

    def new_gradients(self, seed):
        import torch
        rng = np.random.default_rng(seed)
        for g in self.g:
            g.copy_(torch.from_numpy((rng.standard_normal(g.numel()) * 0.1).astype(np.float32)))

    def set_bits(self, i, e, bits):
        import torch
        self.g[i].view(torch.int32)[e:e + 1].copy_(torch.from_numpy(np.array([bits], np.uint32).view(np.int32)))

    def step_unguarded(self):
        from latentdiffeq_amd import _lib as L
        L.call("lde_adamw_flux_step_dev", None, len(self.sizes), self.table(), *HP, L.ptr(self.step), L.raw_stream())

    def step_guarded(self, words):
        from latentdiffeq_amd import _lib as L
        L.call("lde_adamw_flux_step_guarded", None, len(self.sizes), self.table(), *HP, L.ptr(self.step), L.ptr(words), L.raw_stream())


def new_words():
    import torch
    from latentdiffeq_amd import _lib as L
    w = torch.full((L.GUARD_WORDS,), 77, dtype=torch.int64, device="cuda")
    L.call("lde_guard_init", None, L.ptr(w), L.raw_stream())
    assert w.tolist() == CLEAN_WORDS
    return w


def same(a, b):
    """bit for bit (NaNs included: compared as integers)"""
    import torch
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b)) and len(a) == len(b)


def test_clean_guarded_step_is_the_unguarded_step():
    sizes = [1, 3, 2047, 2048, 2049, S - 1, S, S + 1, 2 * S + 3, 4099]
    a = Arrays(sizes, unaligned=(9, 2), seed=1)
    b = a.copy()
    w = new_words()
    for k in range(3):
        a.new_gradients(10 + k)
        b.new_gradients(10 + k)
        a.step_guarded(w)
        b.step_unguarded()
        assert same(a.state(), b.state()), k
        assert w.tolist() == CLEAN_WORDS and int(a.step) == k + 1


@pytest.mark.parametrize("kind", sorted(BAD))
def test_a_non_finite_gradient_withholds_the_whole_update(kind):
    sizes = [3, 2049, 2 * S + 3, 4099, 7]
    a = Arrays(sizes, unaligned=(3,), seed=2)
    w = new_words()
    a.step_guarded(w)                                  # one applied step first: the count is 1, not 0
    assert int(a.step) == 1 and w.tolist() == CLEAN_WORDS
    places = [(0, 0), (4, 6), (2, S - 1), (2, S), (2, 2 * S + 1), (3, 4098), (3, 0), (1, 2048)]
    #          first   last    last of a slice / first of the next / the ragged tail / the unaligned array / the update's slice edge
    for k, (i, e) in enumerate(places, 1):
        keep = a.g[i][e].clone()
        a.set_bits(i, e, BAD[kind])
        before = a.state()
        a.step_guarded(w)
        assert same(a.state(), before), (kind, i, e)
        assert w.tolist() == [-1, k, k, i] and int(a.step) == 1, (kind, i, e, w.tolist())
        a.g[i][e] = keep
    # two bad arrays: the lower index is reported, whatever the order of the workgroups
    a.set_bits(3, 17, BAD[kind])
    a.set_bits(1, 2000, BAD[kind])
    before = a.state()
    a.step_guarded(w)
    n = len(places) + 1
    assert same(a.state(), before) and w.tolist() == [-1, n, n, 1]
    # … and with the gradients clean again the step is the unguarded one, and the streak ends
    a.new_gradients(5)
    b = a.copy()
    a.step_guarded(w)
    b.step_unguarded()
    assert same(a.state(), b.state()) and w.tolist() == [-1, n, 0, 1] and int(a.step) == 2


def test_denormals_zeros_and_the_largest_floats_are_finite():
    sizes = [9, 2 * S + 3, 4099]
    a = Arrays(sizes, unaligned=(2,), seed=3)
    fine = [0x00000001, 0x807FFFFF, 0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000]   # denormals, ±0, ±FLT_MAX, the smallest normal
    for j, bits in enumerate(fine):
        a.set_bits(0, j, bits)
        a.set_bits(1, S - 3 + j, bits)
        a.set_bits(2, 4092 + j, bits)
    b = a.copy()
    w = new_words()
    a.step_guarded(w)
    b.step_unguarded()
    assert same(a.state(), b.state()) and w.tolist() == CLEAN_WORDS and int(a.step) == 1


def test_more_arrays_than_one_launch_carries():
    """50 arrays of 1 … 50 elements: two launches of the scan and two of the update (48 arrays a table). The only bad value sits in array
    48, the first of the SECOND launch: arrays 0 … 47 stay untouched only if every scan launch ran before the first update launch."""
    sizes = list(range(1, 51))
    a = Arrays(sizes, seed=4)
    w = new_words()
    for k, i in enumerate((48, 0), 1):
        keep = a.g[i][0].clone()
        a.set_bits(i, 0, BAD["+nan"])
        before = a.state()
        a.step_guarded(w)
        assert same(a.state(), before), i
        assert w.tolist() == [-1, k, k, i] and int(a.step) == 0
        a.g[i][0] = keep
    b = a.copy()
    a.step_guarded(w)
    b.step_unguarded()
    assert same(a.state(), b.state()) and w.tolist() == [-1, 2, 0, 0] and int(a.step) == 1


def test_streak_counts_consecutive_withheld_updates():
    a = Arrays([100, 5000], seed=5)
    b = a.copy()
    w = new_words()
    seen = []
    for bad in (True, True, False, True):
        if bad:
            a.set_bits(1, 4999, BAD["+inf"])
        else:
            a.new_gradients(6)
            b.new_gradients(6)
            b.step_unguarded()
        a.step_guarded(w)
        seen.append(w.tolist())
    assert seen == [[-1, 1, 1, 1], [-1, 2, 2, 1], [-1, 2, 0, 1], [-1, 3, 1, 1]], seen
    assert int(a.step) == 1 and same(a.state(), b.state())


def test_empty_arrays_only_tick_the_count():
    import torch
    from latentdiffeq_amd import _lib as L
    w = new_words()
    step = torch.zeros((), dtype=torch.int64, device="cuda")
    tab = (L.AdamTensor * 2)()
    L.call("lde_adamw_flux_step_guarded", None, 2, tab, *HP, L.ptr(step), L.ptr(w), L.raw_stream())
    L.call("lde_adamw_flux_step_guarded", None, 0, None, *HP, L.ptr(step), L.ptr(w), L.raw_stream())
    assert int(step) == 2 and w.tolist() == CLEAN_WORDS


def test_guard_needs_the_capturable_form():
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    p = [torch.nn.Parameter(torch.ones(10, device="cuda"))]
    with pytest.raises(ValueError):
        FluxADAMW(p, guard=True)
    opt = FluxADAMW(p, capturable=True, guard=True)
    assert opt.guard_state() == dict(skipped=0, streak=0, last_bad_array=-1)
    p[0].grad = torch.full((10,), float("nan"), device="cuda")
    opt.step()
    assert opt.guard_state() == dict(skipped=1, streak=1, last_bad_array=0) and int(opt._step_dev) == 0
    assert torch.equal(p[0].detach(), torch.ones(10, device="cuda"))
    assert "skipped" not in str(opt.state_dict().keys()) and all(set(st) == {"exp_avg", "exp_avg_sq", "step"} for st in opt.state_dict()["state"].values())
    with opt.withheld():                                # a step withheld by hand leaves every counter where it was
        p[0].grad = torch.ones(10, device="cuda")
        opt.step()
    assert opt.guard_state() == dict(skipped=1, streak=1, last_bad_array=0) and int(opt._step_dev) == 0
    assert torch.equal(p[0].detach(), torch.ones(10, device="cuda")) and opt._guard_dev.tolist()[0] == -1
    opt.step()
    assert opt.guard_state() == dict(skipped=1, streak=0, last_bad_array=0) and int(opt._step_dev) == 1 and float(p[0].detach()[0]) < 1.0


REPLAY = r'''
import os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import numpy as np, torch
from latentdiffeq_amd import _lib as L
from tests.test_gpu_guard import Arrays, new_words, same, BAD, S
a = Arrays([5, 2049, S + 3, 4099], unaligned=(3,), seed=7)
b = a.copy()
w = new_words()
scratch, ws = Arrays([5, 2049], seed=8), new_words()         # the kernels are loaded before the capture, on arrays of no consequence
scratch.step_guarded(ws)
torch.cuda.synchronize()
src = [torch.zeros_like(g) for g in a.g]
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    for g, s in zip(a.g, src):
        g.copy_(s)
    a.step_guarded(w)
torch.cuda.synchronize()
assert int(a.step) == 0 and w.tolist() == [-1, 0, 0, -1]      # a capture runs nothing
rng = np.random.default_rng(9)
grads = [[torch.from_numpy((rng.standard_normal(n) * 0.1).astype(np.float32)).cuda() for n in a.sizes] for _ in range(2)]
poison = [g.clone() for g in grads[0]]
poison[2].view(torch.int32)[S:S + 1].copy_(torch.from_numpy(np.array([BAD["-nan-payload"]], np.uint32).view(np.int32)))
for batch in (grads[0], poison, grads[1]):                    # clean, poisoned, clean: nothing on the host touches the words in between
    for s, g in zip(src, batch):
        s.copy_(g)
    graph.replay()
for batch in grads:                                           # two eager unguarded updates
    for d, g in zip(b.g, batch):
        d.copy_(g)
    b.step_unguarded()
torch.cuda.synchronize()
assert same(a.state(), b.state())
assert w.tolist() == [-1, 1, 0, 2] and int(a.step) == 2, w.tolist()
print("ok replay")
'''


def test_replayed_graph_needs_no_reset_of_the_words(tmp_path):
    f = tmp_path / "guard_replay.py"
    f.write_text(REPLAY)
    r = subprocess.run([sys.executable, str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, LDE_ROOT=ROOT))
    assert r.returncode == 0 and "ok replay" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


END_TO_END = r'''
import ctypes as C, os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import numpy as np, torch
import latentdiffeq_amd as M
from latentdiffeq_amd import _lib as L
from latentdiffeq_amd.train import FluxADAMW, GraphedStep
from tests import guard_ref as G
dev = torch.device("cuda", 0)
ts = G.grid()
inputs = {k: tuple(torch.from_numpy(a).to(dev) for a in G.inputs(k)) for k in ("mild", "harsh")}
ibits = lambda t: t.detach().view(torch.int32)

class Model:
    def __init__(self, cap, guard):
        self.pend = M.Pendulum()                               # ForwardDiffSensitivity = LDE_SENSE_DISCRETE: a step record per solve
        assert self.pend.sensealg.code == L.SENSE_DISCRETE
        self.dec = M.Decoder(M.GOKU_basic(), (None, self.pend, None))
        self.h = self.pend._native()
        L.call("lde_set_option", self.h.ptr, b"record_capacity", float(cap))
        self.z0 = torch.nn.Parameter(torch.zeros(G.B, 2, device=dev))
        self.th = torch.nn.Parameter(torch.ones(G.B, 1, device=dev))
        self.z0_in, self.th_in = (t.clone() for t in inputs["mild"])
        self.opt = FluxADAMW([self.z0, self.th], lr=1e-3, decay=1e-10, capturable=True, guard=guard)

    def capacity(self):
        v = C.c_double(0)
        L.call("lde_get_option", self.h.ptr, b"record_capacity", C.byref(v))
        return int(v.value)

    def fn(self):
        self.opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            self.z0.copy_(self.z0_in)
            self.th.copy_(self.th_in)
        zhat = M.diffeq_layer(self.dec, (self.z0.t(), self.th.t()), ts)
        loss = (zhat ** 2).mean()
        loss.backward()
        self.opt.step()
        return loss

    def moments(self):
        return [self.opt.state[p][k].clone() for p in (self.z0, self.th) for k in ("exp_avg", "exp_avg_sq")]

    def eager(self, kind):
        for d, s in zip((self.z0_in, self.th_in), inputs[kind]):
            d.copy_(s)
        return self.fn()

W = 3
# --- the guarded captured step
g = Model(G.CAP, True)
gs = GraphedStep(g.fn, static_inputs=[g.z0_in, g.th_in], warmup=W, guard=g.opt, check_every=1)
for k in range(2):
    loss = gs.replay(*inputs["mild"])
    assert torch.isfinite(loss) and not torch.equal(g.z0.detach(), inputs["mild"][0]) and not torch.equal(g.th.detach(), inputs["mild"][1])
assert int(g.opt._step_dev) == W + 2 and g.opt.guard_state() == dict(skipped=0, streak=0, last_bad_array=-1) and gs.recoveries == 0
assert g.capacity() == G.CAP
m_before = g.moments()
gs.replay(*inputs["harsh"])                                    # the record overflows: NaN gradients, the update withheld, then ONE recovery
# nothing moved: the leaves are the values the step's update started from (fn copied the inputs into them), the moments and the count are
# what they were before the replay
assert torch.equal(ibits(g.z0), ibits(inputs["harsh"][0])) and torch.equal(ibits(g.th), ibits(inputs["harsh"][1]))
assert all(torch.equal(ibits(a), ibits(b)) for a, b in zip(g.moments(), m_before))
st = g.opt.guard_state()
assert st["skipped"] == 1 and st["streak"] == 1 and st["last_bad_array"] == 0, st
assert int(g.opt._step_dev) == W + 2 and gs.recoveries == 1 and g.capacity() >= G.HARSH_STEPS[0], (gs.recoveries, g.capacity())
loss = gs.replay(*inputs["harsh"])                             # the new capture's record holds the solve
assert torch.isfinite(loss) and torch.isfinite(g.z0.grad).all() and torch.isfinite(g.th.grad).all()
assert not torch.equal(g.z0.detach(), inputs["harsh"][0]) and not torch.equal(g.th.detach(), inputs["harsh"][1])
assert int(g.opt._step_dev) == W + 3 and gs.recoveries == 1
assert g.opt.guard_state() == dict(skipped=1, streak=0, last_bad_array=0)
# --- the twin: the same APPLIED steps eagerly, the record large from the start
t = Model(256, False)
for k in range(W + 2):
    t.eager("mild")
lt = t.eager("harsh")
torch.cuda.synchronize()
assert int(t.opt._step_dev) == W + 3 and t.capacity() == 256
diff = max(float((a - b).abs().max()) for a, b in zip([g.z0, g.th, *g.moments()], [t.z0, t.th, *t.moments()]))
print("largest difference from the eager twin:", diff, "loss", float(loss), float(lt))
assert all(torch.equal(ibits(a), ibits(b)) for a, b in zip([g.z0, g.th, *g.moments()], [t.z0, t.th, *t.moments()])), diff
assert float(loss) == float(lt)
# --- the failure the guard removes, shown once: the same sequence without it ends in NaN parameters (lde_adjoint's documented answer
# to a record that overflowed: all-NaN gradients, never a truncated sweep)
u = Model(G.CAP, False)
us = GraphedStep(u.fn, static_inputs=[u.z0_in, u.th_in], warmup=W)
for k in range(2):
    us.replay(*inputs["mild"])
assert torch.isfinite(u.z0).all()
us.replay(*inputs["harsh"])
torch.cuda.synchronize()
assert torch.isnan(u.z0).all() and torch.isnan(u.th).all() and all(torch.isnan(m).all() for m in u.moments())
assert int(u.opt._step_dev) == W + 3
print("ok end to end")
'''


def test_captured_step_survives_a_record_overflow_and_recovers(tmp_path):
    """B = 8 pendulums, T = 8, `loss = mean(ẑ²)`, the leaves ẑ₀ [B, 2] and θ [B, 1] (fn copies the static inputs into them), the record
    capacity set to 20 before the warm-up (tests/guard_ref.py: the mild inputs take ≤ 13 steps, the harsh ones ≥ 41). After the harsh
    replay "nothing moved" reads: the leaves hold exactly what fn copied in (the update started from them and was withheld) and both
    moments and the step count are bit for bit what they were before the replay."""
    f = tmp_path / "guard_end_to_end.py"
    f.write_text(END_TO_END)
    r = subprocess.run([sys.executable, str(f)], capture_output=True, text=True, timeout=600, env=dict(os.environ, LDE_ROOT=ROOT))
    print(r.stdout[-800:])
    assert r.returncode == 0 and "ok end to end" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
