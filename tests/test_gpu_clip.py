"""GPU: the clipped parameter update — lde_clip_ws_bytes / lde_adamw_flux_step_clipped (include/lde.h: "the clipped step"),
`FluxADAMW(capturable=True, guard=True, clip_norm=…)`, `GraphedStep(guard=…)` with it and `train(clip_norm=…)`; every case in both modes.
References: the norms against f64 numpy; a step whose scales are all 1 against lde_adamw_flux_step_guarded on copies, bit for bit; an
active step against tests/clip_ref.py fed the f64 norms rounded to f32 — the library's own norms_dev is never a reference input.
S = 8 192 is the scan's slice per workgroup (csrc/lde_host.h: GUARD_PER_WG), 32 elements a lane; 48 arrays fill one launch's table.
Every workspace and norms buffer here is allocated with a margin filled with a pattern, and the margin is checked after every step."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import clip_ref as R
from tests.test_gpu_guard import BAD, CLEAN_WORDS, HP, Arrays, new_words, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8192
MODES = sorted(R.MODES)
INVALID = -1
WORST = {}          # what the tests measured, printed by each (run with -s): DESIGN.md §4.6 records the values


def note(key, value, show=True):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    if show:
        print(f"[clip] {key} = {WORST[key]:.3e} (the worst so far)")


class Box:
    """Arrays (tests/test_gpu_guard.py) with everything else the clipped step takes: guard words, workspace, norms. `fill` is the byte the
    workspace starts with — its contents have no meaning between calls."""

    def __init__(self, sizes, unaligned=(), seed=0, sigma=1.0, fill=0xA5, arrays=None):
        import torch
        from latentdiffeq_amd import _lib as L
        self.a = arrays if arrays is not None else Arrays(sizes, unaligned=unaligned, seed=seed)
        self.sizes = list(self.a.sizes)
        self.sigma = list(sigma) if np.ndim(sigma) else [float(sigma)] * len(self.sizes)
        if arrays is None:
            self.new_gradients(seed + 1000)
        self.w = new_words()
        self.nbytes = int(L.load().lde_clip_ws_bytes(len(self.sizes), self.a.table()))
        self.ws = torch.full((self.nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
        self.fill = fill
        self.norms = torch.full((len(self.sizes) + 3,), -7.0, device="cuda")

    def copy(self, fill=0x00):
        b = Box(self.sizes, sigma=self.sigma, fill=fill, arrays=self.a.copy())
        b.w.copy_(self.w)
        return b

    def new_gradients(self, seed):
        import torch
        rng = np.random.default_rng(seed)
        for g, s in zip(self.a.g, self.sigma):
            g.copy_(torch.from_numpy((rng.standard_normal(g.numel()) * s).astype(np.float32)))

    def grads(self):
        return [g.cpu().numpy() for g in self.a.g]

    def step(self, c, mode, expect=0):
        from latentdiffeq_amd import _lib as L
        rc = L.load().lde_adamw_flux_step_clipped(len(self.sizes), self.a.table(), *HP, c, R.MODES[mode], L.ptr(self.a.step), L.ptr(self.w),
                                                  L.ptr(self.ws), L.ptr(self.norms), L.raw_stream())
        assert rc == expect, rc
        self.check_margins()

    def check_margins(self):
        n = len(self.sizes)
        assert (self.ws[self.nbytes:] == self.fill).all() and self.norms[n + 1:].tolist() == [-7.0, -7.0]

    def read_norms(self):
        w = self.norms[:len(self.sizes) + 1].tolist()
        return w[:-1], w[-1]

    def host(self):
        return [[x.cpu().numpy() for x in arr] for arr in (self.a.p, self.a.m, self.a.v)]


def tables():
    mixed = [1, 3, 5, 0, 8191, 8192, 8193, 0, 0, 2 * S + 7, 2 ** 20 + 3, 4099]
    many = [1, 3, 5, 0, 17, 300, 2049, 0, 64]

    def cycle(nonempty, stride):                                          # `nonempty` non-empty arrays, empty ones in between
        out, i = [], 0
        while sum(1 for n in out if n) < nonempty:
            out.append(many[(stride * i) % len(many)])
            i += 1
        return out

    t49, t97 = cycle(49, 1), cycle(97, 2)                                 # two launches, three launches
    assert sum(1 for n in t49 if n) == 49 and sum(1 for n in t97 if n) == 97
    return {"mixed": (mixed, (11,)), "49 arrays": (t49, (5,)), "97 arrays": (t97, (7, 40))}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(tables()))
def test_norms_against_f64(name, mode):
    """norms_dev within 2e-6 relative of the f64 numpy norm, per array and in total: a lane adds at most 32 squares in f32 (≤ 33·2⁻²⁴ on Σg²
    with the squares' own rounding), everything above is f64; half of that on the norm, plus the final rounding to f32 = 1.04e-6."""
    sizes, unaligned = tables()[name]
    rng = np.random.default_rng(len(sizes))
    sigma = np.exp(rng.uniform(-3, 3, len(sizes)))                        # N(0, 1)·σ, σ over e⁻³ … e³
    b = Box(sizes, unaligned=unaligned, seed=21, sigma=sigma)
    per, total = R.norms(b.grads())
    b.step(2.0 * total, mode)
    got, got_total = b.read_norms()
    assert int(b.a.step) == 1 and b.w.tolist() == CLEAN_WORDS
    worst = abs(got_total - total) / total
    for n, x, y in zip(sizes, got, per):
        if n == 0:
            assert x == 0.0 and y == 0.0
        else:
            worst = max(worst, abs(x - y) / y)
    note(f"norm relative error ({name})", worst)
    assert worst <= 2e-6, worst


@pytest.mark.parametrize("mode", MODES)
def test_every_scale_one_is_the_guarded_step(mode):
    sizes = [1, 3, 2047, 2048, 2049, 0, S - 1, S, S + 1, 2 * S + 3, 4099, 0]
    b = Box(sizes, unaligned=(10, 2), seed=31, sigma=0.1)
    ref = b.a.copy()
    wref = new_words()
    for k in range(3):
        b.new_gradients(40 + k)
        for d, s in zip(ref.g, b.a.g):
            d.copy_(s)
        per, total = R.norms(b.grads())
        c = 1.5 * total if mode == "global" else 1.5 * max(per)
        b.step(c, mode)
        ref.step_guarded(wref)
        assert same(b.a.state(), ref.state()), k
        assert b.w.tolist() == CLEAN_WORDS and int(b.a.step) == k + 1
        assert same(b.a.g, ref.g)                                          # the gradients are not modified in memory


ACTIVE_SIZES = [5, S + 1, 0, 2 * S + 7, 4099, 3, 300]
ACTIVE_SIGMA = [1.0, 0.02, 1.0, 0.3, 0.05, 2.0, 0.01]


@pytest.mark.parametrize("factor", [0.1, 0.9])
@pytest.mark.parametrize("mode", MODES)
def test_active_clipping_against_the_restatement(mode, factor):
    """Five consecutive steps, new gradients each, c = factor × the first step's total norm (global) or × its median non-empty per-array norm
    (per array: some arrays over c, some under). |p − p_ref| ≤ 1e-5·η + 2⁻²²·|p|; m within 4e-6 and v within 8e-6 of their largest entry:
    the scale differs by ≤ 2e-6 relative (the norm's bound), enters m once and v squared, and Adam's quotient is scale-invariant up to ε.
    The control — the guarded step, no clipping, on copies — must miss the reference's m and v by more than 100× those tolerances."""
    b = Box(ACTIVE_SIZES, unaligned=(4,), seed=51, sigma=ACTIVE_SIGMA)
    ctrl = b.a.copy()
    wctrl = new_words()
    per0, total0 = R.norms(b.grads())
    c = factor * (total0 if mode == "global" else float(np.median([x for x in per0 if x > 0])))
    ps, ms, vs = b.host()
    clipped_arrays = set(range(len(ACTIVE_SIZES)))      # the arrays clipped at EVERY step: the control looks at those
    for k in range(1, 6):
        b.new_gradients(60 + k)
        for d, s in zip(ctrl.g, b.a.g):
            d.copy_(s)
        gs = b.grads()
        ps, ms, vs, per, total, s = R.clipped_step(ps, gs, ms, vs, k, HP, c, R.MODES[mode])
        over = [i for i, x in enumerate(s) if float(x) != 1.0]
        clipped_arrays &= set(i for i in over if ACTIVE_SIZES[i])
        if mode == "global":
            assert len(over) == len(s)
        else:
            assert over and len(over) < sum(1 for n in ACTIVE_SIZES if n), (per, c)
        b.step(c, mode)
        ctrl.step_guarded(wctrl)
        assert int(b.a.step) == k and b.w.tolist() == CLEAN_WORDS
        gp, gm, gv = b.host()
        for i, n in enumerate(ACTIVE_SIZES):
            if n == 0:
                continue
            ep = np.abs(gp[i] - ps[i]) - 2.0 ** -22 * np.abs(ps[i])
            em = np.abs(gm[i] - ms[i]).max() / np.abs(ms[i]).max()
            ev = np.abs(gv[i] - vs[i]).max() / np.abs(vs[i]).max()
            note("p: (|p − p_ref| − 2^-22·|p|) / η", max(ep.max(), 0.0) / HP[0], show=False)
            note("m: error / largest entry", em, show=False)
            note("v: error / largest entry", ev, show=False)
            assert (ep <= 1e-5 * HP[0]).all(), (k, i, ep.max())
            assert em <= 4e-6 and ev <= 8e-6, (k, i, em, ev)
    for key in sorted(WORST):
        note(key, 0.0)
    cm = [x.cpu().numpy() for x in ctrl.m]
    cv = [x.cpu().numpy() for x in ctrl.v]
    assert clipped_arrays
    dm = max(np.abs(cm[i] - ms[i]).max() / np.abs(ms[i]).max() for i in clipped_arrays)
    dv = max(np.abs(cv[i] - vs[i]).max() / np.abs(vs[i]).max() for i in clipped_arrays)
    print(f"[clip] control ({mode}, {factor}): m off by {dm:.3e}, v by {dv:.3e} of the largest entry")
    assert dm > 100 * 4e-6 and dv > 100 * 8e-6, (dm, dv)      # (the arrays whose v is mostly its starting value show less: the largest counts)


WITHHELD = ["nan", "inf", "3e19"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", WITHHELD)
def test_a_non_finite_gradient_or_norm_withholds_the_step(kind, mode):
    """A NaN, an Inf (anywhere: first and last element, either side of a slice boundary, the ragged tail of the unaligned array) and an
    array of finite 3e19 values, whose squares overflow f32: p, m, v and the step count stay bit for bit, skipped and streak go up,
    last_bad_array is the lowest offender, word [0] is −1 again, and the next clean step applies."""
    import torch
    sizes = [3, 2049, 0, 2 * S + 3, 4099, 7]
    b = Box(sizes, unaligned=(4,), seed=71, sigma=0.5)
    per, total = R.norms(b.grads())
    c = 0.5 * (total if mode == "global" else min(x for x in per if x > 0))
    b.step(c, mode)                                    # one applied step first: the count is 1, not 0
    assert int(b.a.step) == 1 and b.w.tolist() == CLEAN_WORDS
    if kind == "3e19":
        places = [(5, None), (1, None), (3, None)]
    else:
        places = [(0, 0), (5, 6), (3, S - 1), (3, S), (3, 2 * S + 2), (4, 4098), (4, 0), (1, 2048)]
    bits = {"nan": BAD["-nan-payload"], "inf": BAD["+inf"]}
    k = 0
    for k, (i, e) in enumerate(places, 1):
        keep = b.a.g[i].clone()
        if kind == "3e19":
            b.a.g[i].fill_(3e19)
            assert torch.isfinite(b.a.g[i]).all()
        else:
            b.a.set_bits(i, e, bits[kind])
        before = b.a.state()
        b.step(c, mode)
        assert same(b.a.state(), before), (kind, i, e)
        assert b.w.tolist() == [-1, k, k, i] and int(b.a.step) == 1, (kind, i, e, b.w.tolist())
        got, got_total = b.read_norms()
        assert not np.isfinite(got[i]) and not np.isfinite(got_total) and all(np.isfinite(x) for j, x in enumerate(got) if j != i)
        b.a.g[i].copy_(keep)
    # two offenders of different kinds: the lower index is reported
    keep = [g.clone() for g in b.a.g]
    b.a.g[3].fill_(3e19)
    b.a.set_bits(4, 17, BAD["+nan"])
    before = b.a.state()
    b.step(c, mode)
    k += 1
    assert same(b.a.state(), before) and b.w.tolist() == [-1, k, k, 3]
    b.a.set_bits(1, 5, BAD["-inf"])
    b.step(c, mode)
    k += 1
    assert same(b.a.state(), before) and b.w.tolist() == [-1, k, k, 1]
    # clean again: the step applies (equal to the same step taken on a copy), the streak ends
    for g, x in zip(b.a.g, keep):
        g.copy_(x)
    twin = b.copy()
    b.step(c, mode)
    twin.step(c, mode)
    assert not same(b.a.state(), before) and same(b.a.state(), twin.a.state())
    assert b.w.tolist() == [-1, k, 0, 1] and int(b.a.step) == 2


@pytest.mark.parametrize("mode", MODES)
def test_same_inputs_same_bits(mode):
    """Twice the same call on copies, the workspaces starting from different bytes: p, m, v, the count and norms_dev agree bit for bit."""
    import torch
    sizes, unaligned = tables()["mixed"]
    b = Box(sizes, unaligned=unaligned, seed=81, sigma=0.7, fill=0xA5)
    twin = b.copy(fill=0x3C)
    per, total = R.norms(b.grads())
    c = 0.3 * (total if mode == "global" else float(np.median([x for x in per if x > 0])))
    for k in range(2):
        b.new_gradients(90 + k)
        for d, s in zip(twin.a.g, b.a.g):
            d.copy_(s)
        b.step(c, mode)
        twin.step(c, mode)
        assert same(b.a.state(), twin.a.state())
        n = len(sizes) + 1
        assert torch.equal(b.norms[:n].view(torch.int32), twin.norms[:n].view(torch.int32))


def test_empty_arrays_only_tick_the_count_and_zero_the_norms():
    import torch
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    w = new_words()
    step = torch.zeros((), dtype=torch.int64, device="cuda")
    norms = torch.full((4,), -7.0, device="cuda")
    tab = (L.AdamTensor * 2)()
    for mode in (0, 1):
        assert lib.lde_adamw_flux_step_clipped(2, tab, *HP, 1.0, mode, L.ptr(step), L.ptr(w), None, L.ptr(norms), L.raw_stream()) == 0
        assert norms.tolist() == [0.0, 0.0, 0.0, -7.0]
        norms.fill_(-7.0)
        assert lib.lde_adamw_flux_step_clipped(0, None, *HP, 1.0, mode, L.ptr(step), L.ptr(w), None, L.ptr(norms), L.raw_stream()) == 0
        assert norms.tolist() == [0.0, -7.0, -7.0, -7.0]
        norms.fill_(-7.0)
    assert int(step) == 4 and w.tolist() == CLEAN_WORDS


@pytest.mark.parametrize("mode", MODES)
def test_refusals_write_nothing(mode):
    import ctypes as C
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    b = Box([5, 0, S + 1], seed=91)
    before = b.a.state() + [b.w.clone(), b.ws.clone(), b.norms.clone()]
    args = dict(c=1.0, mode=R.MODES[mode], step=L.ptr(b.a.step), guard=L.ptr(b.w), ws=L.ptr(b.ws), norms=L.ptr(b.norms))

    def call(**kw):
        a = dict(args, **kw)
        return lib.lde_adamw_flux_step_clipped(3, b.a.table(), *HP, a["c"], a["mode"], a["step"], a["guard"], a["ws"], a["norms"], L.raw_stream())

    for name in ("step", "guard", "ws", "norms"):
        assert call(**{name: None}) == INVALID, name
    for c in (0.0, -1.0, float("nan"), float("inf")):
        assert call(c=c) == INVALID, c
    for m in (-1, 2):
        assert call(mode=m) == INVALID
    assert call(ws=C.c_void_p(b.ws.data_ptr() + 4)) == INVALID
    assert same(b.a.state() + [b.w, b.ws, b.norms], before)
    assert call() == 0 and int(b.a.step) == 1


def test_clip_norm_needs_the_capturable_guarded_form_and_reports_norms():
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    p = [torch.nn.Parameter(torch.ones(10, device="cuda")), torch.nn.Parameter(torch.ones(3, device="cuda"))]
    for kw in (dict(), dict(capturable=True)):
        with pytest.raises(ValueError, match="capturable=True, guard=True"):
            FluxADAMW(p, clip_norm=1.0, **kw)
    opt = FluxADAMW(p, capturable=True, guard=True, clip_norm=1.0, clip_mode="per_array")
    ws, norms = opt._clip_ws.data_ptr(), opt._norms_dev.data_ptr()
    assert opt.grad_norms() == ([0.0, 0.0], 0.0)
    p[0].grad, p[1].grad = torch.full((10,), 2.0, device="cuda"), torch.full((3,), 0.1, device="cuda")
    opt.step()
    per, total = opt.grad_norms()
    want = [np.sqrt(40.0), np.sqrt(0.03)]
    assert abs(per[0] - want[0]) <= 2e-6 * want[0] and abs(per[1] - want[1]) <= 2e-6 * want[1] and abs(total - np.sqrt(40.03)) <= 2e-6 * total
    assert torch.equal(p[0].grad, torch.full((10,), 2.0, device="cuda"))              # the native path leaves the gradients alone
    m0, m1 = opt.state[p[0]]["exp_avg"], opt.state[p[1]]["exp_avg"]
    assert abs(float(m0[0]) - 0.1 * 2.0 / np.sqrt(40.0)) <= 1e-6 and abs(float(m1[0]) - 0.1 * 0.1) <= 1e-7   # array 0 clipped to norm 1, array 1 not
    assert (opt._clip_ws.data_ptr(), opt._norms_dev.data_ptr()) == (ws, norms) and int(opt._step_dev) == 1
    p[1].grad = torch.full((3,), 3e19, device="cuda")
    opt.step()
    assert opt.guard_state() == dict(skipped=1, streak=1, last_bad_array=1) and int(opt._step_dev) == 1


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
from latentdiffeq_amd import _lib as L
from tests import clip_ref as R
from tests.test_gpu_clip import Box, same, S
for mode in sorted(R.MODES):
    a = Box([5, 2049, 0, S + 3, 4099], unaligned=(4,), seed=7, sigma=0.5)
    b = a.copy()
    per, total = R.norms(a.grads())
    c = 0.4 * (total if mode == "global" else float(np.median([x for x in per if x > 0])))
    scratch = Box([5, 2049], seed=8)                    # the kernels are loaded before the capture, on arrays of no consequence
    scratch.step(1.0, mode)
    torch.cuda.synchronize()
    src = [torch.zeros_like(g) for g in a.a.g]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for g, s in zip(a.a.g, src):
            g.copy_(s)
        rc = L.load().lde_adamw_flux_step_clipped(len(a.sizes), a.a.table(), 1e-3, 0.9, 0.999, 1e-8, 1e-3, c, R.MODES[mode], L.ptr(a.a.step),
                                                  L.ptr(a.w), L.ptr(a.ws), L.ptr(a.norms), L.raw_stream())
        assert rc == 0
    torch.cuda.synchronize()
    assert int(a.a.step) == 0 and a.w.tolist() == [-1, 0, 0, -1]      # a capture runs nothing
    rng = np.random.default_rng(9)
    grads = [[torch.from_numpy((rng.standard_normal(n) * 0.5).astype(np.float32)).cuda() for n in a.sizes] for _ in range(3)]
    for batch in grads:                                                # three replays, new gradients copied into the fixed addresses
        for s, g in zip(src, batch):
            s.copy_(g)
        graph.replay()
    eager_norms = []
    for batch in grads:                                                # the eager sequence
        for d, g in zip(b.a.g, batch):
            d.copy_(g)
        b.step(c, mode)
    torch.cuda.synchronize()
    a.check_margins()
    assert same(a.a.state(), b.a.state()) and int(a.a.step) == 3 and a.w.tolist() == [-1, 0, 0, -1]
    n = len(a.sizes) + 1
    assert torch.equal(a.norms[:n].view(torch.int32), b.norms[:n].view(torch.int32))
print("ok replay")
'''


def test_captured_clipped_step_equals_the_eager_sequence(tmp_path):
    _run(tmp_path, "clip_replay.py", REPLAY)


GRAPHED = r'''
import os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import torch
from latentdiffeq_amd.train import FluxADAMW, GraphedStep
dev = torch.device("cuda", 0)
ibits = lambda t: t.detach().view(torch.int32)
for mode in ("global", "per_array"):
    torch.manual_seed(5)
    W = torch.nn.Parameter(torch.randn(40, 30, device=dev) * 0.1)
    bias = torch.nn.Parameter(torch.zeros(40, device=dev))
    x = torch.randn(30, 16, device=dev)
    opt = FluxADAMW([W, bias], lr=1e-3, decay=1e-10, capturable=True, guard=True, clip_norm=0.5, clip_mode=mode)

    def fn():
        opt.zero_grad(set_to_none=True)
        loss = (torch.tanh(W @ x + bias[:, None]) ** 2).mean() * 100.0
        loss.backward()
        opt.step()
        return loss

    gs = GraphedStep(fn, static_inputs=[x], warmup=2, guard=opt, check_every=1)
    for k in range(3):
        loss = gs.replay(torch.randn(30, 16, device=dev))
        assert torch.isfinite(loss)
    per, total = opt.grad_norms()
    assert int(opt._step_dev) == 5 and total > 0.5 and len(per) == 2 and gs.recoveries == 0     # the threshold was active
    assert opt.guard_state() == dict(skipped=0, streak=0, last_bad_array=-1)
    before = [W.detach().clone(), bias.detach().clone(), *[opt.state[p][k].clone() for p in (W, bias) for k in ("exp_avg", "exp_avg_sq")]]
    gs.recover()
    after = [W.detach(), bias.detach(), *[opt.state[p][k] for p in (W, bias) for k in ("exp_avg", "exp_avg_sq")]]
    assert all(torch.equal(ibits(a), ibits(b)) for a, b in zip(before, after))
    assert int(opt._step_dev) == 5 and opt.guard_state() == dict(skipped=0, streak=0, last_bad_array=-1) and gs.recoveries == 1
    loss = gs.replay(torch.randn(30, 16, device=dev))                   # the new capture runs
    assert torch.isfinite(loss) and int(opt._step_dev) == 6 and not torch.equal(W.detach(), before[0])
print("ok graphed")
'''


def test_graphed_step_runs_and_recovers_with_a_clipped_optimiser(tmp_path):
    _run(tmp_path, "clip_graphed.py", GRAPHED)


def test_train_with_clip_norm_on_the_default_goku_model():
    """train() on the default GOKU model (28×28 input, B = 8, T = 10): one epoch of two minibatches with clip_norm = 0.5."""
    import torch
    import latentdiffeq_amd as la
    from latentdiffeq_amd import train as TR
    torch.manual_seed(4)
    mt, diffeq = la.GOKU_basic(), la.Pendulum()
    enc, dec = TR.default_layers(mt, 784, diffeq, device="cuda")
    with torch.no_grad():
        dec[0][1]._dense[-1].bias.fill_(1.0)
    model = TR.LatentDiffEqModel(mt, enc, dec)
    data = torch.rand(784, 24, 12, device="cuda")                       # 12 frames, windows of T = 10 (time_loader)
    loader = [data[:, :8], data[:, 8:16]]
    for mode in MODES:
        hist, best = TR.train(model, loader, data[:, 16:, :10], dt=0.05, epochs=1, seq_len=10, full_seq_len=12, rng=np.random.default_rng(0),
                              clip_norm=0.5, clip_mode=mode)
        opt = model.optimizer
        per, total = opt.grad_norms()
        assert len(hist) == 2 and all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in hist)
        assert all(torch.isfinite(p).all() for p in model.parameters()) and best is not None
        assert opt.clip_norm == 0.5 and opt.capturable and opt.guard and total > 0 and len(per) == len(model.parameters())
        assert int(opt._step_dev) == 2 and opt.guard_state()["skipped"] == 0
