"""GPU: the KL-carrying loss terms with β in device memory (include/lde.h: lde_kl_*_dev, lde_sample_kl_*_dev, lde_sample_kl_pair_*_dev)
against their twins on the same inputs. The reference of every case is the existing entry point called with
scale = np.float32(β) / np.float32(divisor) (numpy's f32 division): the results must be the twin's BIT FOR BIT — the kernels form
s = β ⊘ divisor as one correctly rounded f32 division and are the twin from there. n = 8192 is the largest one-workgroup sum (the
partial kernel makes the last store itself), 8193 the smallest that takes the separate last kernel; divisor 3 gives an inexact quotient."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
SIZES = [1, 37, 8192, 8193]
DIVISORS = [2.0, 3.0, 64.0]
BETAS = [0.0, 1.0, float(np.float32(0.3)), 1e-3]
PAD = 8          # floats of pattern behind every output: checked after every call


def scale_of(beta, divisor):
    return float(np.float32(beta) / np.float32(divisor))


class Buf:
    """Device arrays of n floats each, every one (with `shift`) starting one float past a 16-byte boundary, with a patterned margin."""

    def __init__(self, n, shift, seed):
        import torch
        self.n, self.shift = n, shift
        rng = np.random.default_rng(seed)
        self._store = {}
        for name, sigma in (("mu", 1.0), ("lv", 0.5), ("eps", 1.0), ("dl", 1.0)):
            self._store[name] = self._place(torch.from_numpy((rng.standard_normal(n) * sigma).astype(np.float32)))
        self.g = torch.tensor([0.7], device="cuda")
        self.base = torch.tensor([1.25], device="cuda")

    def _place(self, host):
        import torch
        t = torch.full((self.n + self.shift + PAD + 4,), -7.0, device="cuda")
        t[self.shift:self.shift + self.n].copy_(host)
        return t

    def new(self):
        import torch
        return torch.full((self.n + self.shift + PAD + 4,), -7.0, device="cuda")

    def view(self, t):
        return t[self.shift:self.shift + self.n]

    def __getattr__(self, name):
        return self.view(self._store[name])

    def margins_ok(self, *outs):
        return all((t[:self.shift] == -7.0).all() and (t[self.shift + self.n:] == -7.0).all() for t in outs)


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def scratch():
    import torch
    from latentdiffeq_amd import _lib as L
    return torch.full((L.LOSS_SCRATCH_FLOATS + 1 + PAD,), -7.0, device="cuda")


def p(t, off=0):
    from latentdiffeq_amd import _lib as L
    return L.ptr(t, 4 * off)


CASES = [(n, 0) for n in SIZES] + [(37, 1)]


@pytest.mark.parametrize("n,shift", CASES)
def test_single_forms_equal_their_twins_bit_for_bit(n, shift):
    """lde_kl_forward_dev / _backward_dev and lde_sample_kl_forward_dev / _backward_dev over every (β, divisor), with and without `base`.
    (lde_kl_forward has no base: with one, the twin is lde_kl_forward followed by the f32 addition base + term — the separately rounded
    sum the header states.)"""
    import torch
    from latentdiffeq_amd import _lib as L
    lib, st = L.load(), L.raw_stream()
    b = Buf(n, shift, seed=n + shift)
    word = torch.zeros(1, device="cuda")
    for beta in BETAS:
        word.fill_(beta)
        for div in DIVISORS:
            s = scale_of(beta, div)
            for base in (None, b.base):
                # kl forward
                w0, w1 = scratch(), scratch()
                assert lib.lde_kl_forward(p(b.mu), p(b.lv), n, s, p(w0), p(w0, 1), st) == 0
                assert lib.lde_kl_forward_dev(p(b.mu), p(b.lv), n, p(word), div, L.ptr(base), p(w1), p(w1, 1), st) == 0
                want = w0[0:1] if base is None else base + w0[0:1]
                assert same(want, w1[0:1]), ("kl", beta, div, base is not None, float(want), float(w1[0]))
                assert (w1[-PAD:] == -7.0).all()
                # sample + kl forward
                w0, w1, l0, l1 = scratch(), scratch(), b.new(), b.new()
                assert lib.lde_sample_kl_forward(p(b.mu), p(b.lv), p(b.eps), n, s, L.ptr(base), p(b.view(l0)), p(w0), p(w0, 1), st) == 0
                assert lib.lde_sample_kl_forward_dev(p(b.mu), p(b.lv), p(b.eps), n, p(word), div, L.ptr(base), p(b.view(l1)), p(w1), p(w1, 1),
                                                     st) == 0
                assert same(w0[0:1], w1[0:1]) and same(l0, l1) and b.margins_ok(l1), ("sample_kl", beta, div)
                assert (w1[-PAD:] == -7.0).all()
            # the pullbacks
            d0, d1, e0, e1 = b.new(), b.new(), b.new(), b.new()
            assert lib.lde_kl_backward(p(b.mu), p(b.lv), n, s, p(b.g), p(b.view(d0)), p(b.view(e0)), st) == 0
            assert lib.lde_kl_backward_dev(p(b.mu), p(b.lv), n, p(word), div, p(b.g), p(b.view(d1)), p(b.view(e1)), st) == 0
            assert same(d0, d1) and same(e0, e1) and b.margins_ok(d1, e1), ("kl backward", beta, div)
            d0, d1, e0, e1 = b.new(), b.new(), b.new(), b.new()
            assert lib.lde_sample_kl_backward(p(b.mu), p(b.lv), p(b.eps), p(b.dl), p(b.g), s, n, p(b.view(d0)), p(b.view(e0)), st) == 0
            assert lib.lde_sample_kl_backward_dev(p(b.mu), p(b.lv), p(b.eps), p(b.dl), p(b.g), p(word), div, n, p(b.view(d1)), p(b.view(e1)),
                                                  st) == 0
            assert same(d0, d1) and same(e0, e1) and b.margins_ok(d1, e1), ("sample_kl backward", beta, div)
            if beta:
                assert float(d1.abs().max()) > 0


class Pair:
    """The arguments of the pair forms: two parts, explicit seed / offsets / call indices and an epoch word."""
    SEED, OFF_A, OFF_B, CALL_A, CALL_B = 0x0123456789ABCDEF, (1 << 40) + 8, (1 << 40) + 8, 3, 4

    def __init__(self, n_a, n_b, seed=5):
        import torch
        self.a, self.b = Buf(n_a, 0, seed), Buf(n_b, 0, seed + 1)
        self.epoch = torch.tensor(11, dtype=torch.int64, device="cuda")
        self.g = torch.tensor([0.7], device="cuda")

    def forward(self, dev, beta_or_word, div_a, div_b, base=None, check=True):
        """(eps_a, eps_b, l_a, l_b, total); `dev`: the β word form, else the twin with the f32 quotients as scales. `check=False`: inside a
        capture, where nothing can be read."""
        import torch
        from latentdiffeq_amd import _lib as L
        lib, a, b = L.load(), self.a, self.b
        out = [a.new(), b.new(), a.new(), b.new()]
        ws = torch.full((3 + PAD,), -7.0, device="cuda")
        views = [a.view(out[0]), b.view(out[1]), a.view(out[2]), b.view(out[3])]
        if dev:
            rc = lib.lde_sample_kl_pair_forward_dev(p(a.mu), p(a.lv), a.n, div_a, p(b.mu), p(b.lv), b.n, div_b, p(beta_or_word), L.ptr(base), self.SEED,
                                                    self.OFF_A, self.OFF_B, self.CALL_A, self.CALL_B, p(self.epoch), *[p(v) for v in views], p(ws),
                                                    p(ws, 1), L.raw_stream())
        else:
            rc = lib.lde_sample_kl_pair_forward(p(a.mu), p(a.lv), a.n, scale_of(beta_or_word, div_a), p(b.mu), p(b.lv), b.n,
                                                scale_of(beta_or_word, div_b), L.ptr(base), self.SEED, self.OFF_A, self.OFF_B, self.CALL_A, self.CALL_B,
                                                p(self.epoch), *[p(v) for v in views], p(ws), p(ws, 1), L.raw_stream())
        assert rc == 0, rc
        assert not check or (a.margins_ok(out[0], out[2]) and b.margins_ok(out[1], out[3]) and (ws[3:] == -7.0).all())
        return views + [ws[0:1]]

    def backward(self, dev, beta_or_word, div_a, div_b, eps_a, eps_b, check=True):
        from latentdiffeq_amd import _lib as L
        lib, a, b = L.load(), self.a, self.b
        out = [a.new(), a.new(), b.new(), b.new()]
        views = [a.view(out[0]), a.view(out[1]), b.view(out[2]), b.view(out[3])]
        if dev:
            rc = lib.lde_sample_kl_pair_backward_dev(p(a.mu), p(a.lv), p(eps_a), p(a.dl), a.n, div_a, p(b.mu), p(b.lv), p(eps_b), p(b.dl), b.n, div_b,
                                                     p(beta_or_word), p(self.g), *[p(v) for v in views], L.raw_stream())
        else:
            rc = lib.lde_sample_kl_pair_backward(p(a.mu), p(a.lv), p(eps_a), p(a.dl), a.n, scale_of(beta_or_word, div_a), p(b.mu), p(b.lv), p(eps_b),
                                                 p(b.dl), b.n, scale_of(beta_or_word, div_b), p(self.g), *[p(v) for v in views], L.raw_stream())
        assert rc == 0, rc
        assert not check or (a.margins_ok(out[0], out[1]) and b.margins_ok(out[2], out[3]))
        return views


@pytest.mark.parametrize("n_a,n_b", [(32, 32), (8192, 1)])
def test_pair_forms_equal_their_twins_bit_for_bit(n_a, n_b):
    """ε, l̃, the total and all four gradients of the pair forms, over every (β, divisor) — the two parts with different divisors — with and
    without `base`."""
    import torch
    pr = Pair(n_a, n_b)
    word = torch.zeros(1, device="cuda")
    base = torch.tensor([1.25], device="cuda")
    for beta in BETAS:
        word.fill_(beta)
        for div_a, div_b in zip(DIVISORS, DIVISORS[1:] + DIVISORS[:1]):
            for bs in (None, base):
                want = pr.forward(False, beta, div_a, div_b, bs)
                got = pr.forward(True, word, div_a, div_b, bs)
                assert all(same(x, y) for x, y in zip(want, got)), (beta, div_a, div_b, bs is not None)
            assert float(got[0].abs().max()) > 0 and not same(got[0][:1], got[2][:1])          # ε was drawn, l̃ is not ε
            gw = pr.backward(False, beta, div_a, div_b, want[0], want[1])
            gg = pr.backward(True, word, div_a, div_b, got[0], got[1])
            assert all(same(x, y) for x, y in zip(gw, gg)), (beta, div_a, div_b)


def test_pair_forms_keep_the_size_limit_and_refuse_bad_arguments():
    import torch
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    pr = Pair(32, 32)
    big = Pair(8193, 1)
    word = torch.ones(1, device="cuda")
    for q, n_a, n_b in ((big, 8193, 1), (big, 1, 8193)):
        a, b = q.a, q.b
        x = a.mu          # (refused on the host: never dereferenced)
        rc = lib.lde_sample_kl_pair_forward_dev(p(x), p(x), n_a, 2.0, p(x), p(x), n_b, 2.0, p(word), None, 1, 0, 0, 0, 0, None, p(x), p(x), p(x), p(x),
                                                p(x), p(x), L.raw_stream())
        assert rc == UNSUPPORTED
    a, b = pr.a, pr.b
    outs = [a.new() for _ in range(6)]
    before = [t.clone() for t in outs]

    def fwd(beta=word, div_a=2.0, div_b=3.0):
        return lib.lde_sample_kl_pair_forward_dev(p(a.mu), p(a.lv), a.n, div_a, p(b.mu), p(b.lv), b.n, div_b, L.ptr(beta), None, 1, 0, 0, 0, 0, None,
                                                  *[p(t) for t in outs], L.raw_stream())

    def bwd(beta=word, div_a=2.0, div_b=3.0):
        return lib.lde_sample_kl_pair_backward_dev(p(a.mu), p(a.lv), p(a.eps), p(a.dl), a.n, div_a, p(b.mu), p(b.lv), p(b.eps), p(b.dl), b.n, div_b,
                                                   L.ptr(beta), p(pr.g), *[p(t) for t in outs[:4]], L.raw_stream())

    for f in (fwd, bwd):
        assert f(beta=None) == INVALID
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert f(div_a=bad) == INVALID and f(div_b=bad) == INVALID, bad
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(outs, before))            # a refusal writes nothing
    assert fwd() == 0 and bwd() == 0


def test_single_forms_refuse_bad_arguments():
    import torch
    from latentdiffeq_amd import _lib as L
    lib, st = L.load(), L.raw_stream()
    b = Buf(37, 0, seed=3)
    word = torch.ones(1, device="cuda")
    outs = [b.new() for _ in range(2)]
    ws = scratch()
    before = [t.clone() for t in outs + [ws]]
    o0, o1 = b.view(outs[0]), b.view(outs[1])
    calls = {
        "kl_forward": lambda w, d: lib.lde_kl_forward_dev(p(b.mu), p(b.lv), b.n, L.ptr(w), d, None, p(ws), p(ws, 1), st),
        "kl_backward": lambda w, d: lib.lde_kl_backward_dev(p(b.mu), p(b.lv), b.n, L.ptr(w), d, p(b.g), p(o0), p(o1), st),
        "sample_kl_forward": lambda w, d: lib.lde_sample_kl_forward_dev(p(b.mu), p(b.lv), p(b.eps), b.n, L.ptr(w), d, None, p(o0), p(ws), p(ws, 1), st),
        "sample_kl_backward": lambda w, d: lib.lde_sample_kl_backward_dev(p(b.mu), p(b.lv), p(b.eps), p(b.dl), p(b.g), L.ptr(w), d, b.n, p(o0), p(o1),
                                                                          st),
    }
    for name, f in calls.items():
        assert f(None, 2.0) == INVALID, name
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert f(word, bad) == INVALID, (name, bad)
    # what the twins refuse
    assert lib.lde_kl_forward_dev(None, p(b.lv), b.n, p(word), 2.0, None, p(ws), p(ws, 1), st) == INVALID
    assert lib.lde_kl_forward_dev(p(b.mu), p(b.lv), -1, p(word), 2.0, None, p(ws), p(ws, 1), st) == INVALID
    assert lib.lde_kl_forward_dev(p(b.mu), p(b.lv), b.n, p(word), 2.0, None, None, p(ws, 1), st) == INVALID
    assert lib.lde_kl_backward_dev(p(b.mu), p(b.lv), b.n, p(word), 2.0, None, p(o0), p(o1), st) == INVALID
    assert lib.lde_sample_kl_forward_dev(p(b.mu), p(b.lv), None, b.n, p(word), 2.0, None, p(o0), p(ws), p(ws, 1), st) == INVALID
    assert lib.lde_sample_kl_backward_dev(p(b.mu), p(b.lv), p(b.eps), p(b.dl), None, p(word), 2.0, b.n, p(o0), p(o1), st) == INVALID
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(outs + [ws], before))
    for name, f in calls.items():
        assert f(word, 2.0) == 0, name


def test_python_layer_routes_a_beta_word_to_the_dev_entry_points():
    """loss.sample_with_kl (pair and single forms) and loss.beta_kl with a β word against the same call with the number, ε shared: the
    total and the gradients of μ and logσ² agree bit for bit for the sample forms (scale = f32(β/B) either way at these values), and
    beta_kl equals the chained lde_kl_forward twins."""
    import torch
    from latentdiffeq_amd import loss as LS
    torch.manual_seed(3)
    B, beta = 8, 0.25
    word = torch.full((1,), beta, device="cuda")
    mus = tuple(torch.randn(16, B, device="cuda", requires_grad=True) for _ in range(2))
    lvs = tuple((0.3 * torch.randn(16, B, device="cuda")).requires_grad_() for _ in range(2))
    eps = tuple(torch.randn(16, B, device="cuda") for _ in range(2))
    res = []
    for bt in (beta, word):
        for t in (*mus, *lvs):
            t.grad = None
        (la, lb), total = LS.sample_with_kl(mus, lvs, bt, None, eps=eps)
        (total * 1.5 + (la * la).sum() + lb.sum()).backward()
        res.append([total.detach().clone(), la.detach().clone(), lb.detach().clone(), *[t.grad.clone() for t in (*mus, *lvs)]])
    assert all(same(x, y) for x, y in zip(*res))
    assert word.grad is None
    # the pair form draws its own ε: two calls from the same generator state
    res = []
    for bt in (beta, word):
        torch.manual_seed(9)
        for t in (*mus, *lvs):
            t.grad = None
        (la, lb), total = LS.sample_with_kl(mus, lvs, bt)
        (total * 1.5 + (la * la).sum() + lb.sum()).backward()
        res.append([total.detach().clone(), la.detach().clone(), lb.detach().clone(), *[t.grad.clone() for t in (*mus, *lvs)]])
    assert all(same(x, y) for x, y in zip(*res))
    # beta_kl: (β ⊘ B)·Σ kl_a, then + (β ⊘ B)·Σ kl_b through `base`
    for t in (*mus, *lvs):
        t.grad = None
    got = LS.beta_kl(mus, lvs, word)
    got.backward()
    s = scale_of(beta, B)
    parts = [LS._kl_sum(m.detach(), v.detach(), s) for m, v in zip(mus, lvs)]
    assert same(got, parts[0] + parts[1])
    for m, v in zip(mus, lvs):
        mm, vv = m.detach().clone().requires_grad_(), v.detach().clone().requires_grad_()
        LS._kl_sum(mm, vv, s).backward()
        assert same(m.grad, mm.grad) and same(v.grad, vv.grad)
    assert float(LS.beta_kl(mus, lvs, beta).detach()) == pytest.approx(float(got.detach()), rel=1e-6)      # the number form: beta * vector_kl
    with pytest.raises(TypeError):
        LS.beta_kl(mus, lvs, torch.zeros(2, device="cuda"))
    with pytest.raises(TypeError):
        LS.sample_with_kl(mus, lvs, torch.zeros(1, device="cuda", dtype=torch.float64))


REPLAY = r'''
import os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import numpy as np, torch
from tests.test_gpu_beta_dev import Pair, same
pr = Pair(32, 8192)
word = torch.zeros(1, device="cuda")
div_a, div_b = 3.0, 64.0
word.fill_(1.0)
warm = pr.forward(True, word, div_a, div_b)                      # the kernels are loaded before the capture
pr.backward(True, word, div_a, div_b, warm[0], warm[1])
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    fw = pr.forward(True, word, div_a, div_b, check=False)
    bw = pr.backward(True, word, div_a, div_b, fw[0], fw[1], check=False)
torch.cuda.synchronize()
seen = []
for beta in (0.25, 0.75):
    word.fill_(beta)                                             # the host writes the word; the graph is what it was
    graph.replay()
    torch.cuda.synchronize()
    want_f = pr.forward(False, beta, div_a, div_b)               # the eager twin at this β (the epoch word is fixed: the same ε)
    want_b = pr.backward(False, beta, div_a, div_b, want_f[0], want_f[1])
    assert all(same(x, y) for x, y in zip(want_f + want_b, fw + bw)), beta
    seen.append([t.clone() for t in fw + bw])
assert same(seen[0][0], seen[1][0]) and not same(seen[0][4], seen[1][4]) and not same(seen[0][5], seen[1][5])   # same ε, another total, other gradients
print("ok replay")
'''


def test_the_beta_word_is_read_at_run_time(tmp_path):
    """One forward + backward pair of the pair form captured in a graph; replayed at β = 0.25, then — 0.75 written into the word — again:
    each replay equals the eager twin at that β bit for bit."""
    f = tmp_path / "beta_replay.py"
    f.write_text(REPLAY)
    r = subprocess.run([sys.executable, str(f)], capture_output=True, text=True, timeout=300, env=dict(os.environ, LDE_ROOT=ROOT))
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok replay" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
