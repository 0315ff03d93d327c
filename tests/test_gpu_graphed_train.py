"""GPU: `train.train(graphed=True)` — the epoch loop on captured graphs with the KL weight β in a device word — on the default GOKU
model (784 pixels, B = 8, two minibatches per epoch, windows of T = 10 of 12 frames, validation 8 × 12; the shapes of
tests/test_gpu_clip.py's train() test). The reference is an eager loop this file writes from the public pieces (loss_batch with a β word,
FluxADAMW(capturable=True, guard=True), refresh_weights, the validation pass after each update) from identical initial weights: history,
final parameters and best_state must agree BIT FOR BIT. Both run the encoder on one stream (recurrent._BRANCH_STREAMS = False, which
train(graphed=True) sets for its call: a capture needs one stream, and the one-stream encoder node adds its frame gradients in its own
order). Everything that captures a graph runs in a fresh child process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = r'''
import os, sys
sys.path.insert(0, os.environ["LDE_ROOT"])
import numpy as np, torch
import latentdiffeq_amd as la
from latentdiffeq_amd import train as TR, recurrent as R, loss as LS
ibits = lambda t: t.detach().contiguous().view(torch.int32)
same = lambda a, b: torch.equal(ibits(a), ibits(b))
DT, FULL, T = 0.05, 12, 10

def build():
    torch.manual_seed(4)
    mt, diffeq = la.GOKU_basic(), la.Pendulum()
    enc, dec = TR.default_layers(mt, 784, diffeq, device="cuda")
    with torch.no_grad():
        dec[0][1]._dense[-1].bias.fill_(1.0)
    return TR.LatentDiffEqModel(mt, enc, dec)

torch.manual_seed(7)
data = torch.rand(784, 24, FULL, device="cuda")
loader, val = [data[:, :8], data[:, 8:16]], data[:, 16:]

def eager_loop(model, epochs, variational, prog=None):
    """The loop of train() written out: β word, capturable guarded ADAMW, the validation pass after each update."""
    keep = R._BRANCH_STREAMS
    R._BRANCH_STREAMS = False
    try:
        params = model.parameters()
        opt = TR.FluxADAMW(params, lr=1e-3, betas=(0.9, 0.999), decay=1e-10, capturable=True, guard=True)
        schedule = TR.frange_cycle_linear(epochs, 0.0, 1.0, 1, 1.0)
        word = torch.zeros(1, device="cuda")
        rng = np.random.default_rng(0)
        t_val = np.arange(val.shape[2]) * DT
        hist, best, best_state = [], float("inf"), None
        for epoch in range(1, epochs + 1):
            word.fill_(float(schedule[epoch - 1]))
            sl = prog[epoch - 1] if prog is not None and epoch <= len(prog) else T
            t = np.arange(sl) * DT
            for x in loader:
                xb = TR.time_loader(x, FULL, sl, rng)
                opt.zero_grad(set_to_none=True)
                loss = TR.loss_batch(model, xb, t, word, variational)
                loss.backward()
                opt.step()
                model.refresh_weights()
                with torch.no_grad():
                    v = float(TR.loss_batch(model, val, t_val, word, False))
                hist.append((epoch, float(loss.detach()), v))
            if v < best:
                best, best_state = v, [p.detach().clone() for p in params]
        return hist, best_state, opt
    finally:
        R._BRANCH_STREAMS = keep
'''

COMPARE = COMMON + r'''
progressive = sys.argv[1] == "progressive"
kw = dict(progressive_training=True, prog_training_duration=2, start_seq_len=6) if progressive else {}
a, b = build(), build()
assert all(same(p, q) for p, q in zip(a.parameters(), b.parameters()))
schedule = TR.frange_cycle_linear(3, 0.0, 1.0, 1, 1.0)
assert schedule[0] == 0.0 and abs(float(schedule[1]) - 1 / 3) < 1e-6 and schedule[2] == 1.0       # another β every epoch
hist_g, best_g = TR.train(a, loader, val, dt=DT, epochs=3, seq_len=T, full_seq_len=FULL, lr=1e-3, decay=1e-10, start_beta=0.0, end_beta=1.0,
                          n_cycle=1, ratio=1, variational=False, rng=np.random.default_rng(0), graphed=True, **kw)
hist_e, best_e, opt_e = eager_loop(b, 3, False, prog=[6, 10] if progressive else None)
opt = a.optimizer
print("graphed", hist_g)
print("eager  ", hist_e)
assert len(hist_g) == 6 and [h[0] for h in hist_g] == [1, 1, 2, 2, 3, 3]
assert all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in hist_g)
f32 = lambda h: [(e, np.float32(x).tobytes(), np.float32(y).tobytes()) for e, x, y in h]
assert f32(hist_g) == f32(hist_e), (hist_g, hist_e)
assert all(same(p, q) for p, q in zip(a.parameters(), b.parameters()))
assert int(opt._step_dev) == 6 and int(opt_e._step_dev) == 6 and opt.guard_state()["skipped"] == 0
assert opt.capturable and opt.guard and a.graphed_step is not None and a.graphed_step.recoveries == 0
assert best_g is not None and len(best_g) == len(best_e) and all(same(p, q) for p, q in zip(best_g, best_e))
assert float(a.beta_word) == 1.0
print("ok compare", sys.argv[1])
'''

VARIATIONAL = COMMON + r'''
# (1) train(graphed=True, variational=True), one epoch
R._BRANCH_STREAMS = True
m = build()
hist, best = TR.train(m, loader, val, dt=DT, epochs=1, seq_len=T, full_seq_len=FULL, start_beta=0.0, end_beta=0.5, n_cycle=1, ratio=1,
                      variational=True, rng=np.random.default_rng(0), graphed=True)
opt = m.optimizer
print("variational", hist)
assert len(hist) == 2 and all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in hist) and best is not None
assert int(opt._step_dev) == 2 and opt.guard_state()["skipped"] == 0
assert float(m.beta_word) == float(TR.frange_cycle_linear(1, 0.0, 0.5, 1, 1)[-1]) == 0.5
assert R._BRANCH_STREAMS is True
assert all(torch.isfinite(p).all() for p in m.parameters())

# (2) β takes effect under sampling: one capture with a β word follows the word; at β₂ it equals a capture made with the number β₂
R._BRANCH_STREAMS = False
model = build()
params = model.parameters()
epoch_word = torch.tensor(5, dtype=torch.int64, device="cuda")       # the noise epoch is the test's: fixed, so ε is the same everywhere
LS.set_noise_epoch(epoch_word)
x, t = data[:, :8, :T].contiguous(), np.arange(T) * DT
B1, B2 = 0.25, 0.75
word = torch.full((1,), B1, device="cuda")

def fb(beta):
    for p in params:
        p.grad = None
    loss = TR.loss_batch(model, x, t, beta, True)
    loss.backward()
    return loss

torch.manual_seed(11)
fb(word); fb(B2)                                                     # eager: workspaces sized, the generator state seen outside a capture
model.refresh_weights()
torch.cuda.synchronize()
base = dict(LS._noise_base)

def capture(beta):
    LS._noise_call[0] = 0                                            # the same call indices in both captures
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = fb(beta)
        out = [loss.detach().clone()] + [p.grad for p in params]
    torch.cuda.synchronize()
    return g, out

g1, out1 = capture(word)
calls = LS._noise_call[0]
word.fill_(B1); g1.replay(); torch.cuda.synchronize()
at1 = [o.clone() for o in out1]
word.fill_(B2); g1.replay(); torch.cuda.synchronize()
at2 = [o.clone() for o in out1]
g2, out2 = capture(B2)
assert LS._noise_base == base and LS._noise_call[0] == calls and calls >= 2 and int(epoch_word) == 5
g2.replay(); torch.cuda.synchronize()
assert len(at2) == len(out2) == len(params) + 1
assert all(same(u, v) for u, v in zip(at2, out2)), "the word at β₂ differs from the number β₂"
assert not same(at1[0], at2[0]) and any(not same(u, v) for u, v in zip(at1[1:], at2[1:]))     # β₁ gave another loss and other gradients
print("ok variational")
'''


def _run(tmp_path, name, text, *args):
    f = tmp_path / name
    f.write_text(text)
    r = subprocess.run([sys.executable, str(f), *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, LDE_ROOT=ROOT))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "ok " in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_graphed_train_equals_the_eager_loop_bit_for_bit(tmp_path):
    """variational=False, three epochs at β = 0, ⅓, 1: history, final parameters and best_state of train(graphed=True) against the eager
    loop; six steps counted on the device, none withheld."""
    _run(tmp_path, "graphed_train.py", COMPARE, "plain")


def test_progressive_training_runs_eager_until_the_full_length_then_captures(tmp_path):
    """progressive_training over two epochs from 6 frames: the epochs run at 6, 10, 10 — the first eagerly, the capture at the second."""
    _run(tmp_path, "graphed_train_prog.py", COMPARE, "progressive")


def test_variational_graphed_train_and_the_beta_word_under_sampling(tmp_path):
    """One variational epoch of train(graphed=True) (finite history, two steps, nothing withheld, the β word at the schedule's last value,
    the branch-stream switch put back), and the step-level check: a captured forward + backward of loss_batch(variational=True) with a β
    word, replayed at β₁ and — the word rewritten — at β₂, where the loss and every parameter gradient are the bits of a graph captured
    with the Python float β₂ at the same ε (seed, offset, call indices and the epoch word pinned)."""
    _run(tmp_path, "graphed_train_var.py", VARIATIONAL)
