"""Isolated timing of lde_rnn_forward / lde_rnn_backward (HIP events) of GRU 32-16-16 next to LSTM 32-16-16 and RNN 32-16-16 at B = 256,
T = 50 (RB_B / RB_T override): one process, the three stacks alternated over several rounds, median of the rounds per (stack, call).
RB_OPT="pipe=0" (or "regw=0", "generic=1") sets a kernel-choice knob on every stack — the LSTM without its one-wave-per-cell pipeline is
the like-for-like yardstick of the GRU, which has no such form."""
import ctypes as C, sys, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latentdiffeq_amd import _lib as L
lib = L.load()
B, T = int(os.environ.get('RB_B', 256)), int(os.environ.get('RB_T', 50))
ROUNDS, REPS = 7, 50
opt = os.environ.get('RB_OPT', '')
p = lambda t: C.c_void_p(t.data_ptr())
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
x = torch.randn(T, B, 32, device="cuda"); dy = torch.randn(B, 16, device="cuda")
stacks = []
for cell, name in ((L.CELL_GRU, "gru"), (L.CELL_LSTM, "lstm"), (L.CELL_RNN_RELU, "rnn")):
    d = L.RnnDesc(); d.abi_version, d.cell, d.n_layers, d.reverse = 1, cell, 2, 1
    for i, sz in enumerate((32, 16, 16)): d.sizes[i] = sz
    h = C.c_void_p(); assert lib.lde_rnn_create(C.byref(d), C.byref(h)) == 0
    if opt:
        k, v = opt.split("=")
        assert lib.lde_rnn_set_option(h, k.encode(), float(v)) == 0
    nW = lib.lde_rnn_num_weights(C.byref(d))
    W = (np.random.default_rng(0).standard_normal(nW) * 0.2).astype(np.float32)
    assert lib.lde_rnn_set_weights(h, W.ctypes.data_as(C.c_void_p), nW) == 0
    y = torch.empty(B, 16, device="cuda"); dx = torch.empty_like(x); dW = torch.zeros(nW, device="cuda")
    f = lambda h=h, y=y: lib.lde_rnn_forward(h, p(x), T, B, p(y), s)
    b = lambda h=h, dx=dx, dW=dW: lib.lde_rnn_backward(h, p(x), p(dy), T, B, p(dx), p(dW), s)
    stacks.append((name, h, (("forward", f), ("backward", b)), (y, dx, dW)))
times = {}
for rnd in range(ROUNDS + 1):          # round 0 warms up
    for name, h, fns, _ in stacks:
        for nm, fn in fns:
            for _ in range(5): assert fn() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS): fn()
            e1.record(); torch.cuda.synchronize()
            if rnd: times.setdefault((name, nm), []).append(e0.elapsed_time(e1) / REPS * 1e3)
for (name, nm), v in times.items():
    print(f"{name:5s} {nm:8s} B={B} T={T} {opt or 'default':8s} median {np.median(v):7.1f} us  (min {min(v):.1f}, max {max(v):.1f}, {ROUNDS} rounds of {REPS})")
for _, h, _, _ in stacks: lib.lde_rnn_destroy(h)
