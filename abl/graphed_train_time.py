"""What the captured loop buys: wall time per minibatch of `train.train()` eager beside `train.train(graphed=True)` at the reference's
shapes [REF examples/pendulum_friction-less/model_train.jl:138-218] — the default GOKU model on 784 pixels, minibatches of B = 64 with
windows of T = 50 of 400 frames, the validation pass on 45 × 400 after every update — on the same box in the same process. A minibatch is
the training step AND that validation pass, as in the reference's loop. The two loops ALTERNATE call by call (`--rounds` calls each, two
models from the same initial weights), every call runs `--epochs` epochs of `--batches` minibatches with β changing every epoch, and
the time of an epoch is taken between the `on_epoch` calls — the host has just read the epoch's losses there in either loop, so the
device is idle at both ends. The first epoch of every call is left out (it holds the graphed loop's warm-up and capture, and the eager
loop's first-call workspace growth); the MEDIAN epoch counts. One JSON line. Recorded in DESIGN.md §4.7, not gated.

    python abl/graphed_train_time.py [--rounds 3] [--epochs 4] [--batches 6] [--variational 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import latentdiffeq_amd as la  # noqa: E402
from latentdiffeq_amd import train as TR  # noqa: E402

PIXELS, B, T, FULL, N_VAL = 784, 64, 50, 400, 45


def build(dev):
    torch.manual_seed(100)
    mt, diffeq = la.GOKU_basic(), la.Pendulum()
    enc, dec = TR.default_layers(mt, PIXELS, diffeq, device=dev)
    with torch.no_grad():
        dec[0][1]._dense[-1].bias.fill_(1.0)
    return TR.LatentDiffEqModel(mt, enc, dec)


def one_call(model, loader, val, graphed, epochs, variational, seed):
    """Seconds per epoch (from the second on) of one train() call, and its history."""
    marks = []

    def on_epoch(epoch, history):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    hist, _ = TR.train(model, loader, val, dt=0.05, epochs=epochs, seq_len=T, full_seq_len=FULL, lr=1e-3, decay=1e-10, start_beta=0.0,
                       end_beta=1.0, n_cycle=1, ratio=1, variational=variational, rng=np.random.default_rng(seed), on_epoch=on_epoch,
                       graphed=graphed)
    return [b - a for a, b in zip(marks, marks[1:])], hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--variational", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abl/graphed_train_time.py needs a GPU: a timing taken anywhere else says nothing")
    if a.epochs < 2:
        raise SystemExit("--epochs 2 at least: the first epoch of a call is not timed")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    loader = [torch.rand(PIXELS, B, FULL, device=dev) for _ in range(a.batches)]
    val = torch.rand(PIXELS, N_VAL, FULL, device=dev)
    models = {False: build(dev), True: build(dev)}
    secs = {False: [], True: []}
    finite, withheld, recoveries = True, 0, 0
    for r in range(a.rounds):
        for graphed in (False, True):
            per_epoch, hist = one_call(models[graphed], loader, val, graphed, a.epochs, bool(a.variational), seed=r)
            secs[graphed] += per_epoch
            finite = finite and all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in hist)
            if graphed:
                withheld += models[True].optimizer.guard_state()["skipped"]
                recoveries += models[True].graphed_step.recoveries
    ms = {k: [1e3 * s / a.batches for s in v] for k, v in secs.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(shape=dict(pixels=PIXELS, B=B, T=T, frames=FULL, validation=[N_VAL, FULL], batches_per_epoch=a.batches),
                          variational=bool(a.variational), rounds=a.rounds, timed_epochs_per_call=a.epochs - 1,
                          eager_ms_per_minibatch=round(med[False], 3), graphed_ms_per_minibatch=round(med[True], 3),
                          eager_min_max_ms=[round(min(ms[False]), 3), round(max(ms[False]), 3)],
                          graphed_min_max_ms=[round(min(ms[True]), 3), round(max(ms[True]), 3)],
                          eager_over_graphed=round(med[False] / med[True], 3), losses_finite=bool(finite), steps_withheld=int(withheld),
                          recoveries=int(recoveries))), flush=True)


if __name__ == "__main__":
    main()
