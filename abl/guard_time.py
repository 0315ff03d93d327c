"""What the guard costs: lde_adamw_flux_step_guarded (a scan of every gradient, then the update) beside lde_adamw_flux_step_dev on the same
arrays, on the same box in the same run. Back-to-back C ABI calls between HIP events, `--iters` calls a window after a warm-up; the two
entry points ALTERNATE window by window (`--rounds` windows each) and the median window counts, so that whatever else shares the box
falls on both alike. Shapes: (a) the parameter arrays of the default GOKU model (784 pixels: ≈ 1.3 MB in all — launch-bound: the guard
is about one more launch); (b) one array of 2²⁶ floats (HBM-bound: the scan reads 4 bytes per element where the update moves 28).
The scan alone is timed as guarded − unguarded; its TB/s is 4 bytes · elements over that. One JSON line per shape. Recorded in
DESIGN.md §4.6, not gated.

    python abl/guard_time.py [--iters 200] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from latentdiffeq_amd import _lib as L  # noqa: E402

HP = (1e-3, 0.9, 0.999, 1e-8, 1e-10)


def goku_sizes(dev):
    import latentdiffeq_amd as M
    from latentdiffeq_amd.chain import default_decoder_layers
    from latentdiffeq_amd.recurrent import Encoder, default_encoder_layers
    mt = M.GOKU_basic()
    enc = Encoder(mt, default_encoder_layers(mt, 784, device=dev))
    dec = M.Decoder(mt, default_decoder_layers(mt, 784, M.Pendulum(), device=dev))
    mods = [enc.feature_extractor, *enc.pattern_extractor, *enc.latent_in, *dec.latent_out, dec.reconstructor]
    return [p.numel() for m in mods for p in m.parameters()]


def run(name, sizes, iters, rounds):
    dev = torch.device("cuda", 0)
    n = len(sizes)
    tab = (L.AdamTensor * n)()
    keep = []
    for i, k in enumerate(sizes):
        p, g, m, v = torch.randn(k, device=dev), torch.randn(k, device=dev) * 0.1, torch.zeros(k, device=dev), torch.zeros(k, device=dev)
        keep += [p, g, m, v]
        t = tab[i]
        t.p, t.g, t.m, t.v, t.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), k
    step = torch.zeros((), dtype=torch.int64, device=dev)
    words = torch.empty(L.GUARD_WORDS, dtype=torch.int64, device=dev)
    s = L.raw_stream(0)
    L.call("lde_guard_init", None, L.ptr(words), s)

    def plain():
        L.call("lde_adamw_flux_step_dev", None, n, tab, *HP, L.ptr(step), s)

    def guarded():
        L.call("lde_adamw_flux_step_guarded", None, n, tab, *HP, L.ptr(step), L.ptr(words), s)

    def window(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for _ in range(10):
        plain()
        guarded()
    torch.cuda.synchronize()
    us = {"unguarded": [], "guarded": []}
    for _ in range(rounds):
        us["unguarded"].append(window(plain))
        us["guarded"].append(window(guarded))
    assert words.tolist() == [-1, 0, 0, -1] and int(step) == 20 + 2 * rounds * iters      # every step was applied
    med = {k: statistics.median(v) for k, v in us.items()}
    total = sum(sizes)
    scan_us = med["guarded"] - med["unguarded"]
    return dict(shape=name, arrays=n, floats=total, iters=iters, rounds=rounds,
                unguarded_us=round(med["unguarded"], 2), guarded_us=round(med["guarded"], 2),
                unguarded_min_max_us=[round(min(us["unguarded"]), 2), round(max(us["unguarded"]), 2)],
                guarded_min_max_us=[round(min(us["guarded"]), 2), round(max(us["guarded"]), 2)],
                overhead_pct=round(100.0 * scan_us / med["unguarded"], 1), scan_us=round(scan_us, 2),
                update_TBps=round(28.0 * total / med["unguarded"] * 1e-6, 3),
                scan_TBps=round(4.0 * total / scan_us * 1e-6, 3) if scan_us > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abl/guard_time.py needs a GPU: a timing taken anywhere else says nothing")
    print(json.dumps(run("goku-default", goku_sizes(torch.device("cuda", 0)), a.iters, a.rounds)), flush=True)
    print(json.dumps(run("one-array-2^26", [1 << 26], max(a.iters // 10, 10), a.rounds)), flush=True)


if __name__ == "__main__":
    main()
