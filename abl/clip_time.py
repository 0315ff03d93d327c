"""What clipping costs: lde_adamw_flux_step_clipped (the guard's scan with Σg² on the same loads, one finalising workgroup, the update
with g scaled as it is loaded) beside lde_adamw_flux_step_guarded on the same arrays, on the same box in the same run. Back-to-back C ABI
calls between HIP events, `--iters` calls a window after a warm-up; the two entry points ALTERNATE window by window (`--rounds` windows
each) and the median window counts, so that whatever else shares the box falls on both alike. Shapes: (a) the parameter arrays of the
default GOKU model (784 pixels: launch-bound — the clipped step is one more launch, and its scan and finalising kernel end in a
workgroup-wide sum); (b) one array of 2²⁶ floats (HBM-bound: the same bytes as the guarded step, plus 8 192 partials for ONE wave of the
finalising kernel to add). The threshold is half the gradient norm, so the scale is active; both modes. One JSON line per shape and
mode. Recorded in DESIGN.md §4.6, not gated.

    python abl/clip_time.py [--iters 200] [--rounds 9]
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


def run(name, sizes, mode, iters, rounds):
    dev = torch.device("cuda", 0)
    n = len(sizes)
    tab = (L.AdamTensor * n)()
    keep = []
    for i, k in enumerate(sizes):
        p, g, m, v = torch.randn(k, device=dev), torch.randn(k, device=dev) * 0.1, torch.zeros(k, device=dev), torch.zeros(k, device=dev)
        keep += [p, g, m, v]
        t = tab[i]
        t.p, t.g, t.m, t.v, t.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), k
    total = sum(sizes)
    norm = 0.1 * total ** 0.5
    clip = 0.5 * norm if mode == "global" else 0.5 * 0.1 * (sorted(sizes)[n // 2]) ** 0.5      # half the norm / half the median array's
    step = torch.zeros((), dtype=torch.int64, device=dev)
    words = torch.empty(L.GUARD_WORDS, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(L.load().lde_clip_ws_bytes(n, tab)), 8), dtype=torch.uint8, device=dev)
    norms = torch.zeros(n + 1, device=dev)
    s = L.raw_stream(0)
    L.call("lde_guard_init", None, L.ptr(words), s)

    def guarded():
        L.call("lde_adamw_flux_step_guarded", None, n, tab, *HP, L.ptr(step), L.ptr(words), s)

    def clipped():
        L.call("lde_adamw_flux_step_clipped", None, n, tab, *HP, clip, L.CLIP_MODES[mode], L.ptr(step), L.ptr(words), L.ptr(ws), L.ptr(norms), s)

    def window(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for _ in range(10):
        guarded()
        clipped()
    torch.cuda.synchronize()
    us = {"guarded": [], "clipped": []}
    for _ in range(rounds):
        us["guarded"].append(window(guarded))
        us["clipped"].append(window(clipped))
    assert words.tolist() == [-1, 0, 0, -1] and int(step) == 20 + 2 * rounds * iters      # every step was applied
    got = float(norms[n])
    assert abs(got - norm) <= 0.02 * norm, (got, norm)                                      # the norm it measured is the gradients'
    med = {k: statistics.median(v) for k, v in us.items()}
    extra = med["clipped"] - med["guarded"]
    return dict(shape=name, mode=mode, arrays=n, floats=total, iters=iters, rounds=rounds, ws_bytes=int(ws.numel()),
                guarded_us=round(med["guarded"], 2), clipped_us=round(med["clipped"], 2),
                guarded_min_max_us=[round(min(us["guarded"]), 2), round(max(us["guarded"]), 2)],
                clipped_min_max_us=[round(min(us["clipped"]), 2), round(max(us["clipped"]), 2)],
                clip_us=round(extra, 2), overhead_pct=round(100.0 * extra / med["guarded"], 1),
                guarded_TBps=round(32.0 * total / med["guarded"] * 1e-6, 3), clipped_TBps=round(32.0 * total / med["clipped"] * 1e-6, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abl/clip_time.py needs a GPU: a timing taken anywhere else says nothing")
    sizes = goku_sizes(torch.device("cuda", 0))
    for mode in ("global", "per_array"):
        print(json.dumps(run("goku-default", sizes, mode, a.iters, a.rounds)), flush=True)
        print(json.dumps(run("one-array-2^26", [1 << 26], mode, max(a.iters // 10, 10), a.rounds)), flush=True)


if __name__ == "__main__":
    main()
