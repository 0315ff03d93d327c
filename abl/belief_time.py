"""What the second rule costs: the AdaBelief entry points (lde_adabelief_flux_step_dev / _guarded / _clipped) beside their ADAMW twins on
the same arrays, on the same box in the same run. The bytes are the same (28 per element in the update, the scans are the same kernels);
the rule has one more subtract and one more add per element — the expectation is level. Back-to-back C ABI calls between HIP events,
`--iters` calls a window after a warm-up; the two rules ALTERNATE window by window (`--rounds` windows each) and the median window counts,
so that whatever else shares the box falls on both alike. Shapes: (a) the parameter arrays of the default GOKU model (784 pixels:
launch-bound); (b) one array of 2²⁶ floats (HBM-bound). Each rule has arrays of its own (the state of one must not feed the other). The
clipped form runs in global mode with the threshold at half the gradient norm. One JSON line per shape and form. Recorded in DESIGN.md
§4.6, not gated.

    python abl/belief_time.py [--iters 200] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from latentdiffeq_amd import _lib as L  # noqa: E402

from clip_time import goku_sizes  # noqa: E402  (abl/ is this script's directory)

ADAMW_HP = (1e-3, 0.9, 0.999, 1e-8, 1e-10)
BELIEF_HP = (1e-3, 0.9, 0.999, 1e-16, 1e-16, 1e-10)


class Rule:
    def __init__(self, prefix, hp, sizes, dev):
        self.prefix, self.hp, self.n = prefix, hp, len(sizes)
        self.tab = (L.AdamTensor * self.n)()
        self.keep = []
        for i, k in enumerate(sizes):
            p, g, m, v = torch.randn(k, device=dev), torch.randn(k, device=dev) * 0.1, torch.zeros(k, device=dev), torch.zeros(k, device=dev)
            self.keep += [p, g, m, v]
            t = self.tab[i]
            t.p, t.g, t.m, t.v, t.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), k
        self.step = torch.zeros((), dtype=torch.int64, device=dev)
        self.words = torch.empty(L.GUARD_WORDS, dtype=torch.int64, device=dev)
        self.ws = torch.empty(max(int(L.load().lde_clip_ws_bytes(self.n, self.tab)), 8), dtype=torch.uint8, device=dev)
        self.norms = torch.zeros(self.n + 1, device=dev)
        self.s = L.raw_stream(0)
        self.clip = 0.5 * 0.1 * sum(sizes) ** 0.5
        L.call("lde_guard_init", None, L.ptr(self.words), self.s)

    def call(self, form):
        if form == "dev":
            L.call(self.prefix + "_dev", None, self.n, self.tab, *self.hp, L.ptr(self.step), self.s)
        elif form == "guarded":
            L.call(self.prefix + "_guarded", None, self.n, self.tab, *self.hp, L.ptr(self.step), L.ptr(self.words), self.s)
        else:
            L.call(self.prefix + "_clipped", None, self.n, self.tab, *self.hp, self.clip, L.CLIP_GLOBAL, L.ptr(self.step), L.ptr(self.words),
                   L.ptr(self.ws), L.ptr(self.norms), self.s)


def window(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def run(name, sizes, form, iters, rounds):
    dev = torch.device("cuda", 0)
    rules = {"adamw": Rule("lde_adamw_flux_step", ADAMW_HP, sizes, dev), "adabelief": Rule("lde_adabelief_flux_step", BELIEF_HP, sizes, dev)}
    for _ in range(10):
        for r in rules.values():
            r.call(form)
    torch.cuda.synchronize()
    us = {k: [] for k in rules}
    for _ in range(rounds):
        for k, r in rules.items():
            us[k].append(window(lambda: r.call(form), iters))
    for r in rules.values():
        assert int(r.step) == 10 + rounds * iters                                # every step was applied
        assert form == "dev" or r.words.tolist() == [-1, 0, 0, -1]
        assert all(bool(torch.isfinite(x).all()) for x in r.keep)
    med = {k: statistics.median(v) for k, v in us.items()}
    total = sum(sizes)
    return dict(shape=name, form=form, arrays=len(sizes), floats=total, iters=iters, rounds=rounds,
                adamw_us=round(med["adamw"], 2), adabelief_us=round(med["adabelief"], 2),
                adamw_min_max_us=[round(min(us["adamw"]), 2), round(max(us["adamw"]), 2)],
                adabelief_min_max_us=[round(min(us["adabelief"]), 2), round(max(us["adabelief"]), 2)],
                diff_us=round(med["adabelief"] - med["adamw"], 2), diff_pct=round(100.0 * (med["adabelief"] - med["adamw"]) / med["adamw"], 1),
                adabelief_update_TBps=round(28.0 * total / med["adabelief"] * 1e-6, 3) if form == "dev" else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abl/belief_time.py needs a GPU: a timing taken anywhere else says nothing")
    sizes = goku_sizes(torch.device("cuda", 0))
    for form in ("dev", "guarded", "clipped"):
        print(json.dumps(run("goku-default", sizes, form, a.iters, a.rounds)), flush=True)
        print(json.dumps(run("one-array-2^26", [1 << 26], form, max(a.iters // 10, 10), a.rounds)), flush=True)


if __name__ == "__main__":
    main()
