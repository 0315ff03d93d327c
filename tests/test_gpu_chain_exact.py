"""GPU: the dense chains, f32 and native bf16 (csrc/lde_chain_bf16.h), BIT FOR BIT at the tile, chunk and layout edges.

The tolerance legs (tests/test_gpu_chain.py, tests/test_gpu_chain_bf16.py) allow a share of the largest entry — in bf16 because a hidden
value on a rounding boundary may round the other way when the summation order differs — so one wrong ragged column, K-group tail or
64-row chunk of the weight gradient can pass them. Here the inputs are such that no rounding happens at all (tests/chain_exact_ref.py:
sparse weights from {±1, ±½}, small integers elsewhere, relu / identity; tests/test_chain_exact_ref.py holds every case to its
conditions on the CPU): the f32 kernels, the bf16 kernels and the float64 restatement must agree in every bit, whatever the summation
order, tile width, number of parts or layout. Every comparison is np.array_equal against the restatement cast to f32, for y, dx and dW,
in both dtypes on one handle, in the order f32, bf16, f32."""
import numpy as np
import pytest
import torch

from tests import chain_exact_ref as E

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16", "f32")


def _where_dW(sizes, idx):
    """flat weight index → (layer, "W", in-index, out-index) / (layer, "b", out-index)"""
    off = 0
    for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        if idx < off + i * o:
            return (l, "W", (idx - off) // o, (idx - off) % o)
        off += i * o
        if idx < off + o:
            return (l, "b", idx - off)
        off += o
    return None


class _Diffs:
    """Collects every mismatch of a case before failing: one GPU run then names all of them."""

    def __init__(self, case):
        self.case, self.sizes, self.bad = case, E.SPECS[case.spec][0], []

    def same(self, got, want, what, ctx):
        if got.shape == want.shape and np.array_equal(got, want):
            return
        if got.shape != want.shape:
            self.bad.append((ctx, what, "shape", got.shape, want.shape))
            return
        ne = np.argwhere(got != want)
        first = tuple(int(v) for v in ne[0])
        where = _where_dW(self.sizes, first[0]) if what == "dW" else first
        self.bad.append((ctx, what, f"{len(ne)} of {got.size} entries differ; first at {where}: got {got[first]!r}, want {want[first]!r}"))

    def check(self):
        assert not self.bad, (self.case, self.bad)


def _handle(case, options=()):
    from tests.gpu_util import NativeChain
    sizes, acts, skips, W, x, dy = E.case_inputs(case)
    ch = NativeChain(sizes, acts, skips)
    for k_, v_ in options:
        ch.set_option(k_, v_)
    ch.set_weights(W)
    return ch, x, dy


def _every_entry_point(ch, case, x, dy, d, ctx):
    """forward; the recomputing pullback; the training variant; the pullback without dx — each against the restatement of the case.
    x, dy and the forward output the pullbacks take live on the device once (the output IS the restatement's y when it is asserted)."""
    yr, dxr, dWr = E.reference(case)
    xd, dyd, yd = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x, dy, np.array(yr)))
    d.same(ch.forward(xd), yr, "y", ctx + " forward")
    dx, dW = ch.backward(xd, yd, dyd)
    d.same(dx, dxr, "dx", ctx + " backward")
    d.same(dW, dWr, "dW", ctx + " backward")
    ys, saved = ch.forward_save(xd)
    d.same(ys, yr, "y", ctx + " forward_save")
    dx, dW = ch.backward_saved(xd, yd, dyd, saved)
    d.same(dx, dxr, "dx", ctx + " backward_saved")
    d.same(dW, dWr, "dW", ctx + " backward_saved")
    dx, dW = ch.backward(xd, yd, dyd, need_dx=False)
    assert dx is None
    d.same(dW, dWr, "dW", ctx + " backward(need_dx=False)")


@pytest.mark.parametrize("case", E.cases("edge"), ids=lambda c: f"{c.spec}-{c.N}")
def test_every_tile_and_chunk_edge(case):
    """(a) Every spec at N = 1, 15 … 17, 31 … 33, 63 … 65, 127 … 129: one tile with almost every column beyond N, each column-tile
    width's boundary (16·cg columns, cg = 1, 2, 4), the weight gradient's 64-row chunks (65, 127, 129: 2 – 3 chunks, parts > 1 with a
    ragged last chunk for the specs with few jobs), and for the wide-input chains N < 16·cgx, the fall-back to the panel layout."""
    ch, x, dy = _handle(case)
    d = _Diffs(case)
    for i, dtype in enumerate(DTYPES):
        ch.set_dtype(dtype)
        _every_entry_point(ch, case, x, dy, d, f"{dtype}#{i}")
    d.check()


@pytest.mark.parametrize("case", E.cases("switch"), ids=lambda c: f"{c.spec}-{c.N}")
def test_either_side_of_the_tile_width_switches(case):
    """(b) lde_host.h: chain_tile_pick takes, per handle, the widest tile (candidates: 64, 32, 16 columns for the f32 forward; 32, 16 for
    the f32 pullback and for bf16) whose chain_lds_bytes fit HALF the 160 KiB LDS = 81 920 bytes, else the widest that fits at all;
    chain_narrow halves that width per call while the grid has fewer than 192 tiles. A width w serves N ≥ 191·w + 1.

    reconstructor 2-200-200-200-784 (panel strides ld0 = 40, ldh = ldg = 232 floats, ldb = 272 bf16, 1 384 biases, a third bf16 panel):
      f32 forward   64 col: 134 560 B, 32 col: 70 048 B → 32;   f32 pullback 32 col: 99 744 B, 16 col: 52 640 B → 16
      bf16 forward  32 col: 57 760 B → 32;                       bf16 pullback 32 col: 64 512 B → 32
    feature_extractor 784-200-200-200-32, x read in place (aligned x, N ≥ one tile; ldh = ldg = 232, ldb = 272, 632 biases, 9 216 B of
    chunk buffers per column group in the bf16 forward):
      f32 forward   64 col: 121 312 B, 32 col: 61 920 B → 32;   f32 pullback 32 col: 91 616 B, 16 col: 47 072 B → 16
      bf16 forward  32 col: 73 184 B → 32;                       bf16 pullback 32 col: 64 512 B → 32
      (its panel layout, ld0 = 808 / ldb = 848, fits 16 columns only — 83 936, 98 784, 83 936, 69 120 B: legs (a) and (c))
    So for BOTH chains every kernel but the f32 pullback switches between N = 6 112 (191 tiles of 32 → 382 full tiles of 16) and
    N = 6 113 (192 tiles of 32, the last holding ONE column); the f32 pullback runs 16-column tiles throughout (6 113 and 12 225: a last
    tile of one column). Neither chain's f32 forward takes 64 columns, so for them 12 224 / 12 225 is no switch of width but 382 full
    32-column tiles against 383 with one column in the last (and 191 / 192 chunks of the bf16 weight gradient, 12 225 = 191·64 + 1).
    The 64 → 32 switch of the f32 forward at 12 224 / 12 225 belongs to narrow chains: `one` (24-10; ld0 = ldh = 40, 12 biases:
    64 col 30 768 B → 64) runs 32-column tiles at 12 224 and 64-column tiles at 12 225, the last with one column — hence its two cases."""
    ch, x, dy = _handle(case)
    d = _Diffs(case)
    for i, dtype in enumerate(DTYPES):
        ch.set_dtype(dtype)
        _every_entry_point(ch, case, x, dy, d, f"{dtype}#{i}")
    d.check()


@pytest.mark.parametrize("spec", E.WIDE_INPUT)
@pytest.mark.parametrize("N", [17, 64, 129])
def test_layout_fallbacks_of_the_wide_input_chains(spec, N):
    """(c) chain_call_choice: a wide-input chain reads x in place only when x is 16-byte aligned and N fills a tile; an x one float
    past a 16-byte boundary, and lde_chain_set_option("gx", 0), take the layout with an input panel. Same bits as the aligned call in
    the default layout — which are the restatement's (N = 15, 17, 31 of leg (a): the N < 16·cgx fall-back)."""
    case = E.case("edge", spec, N)
    yr, dxr, dWr = E.reference(case)
    ch, x, dy = _handle(case)
    panel, _, _ = _handle(case, options=(("gx", 0),))
    d = _Diffs(case)
    for i, dtype in enumerate(DTYPES):
        ch.set_dtype(dtype)
        panel.set_dtype(dtype)
        y0 = ch.forward(x)
        dx0, dW0 = ch.backward(x, y0, dy)
        for what, got, want in (("y", y0, yr), ("dx", dx0, dxr), ("dW", dW0, dWr)):
            d.same(got, want, what, f"{dtype}#{i} aligned")
        for ctx, h, off in ((f"{dtype}#{i} x one float past 16 bytes", ch, 1), (f"{dtype}#{i} gx=0", panel, 0)):
            y = h.forward(x, x_offset=off)
            d.same(y, y0, "y", ctx + " forward")
            for name, (dx, dW) in (("backward", h.backward(x, y0, dy, x_offset=off)),
                                   ("backward_saved", h.backward_saved(x, y0, dy, h.forward_save(x, x_offset=off)[1], x_offset=off))):
                d.same(dx, dx0, "dx", f"{ctx} {name}")
                d.same(dW, dW0, "dW", f"{ctx} {name}")
    d.check()


@pytest.mark.parametrize("spec", sorted(E.SPECS))
@pytest.mark.parametrize("N", [17, 129])
def test_weight_gradient_accumulates_exactly(spec, N):
    """(d) dW += gradient onto a table of small integers: dW0 + the restatement's dW, exactly (tests/test_chain_exact_ref.py: every
    partial sum stays exact with |dW0| ≤ 3 on top), from both pullbacks in both dtypes; and the same call twice gives the same bits."""
    case = E.case("edge", spec, N)
    yr, dxr, dWr = E.reference(case)
    yr = np.array(yr)
    ch, x, dy = _handle(case)
    dW0 = E.accumulation_base(case)
    want64 = dW0.astype(np.float64) + dWr.astype(np.float64)
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64)
    d = _Diffs(case)
    for i, dtype in enumerate(DTYPES):
        ch.set_dtype(dtype)
        _, saved = ch.forward_save(x)
        for rep in range(2):
            dx, dW = ch.backward(x, yr, dy, dW0=dW0)
            d.same(dx, dxr, "dx", f"{dtype}#{i} backward onto dW0, call {rep}")
            d.same(dW, want, "dW", f"{dtype}#{i} backward onto dW0, call {rep}")
            dx, dW = ch.backward_saved(x, yr, dy, saved, need_dx=False, dW0=dW0)
            d.same(dW, want, "dW", f"{dtype}#{i} backward_saved onto dW0, call {rep}")
    d.check()


@pytest.mark.parametrize("spec", E.WALK_SPECS)
def test_one_handle_over_changing_column_counts(spec):
    """(e) One handle walks N = 129 → 6 113 → 17 → 1 → 64 → 6 112 with a fresh draw of weights and data per call (its own seed): the δ
    workspace, the saved-activation scratch of the recomputing bf16 pullback and the slab keep rows of the larger call, none of which
    may reach a result. At every N both dtypes run (their order alternates from N to N), each with the recomputing and the
    saved-activation pullback (their order alternates too); every call against the restatement of ITS inputs."""
    from tests.gpu_util import NativeChain
    sizes, acts, skips = E.SPECS[spec]
    ch = NativeChain(sizes, acts, skips)
    bad = []
    for i, N in enumerate(E.WALK_N):
        case = E.case("walk", spec, N)
        _, _, _, W, x, dy = E.case_inputs(case)
        yr, dxr, dWr = E.reference(case)
        d = _Diffs(case)
        ch.set_weights(W)
        xd, dyd, yd = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x, dy, np.array(yr)))
        for dtype in (("f32", "bf16"), ("bf16", "f32"))[i % 2]:
            ch.set_dtype(dtype)
            for variant in (("plain", "saved"), ("saved", "plain"))[(i // 2) % 2]:
                ctx = f"call {i} N={N} {dtype} {variant}"
                if variant == "plain":
                    d.same(ch.forward(xd), yr, "y", ctx)
                    dx, dW = ch.backward(xd, yd, dyd)
                else:
                    ys, saved = ch.forward_save(xd)
                    d.same(ys, yr, "y", ctx)
                    dx, dW = ch.backward_saved(xd, yd, dyd, saved)
                d.same(dx, dxr, "dx", ctx)
                d.same(dW, dWr, "dW", ctx)
        bad += d.bad
    assert not bad, (spec, bad)
