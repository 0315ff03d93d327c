"""The float64 restatement of the dense chains (f32 and native-bf16 arithmetic, csrc/lde_chain_bf16.h) and the EXACT-INPUT cases of
tests/test_gpu_chain_exact.py.

Exact inputs: weights with k non-zeros per row drawn from {±1, ±½}, biases from {−1, 0, 1}, x from {−2 … 2}, dy from {−2 … 2}·2⁻¹⁰,
relu / identity activations. Every product is then exact, every partial sum a small multiple of a power of two, and — this is what
`conditions` checks per case, on the restatement alone — every value the bf16 mode stores has 8 significant bits. The f32 kernels, the
bf16 kernels and the restatement must then agree bit for bit whatever the summation order, tile width, split or layout.

A plain module (no tests): tests/test_chain_exact_ref.py holds the table to its conditions on the CPU, tests/test_gpu_chain_exact.py
runs it on the GPU, tests/test_gpu_chain_bf16.py takes `chain_ref` for its tolerance legs."""
import functools
from typing import NamedTuple

import numpy as np

from latentdiffeq_amd import _lib as L


def bf16r(a):
    """float32 → nearest bfloat16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def identity(a):
    return a


def _act(kind, x):
    if kind == L.CACT_RELU:
        return np.maximum(x, 0)
    if kind == L.CACT_TANH:
        return np.tanh(x)
    if kind == L.CACT_SIGMOID:
        return 1 / (1 + np.exp(-x))
    if kind == L.CACT_SOFTPLUS:
        return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
    return x


def _act_grad_out(kind, f):
    if kind == L.CACT_RELU:
        return (f > 0).astype(f.dtype)
    if kind == L.CACT_TANH:
        return 1 - f * f
    if kind == L.CACT_SIGMOID:
        return f * (1 - f)
    if kind == L.CACT_SOFTPLUS:
        return 1 - np.exp(-f)
    return np.ones_like(f)


def _split(sizes, W):
    out, off = [], 0
    for i, o in zip(sizes[:-1], sizes[1:]):
        Wl = W[off:off + i * o].reshape(i, o).T          # vec(W) column-major [out×in]
        off += i * o
        out.append((Wl, W[off:off + o]))
        off += o
    return out


KGROUP = 32          # K-group of the bf16 products (v_mfma_f32_16x16x32_bf16)


def chain_ref_full(sizes, acts, skips, W, x, dy, rnd, fault=None):
    """x (N, in), dy (N, out) → y, dx, dW of the mode `rnd` defines (identity: the f32 chain; bf16r: the native bf16 mode of
    csrc/lde_chain_bf16.h): both operands of every product are `rnd`-ed, and the hidden activations, the activation before a skip
    addition and δ are STORED `rnd`-ed; biases, the gradient that flows around a skip connection, y, dx and dW are f32.

    Returns a dict: y, dx, dW; a[l] = the input of layer l as the products read it [in_l × N]; delta[l] = δ_l as stored [out_l × N];
    stored = every array the bf16 mode keeps in bf16, BEFORE its rounding (hidden activations, the activation before a skip addition,
    δ); products = (A, B) of every matrix product A·B that is formed.

    `fault` restates one kernel mistake, for the tests that show that the exact-input legs would see it:
    ("dw_row", l): layer l's weight-gradient product without its last row n; ("kgroup",): every product over K = 784 (the feature
    extractor's first layer, the reconstructor's last input-gradient product) without its last K-group, k ≥ 768; ("dx_col",): column
    N − 1 of dx left zero."""
    layers = _split(sizes, W.astype(np.float64))
    L_ = len(layers)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    r64 = lambda a: rnd(a).astype(np.float64)
    kcut = lambda K: (K // KGROUP) * KGROUP if (fault == ("kgroup",) and K == 784) else K
    stored, products = [], []
    h = [x.astype(np.float64).T]
    f = []
    for l, ((Wl, bl), a, s) in enumerate(zip(layers, acts, skips)):
        A, B = r64(Wl), r64(h[-1])
        kc = kcut(A.shape[1])
        products.append((A, B))
        pre = A[:, :kc] @ B[:kc] + bl[:, None]
        fl = f32(_act(a, pre))                                        # the epilogue's f32 value
        if l == L_ - 1:
            f.append(fl)
            h.append(fl)                                               # y stays f32
        else:
            stored.append(fl)
            f.append(r64(fl))                                          # stored: what the activation derivative is taken from
            hn = f32(r64(h[-1]) + fl) if s else fl
            stored.append(hn)
            h.append(r64(hn))
    G = dy.astype(np.float64).T
    dW, delta = [], [None] * L_
    for l in range(L_ - 1, -1, -1):
        Wl, _ = layers[l]
        d0 = f32(G * _act_grad_out(acts[l], f[l]))
        stored.append(d0)
        d = r64(d0)                                                    # δ_l as stored
        delta[l] = d
        hl = r64(h[l])
        products.append((d, hl.T))
        nc = d.shape[1] - 1 if fault == ("dw_row", l) else d.shape[1]
        gW = d[:, :nc] @ hl[:, :nc].T
        dW = [gW.T.reshape(-1), d.sum(axis=1)] + dW
        A = r64(Wl.T)
        kc = kcut(A.shape[1])
        products.append((A, d))
        G = A[:, :kc] @ d[:kc] + (G if skips[l] else 0)
    dx = G.T.copy()
    if fault == ("dx_col",):
        dx[-1] = 0
    return dict(y=h[-1].T, dx=dx, dW=np.concatenate(dW), a=[r64(v) for v in h[:-1]], delta=delta, stored=stored, products=products)


def chain_ref(sizes, acts, skips, W, x, dy, rnd):
    """y, dx, dW of `chain_ref_full`."""
    r = chain_ref_full(sizes, acts, skips, W, x, dy, rnd)
    return r["y"], r["dx"], r["dW"]


# ---- the exact-input cases -------------------------------------------------------------------------------------------------------------
R, I = L.CACT_RELU, L.CACT_IDENTITY
SPECS = {
    "reconstructor": ((2, 200, 200, 200, 784), (R, R, R, I), (0, 1, 1, 0)),        # the decoder; two skip layers; dw<4>
    "feature_extractor": ((784, 200, 200, 200, 32), (R, R, R, R), (0, 1, 1, 0)),   # x read in place in chunks; 784 = 24·32 + 16
    "one": ((24, 10), (I,), (0,)),                                                 # single layer; last-layer δ row width pad32
    "one_wide": ((256, 24), (R,), (0,)),                                           # single layer, x in place
    "odd": ((5, 33, 33, 7, 7, 19), (R, R, I, R, I), (0, 1, 0, 1, 0)),              # widths % 8 ≠ 0; skips at odd widths
    "ndw2": ((40, 100, 100, 12), (R, R, I), (0, 1, 0)),                            # 4·4 = 16 tiles: k_chain_dw_b<2>, k_mlp_dw<2>
    "wide": ((32, 512, 512, 40), (R, R, I), (0, 1, 0)),                            # the widest panels; jobs cut along the longer side
}
WIDE_INPUT = ("feature_extractor", "one_wide")           # the chains whose x can be read in place (in % 16 == 0, in ≥ 128)
EDGE_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SWITCH_N = (6112, 6113, 12224, 12225)
WALK_N = (129, 6113, 17, 1, 64, 6112)
WALK_SPECS = ("reconstructor", "feature_extractor", "ndw2")


class Case(NamedTuple):
    leg: str          # "edge" (a; also the inputs of c and d), "switch" (b), "walk" (e)
    spec: str
    N: int
    k: int
    seed: int


def exact_inputs(sizes, N, seed, k):
    """W (flat, Flux.destructure order), x (N, in), dy (N, out), float32. Every row of every weight matrix holds min(k, in) non-zeros
    at random places from {±1, ±½}; biases from {−1, 0, 1}; x from {−2 … 2}; dy from {−2 … 2}·2⁻¹⁰. A row of x or dy that came out all
    zero gets one entry set to 1 (·2⁻¹⁰), so that every column n takes part in every product. W depends on (sizes, seed, k) alone."""
    rw = np.random.default_rng([seed, 0])
    flat = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        kk = min(k, i)
        Wl = np.zeros((o, i))
        cols = np.argsort(rw.random((o, i)), axis=1)[:, :kk]
        np.put_along_axis(Wl, cols, rw.choice([1.0, -1.0, 0.5, -0.5], (o, kk)), axis=1)
        flat += [Wl.T.reshape(-1), rw.integers(-1, 2, o).astype(np.float64)]
    rx = np.random.default_rng([seed, 1, N])
    x = rx.integers(-2, 3, (N, sizes[0])).astype(np.float64)
    dy = rx.integers(-2, 3, (N, sizes[-1])).astype(np.float64)
    for a in (x, dy):
        z = np.flatnonzero(~a.any(axis=1))
        a[z, z % a.shape[1]] = 1.0
    return np.concatenate(flat).astype(np.float32), x.astype(np.float32), (dy * 2.0 ** -10).astype(np.float32)


def case_inputs(case):
    sizes, acts, skips = SPECS[case.spec]
    return (sizes, acts, skips) + exact_inputs(sizes, case.N, case.seed, case.k)


@functools.lru_cache(maxsize=4)
def reference(case):
    """(y, dx, dW) of the case: the float64 restatement (no rounding) cast to float32. Shared by the tests of one case; read-only."""
    sizes, acts, skips, W, x, dy = case_inputs(case)
    out = tuple(np.ascontiguousarray(v, np.float32) for v in chain_ref(sizes, acts, skips, W, x, dy, identity))
    for v in out:
        v.setflags(write=False)
    return out


def _grain(a):
    """The largest power of two that divides every entry of `a` (dyadic rationals well inside float64)."""
    s = np.abs(a[a != 0]) * 2.0 ** 40
    if s.size == 0:
        return 1.0
    i = s.astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s), "entries finer than 2⁻⁴⁰"
    g = int(np.bitwise_or.reduce(i.reshape(-1)))
    return float(g & -g) * 2.0 ** -40


def conditions(case):
    """What makes the case a fair and non-vacuous bit-for-bit test, from the restatement alone:
    exact — y, dx and dW agree entry for entry between bf16 rounding, no rounding, and the result cast to f32 and back;
    order_free — for every matrix product, Σ|terms| of every entry is below 2²⁴ grains of its terms (the grain: the power of two
      that divides every term), so every partial sum, in ANY order and grouping, is an integer number of grains an f32 holds exactly;
    storable — every hidden activation, activation before a skip addition and δ equals its bf16 rounding;
    contributes — every column n has a non-zero entry in row n of y and of dx and, for every layer l, in a_l[:, n] and δ_l[:, n]:
      dropping a row n from any layer's weight-gradient product then changes dW."""
    sizes, acts, skips, W, x, dy = case_inputs(case)
    rb = chain_ref_full(sizes, acts, skips, W, x, dy, bf16r)
    ri = chain_ref_full(sizes, acts, skips, W, x, dy, identity)
    exact = all(np.array_equal(rb[q], ri[q]) and np.array_equal(ri[q].astype(np.float32).astype(np.float64), ri[q]) for q in ("y", "dx", "dW"))
    order_free = True
    for A, B in ri["products"]:
        grains = (np.abs(A) @ np.abs(B)).max() / (_grain(A) * _grain(B))
        order_free = order_free and grains < 2.0 ** 24
    storable = all(np.array_equal(bf16r(v.astype(np.float32)).astype(np.float64), v) for v in ri["stored"])
    cols = [ri["y"].T, ri["dx"].T] + ri["a"] + ri["delta"]
    contributes = all(bool((v != 0).any(axis=0).all()) for v in cols)
    return dict(exact=bool(exact), order_free=bool(order_free), storable=bool(storable), contributes=contributes)


ACC_MAX = 3          # |entries| of the table a pullback accumulates onto


def accumulation_base(case):
    """The table of small integers (−3 … 3, float32) the accumulating pullbacks of the case start from."""
    sizes = SPECS[case.spec][0]
    n = sum(i * o + o for i, o in zip(sizes[:-1], sizes[1:]))
    return np.random.default_rng([case.seed, 2, case.N]).integers(-ACC_MAX, ACC_MAX + 1, n).astype(np.float32)


def accumulation_is_exact(case):
    """dW0 + dW with every partial sum exact wherever dW0 enters the sum: (ACC_MAX + Σ|terms|) of every weight-gradient entry stays
    below 2²⁴ grains (the grain of the terms also divides the integers of dW0)."""
    sizes, acts, skips, W, x, dy = case_inputs(case)
    r = chain_ref_full(sizes, acts, skips, W, x, dy, identity)
    ok = True
    for d, a in zip(r["delta"], r["a"]):
        grain = min(_grain(d) * _grain(a), _grain(d), 1.0)           # weight entries, bias sums, the integers
        ok = ok and (ACC_MAX + max((np.abs(d) @ np.abs(a).T).max(), np.abs(d).sum(axis=1).max())) / grain < 2.0 ** 24
    return bool(ok)


# (k, seed) per case, found by tests/test_chain_exact_ref.py's conditions (the smallest seed that holds them, k = 3 before k = 2). A pair
# that fails a condition is replaced HERE, never excused at run time.
TABLE = (
    Case("edge", "reconstructor", 1, 3, 2),
    Case("edge", "reconstructor", 15, 3, 1),
    Case("edge", "reconstructor", 16, 3, 1),
    Case("edge", "reconstructor", 17, 3, 1),
    Case("edge", "reconstructor", 31, 3, 1),
    Case("edge", "reconstructor", 32, 3, 4),
    Case("edge", "reconstructor", 33, 3, 1),
    Case("edge", "reconstructor", 63, 3, 2),
    Case("edge", "reconstructor", 64, 3, 3),
    Case("edge", "reconstructor", 65, 3, 2),
    Case("edge", "reconstructor", 127, 3, 1),
    Case("edge", "reconstructor", 128, 3, 2),
    Case("edge", "reconstructor", 129, 3, 1),
    Case("edge", "feature_extractor", 1, 3, 1),
    Case("edge", "feature_extractor", 15, 3, 1),
    Case("edge", "feature_extractor", 16, 3, 1),
    Case("edge", "feature_extractor", 17, 3, 1),
    Case("edge", "feature_extractor", 31, 3, 1),
    Case("edge", "feature_extractor", 32, 3, 1),
    Case("edge", "feature_extractor", 33, 3, 1),
    Case("edge", "feature_extractor", 63, 3, 1),
    Case("edge", "feature_extractor", 64, 3, 1),
    Case("edge", "feature_extractor", 65, 3, 1),
    Case("edge", "feature_extractor", 127, 3, 1),
    Case("edge", "feature_extractor", 128, 3, 1),
    Case("edge", "feature_extractor", 129, 3, 1),
    Case("edge", "one", 1, 3, 1),
    Case("edge", "one", 15, 3, 1),
    Case("edge", "one", 16, 3, 1),
    Case("edge", "one", 17, 3, 1),
    Case("edge", "one", 31, 3, 1),
    Case("edge", "one", 32, 3, 1),
    Case("edge", "one", 33, 3, 1),
    Case("edge", "one", 63, 3, 1),
    Case("edge", "one", 64, 3, 1),
    Case("edge", "one", 65, 3, 1),
    Case("edge", "one", 127, 3, 1),
    Case("edge", "one", 128, 3, 1),
    Case("edge", "one", 129, 3, 1),
    Case("edge", "one_wide", 1, 3, 1),
    Case("edge", "one_wide", 15, 3, 1),
    Case("edge", "one_wide", 16, 3, 1),
    Case("edge", "one_wide", 17, 3, 1),
    Case("edge", "one_wide", 31, 3, 1),
    Case("edge", "one_wide", 32, 3, 1),
    Case("edge", "one_wide", 33, 3, 1),
    Case("edge", "one_wide", 63, 3, 1),
    Case("edge", "one_wide", 64, 3, 1),
    Case("edge", "one_wide", 65, 3, 1),
    Case("edge", "one_wide", 127, 3, 1),
    Case("edge", "one_wide", 128, 3, 1),
    Case("edge", "one_wide", 129, 3, 1),
    Case("edge", "odd", 1, 3, 1),
    Case("edge", "odd", 15, 3, 1),
    Case("edge", "odd", 16, 3, 1),
    Case("edge", "odd", 17, 3, 2),
    Case("edge", "odd", 31, 3, 1),
    Case("edge", "odd", 32, 3, 1),
    Case("edge", "odd", 33, 3, 1),
    Case("edge", "odd", 63, 3, 1),
    Case("edge", "odd", 64, 3, 1),
    Case("edge", "odd", 65, 3, 1),
    Case("edge", "odd", 127, 3, 1),
    Case("edge", "odd", 128, 3, 3),
    Case("edge", "odd", 129, 3, 7),
    Case("edge", "ndw2", 1, 3, 1),
    Case("edge", "ndw2", 15, 3, 1),
    Case("edge", "ndw2", 16, 3, 1),
    Case("edge", "ndw2", 17, 3, 1),
    Case("edge", "ndw2", 31, 3, 1),
    Case("edge", "ndw2", 32, 3, 1),
    Case("edge", "ndw2", 33, 3, 1),
    Case("edge", "ndw2", 63, 3, 1),
    Case("edge", "ndw2", 64, 3, 1),
    Case("edge", "ndw2", 65, 3, 1),
    Case("edge", "ndw2", 127, 3, 1),
    Case("edge", "ndw2", 128, 3, 1),
    Case("edge", "ndw2", 129, 3, 1),
    Case("edge", "wide", 1, 3, 1),
    Case("edge", "wide", 15, 3, 1),
    Case("edge", "wide", 16, 3, 1),
    Case("edge", "wide", 17, 3, 1),
    Case("edge", "wide", 31, 3, 1),
    Case("edge", "wide", 32, 3, 1),
    Case("edge", "wide", 33, 3, 1),
    Case("edge", "wide", 63, 3, 1),
    Case("edge", "wide", 64, 3, 1),
    Case("edge", "wide", 65, 3, 1),
    Case("edge", "wide", 127, 3, 1),
    Case("edge", "wide", 128, 3, 1),
    Case("edge", "wide", 129, 3, 1),
    Case("switch", "reconstructor", 6112, 2, 3),
    Case("switch", "reconstructor", 6113, 2, 2),
    Case("switch", "reconstructor", 12224, 2, 2),
    Case("switch", "reconstructor", 12225, 2, 3),
    Case("switch", "feature_extractor", 6112, 3, 1),
    Case("switch", "feature_extractor", 6113, 3, 1),
    Case("switch", "feature_extractor", 12224, 3, 1),
    Case("switch", "feature_extractor", 12225, 3, 1),
    Case("switch", "one", 12224, 3, 1),
    Case("switch", "one", 12225, 3, 1),
    Case("walk", "reconstructor", 129, 3, 104),
    Case("walk", "reconstructor", 6113, 2, 111),
    Case("walk", "reconstructor", 17, 3, 121),
    Case("walk", "reconstructor", 1, 3, 131),
    Case("walk", "reconstructor", 64, 3, 141),
    Case("walk", "reconstructor", 6112, 2, 151),
    Case("walk", "feature_extractor", 129, 3, 101),
    Case("walk", "feature_extractor", 6113, 3, 111),
    Case("walk", "feature_extractor", 17, 3, 121),
    Case("walk", "feature_extractor", 1, 3, 131),
    Case("walk", "feature_extractor", 64, 3, 141),
    Case("walk", "feature_extractor", 6112, 3, 151),
    Case("walk", "ndw2", 129, 3, 101),
    Case("walk", "ndw2", 6113, 3, 111),
    Case("walk", "ndw2", 17, 3, 121),
    Case("walk", "ndw2", 1, 3, 131),
    Case("walk", "ndw2", 64, 3, 141),
    Case("walk", "ndw2", 6112, 3, 151),
)


def cases(leg, spec=None):
    return [c for c in TABLE if c.leg == leg and (spec is None or c.spec == spec)]


def case(leg, spec, N):
    (c,) = [c for c in TABLE if (c.leg, c.spec, c.N) == (leg, spec, N)]
    return c
