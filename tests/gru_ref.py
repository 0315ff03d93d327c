"""The GRU stack of the recurrent pattern extractor (LDE_CELL_GRU, include/lde.h) restated in numpy: what tests/test_gpu_gru.py compares
the kernels against, and what tests/test_gru_host.py checks against torch.nn.GRU in float64 and against its own finite differences.

Cell (Flux 0.13.6 GRUCell, "GRU v1"), gx = Wi·x, gh = Wh·h, row blocks (r, z, n):
    r = σ(gx₁ + gh₁ + b₁),  z = σ(gx₂ + gh₂ + b₂),  n = tanh(gx₃ + r ⊙ gh₃ + b₃),  h′ = (1 − z) ⊙ n + z ⊙ h
Flat weights per cell in Flux.destructure order: vec(Wi) [3h × in] column-major, vec(Wh) [3h × h], b [3h], state0 [h].
Layout: x (T, B, in); y (B, h_last) = the top cell's output after the last frame (reverse: frames fed T−1 … 0); every call starts from
state0. dtype = np.float64 or np.float32: every operation is carried out in that type."""
import numpy as np


def num_weights(sizes):
    return sum(3 * h * i + 3 * h * h + 3 * h + h for i, h in zip(sizes[:-1], sizes[1:]))


def pack(cells):
    """[(Wi [3h × in], Wh [3h × h], b [3h], state0 [h]), …] → the flat vector."""
    return np.concatenate([np.concatenate([Wi.T.reshape(-1), Wh.T.reshape(-1), b, s0]) for Wi, Wh, b, s0 in cells])


def unpack(W, sizes):
    cells, o = [], 0
    for i, h in zip(sizes[:-1], sizes[1:]):
        Wi = W[o:o + 3 * h * i].reshape(i, 3 * h).T; o += 3 * h * i
        Wh = W[o:o + 3 * h * h].reshape(h, 3 * h).T; o += 3 * h * h
        b = W[o:o + 3 * h]; o += 3 * h
        s0 = W[o:o + h]; o += h
        cells.append((Wi, Wh, b, s0))
    assert o == W.size
    return cells


def weights(sizes, seed=0, dtype=np.float32):
    """Flat weights in destructure order: U(±1/√fan_in) matrices, biases and initial states away from zero."""
    rng = np.random.default_rng(seed)
    cells = []
    for i, h in zip(sizes[:-1], sizes[1:]):
        cells.append((rng.uniform(-1, 1, (3 * h, i)) / np.sqrt(i), rng.uniform(-1, 1, (3 * h, h)) / np.sqrt(h),
                      rng.uniform(-0.3, 0.3, 3 * h), rng.uniform(-0.5, 0.5, h)))
    return pack(cells).astype(dtype)


def _sig(v):
    one = v.dtype.type(1)
    return one / (one + np.exp(-v))


def _sweep(sizes, W, x, reverse, dtype):
    W, x = np.asarray(W, dtype), np.asarray(x, dtype)
    cells = unpack(W, sizes)
    T, B, _ = x.shape
    one = dtype(1)
    hs = [np.broadcast_to(s0, (B, s0.size)).astype(dtype) for _, _, _, s0 in cells]
    tape = []
    for s in range(T):
        inp = x[T - 1 - s if reverse else s]
        step = []
        for l, (Wi, Wh, b, _) in enumerate(cells):
            h = sizes[l + 1]
            gx, gh = inp @ Wi.T, hs[l] @ Wh.T
            r = _sig(gx[:, :h] + gh[:, :h] + b[:h])
            z = _sig(gx[:, h:2 * h] + gh[:, h:2 * h] + b[h:2 * h])
            n = np.tanh(gx[:, 2 * h:] + r * gh[:, 2 * h:] + b[2 * h:])
            hn = (one - z) * n + z * hs[l]
            step.append((inp, hs[l], r, z, n, gh[:, 2 * h:]))
            hs[l] = hn
            inp = hn
        tape.append(step)
    return cells, tape, hs[-1]


def forward(sizes, W, x, reverse=False, dtype=np.float64):
    return _sweep(sizes, W, x, reverse, np.dtype(dtype).type)[2]


def backward(sizes, W, x, dy, reverse=False, dtype=np.float64):
    """(dx (T, B, in), dW flat) of Σ y·dy by hand-written back-propagation through time."""
    dtype = np.dtype(dtype).type
    cells, tape, _ = _sweep(sizes, W, x, reverse, dtype)
    x = np.asarray(x, dtype)
    T, B, _ = x.shape
    one = dtype(1)
    L = len(cells)
    dh = [np.zeros((B, h), dtype) for h in sizes[1:]]
    dh[-1] = np.asarray(dy, dtype).copy()
    g = [[np.zeros_like(Wi), np.zeros_like(Wh), np.zeros_like(b), None] for Wi, Wh, b, _ in cells]
    dx = np.zeros_like(x)
    for s in range(T - 1, -1, -1):
        for l in range(L - 1, -1, -1):
            Wi, Wh, _, _ = cells[l]
            inp, hp, r, z, n, gh3 = tape[s][l]
            d = dh[l]
            dn = d * (one - z) * (one - n * n)
            dz = d * (hp - n) * z * (one - z)
            dr = dn * gh3 * r * (one - r)
            di = np.concatenate([dr, dz, dn], axis=1)          # what Wi and b see
            dhh = np.concatenate([dr, dz, dn * r], axis=1)     # what Wh sees
            g[l][0] += di.T @ inp
            g[l][1] += dhh.T @ hp
            g[l][2] += di.sum(axis=0)
            dh[l] = d * z + dhh @ Wh
            din = di @ Wi
            if l > 0:
                dh[l - 1] = dh[l - 1] + din
            else:
                dx[T - 1 - s if reverse else s] = din
    for l in range(L):
        g[l][3] = dh[l].sum(axis=0)                            # what is left at step 0 goes to state0
    return dx, pack([tuple(c) for c in g]).astype(dtype)
