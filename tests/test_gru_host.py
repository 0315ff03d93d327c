"""CPU: the GRU cell of the recurrent pattern extractor (LDE_CELL_GRU, include/lde.h) without a GPU — (1) the weight count and which
descriptions the built library accepts; (2) the numpy restatement the GPU tests compare against (tests/gru_ref.py): against torch.nn.GRU
in float64, its gradients against central differences of its own values, its f32 mode against its f64 mode; (3) the Python tags;
(4) the pure part of the plan in csrc/lde_host.h under AddressSanitizer + UndefinedBehaviorSanitizer (tests/gru_host_driver.cpp, run as
a program)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gru_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STACKS = [(32, 16, 16), (5, 7, 3, 9), (3, 10), (40, 21, 11), (40, 22), (32, 32, 32), (16, 64), (256, 64, 64, 64, 64), (1, 1)]


def _desc(cell, sizes, reverse=False):
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    d = L.RnnDesc()
    d.abi_version, d.cell, d.n_layers, d.reverse = L.LDE_ABI_VERSION, cell, len(sizes) - 1, int(reverse)
    for i, s in enumerate(sizes):
        d.sizes[i] = s
    return lib, d


def _formula(sizes):
    return sum(3 * h * i + 3 * h * h + 3 * h + h for i, h in zip(sizes[:-1], sizes[1:]))


def test_num_weights_of_gru_descriptions():
    for sizes in STACKS:
        lib, d = _desc(3, sizes)
        assert lib.lde_rnn_num_weights(C.byref(d)) == _formula(sizes) == G.num_weights(sizes), sizes
    # the other kinds count what they counted
    lib, d = _desc(2, (32, 16, 16))
    assert lib.lde_rnn_num_weights(C.byref(d)) == 4 * 16 * 32 + 4 * 16 * 16 + 4 * 16 + 2 * 16 + 2 * 4 * 16 * 16 + 4 * 16 + 2 * 16
    lib, d = _desc(0, (32, 16, 16))
    assert lib.lde_rnn_num_weights(C.byref(d)) == 16 * 32 + 16 * 16 + 16 + 16 + 2 * 16 * 16 + 16 + 16


def test_create_accepts_gru_and_refuses_unknown_kinds():
    for sizes in [(32, 16, 16), (5, 7, 3, 9), (3, 10), (32, 32, 32), (16, 64)]:
        lib, d = _desc(3, sizes, reverse=True)
        h = C.c_void_p()
        rc = lib.lde_rnn_create(C.byref(d), C.byref(h))
        assert rc in (0, -3), (sizes, rc)          # LDE_OK with a GPU, LDE_ERR_NO_DEVICE without: never an argument error
        if rc == 0:
            lib.lde_rnn_destroy(h)
    for cell in (4, -1, 7):
        lib, d = _desc(cell, (8, 8))
        h = C.c_void_p()
        assert lib.lde_rnn_create(C.byref(d), C.byref(h)) == -1 and not h.value, cell      # LDE_ERR_INVALID_ARG
        assert lib.lde_rnn_num_weights(C.byref(d)) == -1, cell


def _torch_gru(sizes, W, x, dy, reverse):
    """The stack as torch.nn.GRU cells in float64: weight_ih = Wi, weight_hh = Wh, bias_ih = b, bias_hh = 0 (the reset gate then multiplies
    Wh₃·h alone), gate order (r, z, n), state0 as h0. Returns y, dx, flat dW."""
    import torch
    cells = G.unpack(np.asarray(W, np.float64), sizes)
    T, B, _ = x.shape
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    seq = torch.flip(xt, dims=[0]) if reverse else xt
    mods, h0s = [], []
    for (Wi, Wh, b, s0), i, h in zip(cells, sizes[:-1], sizes[1:]):
        m = torch.nn.GRU(i, h, dtype=torch.float64)
        with torch.no_grad():
            m.weight_ih_l0.copy_(torch.tensor(np.ascontiguousarray(Wi)))
            m.weight_hh_l0.copy_(torch.tensor(np.ascontiguousarray(Wh)))
            m.bias_ih_l0.copy_(torch.tensor(np.ascontiguousarray(b)))
            m.bias_hh_l0.zero_()
        h0 = torch.tensor(np.ascontiguousarray(s0), dtype=torch.float64, requires_grad=True)
        seq, _ = m(seq, h0.unsqueeze(0).expand(B, h).unsqueeze(0).contiguous())
        mods.append(m)
        h0s.append(h0)
    y = seq[-1]
    (y * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    dW = G.pack([(m.weight_ih_l0.grad.numpy(), m.weight_hh_l0.grad.numpy(), m.bias_ih_l0.grad.numpy(), h0.grad.numpy()) for m, h0 in zip(mods, h0s)])
    return y.detach().numpy(), xt.grad.numpy(), dW


@pytest.mark.parametrize("sizes,reverse,T,B", [((32, 16, 16), True, 9, 37), ((5, 7, 3, 9), False, 9, 37), ((3, 10), False, 1, 1)])
def test_reference_equals_torch_gru_in_float64(sizes, reverse, T, B):
    rng = np.random.default_rng(11)
    W = G.weights(sizes, seed=2, dtype=np.float64)
    x = rng.standard_normal((T, B, sizes[0]))
    dy = rng.standard_normal((B, sizes[-1])) / B
    y = G.forward(sizes, W, x, reverse)
    dx, dW = G.backward(sizes, W, x, dy, reverse)
    ty, tdx, tdW = _torch_gru(sizes, W, x, dy, reverse)
    errs = [np.abs(a - b).max() for a, b in ((y, ty), (dx, tdx), (dW, tdW))]
    print(f"{sizes}: y {errs[0]:.2e} dx {errs[1]:.2e} dW {errs[2]:.2e}")
    assert max(errs) <= 1e-12, errs


def test_reference_gradients_are_the_finite_differences_of_its_values():
    """A small stack in f64: central differences of Σ y·dy in every weight and a sample of the inputs, to 1e-7 of the largest gradient entry
    (step 1e-6: truncation ≈ 1e-12·|f‴|, round-off ≈ 1e-16/1e-6 = 1e-10)."""
    sizes, T, B = (4, 5, 3), 6, 3
    rng = np.random.default_rng(5)
    W = G.weights(sizes, seed=1, dtype=np.float64)
    x = rng.standard_normal((T, B, sizes[0]))
    dy = rng.standard_normal((B, sizes[-1]))
    for reverse in (False, True):
        dx, dW = G.backward(sizes, W, x, dy, reverse)
        f = lambda Wv, xv: float((G.forward(sizes, Wv, xv, reverse) * dy).sum())
        eps = 1e-6
        fdW = np.zeros_like(W)
        for i in range(W.size):
            e = np.zeros_like(W); e[i] = eps
            fdW[i] = (f(W + e, x) - f(W - e, x)) / (2 * eps)
        fdx = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            e = np.zeros_like(x); e[idx] = eps
            fdx[idx] = (f(W, x + e) - f(W, x - e)) / (2 * eps)
        eW, ex = np.abs(fdW - dW).max() / np.abs(dW).max(), np.abs(fdx - dx).max() / np.abs(dx).max()
        print(f"reverse {reverse}: dW {eW:.2e} dx {ex:.2e}")
        assert eW <= 1e-7 and ex <= 1e-7, (eW, ex)


def test_reference_f32_mode_stays_close_to_f64():
    """Within 2e-6 of f64 relative to each array's largest entry (four times the worst deviation measured when the reference was written:
    1.2e-7 outputs, 2.3e-7 dx, 4.7e-7 dW)."""
    worst = [0.0, 0.0, 0.0]
    for sizes, T, B in [((32, 16, 16), 50, 256), ((5, 7, 3, 9), 9, 37), ((40, 21, 11), 9, 37), ((3, 10), 1, 1), ((32, 32, 32), 9, 37), ((16, 64), 9, 37)]:
        rng = np.random.default_rng(T + B)
        W = G.weights(sizes, seed=4)
        x = rng.standard_normal((T, B, sizes[0])).astype(np.float32)
        dy = (rng.standard_normal((B, sizes[-1])) / B).astype(np.float32)
        y32 = G.forward(sizes, W, x, True, np.float32)
        dx32, dW32 = G.backward(sizes, W, x, dy, True, np.float32)
        assert y32.dtype == dx32.dtype == dW32.dtype == np.float32
        y64 = G.forward(sizes, W, x, True)
        dx64, dW64 = G.backward(sizes, W, x, dy, True)
        for i, (a, b) in enumerate(((y32, y64), (dx32, dx64), (dW32, dW64))):
            worst[i] = max(worst[i], np.abs(a - b).max() / np.abs(b).max())
    print("f32 against f64: y %.2e dx %.2e dW %.2e" % tuple(worst))
    assert max(worst) <= 2e-6, worst


def test_python_tags():
    import latentdiffeq_amd as M
    from latentdiffeq_amd import _lib as L
    from latentdiffeq_amd.recurrent import GRU, LSTM, Recurrent
    assert M.GRU is GRU and L.CELL_GRU == 3
    c = GRU(8, 12)
    assert (c.code, c.G, c.S) == (3, 3, 1) and c.Wi.shape == (36, 8) and c.Wh.shape == (36, 12) and c.b.shape == (36,) and c.state0.shape == (12,)
    m = Recurrent(GRU(8, 12), GRU(12, 12))
    assert m.num_weights == _formula((8, 12, 12)) == m.theta.numel() and m.code == 3 and m.sizes == [8, 12, 12]
    # the flat parameter is the reference's destructure order
    cells = G.unpack(m.theta.detach().numpy(), (8, 12, 12))
    for cell, (Wi, Wh, b, s0) in zip(m.cells, cells):
        assert np.array_equal(cell.Wi.detach().numpy(), Wi) and np.array_equal(cell.Wh.detach().numpy(), Wh)
        assert np.array_equal(cell.b.detach().numpy(), b) and np.array_equal(cell.state0.detach().numpy(), s0)
    with pytest.raises(TypeError, match="GRU"):
        Recurrent(GRU(8, 12), LSTM(12, 12))


def test_gru_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tmp_path, "gru_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "gru_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "gru host plan under ASan + UBSan" in r.stdout
    # the map in numpy agrees with the reference's layout: scattering a flat cell through it gives the pseudo-row matrix
    i, h = 5, 3
    W = G.weights((i, h), seed=3, dtype=np.float64)
    Wi, Wh, b, _ = G.unpack(W, (i, h))[0]
    pseudo = np.zeros((4 * h, i + h))
    pseudo[:3 * h, :i] = Wi
    pseudo[:2 * h, i:] = Wh[:2 * h]
    pseudo[3 * h:, i:] = Wh[2 * h:]
    staged = np.concatenate([pseudo.T.reshape(-1), b, np.zeros(h)])
    R, P = 3 * h, 4 * h

    def idx(e):
        if e < R * i:
            return (e // R) * P + e % R
        e -= R * i
        if e < R * h:
            r = e % R
            return (i + e // R) * P + (r if r < 2 * h else r + h)
        return P * (i + h) + e - R * h
    assert np.array_equal(np.array([staged[idx(e)] for e in range(W.size - h)]), W[:W.size - h])
