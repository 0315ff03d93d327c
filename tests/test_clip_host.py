"""CPU: the clipped parameter update (lde_clip_ws_bytes / lde_adamw_flux_step_clipped, include/lde.h: "the clipped step";
`FluxADAMW(clip_norm=…)`, `train(clip_norm=…)`) without a GPU — (1) the entry points exist, size the workspace on the host and refuse bad
arguments before any device call; (2) csrc/lde_host.h's workspace plan (clip_plan) and refusals (clip_args_ok) under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/clip_host_driver.cpp, run as a program); (3) the Python layer's refusals; (4) the non-native path of
`FluxADAMW(clip_norm=…)` against the numpy restatement (tests/clip_ref.py) in both modes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FAKE = C.c_void_p(0x1000)      # a non-NULL, 8-byte aligned pointer that is never dereferenced: every call below is refused on the host
HP = (1e-3, 0.9, 0.999, 1e-8, 1e-3)
S = 8192


def test_entry_points_exist_size_the_workspace_and_refuse_bad_arguments_without_a_device():
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    assert {"lde_clip_ws_bytes", "lde_adamw_flux_step_clipped"} <= set(L.EXPORTS)
    assert (L.CLIP_GLOBAL, L.CLIP_PER_ARRAY) == (R.GLOBAL, R.PER_ARRAY) == (0, 1) and L.CLIP_MODES == R.MODES
    # the workspace: 8 bytes per scan workgroup (8 192 elements each), and 8 + 16 + 4 per non-empty array
    sizes = [1, 0, S, S + 1, 0, 2 * S + 7]
    t = (L.AdamTensor * len(sizes))()
    for a, n in zip(t, sizes):
        a.n = n
    assert lib.lde_clip_ws_bytes(len(sizes), t) == 8 * (1 + 1 + 2 + 3) + 28 * 4
    assert lib.lde_clip_ws_bytes(0, None) == 0 and lib.lde_clip_ws_bytes(0, t) == 0 and lib.lde_clip_ws_bytes(3, None) == 0
    empty = (L.AdamTensor * 2)()
    assert lib.lde_clip_ws_bytes(2, empty) == 0
    for a in t:
        a.p = a.g = a.m = a.v = 0x2000
    clipped = lib.lde_adamw_flux_step_clipped
    ok = dict(c=1.0, mode=0, step=FAKE, guard=FAKE, ws=FAKE, norms=FAKE)

    def call(n=len(sizes), tab=t, hp=HP, **kw):
        a = dict(ok, **kw)
        return clipped(n, tab, *hp, a["c"], a["mode"], a["step"], a["guard"], a["ws"], a["norms"], None)

    for name in ("step", "guard", "ws", "norms"):
        assert call(**{name: None}) == INVALID, name
    assert call(ws=C.c_void_p(0x1004)) == INVALID                   # a workspace that cannot hold an f64
    for c in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(c=c) == INVALID, c
    for mode in (-1, 2, 99):
        assert call(mode=mode) == INVALID, mode
    # what lde_adamw_flux_step_dev refuses
    assert call(n=-1) == INVALID and call(tab=None) == INVALID
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, float("nan"))):
        assert call(hp=(1e-3, b1, b2, 1e-8, 0.0)) == INVALID, (b1, b2)
    t[3].n = -3
    assert call() == INVALID
    t[3].n = S + 1
    for field in ("p", "g", "m", "v"):
        setattr(t[3], field, None)
        assert call() == INVALID, field
        setattr(t[3], field, 0x2000)
    t[0].n = 2 ** 30 * 2048 + 1                                     # one array beyond 2³⁰ workgroups of the update
    assert call() == INVALID
    assert call(n=0, tab=None, norms=None, ws=None) == INVALID      # even a step over nothing writes norms_dev[0]


def test_python_layer_refusals():
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    p = [torch.nn.Parameter(torch.ones(3))]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_norm"):
            FluxADAMW(p, clip_norm=bad)
    with pytest.raises(ValueError, match="clip_mode"):
        FluxADAMW(p, clip_norm=1.0, clip_mode="value")
    with pytest.raises(ValueError, match="clip_mode"):
        FluxADAMW(p, clip_mode="l2")
    with pytest.raises(ValueError, match="capturable"):              # the guard's own rule still comes first
        FluxADAMW(p, clip_norm=1.0, guard=True)
    with pytest.raises(ValueError):                                  # native=True on CPU tensors
        FluxADAMW(p, clip_norm=1.0, native=True)
    with pytest.raises(ValueError, match="grad_norms"):
        FluxADAMW(p).grad_norms()
    opt = FluxADAMW(p, clip_norm=2.0, clip_mode="per_array")         # CPU tensors: the non-native path, nothing allocated on a device
    assert opt.native is False and opt._clip_ws is None and opt._norms_dev is None and opt.clip_norm == 2.0
    assert opt.grad_norms() == ([0.0], 0.0)


def test_native_path_needs_the_capturable_guarded_form():
    """The rule `clip_norm` on the native path → capturable=True, guard=True, checked without a device: the constructor decides `native`
    from the tensors' `is_cuda`, so a parameter that only claims to be on the GPU takes it as far as the refusal."""
    import torch
    from latentdiffeq_amd.train import FluxADAMW

    class OnGpu(torch.nn.Parameter):
        is_cuda = True

    p = [OnGpu(torch.ones(3))]
    with pytest.raises(ValueError, match="capturable=True, guard=True"):
        FluxADAMW(p, clip_norm=1.0, fused=False, native=True)


def test_workspace_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "clip_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "clip_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "clipped step host logic under ASan + UBSan" in r.stdout


def _arrays(seed, sigma):
    rng = np.random.default_rng(seed)
    sizes = [5, 0, 300, 17, 1]
    ps = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [[(rng.standard_normal(n) * s).astype(np.float32) for n, s in zip(sizes, sigma)] for _ in range(3)]
    return sizes, ps, gs


@pytest.mark.parametrize("mode", ["global", "per_array"])
def test_non_native_path_matches_the_restatement(mode):
    """Three steps of `FluxADAMW(native=False, clip_norm=c)` on CPU tensors against tests/clip_ref.py. Arrays 0 and 3 lie under the per-array
    threshold, 2 and 4 over it; the global norm is over it. The scale must be the restatement's BIT FOR BIT (f64 norm → f32 → f32 scale:
    the same operations on both sides); the step after it is torch's Adam against Flux's formula, equal up to rounding. This path forms
    (1 − decay)·p − Δ where the formula has p − (Δ + decay·p): p is rounded at other places, up to two ulps (≤ 2⁻²²·|p|) apart per step,
    and the steps add up — after step k, |p − p_ref| ≤ k·(1e-5·η + 2⁻²²·|p|); m within 4e-6 and v within 8e-6 of their largest entries
    (the per-step bounds of tests/test_gpu_clip.py)."""
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    sigma = [0.1, 1.0, 0.5, 0.05, 3.0]
    sizes, ps, gs = _arrays(11, sigma)
    c = 1.0
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = FluxADAMW(params, lr=HP[0], betas=(HP[1], HP[2]), eps=HP[3], decay=HP[4], native=False, clip_norm=c, clip_mode=mode)
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    ref_p = [p.copy() for p in ps]
    for k, g in enumerate(gs, 1):
        for p, a in zip(params, g):
            p.grad = torch.from_numpy(a.copy())
        opt.step()
        ref_p, ms, vs, per, total, s = R.clipped_step(ref_p, g, ms, vs, k, HP, c, R.MODES[mode], one_minus_beta_in_f64=True)
        got_per, got_total = opt.grad_norms()
        assert got_per == [float(np.float32(x)) for x in per] and got_total == float(np.float32(total)), (got_per, per)
        if mode == "per_array":
            over = [float(x) != 1.0 for x in s]
            assert over == [np.float32(n) > np.float32(c) for n in per] and over[2] and not over[0] and not over[1] and not over[3], (per, s)
        else:
            assert float(s[0]) < 1.0 and len(set(float(x) for x in s)) == 1
        for i, (p, a) in enumerate(zip(params, g)):                 # the gradients were scaled in place, by exactly the restatement's scale
            assert np.array_equal(p.grad.numpy(), (np.float32(s[i]) * a).astype(np.float32)), (k, i)
            got = p.detach().numpy()
            assert (np.abs(got - ref_p[i]) <= k * (1e-5 * HP[0] + 2.0 ** -22 * np.abs(ref_p[i]))).all(), (k, i, np.abs(got - ref_p[i]).max())
            st = opt.state[p]
            if sizes[i]:
                assert np.abs(st["exp_avg"].numpy() - ms[i]).max() <= 4e-6 * np.abs(ms[i]).max(), (k, i)
                assert np.abs(st["exp_avg_sq"].numpy() - vs[i]).max() <= 8e-6 * np.abs(vs[i]).max(), (k, i)


@pytest.mark.parametrize("mode", ["global", "per_array"])
def test_a_norm_under_the_threshold_changes_nothing_bitwise(mode):
    """Every norm under c: the clipped optimiser and the plain one end bit for bit alike, and the gradients are untouched. (Global mode:
    ‖g‖ + 1e-6 < c, so min(1, ·) = 1 exactly.)"""
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    sizes, ps, gs = _arrays(12, [0.1, 0.1, 0.1, 0.1, 0.1])
    per, total = R.norms(gs[0])
    c = 2.0 * total
    a = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    b = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    oa = FluxADAMW(a, lr=HP[0], decay=HP[4], native=False, clip_norm=c, clip_mode=mode)
    ob = FluxADAMW(b, lr=HP[0], decay=HP[4], native=False)
    for g in gs:
        for x, y, arr in zip(a, b, g):
            x.grad, y.grad = torch.from_numpy(arr.copy()), torch.from_numpy(arr.copy())
        oa.step()
        ob.step()
        for x, y, arr in zip(a, b, g):
            assert np.array_equal(x.grad.numpy(), arr)
            assert np.array_equal(x.detach().numpy().view(np.int32), y.detach().numpy().view(np.int32))
            for key in ("exp_avg", "exp_avg_sq"):
                assert np.array_equal(oa.state[x][key].numpy().view(np.int32), ob.state[y][key].numpy().view(np.int32))
    assert all(float(x) == 1.0 for x in R.scales(per, total, c, R.MODES[mode]))


@pytest.mark.parametrize("mode", ["global", "per_array"])
def test_a_norm_over_the_threshold_scales_as_defined(mode):
    """One array of norm N, c = N/4: after clipping the gradient has norm c·N/(N + 1e-6) (global: torch's rule) or c (per array: Flux's),
    to f32 rounding, and the first step moves every parameter by η against the gradient's sign whatever the scale (Adam's first step is
    ±η·g/(|g| + ε)) — so clipping shows in the moments: m = (1 − β₁)·s·g, v = (1 − β₂)·(s·g)²."""
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    rng = np.random.default_rng(13)
    g = rng.standard_normal(1000).astype(np.float32)
    N = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    c = N / 4
    p = torch.nn.Parameter(torch.zeros(1000))
    opt = FluxADAMW([p], lr=1e-3, decay=0.0, native=False, clip_norm=c, clip_mode=mode)
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    s = R.scales([N], N, c, R.MODES[mode])[0]
    want = c * N / (N + 1e-6) if mode == "global" else c
    clipped = p.grad.numpy()
    assert np.array_equal(clipped, np.float32(s) * g)
    assert abs(float(np.sqrt(np.sum(clipped.astype(np.float64) ** 2))) - want) <= 4 * 2.0 ** -24 * want
    assert opt.grad_norms() == ([float(np.float32(N))], float(np.float32(N)))
    m, v = opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()
    assert np.allclose(m, 0.1 * clipped, rtol=1e-5, atol=0) and np.allclose(v, 0.001 * clipped * clipped, rtol=1e-4, atol=1e-30)


def test_train_takes_clip_norm():
    """`train(..., clip_norm=, clip_mode=)` exists with the defaults of the issue; the loop itself needs the GPU (tests/test_gpu_clip.py)."""
    import inspect
    from latentdiffeq_amd.train import FluxADAMW, train
    sig = inspect.signature(train).parameters
    assert sig["clip_norm"].default is None and sig["clip_mode"].default == "global"
    sig = inspect.signature(FluxADAMW.__init__).parameters
    assert sig["clip_norm"].default is None and sig["clip_mode"].default == "global"
