"""CPU: the AdaBelief step (lde_adabelief_flux_step / _dev / _guarded / _clipped, include/lde.h: "the AdaBelief step"; `FluxAdaBelief`,
`train(optimiser="adabelief")`) without a GPU — (1) the entry points exist and refuse bad arguments before any device call; (2) what
csrc/lde_host.h decides for them under AddressSanitizer + UndefinedBehaviorSanitizer (tests/belief_host_driver.cpp, run as a program);
(3) the Python layer's refusals; (4) the numpy restatement (tests/belief_ref.py) on answers known in closed form; (5) the non-native path
of `FluxAdaBelief` against the restatement; (6) THE FLOOR: the restatement's f32 mode against its f64 mode on the inputs of
tests/test_gpu_belief.py, per quantity and per step — the GPU tests' bounds are 4× these numbers, computed there from the same function.

Measured here (x in units of 2⁻²⁴·(|x| + η); m and s relative to the largest entry of the step), steps 1 … :
    "paths"      x 2.95 4.02 3.14 3.75   m 4.57e-08 7.10e-08 8.53e-08 8.72e-08   s 1.03e-07 1.36e-07 1.55e-07 1.21e-07
    "49 arrays"  x 2.34 3.02 3.61        m 4.56e-08 6.96e-08 8.91e-08            s 1.18e-07 9.59e-08 1.03e-07
(the non-native path of FluxAdaBelief lands ON the floor, digit for digit: it is the f32 mode's operations in torch).
"""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import belief_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FAKE = C.c_void_p(0x1000)      # a non-NULL, 8-byte aligned pointer that is never dereferenced: every call below is refused on the host
HP = R.HP
S = 8192
FORMS = ("lde_adabelief_flux_step", "lde_adabelief_flux_step_dev", "lde_adabelief_flux_step_guarded", "lde_adabelief_flux_step_clipped")


def test_entry_points_exist_and_refuse_bad_arguments_without_a_device():
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    assert set(FORMS) <= set(L.EXPORTS) and all(hasattr(lib, f) for f in FORMS)
    sizes = [1, 0, S, S + 1, 0, 2 * S + 7]
    t = (L.AdamTensor * len(sizes))()
    for a, n in zip(t, sizes):
        a.n = n
        a.p = a.g = a.m = a.v = 0x2000
    ok = dict(c=1.0, mode=0, step=FAKE, guard=FAKE, ws=FAKE, norms=FAKE)

    def call(form, n=len(sizes), tab=t, hp=HP, t_host=1, **kw):
        a = dict(ok, **kw)
        if form == FORMS[0]:
            return lib.lde_adabelief_flux_step(n, tab, *hp, t_host, None)
        if form == FORMS[1]:
            return lib.lde_adabelief_flux_step_dev(n, tab, *hp, a["step"], None)
        if form == FORMS[2]:
            return lib.lde_adabelief_flux_step_guarded(n, tab, *hp, a["step"], a["guard"], None)
        return lib.lde_adabelief_flux_step_clipped(n, tab, *hp, a["c"], a["mode"], a["step"], a["guard"], a["ws"], a["norms"], None)

    clipped = FORMS[3]
    # the list of tests/test_clip_host.py, on the clipped form …
    for name in ("step", "guard", "ws", "norms"):
        assert call(clipped, **{name: None}) == INVALID, name
    assert call(clipped, ws=C.c_void_p(0x1004)) == INVALID
    for c in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(clipped, c=c) == INVALID, c
    for mode in (-1, 2, 99):
        assert call(clipped, mode=mode) == INVALID, mode
    assert call(clipped, n=0, tab=None, norms=None, ws=None) == INVALID
    # … the pointers of the other forms …
    assert call(FORMS[1], step=None) == INVALID and call(FORMS[2], step=None) == INVALID and call(FORMS[2], guard=None) == INVALID
    for bad_t in (0, -3):
        assert call(FORMS[0], t_host=bad_t) == INVALID
    # … and what every form refuses: the table, the βs, and BOTH ε's in {−1, NaN, ±Inf}
    for form in FORMS:
        assert call(form, n=-1) == INVALID and call(form, tab=None) == INVALID, form
        for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, float("nan"))):
            assert call(form, hp=(1e-3, b1, b2, 1e-16, 1e-16, 0.0)) == INVALID, (form, b1, b2)
        for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
            assert call(form, hp=(1e-3, 0.9, 0.999, bad, 1e-16, 0.0)) == INVALID, (form, "eps_var", bad)
            assert call(form, hp=(1e-3, 0.9, 0.999, 1e-16, bad, 0.0)) == INVALID, (form, "eps_den", bad)
        t[3].n = -3
        assert call(form) == INVALID, form
        t[3].n = S + 1
        for field in ("p", "g", "m", "v"):
            setattr(t[3], field, None)
            assert call(form) == INVALID, (form, field)
            setattr(t[3], field, 0x2000)
        t[0].n = 2 ** 30 * 2048 + 1                                     # one array beyond 2³⁰ workgroups of the update
        assert call(form) == INVALID, form
        t[0].n = 1


def test_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "belief_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "belief_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "AdaBelief step host logic under ASan + UBSan" in r.stdout


def test_python_layer_refusals():
    import torch
    from latentdiffeq_amd.train import FluxAdaBelief, train
    p = [torch.nn.Parameter(torch.ones(3))]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"FluxAdaBelief\(clip_norm"):
            FluxAdaBelief(p, clip_norm=bad)
    with pytest.raises(ValueError, match=r"FluxAdaBelief\(clip_mode"):
        FluxAdaBelief(p, clip_norm=1.0, clip_mode="value")
    with pytest.raises(ValueError, match=r"FluxAdaBelief\(guard=True\) needs capturable=True"):
        FluxAdaBelief(p, clip_norm=1.0, guard=True)
    with pytest.raises(ValueError, match=r"FluxAdaBelief\(native=True\)"):
        FluxAdaBelief(p, native=True)
    with pytest.raises(ValueError, match=r"FluxAdaBelief\(capturable=True\) needs the native path"):
        FluxAdaBelief(p, capturable=True)
    with pytest.raises(ValueError, match=r"FluxAdaBelief.grad_norms"):
        FluxAdaBelief(p).grad_norms()
    with pytest.raises(ValueError, match=r"FluxAdaBelief.guard_state"):
        FluxAdaBelief(p).guard_state()
    for bad in (-1.0, float("nan"), float("inf"), (1e-8,), (1e-8, -1.0), (float("nan"), 1e-8), "x"):
        with pytest.raises(ValueError, match="eps"):
            FluxAdaBelief(p, eps=bad)
    for bad in ((1.0, 0.999), (0.9, -0.1), (0.9,)):
        with pytest.raises(ValueError, match="betas"):
            FluxAdaBelief(p, betas=bad)
    opt = FluxAdaBelief(p, clip_norm=2.0, clip_mode="per_array")      # CPU tensors: the non-native path, nothing allocated on a device
    assert opt.native is False and opt._clip_ws is None and opt._norms_dev is None and opt.clip_norm == 2.0 and opt.guard is False
    assert opt.grad_norms() == ([0.0], 0.0)
    ev, ed = FluxAdaBelief(p)._eps_args(dict(eps=1e-8))                                  # a number: ε² in both places (Flux's, as recalled)
    assert np.float32(ev) == np.float32(ed) == np.float32(1e-16)                         # (the C ABI takes f32)
    assert FluxAdaBelief(p, eps=(1e-8, 1e-3))._eps_args(dict(eps=(1e-8, 1e-3))) == (1e-8, 1e-3)     # a pair: as given (the paper's placement)

    class OnGpu(torch.nn.Parameter):
        is_cuda = True

    with pytest.raises(ValueError, match=r"FluxAdaBelief\(clip_norm=...\) on the native path needs capturable=True, guard=True"):
        FluxAdaBelief([OnGpu(torch.ones(3))], clip_norm=1.0, native=True)
    with pytest.raises(ValueError, match="optimiser"):
        train(None, [], None, 0.05, 1, 10, 12, optimiser="sgd")
    import inspect
    assert inspect.signature(train).parameters["optimiser"].default == "adamw"
    sig = inspect.signature(FluxAdaBelief.__init__).parameters
    assert [k for k in sig][1:] == ["params", "lr", "betas", "eps", "decay", "native", "capturable", "guard", "clip_norm", "clip_mode"]
    assert (sig["lr"].default, sig["betas"].default, sig["eps"].default, sig["decay"].default) == (1e-3, (0.9, 0.999), 1e-8, 0.0)


def test_the_adamw_messages_are_what_they_were():
    """The plumbing is shared by factoring: FluxADAMW's texts keep its own name."""
    import torch
    from latentdiffeq_amd.train import FluxADAMW
    p = [torch.nn.Parameter(torch.ones(3))]
    for kw, text in ((dict(guard=True), "FluxADAMW(guard=True) needs capturable=True (the guard is part of the device-counted step)"),
                     (dict(clip_norm=-1.0), "FluxADAMW(clip_norm=...) takes a finite threshold > 0 (None: no clipping)"),
                     (dict(native=True), "FluxADAMW(native=True) needs contiguous float32 HIP parameters"),
                     (dict(capturable=True), "FluxADAMW(capturable=True) needs the native path")):
        with pytest.raises(ValueError) as e:
            FluxADAMW(p, **kw)
        assert str(e.value) == text


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_restatement_first_step_moves_every_element_by_eta_over_beta1(mode):
    """ε negligible, decay 0, m = s = 0: m = (1 − β₁)g, g − m = β₁g, s = (1 − β₂)β₁²g², m̂ = g, ŝ = β₁²g², so Δ = η·g/(β₁|g|) = ±η/β₁."""
    rng = np.random.default_rng(1)
    g = (rng.standard_normal(5000) * np.exp(rng.uniform(-6, 3, 5000))).astype(np.float32)
    g = g[g != 0]
    x = rng.standard_normal(g.size).astype(np.float32)
    hp = (1e-3, 0.9, 0.999, 1e-30, 1e-30, 0.0)
    p, m, s, d = R.step(x, g, np.zeros_like(x), np.zeros_like(x), 1, hp, mode)
    want = float(np.float32(1e-3)) / float(np.float32(0.9))
    ratio = np.asarray(d, np.float64) * np.sign(g) / want
    tol = 1e-12 if mode == "f64" else 8 * 2.0 ** -24
    assert np.abs(ratio - 1.0).max() <= tol, np.abs(ratio - 1.0).max()
    assert np.array_equal(np.sign(np.asarray(x, np.float64) - p), np.sign(g)) or mode == "f32"


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_restatement_zero_gradient_moves_nothing(mode):
    """g ≡ 0 from a zero state: m and Δ stay 0, x = 0 stays 0 (with a decay too), s is the sum of the ε_var's and nothing is NaN."""
    z = np.zeros(100, np.float32)
    p, m, s = z, z, z
    for t in range(1, 4):
        p, m, s, d = R.step(p, z, m, s, t, R.HP, mode)
        assert not np.isnan(np.concatenate([p, m, s, d])).any()
        assert not p.any() and not m.any() and not d.any() and (s > 0).all()


def _three_steps(eps, hp, clip=None, mode="global"):
    import torch
    from latentdiffeq_amd.train import FluxAdaBelief
    sizes, _, ps, grads = R.inputs("paths")
    grads = grads[:3]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = FluxAdaBelief(params, lr=hp[0], betas=(hp[1], hp[2]), eps=eps, decay=hp[5], native=False, clip_norm=clip, clip_mode=mode)
    scales = [R.clip_scales(gs, clip, R.C.MODES[mode])[0] for gs in grads] if clip is not None else None
    fl, ref = R.floors(ps, grads, R.zeros(ps), R.zeros(ps), hp, scales=scales)
    for k, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        got = ([p.detach().numpy() for p in params], [opt.state[p]["exp_avg"].numpy() for p in params],
               [opt.state[p]["exp_avg_var"].numpy() for p in params])
        err = R.errors(got, ref[k], hp[0])
        print(f"[belief] non-native step {k + 1}: x {err[0]:.2f} m {err[1]:.2e} s {err[2]:.2e}  floor x {fl[k][0]:.2f} m {fl[k][1]:.2e} s {fl[k][2]:.2e}")
        assert all(e <= R.BOUND_FACTOR * f for e, f in zip(err, fl[k])), (k, err, fl[k])
        assert all(opt.state[p]["step"] == k + 1 and set(opt.state[p]) == {"step", "exp_avg", "exp_avg_var"} for p in params)
    return opt


def test_non_native_path_matches_the_restatement():
    """Three steps of `FluxAdaBelief(native=False)` on CPU tensors on the "paths" inputs: within 4 floors of the f64 restatement, per quantity
    and step; with the default ε (a number: ε² in both places) and with a pair."""
    _three_steps(1e-8, R.HP)
    _three_steps((1e-8, 1e-3), (1e-3, 0.9, 0.999, 1e-8, 1e-3, 1e-3))


@pytest.mark.parametrize("mode", ["global", "per_array"])
def test_non_native_path_clips_in_front(mode):
    sizes, _, ps, grads = R.inputs("paths")
    per, total = R.C.norms(grads[0])
    c = 0.5 * (total if mode == "global" else float(np.median([x for x in per if x > 0])))
    opt = _three_steps(1e-8, R.HP, clip=c, mode=mode)
    got_per, got_total = opt.grad_norms()
    per3, total3 = R.C.norms(grads[2])
    assert got_per == [float(np.float32(x)) for x in per3] and got_total == float(np.float32(total3))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_floor_on_the_gpu_tests_inputs(name):
    """The restatement's f32 mode against its f64 mode on the GPU tests' own inputs, per quantity and step (printed: the module docstring and
    DESIGN.md §4.6 record them). What is asserted is only that the floor is what f32 rounding can produce: not zero (the bound 4 × floor would
    be empty), x within a few half-ulps per step taken, m and s within a few 2⁻²⁴ of the largest entry."""
    sizes, _, ps, grads = R.inputs(name)
    fl, ref = R.floors(ps, grads, R.zeros(ps), R.zeros(ps), R.HP)
    assert len(fl) == R.CASES[name]["steps"] >= 3
    for k, (ex, em, es) in enumerate(fl, 1):
        print(f"[belief] floor {name!r} step {k}: x {ex:.2f} × 2^-24·(|x| + η)   m {em:.2e}   s {es:.2e} of the largest entry")
        assert 0.0 < ex <= 2.0 * (k + 1) and 0.0 < em <= 4 * 2.0 ** -24 and 0.0 < es <= 4 * 2.0 ** -24, (k, ex, em, es)
    for k in range(len(ref)):                                            # fresh gradients: s does not collapse to ε_var = 1e-16
        assert float(np.median(np.concatenate([s for s in ref[k][2] if s.size]))) > 1e-8


def test_state_dict_round_trip_off_the_native_path():
    import torch
    from latentdiffeq_amd.train import FluxAdaBelief
    a = [torch.nn.Parameter(torch.ones(7))]
    oa = FluxAdaBelief(a, native=False, decay=1e-3)
    for k in range(2):
        a[0].grad = torch.full((7,), 0.1 * (k + 1))
        oa.step()
    b = [torch.nn.Parameter(a[0].detach().clone())]
    ob = FluxAdaBelief(b, native=False, decay=1e-3)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))     # (torch hands out and takes in the state tensors themselves: a checkpoint is a copy)
    a[0].grad = torch.full((7,), -0.2)
    b[0].grad = torch.full((7,), -0.2)
    oa.step()
    ob.step()
    assert torch.equal(a[0].detach(), b[0].detach()) and int(ob.state[b[0]]["step"]) == 3
