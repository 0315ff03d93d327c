"""CPU: the guarded parameter update (lde_guard_init / lde_adamw_flux_step_guarded, include/lde.h: "the guarded step") without a GPU —
(1) the two entry points exist and refuse NULL words, a NULL step count and everything lde_adamw_flux_step_dev refuses, before any device
call; (2) csrc/lde_host.h's launch packing (opt_next_launch), which the update and the gradient scan share, under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/guard_host_driver.cpp, run as a program); (3) the step counts of the inputs of the end-to-end GPU test
(tests/guard_ref.py) on the CPU oracle: the "mild" ones stay two steps below the record capacity the test starts from, the "harsh" ones
pass it by two, for every trajectory."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from tests import guard_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FAKE = C.c_void_p(0x1000)      # a non-NULL pointer that is never dereferenced: every call below is refused on the host


def test_entry_points_exist_and_refuse_bad_arguments_without_a_device():
    from latentdiffeq_amd import _lib as L
    lib = L.load()
    assert {"lde_guard_init", "lde_adamw_flux_step_guarded"} <= set(L.EXPORTS) and L.GUARD_WORDS == 4
    assert hasattr(lib, "lde_guard_init") and hasattr(lib, "lde_adamw_flux_step_guarded")
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.lde_guard_init(None, None) == INVALID
    t = (L.AdamTensor * 2)()
    for a in t:
        a.p = a.g = a.m = a.v = 0x2000
        a.n = 4
    guarded = lib.lde_adamw_flux_step_guarded
    assert guarded(2, t, *hp, FAKE, None, None) == INVALID          # NULL guard words
    assert guarded(2, t, *hp, None, FAKE, None) == INVALID          # NULL step count
    assert guarded(0, None, *hp, None, None, None) == INVALID
    assert lib.lde_adamw_flux_step_dev(2, t, *hp, None, None) == INVALID
    # what adamw_impl refuses for every form of the update
    assert guarded(-1, t, *hp, FAKE, FAKE, None) == INVALID         # n < 0
    assert guarded(2, None, *hp, FAKE, FAKE, None) == INVALID       # arrays without a table
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-3), (float("nan"), 0.999), (0.9, float("nan"))):
        assert guarded(2, t, 1e-3, b1, b2, 1e-8, 0.0, FAKE, FAKE, None) == INVALID, (b1, b2)
        assert lib.lde_adamw_flux_step_dev(2, t, 1e-3, b1, b2, 1e-8, 0.0, FAKE, None) == INVALID, (b1, b2)
    t[1].n = -3
    assert guarded(2, t, *hp, FAKE, FAKE, None) == INVALID          # a negative size
    t[1].n = 4
    for field in ("p", "g", "m", "v"):
        setattr(t[1], field, None)
        assert guarded(2, t, *hp, FAKE, FAKE, None) == INVALID, field      # a NULL array of a non-empty entry
        assert lib.lde_adamw_flux_step_dev(2, t, *hp, FAKE, None) == INVALID, field
        setattr(t[1], field, 0x2000)
    t[0].n = 2 ** 30 * 2048 + 1                                     # one array beyond 2³⁰ workgroups: refused before the scan is launched
    assert guarded(2, t, *hp, FAKE, FAKE, None) == INVALID


def test_python_layer_refuses_a_guard_without_the_capturable_form():
    import pytest
    import torch
    from latentdiffeq_amd.train import FluxADAMW, GraphedStep
    p = [torch.nn.Parameter(torch.ones(3))]
    with pytest.raises(ValueError, match="capturable"):
        FluxADAMW(p, guard=True)
    with pytest.raises(ValueError, match="capturable"):
        FluxADAMW(p, guard=True, native=False)
    opt = FluxADAMW(p)                      # the default: no guard, nothing allocated
    assert opt.guard is False and opt._guard_dev is None
    with pytest.raises(ValueError):
        opt.guard_state()
    with pytest.raises(ValueError):
        GraphedStep(lambda: None, guard=opt)


def test_launch_packing_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "guard_host_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "guard_host_driver.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]
    assert "guarded step host logic under ASan + UBSan" in r.stdout


def test_end_to_end_inputs_sit_on_either_side_of_the_record_capacity():
    """The oracle's accepted steps per trajectory (f32, Tsit5 at the default tolerances, T = 8 save times 0.25 apart): mild 10, 10, 11, 13,
    11, 11, 10, 10 ≤ CAP − 2 = 18; harsh 41, 45, 46, 49, 45, 43, 42, 50 ≥ CAP + 2 = 22 — a margin of 8 and 19 steps where the kernel's
    controller differs from the oracle's by about 3 % (one or two steps)."""
    from oracle import oracle as O
    orc = O.Oracle("f32")
    d = O.make_desc(sensealg=O.SENSE_DISCRETE)
    counts = {}
    for kind in ("mild", "harsh"):
        z0, th = G.inputs(kind)
        assert z0.shape == (G.B, 2) and th.shape == (G.B, 1) and z0.dtype == np.float32
        z, ret, rec, _ = orc.forward_steps(d, z0, th, G.grid())
        assert (ret == 0).all() and np.isfinite(z).all()
        counts[kind] = rec["n"]
        print(kind, rec["n"].tolist())
    assert counts["mild"].max() <= G.CAP - 2 and counts["harsh"].min() >= G.CAP + 2, counts
    assert (int(counts["mild"].min()), int(counts["mild"].max())) == G.MILD_STEPS
    assert (int(counts["harsh"].min()), int(counts["harsh"].max())) == G.HARSH_STEPS
