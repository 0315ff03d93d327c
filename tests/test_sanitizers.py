"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer over what runs on the CPU (SURVEY.md §5 "race detection / sanitizers"; GPU sanitizers are
not available on this pool): (1) the oracle — everything the parity tests trust — driven at small, ragged, degenerate and failing shapes
through every family of its entry points (oracle/asan_driver.c, f32 and f64 builds); (2) the C ABI's host-side logic — validation of a
problem description, the weight count, the step-record layout arithmetic, the option block, grid checks, the analytic path's kernel
choices, the MLP path's kernel families, the dense chains' tile / layout / split choices and the recurrent stacks' layout / launch plan (csrc/lde_host.h, which lde_api.hip and the launch code are built from) — with 200 000 hostile descriptions (tests/host_logic_driver.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
           OMP_NUM_THREADS="2")


def _clean(r):
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    for bad in ("AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr and bad not in r.stdout, r.stderr[-3000:]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_oracle_under_asan_ubsan(prec):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"], check=True)
    r = subprocess.run([os.path.join(ROOT, "oracle", "_build", f"oracle_asan_{prec}")], capture_output=True, text=True, env=ENV, timeout=600)
    _clean(r)
    assert "rc = 0" in r.stdout


def test_c_abi_host_logic_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    exe = os.path.join(tmp_path, "host_logic_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "host_logic_driver.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=600)
    _clean(r)
    assert "accepted" in r.stdout and "forward mappings as measured" in r.stdout
    assert "pullback mappings, ring shapes and kernel dispatch checked" in r.stdout
    assert "MLP family mappings as measured, reserve rows and solver dispatch checked" in r.stdout
    assert "dense chains: LDS bytes, tile picks, call layouts, tile narrowing and weight-gradient splits as measured; hostile sizes checked" in r.stdout
    assert "recurrent stacks: weight counts, layouts, refusals, launch plans, groupability, k-split and kernel dispatch as in the launch code" in r.stdout


def test_lde_api_is_built_from_the_checked_logic():
    """lde_api.hip must USE lde_host.h's functions (not keep private copies that the sanitizers never see)."""
    src = open(os.path.join(ROOT, "latentdiffeq.jl_amd", "csrc", "lde_api.hip")).read()
    assert '#include "lde_host.h"' in src and "using namespace lde_host" in src
    pend = open(os.path.join(ROOT, "latentdiffeq.jl_amd", "csrc", "lde_pendulum.hip")).read()
    dual = open(os.path.join(ROOT, "latentdiffeq.jl_amd", "csrc", "lde_dual.hip")).read()
    assert "lde_host::pend_forward_mapping(" in pend and "tn.sh_max_b" not in pend and "tn.tl_max_b" not in pend   # the launch code follows the checked function, no thresholds of its own
    assert "lde_host::pend_adjoint_mapping(" in pend and "lde_host::pend_ring_shape(" in pend
    assert "tn." not in pend and "24576" not in pend   # no PendTune field read and no pullback threshold outside lde_host.h
    for s in (pend, dual):   # the (rhs_kind, solver, adaptive) → template-argument chain lives in lde_host::pend_dispatch only
        assert "lde_host::pend_dispatch(" in s and "#define LDE_LAUNCH" not in s
    assert "lde_host::lv_dispatch(" in dual   # (Lotka–Volterra's three combinations likewise)
    # the MLP path likewise: the family choice and every threshold live in lde_host.h's two mappings, the launch code switches on their result
    mlp = open(os.path.join(ROOT, "latentdiffeq.jl_amd", "csrc", "lde_mlp.hip")).read()
    assert "lde_host::mlp_forward_mapping(" in mlp and "lde_host::mlp_adjoint_mapping(" in mlp
    for gone in ("_applicable(", "attr_set", "65536", "tune.mlp64", "tune.mlpv", "tune.mlpw", "tune.mlpb", "tune.mlp4"):
        assert gone not in mlp, gone
    # the dense chains: the tile widths, the layout of a call and the weight-gradient split come from lde_host.h; the launch code keeps no
    # threshold, no per-call state outside its arguments and no per-function attribute table
    chain = open(os.path.join(ROOT, "latentdiffeq.jl_amd", "csrc", "lde_chain.hip")).read()
    for used in ("lde_host::chain_call_choice(", "lde_host::chain_dw_split(", "lde_host::chain_dw_parts_bf16(", "lde_host::chain_tile_pick(", "lde_host::chain_lds_bytes("):
        assert used in chain, used
    for gone in ("thread_local", "attr[", "< 192", "256 /"):
        assert gone not in chain, gone
    assert "bool set_max_lds_(" not in chain   # (shared with the recurrent stacks: csrc/lde_mfma.h)
    # the recurrent stacks: the layout, the kernel form and launch shape of a call and the weight count come from lde_host.h; the launch code
    # keeps no threshold, no spelled-out default shape, no per-call state outside its arguments and no per-function attribute table
    rnn = open(os.path.join(ROOT, "latentdiffeq.jl_amd", "csrc", "lde_rnn.hip")).read()
    for used in ("lde_host::rnn_layout(", "lde_host::rnn_launch_plan(", "lde_host::rnn_num_weights("):
        assert used in rnn, used
    for gone in ("thread_local", "attr[", "io_ld", "io_dy2", "> 1024", "cdiv(512", "sizes[0] == 32"):
        assert gone not in rnn, gone
    for fn in ("static int validate(", "static size_t rec_bytes(", "static lde::StepRec rec_view(", "static lde::KOpts make_opts("):
        assert fn not in src, fn
