// lde_types.h — the plain-C++ structs the host side of the C ABI and the kernels share: step records, kernel-choice knobs, the option
// block handed to every kernel. No HIP in here: csrc/lde_host.h (the C ABI's argument / workspace / record logic) includes this file and
// is compiled by an ordinary host compiler too — under AddressSanitizer + UBSan in tests/host_logic_driver.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lde.h"

namespace lde {

// A step record in device memory (include/lde.h: lde_set_step_record): the accepted steps of each of `nseq` step sequences (one per
// trajectory, or one for a coupled solve) — written by a forward solve (LDE_SENSE_DISCRETE: start time, step size and start state of
// every accepted step, what the discrete adjoint sweeps in reverse), read by that adjoint; the continuous adjoint writes the magnitudes of
// its reverse-time steps into one when step tracing is on (y == nullptr). n == nullptr: no record.
struct StepRec {
  int32_t* n;    // [nseq] accepted steps; a count > cap means the record is incomplete
  double* t;     // [cap][nseq] start time of step n
  double* dt;    // [cap][nseq] its size (the state advances by (float)dt)
  float* y;      // [cap][B][D'] state at the start of step n
  int cap, nseq;
};

// LDE_SENSE_FORWARD_DUAL's record in device memory (include/lde.h: lde_set_step_record): written by k_forward_dual (csrc/lde_dual.hip) or
// k_pend_forward_sde, read by k_adjoint_dual. J holds ∂ẑ(t_j)/∂q of every save time, trajectory fastest, with NP partials per component — a
// compile-time constant of the kernels (the system's: 3 for the pendulums, q = (x₀, v₀, L); 6 for Lotka–Volterra, q = (x₀, y₀, α, β, γ, δ)):
// element (j, i, q, b) at ((j·2 + i)·NP + q)·B + b. No field says which NP: the kernels read none. The lane-per-direction kernels
// (csrc/lde_dual_dir.hip: Kuramoto, the double pendulum) use the same struct with extents of their own, J [T][D][B][G]: element (j, i, b, q) at
// ((j·D + i)·B + b)·G + q.
struct DualRec {
  int32_t* n;    // [B] accepted steps; −retcode for a failed trajectory
  float* J;      // [T][2][NP][B]
  double* t;     // [cap][B] start time of accepted step n (option "step_trace"; nullptr otherwise)
  double* dt;    // [cap][B] its size
  int cap;       // 0 without the trace
};

// The stochastic pendulum's noise (include/lde.h: lde_set_noise), handed to k_pend_forward_sde by value: the Philox key, the two counter
// words a caller steers and the device word the kernel adds to `offset` at run time.
struct SdeNoise {
  unsigned long long seed = 0, offset = 0, first_trajectory = 0;
  const long long* epoch_dev = nullptr;
};

// Substeps of one save interval of length D under the nominal step dt (include/lde.h: "the substep rule"): max(1, ceil(D/dt − 1e-9)), at
// most 1e9. ONE definition for the host's plan (csrc/lde_host.h: sde_plan) and the kernel's loop: f64 division and ceil round the same way
// on both sides.
#ifdef __HIPCC__
#define LDE_HD __host__ __device__
#else
#define LDE_HD
#endif
LDE_HD inline int sde_substeps(double D, double dt) {
  const double n = __builtin_ceil(D / dt - 1e-9);
  return !(n >= 1.0) ? 1 : n > 1e9 ? 1000000000 : (int)n;
}

// Kernel-choice knobs of a handle (lde_set_option; tests force a family / a threshold through them — formerly LDE_* environment variables,
// which a library behind a `ccall` host must not read). Defaults = the measured choices.
struct PendTune {
  int ws = 1;                 // "pend_ws": k_pend_forward_ws for B ≤ 16384
  int tl_max_b = 2048;        // "pend_tl_max_b": k_pend_forward_tl up to this batch (solves that write no step record; 13.5 against k_pend_forward_ws's 15.9 µs at 2 048, 20.9 against 15.8 at 4 096)
  int sh_max_b = -1;          // "pend_sh_max_b": k_pend_forward_sh / k_pend_forward_lp (a trajectory per workgroup) up to this batch; −1: the measured thresholds (lp 1 024; sh 768 with a step record, 256 without)
  int lp = 1;                 // "pend_lp": frictionless Tsit5 adaptive solves of that shape run k_pend_forward_lp (lane pairs, Nyström form); 0: k_pend_forward_sh
  int lb_ring = 16;           // "pend_lb": rows of the large-batch row ring (8 / 16 / 32; 0: off)
  int lb_min_b = 1 << 17;     // "pend_lb_min_b": the large-batch form from this batch on
  int lb_hold = -1;           // "pend_lb_hold": its hold margin (−1: half the ring)
  int disc_tp_max_b = 16384;  // "pend_disc_tp_max_b": LDE_SENSE_DISCRETE pullback with a wave per trajectory (k_pend_adjoint_disc_tp) up to this batch
};
struct MlpTune {
  int mlp64 = 1, mlpv = 1, mlpw = 1, mlp4 = 1;   // "mlp64", "mlpv", "mlpw", "mlp4": 0 switches the family off
  int mlpb = 1;               // "mlpb": 0 off (k_mlpw instead: the parity reference), 2 also the networks of ≤ 128 units
  int mlp4_maxw = 64;         // "mlp4_maxw": widest layer k_mlp4_adjoint takes
  int stage_slots = 0;        // "mlp_stage_slots": staging slots per workgroup (0: automatic)
  int peer_spin_k = 0;        // "peer_spin_k": lde_set_global_sum_peers' cross-rank wait gives up after this many × 1024 polls (0: 8192 ≈ 10 s)
};

// What the kernel-family choice of the MLP path knows about a plan (csrc/lde_host.h: mlp_forward_mapping / mlp_adjoint_mapping); filled
// once by mlp_plan_create (csrc/lde_mlp.hip).
struct MlpShape {
  int nL = 0, Dp = 0, P = 0;  // Dense layers, state rows D′ = D + augment_dim, per-trajectory parameters
  int hm = 0;                 // the wider of the two hidden layers of a three-layer network (0: another depth)
  int maxw = 0;               // the widest layer, input and output included
  bool coupled = false;       // LDE_BATCH_COUPLED[_GLOBAL]: one step sequence for the batch
  bool global = false;        // LDE_BATCH_COUPLED_GLOBAL: the batch is sharded over ranks
  bool disc = false;          // LDE_SENSE_DISCRETE: lde_adjoint sweeps the forward solve's step record
  bool vec_ok = false, w_ok = false, b_ok = false, c_ok = false;   // the network fits k_mlpv / k_mlpw / k_mlpb / k_mlpc
  int v_nt = 0;               // k_mlpv: lanes per workgroup (64 / 128 / 256)
  bool v_reg = false;         // k_mlpv: the hidden×hidden product keeps its weights in registers
  int w_waves = 0;            // k_mlpw: waves per trajectory (2 / 4)
};
// LDS bytes of the candidate families for one (save grid, forward or adjoint), from the formulas beside the kernels whose carve-up they
// describe (csrc/lde_mlp.hip: mlp_lds_numbers); the mappings only compare them. 0 where the network does not fit the family.
struct MlpLds {
  size_t cap = 0;             // what a workgroup can get (LDS_MAX)
  size_t v_fixed = 0;         // k_mlpv without its weight cache
  size_t w = 0, b = 0, c = 0; // k_mlpw, k_mlpb, k_mlpc without the cotangent copies
  size_t b_disc = 0, c_disc = 0;   // the discrete sweeps of k_mlpb (with its cotangent copy) and k_mlpc (with its second slot bank)
  size_t mlp4 = 0;            // k_mlp4_adjoint
  int mlp4_blocks = 0;        // … and its workgroups
};

// What the LDS carve-up of a dense chain's tile kernels depends on (csrc/lde_host.h: chain_lds_bytes / chain_tile_pick); filled from
// ChainDims / BfDims, whose layouts the kernels of csrc/lde_chain.hip and csrc/lde_chain_bf16.h walk.
struct ChainLdsDims {
  int ld0 = 0, ldh = 0;       // f32: stride (floats) of the input panel (0: x is read in place) and of the hidden / gradient panels
  int nbias = 0;              // biases of all layers (floats), kept in LDS by the forward kernels
  int ldb = 0, ldg = 0;       // bf16: stride (elements) of the bf16 panels, stride (floats) of the f32 skip-gradient panel
  int fpanel = 0;             // bf16 forward: a third panel (chains with skip layers)
  size_t xs_per_cg = 0;       // bf16 forward reading x in place: bytes of the first layer's chunk buffers per column group (else 0)
};

// The layout of a recurrent stack (csrc/lde_rnn.hip), filled by csrc/lde_host.h: rnn_layout and handed to the kernels by value: the rows
// of [Wi | Wh], biases and initial states of every cell in LDS, the cells' places in the flat weight vector, the per-trajectory buffers.
constexpr int RNN_ML = LDE_RNN_MAX_LAYERS;
struct RnnDims {
  int cell, nL, reverse, G;
  int sizes[RNN_ML + 1];
  int Hp;               // lanes per trajectory
  int K[RNN_ML];        // in_l + h_l
  int ldk[RNN_ML];      // row stride of [Wi | Wh] in LDS: ≥ pad4(K), (ldk/4) odd
  int w_off[RNN_ML];    // LDS float offsets: rows [G·h][ldk]
  int b_off[RNN_ML];    // bias [G·h]
  int s_off[RNN_ML];    // state0: h0 [h] (LSTM: then c0 [h])
  int f_off[RNN_ML];    // offset of the cell in the flat weight vector
  int wt;               // 1: LDS also holds the transposed copies [K][ldr] (the pullback's Wᵀδ then reads 16-byte rows too)
  int ldr[RNN_ML];      // their row stride: ≥ pad4(G·h), (ldr/4) odd
  int wt_off[RNN_ML];
  int lds_w;            // floats of the weight area
  int vmax;             // floats of one trajectory's [x; h] vector (pad4(max K) + 4)
  int rmax;             // floats of one trajectory's δ vector (pad4(max G·h))
  int hmax;
  int recw;             // floats of one (step, layer, trajectory) record: gates G·hmax | c hmax | h hmax
};
LDE_HD constexpr int rnn_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
LDE_HD constexpr int rnn_ldk(int K) { int v = (K + 3) & ~3; return ((v >> 2) & 1) ? v : v + 4; }
constexpr int PIPE_R = 8;   // steps of the LDS rings of the two-wave pipeline (rnn_body2)

// Options handed to every kernel by value (mirrors the `kwargs...` splat into solve()).
struct KOpts {
  float abstol, reltol;
  float beta1, beta2;
  float inv_gamma;   // 1/γ
  float q_lo;        // 1/qmax : lower clamp of q
  float q_hi;        // 1/qmin : upper clamp of q
  float qmin;
  double dtmin;
  double dt_fixed;   // fixed step (adaptive=0) or user initial dt (adaptive=1, >0)
  long long maxiters;
  int adaptive;
  int checkpoint;    // adjoint: reset z to the saved ẑ(t_j) at every save time
  int T, B;
  double t_first, t_last;   // ts[0], ts[T−1] (the host has the grid): a kernel need not load them before its first step
  int lb_hold;              // large-batch forward: a lane this close to the end of the row ring waits for its wave (0: never)
  StepRec rec;              // forward: the record to write; discrete adjoint: the record to read; continuous adjoint: the trace to write
  int dw_overwrite;         // adjoint: dW is written, not accumulated (option "adjoint_overwrite")
};


}  // namespace lde
