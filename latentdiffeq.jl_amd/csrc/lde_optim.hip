// lde_optim.hip — the parameter update of the training step (scope row f-3).
//
// Replaces `Flux.Optimise.update!(opt, ps, grads)` with `opt = ADAMW(η, (β₁, β₂), decay)`
// [REF examples/pendulum_friction-less/model_train.jl:138, :190-192]; in the pinned Flux 0.13.6 [REF Manifest.toml:452] that is
// `Optimiser(ADAM(η, β), WeightDecay(decay))`, applied array by array as broadcast expressions:
//     m ← β₁·m + (1 − β₁)·g;   v ← β₂·v + (1 − β₂)·g²;   Δ = m/(1 − β₁ᵗ) / (√(v/(1 − β₂ᵗ)) + ε) · η;   Δ ← Δ + decay·x;   x ← x − Δ
// (the decay is NOT scaled by η). Here: ONE launch for all parameter arrays of a model. The array table travels in the kernel
// arguments (the gradient pointers change every step, so a device-resident table would need an upload per step); a
// workgroup owns 2048 consecutive elements of one array; 16-byte accesses; 28 algorithmic bytes per element (read x, g, m,
// v; write x, m, v) — HBM-bound in principle, launch-bound at a model's size (1.3 MB of parameters).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lde.h"
#include "lde_host.h"

namespace lde {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

constexpr int GUARD_LOADS = 8;   // 16-byte loads a lane of the scan has in flight: one round of a full slice (measured against 4: DESIGN.md §4.6)
using lde_host::GUARD_PER_WG;    // the slices and the table size: csrc/lde_host.h, beside the function that packs the launches
using lde_host::OPT_MAXT;
using lde_host::OPT_PER_WG;
using lde_host::OPT_WG;

struct OptTable {
  lde_adam_tensor t[OPT_MAXT];
  int blk0[OPT_MAXT + 1];   // first workgroup of array i
  int n;
};
struct OptIdx { int idx[OPT_MAXT]; };   // (the scan) array i's index in the caller's t[]

struct OptCoef { float b1, b2, omb1, omb2, inv_bc1, inv_bc2, eps, lr, decay; };

__device__ __forceinline__ void adam1(float& x, float g, float& m, float& v, const OptCoef& c) {
  m = c.b1 * m + c.omb1 * g;
  v = c.b2 * v + c.omb2 * g * g;
  const float d = (m * c.inv_bc1) / (__builtin_sqrtf(v * c.inv_bc2) + c.eps) * c.lr + c.decay * x;
  x -= d;
}

// `step_dev` != nullptr: the step count t lives in device memory (a captured hipGraph replays the SAME kernel arguments every step, so
// the bias corrections 1/(1 − βᵗ) cannot travel in them): every thread derives them from t = *step_dev + 1, and the count is advanced
// by the update kernel itself (`bump`, the step's last launch) — by the last workgroup to have READ it: each workgroup counts itself
// in behind a barrier, i.e. after all of its waves hold t. (Until round 3 a one-thread kernel in front of the update did it: one more
// launch per training step.)
//
// GUARD (lde_adamw_flux_step_guarded, include/lde.h: "the guarded step"): k_grad_guard has scanned every gradient in launches of its own
// BEFORE the first update launch, and left in guard word [0] the lowest index of an array with a non-finite gradient element (−1: none) —
// the decision exists at a kernel boundary; nothing here waits for another workgroup. A workgroup reads the word once (thread 0, shared
// through LDS at the barrier it has anyway) and, when it is not −1, leaves without touching an element. The last workgroup of the step's
// LAST launch to have read the word (`g_guard_seen`, the same counting-in) does the bookkeeping and puts the word back to −1: by then every
// workgroup of this launch holds its copy and every earlier launch of the call has ended (one stream). GUARD = false is the kernel as it was.
template <bool GUARD> struct GuardArg {};
template <> struct GuardArg<true> { int64_t* w; };   // the LDE_GUARD_WORDS words

// guard words [1..3] at the end of a step (one thread): `bad` = word [0] as the step's workgroups read it
__device__ __forceinline__ void guard_bookkeeping(int64_t* w, int64_t bad, int64_t* step_dev, int64_t ti) {
  if (bad != -1) {
    w[1] += 1;
    w[2] += 1;
    w[3] = bad;
    w[0] = -1;
  } else {
    *step_dev = ti;
    w[2] = 0;
  }
}

__device__ unsigned g_adam_seen = 0;
__device__ unsigned g_guard_seen = 0;
__global__ void k_adam_tick(int64_t* step_dev) { *step_dev += 1; }   // (a step over empty arrays only)
__global__ void k_adam_tick_guarded(int64_t* step_dev, int64_t* w) { guard_bookkeeping(w, w[0], step_dev, *step_dev + 1); }
__global__ void k_guard_init(int64_t* w) {
  w[0] = -1; w[1] = 0; w[2] = 0; w[3] = -1;
}
template <bool GUARD>
__global__ void __launch_bounds__(OPT_WG) k_adamw_flux(OptTable tab, OptCoef c, int64_t* __restrict__ step_dev, int bump, GuardArg<GUARD> ga) {
  if constexpr (GUARD) {
    __shared__ int64_t s_bad;
    if (threadIdx.x == 0) s_bad = __hip_atomic_load(ga.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t ti = *step_dev + 1;
    const double t = (double)ti;
    c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)c.b1, t)));
    c.inv_bc2 = (float)(1.0 / (1.0 - pow((double)c.b2, t)));
    __syncthreads();
    const int64_t bad = s_bad;
    if (bump && threadIdx.x == 0 && atomicAdd(&g_guard_seen, 1u) == gridDim.x - 1) {
      guard_bookkeeping(ga.w, bad, step_dev, ti);
      g_guard_seen = 0;
    }
    if (bad != -1) return;
  } else if (step_dev) {
    const int64_t ti = *step_dev + 1;
    const double t = (double)ti;
    c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)c.b1, t)));
    c.inv_bc2 = (float)(1.0 / (1.0 - pow((double)c.b2, t)));
    if (bump) {
      __syncthreads();
      if (threadIdx.x == 0 && atomicAdd(&g_adam_seen, 1u) == gridDim.x - 1) {
        *step_dev = ti;
        g_adam_seen = 0;
      }
    }
  }
  int i = 0;
  while (i + 1 < tab.n && (int)blockIdx.x >= tab.blk0[i + 1]) i++;
  const lde_adam_tensor t = tab.t[i];
  const int64_t lo = (int64_t)((int)blockIdx.x - tab.blk0[i]) * OPT_PER_WG;
  const int64_t hi = lo + OPT_PER_WG < t.n ? lo + OPT_PER_WG : t.n;
  const bool al = ((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v)) & 15) == 0;
  int64_t e = lo + 4 * (int64_t)threadIdx.x;
  if (al) {
    for (; e + 4 <= hi; e += 4 * OPT_WG) {
      f4 x = *reinterpret_cast<f4*>(t.p + e), m = *reinterpret_cast<f4*>(t.m + e), v = *reinterpret_cast<f4*>(t.v + e);
      const f4 g = *reinterpret_cast<const f4*>(t.g + e);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float xq = x[q], mq = m[q], vq = v[q];
        adam1(xq, g[q], mq, vq, c);
        x[q] = xq; m[q] = mq; v[q] = vq;
      }
      *reinterpret_cast<f4*>(t.p + e) = x;
      *reinterpret_cast<f4*>(t.m + e) = m;
      *reinterpret_cast<f4*>(t.v + e) = v;
    }
  }
  for (; e < hi; e += 4 * OPT_WG)   // unaligned arrays, and the ragged end
    for (int q = 0; q < 4 && e + q < hi; q++) adam1(t.p[e + q], t.g[e + q], t.m[e + q], t.v[e + q], c);
}

// The update of the clipped step (lde_adamw_flux_step_clipped): k_adamw_flux<true> with g ← s·g in front of adam1, s = scale[i] = what
// k_clip_finalise left for the launch's array i (memory keeps the raw g; s = 1: s·g is g bit for bit and the step is the guarded one). A
// kernel of its own and not a third instantiation: sharing the body through an inlined function changed the register assignment of the two
// existing instantiations, and they are to stay the code they were.
__global__ void __launch_bounds__(OPT_WG) k_adamw_flux_clipped(OptTable tab, OptCoef c, int64_t* __restrict__ step_dev, int bump, GuardArg<true> ga,
                                                               const float* __restrict__ scale) {
  __shared__ int64_t s_bad;
  if (threadIdx.x == 0) s_bad = __hip_atomic_load(ga.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int64_t ti = *step_dev + 1;
  const double td = (double)ti;
  c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)c.b1, td)));
  c.inv_bc2 = (float)(1.0 / (1.0 - pow((double)c.b2, td)));
  __syncthreads();
  const int64_t bad = s_bad;
  if (bump && threadIdx.x == 0 && atomicAdd(&g_guard_seen, 1u) == gridDim.x - 1) {
    guard_bookkeeping(ga.w, bad, step_dev, ti);
    g_guard_seen = 0;
  }
  if (bad != -1) return;
  int i = 0;
  while (i + 1 < tab.n && (int)blockIdx.x >= tab.blk0[i + 1]) i++;
  const lde_adam_tensor t = tab.t[i];
  const float s = scale[i];
  const int64_t lo = (int64_t)((int)blockIdx.x - tab.blk0[i]) * OPT_PER_WG;
  const int64_t hi = lo + OPT_PER_WG < t.n ? lo + OPT_PER_WG : t.n;
  const bool al = ((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v)) & 15) == 0;
  int64_t e = lo + 4 * (int64_t)threadIdx.x;
  if (al) {
    for (; e + 4 <= hi; e += 4 * OPT_WG) {
      f4 x = *reinterpret_cast<f4*>(t.p + e), m = *reinterpret_cast<f4*>(t.m + e), v = *reinterpret_cast<f4*>(t.v + e);
      const f4 g = *reinterpret_cast<const f4*>(t.g + e);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float xq = x[q], mq = m[q], vq = v[q];
        adam1(xq, s * g[q], mq, vq, c);
        x[q] = xq; m[q] = mq; v[q] = vq;
      }
      *reinterpret_cast<f4*>(t.p + e) = x;
      *reinterpret_cast<f4*>(t.m + e) = m;
      *reinterpret_cast<f4*>(t.v + e) = v;
    }
  }
  for (; e < hi; e += 4 * OPT_WG)   // unaligned arrays, and the ragged end
    for (int q = 0; q < 4 && e + q < hi; q++) adam1(t.p[e + q], s * t.g[e + q], t.m[e + q], t.v[e + q], c);
}

// The scan of the guarded step: a workgroup owns GUARD_PER_WG consecutive elements of one array's GRADIENT (the same table, packed with the
// larger slice: 4 bytes per element are read where the update moves 28). Non-finite = exponent bits all ones — NaN of any sign and payload,
// ±Inf — as an integer test, OR-ed over a lane's elements; one ballot per wave; only a wave that saw one issues a global atomicMin of the
// array's index in the caller's t[] on guard word [0] (unsigned: −1 is the largest value). A clean scan writes nothing.
__device__ __forceinline__ unsigned nonfinite(unsigned bits) { return (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }
__device__ __forceinline__ unsigned nonfinite4(u4 b) { return nonfinite(b[0]) | nonfinite(b[1]) | nonfinite(b[2]) | nonfinite(b[3]); }
__global__ void __launch_bounds__(OPT_WG) k_grad_guard(OptTable tab, OptIdx ix, unsigned long long* __restrict__ word0) {
  int i = 0;
  while (i + 1 < tab.n && (int)blockIdx.x >= tab.blk0[i + 1]) i++;
  const unsigned* g = reinterpret_cast<const unsigned*>(tab.t[i].g);
  const int64_t n = tab.t[i].n;
  const int64_t lo = (int64_t)((int)blockIdx.x - tab.blk0[i]) * GUARD_PER_WG;
  const int64_t hi = lo + GUARD_PER_WG < n ? lo + GUARD_PER_WG : n;
  unsigned bad = 0;
  int64_t e = lo + 4 * (int64_t)threadIdx.x;
  if ((((uintptr_t)g) & 15) == 0) {   // (lo is a multiple of 4: the slice keeps the array's alignment)
    constexpr int64_t S = 4 * OPT_WG;
    for (; e + (GUARD_LOADS - 1) * S + 4 <= hi; e += GUARD_LOADS * S) {   // GUARD_LOADS independent 16-byte loads in flight per lane
      u4 x[GUARD_LOADS];
#pragma unroll
      for (int k = 0; k < GUARD_LOADS; k++) x[k] = *reinterpret_cast<const u4*>(g + e + k * S);
#pragma unroll
      for (int k = 0; k < GUARD_LOADS; k++) bad |= nonfinite4(x[k]);
    }
    for (; e + 4 <= hi; e += S) bad |= nonfinite4(*reinterpret_cast<const u4*>(g + e));
  }
  for (; e < hi; e += 4 * OPT_WG)   // unaligned arrays, and the ragged end
    for (int q = 0; q < 4 && e + q < hi; q++) bad |= nonfinite(g[e + q]);
  if (__ballot(bad != 0) != 0 && (threadIdx.x & 63) == 0) atomicMin(word0, (unsigned long long)ix.idx[i]);
}

// The scan of the clipped step (lde_adamw_flux_step_clipped, include/lde.h: "the clipped step"): k_grad_guard's walk and test, and Σg² on
// the same loads. A lane adds the squares of its (at most GUARD_PER_WG / OPT_WG = 32) elements in f32; everything above the lane is f64:
// a butterfly over the wave (every lane ends with the same sum, whatever the order the waves ran in), the workgroup's waves in wave order.
// One f64 per workgroup goes to the workgroup's own slot `part[blockIdx.x]` (`part` = the launch's slot base, lde_host::clip_plan) — no
// floating-point atomic, nothing that depends on arrival order. The workgroup that owns an array's first slice also leaves the array's
// descriptor (`desc` = the launch's first ordinal) for the finalising kernel, which sees no launch's table.
using lde_host::ClipDesc;
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
__device__ __forceinline__ float sq4(float acc, u4 b) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float g = __uint_as_float(b[q]);
    acc += g * g;
  }
  return acc;
}
__global__ void __launch_bounds__(OPT_WG) k_grad_norm_guard(OptTable tab, OptIdx ix, unsigned long long* __restrict__ word0, double* __restrict__ part,
                                                            ClipDesc* __restrict__ desc, int64_t slot0) {
  __shared__ double s_wave[OPT_WG / 64];
  int i = 0;
  while (i + 1 < tab.n && (int)blockIdx.x >= tab.blk0[i + 1]) i++;
  const unsigned* g = reinterpret_cast<const unsigned*>(tab.t[i].g);
  const int64_t n = tab.t[i].n;
  const int64_t lo = (int64_t)((int)blockIdx.x - tab.blk0[i]) * GUARD_PER_WG;
  const int64_t hi = lo + GUARD_PER_WG < n ? lo + GUARD_PER_WG : n;
  unsigned bad = 0;
  float acc = 0.0f;
  int64_t e = lo + 4 * (int64_t)threadIdx.x;
  if ((((uintptr_t)g) & 15) == 0) {
    constexpr int64_t S = 4 * OPT_WG;
    for (; e + (GUARD_LOADS - 1) * S + 4 <= hi; e += GUARD_LOADS * S) {   // GUARD_LOADS independent 16-byte loads in flight per lane
      u4 x[GUARD_LOADS];
#pragma unroll
      for (int k = 0; k < GUARD_LOADS; k++) x[k] = *reinterpret_cast<const u4*>(g + e + k * S);
#pragma unroll
      for (int k = 0; k < GUARD_LOADS; k++) {
        bad |= nonfinite4(x[k]);
        acc = sq4(acc, x[k]);
      }
    }
    for (; e + 4 <= hi; e += S) {
      const u4 x = *reinterpret_cast<const u4*>(g + e);
      bad |= nonfinite4(x);
      acc = sq4(acc, x);
    }
  }
  for (; e < hi; e += 4 * OPT_WG)   // unaligned arrays, and the ragged end
    for (int q = 0; q < 4 && e + q < hi; q++) {
      const unsigned b = g[e + q];
      const float gq = __uint_as_float(b);
      bad |= nonfinite(b);
      acc += gq * gq;
    }
  if (__ballot(bad != 0) != 0 && (threadIdx.x & 63) == 0) atomicMin(word0, (unsigned long long)ix.idx[i]);
  const double w = wave_sum((double)acc);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = s_wave[0];
#pragma unroll
    for (int k = 1; k < OPT_WG / 64; k++) s += s_wave[k];
    part[blockIdx.x] = s;
    if ((int)blockIdx.x == tab.blk0[i]) {
      ClipDesc d;
      d.slot0 = slot0 + tab.blk0[i];
      d.nslots = tab.blk0[i + 1] - tab.blk0[i];
      d.idx = ix.idx[i];
      desc[i] = d;
    }
  }
}

// The finalising kernel of the clipped step: ONE workgroup, after every scan launch. A wave takes the arrays wave, wave + 4, … (ordinals:
// lde_host::clip_plan): its lanes add the array's partials lane, lane + 64, … in that order, the butterfly adds the lanes — a fixed order
// for a given table. Σ of every array goes to `sums` (f64); behind a barrier every wave adds them all in the same order (every thread
// then holds the same ΣΣ), and the threads write norms[idx] = (float)√Σ, the scale (f32, from the f32 norm: the contract of include/lde.h)
// and, for a norm that is not finite, the array's index into guard word [0] (atomicMin: the lowest wins, as in the scan).
struct ClipArg { float c; int mode; };
__global__ void __launch_bounds__(OPT_WG) k_clip_finalise(const double* __restrict__ part, double* sums, const ClipDesc* __restrict__ desc,
                                                          float* __restrict__ scale, int64_t nne, int n, float* __restrict__ norms, ClipArg a,
                                                          unsigned long long* __restrict__ word0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < n; i += OPT_WG) norms[i] = 0.0f;   // (the empty arrays keep this)
  for (int64_t k = wave; k < nne; k += OPT_WG / 64) {
    const ClipDesc d = desc[k];
    double s = 0.0;
    for (int j = lane; j < d.nslots; j += 64) s += part[d.slot0 + j];
    s = wave_sum(s);
    if (lane == 0) sums[k] = s;
  }
  __syncthreads();
  double tot = 0.0;
  for (int64_t k = lane; k < nne; k += 64) tot += sums[k];
  tot = wave_sum(tot);
  const float gn = (float)sqrt(tot);
  int any_bad = 0;
  for (int64_t k = threadIdx.x; k < nne; k += OPT_WG) {
    const float ni = (float)sqrt(sums[k]);
    const int idx = desc[k].idx;
    norms[idx] = ni;
    scale[k] = a.mode == LDE_CLIP_GLOBAL ? fminf(1.0f, a.c / (gn + 1e-6f)) : (ni > a.c ? a.c / ni : 1.0f);
    if (!isfinite(ni)) {
      any_bad = 1;
      atomicMin(word0, (unsigned long long)idx);
    }
  }
  any_bad = __syncthreads_or(any_bad);
  if (threadIdx.x == 0) {
    norms[n] = gn;
    if (a.mode == LDE_CLIP_GLOBAL && !any_bad && !isfinite(gn)) atomicMin(word0, (unsigned long long)desc[0].idx);   // (ΣΣ alone beyond f32)
  }
}

// ---- the AdaBelief step (lde_adabelief_flux_step*, include/lde.h: "the AdaBelief step"): Flux's `Optimiser(AdaBelief(η, β), WeightDecay(decay))`,
// the optimiser the reference's scripts name as the alternative [REF examples/pendulum_friction-less/model_train.jl:136-138]:
//     m ← β₁·m + (1 − β₁)·g;   s ← β₂·s + (1 − β₂)·(g − m)² + ε_var  (the NEW m);   Δ = η·(m/(1 − β₁ᵗ))/(√(s/(1 − β₂ᵗ)) + ε_den) + decay·x;   x ← x − Δ
// k_adamw_flux's geometry — the same table, a workgroup owns 2048 consecutive elements of one array, 16-byte accesses when all four
// pointers are aligned, the scalar path for unaligned arrays and the ragged end, 28 bytes per element (`v` of the table holds s) — and
// its three forms as ONE template (these kernels are new: they may share a body, see the comment above k_adamw_flux_clipped):
// BELIEF_PLAIN (step_dev == nullptr: the coefficients arrive complete; otherwise the device-counted form), BELIEF_GUARDED (word [0] read
// once per workgroup, the last workgroup of the last launch does guard_bookkeeping), BELIEF_CLIPPED (guarded, with g ← scale[i]·g as it
// is loaded). The scans in front of the guarded and clipped forms are k_grad_guard / k_grad_norm_guard / k_clip_finalise themselves.
// The counting-in has counters of its own, one per form: a step of this rule and an ADAMW step on another stream do not meet in one.
// The arithmetic is written out operation by operation (two fused multiply-adds where the rule has a·b + c·d, nothing else contracted),
// so that the three forms round alike: a clean guarded step is the device-counted one bit for bit, a clipped one with s = 1 the guarded.
enum { BELIEF_PLAIN = 0, BELIEF_GUARDED = 1, BELIEF_CLIPPED = 2 };
struct BeliefCoef { float b1, b2, omb1, omb2, inv_bc1, inv_bc2, eps_var, eps_den, lr, decay; };

__device__ __forceinline__ void belief1(float& x, float g, float& m, float& s, const BeliefCoef& c) {
#pragma clang fp contract(off)
  m = __builtin_fmaf(c.b1, m, c.omb1 * g);
  const float d = g - m;
  s = __builtin_fmaf(c.b2, s, c.omb2 * d * d) + c.eps_var;
  const float q = (m * c.inv_bc1) / (__builtin_sqrtf(s * c.inv_bc2) + c.eps_den);
  x -= __builtin_fmaf(q, c.lr, c.decay * x);
}

__device__ unsigned g_belief_seen[3] = {0, 0, 0};
template <int FORM>
__global__ void __launch_bounds__(OPT_WG) k_adabelief_flux(OptTable tab, BeliefCoef c, int64_t* __restrict__ step_dev, int bump, int64_t* gw,
                                                           const float* __restrict__ scale) {
  if constexpr (FORM != BELIEF_PLAIN) {
    __shared__ int64_t s_bad;
    if (threadIdx.x == 0) s_bad = __hip_atomic_load(gw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t ti = *step_dev + 1;
    const double td = (double)ti;
    c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)c.b1, td)));
    c.inv_bc2 = (float)(1.0 / (1.0 - pow((double)c.b2, td)));
    __syncthreads();
    const int64_t bad = s_bad;
    if (bump && threadIdx.x == 0 && atomicAdd(&g_belief_seen[FORM], 1u) == gridDim.x - 1) {
      guard_bookkeeping(gw, bad, step_dev, ti);
      g_belief_seen[FORM] = 0;
    }
    if (bad != -1) return;
  } else if (step_dev) {
    const int64_t ti = *step_dev + 1;
    const double td = (double)ti;
    c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)c.b1, td)));
    c.inv_bc2 = (float)(1.0 / (1.0 - pow((double)c.b2, td)));
    if (bump) {
      __syncthreads();
      if (threadIdx.x == 0 && atomicAdd(&g_belief_seen[FORM], 1u) == gridDim.x - 1) {
        *step_dev = ti;
        g_belief_seen[FORM] = 0;
      }
    }
  }
  int i = 0;
  while (i + 1 < tab.n && (int)blockIdx.x >= tab.blk0[i + 1]) i++;
  const lde_adam_tensor t = tab.t[i];
  float sc = 1.0f;
  if constexpr (FORM == BELIEF_CLIPPED) sc = scale[i];
  const int64_t lo = (int64_t)((int)blockIdx.x - tab.blk0[i]) * OPT_PER_WG;
  const int64_t hi = lo + OPT_PER_WG < t.n ? lo + OPT_PER_WG : t.n;
  const bool al = ((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v)) & 15) == 0;
  int64_t e = lo + 4 * (int64_t)threadIdx.x;
  if (al) {
    for (; e + 4 <= hi; e += 4 * OPT_WG) {
      f4 x = *reinterpret_cast<f4*>(t.p + e), m = *reinterpret_cast<f4*>(t.m + e), v = *reinterpret_cast<f4*>(t.v + e);
      const f4 g = *reinterpret_cast<const f4*>(t.g + e);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float xq = x[q], mq = m[q], vq = v[q];
        belief1(xq, FORM == BELIEF_CLIPPED ? sc * g[q] : g[q], mq, vq, c);
        x[q] = xq; m[q] = mq; v[q] = vq;
      }
      *reinterpret_cast<f4*>(t.p + e) = x;
      *reinterpret_cast<f4*>(t.m + e) = m;
      *reinterpret_cast<f4*>(t.v + e) = v;
    }
  }
  for (; e < hi; e += 4 * OPT_WG)   // unaligned arrays, and the ragged end
    for (int q = 0; q < 4 && e + q < hi; q++) belief1(t.p[e + q], FORM == BELIEF_CLIPPED ? sc * t.g[e + q] : t.g[e + q], t.m[e + q], t.v[e + q], c);
}

}  // namespace lde

using namespace lde;

static OptTable opt_table(const lde_adam_tensor* t, const lde_host::OptLaunch& L) {
  OptTable tab;
  tab.n = L.n;
  for (int i = 0; i < L.n; i++) tab.t[i] = t[L.idx[i]];
  for (int i = 0; i <= L.n; i++) tab.blk0[i] = L.blk0[i];
  return tab;
}

static OptCoef opt_coef(float lr, float beta1, float beta2, float eps, float decay, int64_t step, const int64_t* step_dev) {
  OptCoef c;
  c.b1 = beta1; c.b2 = beta2; c.omb1 = 1.0f - beta1; c.omb2 = 1.0f - beta2; c.eps = eps; c.lr = lr; c.decay = decay;
  c.inv_bc1 = (float)(1.0 / (1.0 - __builtin_pow((double)beta1, (double)(step_dev ? 1 : step))));   // Flux carries β₁ᵗ, β₂ᵗ as a running product
  c.inv_bc2 = (float)(1.0 / (1.0 - __builtin_pow((double)beta2, (double)(step_dev ? 1 : step))));
  return c;
}

// The plan of the host-counted, device-counted and guarded forms, for either rule: `update(L, bump)` enqueues the rule's update kernel for
// the launch L (`bump`: the step's last launch of a device-counted form — its last workgroup advances the count).
template <bool GUARD, class Update>
static int opt_impl(int n, const lde_adam_tensor* t, float beta1, float beta2, int64_t step, int64_t* step_dev, int64_t* guard_dev, void* stream,
                    Update&& update) {
  if (!lde_host::opt_args_ok(n, t, beta1, beta2, step, step_dev)) return LDE_ERR_INVALID_ARG;
  if constexpr (GUARD) {
    // ALL scan launches go first — after a look at the update's plan: a call that will be refused launches nothing
    for (int first = 0; first < n;) {
      const lde_host::OptLaunch L = lde_host::opt_next_launch(n, t, first, OPT_PER_WG);
      if (L.too_large) return LDE_ERR_INVALID_ARG;
      if (L.n == 0) break;
      first = L.next;
    }
    for (int first = 0; first < n;) {
      const lde_host::OptLaunch L = lde_host::opt_next_launch(n, t, first, GUARD_PER_WG);
      if (L.n == 0) break;   // (never too_large: the update's plan, with the smaller slice, fits)
      first = L.next;
      OptIdx ix;
      for (int i = 0; i < L.n; i++) ix.idx[i] = L.idx[i];
      hipLaunchKernelGGL(k_grad_guard, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, (hipStream_t)stream, opt_table(t, L), ix, (unsigned long long*)guard_dev);
      if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
    }
  }
  bool launched = false;
  for (int first = 0; first < n;) {
    const lde_host::OptLaunch L = lde_host::opt_next_launch(n, t, first, OPT_PER_WG);
    first = L.next;
    if (L.n == 0) {
      if (L.too_large) return LDE_ERR_INVALID_ARG;   // a single array beyond 2³⁰ workgroups
      break;
    }
    launched = true;
    update(L, (step_dev && L.last) ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
  }
  if (step_dev && !launched) {
    if constexpr (GUARD) hipLaunchKernelGGL(k_adam_tick_guarded, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, guard_dev);
    else hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
    if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
  }
  return LDE_OK;
}
template <bool GUARD>
static int adamw_impl(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps, float decay, int64_t step,
                      int64_t* step_dev, int64_t* guard_dev, void* stream) {
  const OptCoef c = opt_coef(lr, beta1, beta2, eps, decay, step, step_dev);
  GuardArg<GUARD> ga;
  if constexpr (GUARD) ga.w = guard_dev;
  return opt_impl<GUARD>(n, t, beta1, beta2, step, step_dev, guard_dev, stream, [&](const lde_host::OptLaunch& L, int bump) {
    hipLaunchKernelGGL(k_adamw_flux<GUARD>, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, (hipStream_t)stream, opt_table(t, L), c, step_dev, bump, ga);
  });
}

// The clipped step: every scan launch, the finalising kernel, every update launch — in that order on one stream (lde_host::clip_plan says
// where each scan launch's partials and descriptors go; the update's launches meet the non-empty arrays in the same order, so launch
// by launch they take the next L.n scales).
// `update(L, bump, scale)` enqueues the rule's clipped update kernel for the launch L, `scale` = the scales of ITS arrays.
template <class Update>
static int opt_clipped(int n, const lde_adam_tensor* t, float clip_norm, int clip_mode, int64_t* step_dev, int64_t* guard_dev, void* ws_dev,
                       float* norms_dev, hipStream_t stream, Update&& update) {
  const lde_host::ClipWs w = lde_host::clip_plan(n, t, [](const lde_host::OptLaunch&, int64_t, int64_t) {});
  char* const ws = static_cast<char*>(ws_dev);
  double* const part = w.nne ? reinterpret_cast<double*>(ws) : nullptr;
  double* const sums = w.nne ? reinterpret_cast<double*>(ws + w.off_sums) : nullptr;
  ClipDesc* const desc = w.nne ? reinterpret_cast<ClipDesc*>(ws + w.off_desc) : nullptr;
  float* const scale = w.nne ? reinterpret_cast<float*>(ws + w.off_scale) : nullptr;
  unsigned long long* const word0 = reinterpret_cast<unsigned long long*>(guard_dev);
  int rc = LDE_OK;
  lde_host::clip_plan(n, t, [&](const lde_host::OptLaunch& L, int64_t slot0, int64_t ord0) {
    if (rc != LDE_OK) return;
    OptIdx ix;
    for (int i = 0; i < L.n; i++) ix.idx[i] = L.idx[i];
    hipLaunchKernelGGL(k_grad_norm_guard, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, stream, opt_table(t, L), ix, word0, part + slot0, desc + ord0, slot0);
    if (hipGetLastError() != hipSuccess) rc = LDE_ERR_HIP;
  });
  if (rc != LDE_OK) return rc;
  ClipArg a;
  a.c = clip_norm; a.mode = clip_mode;
  hipLaunchKernelGGL(k_clip_finalise, dim3(1), dim3(OPT_WG), 0, stream, part, sums, desc, scale, w.nne, n, norms_dev, a, word0);
  if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
  int64_t ord0 = 0;
  for (int first = 0; first < n;) {
    const lde_host::OptLaunch L = lde_host::opt_next_launch(n, t, first, OPT_PER_WG);
    first = L.next;
    if (L.n == 0) break;
    update(L, L.last ? 1 : 0, scale + ord0);
    if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
    ord0 += L.n;
  }
  if (w.nne == 0) {
    hipLaunchKernelGGL(k_adam_tick_guarded, dim3(1), dim3(1), 0, stream, step_dev, guard_dev);
    if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
  }
  return LDE_OK;
}

extern "C" size_t lde_clip_ws_bytes(int n, const lde_adam_tensor* t) {
  if (n <= 0 || !t) return 0;
  return lde_host::clip_plan(n, t, [](const lde_host::OptLaunch&, int64_t, int64_t) {}).bytes;
}
extern "C" int lde_adamw_flux_step_clipped(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps, float decay,
                                           float clip_norm, int clip_mode, int64_t* step_dev, int64_t* guard_dev, void* ws_dev,
                                           float* norms_dev, void* stream) {
  if (!lde_host::clip_args_ok(n, t, beta1, beta2, clip_norm, clip_mode, step_dev, guard_dev, ws_dev, norms_dev)) return LDE_ERR_INVALID_ARG;
  const OptCoef c = opt_coef(lr, beta1, beta2, eps, decay, 0, step_dev);
  GuardArg<true> ga;
  ga.w = guard_dev;
  return opt_clipped(n, t, clip_norm, clip_mode, step_dev, guard_dev, ws_dev, norms_dev, (hipStream_t)stream,
                     [&](const lde_host::OptLaunch& L, int bump, const float* scale) {
                       hipLaunchKernelGGL(k_adamw_flux_clipped, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, (hipStream_t)stream, opt_table(t, L), c, step_dev, bump, ga, scale);
                     });
}

extern "C" int lde_adamw_flux_step(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps, float decay,
                                   int64_t step, void* stream) {
  return adamw_impl<false>(n, t, lr, beta1, beta2, eps, decay, step, nullptr, nullptr, stream);
}
extern "C" int lde_adamw_flux_step_dev(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps, float decay,
                                       int64_t* step_dev, void* stream) {
  if (!step_dev) return LDE_ERR_INVALID_ARG;
  return adamw_impl<false>(n, t, lr, beta1, beta2, eps, decay, 0, step_dev, nullptr, stream);
}
extern "C" int lde_guard_init(int64_t* guard_dev, void* stream) {
  if (!guard_dev) return LDE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_guard_init, dim3(1), dim3(1), 0, (hipStream_t)stream, guard_dev);
  return hipGetLastError() != hipSuccess ? LDE_ERR_HIP : LDE_OK;
}
extern "C" int lde_adamw_flux_step_guarded(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps, float decay,
                                           int64_t* step_dev, int64_t* guard_dev, void* stream) {
  if (!step_dev || !guard_dev) return LDE_ERR_INVALID_ARG;
  return adamw_impl<true>(n, t, lr, beta1, beta2, eps, decay, 0, step_dev, guard_dev, stream);
}

// ---- the AdaBelief step: the four forms of the ADAMW step, through the same plans
static BeliefCoef belief_coef(float lr, float beta1, float beta2, float eps_var, float eps_den, float decay, int64_t step, const int64_t* step_dev) {
  BeliefCoef c;
  c.b1 = beta1; c.b2 = beta2; c.omb1 = 1.0f - beta1; c.omb2 = 1.0f - beta2; c.eps_var = eps_var; c.eps_den = eps_den; c.lr = lr; c.decay = decay;
  c.inv_bc1 = (float)(1.0 / (1.0 - __builtin_pow((double)beta1, (double)(step_dev ? 1 : step))));
  c.inv_bc2 = (float)(1.0 / (1.0 - __builtin_pow((double)beta2, (double)(step_dev ? 1 : step))));
  return c;
}
template <bool GUARD>
static int belief_impl(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps_var, float eps_den, float decay, int64_t step,
                       int64_t* step_dev, int64_t* guard_dev, void* stream) {
  if (!lde_host::belief_eps_ok(eps_var, eps_den)) return LDE_ERR_INVALID_ARG;
  const BeliefCoef c = belief_coef(lr, beta1, beta2, eps_var, eps_den, decay, step, step_dev);
  return opt_impl<GUARD>(n, t, beta1, beta2, step, step_dev, guard_dev, stream, [&](const lde_host::OptLaunch& L, int bump) {
    hipLaunchKernelGGL(k_adabelief_flux<GUARD ? BELIEF_GUARDED : BELIEF_PLAIN>, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, (hipStream_t)stream, opt_table(t, L), c,
                       step_dev, bump, guard_dev, (const float*)nullptr);
  });
}
extern "C" int lde_adabelief_flux_step(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps_var, float eps_den, float decay,
                                       int64_t step, void* stream) {
  return belief_impl<false>(n, t, lr, beta1, beta2, eps_var, eps_den, decay, step, nullptr, nullptr, stream);
}
extern "C" int lde_adabelief_flux_step_dev(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps_var, float eps_den,
                                           float decay, int64_t* step_dev, void* stream) {
  if (!step_dev) return LDE_ERR_INVALID_ARG;
  return belief_impl<false>(n, t, lr, beta1, beta2, eps_var, eps_den, decay, 0, step_dev, nullptr, stream);
}
extern "C" int lde_adabelief_flux_step_guarded(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps_var, float eps_den,
                                               float decay, int64_t* step_dev, int64_t* guard_dev, void* stream) {
  if (!step_dev || !guard_dev) return LDE_ERR_INVALID_ARG;
  return belief_impl<true>(n, t, lr, beta1, beta2, eps_var, eps_den, decay, 0, step_dev, guard_dev, stream);
}
extern "C" int lde_adabelief_flux_step_clipped(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps_var, float eps_den,
                                               float decay, float clip_norm, int clip_mode, int64_t* step_dev, int64_t* guard_dev, void* ws_dev,
                                               float* norms_dev, void* stream) {
  if (!lde_host::belief_eps_ok(eps_var, eps_den)) return LDE_ERR_INVALID_ARG;
  if (!lde_host::clip_args_ok(n, t, beta1, beta2, clip_norm, clip_mode, step_dev, guard_dev, ws_dev, norms_dev)) return LDE_ERR_INVALID_ARG;
  const BeliefCoef c = belief_coef(lr, beta1, beta2, eps_var, eps_den, decay, 0, step_dev);
  return opt_clipped(n, t, clip_norm, clip_mode, step_dev, guard_dev, ws_dev, norms_dev, (hipStream_t)stream,
                     [&](const lde_host::OptLaunch& L, int bump, const float* scale) {
                       hipLaunchKernelGGL(k_adabelief_flux<BELIEF_CLIPPED>, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, (hipStream_t)stream, opt_table(t, L), c,
                                          step_dev, bump, guard_dev, scale);
                     });
}
