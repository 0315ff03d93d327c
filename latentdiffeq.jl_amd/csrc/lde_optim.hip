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

}  // namespace lde

using namespace lde;

static OptTable opt_table(const lde_adam_tensor* t, const lde_host::OptLaunch& L) {
  OptTable tab;
  tab.n = L.n;
  for (int i = 0; i < L.n; i++) tab.t[i] = t[L.idx[i]];
  for (int i = 0; i <= L.n; i++) tab.blk0[i] = L.blk0[i];
  return tab;
}

template <bool GUARD>
static int adamw_impl(int n, const lde_adam_tensor* t, float lr, float beta1, float beta2, float eps, float decay, int64_t step,
                      int64_t* step_dev, int64_t* guard_dev, void* stream) {
  if (n < 0 || (n > 0 && !t) || (!step_dev && step < 1) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return LDE_ERR_INVALID_ARG;
  for (int i = 0; i < n; i++)
    if (t[i].n < 0 || (t[i].n > 0 && (!t[i].p || !t[i].g || !t[i].m || !t[i].v))) return LDE_ERR_INVALID_ARG;
  OptCoef c;
  c.b1 = beta1; c.b2 = beta2; c.omb1 = 1.0f - beta1; c.omb2 = 1.0f - beta2; c.eps = eps; c.lr = lr; c.decay = decay;
  c.inv_bc1 = (float)(1.0 / (1.0 - __builtin_pow((double)beta1, (double)(step_dev ? 1 : step))));   // Flux carries β₁ᵗ, β₂ᵗ as a running product
  c.inv_bc2 = (float)(1.0 / (1.0 - __builtin_pow((double)beta2, (double)(step_dev ? 1 : step))));
  GuardArg<GUARD> ga;
  if constexpr (GUARD) {
    ga.w = guard_dev;
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
    hipLaunchKernelGGL(k_adamw_flux<GUARD>, dim3(L.blk0[L.n]), dim3(OPT_WG), 0, (hipStream_t)stream, opt_table(t, L), c, step_dev, (step_dev && L.last) ? 1 : 0, ga);
    if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
  }
  if (step_dev && !launched) {
    if constexpr (GUARD) hipLaunchKernelGGL(k_adam_tick_guarded, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, guard_dev);
    else hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
    if (hipGetLastError() != hipSuccess) return LDE_ERR_HIP;
  }
  return LDE_OK;
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
