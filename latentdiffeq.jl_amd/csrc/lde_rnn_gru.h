// lde_rnn_gru.h — the GRU cell of the recurrent pattern extractor (LDE_CELL_GRU, include/lde.h), included by lde_rnn.hip.
//
// Flux 0.13.6 GRUCell ("GRU v1"):  r = σ(gx₁ + gh₁ + b₁), z = σ(gx₂ + gh₂ + b₂), n = tanh(gx₃ + r ⊙ gh₃ + b₃), h′ = (1 − z) ⊙ n + z ⊙ h,
// gx = Wi·x, gh = Wh·h. Two things set it apart from the LSTM: the candidate needs the x part and the h part of its row SEPARATELY, and the
// weight gradient is not one outer product per row (Wh₃ sees dn·r where Wi₃ and b₃ see dn). Both are met by running the cell as P = 4h
// PSEUDO-ROWS (r, z, n_x, n_h): n_x = [Wi₃ | 0] with the bias, n_h = [0 | Wh₃] without one. A step is then what the LSTM's is — one dot
// product of an LDS (or register) row with [x; h] per pseudo-row, the unit lanes combine four pre-activations — the pre-activation of n_h IS
// gh₃ (kept in the record beside r, z, n), and with the deltas (dr, dz, dn, dn·r) both [d_in; dh_prev] = Wᵀδ (+ dh′·z) and the staged
// (a, δ) panels of the weight gradient are the plain products again: k_mlp_dw serves unchanged on a [K → 4h] layer, and k_gru_gather moves
// its [4h × K] + [4h] result into the cell's flat order (lde_host::gru_staged_index; the structural zeros are never read).
// For h = 16 that is exactly the LSTM's 64-row footprint. Above 64 pseudo-rows (h > 16) a lane owns several: Hp = 64, rows u, u + 64, … —
// in the run-time-shaped kernel only. A body of its own: the RNN / LSTM kernels (rnn_body) keep their code, registers and bits.
// Mapping, staging, prefetch and the four modes are rnn_body's (see there); what differs is marked. The one-wave-per-cell pipeline of the
// 32 → 16 → 16 stacks (rnn_pipe_wave in lde_rnn.hip) has compile-time branches for the cell: same formulas in the same order, same bits.
#pragma once

namespace lde {

// weights → LDS as pseudo-rows of [Wi | Wh] (zero where a pseudo-row has no part), biases (none for n_h), state0
__device__ __forceinline__ void gru_load_weights(const RnnDims& rd, const float* Wflat, float* lw, int nthr, bool transposed) {
  const int tid = threadIdx.x;
  for (int i = tid; i < rd.lds_w; i += nthr) lw[i] = 0.f;
  __syncthreads();
  for (int l = 0; l < rd.nL; l++) {
    const int in = rd.sizes[l], h = rd.sizes[l + 1], R = 3 * h, ldk = rd.ldk[l];
    const float* Wi = Wflat + rd.f_off[l];
    const float* Wh = Wi + (size_t)R * in;
    const float* b = Wh + (size_t)R * h;
    const float* s0 = b + R;
    const bool wt = transposed && rd.wt;
    for (int e = tid; e < R * in; e += nthr) {   // rows r, z, n of Wi → pseudo-rows r, z, n_x
      const int k = e / R, p = e - k * R;
      const float w = Wi[e];
      lw[rd.w_off[l] + p * ldk + k] = w;
      if (wt) lw[rd.wt_off[l] + k * rd.ldr[l] + p] = w;
    }
    for (int e = tid; e < R * h; e += nthr) {    // rows r, z, n of Wh → pseudo-rows r, z, n_h
      const int k = e / R, r = e - k * R, p = r < 2 * h ? r : r + h;
      const float w = Wh[e];
      lw[rd.w_off[l] + p * ldk + in + k] = w;
      if (wt) lw[rd.wt_off[l] + (in + k) * rd.ldr[l] + p] = w;
    }
    for (int e = tid; e < R; e += nthr) lw[rd.b_off[l] + e] = b[e];
    for (int e = tid; e < h; e += nthr) lw[rd.s_off[l] + e] = s0[e];
  }
  __syncthreads();
}

// SP: the instantiation for 32 → 16 → 16 (64 pseudo-rows = 64 lanes per trajectory; MODE_ compile-time; REGW: weight rows in registers,
// one wave per workgroup). !SP: any shape at run time (mode from the arguments).
template <bool SP, int MODE_, bool REGW>
__device__ __forceinline__ void gru_body(const RnnDims& rd, const RnnArgs& a, const unsigned bx) {
  extern __shared__ __attribute__((aligned(16))) float rsm[];
  static_assert(!REGW || SP, "register-resident weights need a compile-time shape");
  constexpr int IN0_ = 32, H_ = 16, L_ = 2;
  constexpr int UL = SP ? L_ : 1, UK = SP ? 16 : 4;
  const int L = SP ? L_ : rd.nL;
  const int Hp = SP ? 64 : rd.Hp, hmaxv = SP ? H_ : rd.hmax;
  auto size_of = [&](int l) { return SP ? (l == 0 ? IN0_ : H_) : rd.sizes[l]; };
  auto ldk_of = [&](int l) { return SP ? rnn_ldk(size_of(l) + size_of(l + 1)) : rd.ldk[l]; };
  const int tpw = a.tpw, nthr = tpw * Hp, tid = threadIdx.x, tr = tid / Hp, u = tid - tr * Hp;
  const int T = a.T, B = a.B;
  const int mode = SP ? MODE_ : a.mode;
  float* lw = rsm;
  float* vbuf = lw + rd.lds_w + tr * rd.vmax;                     // this trajectory's [x; h_prev]
  float* dbuf = lw + rd.lds_w + tpw * rd.vmax + tr * rd.rmax;      // its pseudo-row pre-activations / deltas
  float* hst = lw + rd.lds_w + tpw * (rd.vmax + rd.rmax) + tr * (2 * L * hmaxv);   // h[l][hmax]
  float* dhs = lw + rd.lds_w + tpw * (rd.vmax + rd.rmax + 2 * L * hmaxv) + tr * (2 * L * hmaxv);   // dh, then dh′·z
  float* dzs = dhs + L * hmaxv;
  const bool keep = mode == 1 || mode == 2, bptt = mode == 1 || mode == 3;
  gru_load_weights(rd, a.Wflat, lw, nthr, bptt);
  constexpr int KF4 = REGW ? (IN0_ + H_ + 3) / 4 : 1;
  constexpr int RB4 = REGW ? (4 * H_ + 3) / 4 : 1;
  constexpr int NKI = REGW ? (IN0_ + H_ + 63) / 64 : 1;
  f32x4 wrow[REGW ? L_ : 1][KF4];
  constexpr bool BP = MODE_ == 1 || MODE_ == 3;
  f32x4 wcol[(REGW && BP) ? L_ : 1][(REGW && BP) ? NKI : 1][(REGW && BP) ? RB4 : 1];
  if (REGW) {
#pragma unroll
    for (int l = 0; l < (REGW ? L_ : 0); l++) {
      const int K = size_of(l) + size_of(l + 1), ldk = ldk_of(l), Pl = 4 * size_of(l + 1);
      const float* wr = lw + rd.w_off[l] + (u < Pl ? u : 0) * ldk;
#pragma unroll
      for (int k4 = 0; k4 < KF4; k4++)
        wrow[l][k4] = (u < Pl && 4 * k4 < K) ? *reinterpret_cast<const f32x4*>(wr + 4 * k4) : f32x4{0.f, 0.f, 0.f, 0.f};
      if (BP) {
        const int ldr = rnn_ldk(Pl);
#pragma unroll
        for (int q = 0; q < ((REGW && BP) ? NKI : 0); q++) {
          const int k = u + q * 64;
          const float* wk = lw + rd.wt_off[l] + (k < K ? k : 0) * ldr;
#pragma unroll
          for (int r4 = 0; r4 < RB4; r4++)
            wcol[l][q][r4] = (k < K && 4 * r4 < Pl) ? *reinterpret_cast<const f32x4*>(wk + 4 * r4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  }
  const long long b = (long long)bx * tpw + tr;
  const bool valid = b < B;
  const size_t tile = (size_t)(b >> 4);
  const int row = (int)(b & 15);
  const int in0 = size_of(0);
  const size_t bc = (size_t)(valid ? b : B - 1);   // (a trajectory past B computes on a copy of trajectory B−1 and stores nothing)

  // ---- forward sweep ----------------------------------------------------------------------------------------------------
  if (mode != 3) {
#pragma unroll UL
    for (int l = 0; l < L; l++) {
      const int h = size_of(l + 1);
      if (u < h) hst[l * hmaxv + u] = lw[rd.s_off[l] + u];
    }
    constexpr int XQ = 4;
    float xq[XQ];
    auto fetch_x = [&](int s) {   // branch-free, always in bounds (rnn_body)
      const int t = rd.reverse ? T - 1 - s : s;
#pragma unroll
      for (int q = 0; q < XQ; q++) {
        const int k = u + q * Hp;
        if (SP && k >= in0) { xq[q] = 0.f; continue; }
        xq[q] = a.x[(size_t)in0 * (bc + (size_t)B * t) + (k < in0 ? k : in0 - 1)];
      }
    };
    fetch_x(0);
    for (int s = 0; s < T; s++) {
      const int t = rd.reverse ? T - 1 - s : s;
#pragma unroll UL
      for (int l = 0; l < L; l++) {
        const int in = size_of(l), h = size_of(l + 1), K = in + h, ldk = ldk_of(l), Pl = 4 * h;
        if (l == 0) {
#pragma unroll
          for (int q = 0; q < XQ; q++)
            if (u + q * Hp < in) vbuf[u + q * Hp] = xq[q];
          for (int k = u + XQ * Hp; k < in; k += Hp) vbuf[k] = a.x[(size_t)in0 * (bc + (size_t)B * t) + k];
          fetch_x(s + 1 < T ? s + 1 : s);
        } else {
          for (int k = u; k < in; k += Hp) vbuf[k] = hst[(l - 1) * hmaxv + k];
        }
        for (int k = u; k < h; k += Hp) vbuf[in + k] = hst[l * hmaxv + k];
        for (int k = K + u; k < ((K + 3) & ~3); k += Hp) vbuf[k] = 0.f;
        if (keep) {
          float* ga = a.stage[l] + (tile * T + s) * a.blk[l] + row * pad32(K);
          for (int k = u; k < pad32(K); k += Hp) ga[k] = (valid && k < K) ? vbuf[k] : 0.f;
        }
        // one lane per pseudo-row (several rows per lane above 64 of them): pre_p = b_p + row_p · [x; h]
        if (REGW) {
          f32x2 c01 = {0.f, 0.f}, c23 = {0.f, 0.f};
#pragma unroll
          for (int k4 = 0; k4 < KF4; k4++) {
            if (4 * k4 < K) {
              const f32x4 xv = *reinterpret_cast<const f32x4*>(vbuf + 4 * k4);
              c01 += wrow[REGW ? l : 0][k4].lo * xv.lo;
              c23 += wrow[REGW ? l : 0][k4].hi * xv.hi;
            }
          }
          dbuf[u] = lw[rd.b_off[l] + u] + ((c01.x + c01.y) + (c23.x + c23.y));
        } else {
          const int K4 = (K + 3) >> 2;
          for (int p = u; p < Pl; p += Hp) {
            const float* wr = lw + rd.w_off[l] + p * ldk;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll UK
            for (int k4 = 0; k4 < K4; k4++)
              acc += *reinterpret_cast<const f32x4*>(wr + 4 * k4) * *reinterpret_cast<const f32x4*>(vbuf + 4 * k4);
            dbuf[p] = lw[rd.b_off[l] + p] + ((acc[0] + acc[1]) + (acc[2] + acc[3]));
          }
        }
        if (u < h) {
          const float rg = sigm(dbuf[u]), zg = sigm(dbuf[h + u]), gh = dbuf[3 * h + u];   // (n_h has no bias: its pre-activation is Wh₃·h)
          const float ng = fast_tanh(__builtin_fmaf(rg, gh, dbuf[2 * h + u]));
          const float hn = __builtin_fmaf(zg, hst[l * hmaxv + u] - ng, ng);                 // (1 − z)·n + z·h
          if (keep && valid) {
            float* r = a.rec + (((size_t)s * L + l) * B + (size_t)b) * rd.recw;
            r[u] = rg;
            r[h + u] = zg;
            r[2 * h + u] = ng;
            r[3 * h + u] = gh;
            r[4 * h + u] = hn;
          }
          hst[l * hmaxv + u] = hn;   // every lane of the trajectory has copied h_prev into vbuf already (same wave, in order)
        }
      }
    }
    if (mode == 0 || mode == 2) {
      const int hL = size_of(L);
      if (valid && u < hL) a.y[(size_t)a.ldy * b + u] = hst[(L - 1) * hmaxv + u];
      return;
    }
  }   // (mode 3 starts here)
  __syncthreads();   // the records are read back below by other lanes of the trajectory: stores drained first

  // ---- back-propagation through time -----------------------------------------------------------------------------------
#pragma unroll UL
  for (int l = 0; l < L; l++) {
    const int h = size_of(l + 1);
    if (u < h) {
      dhs[l * hmaxv + u] = (l == L - 1 && valid) ? rnn_dy(a, b, u) : 0.f;
      dzs[l * hmaxv + u] = 0.f;
    }
  }
  float rq[5];   // r, z, n, Wh₃·h, h_prev
  auto fetch_rec = [&](int s, int l) {   // branch-free; h_prev of step 0 (the trainable state0) is patched in at the use
    const int h = size_of(l + 1);
    const int uc = u < h ? u : h - 1;
    const float* r = a.rec + (((size_t)s * L + l) * B + bc) * rd.recw;
#pragma unroll
    for (int g = 0; g < 4; g++) rq[g] = r[g * h + uc];
    rq[4] = a.rec[(((size_t)(s > 0 ? s - 1 : 0) * L + l) * B + bc) * rd.recw + 4 * h + uc];
  };
  fetch_rec(T - 1, L - 1);
  for (int s = T - 1; s >= 0; s--) {
    const int t = rd.reverse ? T - 1 - s : s;
    if (u == 0) a.wts[(tile * T + s) * NB + row] = valid ? 1.f : 0.f;
#pragma unroll UL
    for (int l = L - 1; l >= 0; l--) {
      const int in = size_of(l), h = size_of(l + 1), K = in + h, R = 4 * h, ldk = ldk_of(l);
      const int K32 = pad32(K), R32 = pad32(R);
      float cur[5];
#pragma unroll
      for (int q = 0; q < 5; q++) cur[q] = rq[q];
      if (l > 0) fetch_rec(s, l - 1);
      else fetch_rec(s > 0 ? s - 1 : 0, L - 1);
      if (u < h) {   // pseudo-row deltas of this lane's unit: (dr, dz, dn, dn·r)
        const float dh = dhs[l * hmaxv + u];
        const float rg = cur[0], zg = cur[1], ng = cur[2], gh = cur[3];
        const float hp = s > 0 ? cur[4] : lw[rd.s_off[l] + u];
        const float dn = dh * (1.f - zg) * __builtin_fmaf(-ng, ng, 1.f);
        dbuf[u] = dn * gh * rg * (1.f - rg);
        dbuf[h + u] = dh * (hp - ng) * zg * (1.f - zg);
        dbuf[2 * h + u] = dn;
        dbuf[3 * h + u] = dn * rg;
        dzs[l * hmaxv + u] = dh * zg;   // the direct path h → h′
      }
      {
        float* gd = a.stage[l] + (tile * T + s) * a.blk[l] + NB * K32 + row * R32;
        for (int k = u; k < R32; k += Hp) gd[k] = (valid && k < R) ? dbuf[k] : 0.f;
      }
      // [d_in ; dh_prev] = (pseudo-rows)ᵀ δ, dh_prev += dh′·z
      const bool wt = SP || rd.wt;
      if (REGW) {
#pragma unroll
        for (int q = 0; q < ((REGW && BP) ? NKI : 0); q++) {
          const int k = u + q * 64;
          if (k < K) {
            f32x2 c01 = {0.f, 0.f}, c23 = {0.f, 0.f};
#pragma unroll
            for (int r4 = 0; r4 < RB4; r4++) {
              const f32x4 dq = *reinterpret_cast<const f32x4*>(dbuf + 4 * r4);
              c01 += wcol[(REGW && BP) ? l : 0][q][r4].lo * dq.lo;
              c23 += wcol[(REGW && BP) ? l : 0][q][r4].hi * dq.hi;
            }
            const float acc = (c01.x + c01.y) + (c23.x + c23.y);
            if (k < in) {
              if (l > 0) dhs[(l - 1) * hmaxv + k] += acc;
              else if (a.dx && valid) a.dx[(size_t)in0 * ((size_t)b + (size_t)B * t) + k] = acc;
            } else
              dhs[l * hmaxv + (k - in)] = acc + dzs[l * hmaxv + (k - in)];
          }
        }
      } else
      for (int k = u; k < K; k += Hp) {
        f32x4 acc4 = {0.f, 0.f, 0.f, 0.f};
        const int R4 = R >> 2;   // (4h: whole float4 groups)
        if (wt) {
          const float* wk = lw + rd.wt_off[l] + k * (SP ? rnn_ldk(R) : rd.ldr[l]);
#pragma unroll UK
          for (int r4 = 0; r4 < R4; r4++)
            acc4 += *reinterpret_cast<const f32x4*>(wk + 4 * r4) * *reinterpret_cast<const f32x4*>(dbuf + 4 * r4);
        } else {
          const float* wc = lw + rd.w_off[l] + k;
#pragma unroll 4
          for (int r4 = 0; r4 < R4; r4++) {
            const f32x4 dq = *reinterpret_cast<const f32x4*>(dbuf + 4 * r4);
            const float* w = wc + (4 * r4) * ldk;
            acc4[0] += w[0] * dq[0];
            acc4[1] += w[ldk] * dq[1];
            acc4[2] += w[2 * ldk] * dq[2];
            acc4[3] += w[3 * ldk] * dq[3];
          }
        }
        const float acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
        if (k < in) {
          if (l > 0) dhs[(l - 1) * hmaxv + k] += acc;
          else if (a.dx && valid) a.dx[(size_t)in0 * ((size_t)b + (size_t)B * t) + k] = acc;
        } else
          dhs[l * hmaxv + (k - in)] = acc + dzs[l * hmaxv + (k - in)];
      }
    }
  }
  // what is left flows into the trainable initial states
  if (valid) {
    int off = 0;
#pragma unroll UL
    for (int l = 0; l < L; l++) {
      const int h = size_of(l + 1);
      if (u < h) a.g0[(size_t)b * a.g0w + off + u] = dhs[l * hmaxv + u];
      off += h;
    }
  }
}

template <bool SP, int MODE_, bool REGW = false>
__global__ void __launch_bounds__(REGW ? 64 : 1024) k_gru(RnnDims rd, RnnArgs a) {
  gru_body<SP, MODE_, REGW>(rd, a, blockIdx.x);
}

// dW[cell, flat order] (+)= the staged product's [4h × K] + [4h] result (k_mlp_dw + k_reduce_tiles wrote it, assigned, into `staged`)
__global__ void __launch_bounds__(256) k_gru_gather(const float* __restrict__ staged, float* __restrict__ dW, int in, int h, int assign) {
  const long long n = lde_host::gru_staged_count(in, h);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const float v = staged[lde_host::gru_staged_index(in, h, e)];
    dW[e] = assign ? v : dW[e] + v;
  }
}

}  // namespace lde
