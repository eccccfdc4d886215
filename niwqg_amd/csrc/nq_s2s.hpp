// Shell-to-shell (giver-receiver) transfers of enstrophy and wave kinetic energy (include/niwqg_amd.h:
// nq_shell_transfer; niwqg_amd/shelltoshell.py: reference restates the definitions in numpy).
//
// T(b | Q): the transfer into receiver shell b with the ADVECTED field restricted to a donor band Q.  g_Q is a real table per
// shell, G_Q(l, k) = g_Q[shell of (l, k)], zero on the shells >= N/2 (the Nyquist rule of nq_coarse.hpp).  With the state of
// nq_transfer_binned -- P = psi-hat, Q-hat the q-hat the tick bins, W the current phi-hat, u, v and q_psi those of the tick's
// products pass --
//   q^Q = Re F^-1[G_Q Q-hat],  phi^Q = F^-1[G_Q W],  phi^Q_x, phi^Q_y = F^-1[ik G_Q W], F^-1[il G_Q W]
//   Jq^Q = ik F[u q^Q] + il F[v q^Q]        J^Q = F[u phi^Q_x + v phi^Q_y]        R^Q = i F[phi^Q q_psi]
// and the rows of a band are the raw shell sums nq_transfer_binned forms of the unfiltered planes:
//   [0] Re(conj P Jq^Q)   [1] Re(conj Q-hat Jq^Q)   [2] Re(conj W J^Q)   [3] Re(conj W R^Q)
//
// Per band: k_s_band, the inverse column sub-passes (k_y_B, k_y_A) on its planes, k_x_band once for (Jq^Q, J^Q) and once for
// R^Q (J^Q and R^Q leave through the one full mixed plane of the pipeline, Mw, as the tick's two products passes do), then the
// forward column sub-passes and the bins of the transfer (BinTrQ, BinTrW) into the band's rows.
//   k_s_band      one thread per (l, k): each selected source is read once, multiplied by g[shell] and written: G Q-hat (half
//                 spectrum), G W and il G W (full planes; il is not available in mixed space).
//   k_x_band<N>   k_x_coarse's sibling with the forward transforms of k_x_products: u, v from the last inversion's rows of
//                 -il psi-hat and psi-hat (the pair the products pass reads: nothing of psi is filtered, so nothing of it is
//                 transformed again), q^Q alone, phi^Q_x = ik . and phi^Q_y one after the other, phi^Q, q_psi from the rows of q
//                 (and q_w); the products in registers; forward row transforms into Muq, Mvq and Mw, which are free between
//                 steps.  No physical plane is stored.
// Two-for-one packing: (u, v) as everywhere; q^Q travels alone (its partner would be its own derivative or
// a field of another magnitude); (q, q_w) only for their difference q_psi, whose rounding is that of the larger either way.
// Live values of a thread at the widest point (J^Q): u, v, the accumulator and the transform's own P complex values, 6 P
// doubles; R^Q: 5 P.  Registers of every instantiation: DESIGN.md section 5p.
#pragma once
#include "nq_coarse.hpp"

namespace nq {

enum { S2S_Q = 1, S2S_ADV = 2, S2S_REF = 4 };

struct BandSpec {
  const cd* Q;                        // half spectrum, pitch ph
  const cd* W;                        // full plane, pitch N (waves)
  cd *gq, *gw, *wy;                   // G Q, G W, il G W
  const double* g;                    // the table of this band, nb entries
  const double* ll;
  int N, ph, what;
};

// grid (ceil(columns / 256), N): thread (l, k); columns = N with a wave row selected, else N/2 + 1
__global__ void __launch_bounds__(256) k_s_band(BandSpec s) {
  const int N = s.N, l = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  const int i = k <= N / 2 ? k : N - k, j = l <= N / 2 ? l : N - l;
  const double g = s.g[nq_shell_of(i, j)];
  if ((s.what & S2S_Q) && k <= N / 2) {
    const size_t idx = (size_t)l * s.ph + k;
    s.gq[idx] = cscale(s.Q[idx], g);
  }
  if (s.what & (S2S_ADV | S2S_REF)) {
    const size_t idx = (size_t)l * N + k;
    const cd w = cscale(s.W[idx], g);
    s.gw[idx] = w;
    if (s.what & S2S_ADV) {
      const double ly = s.ll[l];
      s.wy[idx] = cmake(-(ly * w.y), ly * w.x);               // il G W
    }
  }
}

struct BandRows {
  MArr mU, mP;                        // the last inversion's rows of -il psi-hat and psi-hat (u, v)
  MArr mQ, mQw;                       // and of q-hat, q_w-hat (q_psi)
  MArr gq;                            // mixed-space half plane of G Q-hat
  const cd *gw, *wy;                  // mixed-space full planes of G W, il G W, pitch N
  MArr oUq, oVq, oW;                  // the forward row transforms: F_x[u q^Q], F_x[v q^Q]; F_x[J^Q] or F_x[R^Q]
  int what;                           // the rows of THIS launch: S2S_Q and / or S2S_ADV, or S2S_REF alone
  int v_zero_nyq;                     // k_x_products' rule for v: 1 in the Kernel family
};

template <int N>
__device__ __forceinline__ void band_store_full(const cd (&w)[XPlan<N>::P], const MArr& M, size_t row, int j) {
  constexpr int P = XPlan<N>::P, T = XPlan<N>::T;
  const XRowT<false> rp = xrow<false>(M, row);
#pragma unroll
  for (int t = 0; t < P; ++t) *rp.at(j + t * T) = w[t];
}

template <int N, int MODE>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_band(BandRows a, const cd* __restrict__ tw, const double* __restrict__ kk) {
#pragma clang fp contract(off)
  typedef XPlan<N> X;
  typedef typename X::F F;
  constexpr int P = X::P, T = X::T;
  constexpr bool WAVES = (MODE == MODE_COUPLED || MODE == MODE_UNCOUPLED);
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t row = (size_t)blockIdx.x * X::C + c;
  cd* lds = reinterpret_cast<cd*>(nq_smem);
  cd* twl = lds + F::LDS_ELEMS;
  for (int i = threadIdx.x; i < F::TW_LDS_ELEMS; i += X::THREADS) twl[i] = tw[i];
  typename F::TwLds twr;
  twr.base = twl;
  cd w[P];
#pragma unroll
  for (int t = 0; t < P; ++t) w[t] = cmake(0, 0);
  wg_barrier_all();
  if (a.what & (S2S_Q | S2S_ADV)) {
    double u[P], v[P];
    {                                                                         // u, v: k_x_products' pair
      HsRegs<P> h;
      hs_load<N, P, T, true>(h, xrow<false>(a.mU, row), xrow<false>(a.mP, row), j);
      NQ_PHASE_FENCE();
      hs_pack<N, P, T, F, true>(w, h, j, c, lds, kk, true, a.v_zero_nyq != 0);
    }
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
#pragma unroll
    for (int t = 0; t < P; ++t) {
      u[t] = w[t].x;
      v[t] = w[t].y;
    }
    NQ_PHASE_FENCE();
    if (a.what & S2S_Q) {
      flow_pair<N, 0, false, 0>(w, a.gq, a.gq, row, j, c, lds, kk);            // q^Q, alone
      NQ_PHASE_FENCE();
      F::template run<true>(w, j, c, lds, twr);
#pragma unroll
      for (int t = 0; t < P; ++t) {
        const double q = w[t].x;
        w[t] = cmake(u[t] * q, v[t] * q);                                       // u q^Q + i v q^Q
      }
      NQ_PHASE_FENCE();
      F::template run<false>(w, j, c, lds, twr);
      NQ_PHASE_FENCE();
      unpack_pair_store<N, P, T, F>(w, j, c, lds, xrow<false>(a.oUq, row), xrow<false>(a.oVq, row));
      NQ_PHASE_FENCE();
    }
    if (WAVES && (a.what & S2S_ADV)) {
      cd acc[P];
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {                                    // phi^Q_x, phi^Q_y
        const cd* __restrict__ rp = (pass == 0 ? a.gw : a.wy) + row * N;
#pragma unroll
        for (int t = 0; t < P; ++t) {
          const cd z = rp[j + t * T];
          w[t] = pass == 0 ? cscale(cmul_i(z), kk[j + t * T]) : z;
        }
        NQ_PHASE_FENCE();
        F::template run<true>(w, j, c, lds, twr);
#pragma unroll
        for (int t = 0; t < P; ++t) {
          if (pass == 0) acc[t] = cmake(u[t] * w[t].x, u[t] * w[t].y);
          else acc[t] = cmake(acc[t].x + v[t] * w[t].x, acc[t].y + v[t] * w[t].y);
        }
        NQ_PHASE_FENCE();
      }
      F::template run<false>(acc, j, c, lds, twr);
      NQ_PHASE_FENCE();
      band_store_full<N>(acc, a.oW, row, j);
      NQ_PHASE_FENCE();
    }
  }
  if (WAVES && (a.what & S2S_REF)) {
    double qp[P];
    flow_pair<N, MODE == MODE_COUPLED, false, 0>(w, a.mQ, MODE == MODE_COUPLED ? a.mQw : a.mQ, row, j, c, lds, kk);
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
#pragma unroll
    for (int t = 0; t < P; ++t) qp[t] = (MODE == MODE_COUPLED) ? w[t].x - w[t].y : w[t].x;
    NQ_PHASE_FENCE();
    {
      const cd* __restrict__ rp = a.gw + row * N;
#pragma unroll
      for (int t = 0; t < P; ++t) w[t] = rp[j + t * T];
    }
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
#pragma unroll
    for (int t = 0; t < P; ++t) w[t] = cmake(-(qp[t] * w[t].y), qp[t] * w[t].x);     // i phi^Q q_psi
    NQ_PHASE_FENCE();
    F::template run<false>(w, j, c, lds, twr);
    NQ_PHASE_FENCE();
    band_store_full<N>(w, a.oW, row, j);
  }
}

}  // namespace nq
