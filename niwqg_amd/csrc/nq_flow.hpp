// Velocity, strain, Okubo-Weiss and wave-gradient values for the PDFs and the averages (include/niwqg_amd.h:
// NQ_FLOW_*; niwqg_amd/flow.py: reference restates the definitions in numpy).
//
// x_flow_values is x_row_values' sibling: one row block, every value of the last inversion's mixed-space rows, up to three
// SELECTED values per point kept in registers, no physical plane written.  Up to six inverse row transforms, each skipped by a
// workgroup-uniform branch (the selection is a kernel argument) when none of the selected values needs it:
//   1. (q, q_w) two-for-one                       -> q, q_psi                 [q, q_psi, ss, strain2, ow]
//   2. (mU, ik mP) two-for-one                    -> u, v                     [u, v]
//   3. (ik mU, -k^2 mP) two-for-one               -> u_x, v_x                 [sn, ss, strain2, ow]
//   4. ik mPhi                                    -> phi_x                    [gradphi2]
//   5. mPhiy                                      -> phi_y                    [gradphi2]
//   6. mPhi                                       -> phi (left in w)          [phi2, the averages' complex phi plane]
// with sn = 2 u_x, ss = 2 v_x - q_psi, strain2 = sn^2 + ss^2, ow = strain2 - q_psi^2, gradphi2 = |phi_x|^2 + |phi_y|^2.
// Self-mirrored columns (hs_pack's rules, what k_x_get_uv and k_x_products apply): the imaginary part of columns 0 and N/2 is
// dropped after the multiplication; a real field's odd x-derivative has nothing from column N/2 (v: zero_nyq; u_x: the same
// rule), its even one (v_x) keeps the real part.  The rows a transform multiplies are fetched again for it instead of being held
// across the transform before (HsRegs: 5 P registers); the second read should be served by the L2 (not measured).
// One term no mixed-space row holds: the corner mode (l, k) = (N/2, N/2) of ik (-il psi-hat) is REAL (k l Re psi-hat there:
// neither wavenumber changes sign under the mirror), so it survives the real part, while mU has its row N/2 dropped for u.  It
// is added to u_x from the spectral psi-hat plane: k l Re psi-hat(N/2, N/2) (-1)^(x + y) / N^2.
// 8192-point rows run 1024 threads of 128 registers: a thread holds ONE value there (flow_nv) and the host issues one launch per
// selected value, each counting into (adding to) its own slot.  A joint table or a product of two different values needs both
// in one thread and is refused at that size.
#pragma once
#include "nq_avg.hpp"

namespace nq {

// value codes of a slot: the three old fields (NQ_PDF_Q, NQ_PDF_QPSI, NQ_PDF_PHI2) and the flow fields (NQ_FLOW_*)
enum { FLOW_Q = 0, FLOW_QPSI = 1, FLOW_PHI2 = 2, FLOW_U = 16, FLOW_V = 17, FLOW_SN = 18, FLOW_SS = 19, FLOW_STRAIN2 = 20,
       FLOW_OW = 21, FLOW_GRADPHI2 = 22, FLOW_NONE = -1 };
constexpr int FLOW_FIRST = FLOW_U, FLOW_LAST = FLOW_GRADPHI2;

struct FlowSel {
  int code[HIST_SLOTS];       // what slot s holds (FLOW_NONE: nothing, the slot's registers stay zero)
  int phi;                    // 1: transform phi into w although no slot holds phi2 (the averages' complex plane)
  const cd* ph_corner;        // psi-hat(N/2, N/2) in the spectral plane
  const double* ll;           // the l wavenumbers
};
template <int N> constexpr int flow_nv() { return N >= 8192 ? 1 : HIST_SLOTS; }      // values a thread holds
__host__ __device__ inline bool flow_any(const FlowSel& s, int a, int b = FLOW_NONE - 1, int c = FLOW_NONE - 1, int d = FLOW_NONE - 1,
                                         int e = FLOW_NONE - 1) {
  for (int i = 0; i < HIST_SLOTS; ++i)
    if (s.code[i] == a || s.code[i] == b || s.code[i] == c || s.code[i] == d || s.code[i] == e) return true;
  return false;
}

// the (ik A, -k^2 B) pair of transform 3 from the (A, B) = (mU, mP) rows as loaded; column N/2 of ik A is dropped whole
template <int N, int P, int T>
__device__ __forceinline__ void flow_grad_rows(HsRegs<P>& r, int j, const double* __restrict__ kk) {
#pragma unroll
  for (int t = 0; t < P / 2; ++t) {
    const double k = kk[j + t * T];
    r.a[t] = cscale(cmul_i(r.a[t]), k);
    r.b[t] = cscale(r.b[t], -(k * k));
  }
  const double kn = kk[N / 2];
  r.an = cmake(0, 0);
  r.bn = cscale(r.bn, -(kn * kn));
}

// the packed pair of one transform into w: hs_load, the multiplication MUL (0: none; 1: B' = ik B, column N/2 of B' dropped, as
// k_x_products packs (u, v); 2: A' = ik A, column N/2 dropped, B' = -k^2 B), hs_pack
template <int N, int MODE_PAIR, bool SLAB, int MUL>
__device__ __forceinline__ void flow_pair(cd (&w)[XPlan<N>::P], const MArr& A, const MArr& B, size_t row, int j, int c, cd* lds,
                                          const double* __restrict__ kk) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T;
  constexpr bool PAIR = MODE_PAIR != 0;
  HsRegs<P> h;
  hs_load<N, P, T, PAIR>(h, xrow<SLAB>(A, row), xrow<SLAB>(B, row), j);
  NQ_PHASE_FENCE();
  if (MUL == 2) flow_grad_rows<N, P, T>(h, j, kk);
  hs_pack<N, P, T, typename X::F, PAIR>(w, h, j, c, lds, kk, MUL == 1, MUL == 1);
}

template <int N, int MODE, bool SLAB>
__device__ __forceinline__ void x_flow_values(const MArr& Mq, const MArr& Mqw, const MArr& Mu, const MArr& Mp, const MArr& Mphi,
                                              const MArr& Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
                                              const FlowSel& sel, double (&val)[flow_nv<N>()][XPlan<N>::P], cd (&w)[XPlan<N>::P]) {
  // the formulas on the transforms' outputs are not contracted into fused multiply-adds, so they round the same way in the range
  // pass, the counting pass and the averages' pass (three instantiations).  The transforms themselves are the one inlined WgFft
  // in all three, built under the compiler's default; tests/test_gpu_flow.py asserts that the range pass's extremes are values
  // the counting pass sees.
#pragma clang fp contract(off)
  typedef XPlan<N> X;
  typedef typename X::F F;
  constexpr int P = X::P, T = X::T, NV = flow_nv<N>();
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t row = (size_t)blockIdx.x * X::C + c;
  cd* lds = reinterpret_cast<cd*>(nq_smem);
  cd* twl = lds + F::LDS_ELEMS;
  for (int i = threadIdx.x; i < F::TW_LDS_ELEMS; i += X::THREADS) twl[i] = tw[i];
  typename F::TwLds twr;
  twr.base = twl;
#pragma unroll
  for (int s = 0; s < NV; ++s) {
#pragma unroll
    for (int t = 0; t < P; ++t) val[s][t] = 0.0;
  }
#pragma unroll
  for (int t = 0; t < P; ++t) w[t] = cmake(0, 0);
  wg_barrier_all();
  // 1. q, q_psi.  Slots that hold ss, strain2 or ow keep q_psi until transform 3.
  if (flow_any(sel, FLOW_Q, FLOW_QPSI, FLOW_SS, FLOW_STRAIN2, FLOW_OW)) {
    flow_pair<N, MODE == MODE_COUPLED, SLAB, 0>(w, Mq, MODE == MODE_COUPLED ? Mqw : Mq, row, j, c, lds, kk);
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int code = sel.code[s];
      if (code == FLOW_Q) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = w[t].x;
      } else if (code == FLOW_QPSI || code == FLOW_SS || code == FLOW_STRAIN2 || code == FLOW_OW) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = (MODE == MODE_COUPLED) ? w[t].x - w[t].y : w[t].x;
      }
    }
    NQ_PHASE_FENCE();
  }
  // 2. u, v: k_x_products' pair (Kernel family: v has nothing from column N/2)
  if (flow_any(sel, FLOW_U, FLOW_V)) {
    flow_pair<N, 1, SLAB, 1>(w, Mu, Mp, row, j, c, lds, kk);
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int code = sel.code[s];
      if (code == FLOW_U) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = w[t].x;
      } else if (code == FLOW_V) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = w[t].y;
      }
    }
    NQ_PHASE_FENCE();
  }
  // 3. u_x, v_x
  if (flow_any(sel, FLOW_SN, FLOW_SS, FLOW_STRAIN2, FLOW_OW)) {
    flow_pair<N, 1, SLAB, 2>(w, Mu, Mp, row, j, c, lds, kk);
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
    {
      const double kl = kk[N / 2] * sel.ll[N / 2] * sel.ph_corner->x * (1.0 / ((double)N * N));
      static_assert(T % 2 == 0, "x = j + t T has j's parity");
      const double corner = ((j + (int)row) & 1) ? -kl : kl;
#pragma unroll
      for (int t = 0; t < P; ++t) w[t].x += corner;
    }
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int code = sel.code[s];
      if (code == FLOW_SN) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = 2.0 * w[t].x;
      } else if (code == FLOW_SS) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = 2.0 * w[t].y - val[s][t];
      } else if (code == FLOW_STRAIN2 || code == FLOW_OW) {
#pragma unroll
        for (int t = 0; t < P; ++t) {
          const double qp = val[s][t], sn = 2.0 * w[t].x, ss = 2.0 * w[t].y - qp;
          const double s2 = sn * sn + ss * ss;
          val[s][t] = code == FLOW_OW ? s2 - qp * qp : s2;
        }
      }
    }
    NQ_PHASE_FENCE();
  }
  // 4, 5. phi_x, phi_y of the current phi-hat
  if (flow_any(sel, FLOW_GRADPHI2)) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const XRowT<SLAB> rp = xrow<SLAB>(pass == 0 ? Mphi : Mphiy, row);
#pragma unroll
      for (int t = 0; t < P; ++t) {
        const cd v = *rp.at(j + t * T);
        w[t] = pass == 0 ? cscale(cmul_i(v), kk[j + t * T]) : v;
      }
      NQ_PHASE_FENCE();
      F::template run<true>(w, j, c, lds, twr);
#pragma unroll
      for (int s = 0; s < NV; ++s) {
        if (sel.code[s] == FLOW_GRADPHI2) {
#pragma unroll
          for (int t = 0; t < P; ++t) {
            const double a2 = w[t].x * w[t].x + w[t].y * w[t].y;
            val[s][t] = pass == 0 ? a2 : val[s][t] + a2;
          }
        }
      }
      NQ_PHASE_FENCE();
    }
  }
  // 6. phi, as x_row_values leaves it
  if (sel.phi || flow_any(sel, FLOW_PHI2)) {
    const XRowT<SLAB> rp = xrow<SLAB>(Mphi, row);
#pragma unroll
    for (int t = 0; t < P; ++t) w[t] = *rp.at(j + t * T);
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      if (sel.code[s] == FLOW_PHI2) {
#pragma unroll
        for (int t = 0; t < P; ++t) val[s][t] = w[t].x * w[t].x + w[t].y * w[t].y;
      }
    }
    NQ_PHASE_FENCE();
  }
  wg_barrier_all();                                  // every wave is through its last exchange: the LDS is free
}

// k_x_hist on the selected values: slot s of the tables (and of part[block][6]) is slot s of the selection.  A launch that holds
// fewer values than the call has slots is handed `h.tab` and `part` moved to its first slot, and a mask without the others.
template <int N, int MODE, bool SLAB, bool MINMAX>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_flow_hist(MArr Mq, MArr Mqw, MArr Mu, MArr Mp, MArr Mphi, MArr Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
              FlowSel sel, HistArgs h, double* __restrict__ part) {
  typedef XPlan<N> X;
  static_assert(hist_lds_bytes<N>(HIST_MAX_WORDS) <= 160 * 1024, "row plan or LDS tables exceed the 160 KB of a CU");
  static_assert(X::LDS_BYTES >= 16 * 6 * sizeof(double), "min/max scratch");
  constexpr int P = X::P, NV = flow_nv<N>();
  double val[NV][P];
  cd w[P];
  x_flow_values<N, MODE, SLAB>(Mq, Mqw, Mu, Mp, Mphi, Mphiy, tw, kk, sel, val, w);
  if (MINMAX) {
    double mn[NV], mx[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) mn[s] = mx[s] = val[s][0];
#pragma unroll
    for (int t = 1; t < P; ++t) {
#pragma unroll
      for (int s = 0; s < NV; ++s) {
        mn[s] = nan_min(mn[s], val[s][t]);
        mx[s] = nan_max(mx[s], val[s][t]);
      }
    }
    block_minmax_store<NV>(mn, mx, reinterpret_cast<double*>(nq_smem), part + 6 * (size_t)blockIdx.x);
  } else {
    unsigned* tab = reinterpret_cast<unsigned*>(nq_smem);
    const int words = hist_words(h.bins, h.jbins);
    hist_zero(tab, words);
    wg_barrier_all();
#pragma unroll
    for (int t = 0; t < P; ++t) hist_count(tab, h, val[0][t], val[NV > 1 ? 1 : 0][t], val[NV - 1][t]);
    wg_barrier_all();
    hist_flush(tab, words, h.tab);
  }
}

// k_x_moments on the selected values: AvgArgs' slot s is slot s of the selection, phi is w
template <int N, int MODE, bool SLAB>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_flow_moments(MArr Mq, MArr Mqw, MArr Mu, MArr Mp, MArr Mphi, MArr Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
                 FlowSel sel, AvgArgs a) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T, NV = flow_nv<N>();
  double val[NV][P];
  cd w[P];
  x_flow_values<N, MODE, SLAB>(Mq, Mqw, Mu, Mp, Mphi, Mphiy, tw, kk, sel, val, w);
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t at = ((size_t)blockIdx.x * X::C + c) * N + j;           // point t of the thread: at + t * T
  if (a.mask & (1 << AVG_PHI)) {
    cd* __restrict__ pl = a.sum_phi + at;
    cd s[P];
#pragma unroll
    for (int t = 0; t < P; ++t) s[t] = pl[t * T];
#pragma unroll
    for (int t = 0; t < P; ++t) pl[t * T] = cmake(avg_add(s[t].x, w[t].x), avg_add(s[t].y, w[t].y));
  }
  if (a.mask & 1) avg_row_add<P, T>(a.sum[0] + at, val[0]);
  if (NV > 1 && (a.mask & 2)) avg_row_add<P, T>(a.sum[1] + at, val[NV > 1 ? 1 : 0]);
  if (NV > 2 && (a.mask & 4)) avg_row_add<P, T>(a.sum[2] + at, val[NV - 1]);
#pragma unroll
  for (int p = 0; p < AVG_MAX_PRODUCTS; ++p) {
    if (p < a.np) {
      double* __restrict__ pl = a.prod[p] + at;
      const int sa = a.pa[p], sb = a.pb[p];
      double s[P];
#pragma unroll
      for (int t = 0; t < P; ++t) s[t] = pl[t * T];
#pragma unroll
      for (int t = 0; t < P; ++t)
        pl[t * T] = avg_add(s[t], avg_pick(sa, val[0][t], val[NV > 1 ? 1 : 0][t], val[NV - 1][t]), avg_pick(sb, val[0][t], val[NV > 1 ? 1 : 0][t], val[NV - 1][t]));
    }
  }
}

}  // namespace nq
