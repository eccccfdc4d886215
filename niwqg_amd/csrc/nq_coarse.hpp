// Coarse-grained (sub-filter) energy and enstrophy flux maps (include/niwqg_amd.h: nq_coarse_flux;
// niwqg_amd/coarse.py: reference restates the definitions in numpy).
//
// G is a real isotropic filter given per shell, G(l, k) = g[shell of (l, k)], an overbar is F^-1[G .].  From the planes the
// spectral transfer bins -- P = psi-hat, Q = the q-hat the tick bins, Fu = F[u q], Fv = F[v q], W = phi-hat and J, the J plane
// of the tick's first products pass --
//   ke_qg       v-bar F^-1[G Fu] - u-bar F^-1[G Fv]                                      (= tau . grad psi-bar)
//   ens         -(F^-1[G Fu] q-bar_x + F^-1[G Fv] q-bar_y) + q-bar (u-bar q-bar_x + v-bar q-bar_y)   (= -tau . grad q-bar)
//   ke_niw_adv  Re(conj(phi-bar) (F^-1[G J] - u-bar phi-bar_x - v-bar phi-bar_y))
// with tau = (F^-1[G Fu] - u-bar q-bar, F^-1[G Fv] - v-bar q-bar).  Positive: transfer towards scales below the cut.
//
// NYQUIST RULE: every filter table is zero on the shells b >= N/2 (the call refuses any other).  Row N/2, column N/2, the
// passenger row of q-hat and the corner mode then have nothing in any filtered plane, and the only rule of the self-mirrored
// columns left is hs_pack's for column 0: its imaginary part is dropped after the multiplication, i.e. the real fields are the
// real parts of the full-plane transforms.
//
// Two kernels per filter scale, the inverse column sub-passes (k_y_B, k_y_A) between them:
//   k_s_coarse     one pass over the spectral planes: each source value is read once, multiplied by g[shell] and written to
//                  the filtered planes the row pass needs.  The y-derivatives are taken here (il is not available in mixed
//                  space): G P and -il G P; G Q and il G Q; G Fu, G Fv; with waves G W, il G W and G J (full planes).
//   k_x_coarse<N>  x_flow_values' sibling: one row block, up to four inverse row transforms of real fields, two-for-one packed
//                  where two of one magnitude go together: (u-bar, v-bar = ik .), q-bar alone, (q-bar_x = ik ., q-bar_y),
//                  (F^-1[G Fu], F^-1[G Fv]), and four complex ones, phi-bar_x = ik ., phi-bar_y, F^-1[G J], phi-bar, each
//                  skipped by a workgroup-uniform branch when no selected map needs it.  The maps are formed in registers, no intermediate physical plane is written; a map
//                  plane is stored only when the caller asked for maps, the sum and the sum of squares of every selected map
//                  always go to one slot per workgroup (added up in a fixed order by k_reduce_partials: no atomics).
// Live values of a thread at the widest point (ens with ke_qg selected): u-bar, v-bar, q-bar (u-bar q-bar_x + v-bar q-bar_y),
// q-bar_x, q-bar_y and the transform's own P complex values: 7 P doubles.  The 8192-point row plan gives a thread 128 registers
// for P = 8, which that does not fit: nq_coarse_flux refuses that size.
#pragma once
#include "nq_flow.hpp"

namespace nq {

enum { CG_KE = 1, CG_ENS = 2, CG_NIW = 4 };

struct CoarseSpec {
  const cd *P, *Q, *Fu, *Fv;          // half spectra, pitch ph
  const cd *W, *J;                    // full planes, pitch N (waves)
  cd *gp, *up, *gq, *qy, *fu, *fv;    // G P, -il G P, G Q, il G Q, G Fu, G Fv
  cd *gw, *wy, *gj;                   // G W, il G W, G J
  const double* g;                    // the table of this scale, nb entries
  const double* ll;
  int N, ph, what;
};

// grid (ceil(columns / 256), N): thread (l, k); columns = N with the wave maps selected, else N/2 + 1
__global__ void __launch_bounds__(256) k_s_coarse(CoarseSpec s) {
  const int N = s.N, l = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  const int i = k <= N / 2 ? k : N - k, j = l <= N / 2 ? l : N - l;
  const double g = s.g[nq_shell_of(i, j)], ly = s.ll[l];
  if (k <= N / 2) {
    const size_t idx = (size_t)l * s.ph + k;
    const cd p = cscale(s.P[idx], g);
    s.gp[idx] = p;
    s.up[idx] = cmake(ly * p.y, -(ly * p.x));                 // -il G P
    if (s.what & CG_ENS) {
      const cd q = cscale(s.Q[idx], g);
      s.gq[idx] = q;
      s.qy[idx] = cmake(-(ly * q.y), ly * q.x);               // il G Q
    }
    if (s.what & (CG_KE | CG_ENS)) {
      s.fu[idx] = cscale(s.Fu[idx], g);
      s.fv[idx] = cscale(s.Fv[idx], g);
    }
  }
  if (s.what & CG_NIW) {
    const size_t idx = (size_t)l * N + k;
    const cd w = cscale(s.W[idx], g);
    s.gw[idx] = w;
    s.wy[idx] = cmake(-(ly * w.y), ly * w.x);                 // il G W
    s.gj[idx] = cscale(s.J[idx], g);
  }
}

struct CoarseRows {
  MArr gp, up, gq, qy, fu, fv;        // mixed-space half planes, as the inverse column passes leave them
  const cd *gw, *wy, *gj;             // mixed-space full planes, pitch N
  int what;
  double* map[3];                     // physical (N, N) planes of ke_qg, ens, ke_niw_adv, or null
  double* part;                       // [workgroup][6]: sum, sum of squares of the three maps
};

// one finished map: its moments into the thread's sums, its plane when asked for
template <int P, int T>
__device__ __forceinline__ void coarse_emit(const double (&val)[P], double* __restrict__ plane, size_t at, double& s1, double& s2) {
#pragma unroll
  for (int t = 0; t < P; ++t) {
    s1 += val[t];
    s2 += val[t] * val[t];
  }
  if (plane) {
#pragma unroll
    for (int t = 0; t < P; ++t) plane[at + t * T] = val[t];
  }
}

// the packed pair (ik A, B) into w: the x- and the y-derivative of one real field from its rows G X and il G X.  An odd
// x-derivative has nothing from column N/2 (hs_pack's rule for v).  The two are of one magnitude; a field packed with its own
// derivative is not (|il| is 1e-5 on the reference's domains), and the smaller value of a packed pair carries the rounding of
// the larger ("Two-for-one packing and magnitudes").
template <int N>
__device__ __forceinline__ void coarse_grad_pair(cd (&w)[XPlan<N>::P], const MArr& A, const MArr& B, size_t row, int j, int c, cd* lds,
                                                 const double* __restrict__ kk) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T;
  HsRegs<P> h;
  hs_load<N, P, T, true>(h, xrow<false>(A, row), xrow<false>(B, row), j);
  NQ_PHASE_FENCE();
#pragma unroll
  for (int t = 0; t < P / 2; ++t) h.a[t] = cscale(cmul_i(h.a[t]), kk[j + t * T]);
  h.an = cmake(0, 0);
  hs_pack<N, P, T, typename X::F, true>(w, h, j, c, lds, kk, false, false);
}

template <int N, bool WAVES>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_coarse(CoarseRows a, const cd* __restrict__ tw, const double* __restrict__ kk) {
#pragma clang fp contract(off)
  typedef XPlan<N> X;
  typedef typename X::F F;
  constexpr int P = X::P, T = X::T;
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t row = (size_t)blockIdx.x * X::C + c;
  const size_t at = row * N + j;                                   // point t of the thread: at + t * T
  cd* lds = reinterpret_cast<cd*>(nq_smem);
  cd* twl = lds + F::LDS_ELEMS;
  for (int i = threadIdx.x; i < F::TW_LDS_ELEMS; i += X::THREADS) twl[i] = tw[i];
  typename F::TwLds twr;
  twr.base = twl;
  double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};         // sums, sums of squares
  double u[P], v[P], val[P];
  cd w[P];
#pragma unroll
  for (int t = 0; t < P; ++t) w[t] = cmake(0, 0);
  wg_barrier_all();
  // u-bar, v-bar: k_x_products' pair (v has nothing from column N/2)
  flow_pair<N, 1, false, 1>(w, a.up, a.gp, row, j, c, lds, kk);
  NQ_PHASE_FENCE();
  F::template run<true>(w, j, c, lds, twr);
#pragma unroll
  for (int t = 0; t < P; ++t) {
    u[t] = w[t].x;
    v[t] = w[t].y;
  }
  NQ_PHASE_FENCE();
  if (a.what & (CG_KE | CG_ENS)) {
    double r[P], qx[P], qy[P];
    if (a.what & CG_ENS) {
      flow_pair<N, 0, false, 0>(w, a.gq, a.gq, row, j, c, lds, kk);            // q-bar, alone
      NQ_PHASE_FENCE();
      F::template run<true>(w, j, c, lds, twr);
#pragma unroll
      for (int t = 0; t < P; ++t) r[t] = w[t].x;
      NQ_PHASE_FENCE();
      coarse_grad_pair<N>(w, a.gq, a.qy, row, j, c, lds, kk);                  // q-bar_x, q-bar_y
      NQ_PHASE_FENCE();
      F::template run<true>(w, j, c, lds, twr);
#pragma unroll
      for (int t = 0; t < P; ++t) {
        qx[t] = w[t].x;
        qy[t] = w[t].y;
        r[t] = r[t] * (u[t] * qx[t] + v[t] * qy[t]);                            // the resolved term q-bar u-bar . grad q-bar
      }
      NQ_PHASE_FENCE();
    }
    flow_pair<N, 1, false, 0>(w, a.fu, a.fv, row, j, c, lds, kk);              // F^-1[G Fu], F^-1[G Fv]
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
    if (a.what & CG_KE) {
#pragma unroll
      for (int t = 0; t < P; ++t) val[t] = v[t] * w[t].x - u[t] * w[t].y;
      coarse_emit<P, T>(val, a.map[0], at, sa[0], sb[0]);
    }
    if (a.what & CG_ENS) {
#pragma unroll
      for (int t = 0; t < P; ++t) val[t] = r[t] - (w[t].x * qx[t] + w[t].y * qy[t]);
      coarse_emit<P, T>(val, a.map[1], at, sa[1], sb[1]);
    }
    NQ_PHASE_FENCE();
  }
  if (WAVES && (a.what & CG_NIW)) {
    cd acc[P];
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {                          // phi-bar_x, phi-bar_y, F^-1[G J], phi-bar
      const cd* __restrict__ rp = (pass == 1 ? a.wy : pass == 2 ? a.gj : a.gw) + row * N;
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
        else if (pass == 1) acc[t] = cmake(acc[t].x + v[t] * w[t].x, acc[t].y + v[t] * w[t].y);
        else if (pass == 2) acc[t] = cmake(w[t].x - acc[t].x, w[t].y - acc[t].y);
        else val[t] = w[t].x * acc[t].x + w[t].y * acc[t].y;
      }
      NQ_PHASE_FENCE();
    }
    coarse_emit<P, T>(val, a.map[2], at, sa[2], sb[2]);
  }
  wg_barrier_all();                                  // every wave is through its last exchange: the LDS is free
  double* red = reinterpret_cast<double*>(nq_smem + X::LDS_BYTES - 512);
  block_sum_thread0<3>(sa, red);
  block_sum_thread0<3>(sb, red);
  if (threadIdx.x == 0) {
    double* __restrict__ o = a.part + 6 * (size_t)blockIdx.x;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      o[2 * m] = sa[m];
      o[2 * m + 1] = sb[m];
    }
  }
}

}  // namespace nq
