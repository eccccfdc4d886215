// Time-mean and covariance maps of the physical fields, accumulated inside the step (include/niwqg_amd.h:
// nq_avg_attach, nq_any_moments).
//
// Running sums only: one fp64 plane per kept field (phi: one complex plane) and per kept product, row-major in physical order
// (the layout nq_get_field returns).  THE accumulation rule (niwqg_amd/averages.py: accumulate restates it): every sample does
// S <- S + x, products S <- S + x y, in fp64 and in sample order.  One thread owns a point: no atomics, no reduction, so two runs
// are bit-identical and a first-moment plane is the sequential fp64 sum exactly.  S + x y may contract into one fma: one
// rounding less per sample than numpy's, never more.  Non-finite values propagate as IEEE addition does.
#pragma once
#include "nq_hist.hpp"

namespace nq {

constexpr int AVG_SLOTS = HIST_SLOTS;          // real values of a point, hist_slot's: Kernel family q, q_psi, |phi|^2; QGModel q, c
constexpr int AVG_PHI = AVG_SLOTS;             // the mask bit of the complex phi plane
constexpr int AVG_MAX_PRODUCTS = AVG_SLOTS * (AVG_SLOTS + 1) / 2;      // unordered pairs of the real slots

struct AvgArgs {
  double* sum[AVG_SLOTS];                      // first-moment planes of the real slots
  cd* sum_phi;                                 // and of phi
  double* prod[AVG_MAX_PRODUCTS];              // product planes
  int mask;                                    // bit s: sum[s] is kept; bit AVG_PHI: sum_phi
  int np;                                      // products kept
  int pa[AVG_MAX_PRODUCTS], pb[AVG_MAX_PRODUCTS];      // their slots
};

// THE add of both kernels
__device__ __forceinline__ double avg_add(double s, double x) { return s + x; }
__device__ __forceinline__ double avg_add(double s, double x, double y) { return s + x * y; }
__device__ __forceinline__ double avg_pick(int slot, double v0, double v1, double v2) { return slot == 0 ? v0 : (slot == 1 ? v1 : v2); }

// ---- fused grids, Kernel family: k_x_hist's values (x_row_values), then a read-add-write of the thread's points per kept plane -----
// One plane at a time, its P loads in flight together and its P stores after them: the planes may alias as far as the compiler
// knows, so a point-by-point loop over the planes would wait for every load on its own.  A wave's accesses to one plane are 64
// consecutive doubles (phi: complex) of one row, or eight rows of eight at N = 64.
template <int P, int T>
__device__ __forceinline__ void avg_row_add(double* __restrict__ pl, const double (&v)[P]) {
  double s[P];
#pragma unroll
  for (int t = 0; t < P; ++t) s[t] = pl[t * T];
#pragma unroll
  for (int t = 0; t < P; ++t) pl[t * T] = avg_add(s[t], v[t]);
}
template <int N, int MODE, bool SLAB>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_moments(MArr Mq, MArr Mqw, MArr Mphi, const cd* __restrict__ tw, const double* __restrict__ kk, AvgArgs a) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T;
  double q[P], qpsi[P];
  cd w[P];
  x_row_values<N, MODE, SLAB>(Mq, Mqw, Mphi, tw, kk, q, qpsi, w);
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
  double a2[P];
#pragma unroll
  for (int t = 0; t < P; ++t) a2[t] = w[t].x * w[t].x + w[t].y * w[t].y;
  if (a.mask & 1) avg_row_add<P, T>(a.sum[0] + at, q);
  if (a.mask & 2) avg_row_add<P, T>(a.sum[1] + at, qpsi);
  if (a.mask & 4) avg_row_add<P, T>(a.sum[2] + at, a2);
#pragma unroll
  for (int p = 0; p < AVG_MAX_PRODUCTS; ++p) {
    if (p < a.np) {
      double* __restrict__ pl = a.prod[p] + at;
      const int sa = a.pa[p], sb = a.pb[p];
      double s[P];
#pragma unroll
      for (int t = 0; t < P; ++t) s[t] = pl[t * T];
#pragma unroll
      for (int t = 0; t < P; ++t) pl[t * T] = avg_add(s[t], avg_pick(sa, q[t], qpsi[t], a2[t]), avg_pick(sb, q[t], qpsi[t], a2[t]));
    }
  }
}

// ---- element-wise: the any-size path and QGModel on the fused grids ----------------------------------------------------
// Values of slot s from plane p[s] as hist_val reads them (stride 1: a real plane, 2: a complex one; what 0: Re, 1: |a|^2),
// phi from a complex plane; null: the slot is not kept.  Every kept sum of a point is loaded before the first is stored.
struct AvgSrc {
  const double* p[AVG_SLOTS];
  int stride[AVG_SLOTS], what[AVG_SLOTS];
  const cd* phi;
};
__global__ void __launch_bounds__(256) k_moments_plane(AvgSrc src, size_t n, AvgArgs a) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    double v[AVG_SLOTS], s[AVG_SLOTS], sp[AVG_MAX_PRODUCTS];
    cd ph = cmake(0, 0), sph = cmake(0, 0);
#pragma unroll
    for (int k = 0; k < AVG_SLOTS; ++k) {
      const bool on = (a.mask >> k) & 1;
      v[k] = on ? hist_val(src.p[k], i, src.stride[k], src.what[k]) : 0.0;
      s[k] = on ? a.sum[k][i] : 0.0;
    }
    if (a.mask & (1 << AVG_PHI)) {
      ph = src.phi[i];
      sph = a.sum_phi[i];
    }
#pragma unroll
    for (int p = 0; p < AVG_MAX_PRODUCTS; ++p) sp[p] = p < a.np ? a.prod[p][i] : 0.0;
#pragma unroll
    for (int k = 0; k < AVG_SLOTS; ++k)
      if ((a.mask >> k) & 1) a.sum[k][i] = avg_add(s[k], v[k]);
    if (a.mask & (1 << AVG_PHI)) a.sum_phi[i] = cmake(avg_add(sph.x, ph.x), avg_add(sph.y, ph.y));
#pragma unroll
    for (int p = 0; p < AVG_MAX_PRODUCTS; ++p)
      if (p < a.np) a.prod[p][i] = avg_add(sp[p], avg_pick(a.pa[p], v[0], v[1], v[2]), avg_pick(a.pb[p], v[0], v[1], v[2]));
  }
}

}  // namespace nq
