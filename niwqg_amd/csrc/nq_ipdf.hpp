// PDFs of the field increments: COUNTS of d_r a(x, y) = a((x + r_x) mod nx, (y + r_y) mod ny) - a(x, y) per separation and field
// (include/niwqg_amd.h: nq_increment_hist, nq_increment_hist2, nq_any_increment_hist;
// niwqg_amd/increments.py: reference restates the definitions in numpy).
//
// A real field is binned signed, the complex phi as |d phi| = sqrt(dr^2 + di^2); the bin rule is hist_bin (csrc/nq_hist.hpp),
// with lo, hi and s = bins / (hi - lo) per (separation, field) read from a small device array.  Field slots of a launch are the
// canonical ones of csrc/nq_sf.hpp (real fields first, then phi); `out[slot]` is the field's position in the CALL's list, and
// the global table and the ranges are laid out in the call's order:
//   tab [separation][field of the call][bins + 3]   64-bit: the bins, below, above, NaN
//   rng [separation][field of the call][3]          lo, hi, s
// Counts only, as in csrc/nq_hist.hpp: 32-bit counters in LDS (atomicAdd on LDS), the non-zero ones added to the global table with
// integer atomics.  No floating-point atomics: the result is bit-reproducible.
//
// MAX_BINS: IPDF_MAX_BINS = HIST_MAX_BINS = 1024.  The largest launch (4096-point rows, two real rows and phi: 128 KB) with its
// TWO alternating tables of 3 x 1027 counters (24 KB) stays inside the 160 KB of a CU: ipdf_lds_bytes is asserted for every N.
#pragma once
#include "nq_sf2.hpp"

namespace nq {

constexpr int IPDF_MAX_BINS = HIST_MAX_BINS, IPDF_PLANE_THREADS = 256;

struct IpdfArgs {
  int nsep;
  const int* seps;                    // nsep separations on the device, 1 <= r <= N - 1 (k_x_flow_ipdf)
  const Sf2Vec* vecs;                 // nsep vectors on the device (k_ipdf_plane): rx in [0, cols), ry in [0, rows), slot = table row
  const double* proj;                 // on the device, [table row][2] = (c_x, c_y), or null: no rotation (k_ipdf_plane)
  int pa, pb;                         // the rotated pair of real slots (-1, -1: none)
  int nreal, phi;                     // real field slots 0..nreal-1, phi (0 / 1) in slot nreal
  int nfields, out[SF_MAX_FIELDS];    // fields of the call; position of slot f in the call's list
  int bins;
  const double* rng;
  unsigned long long* tab;
};

// words of one LDS table of a launch with nf field slots
__host__ __device__ constexpr int ipdf_words(int nf, int bins) { return nf * (bins + 3); }
// LDS of a row launch: the value rows of k_x_flow_sf, then two alternating tables
template <int N> constexpr size_t ipdf_lds_bytes(int nreal, int phi, int bins) {
  const size_t mine = sf_row_doubles<N>(nreal, phi) * sizeof(double) + 2 * (size_t)ipdf_words(nreal + phi, bins) * sizeof(unsigned);
  return XPlan<N>::LDS_BYTES > mine ? XPlan<N>::LDS_BYTES : mine;
}

// the non-zero counters of a launch's LDS table (nf slots of bins + 3) -> row `row` of the global table; the thread that flushes a
// counter zeroes it, so the table is clean again without a pass and a barrier of its own
__device__ __forceinline__ void ipdf_flush(unsigned* t, int nf, const IpdfArgs& a, int row) {
  const int stride = a.bins + 3;
  unsigned long long* __restrict__ g = a.tab + (size_t)row * a.nfields * stride;
  for (int f = 0; f < nf; ++f) {
    const int o = a.out[f] * stride;
    for (int i = threadIdx.x; i < stride; i += blockDim.x) {
      const unsigned v = t[f * stride + i];
      if (v) {
        atomicAdd(&g[o + i], (unsigned long long)v);
        t[f * stride + i] = 0u;
      }
    }
  }
}
__device__ __forceinline__ void ipdf_count(unsigned* t, const double* __restrict__ rng, double x, int bins) {
  atomicAdd(&t[hist_bin(x, rng[0], rng[1], rng[2], bins)], 1u);
}

// ---- fused grids, Kernel family: k_x_flow_sf's front, then one LDS table per separation ------------------------------------------
// The value rows go to LDS as in k_x_flow_sf; per separation every thread counts the increments of its P points of each selected
// slot (the LDS row minus its registers, the very subtraction of k_x_flow_sf) and, after ONE barrier, the table is flushed and left
// zero.  Two tables alternate: the flush of separation s runs beside the counting of s + 1 in the other table; a table is counted
// into again at s + 2, behind the barrier of s + 1, which every thread reaches only after its flush of s.
template <int N, int MODE>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_flow_ipdf(MArr Mq, MArr Mqw, MArr Mu, MArr Mp, MArr Mphi, MArr Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
              FlowSel sel, IpdfArgs a) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T, C = X::C, NV = flow_nv<N>();
  static_assert(ipdf_lds_bytes<N>(NV, 0, IPDF_MAX_BINS) <= 160 * 1024 && ipdf_lds_bytes<N>(NV - 1, 1, IPDF_MAX_BINS) <= 160 * 1024,
                "value rows and the two tables exceed the 160 KB of a CU");
  double val[NV][P];
  cd w[P];
  x_flow_values<N, MODE, false>(Mq, Mqw, Mu, Mp, Mphi, Mphiy, tw, kk, sel, val, w);
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  double* rows = reinterpret_cast<double*>(nq_smem);
  cd* prow = reinterpret_cast<cd*>(rows + (size_t)a.nreal * C * N) + c * N;
  const int nf = a.nreal + a.phi, stride = a.bins + 3, words = ipdf_words(nf, a.bins);
  unsigned* tabs = reinterpret_cast<unsigned*>(rows + sf_row_doubles<N>(a.nreal, a.phi));
#pragma unroll
  for (int f = 0; f < NV; ++f) {
    if (f < a.nreal) {
      double* row = rows + ((size_t)f * C + c) * N + j;
#pragma unroll
      for (int t = 0; t < P; ++t) row[t * T] = val[f][t];
    }
  }
  if (a.phi) {
#pragma unroll
    for (int t = 0; t < P; ++t) prow[j + t * T] = w[t];
  }
  hist_zero(tabs, 2 * words);
  NQ_PHASE_FENCE();
  wg_barrier();
#pragma unroll 1
  for (int s = 0; s < a.nsep; ++s) {
    const int r = a.seps[s];
    unsigned* tab = tabs + (s & 1) * words;
    const double* __restrict__ rng = a.rng + (size_t)s * a.nfields * 3;
#pragma unroll
    for (int t = 0; t < P; ++t) {
      int xr = j + t * T + r;
      xr = xr >= N ? xr - N : xr;
#pragma unroll
      for (int f = 0; f < NV; ++f) {
        if (f < a.nreal) {
          const double d = rows[((size_t)f * C + c) * N + xr] - val[f][t];
          ipdf_count(tab + f * stride, rng + 3 * a.out[f], d, a.bins);
        }
      }
      if (a.phi) {
        const cd p = prow[xr];
        const double dr = p.x - w[t].x, di = p.y - w[t].y;
        ipdf_count(tab + a.nreal * stride, rng + 3 * a.out[a.nreal], sqrt(dr * dr + di * di), a.bins);
      }
    }
    wg_barrier();
    ipdf_flush(tab, nf, a, s);
  }
}

// ---- planes: QGModel on the fused grids, the any-size path, every two-dimensional call -------------------------------------------
// Planes as in SfPlanes (stride doubles per element, the complex one last).  Per vector a workgroup walks rows y = blockIdx.x,
// blockIdx.x + gridDim.x, ... (both values of an increment from global memory), counts into one of two alternating LDS tables and
// flushes once (as above).  The optional rotation of the pair (pa, pb) is sf2_point's: L = c_x d_a + c_y d_b, T = c_x d_b - c_y d_a.
__global__ void __launch_bounds__(IPDF_PLANE_THREADS) k_ipdf_plane(SfPlanes pl, IpdfArgs a) {
  constexpr int NF = SF_MAX_FIELDS;
  const int nf = a.nreal + a.phi, stride = a.bins + 3, words = ipdf_words(nf, a.bins);
  unsigned* tabs = reinterpret_cast<unsigned*>(nq_smem);
  hist_zero(tabs, 2 * words);
  __syncthreads();
#pragma unroll 1
  for (int v = 0; v < a.nsep; ++v) {
    const Sf2Vec r = a.vecs[v];
    unsigned* tab = tabs + (v & 1) * words;
    const double* __restrict__ rng = a.rng + (size_t)r.slot * a.nfields * 3;
    double cx = 1.0, cy = 0.0;
    if (a.proj) {
      cx = a.proj[2 * r.slot];
      cy = a.proj[2 * r.slot + 1];
    }
    for (int y = blockIdx.x; y < pl.rows; y += gridDim.x) {
      int yr = y + r.ry;
      yr = yr >= pl.rows ? yr - pl.rows : yr;
      for (int x = threadIdx.x; x < pl.cols; x += IPDF_PLANE_THREADS) {
        int xr = x + r.rx;
        xr = xr >= pl.cols ? xr - pl.cols : xr;
        const size_t at = (size_t)y * pl.cols + x, atr = (size_t)yr * pl.cols + xr;
        double d[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) d[f] = f < a.nreal ? pl.p[f][atr * pl.stride[f]] - pl.p[f][at * pl.stride[f]] : 0.0;
        if (a.pa >= 0) {
          const double da = sf_pick(a.pa, d[0], d[1], d[2]), db = sf_pick(a.pb, d[0], d[1], d[2]);
          const double L = cx * da + cy * db, Tr = cx * db - cy * da;
#pragma unroll
          for (int f = 0; f < NF; ++f) d[f] = f == a.pa ? L : (f == a.pb ? Tr : d[f]);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f)
          if (f < a.nreal) ipdf_count(tab + f * stride, rng + 3 * a.out[f], d[f], a.bins);
        if (a.phi) {
          const double* __restrict__ p = pl.p[a.nreal];
          const double dr = p[atr * 2] - p[at * 2], di = p[atr * 2 + 1] - p[at * 2 + 1];
          ipdf_count(tab + a.nreal * stride, rng + 3 * a.out[a.nreal], sqrt(dr * dr + di * di), a.bins);
        }
      }
    }
    __syncthreads();
    ipdf_flush(tab, nf, a, r.slot);
  }
}

}  // namespace nq
