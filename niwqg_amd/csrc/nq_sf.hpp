// Structure functions of the physical fields: moments of the x-increments d_r a(x, y) = a((x + r) mod nx, y) - a(x, y)
// (include/niwqg_amd.h: nq_structure, nq_any_increments; niwqg_amd/structure.py: reference restates the
// definitions in numpy).
//
// Raw SUMS over the plane, SF_COLS = 9 columns per field and separation:
//   a real field      [p - 1] = sum d^p, p = 1..6;      [6] = sum |d|,    [7] = sum |d|^3,  [8] = sum |d|^5
//   the complex phi   [p - 1] = sum |d phi|^p, p = 1..6; [6] = sum Re d,   [7] = sum Im d,   [8] = 0
// and one column per mixed triple (a, b, c): sum d_a d_b d_c, or sum d_a |d phi|^2 for (a, phi, phi).  Powers are formed by
// successive multiplication (d^p = d^(p-1) d; |d|^3 = |d^3|; |d phi|^3 = |d phi|^2 |d phi|, ^5 = ^4 |d phi|).
//
// Field slots of a launch are CANONICAL: the real fields first, in the call's order (slot f < nreal reads value register f of
// x_flow_values), then phi, if selected, in slot nreal.  The host maps the call's order to this one.
//
// Sums are deterministic: a thread adds its points, a wave its lanes (wave_sum_full), the workgroup its waves in index order,
// one slot per workgroup and separation in `part`; k_sf_total adds the slots in a fixed order into the running table.  No
// floating-point atomics.
#pragma once
#include "nq_flow.hpp"

namespace nq {

constexpr int SF_COLS = 9, SF_MAX_SEPS = 64, SF_MAX_FIELDS = 3, SF_MAX_TRIPLES = 4;
constexpr int SF_PLANE_THREADS = 256;
// triples a launch of NF field slots can hold (one slot: only (a, a, a)) and the columns of one of its partial slots
template <int NF> constexpr int sf_ntri() { return NF == 1 ? 1 : SF_MAX_TRIPLES; }
template <int NF> constexpr int sf_ncols() { return NF * SF_COLS + sf_ntri<NF>(); }

struct SfArgs {
  int nsep;
  const int* seps;                    // nsep separations on the device, 1 <= r <= N - 1
  int nreal, phi;                     // real field slots 0..nreal-1, phi (0 / 1) in slot nreal
  int ntri, ta[SF_MAX_TRIPLES], tb[SF_MAX_TRIPLES], tc[SF_MAX_TRIPLES];      // slots of a triple; tb = -1: (ta, phi, phi)
  double* part;                       // [block][separation][sf_ncols<NF>()]
};

__device__ __forceinline__ double sf_pick(int s, double d0, double d1, double d2) { return s == 0 ? d0 : (s == 1 ? d1 : d2); }

// the nine columns of one real increment / of one complex increment, added to acc
__device__ __forceinline__ void sf_add_real(double (&acc)[SF_COLS], double d) {
  const double d2 = d * d, d3 = d2 * d, d4 = d3 * d, d5 = d4 * d, d6 = d5 * d;
  acc[0] += d;
  acc[1] += d2;
  acc[2] += d3;
  acc[3] += d4;
  acc[4] += d5;
  acc[5] += d6;
  acc[6] += fabs(d);
  acc[7] += fabs(d3);
  acc[8] += fabs(d5);
}
__device__ __forceinline__ void sf_add_phi(double (&acc)[SF_COLS], double dr, double di, double m2) {
  const double m1 = sqrt(m2), m3 = m2 * m1, m4 = m2 * m2, m5 = m4 * m1, m6 = m4 * m2;
  acc[0] += m1;
  acc[1] += m2;
  acc[2] += m3;
  acc[3] += m4;
  acc[4] += m5;
  acc[5] += m6;
  acc[6] += dr;
  acc[7] += di;
}

template <int NF>
__device__ __forceinline__ void sf_zero(double (&acc)[NF][SF_COLS], double (&tri)[sf_ntri<NF>()]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
#pragma unroll
    for (int i = 0; i < SF_COLS; ++i) acc[f][i] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < sf_ntri<NF>(); ++k) tri[k] = 0.0;
}
// Workgroup sums of the NC = sf_ncols<NF>() per-thread values (full waves) -> dst[0..NC), waves added in index order.  `buf`:
// nw * NC doubles of LDS; the caller alternates two of them, so one barrier per call suffices (a buffer is rewritten two calls
// later, after the barrier of the call in between, which its readers reach only after their reads).
template <int NF>
__device__ __forceinline__ void sf_block_store(double (&acc)[NF][SF_COLS], double (&tri)[sf_ntri<NF>()], double* buf, double* __restrict__ dst,
                                               bool add = false) {          // add: on top of dst (the same workgroup wrote it before)
  constexpr int NC = sf_ncols<NF>();
  const int tid = threadIdx.x, wave = tid >> 6, nw = (int)blockDim.x >> 6;
#pragma unroll
  for (int i = 0; i < NC; ++i) {                         // one value at a time: the wave sum's lane reads stay short-lived
    const double x = wave_sum_full(i < NF * SF_COLS ? acc[i / SF_COLS][i % SF_COLS] : tri[i < NF * SF_COLS ? 0 : i - NF * SF_COLS]);
    if ((tid & 63) == 0) buf[wave * NC + i] = x;
    __builtin_amdgcn_sched_barrier(0);
  }
  wg_barrier();
  if (tid < NC) {
    double x = 0.0;
    for (int w = 0; w < nw; ++w) x += buf[w * NC + tid];
    dst[tid] = add ? dst[tid] + x : x;
  }
}

// LDS of a launch: the rows of the selected values (a real value C N doubles, phi C N complex), then the two reduction buffers
template <int N> __host__ __device__ constexpr size_t sf_row_doubles(int nreal, int phi) {
  return (size_t)(nreal + 2 * phi) * XPlan<N>::C * N;
}
template <int N> constexpr size_t sf_lds_bytes(int nreal, int phi) {
  const size_t mine = (sf_row_doubles<N>(nreal, phi) + 2 * (XPlan<N>::THREADS / 64) * sf_ncols<flow_nv<N>()>()) * sizeof(double);
  return XPlan<N>::LDS_BYTES > mine ? XPlan<N>::LDS_BYTES : mine;
}

// ---- fused grids, Kernel family: x_flow_values' row block, then the increments out of LDS rows ------------------------------------
// Each thread stores its P points of every selected value to a row-major LDS row (row c of the workgroup at offset c N), and
// reads point (j + t T + r) mod N of its own row per separation: lanes read consecutive doubles.
template <int N, int MODE, bool SLAB = false>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_flow_sf(MArr Mq, MArr Mqw, MArr Mu, MArr Mp, MArr Mphi, MArr Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
            FlowSel sel, SfArgs a) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T, C = X::C, NV = flow_nv<N>(), NF = NV, NC = sf_ncols<NF>();
  static_assert(sf_lds_bytes<N>(NV, 0) <= 160 * 1024 && sf_lds_bytes<N>(NV - 1, 1) <= 160 * 1024, "value rows exceed the 160 KB of a CU");
  static_assert(X::THREADS % 64 == 0 && X::THREADS >= NC, "full waves; one thread per column in the workgroup sum");
  double val[NV][P];
  cd w[P];
  x_flow_values<N, MODE, SLAB>(Mq, Mqw, Mu, Mp, Mphi, Mphiy, tw, kk, sel, val, w);
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  double* rows = reinterpret_cast<double*>(nq_smem);
  cd* prow = reinterpret_cast<cd*>(rows + (size_t)a.nreal * C * N) + c * N;
  double* red = rows + sf_row_doubles<N>(a.nreal, a.phi);
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
  NQ_PHASE_FENCE();
  wg_barrier();
#pragma unroll 1
  for (int s = 0; s < a.nsep; ++s) {
    const int r = a.seps[s];
    double acc[NF][SF_COLS], tri[sf_ntri<NF>()];
    sf_zero<NF>(acc, tri);
#pragma unroll
    for (int t = 0; t < P; ++t) {
      int xr = j + t * T + r;
      xr = xr >= N ? xr - N : xr;
      double d[NF], m2 = 0.0;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        d[f] = 0.0;
        if (f < a.nreal) {
          d[f] = rows[((size_t)f * C + c) * N + xr] - val[f][t];
          sf_add_real(acc[f], d[f]);
        } else if (f == a.nreal && a.phi) {
          const cd p = prow[xr];
          const double dr = p.x - w[t].x, di = p.y - w[t].y;
          m2 = dr * dr + di * di;
          sf_add_phi(acc[f], dr, di, m2);
        }
      }
#pragma unroll
      for (int k = 0; k < sf_ntri<NF>(); ++k) {
        if (k < a.ntri) {
          const double da = sf_pick(a.ta[k], d[0], d[NF > 1 ? 1 : 0], d[NF - 1]);
          tri[k] += a.tb[k] < 0 ? da * m2
                                : da * sf_pick(a.tb[k], d[0], d[NF > 1 ? 1 : 0], d[NF - 1]) * sf_pick(a.tc[k], d[0], d[NF > 1 ? 1 : 0], d[NF - 1]);
        }
      }
    }
    sf_block_store<NF>(acc, tri, red + (s & 1) * (X::THREADS / 64) * NC, a.part + ((size_t)blockIdx.x * a.nsep + s) * NC);
  }
}

// ---- planes: QGModel on the fused grids and the any-size path ------------------------------------------------------------------
// Up to SF_MAX_FIELDS planes of (rows, cols) elements, `stride` doubles per element (1: a real plane, 2: a complex one), kind 0:
// the first double (Re), 2: the complex value (the phi columns).  Field slots in the canonical order above (a complex plane
// last).  One workgroup walks rows with a grid-stride loop; increments come straight from global memory (a row is re-read per
// separation).  part: [block][separation][sf_ncols<SF_MAX_FIELDS>()].
struct SfPlanes {
  const double* p[SF_MAX_FIELDS];
  int stride[SF_MAX_FIELDS];
  int rows, cols;
};
__global__ void __launch_bounds__(SF_PLANE_THREADS) k_sf_plane(SfPlanes pl, SfArgs a) {
  constexpr int NF = SF_MAX_FIELDS, NC = sf_ncols<NF>();
  __shared__ double red[2 * (SF_PLANE_THREADS / 64) * NC];
#pragma unroll 1
  for (int s = 0; s < a.nsep; ++s) {
    const int r = a.seps[s];
    double acc[NF][SF_COLS], tri[sf_ntri<NF>()];
    sf_zero<NF>(acc, tri);
    for (int row = blockIdx.x; row < pl.rows; row += gridDim.x) {
      for (int x = threadIdx.x; x < pl.cols; x += SF_PLANE_THREADS) {
        int xr = x + r;
        xr = xr >= pl.cols ? xr - pl.cols : xr;
        const size_t at = (size_t)row * pl.cols + x, atr = (size_t)row * pl.cols + xr;
        double d[NF], m2 = 0.0;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          d[f] = 0.0;
          if (f < a.nreal) {
            d[f] = pl.p[f][atr * pl.stride[f]] - pl.p[f][at * pl.stride[f]];
            sf_add_real(acc[f], d[f]);
          } else if (f == a.nreal && a.phi) {
            const double dr = pl.p[f][atr * 2] - pl.p[f][at * 2], di = pl.p[f][atr * 2 + 1] - pl.p[f][at * 2 + 1];
            m2 = dr * dr + di * di;
            sf_add_phi(acc[f], dr, di, m2);
          }
        }
#pragma unroll
        for (int k = 0; k < sf_ntri<NF>(); ++k) {
          if (k < a.ntri) {
            const double da = sf_pick(a.ta[k], d[0], d[1], d[2]);
            tri[k] += a.tb[k] < 0 ? da * m2 : da * sf_pick(a.tb[k], d[0], d[1], d[2]) * sf_pick(a.tc[k], d[0], d[1], d[2]);
          }
        }
      }
    }
    sf_block_store<NF>(acc, tri, red + (s & 1) * (SF_PLANE_THREADS / 64) * NC, a.part + ((size_t)blockIdx.x * a.nsep + s) * NC);
  }
}

// The second step: entry i = separation * nc + column of the table gets the slots of the nblk workgroups, added in a FIXED order
// (on top of what it holds with `accumulate`): the slots are cut into SF_TOTAL_RUNS contiguous runs, one thread adds a run in
// index order, then the run sums are added in index order.  (One thread per entry walking all slots is a chain of up to 8192
// dependent loads: 1.4 ms of a 4096^2 call.)  Column c of the partials lands in column map[c] of the table row (nout wide; map[c]
// < 0: not part of the call).
constexpr int SF_TOTAL_RUNS = 64, SF_TOTAL_ENTRIES = 4;       // per workgroup of 256 threads
struct SfMap {
  int col[sf_ncols<SF_MAX_FIELDS>()];
};
__global__ void __launch_bounds__(SF_TOTAL_RUNS * SF_TOTAL_ENTRIES)
k_sf_total(const double* __restrict__ part, int nblk, int nsep, int nc, SfMap map, int nout, int accumulate, double* __restrict__ tab) {
  __shared__ double run[SF_TOTAL_RUNS][SF_TOTAL_ENTRIES];
  const int e = threadIdx.x % SF_TOTAL_ENTRIES, g = threadIdx.x / SF_TOTAL_ENTRIES;
  const int n = nsep * nc, i = blockIdx.x * SF_TOTAL_ENTRIES + e;
  double x = 0.0;
  if (i < n) {
    const int per = (nblk + SF_TOTAL_RUNS - 1) / SF_TOTAL_RUNS, b0 = g * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    for (int b = b0; b < b1; ++b) x += part[(size_t)b * n + i];
  }
  run[g][e] = x;
  __syncthreads();
  if (g != 0 || i >= n) return;
  const int s = i / nc, c = i - s * nc;
  const int o = map.col[c];
  if (o < 0) return;
  double t = 0.0;
  for (int k = 0; k < SF_TOTAL_RUNS; ++k) t += run[k][e];
  double* dst = tab + (size_t)s * nout + o;
  *dst = accumulate ? *dst + t : t;
}

}  // namespace nq
