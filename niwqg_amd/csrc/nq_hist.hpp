// PDFs and joint PDFs of the physical fields (include/niwqg_amd.h: nq_field_hist, nq_any_hist).
//
// Counts only: integer counters are the one reduction that may use atomics and still be bit-reproducible.  Every workgroup
// counts into a table of 32-bit counters in LDS (atomicAdd on LDS) and adds its non-zero entries to the 64-bit global tables
// with integer atomics.  Real fields are sharply peaked (most of a plane sits in a handful of bins), so counting straight into
// global memory would serialise on a few words.
//
// Table layout, LDS and global alike (`bins`, `jbins` of the call):
//   slot f (0..2) at f * (bins + 3): [0, bins) the bins, [bins] below, [bins + 1] above, [bins + 2] NaN
//   joint table at 3 * (bins + 3):   [ib * jbins + ia], then [jbins^2] = points with either value outside or NaN
#pragma once
#include "nq_step.hpp"

namespace nq {

constexpr int HIST_SLOTS = 3;
constexpr int HIST_MAX_BINS = 1024, HIST_MAX_JBINS = 128;
constexpr int HIST_MAX_WORDS = HIST_SLOTS * (HIST_MAX_BINS + 3) + HIST_MAX_JBINS * HIST_MAX_JBINS + 1;
constexpr int HIST_PART_BLOCKS = 8192;        // workgroup partials of the min/max pass: [block][6] doubles
// the LDS tables ALIAS the row plan's exchange (they are used only after the row's last transform), so a launch needs
// max(plan, tables) bytes: both are checked against the 160 KB of a CU for every N (hist_lds_bytes below)
static_assert((size_t)HIST_MAX_WORDS * sizeof(unsigned) <= 160 * 1024, "the largest LDS tables exceed the 160 KB of a CU");

struct HistArgs {
  double lo[HIST_SLOTS], hi[HIST_SLOTS], s[HIST_SLOTS];   // s = bins / (hi - lo), formed once on the host
  double js[2];                                           // jbins / (hi - lo) of the joint pair
  int bins, jbins;                                        // jbins = 0: no joint table
  int mask;                                               // bit f: slot f is binned
  int ja, jb;                                             // slots of the joint pair
  unsigned long long* tab;                                // global tables
};
__host__ __device__ inline int hist_words(int bins, int jbins) {
  return HIST_SLOTS * (bins + 3) + (jbins ? jbins * jbins + 1 : 0);
}

// THE bin rule (fp64, host and device alike; niwqg_amd/pdfs.py: bin_index restates it): NaN -> bins + 2, x < lo -> bins,
// x > hi -> bins + 1, else min((int) floor((x - lo) * s), bins - 1): x == hi lands in the last bin.  (x - lo) * s is not reordered.
__host__ __device__ __forceinline__ int hist_bin(double x, double lo, double hi, double s, int bins) {
  if (x != x) return bins + 2;
  if (x < lo) return bins;
  if (x > hi) return bins + 1;
  const double d = x - lo;
  const int i = (int)floor(d * s);
  return i < bins - 1 ? i : bins - 1;
}

__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || a < b) ? a : b; }    // see nan_max (nq_generic.hpp)

__device__ __forceinline__ void hist_zero(unsigned* t, int words) {
  for (int i = threadIdx.x; i < words; i += blockDim.x) t[i] = 0u;
}
__device__ __forceinline__ void hist_flush(const unsigned* t, int words, unsigned long long* __restrict__ g) {
  for (int i = threadIdx.x; i < words; i += blockDim.x) {
    const unsigned v = t[i];
    if (v) atomicAdd(&g[i], (unsigned long long)v);
  }
}
// one point: its (up to) three values into the 1-D tables of the masked slots and the pair's into the joint table
__device__ __forceinline__ void hist_count(unsigned* t, const HistArgs& h, double v0, double v1, double v2) {
  const int stride = h.bins + 3;
  if (h.mask & 1) atomicAdd(&t[hist_bin(v0, h.lo[0], h.hi[0], h.s[0], h.bins)], 1u);
  if (h.mask & 2) atomicAdd(&t[stride + hist_bin(v1, h.lo[1], h.hi[1], h.s[1], h.bins)], 1u);
  if (h.mask & 4) atomicAdd(&t[2 * stride + hist_bin(v2, h.lo[2], h.hi[2], h.s[2], h.bins)], 1u);
  if (h.jbins) {
    const double va = h.ja == 0 ? v0 : (h.ja == 1 ? v1 : v2), vb = h.jb == 0 ? v0 : (h.jb == 1 ? v1 : v2);
    const int ia = hist_bin(va, h.lo[h.ja], h.hi[h.ja], h.js[0], h.jbins);
    const int ib = hist_bin(vb, h.lo[h.jb], h.hi[h.jb], h.js[1], h.jbins);
    const int slot = (ia < h.jbins && ib < h.jbins) ? ib * h.jbins + ia : h.jbins * h.jbins;
    atomicAdd(&t[HIST_SLOTS * stride + slot], 1u);
  }
}

// NaN-propagating minima and maxima of NV values over a workgroup of full waves -> dst[2 i] = min, dst[2 i + 1] = max of value i
// (thread 0 stores; one slot per workgroup, the host takes the minimum of the slots: order does not matter to min and max).
// `scratch`: 16 waves x 2 NV doubles of LDS nobody else uses any more.
template <int NV>
__device__ __forceinline__ void block_minmax_store(double (&mn)[NV], double (&mx)[NV], double* scratch, double* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[i] = nan_min(mn[i], __shfl_xor(mn[i], off, 64));
      mx[i] = nan_max(mx[i], __shfl_xor(mx[i], off, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      scratch[(wave * NV + i) * 2] = mn[i];
      scratch[(wave * NV + i) * 2 + 1] = mx[i];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double a = scratch[i * 2], b = scratch[i * 2 + 1];
      for (int w = 1; w < nw; ++w) {
        a = nan_min(a, scratch[(w * NV + i) * 2]);
        b = nan_max(b, scratch[(w * NV + i) * 2 + 1]);
      }
      dst[2 * i] = a;
      dst[2 * i + 1] = b;
    }
  }
}

template <int N> constexpr size_t hist_lds_bytes(int words) {
  return XPlan<N>::LDS_BYTES > (size_t)words * sizeof(unsigned) ? XPlan<N>::LDS_BYTES : (size_t)words * sizeof(unsigned);
}

// ---- fused grids, Kernel family: k_x_diag's loads, packing and two transforms, then bin instead of sum ----------------------
// One row block: q, q_psi from the (q, qw) half-spectrum pair, phi from its mixed-space row (the values the tick's sums
// [16..23] see); slots 0 = q, 1 = q_psi, 2 = |phi|^2.  No physical plane is written.  MINMAX: the range pass instead, part[block][6] =
// min q, max q, min q_psi, max q_psi, min |phi|^2, max |phi|^2 (NaN when any value is).
// The tables alias the exchange: the row's values are in registers after the second transform and nothing reads the exchange
// or the twiddles after it.
// The part both k_x_hist and k_x_moments (nq_avg.hpp) run: the loads, the packing and the two transforms of one row block, up to
// "values in registers": q[t], qpsi[t] and phi[t] of point j + t * T of the thread's row.  On return every wave is through its
// last exchange: the LDS (the twiddles included) is free.  PHI = false (k_x_get_zeta, nq_particles.hpp): q and q_psi only, the phi row
// is neither read nor transformed (w returns the transformed (q, q_w) pair).
template <int N, int MODE, bool SLAB, bool PHI = true>
__device__ __forceinline__ void x_row_values(const MArr& Mq, const MArr& Mqw, const MArr& Mphi, const cd* __restrict__ tw,
                                             const double* __restrict__ kk, double (&q)[XPlan<N>::P], double (&qpsi)[XPlan<N>::P],
                                             cd (&w)[XPlan<N>::P]) {
  typedef XPlan<N> X;
  typedef typename X::F F;
  constexpr int P = X::P, T = X::T;
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t row = (size_t)blockIdx.x * X::C + c;
  cd* lds = reinterpret_cast<cd*>(nq_smem);
  cd* twl = lds + F::LDS_ELEMS;
  for (int i = threadIdx.x; i < F::TW_LDS_ELEMS; i += X::THREADS) twl[i] = tw[i];
  typename F::TwLds twr;
  twr.base = twl;
  wg_barrier_all();
  HsRegs<P> h1;
  hs_load<N, P, T, MODE == MODE_COUPLED>(h1, xrow<SLAB>(Mq, row), xrow<SLAB>(MODE == MODE_COUPLED ? Mqw : Mq, row), j);
  NQ_PHASE_FENCE();
  hs_pack<N, P, T, F, MODE == MODE_COUPLED>(w, h1, j, c, lds, kk, false, false);
  NQ_PHASE_FENCE();
  F::template run<true>(w, j, c, lds, twr);
#pragma unroll
  for (int t = 0; t < P; ++t) {
    q[t] = w[t].x;
    qpsi[t] = (MODE == MODE_COUPLED) ? w[t].x - w[t].y : w[t].x;
  }
  if constexpr (PHI) {
    const XRowT<SLAB> rp = xrow<SLAB>(Mphi, row);
#pragma unroll
    for (int t = 0; t < P; ++t) w[t] = *rp.at(j + t * T);
    NQ_PHASE_FENCE();
    F::template run<true>(w, j, c, lds, twr);
  }
  NQ_PHASE_FENCE();
  wg_barrier_all();                                  // every wave is through its last exchange: the LDS is free
}

template <int N, int MODE, bool SLAB, bool MINMAX>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_hist(MArr Mq, MArr Mqw, MArr Mphi, const cd* __restrict__ tw, const double* __restrict__ kk, HistArgs h,
         double* __restrict__ part) {
  typedef XPlan<N> X;
  static_assert(hist_lds_bytes<N>(HIST_MAX_WORDS) <= 160 * 1024, "row plan or LDS tables exceed the 160 KB of a CU");
  static_assert(X::LDS_BYTES >= 16 * 6 * sizeof(double), "min/max scratch");
  constexpr int P = X::P;
  double q[P], qpsi[P];
  cd w[P];
  x_row_values<N, MODE, SLAB>(Mq, Mqw, Mphi, tw, kk, q, qpsi, w);
  if (MINMAX) {
    double mn[3] = {q[0], qpsi[0], 0.0}, mx[3] = {q[0], qpsi[0], 0.0};
    mn[2] = mx[2] = w[0].x * w[0].x + w[0].y * w[0].y;
#pragma unroll
    for (int t = 1; t < P; ++t) {
      const double a2 = w[t].x * w[t].x + w[t].y * w[t].y;
      mn[0] = nan_min(mn[0], q[t]);
      mx[0] = nan_max(mx[0], q[t]);
      mn[1] = nan_min(mn[1], qpsi[t]);
      mx[1] = nan_max(mx[1], qpsi[t]);
      mn[2] = nan_min(mn[2], a2);
      mx[2] = nan_max(mx[2], a2);
    }
    block_minmax_store<3>(mn, mx, reinterpret_cast<double*>(nq_smem), part + 6 * (size_t)blockIdx.x);
  } else {
    unsigned* tab = reinterpret_cast<unsigned*>(nq_smem);
    const int words = hist_words(h.bins, h.jbins);
    hist_zero(tab, words);
    wg_barrier_all();
#pragma unroll
    for (int t = 0; t < P; ++t) hist_count(tab, h, q[t], qpsi[t], w[t].x * w[t].x + w[t].y * w[t].y);
    wg_barrier_all();
    hist_flush(tab, words, h.tab);
  }
}

// ---- element-wise: the any-size path and QGModel on the fused grids ----------------------------------------------------
// Values of up to two planes of `n` elements, `stride` doubles per element (1: a real plane, 2: a complex one); what = 0: the
// first double (Re), 1: |a|^2 (complex planes).  Plane a -> slot 0, plane b -> slot 1.
__device__ __forceinline__ double hist_val(const double* __restrict__ p, size_t i, int stride, int what) {
  const double re = p[i * stride];
  if (what == 0) return re;
  const double im = p[i * stride + 1];
  return re * re + im * im;
}
__global__ void __launch_bounds__(256) k_hist_plane(const double* __restrict__ a, const double* __restrict__ b, size_t n, int stride,
                                                    int wa, int wb, HistArgs h) {
  unsigned* tab = reinterpret_cast<unsigned*>(nq_smem);
  const int words = hist_words(h.bins, h.jbins);
  hist_zero(tab, words);
  __syncthreads();
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
    hist_count(tab, h, a ? hist_val(a, i, stride, wa) : 0.0, b ? hist_val(b, i, stride, wb) : 0.0, 0.0);
  __syncthreads();
  hist_flush(tab, words, h.tab);
}
// part[block][4] = min a, max a, min b, max b (NaN when any value is); n >= 1
__global__ void __launch_bounds__(256) k_minmax_plane(const double* __restrict__ a, const double* __restrict__ b, size_t n, int stride,
                                                      int wa, int wb, double* __restrict__ part) {
  __shared__ double scratch[4 * 2 * 2];
  // threads past the end start from element 0: min and max do not mind a value seen twice
  const size_t step = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double a0 = a ? hist_val(a, i0 < n ? i0 : 0, stride, wa) : 0.0, b0 = b ? hist_val(b, i0 < n ? i0 : 0, stride, wb) : 0.0;
  double mn[2] = {a0, b0}, mx[2] = {a0, b0};
  for (size_t i = i0 + step; i < n; i += step) {
    if (a) {
      const double v = hist_val(a, i, stride, wa);
      mn[0] = nan_min(mn[0], v);
      mx[0] = nan_max(mx[0], v);
    }
    if (b) {
      const double v = hist_val(b, i, stride, wb);
      mn[1] = nan_min(mn[1], v);
      mx[1] = nan_max(mx[1], v);
    }
  }
  block_minmax_store<2>(mn, mx, scratch, part + 4 * (size_t)blockIdx.x);
}

}  // namespace nq
