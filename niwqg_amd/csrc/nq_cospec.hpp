// Isotropic co-spectra of up to three physical fields (include/niwqg_amd.h: nq_cospectra;
// niwqg_amd/cospectra.py: reference restates the definitions in numpy).
//
// With F the unnormalised full-plane transform, A = F[a], B = F[b], C = F[c] of the real fields a, b, c of a call, the rows are the
// raw shell sums (no 1 / M^2)
//   [0] |A|^2   [1] |B|^2   [2] |C|^2   [3] Re(conj A B)   [4] Re(conj A C)   [5] Re(conj B C)
// (rows of fields the call does not have are zero).  The quadrature parts Im(conj A B) sum to zero over +-k and are not formed.
//
//   k_x_cross<N, MODE, SLAB, FLOW>  one row block: the selected values in registers by x_row_values (a list of q, q_psi, phi2) or
//                 x_flow_values (FLOW: a list that names a flow field) -- exactly what the PDFs bin and the averages sum --, packed
//                 as the complex row a + i b, transformed forward and stored as a FULL mixed-space row into Mw, which is free
//                 between steps; with a third field c + i 0 follows into a scratch plane (not into Muq, Mvq: their padding column
//                 Muq.W carries k_x_products' passenger sums and must stay zero on the rows that kernel does not write).
//                 A thread keeps c across the first forward transform, nothing else.  No physical plane is written.
//   BinCross      k_bin_shells term on the full planes Z = F[a + i b] and C: with Z* = conj Z(-l, -k), indices modulo N,
//                 A = (Z + Z*) / 2 and B = (Z - Z*) / (2i), the split unpack_pair_store applies to a row.
//   BinQC         QGModel: q-hat and c-hat are the state, so the term reads the half spectra: weight 2 on the interior columns,
//                 the Hermitian part in l on columns 0 and N/2 with weight 1 (k_diag_c's rule: what physical space sees).
//   k_cospec_add  the call's table into the running sums.
//   k_cospec_scale  the powers of two the fields are packed with, from the range pass's workgroup partials:
// Two fields that share a transform share its rounding: every coefficient of Z carries an error of a few ulp of the LARGER
// field's coefficients, so q_psi (1e-5) packed with |phi|^2 (1e-2), or q_psi with ow (1e-11), would lose the smaller one's
// digits in proportion (the reason k_x_products rescales q_w against q).  Each field is therefore multiplied by a power of two
// that brings its largest |value| into [1, 2) before packing, and BinCross multiplies the split parts by the inverse powers:
// both exact.  The largest |values| come from the PDFs' own range pass (k_x_hist / k_x_flow_hist with MINMAX: one more row pass,
// no new kernel) through k_cospec_scale; nothing of it crosses to the host.
// 8192-point rows: a thread holds one flow value there (flow_nv), so FLOW is not instantiated and such a list is refused.
#pragma once
#include "nq_flow.hpp"

namespace nq {

constexpr int COSPEC_FIELDS = 3, COSPEC_ROWS = 6;
static_assert(COSPEC_FIELDS == HIST_SLOTS, "one value slot of the row pass per field");

__device__ __forceinline__ double cross_pick(int code, double q, double qpsi, double a2) {
  return code == FLOW_Q ? q : (code == FLOW_QPSI ? qpsi : (code == FLOW_PHI2 ? a2 : 0.0));
}
template <int N, bool SLAB>
__device__ __forceinline__ void cross_store(const cd (&w)[XPlan<N>::P], const MArr& M, size_t row, int j) {
  constexpr int P = XPlan<N>::P, T = XPlan<N>::T;
  const XRowT<SLAB> rp = xrow<SLAB>(M, row);
#pragma unroll
  for (int t = 0; t < P; ++t) *rp.at(j + t * T) = w[t];
}

// The scales of a call: scl[i] = 2^-e_i with e_i the binary exponent of max |field i| over the plane (1 for a field that is zero,
// subnormal throughout, not finite or not in the list), scl[3 + i] = 2^e_i, and 0 for a field whose maximum |value| is exactly 0:
// BinCross multiplies the field's split part by it, so the rows of a vanishing field are exact zeros.  part: the workgroup partials of the PDFs' range pass (k_x_hist /
// k_x_flow_hist with MINMAX), `per` doubles per workgroup, minimum and maximum of field i at [2 slot[i]], [2 slot[i] + 1].
// One workgroup of 256 threads; a maximum does not depend on the order it is taken in.
struct CrossSlots { int slot[COSPEC_FIELDS]; };
__global__ void __launch_bounds__(256) k_cospec_scale(const double* __restrict__ part, int nblk, int per, CrossSlots s, double* __restrict__ scl) {
  __shared__ double sh[4][COSPEC_FIELDS];
  double top[COSPEC_FIELDS] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += 256) {
#pragma unroll
    for (int i = 0; i < COSPEC_FIELDS; ++i) {
      if (s.slot[i] >= 0) {
        const double lo = fabs(part[(size_t)b * per + 2 * s.slot[i]]), hi = fabs(part[(size_t)b * per + 2 * s.slot[i] + 1]);
        top[i] = nan_max(top[i], nan_max(lo, hi));
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < COSPEC_FIELDS; ++i) {
    double x = top[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = nan_max(x, __shfl_xor(x, off, 64));
    if (lane == 0) sh[wave][i] = x;
  }
  __syncthreads();
  if (threadIdx.x < COSPEC_FIELDS) {
    const int i = threadIdx.x;
    const double x = nan_max(nan_max(sh[0][i], sh[1][i]), nan_max(sh[2][i], sh[3][i]));
    // zero, NaN, infinity: unscaled; so is a field below the smallest normal number, whose 2^-e would overflow
    const int e = (x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308) ? ilogb(x) : 0;
    scl[i] = ldexp(1.0, -e);
    // A field that vanishes everywhere (or is not in the list) comes back out with the factor 0: packed with a partner, its
    // split part (Z - Z*) / (2i) is the round-off of the PARTNER's transform, not zero, and would give it a spectrum of ~1e-32
    // of the partner's and a coherence of order one.  0 times that round-off is an exact zero in every row the field is in.
    scl[COSPEC_FIELDS + i] = x == 0.0 ? 0.0 : ldexp(1.0, e);
  }
}

// A first field that vanishes everywhere beside a second one that does not: the two change places in the packed row, so that the
// second field's transform is the one a call of that field alone runs, F[b + i 0], and its rows do not depend on where in the list
// the zero field stands (F[0 + i b] is i F[b] only up to the last bit).  k_x_cross and BinCross read it off the scales alike.
__device__ __forceinline__ bool cross_swapped(const double* __restrict__ scl) {
  return scl[COSPEC_FIELDS] == 0.0 && scl[COSPEC_FIELDS + 1] != 0.0;
}

// sel.code[i]: the i-th field of the list (FLOW_NONE past its end); scl: k_cospec_scale's; oAB, oC: full-width rows
template <int N, int MODE, bool SLAB = false, bool FLOW = false>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_cross(MArr Mq, MArr Mqw, MArr Mu, MArr Mp, MArr Mphi, MArr Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
          FlowSel sel, const double* __restrict__ scl, MArr oAB, MArr oC) {
  typedef XPlan<N> X;
  typedef typename X::F F;
  constexpr int P = X::P, T = X::T;
  static_assert(!FLOW || flow_nv<N>() == COSPEC_FIELDS, "a pair needs both values in one thread");
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t row = (size_t)blockIdx.x * X::C + c;
  cd* lds = reinterpret_cast<cd*>(nq_smem);
  typename F::TwLds twr;
  twr.base = lds + F::LDS_ELEMS;                       // the twiddles x_row_values / x_flow_values staged: nothing overwrote them
  cd w[P];
  double cv[P];
  const bool swap = cross_swapped(scl);                // workgroup-uniform
  if constexpr (FLOW) {
    double val[COSPEC_FIELDS][P];
    x_flow_values<N, MODE, SLAB>(Mq, Mqw, Mu, Mp, Mphi, Mphiy, tw, kk, sel, val, w);
    const double s0 = scl[0], s1 = scl[1], s2 = scl[2];
#pragma unroll
    for (int t = 0; t < P; ++t) {                      // slots nothing was selected for are zero
      const double a = s0 * val[0][t], b = s1 * val[1][t];
      w[t] = swap ? cmake(b, a) : cmake(a, b);
      cv[t] = s2 * val[2][t];
    }
  } else {
    double q[P], qpsi[P];
    x_row_values<N, MODE, SLAB>(Mq, Mqw, Mphi, tw, kk, q, qpsi, w);
    const double s0 = scl[0], s1 = scl[1], s2 = scl[2];
#pragma unroll
    for (int t = 0; t < P; ++t) {
      const double a2 = w[t].x * w[t].x + w[t].y * w[t].y;
      const double a = s0 * cross_pick(sel.code[0], q[t], qpsi[t], a2), b = s1 * cross_pick(sel.code[1], q[t], qpsi[t], a2);
      w[t] = swap ? cmake(b, a) : cmake(a, b);
      cv[t] = s2 * cross_pick(sel.code[2], q[t], qpsi[t], a2);
    }
  }
  NQ_PHASE_FENCE();
  F::template run<false>(w, j, c, lds, twr);
  NQ_PHASE_FENCE();
  cross_store<N, SLAB>(w, oAB, row, j);
  if (sel.code[2] != FLOW_NONE) {                      // workgroup-uniform
    NQ_PHASE_FENCE();
#pragma unroll
    for (int t = 0; t < P; ++t) w[t] = cmake(cv[t], 0.0);
    F::template run<false>(w, j, c, lds, twr);
    NQ_PHASE_FENCE();
    cross_store<N, SLAB>(w, oC, row, j);
  }
}

// full planes, all columns local (single-rank contexts): z of pitch N, zc of pitch pc; zc null: a call of one or two fields
struct BinCross {
  static constexpr int NQ = COSPEC_ROWS;
  const cd *z, *zc;
  const double* scl;
  int N, pc;
  int single;                 // a call of one field: b is the rounding of a real field's transform, and its rows stay zero
  __device__ void operator()(int l, int k, int kl, double* v) const {
    (void)kl;
    const size_t idx = (size_t)l * N + k, im = (size_t)((N - l) % N) * N + (N - k) % N;
    const cd x = z[idx], xm = z[im];
    const bool swap = cross_swapped(scl);               // the real part of the packed plane is then field 1, the imaginary part field 0
    const double s0 = scl[COSPEC_FIELDS], s1 = scl[COSPEC_FIELDS + 1];
    const double ha = 0.5 * (swap ? s1 : s0), hb = single ? 0.0 : 0.5 * (swap ? s0 : s1);       // the scales taken out again: exact
    const cd a = cmake(ha * (x.x + xm.x), ha * (x.y - xm.y)), b = cmake(hb * (x.y + xm.y), hb * (xm.x - x.x));
    const double aa = a.x * a.x + a.y * a.y, bb = b.x * b.x + b.y * b.y;
    v[0] += swap ? bb : aa;
    v[1] += swap ? aa : bb;
    v[3] += a.x * b.x + a.y * b.y;
    if (zc != nullptr) {
      const cd c = cscale(zc[(size_t)l * pc + k], scl[COSPEC_FIELDS + 2]);
      const double ac = a.x * c.x + a.y * c.y, bc = b.x * c.x + b.y * c.y;
      v[2] += c.x * c.x + c.y * c.y;
      v[4] += swap ? bc : ac;
      v[5] += swap ? ac : bc;
    }
  }
};

// half spectra of the state, f[i] the i-th field of the list (null past its end)
struct BinQC {
  static constexpr int NQ = COSPEC_ROWS;
  const cd* f[COSPEC_FIELDS];
  int N, pitch;
  __device__ void operator()(int l, int k, int kl, double* v) const {
    const size_t idx = (size_t)l * pitch + kl;
    const bool self = k == 0 || k == N / 2;
    const size_t im = (size_t)((N - l) % N) * pitch + kl;
    const double wt = self ? 1.0 : 2.0;
    cd x[COSPEC_FIELDS];
#pragma unroll
    for (int i = 0; i < COSPEC_FIELDS; ++i) {
      x[i] = cmake(0, 0);
      if (f[i] != nullptr) {
        x[i] = f[i][idx];
        if (self) {
          const cd m = f[i][im];
          x[i] = cmake(0.5 * (x[i].x + m.x), 0.5 * (x[i].y - m.y));
        }
      }
    }
#pragma unroll
    for (int i = 0; i < COSPEC_FIELDS; ++i) v[i] += wt * (x[i].x * x[i].x + x[i].y * x[i].y);
    v[3] += wt * (x[0].x * x[1].x + x[0].y * x[1].y);
    v[4] += wt * (x[0].x * x[2].x + x[0].y * x[2].y);
    v[5] += wt * (x[1].x * x[2].x + x[1].y * x[2].y);
  }
};

__global__ void __launch_bounds__(256) k_cospec_add(const double* __restrict__ cur, double* __restrict__ sum, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) sum[i] += cur[i];
}

}  // namespace nq
