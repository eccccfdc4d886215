// Time-mean spectra, transfer and flux, accumulated inside the step (include/niwqg_amd.h: nq_tspec_attach).
//
// Running sums of the raw shell tables only: the 32 x nb rows of nq_diagnostics_binned and the NQ_TRANSFER_ROWS x nb rows of
// nq_transfer_binned as a sample leaves them on the device, and the running sum over the shells of every transfer row (the flux
// before its sign and factor).  THE accumulation rule (niwqg_amd/timespectra.py: accumulate restates it): for every raw element x
// S1 <- S1 + x, S2 <- S2 + x x; for every transfer row c[b] = sum_{b' <= b} x[b'] added in shell order, one after the other, as
// np.cumsum does, then P1 <- P1 + c, P2 <- P2 + c c.  fp64, sample order, one thread per element, no atomics: a first-moment
// table is the sequential fp64 sum exactly; S2 + x x may contract into one fma (one rounding less per sample than numpy's).
//
// Included by nq_lib.hip below DevOwned and RecordRing, which the state is made of.
#pragma once

namespace nq {

constexpr int TSPEC_SPEC_ROWS = 32;            // rows of nq_diagnostics_binned
constexpr int TSPEC_TR_ROWS = 6;               // NQ_TRANSFER_ROWS (checked where this file is included)
constexpr int TSPEC_TABLES = 6;                // S1, S2 of the spectra, S1, S2 of the transfer, P1, P2
constexpr int TSPEC_MAX_NB = 5794;             // shells of the largest fused grid, 8192^2: the LDS row of the running sum
constexpr int TSPEC_THREADS = 256;

struct TspecArgs {
  const double* spec;                          // this sample's 32 x nb shell sums; null: that body is not attached
  const double* tr;                            // this sample's TSPEC_TR_ROWS x nb shell sums; null: idem
  double *s1, *s2;                             // 32 x nb
  double *t1, *t2, *p1, *p2;                   // TSPEC_TR_ROWS x nb each
  int nb;
};

// THE adds of the kernel
__device__ __forceinline__ double tspec_add(double s, double x) { return s + x; }
__device__ __forceinline__ double tspec_add2(double s, double x) { return s + x * x; }

// Workgroups 0 .. TSPEC_TR_ROWS - 1 (launched only with a transfer table): workgroup r loads row r into LDS, lane 0 turns it into
// its running sum in shell order -- that order is the contract, so one lane walks the row, eight shells per trip to keep the LDS
// reads of a trip in flight together -- and all lanes add c and c c into P1 and P2.  The workgroups after them: one thread per
// raw element of the two tables.
__global__ void __launch_bounds__(TSPEC_THREADS) k_tspec_accumulate(TspecArgs a) {
  __shared__ double row[TSPEC_MAX_NB];
  const int nb = a.nb, tid = threadIdx.x;
  int blk = blockIdx.x;
  if (a.tr) {
    if (blk < TSPEC_TR_ROWS) {
      const size_t at = (size_t)blk * nb;
      for (int b = tid; b < nb; b += TSPEC_THREADS) row[b] = a.tr[at + b];
      __syncthreads();
      if (tid == 0) {
        double c = 0.0;
        int b = 0;
        for (; b + 8 <= nb; b += 8) {
          double x[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) x[i] = row[b + i];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            c = tspec_add(c, x[i]);
            row[b + i] = c;
          }
        }
        for (; b < nb; ++b) {
          c = tspec_add(c, row[b]);
          row[b] = c;
        }
      }
      __syncthreads();
      for (int b = tid; b < nb; b += TSPEC_THREADS) {
        const double c = row[b];
        a.p1[at + b] = tspec_add(a.p1[at + b], c);
        a.p2[at + b] = tspec_add2(a.p2[at + b], c);
      }
      return;
    }
    blk -= TSPEC_TR_ROWS;
  }
  const size_t ns = a.spec ? (size_t)TSPEC_SPEC_ROWS * nb : 0, nt = a.tr ? (size_t)TSPEC_TR_ROWS * nb : 0;
  const size_t e = (size_t)blk * TSPEC_THREADS + tid;
  if (e < ns) {
    const double x = a.spec[e];
    a.s1[e] = tspec_add(a.s1[e], x);
    a.s2[e] = tspec_add2(a.s2[e], x);
  } else if (e < ns + nt) {
    const size_t i = e - ns;
    const double x = a.tr[i];
    a.t1[i] = tspec_add(a.t1[i], x);
    a.t2[i] = tspec_add2(a.t2[i], x);
  }
}
// workgroups of one launch
inline int tspec_grid(bool spec, bool tr, int nb) {
  const size_t n = (spec ? (size_t)TSPEC_SPEC_ROWS * nb : 0) + (tr ? (size_t)TSPEC_TR_ROWS * nb : 0);
  return (tr ? TSPEC_TR_ROWS : 0) + (int)((n + TSPEC_THREADS - 1) / TSPEC_THREADS);
}

}  // namespace nq

struct NqTspec : DevOwned {                // time-mean spectra, transfer and flux (section 5n)
  int mask = 0;                            // NQ_TSPEC_SPECTRA | NQ_TSPEC_TRANSFER: the bodies a sample runs
  int nb = 0;
  double* tab = nullptr;                   // one allocation: S1, S2 (32 x nb each), then T1, T2, P1, P2 (NQ_TRANSFER_ROWS x nb each)
  nq::TspecArgs args = {};
  RecordRing rg;                           // cap = 1: only tick() and the two counters are used (count = samples in the sums)
  size_t doubles() const { return (size_t)(2 * nq::TSPEC_SPEC_ROWS + 4 * nq::TSPEC_TR_ROWS) * nb; }
};
