// Low-mode time series recorded in the step and their frequency - wavenumber spectra.
//
// A recorder keeps the block |i|, |j| <= K of the spectral state in a device ring, [field][record][row][col] complex128:
// rows j = 0..K, -K..-1 (fftfreq order, R = 2K + 1 of them); columns the same for a full plane (phi-hat), i = 0..K for a half
// spectrum (q-hat, psi-hat).  k_fq_record copies one record of every attached field in ONE launch.  The spectrum pass is three
// steps on the device: k_fq_window un-rotates the ring into a (T, modes) work plane (optionally minus each mode's time mean,
// times the window), the any-length column transform of the any-size engine runs along the record axis, and k_fq_bin forms
// |X_p|^2 with the weights of the field and sums it per (frequency, shell) in a fixed order: no floating-point atomics,
// bit-identical tables from call to call.
//
// Included by nq_lib.hip AFTER its shell rule (nq_shell_of, shell_run): k_fq_bin walks the shells exactly as k_bin_shells does.
#pragma once
#include "nq_step.hpp"

namespace nq {

enum { FQ_PHI = 0, FQ_Q = 1, FQ_PSI = 2, FQ_NFIELDS = 3 };

// block index -> plane index along one axis: 0..K stay, the n_block - K negative ones map to the end of the axis
__host__ __device__ inline int fq_unfold(int i, int K, int n_block, int N) { return i <= K ? i : N - (n_block - i); }

struct FqRecord {
  const cd* src[FQ_NFIELDS];   // the plane that holds the new state
  cd* dst[FQ_NFIELDS];         // the ring slot of this record: (2K + 1, ncols) contiguous
  int pitch[FQ_NFIELDS];       // elements per plane row (N for phi-hat, the half-spectrum pitch for q-hat and psi-hat)
  int ncols[FQ_NFIELDS];       // 2K + 1 (full plane) or K + 1 (half spectrum)
  int proj[FQ_NFIELDS];        // column 0 takes its Hermitian part in l, (z(l) + conj z(-l)) / 2: what Kernel.ph holds there
};

// grid (ceil(max ncols / 64), ceil(R / 4), fields), block (64, 4): a wave walks 64 consecutive columns of one block row, so
// the plane reads and the ring writes coalesce (the negative-k columns are one more contiguous run at the end of the plane row)
__global__ void __launch_bounds__(256) k_fq_record(FqRecord a, int N, int K) {
  const int f = blockIdx.z, c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
  const int R = 2 * K + 1, nc = a.ncols[f];
  if (r >= R || c >= nc) return;
  const int l = fq_unfold(r, K, R, N), k = fq_unfold(c, K, nc, N);
  const cd* __restrict__ s = a.src[f];
  cd z = s[(size_t)l * a.pitch[f] + k];
  if (a.proj[f] && k == 0) {
    const cd w = s[(size_t)((N - l) % N) * a.pitch[f]];
    z = make_double2(0.5 * (z.x + w.x), 0.5 * (z.y - w.y));
  }
  a.dst[f][(size_t)r * nc + c] = z;
}

// work(n, i) = w_n (x_n(i) - mean_i), n = 0..T-1 oldest first: record n sits in ring slot (first + n) % length.  One thread per
// mode i (consecutive threads, consecutive modes: coalesced both ways); the mean is the sum in record order over T.
__global__ void __launch_bounds__(256) k_fq_window(const cd* __restrict__ ring, cd* __restrict__ work, const double* __restrict__ win,
                                                   int nm, int length, int first, int T, int demean) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)nm) return;
  double mx = 0.0, my = 0.0;
  if (demean) {
    for (int n = 0; n < T; ++n) {
      const cd z = ring[(size_t)((first + n) % length) * nm + i];
      mx += z.x;
      my += z.y;
    }
    mx /= (double)T;
    my /= (double)T;
  }
  for (int n = 0; n < T; ++n) {
    const cd z = ring[(size_t)((first + n) % length) * nm + i];
    const double w = win[n];
    work[(size_t)n * nm + i] = make_double2(w * (z.x - mx), w * (z.y - my));
  }
}

// F: the forward transform of the work plane along n, (T, modes); X_p = sum_n w_n x_n e^{+2 pi i p n / T} = F[(T - p) % T] and
// X_{-p} = F[p].  Workgroup (b, p) owns shell b of frequency bin p and walks the block rows |j| <= min(b, K), one row per thread;
// in a row the i of the shell are one run (shell_run), cut at K.  Per wavenumber (i, j):
//   full plane (phi):      |X_p(j, i)|^2, and |X_p(j, -i)|^2 for i > 0
//   half spectrum (q, psi): |X_p(j, i)|^2, and |X_{-p}(j, i)|^2 for i > 0 -- the mirrored half plane of a real field,
//                           X_p(-j, -i) = conj X_{-p}(j, i) for a real window;  psi: times kappa^2 = dk2 (i^2 + j^2)
// out[p * nb + b] = scale * sum.  Fixed order per thread, fixed shuffle tree, four waves added in order (as k_bin_shells).
__global__ void __launch_bounds__(256) k_fq_bin(const cd* __restrict__ F, int T, int K, int ncols, int full, int kappa, double dk2,
                                                double scale, int nb, double* __restrict__ out) {
  const int b = blockIdx.x, p = blockIdx.y;
  const int R = 2 * K + 1;
  const size_t nm = (size_t)R * ncols;
  const cd* __restrict__ Xp = F + (size_t)((T - p) % T) * nm;
  const cd* __restrict__ Xm = F + (size_t)p * nm;
  const int jmax = b < K ? b : K;
  double v = 0.0;
  for (int j = -jmax + (int)threadIdx.x; j <= jmax; j += 256) {
    int lo, hi;
    shell_run(b, j, &lo, &hi);
    if (hi > K) hi = K;
    const size_t row = (size_t)(j >= 0 ? j : R + j) * ncols;
    for (int i = lo; i <= hi; ++i) {
      const cd z = Xp[row + i];
      double a = z.x * z.x + z.y * z.y;
      if (i > 0) {
        const cd y = full ? Xp[row + (ncols - i)] : Xm[row + i];
        a += y.x * y.x + y.y * y.y;
      }
      if (kappa) a *= dk2 * (double)(i * i + j * j);
      v += a;
    }
  }
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[(size_t)p * nb + b] = scale * (((sh[0] + sh[1]) + sh[2]) + sh[3]);
}

}  // namespace nq
