// Lagrangian spectra and dispersion of the particle records.
//
// The records of the particles (section 5g) stay on the device: the fused ring [slot][2 + ncol][n] of doubles, or one engine
// plane per record and name on the any-size path (positions as x + i y interleaved).  Both are addressed through a small device
// table with one LgSeries per held record, oldest first: the pointer of the real part, of the imaginary part (or null: a real
// series) and the stride between particles in doubles.  The host builds the table, so no kernel here knows the ring rotation.
//
// Spectrum: k_lg_window composes a chunk of C particles into a (F, C) complex work plane (optionally minus each particle's own
// time mean, times the window, rows T..F-1 zero), the any-length column transform of the any-size engine runs along the record
// axis, k_lg_power sums |X_p|^2 per (frequency, group).  Particles are taken in the order of a group-sorted index list, so a
// group is one run of columns.  Dispersion: k_lg_disp sums the six single-particle moments per (record, group), k_lg_pairs the
// five pair moments per record.  Every sum: fixed per-thread strides, the fixed 64-lane shuffle tree, the four waves added in
// order (the scheme of k_fq_bin): no floating-point atomics, bit-identical tables from call to call.
#pragma once
#include "nq_step.hpp"
#include "nq_particles.hpp"

namespace nq {

struct LgSeries {
  const double* re;
  const double* im;      // null: a real series
  const double* re2;     // null, or a second series added to the first (re + re2) + i (im + im2): the sum of two velocities
  const double* im2;
  long long stride;      // doubles between consecutive particles
};

enum { LG_SINGLE_SUMS = 6, LG_PAIR_SUMS = 5, LG_STRETCH_SUMS = 4 };

// the sum of v over the 256 threads of the workgroup, valid in thread 0; sh: 4 doubles.  Callers that reduce several values in
// turn pass a slice of their own for each.
__device__ inline double lg_block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// the value of particle i in one record of a series
__device__ __forceinline__ double lg_re(const LgSeries& s, size_t i) {
  const double x = s.re[i * s.stride];
  return s.re2 ? x + s.re2[i * s.stride] : x;
}
__device__ __forceinline__ double lg_im(const LgSeries& s, size_t i) {
  if (!s.im) return 0.0;
  const double y = s.im[i * s.stride];
  return s.im2 ? y + s.im2[i * s.stride] : y;
}

// work(n, s - c0) = w_n (x_n(i) - mean(i)), i = order[s], s = c0 .. c0 + C - 1, n = 0 .. T-1; rows T .. F-1 are zero.  One
// thread per entry of the sorted order (consecutive threads, consecutive columns: the writes coalesce); the mean is the sum in
// record order over T.
__global__ void __launch_bounds__(256) k_lg_window(const LgSeries* __restrict__ ser, const int* __restrict__ order, cd* __restrict__ work,
                                                   const double* __restrict__ win, int c0, int C, int T, int F, int demean) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= C) return;
  const size_t i = (size_t)order[c0 + j];
  double mx = 0.0, my = 0.0;
  if (demean) {
    for (int n = 0; n < T; ++n) {
      const LgSeries s = ser[n];
      mx += lg_re(s, i);
      my += lg_im(s, i);
    }
    mx /= (double)T;
    my /= (double)T;
  }
  for (int n = 0; n < T; ++n) {
    const LgSeries s = ser[n];
    const double w = win[n];
    const double x = lg_re(s, i), y = lg_im(s, i);
    work[(size_t)n * C + j] = make_double2(w * (x - mx), w * (y - my));
  }
  for (int n = T; n < F; ++n) work[(size_t)n * C + j] = make_double2(0.0, 0.0);
}

// Fw: the forward transform of the work plane along n, (F, C); X_p = sum_n w_n x_n e^{+2 pi i p n / F} = Fw[(F - p) % F].
// Workgroup (g, p) sums |X_p|^2 over the columns of this chunk that belong to group g (sorted entries offs[g] .. offs[g+1]-1
// cut to c0 .. c0 + C - 1).  tab[p * G + g] = (first chunk ? 0 : tab) + scale * sum: the chunks are added in chunk order.
__global__ void __launch_bounds__(256) k_lg_power(const cd* __restrict__ Fw, const int* __restrict__ offs, int c0, int C, int F, int G, double scale,
                                                  int first, double* __restrict__ tab) {
  const int g = blockIdx.x, p = blockIdx.y;
  const cd* __restrict__ X = Fw + (size_t)((F - p) % F) * C;
  int lo = offs[g] - c0, hi = offs[g + 1] - c0;
  if (lo < 0) lo = 0;
  if (hi > C) hi = C;
  double v = 0.0;
  for (int j = lo + (int)threadIdx.x; j < hi; j += 256) {
    const cd z = X[j];
    v += z.x * z.x + z.y * z.y;
  }
  __shared__ double sh[4];
  v = lg_block_sum(v, sh);
  if (threadIdx.x == 0) {
    const size_t o = (size_t)p * G + g;
    tab[o] = (first ? 0.0 : tab[o]) + scale * v;
  }
}

// Workgroup (g, n): with d = r_n(i) - r_0(i) over the particles i of group g, out[(n * G + g) * 6 + .] = the sums of dx, dy,
// dx^2, dy^2, dx dy and (dx^2 + dy^2)^2.  pos: one LgSeries per record (re: x, im: y).
__global__ void __launch_bounds__(256) k_lg_disp(const LgSeries* __restrict__ pos, const int* __restrict__ order, const int* __restrict__ offs, int G,
                                                 double* __restrict__ out) {
  const int g = blockIdx.x, n = blockIdx.y;
  const LgSeries a = pos[0], b = pos[n];
  double v[LG_SINGLE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = offs[g] + (int)threadIdx.x; s < offs[g + 1]; s += 256) {
    const size_t i = (size_t)order[s];
    const double dx = b.re[i * b.stride] - a.re[i * a.stride], dy = b.im[i * b.stride] - a.im[i * a.stride];
    const double r2 = dx * dx + dy * dy;
    v[0] += dx;
    v[1] += dy;
    v[2] += dx * dx;
    v[3] += dy * dy;
    v[4] += dx * dy;
    v[5] += r2 * r2;
  }
  __shared__ double sh[LG_SINGLE_SUMS][4];
#pragma unroll
  for (int k = 0; k < LG_SINGLE_SUMS; ++k) {
    const double t = lg_block_sum(v[k], sh[k]);
    if (threadIdx.x == 0) out[((size_t)n * G + g) * LG_SINGLE_SUMS + k] = t;
  }
}

// Stretching statistics of stretch mode.  Workgroup (g, n): over the particles i of group g in record n,
// out[(n * G + g) * 4 + .] = the sums of ln sigma_1, (ln sigma_1)^2, det F and (det F)^2, from the recorded f-columns.  ser: one
// LgSeries per record with re = f11, im = f12, re2 = f21, im2 = f22 (four series of one stride), the summation of k_lg_disp.
__global__ void __launch_bounds__(256) k_lg_stretch(const LgSeries* __restrict__ ser, const int* __restrict__ order, const int* __restrict__ offs,
                                                    int G, double* __restrict__ out) {
  const int g = blockIdx.x, n = blockIdx.y;
  const LgSeries b = ser[n];
  double v[LG_STRETCH_SUMS] = {0.0, 0.0, 0.0, 0.0};
  for (int s = offs[g] + (int)threadIdx.x; s < offs[g + 1]; s += 256) {
    const size_t at = (size_t)order[s] * b.stride;
    const double f11 = b.re[at], f12 = b.im[at], f21 = b.re2[at], f22 = b.im2[at];
    const double ls = pt_ln_sigma(f11, f12, f21, f22), dt = pt_det(f11, f12, f21, f22);
    v[0] += ls;
    v[1] += ls * ls;
    v[2] += dt;
    v[3] += dt * dt;
  }
  __shared__ double sh[LG_STRETCH_SUMS][4];
#pragma unroll
  for (int k = 0; k < LG_STRETCH_SUMS; ++k) {
    const double t = lg_block_sum(v[k], sh[k]);
    if (threadIdx.x == 0) out[((size_t)n * G + g) * LG_STRETCH_SUMS + k] = t;
  }
}

// Workgroup (n): with s = r_n(i) - r_n(j) over the pairs (i, j), out[n * 5 + .] = the sums of sx^2, sy^2, sx sy, |s|^2, |s|^4
__global__ void __launch_bounds__(256) k_lg_pairs(const LgSeries* __restrict__ pos, const int* __restrict__ pi, const int* __restrict__ pj, int npairs,
                                                  double* __restrict__ out) {
  const int n = blockIdx.x;
  const LgSeries b = pos[n];
  double v[LG_PAIR_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = (int)threadIdx.x; q < npairs; q += 256) {
    const size_t i = (size_t)pi[q], j = (size_t)pj[q];
    const double sx = b.re[i * b.stride] - b.re[j * b.stride], sy = b.im[i * b.stride] - b.im[j * b.stride];
    const double r2 = sx * sx + sy * sy;
    v[0] += sx * sx;
    v[1] += sy * sy;
    v[2] += sx * sy;
    v[3] += r2;
    v[4] += r2 * r2;
  }
  __shared__ double sh[LG_PAIR_SUMS][4];
#pragma unroll
  for (int k = 0; k < LG_PAIR_SUMS; ++k) {
    const double t = lg_block_sum(v[k], sh[k]);
    if (threadIdx.x == 0) out[(size_t)n * LG_PAIR_SUMS + k] = t;
  }
}

}  // namespace nq
