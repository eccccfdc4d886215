// Stochastic forcing of q and phi, drawn on the device inside the step.
//
// After a step the library adds the white-in-time increment  sqrt(dt) A(l, k) xi(l, k; s)  to the spectral state, where A is a
// real amplitude plane the caller gave and xi a unit-variance complex Gaussian drawn from a COUNTER-BASED generator: the value at
// (l, k) of step s is a pure function of (l, k, s, stream, seed) -- Philox4x32-10 with counter (l, k, s, stream), key
// (seed & 0xffffffff, seed >> 32) -- so it does not depend on launch geometry and numpy restates it (niwqg_amd/forcing.py: noise).
// From the four output words x0..x3:   n = (x0 >> 5) 2^26 + (x1 >> 6),  u1 = 1 - n 2^-53 in (0, 1],  u2 = (x2 + 0.5) 2^-32,
//                                      xi = sqrt(-ln u1) (cos 2 pi u2 + i sin 2 pi u2),   E |xi|^2 = 1.
// Stream 0 forces q on the half spectrum (k = 0..N/2) under the Hermitian rule of fc_xi_q, stream 1 forces phi on the full plane
// with independent values.  The kernels run over the bounding box of A > 0 in (|l|, |k|) only (FcBox): a ring at k_f touches a
// small corner of the plane.  Each workgroup also forms the partial sum of the work the increment does on the state BEFORE it
// (DESIGN.md section 5i); k_force_accum adds the partials in a fixed order: deterministic, no floating-point atomics.
#pragma once
#include <cstdint>
#include "nq_step.hpp"

namespace nq {

struct Philox4 { uint32_t x[4]; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.x[0] = c0; o.x[1] = c1; o.x[2] = c2; o.x[3] = c3;
  return o;
}

// the unit-variance complex Gaussian of counter (l, k, s, stream)
__host__ __device__ inline cd fc_xi(uint32_t l, uint32_t k, uint32_t s, uint32_t stream, unsigned long long seed) {
  const Philox4 p = philox4x32_10(l, k, s, stream, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
  const double n = (double)(p.x[0] >> 5) * 67108864.0 + (double)(p.x[1] >> 6);
  const double u1 = 1.0 - n * (1.0 / 9007199254740992.0);
  const double u2 = ((double)p.x[2] + 0.5) * (1.0 / 4294967296.0);
  const double r = sqrt(-log(u1)), th = 6.283185307179586 * u2;
  return make_double2(r * cos(th), r * sin(th));
}

// q is real, so its increment is Hermitian.  On the half spectrum (l = 0..N-1, k = 0..N/2): nothing on row N/2, column N/2 and at
// (0, 0) -- the passenger row and the lines without a mirror partner stay alone; on column 0 rows 1..N/2-1 draw and row N - l
// takes the conjugate of the value drawn at (l, 0); interior columns draw freely.
__host__ __device__ inline cd fc_xi_q(int N, int l, int k, uint32_t s, unsigned long long seed) {
  if (l == N / 2 || k == N / 2 || (l == 0 && k == 0)) return make_double2(0.0, 0.0);
  if (k == 0 && l > N / 2) {
    const cd z = fc_xi((uint32_t)(N - l), 0u, s, 0u, seed);
    return make_double2(z.x, -z.y);
  }
  return fc_xi((uint32_t)l, (uint32_t)k, s, 0u, seed);
}
// the same on the full plane (the any-size Kernel family carries the reference's (N, N) qh): columns k > N/2 mirror (-l, -k)
__host__ __device__ inline cd fc_xi_q_full(int N, int l, int k, uint32_t s, unsigned long long seed) {
  if (k <= N / 2) return fc_xi_q(N, l, k, s, seed);
  const cd z = fc_xi_q(N, (N - l) % N, N - k, s, seed);
  return make_double2(z.x, -z.y);
}

// Bounding box of A > 0: |l| <= L (rows 0..L and N-L..N-1: `nrows` of them, all N when 2 L + 1 >= N) and, on the full plane, the
// same in k with K; on the half plane k = 0..K.  Box index -> array index:
struct FcBox {
  int N, L, K, nrows, ncols;
};
__host__ __device__ inline int fc_unfold(int i, int n_box, int half_extent, int N) {      // i in [0, n_box)
  return (n_box >= N || i <= half_extent) ? i : N - (n_box - i);
}

__device__ __forceinline__ double fc_amp(const double* a, size_t i) { return a[i]; }
__device__ __forceinline__ double fc_amp(const cd* a, size_t i) { return a[i].x; }      // (engine planes are complex)

// sum of v over the 256 threads of a (64, 4) workgroup into part[block], waves in a fixed order
template <int NV>
__device__ __forceinline__ void fc_block_store(double (&v)[NV], double* __restrict__ part) {
  __shared__ double sh[4][NV];
  const int lane = threadIdx.x, wave = threadIdx.y;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double x = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) sh[wave][i] = x;
  }
  __syncthreads();
  if (threadIdx.y == 0 && threadIdx.x < NV) {
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[b * NV + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
  }
}

// (q, q2, y and wrk carry no __restrict__: wrk may be the plane itself.)
// Half-spectrum plane(s) of pitch `pitch` += sdt A xi_q; q2: the second copy of a dual-q context (the increment is Hermitian:
// both copies take the same one) or null.  amp: (N, N/2+1) contiguous.  With `inc` non-null nothing is read or added: the
// increment alone is written there ((N, N/2+1) contiguous; the caller zeroed it).  part (null: none): per workgroup
//   [0] sum w Re(conj(W) D)   [1] sum w |D|^2 g,   w = 1 on columns 0 and N/2, else 2;  W = wrk (pitch wpitch);
//   g = 1 / wv2 from kk, ll when given, else 1.
template <typename AmpT>
__global__ void __launch_bounds__(256) k_force_half(cd* q, cd* q2, int pitch, const AmpT* __restrict__ amp,
                                                    FcBox b, double sdt, uint32_t s, unsigned long long seed, const cd* wrk,
                                                    int wpitch, const double* __restrict__ kk, const double* __restrict__ ll,
                                                    double* __restrict__ part, cd* __restrict__ inc) {
  const int k = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
  double v[2] = {0.0, 0.0};
  if (k < b.ncols && r < b.nrows) {
    const int N = b.N, l = fc_unfold(r, b.nrows, b.L, N), Wh = N / 2 + 1;
    const double A = fc_amp(amp, (size_t)l * Wh + k);
    if (A > 0.0) {
      const cd xi = fc_xi_q(N, l, k, s, seed);
      const cd d = make_double2(sdt * A * xi.x, sdt * A * xi.y);
      if (inc) inc[(size_t)l * Wh + k] = d;
      else if (d.x != 0.0 || d.y != 0.0) {
        const size_t idx = (size_t)l * pitch + k;
        if (part) {
          const cd w = wrk[(size_t)l * wpitch + k];
          const double wt = (k == 0 || k == N / 2) ? 1.0 : 2.0;
          const double g = kk ? 1.0 / (kk[k] * kk[k] + ll[l] * ll[l]) : 1.0;
          v[0] = wt * (w.x * d.x + w.y * d.y);
          v[1] = wt * (d.x * d.x + d.y * d.y) * g;
        }
        cd z = q[idx];
        z.x += d.x; z.y += d.y;
        q[idx] = z;
        if (q2) {
          cd z2 = q2[idx];
          z2.x += d.x; z2.y += d.y;
          q2[idx] = z2;
        }
      }
    }
  }
  if (part) fc_block_store(v, part);
}

// Full (N, N) plane of pitch N += sdt A xi.  HERM false: independent values of counter (l, k, s, stream) (phi); true: the Hermitian
// extension of the q rule (the reference's full-plane qh on the any-size path).  part, wrk, kk / ll, inc as above with w = 1.
template <typename AmpT, bool HERM>
__global__ void __launch_bounds__(256) k_force_full(cd* y, const AmpT* __restrict__ amp, FcBox b, double sdt, uint32_t s,
                                                    uint32_t stream, unsigned long long seed, const cd* wrk,
                                                    const double* __restrict__ kk, const double* __restrict__ ll,
                                                    double* __restrict__ part, cd* __restrict__ inc) {
  const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
  double v[2] = {0.0, 0.0};
  if (c < b.ncols && r < b.nrows) {
    const int N = b.N, l = fc_unfold(r, b.nrows, b.L, N), k = fc_unfold(c, b.ncols, b.K, N);
    const size_t idx = (size_t)l * N + k;
    const double A = fc_amp(amp, idx);
    if (A > 0.0) {
      const cd xi = HERM ? fc_xi_q_full(N, l, k, s, seed) : fc_xi((uint32_t)l, (uint32_t)k, s, stream, seed);
      const cd d = make_double2(sdt * A * xi.x, sdt * A * xi.y);
      if (inc) inc[idx] = d;
      else if (d.x != 0.0 || d.y != 0.0) {
        if (part) {
          const cd w = wrk[idx];
          const double g = kk ? 1.0 / (kk[k] * kk[k] + ll[l] * ll[l]) : 1.0;
          v[0] = w.x * d.x + w.y * d.y;
          v[1] = (d.x * d.x + d.y * d.y) * g;
        }
        cd z = y[idx];
        z.x += d.x; z.y += d.y;
        y[idx] = z;
      }
    }
  }
  if (part) fc_block_store(v, part);
}

// work[0] += (-S0 + S1 / 2) / M^2 of the q partials, work[1] += (S0 + S1 / 2) / M^2 of the phi partials (n = 0: none); one
// workgroup of 256 threads, each summing its partials in order, then a fixed tree: bit-reproducible.  out2 (null: none)
// receives the raw sums S0 / M^2, S1 / M^2 of the first set instead of accumulating (nq_any_forcing).
__global__ void __launch_bounds__(256) k_force_accum(const double* __restrict__ pq, int nq, const double* __restrict__ pw, int nw, double invM2,
                                                     double* __restrict__ work, double* __restrict__ out2) {
  __shared__ double sh[4][256];
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nq; i += 256) { a[0] += pq[2 * i]; a[1] += pq[2 * i + 1]; }
  for (int i = threadIdx.x; i < nw; i += 256) { a[2] += pw[2 * i]; a[3] += pw[2 * i + 1]; }
#pragma unroll
  for (int j = 0; j < 4; ++j) sh[j][threadIdx.x] = a[j];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (out2) {
      out2[0] = sh[0][0] * invM2;
      out2[1] = sh[1][0] * invM2;
    } else {
      if (nq > 0) work[0] += (-sh[0][0] + 0.5 * sh[1][0]) * invM2;
      if (nw > 0) work[1] += (sh[2][0] + 0.5 * sh[3][0]) * invM2;
    }
  }
}

}  // namespace nq
