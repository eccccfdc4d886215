// Vortex census: the connected components of a thresholded field, labelled and summed on the device (DESIGN.md section 5y;
// include/niwqg_amd.h: nq_vortex_range, nq_vortex_census, nq_vortex_read, nq_vortex_labels, nq_any_components;
// niwqg_amd/vortices.py: reference restates the definitions in numpy).
//
// Input: one to three physical planes (pointer, stride in doubles per element, rows, cols), any rows, cols >= 4; nothing here
// is templated on a fused size or assumes a multiple of 64.  One plane is the criterion a; point (y, x) is in the SET when
// a < t, a > t or |a| > t for the finite threshold t (NaN fails every comparison; +-inf is in where its comparison holds).  The
// components are those of the set under 4- or 8-connectivity on the doubly periodic grid; the LABEL of a component is the
// smallest linear index y cols + x of its points, -1 outside the set.  That label does not depend on the order of execution.
//
// Phases, each a launch of its own, ordered by the stream; no kernel waits for another workgroup (no flags, no spinning, no grid
// barrier, no cooperative launch), no floating-point atomics:
//   k_vx_range     per field: min, max, max |a|, sum a, sum a^2 over the finite values and the count of the others; one partial
//                  slot per workgroup
//   k_vx_scale     adds the slots in a fixed order (64 contiguous runs per field, then the runs in index order: k_sf_total's
//                  scheme) and writes the fixed-point scale s_f = 61 - ceil(log2(rows cols)) - e, max |a_f| = m 2^e, m in [0.5, 1)
//   k_vx_rows      one workgroup per row: the mask as 64-bit ballot words in LDS, one thread carries the start of the run that
//                  enters each word from the left, then every set point takes y cols + (start of its run) as its label; a run
//                  that reaches x = cols - 1 takes the label y cols + 0 of the run at x = 0 when both are set
//   k_vx_merge     one workgroup per row: a set point whose neighbour(s) in row (y - 1) mod rows are set unites the two labels
//                  when it is the first point of its run to touch that upper run
//   k_vx_flatten   L[p] = find(L[p]); roots and set points counted per row
//   k_vx_prefix    one workgroup: exclusive prefix of the roots over the rows (integers), the totals into info
//   k_vx_rank      one workgroup per row: every root gets its rank (row offset + roots to its left) in the rank plane; the first
//                  `cap` of them start their table row: label, zeros, the identities of the two extrema
//   k_vx_sums      one workgroup per row: per point the periodic offsets from the label's point, the fixed-point values and the
//                  criterion's order-preserving key; a segmented scan within the wave reduces them over each run of equal labels,
//                  the last lane of a run WITHIN THE WAVE issues one 64-bit integer atomicAdd per column (atomicMin / atomicMax for
//                  the keys): a run is flushed once per 64-column piece it covers, never once per point
//   k_vx_finish    the two keys of each table row back to the bit patterns of the doubles
//
// Why every loop ends.  L[p] <= p holds after k_vx_rows and every later write stores a smaller value (atomicMin, or the root
// found), never below 0.  vx_find follows L[i] < i until L[i] = i: at most i steps.  vx_union either returns or continues with
// (old, b), old < a the value its atomicMin returned: the pair's larger index strictly decreases, bounded below by 0.  A read
// that is stale (another CU's store not yet visible) returns an EARLIER value of L[i], which is also an ancestor of i with
// L[i] <= i, so both arguments hold for stale reads; the union trusts only what atomicMin returns: it stops when that value
// says the node was still a root (the link is made) or when both finds meet (links are never removed).  Reads of the label
// plane inside k_vx_merge and k_vx_flatten are device-scope relaxed atomic loads, which are served past the CU's L1.
//
// Indices are int32: rows cols <= 16384^2 = 2^28.  The offset moments are int64: |dx| <= 2^13, area <= 2^28, sum dx^2 < 2^54.
#pragma once
#include "nq_sf2.hpp"

namespace nq {

constexpr int VX_MAX_FIELDS = 3, VX_THREADS = 256, VX_WAVES = VX_THREADS / 64, VX_RANGE_GRID = 1024, VX_RANGE_COLS = 6;
constexpr int VX_BASE_COLS = 9, VX_MAX_WORDS = 16384 / 64, VX_MAX_DIM = 16384, VX_INFO = 7;
enum { VX_BELOW = 0, VX_ABOVE = 1, VX_ABS_ABOVE = 2 };

struct VxPlanes {
  const double* p[VX_MAX_FIELDS];
  int stride[VX_MAX_FIELDS];          // doubles per element (1: a real plane, 2: the real part of a complex one)
  int nf, crit;                       // planes of the call, index of the criterion
  int rows, cols;
};
// what the range pass leaves on the device
struct VxRange {
  double v[VX_MAX_FIELDS][4];         // min, max, sum, sum of squares over the finite values (+inf, -inf, 0, 0 without any)
  long long nonfinite;                // over all fields of the call
  int scale[VX_MAX_FIELDS];
};

__device__ __forceinline__ bool vx_in_set(double a, int mode, double t) {
  return mode == VX_BELOW ? a < t : (mode == VX_ABOVE ? a > t : fabs(a) > t);
}
__device__ __forceinline__ int vx_load(const int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_store(int* L, int i, int v) { __hip_atomic_store(L + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int vx_find(const int* L, int i) {
  for (int p = vx_load(L, i); p != i; p = vx_load(L, i)) i = p;
  return i;
}
__device__ __forceinline__ void vx_union(int* L, int a, int b) {
  for (;;) {
    a = vx_find(L, a);
    b = vx_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;             // a was a root until this very operation
    a = old;                          // a had been linked to old (< a) already: unite old with b
  }
}
// order-preserving key of a double (-0 < +0): smaller double <=> smaller unsigned key
__host__ __device__ inline unsigned long long vx_key(double a) {
  unsigned long long b;
  memcpy(&b, &a, sizeof(b));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline unsigned long long vx_unkey(unsigned long long k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }
// the fixed-point term of one value: rint(a 2^s), half to even; 0 for a non-finite value
__device__ __forceinline__ long long vx_fixed(double a, int s) { return isfinite(a) ? (long long)rint(ldexp(a, s)) : 0ll; }

// ---- range ------------------------------------------------------------------------------------------------------------------------
// part[block][field][VX_RANGE_COLS] = min, max, max |a|, sum, sum of squares, count of non-finite values (as a double: exact)
__global__ void __launch_bounds__(VX_THREADS) k_vx_range(VxPlanes pl, double* __restrict__ part) {
  __shared__ double red[VX_WAVES][VX_MAX_FIELDS][VX_RANGE_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int f = 0; f < pl.nf; ++f) {
    double lo = INFINITY, hi = -INFINITY, ma = 0.0, s1 = 0.0, s2 = 0.0, bad = 0.0;
    const double* __restrict__ p = pl.p[f];
    const int st = pl.stride[f];
    for (int y = blockIdx.x; y < pl.rows; y += gridDim.x)
      for (int x = threadIdx.x; x < pl.cols; x += VX_THREADS) {
        const double a = p[((size_t)y * pl.cols + x) * st];
        if (isfinite(a)) {
          lo = fmin(lo, a);
          hi = fmax(hi, a);
          ma = fmax(ma, fabs(a));
          s1 += a;
          s2 += a * a;
        } else {
          bad += 1.0;
        }
      }
    for (int off = 32; off > 0; off >>= 1) {
      lo = fmin(lo, __shfl_down(lo, off, 64));
      hi = fmax(hi, __shfl_down(hi, off, 64));
      ma = fmax(ma, __shfl_down(ma, off, 64));
      s1 += __shfl_down(s1, off, 64);
      s2 += __shfl_down(s2, off, 64);
      bad += __shfl_down(bad, off, 64);
    }
    if (lane == 0) {
      double* r = red[wave][f];
      r[0] = lo, r[1] = hi, r[2] = ma, r[3] = s1, r[4] = s2, r[5] = bad;
    }
  }
  __syncthreads();
  if (threadIdx.x < pl.nf * VX_RANGE_COLS) {
    const int f = threadIdx.x / VX_RANGE_COLS, c = threadIdx.x % VX_RANGE_COLS;
    double v = red[0][f][c];
    for (int w = 1; w < VX_WAVES; ++w) v = c == 0 ? fmin(v, red[w][f][c]) : (c <= 2 ? fmax(v, red[w][f][c]) : v + red[w][f][c]);
    part[((size_t)blockIdx.x * VX_MAX_FIELDS + f) * VX_RANGE_COLS + c] = v;
  }
}
// One workgroup of 64 x VX_RANGE_COLS threads, field after field: thread (g, c) combines the slots of run g in index order, thread
// (0, c) the runs in index order; then one thread writes the field's scale and, after the last field, the count of non-finite
// values.  lg = ceil(log2(rows cols)).
__global__ void __launch_bounds__(64 * VX_RANGE_COLS) k_vx_scale(const double* __restrict__ part, int nblk, int nf, int lg, VxRange* __restrict__ out,
                                                                  long long* __restrict__ info) {
  __shared__ double run[64][VX_RANGE_COLS];
  __shared__ double tot[VX_RANGE_COLS];
  const int c = threadIdx.x % VX_RANGE_COLS, g = threadIdx.x / VX_RANGE_COLS;
  const int per = (nblk + 63) / 64, b0 = g * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  long long bad = 0;
#pragma unroll 1
  for (int f = 0; f < VX_MAX_FIELDS; ++f) {
    if (f >= nf) {
      if (threadIdx.x == 0) info[4 + f] = 0;
      continue;
    }
    double v = c == 0 ? INFINITY : (c == 1 ? -INFINITY : 0.0);
    for (int b = b0; b < b1; ++b) {
      const double x = part[((size_t)b * VX_MAX_FIELDS + f) * VX_RANGE_COLS + c];
      v = c == 0 ? fmin(v, x) : (c <= 2 ? fmax(v, x) : v + x);
    }
    __syncthreads();                                          // the last field's reads of run and tot
    run[g][c] = v;
    __syncthreads();
    if (g == 0) {
      double t = run[0][c];
      for (int k = 1; k < 64; ++k) t = c == 0 ? fmin(t, run[k][c]) : (c <= 2 ? fmax(t, run[k][c]) : t + run[k][c]);
      tot[c] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      out->v[f][0] = tot[0];
      out->v[f][1] = tot[1];
      out->v[f][2] = tot[3];
      out->v[f][3] = tot[4];
      int e = 0, s = 0;
      if (tot[2] > 0.0) {
        (void)frexp(tot[2], &e);
        s = 61 - lg - e;
      }
      out->scale[f] = s;
      info[4 + f] = s;
      bad += (long long)tot[5];
    }
  }
  if (threadIdx.x == 0) {
    out->nonfinite = bad;
    info[3] = bad;
  }
}

// ---- rows -------------------------------------------------------------------------------------------------------------------------
// start of the run that holds bit `lane` of word b (bit set), when the run begins inside the word; -1: it reaches the word's bit 0
__device__ __forceinline__ int vx_run_start(unsigned long long b, int lane) {
  const unsigned long long zeros = ~b & ((1ull << lane) - 1ull);
  return zeros ? 64 - __clzll(zeros) : -1;
}
__global__ void __launch_bounds__(VX_THREADS) k_vx_rows(VxPlanes pl, int mode, double thr, int* __restrict__ L) {
  __shared__ unsigned long long bits[VX_MAX_WORDS];
  __shared__ int carry[VX_MAX_WORDS];        // start (x) of the run that enters the word from its left neighbour, -1: none
  __shared__ int wrap;                       // start of the run that reaches x = cols - 1 and is joined with a run at x = 0, -1: none
  const int y = blockIdx.x, cols = pl.cols, nw = (cols + 63) >> 6;
  const double* __restrict__ p = pl.p[pl.crit];
  const int st = pl.stride[pl.crit];
  const size_t row = (size_t)y * cols;
  for (int x0 = 0; x0 < nw * 64; x0 += VX_THREADS) {         // whole waves: the ballot of a word needs all of its lanes
    const int x = x0 + threadIdx.x;
    bool in = false;
    if (x < cols) in = vx_in_set(p[(row + x) * st], mode, thr);
    const unsigned long long b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && (x >> 6) < nw) bits[x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = -1;
    for (int w = 0; w < nw; ++w) {
      carry[w] = c;
      const unsigned long long b = bits[w];
      if (!(b >> 63)) {
        c = -1;
      } else {
        const int s = vx_run_start(b, 63);
        c = s >= 0 ? w * 64 + s : (c >= 0 ? c : w * 64);
      }
    }
    // the run that holds x = cols - 1 (bit (cols - 1) & 63 of the last word)
    int ws = -1;
    const int lastw = (cols - 1) >> 6, lastl = (cols - 1) & 63;
    if (((bits[lastw] >> lastl) & 1ull) && (bits[0] & 1ull)) {
      const int s = vx_run_start(bits[lastw], lastl);
      ws = s >= 0 ? lastw * 64 + s : (carry[lastw] >= 0 ? carry[lastw] : lastw * 64);
      if (ws == 0) ws = -1;                  // the whole row is one run already
    }
    wrap = ws;
  }
  __syncthreads();
  const int ws = wrap;
  for (int x = threadIdx.x; x < cols; x += VX_THREADS) {
    const int w = x >> 6, lane = x & 63;
    const unsigned long long b = bits[w];
    int label = -1;
    if ((b >> lane) & 1ull) {
      const int s = vx_run_start(b, lane);
      int start = s >= 0 ? w * 64 + s : (carry[w] >= 0 ? carry[w] : w * 64);
      if (start == ws) start = 0;
      label = (int)row + start;
    }
    L[row + x] = label;
  }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
// Row y against row yu = (y - 1) mod rows.  A union is issued by the first point (in x, from 0) of a run that touches an upper
// run; x = 0 never relies on its left neighbour x = cols - 1 (two full rows would otherwise issue nothing).
__global__ void __launch_bounds__(VX_THREADS) k_vx_merge(int rows, int cols, int conn, int* L) {
  const int y = blockIdx.x, yu = y == 0 ? rows - 1 : y - 1;
  const int row = y * cols, up = yu * cols;
  for (int x = threadIdx.x; x < cols; x += VX_THREADS) {
    if (vx_load(L, row + x) < 0) continue;
    const int xl = x == 0 ? cols - 1 : x - 1, xr = x == cols - 1 ? 0 : x + 1;
    const bool left = x > 0 && vx_load(L, row + xl) >= 0;             // the left neighbour is of this run and has looked up already
    const bool uc = vx_load(L, up + x) >= 0;
    if (conn == 4) {
      if (uc && !(left && vx_load(L, up + xl) >= 0)) vx_union(L, row + x, up + x);
    } else {
      const bool ul = vx_load(L, up + xl) >= 0, ur = vx_load(L, up + xr) >= 0;
      if (ul && !left) vx_union(L, row + x, up + xl);
      if (uc && !ul && !left) vx_union(L, row + x, up + x);
      if (ur && !uc) vx_union(L, row + x, up + xr);
    }
  }
}

// ---- flatten, prefix, rank ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int vx_block_sum(int v, int* red) {        // the sum of v over the workgroup, in every thread
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < VX_WAVES; ++w) t += red[w];
  return t;
}
__global__ void __launch_bounds__(VX_THREADS) k_vx_flatten(int cols, int* L, int* __restrict__ rowroots, int* __restrict__ rowset) {
  __shared__ int red[VX_WAVES];
  const int row = blockIdx.x * cols;
  int nroot = 0, nset = 0;
  for (int x = threadIdx.x; x < cols; x += VX_THREADS) {
    const int l = vx_load(L, row + x);
    if (l < 0) continue;
    ++nset;
    if (l == row + x) {
      ++nroot;
    } else {
      const int r = vx_find(L, l);
      if (r != l) vx_store(L, row + x, r);
    }
  }
  nroot = vx_block_sum(nroot, red);
  nset = vx_block_sum(nset, red);
  if (threadIdx.x == 0) {
    rowroots[blockIdx.x] = nroot;
    rowset[blockIdx.x] = nset;
  }
}
// info[0] = components, [1] = rows of the table, [2] = points in the set; rowoff[y] = roots in the rows before y
__global__ void __launch_bounds__(VX_THREADS) k_vx_prefix(int rows, int cap, const int* __restrict__ rowroots, const int* __restrict__ rowset,
                                                          int* __restrict__ rowoff, long long* __restrict__ info) {
  __shared__ long long sums[VX_THREADS], sets[VX_THREADS];
  const int per = (rows + VX_THREADS - 1) / VX_THREADS, y0 = threadIdx.x * per, y1 = y0 + per < rows ? y0 + per : rows;
  long long a = 0, s = 0;
  for (int y = y0; y < y1; ++y) {
    a += rowroots[y];
    s += rowset[y];
  }
  sums[threadIdx.x] = a;
  sets[threadIdx.x] = s;
  __syncthreads();
  long long before = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += sums[t];
  int at = (int)before;
  for (int y = y0; y < y1; ++y) {
    rowoff[y] = at;
    at += rowroots[y];
  }
  if (threadIdx.x == 0) {
    long long total = 0, set = 0;
    for (int t = 0; t < VX_THREADS; ++t) {
      total += sums[t];
      set += sets[t];
    }
    info[0] = total;
    info[1] = total < cap ? total : cap;
    info[2] = set;
  }
}
// tab: [cap][ncols] 64-bit; R: the rank plane, written at the roots only
__global__ void __launch_bounds__(VX_THREADS) k_vx_rank(int cols, int cap, int ncols, const int* __restrict__ L, const int* __restrict__ rowoff,
                                                        int* __restrict__ R, unsigned long long* __restrict__ tab) {
  __shared__ int wsum[VX_WAVES];
  const int row = blockIdx.x * cols, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = rowoff[blockIdx.x];
  for (int x0 = 0; x0 < cols; x0 += VX_THREADS) {
    const int x = x0 + threadIdx.x;
    const bool root = x < cols && L[row + x] == row + x;
    const unsigned long long b = __ballot(root);
    __syncthreads();                                          // the last round's reads of wsum
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
    for (int w = 0; w < VX_WAVES; ++w) {
      if (w < wave) before += wsum[w];
      all += wsum[w];
    }
    if (root) {
      const int rank = base + before;
      R[row + x] = rank;
      if (rank < cap) {
        unsigned long long* t = tab + (size_t)rank * ncols;
        t[0] = (unsigned long long)(row + x);
        for (int c = 1; c < ncols; ++c) t[c] = 0ull;
        t[7] = ~0ull;                                         // the identity of atomicMin on keys; t[8] = 0 is atomicMax's
      }
    }
    base += all;
  }
}

// ---- sums -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long vx_shfl_up(long long v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ unsigned long long vx_shfl_up(unsigned long long v, int d) { return (unsigned long long)__shfl_up((long long)v, d, 64); }
__device__ __forceinline__ int vx_offset(int d, int n) {     // ((d + n/2) mod n) - n/2 for d in (-n, n)
  int t = d + n / 2;
  t = t < 0 ? t + n : (t >= n ? t - n : t);
  return t - n / 2;
}
__global__ void __launch_bounds__(VX_THREADS) k_vx_sums(VxPlanes pl, int cap, int ncols, const int* __restrict__ L, const int* __restrict__ R,
                                                        const VxRange* __restrict__ rng, unsigned long long* __restrict__ tab) {
  const int y = blockIdx.x, cols = pl.cols, rows = pl.rows, lane = threadIdx.x & 63;
  const int row = y * cols;
  int sc[VX_MAX_FIELDS];
#pragma unroll
  for (int f = 0; f < VX_MAX_FIELDS; ++f) sc[f] = f < pl.nf ? rng->scale[f] : 0;
  for (int x0 = 0; x0 < cols; x0 += VX_THREADS) {            // whole waves take part in every shuffle
    const int x = x0 + threadIdx.x;
    int label = -1, rank = -1;
    if (x < cols) label = L[row + x];
    if (label >= 0) rank = R[label];
    if (rank >= cap) label = -2 - rank;                       // beyond the capacity: not summed (a value no two runs share is not needed: never emitted)
    const bool live = label >= 0;
    long long sdx = 0, sdx2 = 0, fx[VX_MAX_FIELDS] = {0, 0, 0};
    unsigned long long kmin = ~0ull, kmax = 0ull;
    int dy = 0;
    if (live) {
      const int y0 = label / cols, xq = label - y0 * cols;
      const int dx = vx_offset(x - xq, cols);
      dy = vx_offset(y - y0, rows);
      sdx = dx;
      sdx2 = (long long)dx * dx;
#pragma unroll
      for (int f = 0; f < VX_MAX_FIELDS; ++f)
        if (f < pl.nf) {
          const double a = pl.p[f][((size_t)row + x) * pl.stride[f]];
          fx[f] = vx_fixed(a, sc[f]);
          if (f == pl.crit) kmin = kmax = vx_key(a);
        }
    }
    // runs of equal labels within the wave: the head is the first lane of a run
    const int prev = __shfl_up(label, 1, 64);
    const bool head = lane == 0 || prev != label;
    const unsigned long long heads = __ballot(head);
    const int first = 63 - __clzll(heads & ((2ull << lane) - 1ull));   // (2 << 63) - 1 wraps to all ones
    const int dist = lane - first;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long a = vx_shfl_up(sdx, d), b = vx_shfl_up(sdx2, d);
      const unsigned long long lo = vx_shfl_up(kmin, d), hi = vx_shfl_up(kmax, d);
      long long g[VX_MAX_FIELDS];
#pragma unroll
      for (int f = 0; f < VX_MAX_FIELDS; ++f) g[f] = vx_shfl_up(fx[f], d);
      if (dist >= d) {
        sdx += a;
        sdx2 += b;
        kmin = lo < kmin ? lo : kmin;
        kmax = hi > kmax ? hi : kmax;
#pragma unroll
        for (int f = 0; f < VX_MAX_FIELDS; ++f) fx[f] += g[f];
      }
    }
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (live && tail) {
      const long long area = dist + 1;
      unsigned long long* t = tab + (size_t)rank * ncols;
      atomicAdd(&t[1], (unsigned long long)area);
      atomicAdd(&t[2], (unsigned long long)sdx);
      atomicAdd(&t[3], (unsigned long long)(area * dy));
      atomicAdd(&t[4], (unsigned long long)sdx2);
      atomicAdd(&t[5], (unsigned long long)(area * dy * dy));
      atomicAdd(&t[6], (unsigned long long)(sdx * dy));
      atomicMin(&t[7], kmin);
      atomicMax(&t[8], kmax);
#pragma unroll
      for (int f = 0; f < VX_MAX_FIELDS; ++f)
        if (f < pl.nf) atomicAdd(&t[VX_BASE_COLS + f], (unsigned long long)fx[f]);
    }
  }
}
__global__ void __launch_bounds__(VX_THREADS) k_vx_finish(int ncols, const long long* __restrict__ info, unsigned long long* __restrict__ tab) {
  const long long n = info[1];
  for (long long r = (long long)blockIdx.x * VX_THREADS + threadIdx.x; r < n; r += (long long)gridDim.x * VX_THREADS) {
    unsigned long long* t = tab + (size_t)r * ncols;
    t[7] = vx_unkey(t[7]);
    t[8] = vx_unkey(t[8]);
  }
}

}  // namespace nq
