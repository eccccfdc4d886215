// Structure functions at two-dimensional separations: moments of d_r a(x, y) = a((x + r_x) mod nx, (y + r_y) mod ny) - a(x, y) for
// a list of lattice vectors r = (r_x, r_y) (include/niwqg_amd.h: nq_structure2, nq_any_increments2;
// niwqg_amd/structure.py: reference2d restates the definitions in numpy).
//
// The columns, the canonical field slots and the triples are those of csrc/nq_sf.hpp (sf_add_real, sf_add_phi, sf_block_store and
// k_sf_total are reused).  One addition: an ordered pair (pa, pb) of real slots may be ROTATED per vector before anything is summed,
//   d_L = c_x d_a + c_y d_b,   d_T = -c_y d_a + c_x d_b,
// with (c_x, c_y) a pair of doubles per vector that the host supplies; slot pa then holds L and slot pb holds T, in the columns
// and inside the triples.
//
// Two steps.  k_x_flow_store (Kernel family, fused grids) writes the selected values of x_flow_values to physical planes of the
// context; QGModel and the any-size path have their planes already.  k_sf_plane2 then reads planes only: a workgroup owns base
// rows y, y + gridDim.x, ...; a thread keeps the base values of its PTS points of every field in registers; the vectors arrive
// sorted by r_y and row (y + r_y) mod ny of every field is loaded to LDS ONCE per distinct r_y, every r_x of that group is served
// from LDS.  k_sf_plane2_global is the route for rows that do not fit the LDS: shifted (and base) values straight from global memory.
// The sums are deterministic as in csrc/nq_sf.hpp: one partial slot per workgroup and vector (a workgroup that owns several rows
// adds them to its slot in row order), k_sf_total adds the slots in its fixed order.
#pragma once
#include "nq_sf.hpp"

namespace nq {

constexpr int SF2_MAX_VECS = 256, SF2_MAX_THREADS = 1024, SF2_GLOBAL_THREADS = 256;
// threads of a workgroup of the row route: 1024 (128 registers), or 512 (256 registers) where the base values of 8 points of three
// fields, or of 16 points of two, and the 31 / 22 running sums need more than 128
template <int PTS, int NREAL, int PHI> constexpr int sf2_tmax() { return ((PTS == 8 && NREAL + PHI == 3) || PTS == 16) ? 512 : SF2_MAX_THREADS; }
constexpr size_t SF2_LDS_LIMIT = 160 * 1024;

struct Sf2Vec {
  int rx, ry;                 // 0 <= rx < cols (a negative r_x arrives as r_x + cols), 0 <= ry < rows
  int slot;                   // the vector's row in the call's table (its position in the caller's list)
  int pad;
};
struct Sf2Args {
  int nvec;
  const Sf2Vec* vecs;         // on the device, sorted by ry
  const double* proj;         // on the device, [slot][2] = (c_x, c_y), or null: no rotation
  int pa, pb;                 // the rotated pair of real slots (-1, -1: none)
  int nreal, phi;
  int ntri;
  unsigned tri;               // the slots of triple k in bits 6 k .. 6 k + 5, two bits each: a, b, c; 3: phi (one word: scalar registers)
  double* part;               // [block][slot][sf_ncols<NF>()]
};
constexpr unsigned SF2_TRI_PHI = 3;
__host__ __device__ inline unsigned sf2_tri_pack(int k, int ta, int tb, int tc) {
  return ((unsigned)ta | (tb < 0 ? SF2_TRI_PHI : (unsigned)tb) << 2 | (tc < 0 ? SF2_TRI_PHI : (unsigned)tc) << 4) << (6 * k);
}

// ---- the store pass: x_flow_values' row block to physical planes ----------------------------------------------------------------
// re[s]: the (N, N) real plane of value slot s (null: not stored), phi: the complex plane (null: not stored).  Row-major in
// physical order; lanes write consecutive elements (avg_row_add's addressing without the read).
struct Sf2Store {
  double* re[HIST_SLOTS];
  cd* phi;
};
template <int N, int MODE>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_flow_store(MArr Mq, MArr Mqw, MArr Mu, MArr Mp, MArr Mphi, MArr Mphiy, const cd* __restrict__ tw, const double* __restrict__ kk,
               FlowSel sel, Sf2Store st) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T, NV = flow_nv<N>();
  double val[NV][P];
  cd w[P];
  x_flow_values<N, MODE, false>(Mq, Mqw, Mu, Mp, Mphi, Mphiy, tw, kk, sel, val, w);
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const size_t at = ((size_t)blockIdx.x * X::C + c) * N + j;           // point t of the thread: at + t * T
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    if (st.re[s]) {
      double* __restrict__ pl = st.re[s] + at;
#pragma unroll
      for (int t = 0; t < P; ++t) pl[t * T] = val[s][t];
    }
  }
  if (st.phi) {
    cd* __restrict__ pl = st.phi + at;
#pragma unroll
    for (int t = 0; t < P; ++t) pl[t * T] = w[t];
  }
}

// ---- the increments of one point: rotation, columns, triples --------------------------------------------------------------------
template <int NF>
__device__ __forceinline__ void sf2_point(const Sf2Args& a, int nreal, int phi, double cx, double cy, double (&d)[NF], double dr, double di,
                                          double (&acc)[NF][SF_COLS], double (&tri)[sf_ntri<NF>()]) {
  if (a.pa >= 0) {
    const double da = sf_pick(a.pa, d[0], d[NF > 1 ? 1 : 0], d[NF - 1]), db = sf_pick(a.pb, d[0], d[NF > 1 ? 1 : 0], d[NF - 1]);
    const double L = cx * da + cy * db, Tr = cx * db - cy * da;
#pragma unroll
    for (int f = 0; f < NF; ++f) d[f] = f == a.pa ? L : (f == a.pb ? Tr : d[f]);
  }
  double m2 = 0.0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (f < nreal) {
      sf_add_real(acc[f], d[f]);
    } else if (f == nreal && phi) {
      m2 = dr * dr + di * di;
      sf_add_phi(acc[f], dr, di, m2);
    }
  }
#pragma unroll
  for (int k = 0; k < sf_ntri<NF>(); ++k) {
    if (k < a.ntri) {
      const unsigned t = a.tri >> (6 * k);
      const int tb = (t >> 2) & 3, tc = (t >> 4) & 3;
      const double da = sf_pick(t & 3, d[0], d[NF > 1 ? 1 : 0], d[NF - 1]);
      tri[k] += tb == (int)SF2_TRI_PHI ? da * m2 : da * sf_pick(tb, d[0], d[NF > 1 ? 1 : 0], d[NF - 1]) * sf_pick(tc, d[0], d[NF > 1 ? 1 : 0], d[NF - 1]);
    }
  }
}

// LDS of a launch of the row route: the shifted rows (a real field cols doubles, phi cols complex), then the two reduction buffers
template <int NREAL, int PHI> __host__ __device__ constexpr size_t sf2_lds_bytes(int cols, int threads) {
  return ((size_t)(NREAL + 2 * PHI) * cols + 2 * (size_t)(threads / 64) * sf_ncols<NREAL + PHI>()) * sizeof(double);
}

// ---- the row route ---------------------------------------------------------------------------------------------------------------
// blockDim.x = a multiple of 64 with blockDim.x * PTS >= cols; point t of a thread is x = threadIdx.x + t blockDim.x (lanes read
// consecutive elements, in global memory and in LDS).  Planes as in SfPlanes (stride doubles per element; the complex one last).
template <int PTS, int NREAL, int PHI>
__global__ void __launch_bounds__((sf2_tmax<PTS, NREAL, PHI>())) k_sf_plane2(SfPlanes pl, Sf2Args a) {
  constexpr int NF = NREAL + PHI, NC = sf_ncols<NF>();
  const int tid = threadIdx.x, nt = blockDim.x, cols = pl.cols;
  double* rows = reinterpret_cast<double*>(nq_smem);
  double* prow = rows + (size_t)NREAL * cols;              // (re, im) pairs
  double* red = rows + (size_t)(NREAL + 2 * PHI) * cols;
  int calls = 0;
#pragma unroll 1
  for (int y = blockIdx.x; y < pl.rows; y += gridDim.x) {
    const bool add = y != (int)blockIdx.x;                 // a later row of this workgroup: on top of its slot
    double base[NREAL > 0 ? NREAL : 1][PTS], bre[PTS], bim[PTS];
#pragma unroll
    for (int t = 0; t < PTS; ++t) {
      const int x = tid + t * nt;
      const size_t at = (size_t)y * cols + (x < cols ? x : 0);
#pragma unroll
      for (int f = 0; f < NREAL; ++f) base[f][t] = pl.p[f][at * pl.stride[f]];
      bre[t] = PHI ? pl.p[NREAL][at * 2] : 0.0;
      bim[t] = PHI ? pl.p[NREAL][at * 2 + 1] : 0.0;
    }
    int cur = -1;
#pragma unroll 1
    for (int v = 0; v < a.nvec; ++v) {
      const Sf2Vec r = a.vecs[v];
      if (r.ry != cur) {
        // every wave is past the barrier of the last sf_block_store, that is past its reads of the rows in LDS
        cur = r.ry;
        int yr = y + r.ry;
        yr = yr >= pl.rows ? yr - pl.rows : yr;
#pragma unroll
        for (int t = 0; t < PTS; ++t) {
          const int x = tid + t * nt;
          if (x < cols) {
            const size_t at = (size_t)yr * cols + x;
#pragma unroll
            for (int f = 0; f < NREAL; ++f) rows[(size_t)f * cols + x] = pl.p[f][at * pl.stride[f]];
            if (PHI) {
              prow[2 * x] = pl.p[NREAL][at * 2];
              prow[2 * x + 1] = pl.p[NREAL][at * 2 + 1];
            }
          }
        }
        wg_barrier();
      }
      double cx = 1.0, cy = 0.0;
      if (a.proj) {
        cx = a.proj[2 * r.slot];
        cy = a.proj[2 * r.slot + 1];
      }
      double acc[NF][SF_COLS], tri[sf_ntri<NF>()];
      sf_zero<NF>(acc, tri);
#pragma unroll
      for (int t = 0; t < PTS; ++t) {
        const int x = tid + t * nt;
        if (x < cols) {
          int xr = x + r.rx;
          xr = xr >= cols ? xr - cols : xr;
          double d[NF], dr = 0.0, di = 0.0;
#pragma unroll
          for (int f = 0; f < NF; ++f) d[f] = f < NREAL ? rows[(size_t)f * cols + xr] - base[f < NREAL ? f : 0][t] : 0.0;
          if (PHI) {
            dr = prow[2 * xr] - bre[t];
            di = prow[2 * xr + 1] - bim[t];
          }
          sf2_point<NF>(a, NREAL, PHI, cx, cy, d, dr, di, acc, tri);
        }
        __builtin_amdgcn_sched_barrier(0);                 // one point's powers at a time: the registers of the next are not live yet
      }
      sf_block_store<NF>(acc, tri, red + (calls & 1) * (nt >> 6) * NC, a.part + ((size_t)blockIdx.x * a.nvec + r.slot) * NC, add);
      ++calls;
    }
  }
}

// ---- the global route: rows too long for the LDS (three real fields or phi beside a real one at 8192 columns, longer rows) -------
// k_sf_plane with the row shift: both values of an increment come from global memory (the base row of a workgroup stays in its
// cache over the vectors).
template <int NREAL, int PHI>
__global__ void __launch_bounds__(SF2_GLOBAL_THREADS) k_sf_plane2_global(SfPlanes pl, Sf2Args a) {
  constexpr int NF = NREAL + PHI, NC = sf_ncols<NF>();
  __shared__ double red[2 * (SF2_GLOBAL_THREADS / 64) * NC];
  int calls = 0;
#pragma unroll 1
  for (int y = blockIdx.x; y < pl.rows; y += gridDim.x) {
    const bool add = y != (int)blockIdx.x;
#pragma unroll 1
    for (int v = 0; v < a.nvec; ++v) {
      const Sf2Vec r = a.vecs[v];
      int yr = y + r.ry;
      yr = yr >= pl.rows ? yr - pl.rows : yr;
      double cx = 1.0, cy = 0.0;
      if (a.proj) {
        cx = a.proj[2 * r.slot];
        cy = a.proj[2 * r.slot + 1];
      }
      double acc[NF][SF_COLS], tri[sf_ntri<NF>()];
      sf_zero<NF>(acc, tri);
      for (int x = threadIdx.x; x < pl.cols; x += SF2_GLOBAL_THREADS) {
        int xr = x + r.rx;
        xr = xr >= pl.cols ? xr - pl.cols : xr;
        const size_t at = (size_t)y * pl.cols + x, atr = (size_t)yr * pl.cols + xr;
        double d[NF], dr = 0.0, di = 0.0;
#pragma unroll
        for (int f = 0; f < NF; ++f) d[f] = f < NREAL ? pl.p[f][atr * pl.stride[f]] - pl.p[f][at * pl.stride[f]] : 0.0;
        if (PHI) {
          dr = pl.p[NREAL][atr * 2] - pl.p[NREAL][at * 2];
          di = pl.p[NREAL][atr * 2 + 1] - pl.p[NREAL][at * 2 + 1];
        }
        sf2_point<NF>(a, NREAL, PHI, cx, cy, d, dr, di, acc, tri);
      }
      sf_block_store<NF>(acc, tri, red + (calls & 1) * (SF2_GLOBAL_THREADS / 64) * NC, a.part + ((size_t)blockIdx.x * a.nvec + r.slot) * NC, add);
      ++calls;
    }
  }
}

}  // namespace nq
