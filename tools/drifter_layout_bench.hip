// Plane layout of the drifter step: the RK4 kernel gathers the velocity U = u + i v and the wave field
// phi through one 4 x 4 stencil per stage.  Two double2 planes give two 64-byte segments per stencil row; one interleaved plane
// of 32-byte nodes (u, v, Re phi, Im phi) gives one 128-byte line.  This times both on random planes and uniformly placed
// particles: k_pt_rk4_w of the library (csrc/nq_particles.hpp) against the same step on interleaved planes, and the pass that
// would have to interleave them.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/drifter_layout_bench.hip -o tools/drifter_layout_bench
//   tools/drifter_layout_bench [nx = 4096] [reps = 9]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../niwqg_amd/csrc/nq_particles.hpp"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

using namespace nq;

struct Node { cd u, p; };

__device__ __forceinline__ void gather_node(const Node* __restrict__ W, const PtGrid& g, const PtStencil& s, cd& v, cd& w) {
  if (!s.ok) {
    pt_nan(v);
    pt_nan(w);
    return;
  }
  pt_zero(v);
  pt_zero(w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const Node* row = W + (size_t)s.iy[j] * g.n;
    cd rv, rw;
    pt_zero(rv);
    pt_zero(rw);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const Node nd = row[s.ix[i]];
      pt_madd(rv, s.wx[i], nd.u);
      pt_madd(rw, s.wx[i], nd.p);
    }
    pt_madd(v, s.wy[j], rv);
    pt_madd(w, s.wy[j], rw);
  }
}
__device__ __forceinline__ cd vel_node(const Node* __restrict__ W0, const Node* __restrict__ W1, const PtGrid& g, double x, double y, int st,
                                       double Ub, const PtWave& wv) {
  const PtStencil s = pt_stencil(g, x, y);
  cd v, w;
  if (st == 0) gather_node(W0, g, s, v, w);
  else if (st == 2) gather_node(W1, g, s, v, w);
  else {
    cd v1, w1;
    gather_node(W0, g, s, v, w);
    gather_node(W1, g, s, v1, w1);
    v = make_double2(0.5 * (v.x + v1.x), 0.5 * (v.y + v1.y));
    w = make_double2(0.5 * (w.x + w1.x), 0.5 * (w.y + w1.y));
  }
  const cd ww = pt_wave_vel(w, wv.a, wv.c[st], wv.s[st]);
  return make_double2((v.x + Ub) + ww.x, v.y + ww.y);
}
__global__ void __launch_bounds__(256) k_rk4_node(double* __restrict__ px, double* __restrict__ py, int n, const Node* W0, const Node* W1,
                                                  PtGrid g, double Ub, double dt, PtWave wv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double x0 = px[i], y0 = py[i], h = 0.5 * dt;
    const cd k1 = vel_node(W0, W1, g, x0, y0, 0, Ub, wv);
    const cd k2 = vel_node(W0, W1, g, x0 + h * k1.x, y0 + h * k1.y, 1, Ub, wv);
    const cd k3 = vel_node(W0, W1, g, x0 + h * k2.x, y0 + h * k2.y, 1, Ub, wv);
    const cd k4 = vel_node(W0, W1, g, x0 + dt * k3.x, y0 + dt * k3.y, 2, Ub, wv);
    px[i] = x0 + dt / 6.0 * (k1.x + 2.0 * k2.x + 2.0 * k3.x + k4.x);
    py[i] = y0 + dt / 6.0 * (k1.y + 2.0 * k2.y + 2.0 * k3.y + k4.y);
  }
}
// what forming the interleaved plane costs when the row kernels keep writing contiguous planes: one more pass
__global__ void __launch_bounds__(256) k_interleave(const cd* __restrict__ U, const cd* __restrict__ P, Node* __restrict__ W, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Node nd;
    nd.u = U[i];
    nd.p = P[i];
    W[i] = nd;
  }
}

static float median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 4096, reps = argc > 2 ? atoi(argv[2]) : 9;
  const size_t plane = (size_t)N * N;
  const double L = 1.0e6, dx = L / N;
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  std::vector<cd> h(plane);
  cd* d[4];                                          // U0, U1, P0, P1
  for (int k = 0; k < 4; ++k) {
    for (size_t i = 0; i < plane; ++i) h[i] = make_double2(uni(rng), uni(rng));
    CK(hipMalloc(&d[k], plane * sizeof(cd)));
    CK(hipMemcpy(d[k], h.data(), plane * sizeof(cd), hipMemcpyHostToDevice));
  }
  Node* W[2];
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> til;
  for (int k = 0; k < 2; ++k) CK(hipMalloc(&W[k], plane * sizeof(Node)));
  for (int r = 0; r < reps; ++r)
    for (int k = 0; k < 2; ++k) {
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL(k_interleave, dim3(4096), dim3(256), 0, 0, (const cd*)d[k], (const cd*)d[2 + k], W[k], plane);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      til.push_back(ms);
    }
  printf("nx %d: interleaving one pair of planes %.1f us (median of %d)\n", N, 1e3 * median(til), (int)til.size());
  const PtGrid g{N, L, L, dx, dx};
  PtWave wv;
  wv.a = 1.0;
  for (int k = 0; k < 3; ++k) {
    wv.c[k] = cos(0.1 * k);
    wv.s[k] = -sin(0.1 * k);
  }
  const double dt = dx;                              // |velocity| <= a few: a particle crosses a few cells per step
  for (int e = 16; e <= 20; e += 2) {
    const int n = 1 << e, nb = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    std::vector<double> hx(n), hy(n);
    for (int i = 0; i < n; ++i) {
      hx[i] = 0.5 * (uni(rng) + 1.0) * L;
      hy[i] = 0.5 * (uni(rng) + 1.0) * L;
    }
    double *px, *py;
    CK(hipMalloc(&px, n * sizeof(double)));
    CK(hipMalloc(&py, n * sizeof(double)));
    std::vector<float> two, one;
    for (int r = 0; r < reps + 1; ++r)               // alternating; the first pair is the warm-up
      for (int lay = 0; lay < 2; ++lay) {
        CK(hipMemcpy(px, hx.data(), n * sizeof(double), hipMemcpyHostToDevice));
        CK(hipMemcpy(py, hy.data(), n * sizeof(double), hipMemcpyHostToDevice));
        CK(hipEventRecord(e0));
        if (lay == 0)
          hipLaunchKernelGGL(k_pt_rk4_w, dim3(nb), dim3(256), 0, 0, px, py, n, (const cd*)d[0], (const cd*)d[1], (const cd*)d[2], (const cd*)d[3], g,
                             0.1, dt, wv);
        else hipLaunchKernelGGL(k_rk4_node, dim3(nb), dim3(256), 0, 0, px, py, n, (const Node*)W[0], (const Node*)W[1], g, 0.1, dt, wv);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r > 0) (lay == 0 ? two : one).push_back(ms);
      }
    printf("2^%d particles: two double2 planes %.1f us, one interleaved plane %.1f us (medians of %d, alternating)\n", e, 1e3 * median(two),
           1e3 * median(one), reps);
    CK(hipFree(px));
    CK(hipFree(py));
  }
  return 0;
}
