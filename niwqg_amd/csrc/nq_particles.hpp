// Lagrangian particles advected inside the step: the velocity plane of a state, the periodic cubic
// convolution that interpolates a physical plane at a particle, the RK4 step linear in time, and sampling; the same step with
// the near-inertial wave velocity a phi e^{-i f0 t} added (drifter mode, section 5s); and the rays of near-inertial wave packets,
// each particle carrying a wavevector through the flow and its vorticity zeta (ray mode, section 5t); and the deformation gradient
// F = d x(t) / d x0 carried along each trajectory, with or without the wave velocity (stretch mode, section 5u).
//
// Grid value [j, i] of an (n, n) physical plane sits at ((i + 1/2) dx, (j + 1/2) dy) (the reference's _initialize_grid).
// Interpolation is the tensor product of Keys' cubic convolution kernel (a = -1/2) on the 4 x 4 nearest nodes: exact at the
// nodes, C^1, third order.  A coordinate is reduced into [0, L) with fmod first; every node index is reduced modulo n in integer
// arithmetic after the cast, so no input -- NaN and +-inf included -- addresses outside the plane.  A non-finite coordinate
// gives NaN without any load (its indices and weights are zeroed and pt_gather returns before reading the plane).
#pragma once
#include "nq_hist.hpp"

namespace nq {

struct PtGrid {
  int n;             // points per side of the physical plane
  double Lx, Ly;     // domain lengths
  double dx, dy;     // Lx / n, Ly / n
};

// Keys (1981), a = -1/2: weights of the nodes at offsets -1, 0, 1, 2 from the cell's left node, t in [0, 1)
__device__ __forceinline__ void pt_keys(double t, double w[4]) {
  w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
  w[1] = (1.5 * t - 2.5) * t * t + 1.0;
  w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
  w[3] = (0.5 * t - 0.5) * t * t;
}

// node indices and weights along one axis; false for a non-finite coordinate (indices 0, weights 0)
__device__ __forceinline__ bool pt_axis(double x, double L, double d, int n, int idx[4], double w[4]) {
  if (!isfinite(x)) {
#pragma unroll
    for (int o = 0; o < 4; ++o) { idx[o] = 0; w[o] = 0.0; }
    return false;
  }
  double r = fmod(x, L);
  if (r < 0.0) r += L;
  if (r >= L) r -= L;
  const double s = r / d - 0.5;                      // in node units: node i at s = i
  double f = floor(s);
  if (!(f >= -1.0 && f <= (double)n)) f = 0.0;       // (cannot happen for r in [0, L); keeps the cast defined)
  const int i0 = (int)f;
  pt_keys(s - f, w);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    int m = (i0 - 1 + o) % n;
    if (m < 0) m += n;
    idx[o] = m;
  }
  return true;
}

__device__ __forceinline__ void pt_madd(double& acc, double w, double v) { acc += w * v; }
__device__ __forceinline__ void pt_madd(cd& acc, double w, cd v) { acc.x += w * v.x; acc.y += w * v.y; }
__device__ __forceinline__ void pt_zero(double& a) { a = 0.0; }
__device__ __forceinline__ void pt_zero(cd& a) { a = make_double2(0.0, 0.0); }
__device__ __forceinline__ void pt_nan(double& a) { a = __builtin_nan(""); }
__device__ __forceinline__ void pt_nan(cd& a) { a = make_double2(__builtin_nan(""), __builtin_nan("")); }

struct PtStencil {
  int ix[4], iy[4];
  double wx[4], wy[4];
  bool ok;
};
__device__ __forceinline__ PtStencil pt_stencil(const PtGrid& g, double x, double y) {
  PtStencil s;
  const bool okx = pt_axis(x, g.Lx, g.dx, g.n, s.ix, s.wx);
  const bool oky = pt_axis(y, g.Ly, g.dy, g.n, s.iy, s.wy);
  s.ok = okx && oky;
  return s;
}
// sum_j wy[j] (sum_i wx[i] plane[iy[j], ix[i]]): the row sums first, in this order (the numpy restatement of the tests
// follows it)
template <typename T>
__device__ __forceinline__ T pt_gather(const T* __restrict__ plane, const PtGrid& g, const PtStencil& s) {
  T acc;
  if (!s.ok) {
    pt_nan(acc);
    return acc;
  }
  pt_zero(acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const T* row = plane + (size_t)s.iy[j] * g.n;
    T r;
    pt_zero(r);
#pragma unroll
    for (int i = 0; i < 4; ++i) pt_madd(r, s.wx[i], row[s.ix[i]]);
    pt_madd(acc, s.wy[j], r);
  }
  return acc;
}

// One RK4 step of every particle from t to t + dt through the velocity (Ub + u, v), u + i v interpolated from U0 (start of the
// step) and U1 (end), linear in time between them: k2, k3 take the mean of the two interpolated values.  U0 == U1: a steady
// velocity (one gather per stage).  One particle per thread, in the caller's order: each stencil is 4 rows x 64 B of a
// double2 plane; neighbouring particles of a wave share lines only as far as the caller ordered them.
__device__ __forceinline__ cd pt_vel(const cd* __restrict__ U0, const cd* __restrict__ U1, const PtGrid& g, double x, double y,
                                     int which, double Ub) {
  // which 0: U0, 1: U1, 2: (U0 + U1) / 2
  const PtStencil s = pt_stencil(g, x, y);
  cd v;
  if (which == 0) v = pt_gather(U0, g, s);
  else if (which == 1) v = pt_gather(U1, g, s);
  else if (U0 == U1) v = pt_gather(U0, g, s);
  else {
    const cd a = pt_gather(U0, g, s), b = pt_gather(U1, g, s);
    v = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y + b.y));
  }
  v.x += Ub;
  return v;
}
__device__ __forceinline__ void pt_rk4(const cd* __restrict__ U0, const cd* __restrict__ U1, const PtGrid& g, double Ub, double dt,
                                       double& x, double& y) {
  const double x0 = x, y0 = y, h = 0.5 * dt;
  const cd k1 = pt_vel(U0, U1, g, x0, y0, 0, Ub);
  const cd k2 = pt_vel(U0, U1, g, x0 + h * k1.x, y0 + h * k1.y, 2, Ub);
  const cd k3 = pt_vel(U0, U1, g, x0 + h * k2.x, y0 + h * k2.y, 2, Ub);
  const cd k4 = pt_vel(U0, U1, g, x0 + dt * k3.x, y0 + dt * k3.y, 1, Ub);
  x = x0 + dt / 6.0 * (k1.x + 2.0 * k2.x + 2.0 * k3.x + k4.x);
  y = y0 + dt / 6.0 * (k1.y + 2.0 * k2.y + 2.0 * k3.y + k4.y);
}

// fused contexts: positions in two arrays (unwrapped)
__global__ void __launch_bounds__(256) k_pt_rk4(double* __restrict__ px, double* __restrict__ py, int n, const cd* U0, const cd* U1,
                                                PtGrid g, double Ub, double dt) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double x = px[i], y = py[i];
    pt_rk4(U0, U1, g, Ub, dt, x, y);
    px[i] = x;
    py[i] = y;
  }
}
// any-size engine: positions as one complex array x + i y
__global__ void __launch_bounds__(256) k_pt_rk4_c(cd* __restrict__ pos, int n, const cd* U0, const cd* U1, PtGrid g, double Ub,
                                                  double dt) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double x = pos[i].x, y = pos[i].y;
    pt_rk4(U0, U1, g, Ub, dt, x, y);
    pos[i] = make_double2(x, y);
  }
}

// ---- drifter mode: the wave velocity a phi e^{-i f0 t} added to (Ub + u, v) -------------------------
// The amplitude and the phase factors e^{-i f0 t} = (c, s) at the three stage times t, t + dt/2, t + dt of one step; the host
// forms them in double precision.
struct PtWave {
  double a;
  double c[3], s[3];
};
// a (w.x + i w.y) (c + i s)
__device__ __forceinline__ cd pt_wave_vel(const cd w, double a, double c, double s) {
  return make_double2(a * (w.x * c - w.y * s), a * (w.x * s + w.y * c));
}
// pt_vel with the wave term: ONE stencil per stage position, shared by the U and the phi gathers (two 64-byte segments per
// stencil row).  The slow envelope is linear in time (the mean of the two interpolated values at the half step), the fast phase
// exact at the stage time `st` (0: t, 1: t + dt/2, 2: t + dt).
__device__ __forceinline__ cd pt_vel_w(const cd* __restrict__ U0, const cd* __restrict__ U1, const cd* __restrict__ P0,
                                       const cd* __restrict__ P1, const PtGrid& g, double x, double y, int st, double Ub,
                                       const PtWave& wv) {
  const PtStencil s = pt_stencil(g, x, y);
  cd v, w;
  if (st == 0) {
    v = pt_gather(U0, g, s);
    w = pt_gather(P0, g, s);
  } else if (st == 2) {
    v = pt_gather(U1, g, s);
    w = pt_gather(P1, g, s);
  } else {
    v = pt_gather(U0, g, s);
    if (U0 != U1) {
      const cd b = pt_gather(U1, g, s);
      v = make_double2(0.5 * (v.x + b.x), 0.5 * (v.y + b.y));
    }
    const cd p = pt_gather(P0, g, s), q = pt_gather(P1, g, s);
    w = make_double2(0.5 * (p.x + q.x), 0.5 * (p.y + q.y));
  }
  const cd ww = pt_wave_vel(w, wv.a, wv.c[st], wv.s[st]);
  return make_double2((v.x + Ub) + ww.x, v.y + ww.y);
}
__device__ __forceinline__ void pt_rk4_w(const cd* __restrict__ U0, const cd* __restrict__ U1, const cd* __restrict__ P0,
                                         const cd* __restrict__ P1, const PtGrid& g, double Ub, double dt, const PtWave& wv,
                                         double& x, double& y) {
  const double x0 = x, y0 = y, h = 0.5 * dt;
  const cd k1 = pt_vel_w(U0, U1, P0, P1, g, x0, y0, 0, Ub, wv);
  const cd k2 = pt_vel_w(U0, U1, P0, P1, g, x0 + h * k1.x, y0 + h * k1.y, 1, Ub, wv);
  const cd k3 = pt_vel_w(U0, U1, P0, P1, g, x0 + h * k2.x, y0 + h * k2.y, 1, Ub, wv);
  const cd k4 = pt_vel_w(U0, U1, P0, P1, g, x0 + dt * k3.x, y0 + dt * k3.y, 2, Ub, wv);
  x = x0 + dt / 6.0 * (k1.x + 2.0 * k2.x + 2.0 * k3.x + k4.x);
  y = y0 + dt / 6.0 * (k1.y + 2.0 * k2.y + 2.0 * k3.y + k4.y);
}
// fused contexts
__global__ void __launch_bounds__(256) k_pt_rk4_w(double* __restrict__ px, double* __restrict__ py, int n, const cd* U0, const cd* U1,
                                                  const cd* P0, const cd* P1, PtGrid g, double Ub, double dt, PtWave wv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double x = px[i], y = py[i];
    pt_rk4_w(U0, U1, P0, P1, g, Ub, dt, wv, x, y);
    px[i] = x;
    py[i] = y;
  }
}
// any-size engine
__global__ void __launch_bounds__(256) k_pt_rk4_wc(cd* __restrict__ pos, int n, const cd* U0, const cd* U1, const cd* P0, const cd* P1,
                                                   PtGrid g, double Ub, double dt, PtWave wv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double x = pos[i].x, y = pos[i].y;
    pt_rk4_w(U0, U1, P0, P1, g, Ub, dt, wv, x, y);
    pos[i] = make_double2(x, y);
  }
}

// ---- ray mode: near-inertial wave packets traced through the flow -----------------------------------------
// A packet at (x, y) with wavevector (k, l) follows Hamilton's equations of
//   omega = (Ub + u) k + v l + zeta / 2 + (eta / 2) (k^2 + l^2),        eta = f / kappa^2, zeta = q_psi:
//   dx/dt = Ub + u + eta k                    dy/dt = v + eta l
//   dk/dt = -(k u_x + l v_x) - zeta_x / 2     dl/dt = -(k u_y + l v_y) - zeta_y / 2
// u, v, zeta AND their gradients come from the one interpolant: the derivative of the tensor-product Keys interpolant is the
// contraction of the same 16 nodes with the derivative weights w'(t) / d along one axis, so the discrete system is Hamilton's
// of the interpolated omega exactly.
// d/dt of pt_keys' weights
__device__ __forceinline__ void pt_keys_d(double t, double w[4]) {
  w[0] = (-1.5 * t + 2.0) * t - 0.5;
  w[1] = (4.5 * t - 5.0) * t;
  w[2] = (-4.5 * t + 4.0) * t + 0.5;
  w[3] = (1.5 * t - 1.0) * t;
}
// pt_axis with the derivative weights dw = w'(t) / d beside w
__device__ __forceinline__ bool pt_axis_d(double x, double L, double d, int n, int idx[4], double w[4], double dw[4]) {
  if (!isfinite(x)) {
#pragma unroll
    for (int o = 0; o < 4; ++o) { idx[o] = 0; w[o] = 0.0; dw[o] = 0.0; }
    return false;
  }
  double r = fmod(x, L);
  if (r < 0.0) r += L;
  if (r >= L) r -= L;
  const double s = r / d - 0.5;
  double f = floor(s);
  if (!(f >= -1.0 && f <= (double)n)) f = 0.0;
  const int i0 = (int)f;
  pt_keys(s - f, w);
  pt_keys_d(s - f, dw);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    dw[o] /= d;
    int m = (i0 - 1 + o) % n;
    if (m < 0) m += n;
    idx[o] = m;
  }
  return true;
}
struct PtStencilD {
  int ix[4], iy[4];
  double wx[4], wy[4], dwx[4], dwy[4];
  bool ok;
};
__device__ __forceinline__ PtStencilD pt_stencil_d(const PtGrid& g, double x, double y) {
  PtStencilD s;
  const bool okx = pt_axis_d(x, g.Lx, g.dx, g.n, s.ix, s.wx, s.dwx);
  const bool oky = pt_axis_d(y, g.Ly, g.dy, g.n, s.iy, s.wy, s.dwy);
  s.ok = okx && oky;
  return s;
}
// value, d/dx and d/dy of the interpolant: the three contractions w (x) w, w' (x) w, w (x) w' of the 16 loaded nodes; per row the
// sums over i with wx and with dwx first, then over j (the numpy restatement follows this order)
template <typename T>
struct PtJet {
  T f, fx, fy;
};
template <typename T>
__device__ __forceinline__ PtJet<T> pt_gather_d(const T* __restrict__ plane, const PtGrid& g, const PtStencilD& s) {
  PtJet<T> a;
  if (!s.ok) {
    pt_nan(a.f);
    pt_nan(a.fx);
    pt_nan(a.fy);
    return a;
  }
  pt_zero(a.f);
  pt_zero(a.fx);
  pt_zero(a.fy);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const T* row = plane + (size_t)s.iy[j] * g.n;
    T r, rd;
    pt_zero(r);
    pt_zero(rd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const T v = row[s.ix[i]];
      pt_madd(r, s.wx[i], v);
      pt_madd(rd, s.dwx[i], v);
    }
    pt_madd(a.f, s.wy[j], r);
    pt_madd(a.fx, s.wy[j], rd);
    pt_madd(a.fy, s.dwy[j], r);
  }
  return a;
}
__device__ __forceinline__ double pt_mean(double a, double b) { return 0.5 * (a + b); }
__device__ __forceinline__ cd pt_mean(cd a, cd b) { return make_double2(0.5 * (a.x + b.x), 0.5 * (a.y + b.y)); }
template <typename T>
__device__ __forceinline__ PtJet<T> pt_mean(const PtJet<T>& a, const PtJet<T>& b) {
  PtJet<T> m;
  m.f = pt_mean(a.f, b.f);
  m.fx = pt_mean(a.fx, b.fx);
  m.fy = pt_mean(a.fy, b.fy);
  return m;
}
// the jet of plane 0 (st == 0), of plane 1 (st == 2) or the mean of the two (st == 1: the half step, fields linear in time);
// A0 == A1: a steady plane, one gather
template <typename T>
__device__ __forceinline__ PtJet<T> pt_jet_at(const T* __restrict__ A0, const T* __restrict__ A1, const PtGrid& g, const PtStencilD& s,
                                              int st) {
  if (st == 0 || A0 == A1) return pt_gather_d(A0, g, s);
  if (st == 2) return pt_gather_d(A1, g, s);
  return pt_mean(pt_gather_d(A0, g, s), pt_gather_d(A1, g, s));
}
// zeta planes are real (fused contexts) or complex with zeta in the real part (engine planes)
__device__ __forceinline__ double pt_re(double a) { return a; }
__device__ __forceinline__ double pt_re(cd a) { return a.x; }

struct PtRay {
  double x, y, k, l;
};
// the right-hand side of the four ray equations at one stage: ONE stencil serves every gather
template <typename Z>
__device__ __forceinline__ PtRay pt_ray_rhs(const cd* __restrict__ U0, const cd* __restrict__ U1, const Z* __restrict__ Z0,
                                            const Z* __restrict__ Z1, const PtGrid& g, const PtRay& p, int st, double Ub, double eta) {
  const PtStencilD s = pt_stencil_d(g, p.x, p.y);
  const PtJet<cd> U = pt_jet_at(U0, U1, g, s, st);
  const PtJet<Z> z = pt_jet_at(Z0, Z1, g, s, st);
  PtRay d;
  d.x = (U.f.x + Ub) + eta * p.k;
  d.y = U.f.y + eta * p.l;
  d.k = -(p.k * U.fx.x + p.l * U.fx.y) - 0.5 * pt_re(z.fx);
  d.l = -(p.k * U.fy.x + p.l * U.fy.y) - 0.5 * pt_re(z.fy);
  return d;
}
__device__ __forceinline__ PtRay pt_ray_at(const PtRay& p, double h, const PtRay& d) {
  PtRay q;
  q.x = p.x + h * d.x;
  q.y = p.y + h * d.y;
  q.k = p.k + h * d.k;
  q.l = p.l + h * d.l;
  return q;
}
__device__ __forceinline__ double pt_rk4_sum(double a, double dt, double k1, double k2, double k3, double k4) {
  return a + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4);
}
// one classical RK4 step of a ray, the time treatment of pt_rk4: stages at t, t + dt/2, t + dt/2, t + dt
template <typename Z>
__device__ __forceinline__ void pt_rk4_ray(const cd* __restrict__ U0, const cd* __restrict__ U1, const Z* __restrict__ Z0,
                                           const Z* __restrict__ Z1, const PtGrid& g, double Ub, double eta, double dt, PtRay& p) {
  const double h = 0.5 * dt;
  const PtRay k1 = pt_ray_rhs(U0, U1, Z0, Z1, g, p, 0, Ub, eta);
  const PtRay k2 = pt_ray_rhs(U0, U1, Z0, Z1, g, pt_ray_at(p, h, k1), 1, Ub, eta);
  const PtRay k3 = pt_ray_rhs(U0, U1, Z0, Z1, g, pt_ray_at(p, h, k2), 1, Ub, eta);
  const PtRay k4 = pt_ray_rhs(U0, U1, Z0, Z1, g, pt_ray_at(p, dt, k3), 2, Ub, eta);
  p.x = pt_rk4_sum(p.x, dt, k1.x, k2.x, k3.x, k4.x);
  p.y = pt_rk4_sum(p.y, dt, k1.y, k2.y, k3.y, k4.y);
  p.k = pt_rk4_sum(p.k, dt, k1.k, k2.k, k3.k, k4.k);
  p.l = pt_rk4_sum(p.l, dt, k1.l, k2.l, k3.l, k4.l);
}
// fused contexts: positions and wavevectors in four arrays, zeta in real planes
__global__ void __launch_bounds__(256) k_pt_rk4_r(double* __restrict__ px, double* __restrict__ py, double* __restrict__ pk,
                                                  double* __restrict__ pl, int n, const cd* U0, const cd* U1, const double* Z0,
                                                  const double* Z1, PtGrid g, double Ub, double eta, double dt) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    PtRay p = {px[i], py[i], pk[i], pl[i]};
    pt_rk4_ray(U0, U1, Z0, Z1, g, Ub, eta, dt, p);
    px[i] = p.x;
    py[i] = p.y;
    pk[i] = p.k;
    pl[i] = p.l;
  }
}
// any-size engine: pos = x + i y and wv = k + i l, zeta in the real part of complex planes (every engine plane is complex)
__global__ void __launch_bounds__(256) k_pt_rk4_rc(cd* __restrict__ pos, cd* __restrict__ wv, int n, const cd* U0, const cd* U1,
                                                   const cd* Z0, const cd* Z1, PtGrid g, double Ub, double eta, double dt) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    PtRay p = {pos[i].x, pos[i].y, wv[i].x, wv[i].y};
    pt_rk4_ray(U0, U1, Z0, Z1, g, Ub, eta, dt, p);
    pos[i] = make_double2(p.x, p.y);
    wv[i] = make_double2(p.k, p.l);
  }
}
// omega at the rays from the current state: (Ub + u) k + v l + zeta / 2 + (eta / 2) (k^2 + l^2), in this order of operations
__device__ __forceinline__ double pt_omega(double u, double v, double zeta, double k, double l, double Ub, double eta) {
  return (((u + Ub) * k + v * l) + 0.5 * zeta) + 0.5 * eta * (k * k + l * l);
}
__global__ void __launch_bounds__(256) k_pt_omega(const cd* __restrict__ U, const double* __restrict__ Z, const double* __restrict__ px,
                                                  const double* __restrict__ py, const double* __restrict__ pk,
                                                  const double* __restrict__ pl, int n, PtGrid g, double Ub, double eta,
                                                  double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const PtStencil s = pt_stencil(g, px[i], py[i]);
    const cd uv = pt_gather(U, g, s);
    out[i] = pt_omega(uv.x, uv.y, pt_gather(Z, g, s), pk[i], pl[i], Ub, eta);
  }
}
// any-size engine: out[i] = omega + 0 i from pos, wv, the velocity plane and the zeta plane (real part)
__global__ void __launch_bounds__(256) k_pt_omega_c(cd* __restrict__ out, const cd* __restrict__ U, const cd* __restrict__ Z,
                                                    const cd* __restrict__ pos, const cd* __restrict__ wv, int n, PtGrid g, double Ub,
                                                    double eta) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const PtStencil s = pt_stencil(g, pos[i].x, pos[i].y);
    const cd uv = pt_gather(U, g, s);
    out[i] = make_double2(pt_omega(uv.x, uv.y, pt_gather(Z, g, s).x, wv[i].x, wv[i].y, Ub, eta), 0.0);
  }
}

// ---- stretch mode: each particle carries the deformation gradient F = d x(t) / d x0 ----------------------
// dF/dt = A F with A = [[u_x, u_y], [v_x, v_y]] at the particle, the gradients of the one interpolant (pt_gather_d: the same 16
// nodes).  (x, y, f11, f12, f21, f22) take ONE classical RK4 step with the particles' time treatment, the F stages from the stage
// values of F: a Runge-Kutta step commutes with differentiation, so the new F is the exact Jacobian of the discrete position map
// (times the old F).  WAVE: drifter mode's velocity, a phi e^{-i f0 t} and ITS gradient added (the compressible case).
struct PtTan {
  double x, y, f11, f12, f21, f22;
};
template <bool WAVE>
__device__ __forceinline__ PtTan pt_tan_rhs(const cd* __restrict__ U0, const cd* __restrict__ U1, const cd* __restrict__ P0,
                                            const cd* __restrict__ P1, const PtGrid& g, const PtTan& p, int st, double Ub,
                                            const PtWave& wv) {
  const PtStencilD s = pt_stencil_d(g, p.x, p.y);
  const PtJet<cd> U = pt_jet_at(U0, U1, g, s, st);
  double u = U.f.x + Ub, v = U.f.y, ux = U.fx.x, vx = U.fx.y, uy = U.fy.x, vy = U.fy.y;
  if constexpr (WAVE) {
    const PtJet<cd> W = pt_jet_at(P0, P1, g, s, st);
    const cd w = pt_wave_vel(W.f, wv.a, wv.c[st], wv.s[st]);
    const cd wx = pt_wave_vel(W.fx, wv.a, wv.c[st], wv.s[st]), wy = pt_wave_vel(W.fy, wv.a, wv.c[st], wv.s[st]);
    u += w.x;
    v += w.y;
    ux += wx.x;
    vx += wx.y;
    uy += wy.x;
    vy += wy.y;
  }
  PtTan d;
  d.x = u;
  d.y = v;
  d.f11 = ux * p.f11 + uy * p.f21;
  d.f12 = ux * p.f12 + uy * p.f22;
  d.f21 = vx * p.f11 + vy * p.f21;
  d.f22 = vx * p.f12 + vy * p.f22;
  return d;
}
__device__ __forceinline__ PtTan pt_tan_at(const PtTan& p, double h, const PtTan& d) {
  PtTan q;
  q.x = p.x + h * d.x;
  q.y = p.y + h * d.y;
  q.f11 = p.f11 + h * d.f11;
  q.f12 = p.f12 + h * d.f12;
  q.f21 = p.f21 + h * d.f21;
  q.f22 = p.f22 + h * d.f22;
  return q;
}
// acc += w d: the RK4 sum k1 + 2 k2 + 2 k3 + k4 formed as the stages arrive, in pt_rk4_sum's order, so that only the state, the
// running sum and one stage are live at a time
__device__ __forceinline__ void pt_tan_acc(PtTan& a, double w, const PtTan& d) {
  a.x += w * d.x;
  a.y += w * d.y;
  a.f11 += w * d.f11;
  a.f12 += w * d.f12;
  a.f21 += w * d.f21;
  a.f22 += w * d.f22;
}
template <bool WAVE>
__device__ __forceinline__ void pt_rk4_tan(const cd* __restrict__ U0, const cd* __restrict__ U1, const cd* __restrict__ P0,
                                           const cd* __restrict__ P1, const PtGrid& g, double Ub, double dt, const PtWave& wv, PtTan& p) {
  const double h = 0.5 * dt;
  PtTan k = pt_tan_rhs<WAVE>(U0, U1, P0, P1, g, p, 0, Ub, wv);
  PtTan acc = k;
  k = pt_tan_rhs<WAVE>(U0, U1, P0, P1, g, pt_tan_at(p, h, k), 1, Ub, wv);
  pt_tan_acc(acc, 2.0, k);
  k = pt_tan_rhs<WAVE>(U0, U1, P0, P1, g, pt_tan_at(p, h, k), 1, Ub, wv);
  pt_tan_acc(acc, 2.0, k);
  k = pt_tan_rhs<WAVE>(U0, U1, P0, P1, g, pt_tan_at(p, dt, k), 2, Ub, wv);
  pt_tan_acc(acc, 1.0, k);
  p = pt_tan_at(p, dt / 6.0, acc);
}
// fused contexts: positions in two arrays, F in four arrays of n doubles (f11, f12, f21, f22)
template <bool WAVE>
__device__ __forceinline__ void pt_rk4_tan_arrays(double* __restrict__ px, double* __restrict__ py, double* __restrict__ f11,
                                                  double* __restrict__ f12, double* __restrict__ f21, double* __restrict__ f22, int n,
                                                  const cd* U0, const cd* U1, const cd* P0, const cd* P1, const PtGrid& g, double Ub,
                                                  double dt, const PtWave& wv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    PtTan p = {px[i], py[i], f11[i], f12[i], f21[i], f22[i]};
    pt_rk4_tan<WAVE>(U0, U1, P0, P1, g, Ub, dt, wv, p);
    px[i] = p.x;
    py[i] = p.y;
    f11[i] = p.f11;
    f12[i] = p.f12;
    f21[i] = p.f21;
    f22[i] = p.f22;
  }
}
__global__ void __launch_bounds__(256) k_pt_rk4_t(double* __restrict__ px, double* __restrict__ py, double* __restrict__ f11,
                                                  double* __restrict__ f12, double* __restrict__ f21, double* __restrict__ f22, int n,
                                                  const cd* U0, const cd* U1, PtGrid g, double Ub, double dt) {
  pt_rk4_tan_arrays<false>(px, py, f11, f12, f21, f22, n, U0, U1, nullptr, nullptr, g, Ub, dt, PtWave());
}
__global__ void __launch_bounds__(256) k_pt_rk4_wt(double* __restrict__ px, double* __restrict__ py, double* __restrict__ f11,
                                                   double* __restrict__ f12, double* __restrict__ f21, double* __restrict__ f22, int n,
                                                   const cd* U0, const cd* U1, const cd* P0, const cd* P1, PtGrid g, double Ub, double dt,
                                                   PtWave wv) {
  pt_rk4_tan_arrays<true>(px, py, f11, f12, f21, f22, n, U0, U1, P0, P1, g, Ub, dt, wv);
}
// any-size engine: pos = x + i y and the columns of F as two complex arrays, fa = f11 + i f21, fb = f12 + i f22
template <bool WAVE>
__device__ __forceinline__ void pt_rk4_tan_planes(cd* __restrict__ pos, cd* __restrict__ fa, cd* __restrict__ fb, int n, const cd* U0,
                                                  const cd* U1, const cd* P0, const cd* P1, const PtGrid& g, double Ub, double dt,
                                                  const PtWave& wv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    PtTan p = {pos[i].x, pos[i].y, fa[i].x, fb[i].x, fa[i].y, fb[i].y};
    pt_rk4_tan<WAVE>(U0, U1, P0, P1, g, Ub, dt, wv, p);
    pos[i] = make_double2(p.x, p.y);
    fa[i] = make_double2(p.f11, p.f21);
    fb[i] = make_double2(p.f12, p.f22);
  }
}
__global__ void __launch_bounds__(256) k_pt_rk4_tc(cd* __restrict__ pos, cd* __restrict__ fa, cd* __restrict__ fb, int n, const cd* U0,
                                                   const cd* U1, PtGrid g, double Ub, double dt) {
  pt_rk4_tan_planes<false>(pos, fa, fb, n, U0, U1, nullptr, nullptr, g, Ub, dt, PtWave());
}
__global__ void __launch_bounds__(256) k_pt_rk4_wtc(cd* __restrict__ pos, cd* __restrict__ fa, cd* __restrict__ fb, int n, const cd* U0,
                                                    const cd* U1, const cd* P0, const cd* P1, PtGrid g, double Ub, double dt, PtWave wv) {
  pt_rk4_tan_planes<true>(pos, fa, fb, n, U0, U1, P0, P1, g, Ub, dt, wv);
}
// ln of the largest singular value of F, written with no cancellation near F = I:
//   s = ((f11^2 + f12^2) + f21^2) + f22^2,   p = ((f11 - f22)^2 + (f12 + f21)^2) ((f11 + f22)^2 + (f21 - f12)^2) = s^2 - 4 det^2,
//   ln sigma_1 = 1/2 ln(1/2 (s + sqrt p)),
// in this order of operations and with every product rounded on its own (no contraction), as particles.ln_sigma restates it
__host__ __device__ inline double pt_ln_sigma(double f11, double f12, double f21, double f22) {
#pragma clang fp contract(off)
  const double s = ((f11 * f11 + f12 * f12) + f21 * f21) + f22 * f22;
  const double a = f11 - f22, b = f12 + f21, c = f11 + f22, d = f21 - f12;
  const double p = (a * a + b * b) * (c * c + d * d);
  return 0.5 * log(0.5 * (s + sqrt(p)));
}
// det F = f11 f22 - f12 f21, each product rounded on its own
__host__ __device__ inline double pt_det(double f11, double f12, double f21, double f22) {
#pragma clang fp contract(off)
  return f11 * f22 - f12 * f21;
}
// "lnsigma" (which == 0) or "det" (1) of F at every particle; the entries of F are `stride` doubles apart (fused arrays: 1; the
// engine's complex arrays: 2, with f21 = f11 + 1 and f22 = f12 + 1), out likewise `ostride` apart
__global__ void __launch_bounds__(256) k_pt_tan_value(const double* __restrict__ f11, const double* __restrict__ f12,
                                                      const double* __restrict__ f21, const double* __restrict__ f22, int stride, int n,
                                                      int which, double* __restrict__ out, int ostride) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const size_t at = (size_t)i * stride;
    const double a = f11[at], b = f12[at], c = f21[at], d = f22[at];
    out[(size_t)i * ostride] = which == 0 ? pt_ln_sigma(a, b, c, d) : pt_det(a, b, c, d);
    if (ostride == 2) out[(size_t)i * 2 + 1] = 0.0;
  }
}
// F = I at every particle (nq_particles_tangent with no F0, nq_particles_tangent_reset)
__global__ void __launch_bounds__(256) k_pt_tan_identity(double* __restrict__ f11, double* __restrict__ f12, double* __restrict__ f21,
                                                         double* __restrict__ f22, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    f11[i] = 1.0;
    f12[i] = 0.0;
    f21[i] = 0.0;
    f22[i] = 1.0;
  }
}

// values of a physical plane at the particles: T = double (out0), T = cd (out0 = real part, out1 = imaginary part; either may be
// null)
template <typename T>
__device__ __forceinline__ void pt_store(const T& v, double* o0, double* o1, int i);
template <>
__device__ __forceinline__ void pt_store<double>(const double& v, double* o0, double* o1, int i) { (void)o1; o0[i] = v; }
template <>
__device__ __forceinline__ void pt_store<cd>(const cd& v, double* o0, double* o1, int i) {
  if (o0) o0[i] = v.x;
  if (o1) o1[i] = v.y;
}
template <typename T>
__global__ void __launch_bounds__(256) k_pt_sample(const T* __restrict__ plane, const double* __restrict__ px,
                                                   const double* __restrict__ py, int n, PtGrid g, double* o0, double* o1) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    pt_store<T>(pt_gather(plane, g, pt_stencil(g, px[i], py[i])), o0, o1, i);
}
// any-size engine: out[i] = the complex plane interpolated at pos[i] = x + i y (real and imaginary parts each)
__global__ void __launch_bounds__(256) k_pt_interp_c(cd* __restrict__ out, const cd* __restrict__ plane, const cd* __restrict__ pos,
                                                     int n, PtGrid g) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = pt_gather(plane, g, pt_stencil(g, pos[i].x, pos[i].y));
}
// the wave velocity a phi e^{-i f0 t} at the particles ("uw": o0, "vw": o1; either may be null); (c, s) = e^{-i f0 t}
__global__ void __launch_bounds__(256) k_pt_sample_w(const cd* __restrict__ phi, const double* __restrict__ px,
                                                     const double* __restrict__ py, int n, PtGrid g, double a, double c, double s,
                                                     double* o0, double* o1) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    pt_store<cd>(pt_wave_vel(pt_gather(phi, g, pt_stencil(g, px[i], py[i])), a, c, s), o0, o1, i);
}
// any-size engine: out[i] = a phi(pos[i]) e^{-i f0 t}
__global__ void __launch_bounds__(256) k_pt_interp_wc(cd* __restrict__ out, const cd* __restrict__ phi, const cd* __restrict__ pos,
                                                      int n, PtGrid g, double a, double c, double s) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = pt_wave_vel(pt_gather(phi, g, pt_stencil(g, pos[i].x, pos[i].y)), a, c, s);
}

// the velocity plane (u, v) of the fields the last inversion emitted (Hu = column-transformed -il psi, Hp = psi on the x side):
// k_x_get_real's two finishes (u: mode 0; v: mode 1, i kk, column N/2 dropped for the Kernel family) of one row, written
// interleaved so that one gather fetches both components.  ONE = true (8192-point rows, where holding u across the second
// transform spills): one launch per component `comp`, each writing its half of the double2 elements.
template <int N, bool SLAB, bool ONE>
__global__ void __launch_bounds__(XPlan<N>::THREADS)
k_x_get_uv(MArr hu, MArr hp, cd* __restrict__ rows, int nrows, const cd* __restrict__ tw, const double* __restrict__ kk,
           int zero_nyq, int comp) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T;
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  const int row = blockIdx.x * X::C + c;
  cd* lds = reinterpret_cast<cd*>(nq_smem);
  typename X::F::Tw twr;
  X::F::load_tw(twr, j, tw, 1);
  cd r[P];
  double u[ONE ? 1 : P];
  const bool ok = row < nrows;
#pragma unroll
  for (int pass = 0; pass < (ONE ? 1 : 2); ++pass) {
    const int which = ONE ? comp : pass;
    const XRowT<SLAB> src = xrow<SLAB>(which == 0 ? hu : hp, (size_t)(ok ? row : 0));
#pragma unroll
    for (int t = 0; t < P; ++t) {
      const int kx = j + t * T;
      cd v = cmake(0, 0);
      if (ok) {
        const int m = kx <= N / 2 ? kx : N - kx;
        v = *src.at(m);
        if (which == 1) v = cscale(cmul_i(v), kk[m]);
        if (m == 0 || m == N / 2) v.y = 0.0;
        if (which == 1 && zero_nyq && m == N / 2) v.x = 0.0;
        if (kx > N / 2) v = cconj(v);
      }
      r[t] = v;
    }
    if (pass == 1) __syncthreads();           // the first transform's last LDS reads are done before the second writes
    X::F::template run<true>(r, j, c, lds, twr);
    if (!ONE && pass == 0) {
#pragma unroll
      for (int t = 0; t < P; ++t) u[t] = r[t].x;
    }
  }
  if (ok) {
#pragma unroll
    for (int t = 0; t < P; ++t) {
      const size_t at = (size_t)row * N + j + t * T;
      if constexpr (ONE) reinterpret_cast<double*>(rows)[2 * at + comp] = r[t].x;
      else rows[at] = make_double2(u[ONE ? 0 : t], r[t].x);
    }
  }
}

// the zeta plane of ray mode (section 5t): q_psi of the state the last inversion saw, as x_row_values forms it from the (q, q_w)
// mixed-space rows (q - q_w on CoupledModel, q elsewhere), stored as an (N, N) plane of doubles.  One row block per workgroup, the
// grid of k_x_hist.
template <int N, int MODE, bool SLAB = false>
__global__ void __launch_bounds__(XPlan<N>::THREADS, XPlan<N>::MIN_WAVES)
k_x_get_zeta(MArr Mq, MArr Mqw, const cd* __restrict__ tw, const double* __restrict__ kk, double* __restrict__ zeta) {
  typedef XPlan<N> X;
  constexpr int P = X::P, T = X::T;
  double q[P], qpsi[P];
  cd w[P];
  x_row_values<N, MODE, SLAB, false>(Mq, Mqw, Mq, tw, kk, q, qpsi, w);
  const int j = threadIdx.x % T, c = threadIdx.x / T;
  double* __restrict__ out = zeta + ((size_t)blockIdx.x * X::C + c) * N + j;           // point t of the thread: out + t * T
#pragma unroll
  for (int t = 0; t < P; ++t) out[t * T] = qpsi[t];
}

}  // namespace nq
