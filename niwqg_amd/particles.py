"""Lagrangian particles advected on the device inside the step.

    from niwqg_amd import particles
    P = particles.attach(m, x, y, record_every=0, capacity=1024, record=(), wave=None, rays=None, eta=None, stretch=None)
    m.run()                                   # the particles move inside every step, batched or not
    x, y = P.positions()                      # unwrapped coordinates
    s = P.sample(("u", "v", "q", "phi"))      # {name: array(n)} at the current positions, from the current state
    tr = P.trajectory()                       # .step (T,), .t (T,), .x / .y (T, n), .values {name: (T, n)}
    P.detach()

A particle moves through U_tot = (m.U + u, v), u = -d psi/dy, v = d psi/dx of the psi-hat the model holds (``m.ph``): in the
coupled model the Lagrangian-mean flow; the wave signal is what ``"phi"`` records.  One step from t to t + dt is classical RK4,
linear in time between the velocity U0 of the state the step starts from and U1 of the state after it:

    k1 = U0(x), k2 = (U0 + U1)/2 (x + dt/2 k1), k3 = (U0 + U1)/2 (x + dt/2 k2), k4 = U1(x + dt k3)
    x += dt/6 (k1 + 2 k2 + 2 k3 + k4)

Values at a particle come from the periodic tensor-product cubic convolution (Keys, a = -1/2) on the 4 x 4 nearest nodes, grid
value [j, i] sitting at ((i + 1/2) dx, (j + 1/2) dy).  ``interpolate`` below is the same rule in numpy.  The particles write
only buffers of their own: every model output is bit-identical to a run without them.

Drifter mode: ``attach(..., wave=a)``, a finite real a > 0 -- the amplitude of the vertical mode at the
drifters' depth -- moves the particles through the whole velocity, as a surface drifter moves:

    (m.U + u, v) + a (Re, Im)[phi(x, y, t) e^{-i f0 t}]          (phi is back-rotated: u_w + i v_w = phi e^{-i f0 t}, f0 = m.f)

``wave=None`` is the step above, bit for bit, and allocates and launches nothing more.  The time of step s after attach is
t_s = t0 + s dt with t0 = m.t at attach and s counted by the particles themselves: not the accumulated float clock ``m.t``,
from which it differs by rounding only.  One step from t = t_s uses U0, U1 and Phi0, Phi1, the physical phi (``m.phi``) of the
state the step starts from and of the state after it (after the forcing's re-emission).  It is classical RK4 with the slow
envelope linear in time and the fast phase exact at the stage times:

    k1 = U0(x0)                 + a Phi0(x0)                      e^{-i f0 t}
    k2 = (U0+U1)/2 (x0+dt/2 k1) + a (Phi0+Phi1)/2 (x0+dt/2 k1)    e^{-i f0 (t+dt/2)}
    k3 = (U0+U1)/2 (x0+dt/2 k2) + a (Phi0+Phi1)/2 (x0+dt/2 k2)    e^{-i f0 (t+dt/2)}
    k4 = U1(x0+dt k3)           + a Phi1(x0+dt k3)                e^{-i f0 (t+dt)}
    x0 + dt/6 (k1 + 2 k2 + 2 k3 + k4)        k complex: x += Re, y += Im; m.U is added to the real part

The three phase factors are formed on the host in double precision at every step.  Each stage position has ONE stencil, shared
by the U and the phi gathers; a NaN coordinate stays NaN without a load, as above.  YBJModel: psi is steady (U1 = U0) but phi is
not, so Phi0, Phi1 are two planes.  Phi0 is formed again after ``set_phi`` (also on CoupledModel, where quirk Q2 leaves U0 as
it was), ``set_q`` and ``_invert``.  QGModel has no phi: ``wave=`` raises ValueError; slab-decomposed models are refused as
above.  ``rk4_wave`` below is one such step in numpy, in the kernel's operation order.

``"uw"``, ``"vw"`` in ``record=`` and ``sample()`` (Kernel family): a Re / Im [phi(x_p) e^{-i f0 t_s}] at the particle, the wave
velocity a drifter at that depth feels; without drifter mode a = 1.

Ray mode: ``attach(..., rays=(k0, l0), eta=None)``, two arrays of n finite wavenumbers -- every particle
is a near-inertial wave packet and carries its wavevector.  With eta = f / kappa^2 (default ``m.hslash``) and zeta = q_psi, the
YBJ operator of this package has omega = (m.U + u) k + v l + zeta/2 + (eta/2)(k^2 + l^2), and the rays are its Hamilton's equations

    dx/dt = m.U + u + eta k     dy/dt = v + eta l     dk/dt = -(k u_x + l v_x) - zeta_x/2     dl/dt = -(k u_y + l v_y) - zeta_y/2

advanced by one classical RK4 step after every model step, with the time treatment of the particles (U0, Z0 at the start, U1, Z1
after the step, linear in between).  u, v, zeta and their gradients come from ONE interpolant: the gradients are the analytic
derivative of the Keys interpolant (``keys_dweights``), so the discrete rays are Hamilton's equations of the interpolated omega
exactly; on a steady flow its drift measures the time stepping alone (second order at best: w'' jumps at cell faces).  zeta is
q_psi = q - q_w of the state the last inversion saw, ``ifft2(-wv2 * m.ph).real + m.q.mean()``; a bare ``set_phi`` on CoupledModel
(quirk Q2) inverts nothing and leaves zeta, like U0, what it was.  ``rays`` and ``wave`` exclude each other; QGModel raises
ValueError, slab-decomposed models NotImplementedError.  ``P.wavevectors()`` returns (k, l); ``"k"``, ``"l"``, ``"omega"`` (ray mode)
and ``"zeta"`` (any mode) are names of ``record=`` and ``sample()``.  ``rk4_rays`` is one step in numpy, ``ray_omega`` the omega.
``rays=None`` is the step of the first paragraph, bit for bit.

Stretch mode: ``attach(..., stretch=True)`` (or an (n, 2, 2) array, the starting F) -- every particle carries
the deformation gradient F = d x(t) / d x0 of its own trajectory, dF/dt = A F with A = [[u_x, u_y], [v_x, v_y]] at the particle.
The six values (x, y, f11, f12, f21, f22) take ONE classical RK4 step, with the time treatment above and the F stages from the
stage values of F.  A is the analytic derivative of the Keys interpolant on the 16 nodes that give (u, v), and a Runge-Kutta step
commutes with differentiation, so F is the exact Jacobian of the discrete map the positions follow, not an approximation beside
it: central differences of neighbouring runs converge to it.  (The interpolated velocity is solenoidal to second order only:
det F - 1 = O(dx^2).)  With ``wave=a`` A gains the gradient of a phi e^{-i f0 t}: the drifter velocity is compressible and det F
measures clustering.  Every model class, QGModel included; ``rays=`` with ``stretch`` raises ValueError (the ray map lives in four
dimensions), slab-decomposed models NotImplementedError.  ``P.deformation()`` returns (n, 2, 2); ``P.reset_deformation()`` makes
F = I on the device (renormalise before F overflows: overflow itself is loud, inf then NaN) and ``P.stretch_step0`` is the particle
step count at which F was last set.  ``"f11"``, ``"f12"``, ``"f21"``, ``"f22"``, ``"lnsigma"`` (ln of the largest singular value:
``ln_sigma``) and ``"det"`` are names of ``record=`` and ``sample()``.  ``rk4_tangent`` is one step in numpy; ``lattice(m, n)`` places
n x n particles so that ``lagrangian.ftle(P).reshape(n, n)`` is a map.  ``stretch=None`` runs the kernels of the other paragraphs.
"""
import ctypes

import numpy as np

from . import _attach, _lib

FIELDS = ("u", "v", "q", "phi")                                          # the fields of the state
NAMES = FIELDS + ("uw", "vw")                                            # and the wave velocity at the particle (section 5s)
RAY_NAMES = ("zeta", "k", "l", "omega")                                  # q_psi at the particle; the ray's own (section 5t)
_NEED_RAYS = ("k", "l", "omega")                                         # names only ray mode has
_CODES = dict(u=0, v=1, q=2, phi=3, uw=_lib.PT_UW, vw=_lib.PT_VW)        # the new codes: include/niwqg_amd.h
# nq_lagr_spectrum's names: the columns, and the composites u + i v, uw + i vw, (u + uw) + i (v + vw)
_LAGR_CODES = dict(_CODES, uv=4, uvw=_lib.LAGR_UVW, uvt=_lib.LAGR_UVT)
_CODES.update(k=_lib.PT_K, l=_lib.PT_L, zeta=_lib.PT_ZETA, omega=_lib.PT_OMEGA)
STRETCH_NAMES = ("f11", "f12", "f21", "f22", "lnsigma", "det")           # stretch mode's own (section 5u), every model class
_CODES.update(f11=_lib.PT_F11, f12=_lib.PT_F12, f21=_lib.PT_F21, f22=_lib.PT_F22, lnsigma=_lib.PT_LNSIGMA, det=_lib.PT_DET)


def _is_qg(m):
    from .QGModel import Model as QG
    return isinstance(m, QG)


def available(m, wave=False, rays=False, stretch=False):
    """names ``record`` and ``sample`` accept for this model: the fields of the state ("phi": the Kernel family only), which
    ``sample()`` returns by default, with ``wave=True`` also the wave velocity columns "uw", "vw" and with ``rays=True`` "zeta" and
    the ray's "k", "l", "omega" (Kernel family only; the last three in ray mode); with ``stretch=True`` the entries of F, "lnsigma"
    and "det" (every model class; in stretch mode)"""
    tail = list(STRETCH_NAMES) if stretch else []
    if _is_qg(m):
        return ["u", "v", "q"] + tail
    return (list(NAMES) if wave else list(FIELDS)) + (list(RAY_NAMES) if rays else []) + tail


def _names(m, names, what, rays=True, stretch=True):
    """the names as a list, checked; rays=False: the particles are not in ray mode; stretch=False: not in stretch mode"""
    names = [names] if isinstance(names, str) else list(names)
    valid = available(m, wave=True, rays=True)
    bad = [n for n in names if n not in valid and n not in STRETCH_NAMES]
    if bad:                                       # (the names of stretch mode come first: the list of the state's names ends the text)
        raise ValueError("particles.%s: %s not available for %s; stretch mode adds %s; valid names: %s"
                         % (what, ", ".join(map(repr, bad)), type(m).__name__, ", ".join(STRETCH_NAMES), ", ".join(valid)))
    bad = [n for n in names if n in _NEED_RAYS and not rays]
    if bad:
        raise ValueError("particles.%s: %s need ray mode (attach(..., rays=(k0, l0)))" % (what, ", ".join(map(repr, bad))))
    bad = [n for n in names if n in STRETCH_NAMES and not stretch]
    if bad:
        raise ValueError("particles.%s: %s need stretch mode (attach(..., stretch=True))" % (what, ", ".join(map(repr, bad))))
    return names


def _coords(x, y):
    x = np.asarray(x)
    y = np.asarray(y)
    if x.ndim != 1 or y.ndim != 1:
        raise ValueError("particles.attach: x and y must be 1-D (got %d-D and %d-D)" % (x.ndim, y.ndim))
    if x.shape != y.shape:
        raise ValueError("particles.attach: x and y differ in length (%d, %d)" % (x.size, y.size))
    if x.size < 1:
        raise ValueError("particles.attach: no particles (x and y are empty)")
    try:
        x = np.array(x, np.float64)
        y = np.array(y, np.float64)
    except (TypeError, ValueError):
        raise ValueError("particles.attach: x and y must be real numbers")
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("particles.attach: non-finite coordinates")
    return x, y


# ---- the interpolation rule in numpy (the device kernels' restatement; tests use it) --------------------------------------
def keys_weights(t):
    """Keys' cubic convolution weights (a = -1/2) of the nodes at offsets -1, 0, 1, 2; t in [0, 1)"""
    t = np.asarray(t, np.float64)
    return (((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t)


def _axis(x, L, n):
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x)
    xs = np.where(ok, x, 0.0)
    r = np.fmod(xs, L)
    r = np.where(r < 0, r + L, r)
    r = np.where(r >= L, r - L, r)
    s = r / (L / n) - 0.5
    f = np.floor(s)
    i0 = f.astype(np.int64)
    w = keys_weights(s - f)
    idx = [np.mod(i0 - 1 + o, n) for o in range(4)]
    return ok, idx, w


def interpolate(plane, x, y, L, W=None):
    """plane (n, n) (real or complex) at the points (x, y): the library's rule; NaN for non-finite points"""
    plane = np.asarray(plane)
    n = plane.shape[0]
    W = L if W is None else W
    okx, ix, wx = _axis(x, L, n)
    oky, iy, wy = _axis(y, W, n)
    acc = np.zeros(np.shape(x), plane.dtype)
    for j in range(4):
        r = np.zeros(np.shape(x), plane.dtype)
        for i in range(4):
            r = r + wx[i] * plane[iy[j], ix[i]]
        acc = acc + wy[j] * r
    return np.where(okx & oky, acc, np.nan)


def _uv_plane(U):
    """a velocity plane as u + i v: a complex plane, or the pair (u, v)"""
    U = np.asarray(U)
    if U.ndim == 3:
        return U[0].astype(np.float64) + 1j * U[1].astype(np.float64)
    return U.astype(np.complex128)


def wave_phase(f0, t):
    """e^{-i f0 t} as the library forms it: (cos(f0 t), -sin(f0 t)) in double precision"""
    return np.cos(f0 * t), -np.sin(f0 * t)


def wave_velocity(phi, a, f0, t):
    """a phi e^{-i f0 t}, complex (uw + i vw), in the operation order of the kernels (what "uw" and "vw" record)"""
    c, s = wave_phase(f0, t)
    phi = np.asarray(phi)
    return a * (phi.real * c - phi.imag * s) + 1j * (a * (phi.real * s + phi.imag * c))


def rk4_wave(x, y, U0, U1, P0, P1, Ub, a, f0, t, dt, L):
    """One drifter step from t to t + dt in numpy, in the operation order of the kernel (k_pt_rk4_w): U0, U1 the velocity planes
    u + i v (or pairs (u, v)) and P0, P1 the physical phi of the state the step starts from and of the state after it; returns the
    new (x, y).  With a = 0 it is the step of ``wave=None``."""
    A0, A1 = _uv_plane(U0), _uv_plane(U1)
    P0, P1 = np.asarray(P0, np.complex128), np.asarray(P1, np.complex128)
    steady = U0 is U1

    def vel(px, py, st):
        if st == 0:
            v, w = interpolate(A0, px, py, L), interpolate(P0, px, py, L)
        elif st == 2:
            v, w = interpolate(A1, px, py, L), interpolate(P1, px, py, L)
        else:
            v = interpolate(A0, px, py, L)
            if not steady:
                v = 0.5 * (v + interpolate(A1, px, py, L))
            w = 0.5 * (interpolate(P0, px, py, L) + interpolate(P1, px, py, L))
        ww = wave_velocity(w, a, f0, (t, t + 0.5 * dt, t + dt)[st])
        return (v.real + Ub) + ww.real, v.imag + ww.imag
    h = 0.5 * dt
    k1 = vel(x, y, 0)
    k2 = vel(x + h * k1[0], y + h * k1[1], 1)
    k3 = vel(x + h * k2[0], y + h * k2[1], 1)
    k4 = vel(x + dt * k3[0], y + dt * k3[1], 2)
    return (x + dt / 6.0 * (k1[0] + 2.0 * k2[0] + 2.0 * k3[0] + k4[0]), y + dt / 6.0 * (k1[1] + 2.0 * k2[1] + 2.0 * k3[1] + k4[1]))


# ---- ray mode in numpy (section 5t): the kernels' restatement, in their order of sums ---------------------------------------
def keys_dweights(t):
    """d/dt of ``keys_weights``: the derivative weights of the nodes at offsets -1, 0, 1, 2 (they sum to 0; sum o_i w'_i = 1)"""
    t = np.asarray(t, np.float64)
    return ((-1.5 * t + 2.0) * t - 0.5, (4.5 * t - 5.0) * t, (-4.5 * t + 4.0) * t + 0.5, (1.5 * t - 1.0) * t)


def _axis_d(x, L, n):
    """_axis with the derivative weights w'(t) / d beside the weights"""
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x)
    xs = np.where(ok, x, 0.0)
    r = np.fmod(xs, L)
    r = np.where(r < 0, r + L, r)
    r = np.where(r >= L, r - L, r)
    d = L / n
    s = r / d - 0.5
    f = np.floor(s)
    i0 = f.astype(np.int64)
    w = keys_weights(s - f)
    dw = [v / d for v in keys_dweights(s - f)]
    idx = [np.mod(i0 - 1 + o, n) for o in range(4)]
    return ok, idx, w, dw


def interpolate_d(plane, x, y, L, W=None):
    """(f, df/dx, df/dy) of the Keys interpolant of plane (n, n) at the points (x, y): the three contractions of the 16 nodes with
    w (x) w, w' (x) w and w (x) w', the row sums first (the order of pt_gather_d); NaN for non-finite points"""
    plane = np.asarray(plane)
    n = plane.shape[0]
    W = L if W is None else W
    okx, ix, wx, dwx = _axis_d(x, L, n)
    oky, iy, wy, dwy = _axis_d(y, W, n)
    f = np.zeros(np.shape(x), plane.dtype)
    fx, fy = f.copy(), f.copy()
    for j in range(4):
        r = np.zeros(np.shape(x), plane.dtype)
        rd = r.copy()
        for i in range(4):
            v = plane[iy[j], ix[i]]
            r = r + wx[i] * v
            rd = rd + dwx[i] * v
        f = f + wy[j] * r
        fx = fx + wy[j] * rd
        fy = fy + dwy[j] * r
    ok = okx & oky
    return np.where(ok, f, np.nan), np.where(ok, fx, np.nan), np.where(ok, fy, np.nan)


def ray_omega(u, v, zeta, k, l, Ub, eta):
    """omega = (Ub + u) k + v l + zeta/2 + (eta/2)(k^2 + l^2) of values at the rays, in the operation order of the kernel (what
    "omega" records, from the "u", "v", "zeta", "k", "l" of the same record)"""
    u, v, zeta, k, l = (np.asarray(a, np.float64) for a in (u, v, zeta, k, l))
    return (((u + Ub) * k + v * l) + 0.5 * zeta) + 0.5 * eta * (k * k + l * l)


def ray_omega_at(x, y, k, l, U, Z, Ub, eta, L):
    """``ray_omega`` with u, v, zeta interpolated from the velocity plane U (u + i v, or the pair (u, v)) and the zeta plane Z"""
    uv = interpolate(_uv_plane(U), x, y, L)
    return ray_omega(uv.real, uv.imag, interpolate(np.asarray(Z, np.float64), x, y, L), k, l, Ub, eta)


def rk4_rays(x, y, k, l, U0, U1, Z0, Z1, Ub, eta, dt, L):
    """One step of the rays from t to t + dt in numpy, in the operation order of the kernel (k_pt_rk4_r): U0, U1 the velocity planes
    u + i v (or pairs (u, v)) and Z0, Z1 the zeta planes of the state the step starts from and of the state after it (``U0 is U1``,
    ``Z0 is Z1``: steady, one gather per stage); returns the new (x, y, k, l)."""
    A0, A1 = _uv_plane(U0), _uv_plane(U1)
    B0, B1 = np.asarray(Z0, np.float64), np.asarray(Z1, np.float64)
    steady_u, steady_z = U0 is U1, Z0 is Z1

    def jet(P0, P1, steady, px, py, st):
        if st == 0 or steady:
            return interpolate_d(P0, px, py, L)
        if st == 2:
            return interpolate_d(P1, px, py, L)
        a, b = interpolate_d(P0, px, py, L), interpolate_d(P1, px, py, L)
        return tuple(0.5 * (p + q) for p, q in zip(a, b))

    def rhs(p, st):
        px, py, pk, pl = p
        U, Ux, Uy = jet(A0, A1, steady_u, px, py, st)
        _, zx, zy = jet(B0, B1, steady_z, px, py, st)
        return ((U.real + Ub) + eta * pk, U.imag + eta * pl,
                -(pk * Ux.real + pl * Ux.imag) - 0.5 * zx, -(pk * Uy.real + pl * Uy.imag) - 0.5 * zy)

    def at(p, h, d):
        return tuple(a + h * b for a, b in zip(p, d))
    p = tuple(np.asarray(a, np.float64) for a in (x, y, k, l))
    h = 0.5 * dt
    k1 = rhs(p, 0)
    k2 = rhs(at(p, h, k1), 1)
    k3 = rhs(at(p, h, k2), 1)
    k4 = rhs(at(p, dt, k3), 2)
    return tuple(a + dt / 6.0 * (d1 + 2.0 * d2 + 2.0 * d3 + d4) for a, d1, d2, d3, d4 in zip(p, k1, k2, k3, k4))


# ---- stretch mode in numpy (section 5u): the kernels' restatement, in their order of sums ------------------------------------
def ln_sigma(F):
    """ln of the largest singular value of F (..., 2, 2), in the library's order of operations (pt_ln_sigma; what "lnsigma" records),
    written with no cancellation near F = I:  s = ((f11^2 + f12^2) + f21^2) + f22^2,
    p = ((f11 - f22)^2 + (f12 + f21)^2) ((f11 + f22)^2 + (f21 - f12)^2) = s^2 - 4 det^2,  ln sigma_1 = 1/2 ln(1/2 (s + sqrt p))"""
    F = np.asarray(F, np.float64)
    f11, f12, f21, f22 = F[..., 0, 0], F[..., 0, 1], F[..., 1, 0], F[..., 1, 1]
    s = ((f11 * f11 + f12 * f12) + f21 * f21) + f22 * f22
    a, b, c, d = f11 - f22, f12 + f21, f11 + f22, f21 - f12
    p = (a * a + b * b) * (c * c + d * d)
    return 0.5 * np.log(0.5 * (s + np.sqrt(p)))


def det(F):
    """det F of F (..., 2, 2) as the library forms it (what "det" records): f11 f22 - f12 f21"""
    F = np.asarray(F, np.float64)
    return F[..., 0, 0] * F[..., 1, 1] - F[..., 0, 1] * F[..., 1, 0]


def rk4_tangent(x, y, F, U0, U1, Ub, dt, L, P0=None, P1=None, a=0.0, f0=0.0, t=0.0):
    """One step of stretch mode from t to t + dt in numpy, in the operation order of the kernels (k_pt_rk4_t; with P0, P1 and a != 0
    k_pt_rk4_wt): U0, U1 the velocity planes u + i v (or pairs (u, v)) of the state the step starts from and of the state after it
    (``U0 is U1``: steady, one gather per stage), P0, P1 the physical phi likewise, F (n, 2, 2); returns the new (x, y, F)."""
    A0, A1 = _uv_plane(U0), _uv_plane(U1)
    steady = U0 is U1
    wave = P0 is not None and a != 0.0
    if wave:
        P0, P1, steady_p = np.asarray(P0, np.complex128), np.asarray(P1, np.complex128), P0 is P1

    def jet(B0, B1, same, px, py, st):
        if st == 0 or same:
            return interpolate_d(B0, px, py, L)
        if st == 2:
            return interpolate_d(B1, px, py, L)
        p, q = interpolate_d(B0, px, py, L), interpolate_d(B1, px, py, L)
        return tuple(0.5 * (v + w) for v, w in zip(p, q))

    def rhs(p, st):
        px, py, f11, f12, f21, f22 = p
        U, Ux, Uy = jet(A0, A1, steady, px, py, st)
        u, v, ux, vx, uy, vy = U.real + Ub, U.imag, Ux.real, Ux.imag, Uy.real, Uy.imag
        if wave:
            ts = (t, t + 0.5 * dt, t + dt)[st]
            W, Wx, Wy = (wave_velocity(w, a, f0, ts) for w in jet(P0, P1, steady_p, px, py, st))
            u, v, ux, vx, uy, vy = u + W.real, v + W.imag, ux + Wx.real, vx + Wx.imag, uy + Wy.real, vy + Wy.imag
        return (u, v, ux * f11 + uy * f21, ux * f12 + uy * f22, vx * f11 + vy * f21, vx * f12 + vy * f22)

    def at(p, h, d):
        return tuple(v + h * w for v, w in zip(p, d))
    F = np.asarray(F, np.float64)
    p = tuple(np.asarray(v, np.float64) for v in (x, y, F[:, 0, 0], F[:, 0, 1], F[:, 1, 0], F[:, 1, 1]))
    h = 0.5 * dt
    k1 = rhs(p, 0)
    k2 = rhs(at(p, h, k1), 1)
    k3 = rhs(at(p, h, k2), 1)
    k4 = rhs(at(p, dt, k3), 2)
    out = tuple(v + dt / 6.0 * (d1 + 2.0 * d2 + 2.0 * d3 + d4) for v, d1, d2, d3, d4 in zip(p, k1, k2, k3, k4))
    return out[0], out[1], np.stack([np.stack([out[2], out[3]], -1), np.stack([out[4], out[5]], -1)], -2)


def lattice(m, n):
    """(x, y) of an n x n lattice at the centres of n x n equal boxes of the domain of ``m``, flattened row-major (y the slow axis):
    a per-particle value v becomes a map as ``v.reshape(n, n)``, [j, i] at ((i + 1/2) L / n, (j + 1/2) W / n)"""
    if isinstance(n, bool) or int(n) != n or n < 1:
        raise ValueError("particles.lattice: n = %r (an integer >= 1)" % (n,))
    n = int(n)
    xs, ys = (np.arange(n) + 0.5) * (float(m.L) / n), (np.arange(n) + 0.5) * (float(m.W) / n)
    X, Y = np.meshgrid(xs, ys)
    return X.reshape(-1).copy(), Y.reshape(-1).copy()


# ---- the public object -------------------------------------------------------------------------------------------------
class Trajectory(object):
    """records oldest first: step (T,), t (T,), x, y (T, n), values {name: (T, n)}"""

    def __init__(self, step, t, x, y, values):
        self.step, self.t, self.x, self.y, self.values = step, t, x, y, values

    def __repr__(self):
        return "Trajectory(T=%d, n=%d, names=%s)" % (self.x.shape[0], self.x.shape[1], sorted(self.values))


class Particles(_attach.Attachment):
    """A particle set attached to one model (``attach``); see the module's doc"""
    SLOT, LABEL = "_particles", "particles"
    ALREADY = (RuntimeError, "particles.attach: this model has particles attached already (detach them first)")
    NO_SLAB = ("particles.attach: slab-decomposed models have no particles yet (they need the interpolation "
               "partials exchanged between the ranks at every stage; DESIGN.md section 7)")

    def __init__(self, m, n, record_every, capacity, record, wave=None, rays=None, eta=None, stretch=None):
        self.m, self.n = m, n
        self.stretch = stretch is not None        # stretch mode: on or off
        self.record_every, self.capacity, self.record = record_every, capacity, tuple(record)
        self.tc0, self.t0 = m.tc, m.t
        self.wave = wave                          # drifter mode: the amplitude a, or None
        self.rays, self.eta = rays is not None, eta       # ray mode: on or off, and eta = f / kappa^2 (None when off)

    def wavevectors(self):
        """(k, l): the wavevectors of the rays now (host copies; ray mode)"""
        self._check()
        if not self.rays:
            raise RuntimeError("particles.wavevectors: attached without rays=")
        return self._wavevectors()

    def deformation(self):
        """F (n, 2, 2): the deformation gradient of every particle now (a host copy; stretch mode)"""
        self._check()
        if not self.stretch:
            raise RuntimeError("particles.deformation: attached without stretch=")
        f = self._deformation()                   # (4, n): f11, f12, f21, f22
        return np.ascontiguousarray(f.T).reshape(self.n, 2, 2)

    def reset_deformation(self):
        """F = I on the device, now; no record is written.  ``stretch_step0`` moves to the present step count."""
        self._check()
        if not self.stretch:
            raise RuntimeError("particles.reset_deformation: attached without stretch=")
        self._reset_deformation()

    @property
    def stretch_step0(self):
        """the particle step count (steps since attach) at which F was last set: 0, or the count at the last reset"""
        self._check()
        if not self.stretch:
            raise RuntimeError("particles.stretch_step0: attached without stretch=")
        return self._stretch_step0()

    def wave_time(self, step):
        """t_s = t0 + s dt of step s after attach: the clock of the wave phase, counted by the particles"""
        return self.t0 + np.asarray(step, np.float64) * self.m.dt

    def positions(self):
        """(x, y): the unwrapped coordinates (host copies)"""
        self._check()
        return self._positions()

    def sample(self, names=None):
        """{name: array(n)} at the current positions from the current state ("phi": complex); names: a subset of
        available(m) (default: all of them)"""
        self._check()
        names = available(self.m) if names is None else _names(self.m, names, "sample", self.rays, self.stretch)
        return self._sample(names)

    def _times(self, offsets):
        t, out, k = self.t0, np.empty(len(offsets)), 0
        for i, s in enumerate(offsets):          # the reference's float clock t += dt, from the time of attach
            while k < s:
                t += self.m.dt
                k += 1
            out[i] = t
        return out

    def trajectory(self):
        """the last min(count, capacity) records, oldest first (record_every > 0)"""
        self._check()
        if self.record_every <= 0:
            raise RuntimeError("particles.trajectory: attached with record_every = 0")
        offsets, x, y, vals = self._records()
        order = np.argsort(offsets, kind="stable")
        assert np.all(order == np.arange(len(order)))
        return Trajectory(offsets + self.tc0, self._times(offsets), x, y, vals)

    @staticmethod
    def _split(names, cols):
        out, c = {}, 0
        for nm in names:
            if nm == "phi":
                out[nm] = cols[c] + 1j * cols[c + 1]
                c += 2
            else:
                out[nm] = cols[c]
                c += 1
        return out


class _Fused(Particles):
    """fused contexts: positions, velocity planes and records live in the library (nq_particles_*)"""

    def __init__(self, m, x, y, record_every, capacity, record, wave=None, rays=None, eta=None, stretch=None):
        Particles.__init__(self, m, len(x), record_every, capacity, record, wave, rays, eta, stretch)
        self.ctx = m._ctx
        self.ctx.particles_attach(x, y, m.L, m.W, record_every, capacity, [_CODES[r] for r in record])
        try:                                      # the clock of "uw" / "vw" (host values only) or, with it, drifter mode
            if not _is_qg(m):
                if wave is None:
                    self.ctx.particles_clock(m.f, m.t)
                else:
                    self.ctx.particles_wave(wave, m.f, m.t)
                if rays is not None:
                    self.ctx.particles_rays(rays[0], rays[1], eta)
            if stretch is not None:
                self.ctx.particles_tangent(None if stretch is True else stretch)
        except Exception:
            self.ctx.particles_detach()
            raise

    def _positions(self):
        return self.ctx.particles_get(self.n)

    def _wavevectors(self):
        return self.ctx.particles_get_rays(self.n)

    def _deformation(self):
        return self.ctx.particles_get_tangent(self.n)

    def _reset_deformation(self):
        self.ctx.particles_tangent_reset()

    def _stretch_step0(self):
        return self.ctx.particles_tangent_step0()

    def _lagr_stretching(self, T, G, order, offsets):
        return self.ctx.lagr_stretching(T, G, order, offsets)

    def _steps_now(self):
        return self.ctx.particles_steps()

    def _sample(self, names):
        ncols = sum(2 if nm == "phi" else 1 for nm in names)
        return self._split(names, self.ctx.particles_sample(self.n, [_CODES[nm] for nm in names], ncols))

    def _records(self):
        steps, out = self.ctx.particles_records(self.n)
        vals = self._split(self.record, [out[:, 2 + c, :] for c in range(out.shape[1] - 2)])
        return steps, out[:, 0, :].copy(), out[:, 1, :].copy(), vals

    # the device passes of lagrangian.py: the library reads its own ring
    def _held(self):
        return self.ctx.particles_held()

    def _record_steps(self):
        return self.ctx.particles_held(steps=True)

    def _lagr_spectrum(self, name, T, F, w, demean, G, order, offsets, chunk):
        return self.ctx.lagr_spectrum(_LAGR_CODES[name], T, F, w, demean, G, order, offsets, chunk)

    def _lagr_dispersion(self, T, G, order, offsets, pairs):
        return self.ctx.lagr_dispersion(T, G, order, offsets, pairs)

    def _detach(self):
        self.ctx.particles_detach()


class _AnySize(Particles):
    """any-size path: positions (x + i y), velocity planes (u + i v) and records are engine planes; the model's _step_etdrk4 calls
    _before_step / _after_step (nq_any_particles_rk4); U0, U1 are formed from m.ph with the Plane operations"""

    def __init__(self, m, x, y, record_every, capacity, record, wave=None, rays=None, eta=None, stretch=None):
        from ._anysize import Plane
        Particles.__init__(self, m, len(x), record_every, capacity, record, wave, rays, eta, stretch)
        self.eng = m._eng
        self.Fa = self.Fb = None            # the columns of F: f11 + i f21 and f12 + i f22 (stretch mode)
        self._step0 = self._count0 = 0      # steps since attach, and records written, when F was last set
        if self.stretch:
            one, zero = np.ones(len(x)), np.zeros(len(x))
            f = (one, zero, zero, one) if stretch is True else stretch
            self.Fa = self.eng.plane((f[0] + 1j * f[2]).reshape(1, -1), real=False)
            self.Fb = self.eng.plane((f[1] + 1j * f[3]).reshape(1, -1), real=False)
        self.pos = self.eng.plane((x + 1j * y).reshape(1, -1), real=False)
        self.U, self.src = None, None       # velocity plane of the state src (the psi-hat Plane it was formed from)
        self.Z, self.zsrc = None, None      # zeta plane (real part), likewise
        self.wv = self.eng.plane((rays[0] + 1j * rays[1]).reshape(1, -1), real=False) if self.rays else None
        self.rg = _attach.Ring(capacity if record_every > 0 else 0, record_every)
        self.ring = [None] * self.rg.cap
        self._Plane = Plane
        if record_every > 0:
            self._record()

    def _velocity(self):
        m = self.m
        d, K = m._d, m._K
        ph = d["ph"]
        if _is_qg(m):
            u, v = m._irfft(K["mil"] * ph), m._irfft(K["ik"] * ph)
        else:
            u, v = m._ifft(K["mil"] * ph).real, m._ifft(K["ik"] * ph).real
        return u + v * 1j, ph

    def _current_U(self):
        if self.U is None or self.src is not self.m._d["ph"]:
            self.U, self.src = self._velocity()
        return self.U

    def _current_Z(self):
        """q_psi of the state the last inversion saw: Re ifft2(-wv2 ph) + mean(q), formed again when ph is another Plane"""
        m = self.m
        d = m._d
        if self.Z is None or self.zsrc is not d["ph"]:
            self.Z, self.zsrc = m._ifft(m._K["mwv2"] * d["ph"]).real + d["q"].mean(), d["ph"]
        return self.Z

    def _interp_omega(self):
        e, m = self.eng, self.m
        out = self._Plane(e, (1, self.n))
        e.chk(e.L.nq_any_interp_omega(e.h, out.ptr, self._current_U().ptr, self._current_Z().ptr, self.pos.ptr, self.wv.ptr, self.n, m.nx,
                                      float(m.L), float(m.W), float(m.U), self.eta), "nq_any_interp_omega")
        return out

    def _tangent_plane(self, nm):
        """a column of stretch mode as a real plane; NaN without the mode (what the library records there)"""
        e = self.eng
        if not self.stretch:
            return e.plane(np.full((1, self.n), np.nan), real=True)
        if nm in ("lnsigma", "det"):
            out = self._Plane(e, (1, self.n), True)
            e.chk(e.L.nq_any_tangent_value(e.h, out.ptr, self.Fa.ptr, self.Fb.ptr, self.n, 0 if nm == "lnsigma" else 1), "nq_any_tangent_value")
            return out
        col = self.Fa if nm in ("f11", "f21") else self.Fb
        return col.real if nm in ("f11", "f12") else col.imag

    def _interp(self, plane):
        e = self.eng
        out = self._Plane(e, (1, self.n))
        m = self.m
        e.chk(e.L.nq_any_interp(e.h, out.ptr, plane.ptr, self.pos.ptr, self.n, m.nx, float(m.L), float(m.W)), "nq_any_interp")
        return out

    def _interp_wave(self):
        """a phi e^{-i f0 t_s} at the particles, from the current phi (a = 1 without drifter mode)"""
        e, m = self.eng, self.m
        out = self._Plane(e, (1, self.n))
        e.chk(e.L.nq_any_interp_wave(e.h, out.ptr, m._d["phi"].ptr, self.pos.ptr, self.n, m.nx, float(m.L), float(m.W),
                                     1.0 if self.wave is None else self.wave, float(m.f), float(self.wave_time(self.rg.steps))),
              "nq_any_interp_wave")
        return out

    def _planes(self, names):
        d, out = self.m._d, {}
        for nm in names:
            if nm in ("u", "v"):
                uv = self._interp(self._current_U())
                out[nm] = uv.real if nm == "u" else uv.imag
            elif nm in ("uw", "vw"):
                w = self._interp_wave()
                out[nm] = w.real if nm == "uw" else w.imag
            elif nm == "zeta":
                out[nm] = self._interp(self._current_Z())
            elif nm in ("k", "l"):
                out[nm] = self.wv.real if nm == "k" else self.wv.imag
            elif nm == "omega":
                out[nm] = self._interp_omega()
            elif nm in STRETCH_NAMES:
                out[nm] = self._tangent_plane(nm)
            else:
                out[nm] = self._interp(d[nm])
        return out

    def _record(self):
        if not self.ring:
            return
        self.ring[self.rg.slot()] = (self.pos.copy(), self._planes(self.record))
        self.rg.wrote()

    def _before_step(self):
        self.U0 = self._current_U()
        if self.wave is not None:
            self.P0 = self.m._d["phi"]            # the Plane of the state the step starts from (the step puts a new one in its place)
        if self.rays:
            self.Z0 = self._current_Z()

    def _after_step(self):
        e, m = self.eng, self.m
        U1 = self._current_U()
        if self.rays:
            e.chk(e.L.nq_any_particles_rk4_rays(e.h, self.pos.ptr, self.wv.ptr, self.n, self.U0.ptr, U1.ptr, self.Z0.ptr, self._current_Z().ptr,
                                                m.nx, float(m.L), float(m.W), float(m.U), self.eta, float(m.dt)), "nq_any_particles_rk4_rays")
            self.Z0 = None
        elif self.stretch and self.wave is None:
            e.chk(e.L.nq_any_particles_rk4_tangent(e.h, self.pos.ptr, self.Fa.ptr, self.Fb.ptr, self.n, self.U0.ptr, U1.ptr, m.nx, float(m.L),
                                                   float(m.W), float(m.U), float(m.dt)), "nq_any_particles_rk4_tangent")
        elif self.stretch:
            e.chk(e.L.nq_any_particles_rk4_wave_tangent(e.h, self.pos.ptr, self.Fa.ptr, self.Fb.ptr, self.n, self.U0.ptr, U1.ptr, self.P0.ptr,
                                                        m._d["phi"].ptr, m.nx, float(m.L), float(m.W), float(m.U), float(m.dt), self.wave,
                                                        float(m.f), float(self.wave_time(self.rg.steps))), "nq_any_particles_rk4_wave_tangent")
            self.P0 = None
        elif self.wave is None:
            e.chk(e.L.nq_any_particles_rk4(e.h, self.pos.ptr, self.n, self.U0.ptr, U1.ptr, m.nx, float(m.L), float(m.W), float(m.U),
                                           float(m.dt)), "nq_any_particles_rk4")
        else:
            e.chk(e.L.nq_any_particles_rk4_wave(e.h, self.pos.ptr, self.n, self.U0.ptr, U1.ptr, self.P0.ptr, m._d["phi"].ptr, m.nx,
                                                float(m.L), float(m.W), float(m.U), float(m.dt), self.wave, float(m.f),
                                                float(self.wave_time(self.rg.steps))), "nq_any_particles_rk4_wave")
            self.P0 = None
        self.U0 = None
        if self.rg.tick():
            self._record()

    def _positions(self):
        p = self.pos.get().reshape(-1)
        return p.real.copy(), p.imag.copy()

    def _wavevectors(self):
        w = self.wv.get().reshape(-1)
        return w.real.copy(), w.imag.copy()

    def _deformation(self):
        a, b = self.Fa.get().reshape(-1), self.Fb.get().reshape(-1)
        return np.array([a.real, b.real, a.imag, b.imag])

    def _reset_deformation(self):
        one = np.ones((1, self.n), np.complex128)
        self.Fa, self.Fb = self.eng.plane(one, real=False), self.eng.plane(1j * one, real=False)
        self._step0, self._count0 = self.rg.steps, self.rg.count

    def _stretch_step0(self):
        return self._step0

    def _steps_now(self):
        return self.rg.steps

    def _lagr_stretching(self, T, G, order, offsets):
        e, recs = self.eng, self._held_records()
        if self.rg.count - self.rg.held() < self._count0:
            raise RuntimeError("lagrangian.stretching: the ring still holds %d records written before the reset at particle step %d"
                               % (self._count0 - (self.rg.count - self.rg.held()), self._step0))
        ptrs = [r[1][nm].ptr for r in recs for nm in ("f11", "f12", "f21", "f22")]
        out = np.empty((T, G, 4))
        e.chk(e.L.nq_any_lagr_stretching(e.h, self.n, T, (ctypes.c_void_p * (4 * T))(*ptrs), 2, G, _lib._iptr(order), _lib._iptr(offsets),
                                         _lib._dptr(out)), "nq_any_lagr_stretching")
        return out

    def _sample(self, names):
        pl = self._planes(names)
        return {nm: (pl[nm].get().reshape(-1) if nm == "phi" else pl[nm].get().reshape(-1).real.copy()) for nm in names}

    def _records(self):
        rg = self.rg
        m = rg.held()
        slots = [rg.oldest(r) for r in range(m)]
        recs = [self.ring[s] for s in slots]
        steps = np.array([rg.ring_step[s] for s in slots], np.int64)
        pos = np.array([r[0].get().reshape(-1) for r in recs]).reshape(m, self.n)
        vals = {}
        for nm in self.record:
            a = np.array([r[1][nm].get().reshape(-1) for r in recs]).reshape(m, self.n)
            vals[nm] = a if nm == "phi" else a.real.copy()
        return steps, pos.real.copy(), pos.imag.copy(), vals

    # the device passes of lagrangian.py on the planes of the held records, oldest first
    def _held(self):
        return self.rg.held() if self.ring else 0

    def _held_records(self):
        return [self.ring[self.rg.oldest(r)] for r in range(self.rg.held())]

    def _record_steps(self):
        return np.array([self.rg.ring_step[self.rg.oldest(r)] for r in range(self.rg.held())], np.int64)

    def _lagr_spectrum(self, name, T, F, w, demean, G, order, offsets, chunk):
        e, recs = self.eng, self._held_records()
        keep = None
        if name == "uv":                          # the real parts of the u and the v plane
            re, im = [r[1]["u"].ptr for r in recs], [r[1]["v"].ptr for r in recs]
        elif name == "uvw":
            re, im = [r[1]["uw"].ptr for r in recs], [r[1]["vw"].ptr for r in recs]
        elif name == "uvt":                       # the sums as planes of their own, alive until the call returns
            keep = [(r[1]["u"] + r[1]["uw"], r[1]["v"] + r[1]["vw"]) for r in recs]
            re, im = [a.ptr for a, _ in keep], [b.ptr for _, b in keep]
        else:                                     # a complex plane: phi's imaginary part sits 8 bytes on; the others are real
            re = [r[1][name].ptr for r in recs]
            im = [p + 8 for p in re] if name == "phi" else None
        out = np.empty((F, G))
        ptrs = ctypes.c_void_p * T
        e.chk(e.L.nq_any_lagr_spectrum(e.h, self.n, T, ptrs(*re), None if im is None else ptrs(*im), 2, F, _lib._dptr(w), int(demean), G,
                                       _lib._iptr(order), _lib._iptr(offsets), chunk, _lib._dptr(out)), "nq_any_lagr_spectrum")
        return out

    def _lagr_dispersion(self, T, G, order, offsets, pairs):
        e, recs = self.eng, self._held_records()
        out = np.empty((T, G, 6))
        npairs = 0 if pairs is None else len(pairs[0])
        outp = np.empty((T, 5)) if npairs else None
        e.chk(e.L.nq_any_lagr_dispersion(e.h, self.n, T, (ctypes.c_void_p * T)(*[r[0].ptr for r in recs]), G, _lib._iptr(order),
                                         _lib._iptr(offsets), npairs, _lib._iptr(pairs[0]) if npairs else None,
                                         _lib._iptr(pairs[1]) if npairs else None, _lib._dptr(out), _lib._dptr(outp) if npairs else None),
              "nq_any_lagr_dispersion")
        return out, outp

    def _detach(self):
        self.pos = self.U = self.src = self.U0 = self.P0 = self.Z = self.zsrc = self.Z0 = self.wv = self.Fa = self.Fb = None
        self.ring = []
        self.eng.sync()


def _wave(m, wave):
    """the amplitude of drifter mode: None, or a finite real a > 0 (Kernel family only)"""
    if wave is None:
        return None
    if isinstance(wave, (bool, np.bool_)) or not isinstance(wave, (int, float, np.integer, np.floating)):
        raise ValueError("particles.attach: wave = %r (None, or the amplitude: a finite real number > 0)" % (wave,))
    a = float(wave)
    if not np.isfinite(a) or not a > 0.0:
        raise ValueError("particles.attach: wave = %r (None, or the amplitude: a finite real number > 0)" % (wave,))
    if _is_qg(m):
        raise ValueError("particles.attach: wave = %r: QGModel has no wave field (phi)" % (wave,))
    return a


def _rays(m, n, rays, eta, wave):
    """the wavevectors of ray mode: None, or ((k0, l0) two arrays of n finite reals, eta finite)"""
    if rays is None:
        if eta is not None:
            raise ValueError("particles.attach: eta = %r without rays=" % (eta,))
        return None, None
    if wave is not None:
        raise ValueError("particles.attach: rays= and wave= exclude each other (a ray is no drifter)")
    if _is_qg(m):
        raise ValueError("particles.attach: rays=: QGModel has no near-inertial waves")
    try:
        k, l = rays
        k, l = np.array(k, np.float64), np.array(l, np.float64)
    except (TypeError, ValueError):
        raise ValueError("particles.attach: rays = (k0, l0), two arrays of real wavenumbers")
    if k.ndim != 1 or l.ndim != 1 or k.size != n or l.size != n:
        raise ValueError("particles.attach: rays: k0 and l0 of shapes %s, %s for %d particles" % (k.shape, l.shape, n))
    if not (np.all(np.isfinite(k)) and np.all(np.isfinite(l))):
        raise ValueError("particles.attach: rays: non-finite wavenumbers")
    eta = m.hslash if eta is None else eta
    if isinstance(eta, (bool, np.bool_)) or not isinstance(eta, (int, float, np.integer, np.floating)) or not np.isfinite(float(eta)):
        raise ValueError("particles.attach: eta = %r (a finite real number; default m.hslash)" % (eta,))
    return (k, l), float(eta)


def _stretch(n, stretch, rays):
    """the starting F of stretch mode: None (off), True (the identity) or (4, n) float64 rows f11, f12, f21, f22 from an (n, 2, 2)
    array of finite reals"""
    if stretch is None or stretch is False:
        return None
    if rays is not None:
        raise ValueError("particles.attach: rays= and stretch= exclude each other (the ray map lives in four dimensions; its 2 x 2 "
                         "block is no deformation gradient)")
    if stretch is True:
        return True
    try:
        F = np.array(stretch, np.float64)
    except (TypeError, ValueError):
        raise ValueError("particles.attach: stretch = True, or the starting F: an (n, 2, 2) array of real numbers")
    if F.shape != (n, 2, 2):
        raise ValueError("particles.attach: stretch: F of shape %s for %d particles (expected (%d, 2, 2))" % (F.shape, n, n))
    if not np.all(np.isfinite(F)):
        raise ValueError("particles.attach: stretch: non-finite entries of F")
    return np.ascontiguousarray(F.reshape(n, 4).T)


def attach(m, x, y, record_every=0, capacity=1024, record=(), wave=None, rays=None, eta=None, stretch=None):
    """Attach n particles at (x, y) to model m (one set per model); see the module's doc.  ``wave=a``: drifter mode, the wave
    velocity a phi e^{-i f0 t} added to the advecting velocity.  ``rays=(k0, l0)``: ray mode, every particle a near-inertial wave
    packet with its wavevector, ``eta`` = f / kappa^2 (default ``m.hslash``).  ``stretch=True`` (or an (n, 2, 2) starting F): stretch
    mode, every particle carries the deformation gradient of its trajectory.  Argument errors raise ValueError before the device is
    touched; slab-decomposed models raise NotImplementedError."""
    x, y = _coords(x, y)
    wave = _wave(m, wave)
    stretch = _stretch(x.size, stretch, rays)
    rays, eta = _rays(m, x.size, rays, eta, wave)
    if isinstance(record_every, bool) or int(record_every) != record_every or record_every < 0:
        raise ValueError("particles.attach: record_every = %r (an integer >= 0)" % (record_every,))
    record_every = int(record_every)
    if record_every > 0 and (int(capacity) != capacity or capacity < 1):
        raise ValueError("particles.attach: capacity = %r (>= 1 while recording)" % (capacity,))
    capacity = int(capacity) if record_every > 0 else 0
    record = tuple(_names(m, record, "attach", rays is not None, stretch is not None))
    if len(set(record)) != len(record):
        raise ValueError("particles.attach: a name appears twice in record: %s" % (record,))
    return _attach.attach(m, _AnySize, _Fused, x, y, record_every, capacity, record, wave, rays, eta, stretch)
