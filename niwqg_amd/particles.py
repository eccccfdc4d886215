"""Lagrangian particles advected on the device inside the step.

    from niwqg_amd import particles
    P = particles.attach(m, x, y, record_every=0, capacity=1024, record=(), wave=None)
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
"""
import ctypes

import numpy as np

from . import _attach, _lib

FIELDS = ("u", "v", "q", "phi")                                          # the fields of the state
NAMES = FIELDS + ("uw", "vw")                                            # and the wave velocity at the particle (section 5s)
_CODES = dict(u=0, v=1, q=2, phi=3, uw=_lib.PT_UW, vw=_lib.PT_VW)        # the new codes: include/niwqg_amd.h
# nq_lagr_spectrum's names: the columns, and the composites u + i v, uw + i vw, (u + uw) + i (v + vw)
_LAGR_CODES = dict(_CODES, uv=4, uvw=_lib.LAGR_UVW, uvt=_lib.LAGR_UVT)


def _is_qg(m):
    from .QGModel import Model as QG
    return isinstance(m, QG)


def available(m, wave=False):
    """names ``record`` and ``sample`` accept for this model: the fields of the state ("phi": the Kernel family only), which
    ``sample()`` returns by default, and with ``wave=True`` also the wave velocity columns "uw", "vw" (Kernel family only)"""
    if _is_qg(m):
        return ["u", "v", "q"]
    return list(NAMES) if wave else list(FIELDS)


def _names(m, names, what):
    names = [names] if isinstance(names, str) else list(names)
    valid = available(m, wave=True)
    bad = [n for n in names if n not in valid]
    if bad:
        raise ValueError("particles.%s: %s not available for %s; valid names: %s"
                         % (what, ", ".join(map(repr, bad)), type(m).__name__, ", ".join(valid)))
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

    def __init__(self, m, n, record_every, capacity, record, wave=None):
        self.m, self.n = m, n
        self.record_every, self.capacity, self.record = record_every, capacity, tuple(record)
        self.tc0, self.t0 = m.tc, m.t
        self.wave = wave                          # drifter mode: the amplitude a, or None

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
        names = available(self.m) if names is None else _names(self.m, names, "sample")
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

    def __init__(self, m, x, y, record_every, capacity, record, wave=None):
        Particles.__init__(self, m, len(x), record_every, capacity, record, wave)
        self.ctx = m._ctx
        self.ctx.particles_attach(x, y, m.L, m.W, record_every, capacity, [_CODES[r] for r in record])
        if _is_qg(m):
            return
        try:                                      # the clock of "uw" / "vw" (host values only) or, with it, drifter mode
            if wave is None:
                self.ctx.particles_clock(m.f, m.t)
            else:
                self.ctx.particles_wave(wave, m.f, m.t)
        except Exception:
            self.ctx.particles_detach()
            raise

    def _positions(self):
        return self.ctx.particles_get(self.n)

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

    def __init__(self, m, x, y, record_every, capacity, record, wave=None):
        from ._anysize import Plane
        Particles.__init__(self, m, len(x), record_every, capacity, record, wave)
        self.eng = m._eng
        self.pos = self.eng.plane((x + 1j * y).reshape(1, -1), real=False)
        self.U, self.src = None, None       # velocity plane of the state src (the psi-hat Plane it was formed from)
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

    def _after_step(self):
        e, m = self.eng, self.m
        U1 = self._current_U()
        if self.wave is None:
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
        self.pos = self.U = self.src = self.U0 = self.P0 = None
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


def attach(m, x, y, record_every=0, capacity=1024, record=(), wave=None):
    """Attach n particles at (x, y) to model m (one set per model); see the module's doc.  ``wave=a``: drifter mode, the wave
    velocity a phi e^{-i f0 t} added to the advecting velocity.  Argument errors raise ValueError before the device is touched;
    slab-decomposed models raise NotImplementedError."""
    x, y = _coords(x, y)
    wave = _wave(m, wave)
    if isinstance(record_every, bool) or int(record_every) != record_every or record_every < 0:
        raise ValueError("particles.attach: record_every = %r (an integer >= 0)" % (record_every,))
    record_every = int(record_every)
    if record_every > 0 and (int(capacity) != capacity or capacity < 1):
        raise ValueError("particles.attach: capacity = %r (>= 1 while recording)" % (capacity,))
    capacity = int(capacity) if record_every > 0 else 0
    record = tuple(_names(m, record, "attach"))
    if len(set(record)) != len(record):
        raise ValueError("particles.attach: a name appears twice in record: %s" % (record,))
    return _attach.attach(m, _AnySize, _Fused, x, y, record_every, capacity, record, wave)
