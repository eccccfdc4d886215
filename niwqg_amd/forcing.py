"""Stochastic forcing of q and phi, drawn on the device inside the step.

    from niwqg_amd import forcing
    F = forcing.attach(m, q=forcing.ring(m, kf, width, eps), phi=None, seed=1, step0=0)
    m.run()                                   # every step ends with the increment and the re-inversion, batched or not
    F.work()                                  # {"q": ..., "phi": ...}: the energy the forcing has put in so far
    F.kick()                                  # one increment now, outside a step
    F.increment("q", step)                    # the increment of a step as a host plane (the state is untouched)
    F.state()                                 # {"seed", "step"}: attach(..., seed=seed, step0=step) continues the sequence
    F.detach()

After every step (after the filtered ETDRK4 update; the increment itself is not filtered -- put A inside the pass band)

    qh(l, k)   += sqrt(dt) A_q(l, k)   xi_q(l, k; s)        half spectrum (ny, nx/2+1); Hermitian: the forcing of q is a real field
    phih(l, k) += sqrt(dt) A_phi(l, k) xi_phi(l, k; s)      full plane (ny, nx); independent complex values

and then the end of a step again: phi = ifft(phih), _invert, _calc_rel_vorticity.  xi is white in time with E|xi|^2 = 1 and comes
from a counter-based generator (Philox4x32-10, counter (l, k, s, stream), key from the seed), so ``noise`` below restates it in
numpy bit for bit at the integer level, whatever the launch geometry.  ``Ke, Pw, Kw`` stay the unforced rates; ``work()`` holds
the energy put in:  q: the change of ke_qg at fixed q_w, sum_full [-Re(conj(psi-hat) D) + |D|^2 / (2 wv2)] / M^2;
phi: the change of ke_niw, sum [Re(conj(phih) D) + |D|^2 / 2] / M^2, with psi-hat, phih before the increment D.
"""
import numpy as np

from . import _attach, _lib

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
STREAMS = dict(q=0, phi=1)


# ---- the generator in numpy (the device functions' restatement; tests use it) ------------------------------------------------
def philox(counter, key):
    """Philox4x32-10: counter = four arrays (or integers) c0..c3, key = (k0, k1); returns the four output words as uint64
    arrays holding 32-bit values"""
    c = [np.asarray(v, np.uint64) & _MASK for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def noise(l, k, step, stream, seed):
    """xi of counter (l, k, step, stream): the unit-variance complex Gaussian the device draws there (l, k: array indices of the
    plane, broadcast against each other; stream 0: q, 1: phi).  The Hermitian rule of q is ``noise_plane``'s."""
    seed = int(seed)
    x = philox((l, k, int(step) & 0xFFFFFFFF, int(stream)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    n = (x[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (x[1] >> np.uint64(6)).astype(np.float64)
    u1 = 1.0 - n * (1.0 / 9007199254740992.0)
    u2 = (x[2].astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    r, th = np.sqrt(-np.log(u1)), 6.283185307179586 * u2
    return r * np.cos(th) + 1j * (r * np.sin(th))


def noise_plane(nx, step, stream, seed):
    """the whole plane of one step: stream 1 (phi): (nx, nx) independent values; stream 0 (q): (nx, nx/2+1) under the Hermitian
    rule -- zero on row nx/2, column nx/2 and at (0, 0); on column 0 row nx - l is the conjugate of row l, 1 <= l < nx/2"""
    n = int(nx)
    if stream == 1:
        return noise(np.arange(n)[:, None], np.arange(n)[None, :], step, 1, seed)
    z = noise(np.arange(n)[:, None], np.arange(n // 2 + 1)[None, :], step, 0, seed)
    z[n // 2, :] = 0.0
    z[:, n // 2] = 0.0
    z[0, 0] = 0.0
    z[n // 2 + 1:, 0] = np.conj(z[1:n // 2, 0][::-1])
    return z


def ring(m, kf, width, eps, field="q"):
    """Amplitude plane of a Gaussian ring: A^2 proportional to exp(-(kappa - kf)^2 / (2 width^2)), cut at +-3 width, zero on the
    Nyquist lines and at (0, 0), normalised so that the expected injection rate is exactly ``eps``:
    q (half plane (ny, nx/2+1)): 1/2 sum_full A^2 / (wv2 M^2) = eps;   phi (full plane): 1/2 sum A^2 / M^2 = eps."""
    if field not in STREAMS:
        raise ValueError("forcing.ring: field = %r ('q' or 'phi')" % (field,))
    kf, width, eps = float(kf), float(width), float(eps)
    if not (np.isfinite(kf) and kf > 0 and np.isfinite(width) and width > 0 and np.isfinite(eps) and eps >= 0):
        raise ValueError("forcing.ring: kf = %r, width = %r (finite, > 0), eps = %r (finite, >= 0)" % (kf, width, eps))
    n = int(m.nx)
    kk, ll = np.asarray(m.kk, np.float64), np.asarray(m.ll, np.float64)
    kcol = np.abs(kk[:n // 2 + 1]) if field == "q" else kk
    wv2 = kcol[None, :] ** 2 + ll[:, None] ** 2
    kap = np.sqrt(wv2)
    a2 = np.where(np.abs(kap - kf) <= 3.0 * width, np.exp(-(kap - kf) ** 2 / (2.0 * width ** 2)), 0.0)
    a2[n // 2, :] = 0.0
    a2[:, n // 2] = 0.0
    a2[0, 0] = 0.0
    M2 = (float(n) * n) ** 2
    if field == "q":
        w = np.full(n // 2 + 1, 2.0)
        w[0] = w[-1] = 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            dens = np.where(wv2 > 0, a2 / wv2, 0.0) * w[None, :]
    else:
        dens = a2
    tot = 0.5 * dens.sum() / M2
    if not tot > 0:
        raise ValueError("forcing.ring: no mode within 3 width of kf = %g (dk = %g)" % (kf, kk[1]))
    return np.sqrt(a2 * (eps / tot))


# ---- the public object ------------------------------------------------------------------------------------------------------
def _kind(m):
    from .QGModel import Model as QG
    if isinstance(m, QG):
        return "qg"
    return {_lib.COUPLED: "coupled", _lib.UNCOUPLED: "uncoupled", _lib.YBJ: "ybj"}[m.model_id]


def _plane(a, shape, what):
    try:
        a = np.array(a, np.float64)
    except (TypeError, ValueError):
        raise ValueError("forcing.attach: %s must be a real array" % what)
    if a.shape != shape:
        raise ValueError("forcing.attach: %s has shape %s, expected %s" % (what, a.shape, shape))
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError("forcing.attach: %s must be finite and >= 0" % what)
    return np.ascontiguousarray(a)


class Forcing(_attach.Attachment):
    """A forcing attached to one model (``attach``); see the module's doc"""
    SLOT, LABEL = "_forcing", "forcing"
    ALREADY = (ValueError, "forcing.attach: this model has a forcing attached already (detach it first)")
    NO_SLAB = ("forcing.attach: slab-decomposed models have no forcing yet (every rank would draw its own "
               "columns and the work partials would need an all-reduce; DESIGN.md section 7)")

    def __init__(self, m, Aq, Aphi, seed, step0):
        self.m, self.seed = m, seed
        self.forced = tuple(nm for nm, a in (("q", Aq), ("phi", Aphi)) if a is not None)

    def kick(self):
        """one increment and re-inversion now, outside a step (advances the step index)"""
        self._check()
        self._kick()

    def work(self):
        """{"q": ..., "phi": ...}: the energy the increments have put into ke_qg and ke_niw since attach"""
        self._check()
        _, wq, wp = self._state()
        return {"q": wq, "phi": wp}

    def state(self):
        """{"seed", "step"}: attach(m, ..., seed=seed, step0=step) on the same state continues this sequence bit for bit"""
        self._check()
        return {"seed": self.seed, "step": self._state()[0]}

    def increment(self, name, step):
        """the increment sqrt(dt) A xi of step ``step`` as a host plane ("q": (ny, nx/2+1), "phi": (ny, nx)); the state is untouched"""
        self._check()
        if name not in STREAMS:
            raise ValueError("forcing.increment: name = %r ('q' or 'phi')" % (name,))
        if name not in self.forced:
            raise ValueError("forcing.increment: %s is not forced" % name)
        if isinstance(step, bool) or int(step) != step or step < 0:
            raise ValueError("forcing.increment: step = %r (an integer >= 0)" % (step,))
        return self._increment(STREAMS[name], int(step))


class _Fused(Forcing):
    """fused contexts: amplitudes, the step index and the work live in the library (nq_forcing_*)"""

    def __init__(self, m, Aq, Aphi, seed, step0):
        Forcing.__init__(self, m, Aq, Aphi, seed, step0)
        self.ctx = m._ctx
        self.ctx.forcing_attach(Aq, Aphi, seed, step0)

    def _kick(self):
        self.ctx.forcing_apply()
        m = self.m
        m._cache.clear()                        # what was read from the old state
        m._user.pop("q", None)
        m._user.pop("phi", None)

    def _state(self):
        return self.ctx.forcing_state()

    def _increment(self, stream, step):
        return self.ctx.forcing_increment(stream, step)

    def _detach(self):
        self.ctx.forcing_detach()


class _AnySize(Forcing):
    """any-size path: amplitudes are engine planes; the model's _step_etdrk4 calls _after_step (nq_any_forcing on its qh and phih,
    then its own _to_physical sequence)"""

    def __init__(self, m, Aq, Aphi, seed, step0):
        Forcing.__init__(self, m, Aq, Aphi, seed, step0)
        e = self.eng = m._eng
        n = m.nx
        self.s, self.wq, self.wphi = int(step0), 0.0, 0.0
        self.qg = _kind(m) == "qg"
        self.Aq = self.Aq_state = self.gq = self.Aphi = None
        kk, ll = np.asarray(m.kk, np.float64), np.asarray(m.ll, np.float64)
        if Aq is not None:
            self.Aq = e.plane(Aq, real=True)
            wv2 = kk[None, :n // 2 + 1] ** 2 + ll[:, None] ** 2
            with np.errstate(divide="ignore"):
                g = np.where(wv2 > 0, 1.0 / wv2, 0.0)
            if self.qg:                       # qh is the half spectrum: half-spectrum weights folded into 1 / wv2
                g[:, 1:n // 2] *= 2.0
                self.Aq_state = self.Aq
            else:                             # the reference's full-plane qh: A and 1 / wv2 extended to k < 0
                g = _lib_hermitian_real(g, n)
                self.Aq_state = e.plane(_lib_hermitian_real(Aq, n), real=True)
            self.gq = e.plane(g, real=True)
        if Aphi is not None:
            self.Aphi = e.plane(Aphi, real=True)

    def _call(self, plane, amp, layout, stream, step, work_in=None):
        e, n = self.eng, self.m.nx
        out = np.zeros(2) if work_in is not None else None
        e.chk(e.L.nq_any_forcing(e.h, plane.ptr, amp.ptr, n, plane.shape[1], layout, self.seed, int(step), stream,
                                 float(np.sqrt(self.m.dt)), None if work_in is None else work_in.ptr,
                                 None if out is None else _lib._dptr(out)), "nq_any_forcing")
        return out

    def _after_step(self):
        from ._anysize import RD_WSUMABS2
        m, e = self.m, self.eng
        d = m._d
        M2 = float(m.M) ** 2
        if self.Aq is not None:
            inc = e.zeros(d["qh"].shape)
            lin = self._call(inc, self.Aq_state, 0 if self.qg else 2, 0, self.s, work_in=d["ph"])[0]
            quad = float(inc._reduce(RD_WSUMABS2, self.gq)[0]) / M2
            self.wq += -lin + 0.5 * quad
            d["qh"] = d["qh"] + inc
        if self.Aphi is not None:
            w = d["phih"].copy()
            o = self._call(w, self.Aphi, 1, 1, self.s, work_in=w)
            self.wphi += o[0] + 0.5 * o[1]
            d["phih"] = w
        if self.qg:                           # the end of QGFamily's step
            m._invert_d()
            d["q"] = m._irfft(d["qh"])
        elif m.model_id == _lib.YBJ:          # ... of _step_ybj (psi is steady)
            d["phi"] = m._ifft(d["phih"])
        else:
            m._to_physical()
        m._dirty()
        self.s += 1

    _kick = _after_step

    def _state(self):
        return self.s, self.wq, self.wphi

    def _increment(self, stream, step):
        n = self.m.nx
        inc = self.eng.zeros((n, n // 2 + 1) if stream == 0 else (n, n))
        self._call(inc, self.Aq if stream == 0 else self.Aphi, 0 if stream == 0 else 1, stream, step)
        return inc.get()

    def _detach(self):
        self.Aq = self.Aq_state = self.gq = self.Aphi = None
        self.eng.sync()


def _lib_hermitian_real(half, n):
    """a real (n, n/2+1) plane extended to (n, n) by a(l, -k) = a(-l, k)"""
    full = np.empty((n, n))
    full[:, :n // 2 + 1] = half
    inner = half[:, 1:n // 2]
    full[:, n // 2 + 1:] = np.roll(inner[::-1, :], 1, axis=0)[:, ::-1]
    return full


def attach(m, q=None, phi=None, seed=0, step0=0):
    """Attach white-in-time forcing to model m (one per model): ``q`` a real amplitude plane (ny, nx/2+1) on the half spectrum,
    ``phi`` one of (ny, nx) on the full plane, both finite and >= 0, at least one.  CoupledModel and UnCoupledModel take both,
    QGModel q only, YBJModel phi only.  Argument errors raise ValueError before the device is touched; slab-decomposed models
    raise NotImplementedError."""
    kind = _kind(m)
    n = int(m.nx)
    if q is None and phi is None:
        raise ValueError("forcing.attach: give q, phi or both")
    if q is not None and kind == "ybj":
        raise ValueError("forcing.attach: YBJModel takes phi forcing only (its psi is steady)")
    if phi is not None and kind == "qg":
        raise ValueError("forcing.attach: QGModel takes q forcing only (it has no wave field)")
    Aq = None if q is None else _plane(q, (n, n // 2 + 1), "q")
    Aphi = None if phi is None else _plane(phi, (n, n), "phi")
    if Aq is not None and not np.array_equal(Aq[1:n // 2, 0], Aq[n // 2 + 1:, 0][::-1]):
        raise ValueError("forcing.attach: q must be equal on rows l and ny - l of column 0 (the forcing of q is a real field)")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError("forcing.attach: seed = %r (an integer in [0, 2^64))" % (seed,))
    if isinstance(step0, bool) or int(step0) != step0 or step0 < 0:
        raise ValueError("forcing.attach: step0 = %r (an integer >= 0)" % (step0,))
    seed, step0 = int(seed), int(step0)
    return _attach.attach(m, _AnySize, _Fused, Aq, Aphi, seed, step0)
