"""Low-mode time series recorded inside the step, and their frequency - wavenumber spectra formed on the device
(DESIGN.md section 5j).

    from niwqg_amd import frequency
    R = frequency.attach(m, kmax, every=1, length=256, fields=None)
    m.run()                                   # every `every`-th step ends with one record, batched or not
    ts = R.series("phi")                      # .step (T,), .t (T,), .values (T, 2K+1, 2K+1) complex128
    S = R.spectrum(window="hann", demean=False)
    plt.pcolormesh(S.k, S.omega, np.log10(S.values["phi"]))
    R.info()                                  # {"written", "held", "steps"}
    R.detach()

The block: integer wavenumbers |i|, |j| <= K = kmax (1 <= K < nx/2: the Nyquist lines and the passenger row are never recorded),
rows j = 0..K, -K..-1 in fftfreq order; columns the same for a full-plane field, i = 0..K for a half-spectrum field.

    "phi"   phi-hat                                   full plane        (T, 2K+1, 2K+1)
    "q"     q-hat as the device holds it              half spectrum     (T, 2K+1, K+1)     (copy X+ on dual-copy contexts)
    "psi"   the psi-hat the model holds (``m.ph``)    half spectrum     (T, 2K+1, K+1)

Record 0 is written at attach from the current state, then one record after every ``every``-th step since attach (after the
forcing where there is one); the ring keeps the last ``length`` records.

``spectrum``: with the T held records x_n(l, k), Delta = every dt and a real window w_n,  X_p = sum_n w_n x_n e^{+2 pi i p n / T}
(``T * ifft(w * x, axis=0)``: a mode evolving as e^{-i omega t} appears at +omega), omega_p = 2 pi fftfreq(T, Delta), sorted
ascending.  With shell b = ``spectra.shell_of(i, j)`` and M = nx ny:

    P_phi(p, b) = 1/2 sum_{block, shell b} |X_p|^2 / (M^2 T sum w^2)
    P_q(p, b)   = 1/2 [sum_{col 0} |X_p|^2 + sum_{cols 1..K} (|X_p|^2 + |X_-p|^2)] / (M^2 T sum w^2)
    P_psi(p, b) = P_q with kappa^2(l, k) inside the sums

The +-p pairing is what the mirrored half plane of a real field contributes (X_p(-l, -k) = conj X_-p(l, k) for a real window), so
P_q and P_psi are even in omega.  By Parseval in time sum_p P(p, b) = sum_n w_n^2 S_n(b) / sum_n w_n^2 with S_n(b) the shell
spectrum of record n; for phi and b <= K that is ``isotropic_spectra(m, "ke_niw")``.  ``reference_spectrum`` is the same
definition in numpy.
"""
import ctypes

import numpy as np

from . import _attach, _lib
from .spectra import shell_of

FIELDS = ("phi", "q", "psi")                      # ids of the library (include/niwqg_amd.h: nq_freq_attach)
_CLASS_NAMES = {_lib.COUPLED: "CoupledModel", _lib.UNCOUPLED: "UnCoupledModel", _lib.QG: "QGModel", _lib.YBJ: "YBJModel"}
_CLASS_FIELDS = {_lib.COUPLED: FIELDS, _lib.UNCOUPLED: FIELDS, _lib.QG: ("q", "psi"), _lib.YBJ: ("phi",)}


# ---- checks that need no model (the CPU tests drive them) --------------------------------------------------------------------
def available(class_id):
    """names of the fields a model class (``_lib.COUPLED``, ``UNCOUPLED``, ``QG``, ``YBJ``) can record"""
    return list(_CLASS_FIELDS[class_id])


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check(nx, class_id, kmax, every=1, length=256, fields=None):
    """the arguments of ``attach`` checked against the grid size and the model class; returns (kmax, every, length, fields) with
    ``fields`` a tuple of names.  Every error is a ValueError, raised before anything reaches the library."""
    valid = available(class_id)
    if not _integer(kmax) or not 1 <= kmax < nx // 2:
        raise ValueError("frequency.attach: kmax = %r (an integer, 1 <= kmax < nx/2 = %d)" % (kmax, nx // 2))
    if not _integer(every) or every < 1:
        raise ValueError("frequency.attach: every = %r (an integer >= 1)" % (every,))
    if not _integer(length) or length < 2:
        raise ValueError("frequency.attach: length = %r (an integer >= 2)" % (length,))
    if fields is None:
        fields = valid
    fields = [fields] if isinstance(fields, str) else list(fields)
    if not fields:
        raise ValueError("frequency.attach: no fields; valid names: %s" % ", ".join(valid))
    bad = [n for n in fields if n not in valid]
    if bad:
        raise ValueError("frequency.attach: %s not available for %s; valid names: %s"
                         % (", ".join(map(repr, bad)), _CLASS_NAMES[class_id], ", ".join(valid)))
    if len(set(fields)) != len(fields):
        raise ValueError("frequency.attach: a field is given twice: %s" % ", ".join(fields))
    return int(kmax), int(every), int(length), tuple(fields)


def check_window(window, T, what="frequency.spectrum"):
    """the window of ``spectrum`` as T float64 values: "boxcar", "hann" (periodic: 0.5 - 0.5 cos(2 pi n / T)) or T finite reals;
    ``what``: the prefix of the messages (lagrangian.py checks its windows here too)"""
    if not _integer(T) or T < 2:
        raise ValueError("%s: %r records held (at least 2)" % (what, T))
    if isinstance(window, str):
        if window == "boxcar":
            return np.ones(T)
        if window == "hann":
            return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(T) / T)
        raise ValueError("%s: window = %r ('boxcar', 'hann' or an array of %d reals)" % (what, window, T))
    try:
        w = np.array(window, np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: the window must be 'boxcar', 'hann' or an array of %d reals" % (what, T))
    if w.shape != (T,):
        raise ValueError("%s: the window has shape %s, %d records are held" % (what, w.shape, T))
    if not np.all(np.isfinite(w)):
        raise ValueError("%s: the window must be finite" % what)
    if not np.any(w != 0.0):
        raise ValueError("%s: the window is zero everywhere" % what)
    return np.ascontiguousarray(w)


# ---- the block ---------------------------------------------------------------------------------------------------------------
def block_numbers(K):
    """integer wavenumbers of the block's rows (and of a full-plane field's columns): 0..K, -K..-1"""
    return np.append(np.arange(0, K + 1), np.arange(-K, 0))


def block_index(nx, K):
    """indices into an axis of length nx of the block's rows (and of a full-plane field's columns)"""
    return block_numbers(K) % nx


def block_shells(K, full):
    """shell of every element of one record: (2K+1, 2K+1) for a full-plane field, (2K+1, K+1) for a half spectrum"""
    j = block_numbers(K)
    i = j if full else np.arange(K + 1)
    return shell_of(i[None, :], j[:, None])


def block_shell_count(K):
    return int(shell_of(K, K)) + 1


def block_modes(K):
    """full-plane wavenumbers of the block per shell (``spectra.shell_modes(nx)`` for the shells b <= K)"""
    return np.bincount(block_shells(K, True).ravel(), minlength=block_shell_count(K)).astype(np.int64)


def _transform(y):
    """X_p = sum_n y_n e^{+2 pi i p n / T} along axis 0; extended precision by the definition (numpy's FFT is double only)"""
    T = y.shape[0]
    if y.dtype != np.clongdouble:
        return T * np.fft.ifft(y, axis=0)
    pn = (np.arange(T)[:, None] * np.arange(T)[None, :]) % T               # the angle reduced exactly
    a = 2 * np.arccos(np.longdouble(-1)) * pn.astype(np.longdouble) / T      # (np.pi is a double)
    E = np.cos(a) + 1j * np.sin(a)
    return np.tensordot(E, y, axes=(1, 0))


def reference_spectrum(series, dt_rec, kind, window, demean, nx, ny, dk=1.0):
    """The definition of ``Recorder.spectrum`` in numpy: ``series`` (T, 2K+1, cols) of field ``kind`` ("phi": cols = 2K+1; "q",
    "psi": cols = K+1), ``dt_rec`` the time between records, ``window`` as there; ``dk`` enters "psi" only (kappa^2 =
    dk^2 (i^2 + j^2)).  Returns (omega, P): omega ascending (T,), P (T, nb).  A ``clongdouble`` series is worked in extended
    precision throughout."""
    if kind not in FIELDS:
        raise ValueError("frequency.reference_spectrum: kind = %r; valid names: %s" % (kind, ", ".join(FIELDS)))
    x = np.asarray(series)
    ext = x.dtype == np.clongdouble
    real = np.longdouble if ext else np.float64
    x = x.astype(np.clongdouble if ext else np.complex128)
    full = kind == "phi"
    T, R, C = x.shape
    K = (R - 1) // 2
    if R != 2 * K + 1 or K < 1 or C != (R if full else K + 1):
        raise ValueError("frequency.reference_spectrum: a %s series of shape %s" % (kind, x.shape))
    w = check_window(window, T).astype(real)
    if demean:
        x = x - x.mean(axis=0)[None]
    X = _transform(w[:, None, None] * x)
    a = X.real ** 2 + X.imag ** 2
    if not full:                                                # the mirrored half plane: bin -p of the same wavenumber
        minus = a[(-np.arange(T)) % T]
        a = np.concatenate([a[:, :, :1], a[:, :, 1:] + minus[:, :, 1:]], axis=2)
    if kind == "psi":
        j = block_numbers(K).astype(real)
        i = np.arange(K + 1).astype(real)
        a = a * (real(dk) ** 2 * (i[None, :] ** 2 + j[:, None] ** 2))[None]
    sh = block_shells(K, full).ravel()
    nb = block_shell_count(K)
    P = np.zeros((T, nb), real)
    flat = a.reshape(T, -1)
    for b in range(nb):
        P[:, b] = flat[:, sh == b].sum(axis=1)
    M = real(nx) * real(ny)
    P *= real(0.5) / (M * M * T * (w * w).sum())
    f = np.fft.fftfreq(T, float(dt_rec))
    order = np.argsort(f, kind="stable")
    return 2.0 * np.pi * f[order], P[order]


# ---- the public objects ------------------------------------------------------------------------------------------------------
class Series(object):
    """step (T,) steps since attach, t (T,) model time, values (T, 2K+1, cols) complex128 of the held records, oldest first"""

    def __init__(self, step, t, values):
        self.step, self.t, self.values = step, t, values


class FrequencySpectra(object):
    """omega (T,) ascending, shell / k (nb,), dk, k_iso_max = K dk (the shells above it are cut by the block), modes (full-plane
    wavenumbers of the block per shell), values {field: (T, nb) float64}, step (T,) of the held records"""

    def __init__(self, omega, shell, dk, modes, k_iso_max, values, step):
        self.omega, self.shell, self.dk, self.k = omega, shell, dk, shell * dk
        self.modes, self.k_iso_max, self.values, self.step = modes, k_iso_max, values, step

    def __repr__(self):
        return "FrequencySpectra(T=%d, nb=%d, dk=%g, fields=%s)" % (len(self.omega), len(self.shell), self.dk, sorted(self.values))


def _class_id(m):
    from .QGModel import Model as QG
    return _lib.QG if isinstance(m, QG) else m.model_id


class Recorder(_attach.Attachment):
    """A recorder attached to one model (``attach``); see the module's doc"""
    SLOT, LABEL = "_frequency", "frequency"
    ALREADY = (ValueError, "frequency.attach: this model has a recorder attached already (detach it first)")
    NO_SLAB = ("frequency.attach: slab-decomposed models have no recorder yet (every rank would gather the columns "
               "it owns and the block would be assembled at read-out; DESIGN.md section 7)")

    def __init__(self, m, K, every, length, fields):
        self.m, self.kmax, self.every, self.length, self.fields = m, K, every, length, fields
        self.t0, self.dt = float(m.t), float(m.dt)

    def _check(self, name=None):
        _attach.Attachment._check(self)
        if name is not None and name not in self.fields:
            raise ValueError("frequency: %r is not recorded; recorded: %s" % (name, ", ".join(self.fields)))

    def info(self):
        """{"written": records written, "held": records held, "steps": steps since attach}"""
        self._check()
        w, h, s = self._info()
        return {"written": w, "held": h, "steps": s}

    def series(self, name):
        """the held records of one field, oldest first"""
        self._check(name)
        K = self.kmax
        step, v = self._series(name, 2 * K + 1, 2 * K + 1 if name == "phi" else K + 1)
        return Series(step, self.t0 + step * self.dt, v)

    def spectrum(self, window="hann", demean=False, fields=None):
        """the (frequency x shell) table of every recorded field (or of ``fields``), formed on the device"""
        self._check()
        names = self.fields if fields is None else ([fields] if isinstance(fields, str) else list(fields))
        for n in names:
            self._check(n)
        held = self._info()[1]
        w = check_window(window, held)
        K, dk = self.kmax, float(self.m.dk)
        nb = block_shell_count(K)
        f = np.fft.fftfreq(held, self.every * self.dt)
        order = np.argsort(f, kind="stable")
        values = {n: self._spectrum(n, w, bool(demean), dk, nb)[order] for n in names}
        step = self._series(names[0], 0, 0, steps_only=True)
        return FrequencySpectra(2.0 * np.pi * f[order], np.arange(nb, dtype=np.int64), dk, block_modes(K), K * dk, values, step)


class _Fused(Recorder):
    """fused contexts: the ring lives in the library and nq_step records into it (nq_freq_*)"""

    def __init__(self, m, K, every, length, fields):
        Recorder.__init__(self, m, K, every, length, fields)
        self.ctx = m._ctx
        self.ctx.freq_attach(K, every, length, [FIELDS.index(n) for n in fields])

    def _info(self):
        return self.ctx.freq_info()

    def _series(self, name, rows, cols, steps_only=False):
        held = self._info()[1]
        if steps_only:
            steps = (ctypes.c_longlong * held)()
            self.ctx._chk(self.ctx.L.nq_freq_series(self.ctx.h, FIELDS.index(name), steps, None), "nq_freq_series")
            return np.array(steps[:held], np.int64)
        return self.ctx.freq_series(FIELDS.index(name), held, rows, cols)

    def _spectrum(self, name, w, demean, dk, nb):
        return self.ctx.freq_spectrum(FIELDS.index(name), w, demean, dk, nb)

    def _detach(self):
        self.ctx.freq_detach()


class _AnySize(Recorder):
    """any-size path: the rings are engine planes; the model's _step_etdrk4 calls _after_step (nq_any_freq_record on its phih,
    qh and ph, one launch), the spectrum pass is the library's on the engine-owned ring (nq_any_freq_spectrum)"""

    _PLANES = dict(phi="phih", q="qh", psi="ph")

    def __init__(self, m, K, every, length, fields):
        Recorder.__init__(self, m, K, every, length, fields)
        e = self.eng = m._eng
        R = 2 * K + 1
        self.cols = [R if n == "phi" else K + 1 for n in fields]
        self.rings = [e.zeros((length * R, c)) for c in self.cols]
        self.rg = _attach.Ring(length, every)
        nf = len(fields)
        self._rings_c = (ctypes.c_void_p * nf)(*[r.ptr for r in self.rings])
        self._full_c = (ctypes.c_int * nf)(*[1 if n == "phi" else 0 for n in fields])
        self._record()

    def _record(self):
        e, m, nf = self.eng, self.m, len(self.fields)
        planes = [m._d[self._PLANES[n]] for n in self.fields]
        slot = self.rg.slot()
        e.chk(e.L.nq_any_freq_record(e.h, nf, self._rings_c, (ctypes.c_void_p * nf)(*[p.ptr for p in planes]),
                                     (ctypes.c_int * nf)(*[p.shape[1] for p in planes]), self._full_c, m.nx, self.kmax, self.length, slot),
              "nq_any_freq_record")
        self.rg.wrote()

    def _after_step(self):
        if self.rg.tick():
            self._record()

    def _info(self):
        return self.rg.count, self.rg.held(), self.rg.steps

    def _slots(self):
        return [self.rg.oldest(r) for r in range(self.rg.held())]

    def _series(self, name, rows, cols, steps_only=False):
        slots = self._slots()
        step = np.array([self.rg.ring_step[s] for s in slots], np.int64)
        if steps_only:
            return step
        ring = self.rings[self.fields.index(name)].get().reshape(self.length, rows, cols)
        return step, np.ascontiguousarray(ring[slots])

    def _spectrum(self, name, w, demean, dk, nb):
        e = self.eng
        slots = self._slots()
        out = np.empty((len(slots), nb))
        e.chk(e.L.nq_any_freq_spectrum(e.h, self.rings[self.fields.index(name)].ptr, self.m.nx, self.kmax, int(name == "phi"), int(name == "psi"),
                                       self.length, slots[0], len(slots), _lib._dptr(w), int(demean), dk, nb, _lib._dptr(out)),
              "nq_any_freq_spectrum")
        return out

    def _detach(self):
        self.eng.sync()
        self.rings = []


def attach(m, kmax, every=1, length=256, fields=None):
    """Attach a recorder to model m (one per model): the block |i|, |j| <= kmax of ``fields`` (default: everything the class takes;
    CoupledModel and UnCoupledModel "phi", "q", "psi", QGModel "q", "psi", YBJModel "phi") goes into a device ring of ``length``
    records, one at attach and one after every ``every``-th step.  Argument errors raise ValueError before the device is touched;
    slab-decomposed models raise NotImplementedError."""
    K, every, length, fields = check(int(m.nx), _class_id(m), kmax, every, length, fields)
    return _attach.attach(m, _AnySize, _Fused, K, every, length, fields)
