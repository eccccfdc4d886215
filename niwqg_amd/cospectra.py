"""Isotropic co-spectra and coherence of the physical fields, formed on the device.

    from niwqg_amd import cospectra
    cs = cospectra.cross_spectra(m, names=("q_psi", "phi2", "ow"))
    cs.k, cs.shell, cs.dk, cs.modes, cs.k_iso_max       # as IsotropicSpectra
    cs.auto["phi2"]                                      # length nb
    cs.co[("q_psi", "phi2")]                             # length nb; either order of the pair
    cs.coherence("q_psi", "phi2")                        # co / sqrt(auto_a auto_b); NaN where a denominator is 0
    cs.covariance("q_psi", "phi2"), cs.correlation("q_psi", "phi2")     # from the shells >= 1
    A = cospectra.Accumulator(m, names); A.add(); ...; A.result(); A.reset()

``isotropic_spectra`` resolves by scale the quadratic forms of ONE spectral state and ``spectral_transfer`` the nonlinear terms;
this module says at which scales two PHYSICAL fields vary together: where |phi|^2 and q_psi are anti-correlated, where |grad phi|^2
follows the strain.

Names (``available(m)``): ``q``, ``q_psi``, ``phi2`` and the seven names of ``flow.NAMES`` on CoupledModel, UnCoupledModel and
YBJModel (YBJModel: what ``pdfs`` and ``flow`` give it); ``q`` and, with its passive scalar, ``c`` on QGModel (the any-size path
also has ``flow.available(m)`` there).  A call takes 1 to 3 different names.  The values are exactly those ``pdfs.field_pdfs`` bins
and ``averages`` sums for the name: the rows of the last inversion (dual-copy contexts: the mean of the two q-hat copies; ``set_phi``
after ``set_q`` leaves ``q_psi`` wave-free until the first step, quirk Q2), the CURRENT phi-hat for ``gradphi2``.
``flow.reference`` and the planes of one ``averages`` sample are the specification of the values.

Definition (``reference`` restates it in numpy).  F is the unnormalised full-plane 2-D DFT (``numpy.fft.fft2``), A = F[a],
B = F[b], M = nx ny:

    auto[a][s]    = sum over shell s of |A|^2 / M^2
    co[(a, b)][s] = sum over shell s of Re(conj(A) B) / M^2

Shells are ``spectra.shell_of``; every shell is kept, the partial outer ones (beyond ``k_iso_max``) included, so by Parseval the
sum over s of ``co[(a, b)]`` is the plane mean of a b, and shell 0 is mean(a) mean(b): ``covariance`` is the sum over the shells
>= 1.  The quadrature part Im(conj(A) B) is odd under k -> -k for real fields, sums to zero inside every shell and is not returned.

On the device (fused grids, Kernel family) the row pass of the PDFs holds the selected values in registers, packs them as the complex
row a + i b (and c + i 0 for a third field), transforms forward, and the column passes finish the planes; the binning kernel splits
Z = F[a + i b] into A = (Z + Z*) / 2, B = (Z - Z*) / (2i), Z* = conj Z(-l, -k) (``split_packed`` restates it).  Before packing,
every field is multiplied by the power of two that brings its largest |value| into [1, 2) (from the PDFs' range pass, on the
device), and the bins take the powers out again, both exactly: q_psi (1e-5 1/s) and |phi|^2 or ow (1e-11 1/s^2) would otherwise
share one transform's rounding and the smaller would lose digits (``packed_transforms`` restates the route).  A field that is zero
everywhere is taken out with the factor 0 instead (``unpack_scale``): its ``auto`` and every ``co`` row it is in are exactly 0.0 and
its coherence is NaN, not the round-off of its partner's transform.  No physical plane
is written or downloaded; one (6, nb) table leaves the GPU.  QGModel on the fused grids bins its state q-hat, c-hat directly.  Two
calls are bit-identical (no atomics, fixed summation order).

``Accumulator``: running sums of the raw tables on the device, in call order; ``add()`` downloads nothing and does not wait for
the device; ``result()`` returns the means, with ``n``.  A context has one pair of tables: a ``cross_spectra`` call (or another
Accumulator's ``add``) on the same model in between takes them over and the next ``add()`` raises.

Slab-decomposed models raise ``NotImplementedError``, and so does a list with a flow name at nx = 8192 (a device thread of that row
plan holds one value).  ``q``, ``q_psi``, ``phi2`` work there.
"""
import functools

import numpy as np

from . import _lib, flow, pdfs
from .spectra import shell_count, shell_modes, shell_of

MAX_FIELDS, ROWS = _lib.COSPEC_MAX_FIELDS, _lib.COSPEC_ROWS
PAIRS = ((0, 1), (0, 2), (1, 2))            # rows 3, 4, 5 of the table, after the autos of the list in order
_CODES = dict(pdfs._CODES)


def available(m):
    """names cross_spectra(m) takes for this model"""
    return pdfs.available(m) + flow.available(m)


def check(valid, names):
    """the names of a call checked against those a model takes: a list of 1 to 3 different names of ``valid``; every error is a
    ValueError, raised before anything reaches the library"""
    names = [names] if isinstance(names, str) else list(names)
    bad = [n for n in names if n not in valid]
    if bad or not names:
        raise ValueError("cross_spectra: names %r; valid names: %s" % (names, ", ".join(valid)))
    if len(set(names)) != len(names):
        raise ValueError("cross_spectra: names %r; valid: every name once" % (names,))
    if len(names) > MAX_FIELDS:
        raise ValueError("cross_spectra: %d names; valid: 1 to %d per call (the value registers of the row pass)" % (len(names), MAX_FIELDS))
    return tuple(names)


@functools.lru_cache(maxsize=2)
def shell_map(nx):
    """(nx, nx) int64, read-only: the shell of every wavenumber of the full plane in numpy.fft's layout (kept for the last two
    sizes: a reference table bins a dozen planes of one size)"""
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    out = shell_of(n[None, :], n[:, None])
    out.setflags(write=False)
    return out


def bin_shells(term, nx):
    """sum of a real (nx, nx) plane of per-wavenumber terms over every shell"""
    return np.bincount(shell_map(nx).ravel(), weights=np.asarray(term, np.float64).ravel(), minlength=shell_count(nx))


def table(transforms, nx):
    """the raw (ROWS, nb) table of the full-plane transforms of 1 to 3 fields: autos in order, then PAIRS; other rows zero"""
    out = np.zeros((ROWS, shell_count(nx)))
    for i, A in enumerate(transforms):
        out[i] = bin_shells(A.real * A.real + A.imag * A.imag, nx)
    for r, (i, j) in enumerate(PAIRS):
        if j < len(transforms):
            A, B = transforms[i], transforms[j]
            out[MAX_FIELDS + r] = bin_shells(A.real * B.real + A.imag * B.imag, nx)
    return out


def split_packed(Z):
    """A = F[a], B = F[b] from Z = F[a + i b] of two real planes: A = (Z + Z*) / 2, B = (Z - Z*) / (2i) with
    Z*(l, k) = conj Z(-l, -k), indices modulo the size (the split the binning kernel applies)"""
    Zs = np.conj(np.roll(np.roll(Z[::-1, ::-1], 1, axis=0), 1, axis=1))
    return 0.5 * (Z + Zs), -0.5j * (Z - Zs)


def bluestein_growth(nx):
    """the growth factor of ``transform_rounding`` for the any-size path's transforms (csrc/nq_anysize.hpp): per axis two
    power-of-two transforms of length L >= 2 nx - 1 and three chirp multiplies instead of one transform of length nx"""
    L = 1 << int(np.ceil(np.log2(2 * nx - 1)))
    return 2.0 * (2.0 * np.log2(L) + 3.0)


def transform_rounding(A, B, a, b, nx, growth=None, packed=False):
    """Per shell, a bound on the round-off that ANY fp64 transform route leaves in sum_shell Re(conj(A) B) / M^2 (a is b: the auto
    row), numpy's own included.  A transform's error is absolute, not relative to the coefficient: every A(l, k) / M carries about
    eps rms(a) with eps = growth 2^-53 / sqrt(M), growth = log2(M) (the classical log2(M) u bound on the 2-norm, spread over M
    coefficients; ``bluestein_growth`` for a chirp-z route), whatever |A(l, k)| is.  Over the n wavenumbers of a shell, by Cauchy-Schwarz,

        eps sqrt(n) (sqrt(S_a) rms(b) + sqrt(S_b) rms(a)) + n eps^2 rms(a) rms(b),      S_x = sum_shell |X|^2 / M^2.

    On a shell with the plane's average content per wavenumber this is 2 log2(M) 2^-53 = 4e-15 of the content; it reaches
    1e-12 of it where a wavenumber holds less than 2e-5 of the average energy (shell 0 of a mean-free field, shells a filter or
    the hyperviscosity has emptied, the shell where u and v have no wavenumber in common): there two summation orders of numpy
    itself differ by more than 1e-12 of the content (tests/test_cospectra_host.py), and a coherence means little.
    packed: the bound for the device's packed route instead, where a field shares its transform with a partner and the plane the
    transform sees has the size of the PEAKS (rms(x) is replaced by 2 sqrt 2 max |x|)."""
    M = float(A.size)
    Sa = bin_shells(A.real * A.real + A.imag * A.imag, nx) / M ** 2
    Sb = bin_shells(B.real * B.real + B.imag * B.imag, nx) / M ** 2
    return shell_sum_rounding(Sa, Sb, a, b, nx, growth, packed)


def shell_sum_rounding(Sa, Sb, a, b, nx, growth=None, packed=False):
    """``transform_rounding`` from the shell sums S_x = sum_shell |X|^2 / M^2 themselves (a square grid): for a caller that has
    them from a route without a transform of its own, such as 2 x the enstrophy spectrum for q"""
    M = float(nx) ** 2
    eps = (np.log2(M) if growth is None else float(growth)) * 2.0 ** -53 / np.sqrt(M)
    n = shell_modes(nx).astype(np.float64)
    ra, rb = float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))), float(np.sqrt(np.mean(np.asarray(b, np.float64) ** 2)))
    if packed:      # the device's packed route: a transform of s_a a + i s_b b, both peaks in [1, 2): |Z| <= 2 sqrt 2, so a / s_a sees 2 sqrt 2 max |a|
        ra, rb = 2.0 * np.sqrt(2.0) * float(np.abs(a).max()), 2.0 * np.sqrt(2.0) * float(np.abs(b).max())
    return eps * np.sqrt(n) * (np.sqrt(Sa) * rb + np.sqrt(Sb) * ra) + n * eps ** 2 * ra * rb


def pack_scale(x):
    """the power of two the device multiplies a field by before packing: 2^-e with e the binary exponent of max |x|, so the
    largest |value| lands in [1, 2); 1 for a field that is zero, subnormal throughout (2^-e would overflow) or not finite"""
    top = float(np.abs(x).max())
    if not (top >= np.finfo(np.float64).tiny and np.isfinite(top)):
        return 1.0
    return float(np.ldexp(1.0, 1 - np.frexp(top)[1]))


def unpack_scale(x):
    """the factor the bins take a field's split part out with: 1 / pack_scale(x), exactly, and 0 for a field that is zero
    everywhere: packed with a partner, the split part of a vanishing field is the round-off of the PARTNER's transform (1e-16 of
    its coefficients), which would otherwise give it a spectrum and a coherence of order one with its partner"""
    if float(np.abs(x).max()) == 0.0:
        return 0.0
    return 1.0 / pack_scale(x)


def packed_transforms(a, b):
    """F[a], F[b] of two real planes by the device's route: ONE transform of s_a a + i s_b b with the powers of two of
    ``pack_scale`` (two fields that share a transform share its rounding, a few ulp of the LARGER one's coefficients: unscaled,
    q_psi packed with |phi|^2 would lose digits in proportion to their ratio), split by ``split_packed``, the scales taken out"""
    if unpack_scale(a) == 0.0 and unpack_scale(b) != 0.0:
        # a first field that vanishes changes places with its partner: b's transform is then the one b alone gets, F[b + i 0],
        # wherever in the list the zero field stands (F[0 + i b] equals i F[b] only up to the last bit)
        B, A = packed_transforms(b, a)
        return A, B
    sa, sb = pack_scale(a), pack_scale(b)
    A, B = split_packed(np.fft.fft2(sa * np.asarray(a, np.float64) + 1j * (sb * np.asarray(b, np.float64))))
    return A * unpack_scale(a), B * unpack_scale(b)


class CrossSpectra(object):
    """shell (0..nb-1), k = shell * dk, dk, modes (full-plane wavenumbers per shell), k_iso_max = nx/2 * dk, names, n (states in
    the mean: 1 for cross_spectra), raw ((ROWS, nb): the sums of the raw tables of the n states, no 1 / M^2), auto {name: array}
    and co {(a, b): array}, both orders of every pair"""

    def __init__(self, names, raw, dk, nx, ny=None, n=1):
        nb = shell_count(nx)
        raw = np.asarray(raw, np.float64)
        if raw.shape != (ROWS, nb):
            raise ValueError("CrossSpectra: table of shape %s, expected %s" % (raw.shape, (ROWS, nb)))
        self.names, self.raw, self.n = tuple(names), raw, int(n)
        self.shell = np.arange(nb, dtype=np.int64)
        self.dk = float(dk)
        self.k = self.shell * self.dk
        self.modes = shell_modes(nx)
        self.k_iso_max = 0.5 * nx * self.dk
        scale = 1.0 / (self.n * (float(nx) * (nx if ny is None else ny)) ** 2)
        self.auto = {a: raw[i] * scale for i, a in enumerate(self.names)}
        self.co = {}
        for r, (i, j) in enumerate(PAIRS):
            if j < len(self.names):
                a, b = self.names[i], self.names[j]
                self.co[(a, b)] = self.co[(b, a)] = raw[MAX_FIELDS + r] * scale

    def __repr__(self):
        return "CrossSpectra(nb=%d, dk=%g, names=%s, n=%d)" % (len(self.shell), self.dk, list(self.names), self.n)

    def _co(self, a, b):
        for x in (a, b):
            if x not in self.auto:
                raise KeyError("cross spectra: %r is not one of the names of the call (%s)" % (x, ", ".join(self.names)))
        return self.auto[a] if a == b else self.co[(a, b)]

    def coherence(self, a, b):
        """co / sqrt(auto_a auto_b) per shell; NaN where a denominator is 0"""
        co, den = self._co(a, b), np.sqrt(self.auto[a] * self.auto[b])
        out = np.full(len(co), np.nan)
        np.divide(co, den, out=out, where=den > 0)
        return out

    def covariance(self, a, b):
        """plane covariance of a and b: the sum of co over the shells >= 1 (shell 0 is the product of the means)"""
        return float(self._co(a, b)[1:].sum())

    def correlation(self, a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.float64(self.covariance(a, b)) / np.sqrt(np.float64(self.covariance(a, a)) * np.float64(self.covariance(b, b))))


def reference(planes, nx, dk=1.0):
    """THE definition in numpy: ``planes`` {name: real (nx, nx) array}, 1 to 3 of them in the order of the call; fft2 per plane
    and ``numpy.bincount`` over ``shell_of``.  Returns the CrossSpectra."""
    names = check(list(planes), list(planes))
    return CrossSpectra(names, table([np.fft.fft2(np.asarray(planes[n], np.float64)) for n in names], nx), dk, nx)


# ---- the two backends ---------------------------------------------------------------------------------------------------------
def _validate(m, names):
    names = check(available(m), names)
    any_size = getattr(m, "_any_size", False)
    if not any_size and not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("cross_spectra: slab-decomposed models have no co-spectra yet (DESIGN.md section 7); use a single-GPU model")
    if not any_size and m.nx >= flow.ONE_VALUE_NX and any(n in flow.NAMES for n in names):
        raise NotImplementedError("cross_spectra: no flow names at nx = %d yet: a device thread of that row plan holds one value, the "
                                  "packed pair needs two (DESIGN.md section 7); q, q_psi, phi2 work" % m.nx)
    return names


def _any_size_table(m, names):
    """grids without a fused plan: the path's own planes (what its PDFs bin), transformed by the engine, multiplied element-wise
    and binned by nq_any_bin"""
    planes = m._pdf_planes(list(names))
    real = [planes[n][0].abs2() if planes[n][1] == 1 else planes[n][0] for n in names]
    half = pdfs._is_qg(m)                             # QGModel keeps half planes: weights 2 / 1 (the real fields' rffts are Hermitian)
    T = [m._rfft(r) if half else m._fft(r) for r in real]
    w = m._half_weights() if half else None
    out = np.zeros((ROWS, shell_count(m.nx)))
    for i, A in enumerate(T):
        t = A.abs2()
        out[i] = m._bin(t * w if half else t, int(half))
    for r, (i, j) in enumerate(PAIRS):
        if j < len(T):
            t = T[i].conj() * T[j]
            out[MAX_FIELDS + r] = m._bin(t * w if half else t, int(half))
    return out


def _result(m, names, raw, n=1):
    return CrossSpectra(names, raw, float(m.dk), m.nx, m.ny, n)


def cross_spectra(m, names):
    """Auto- and co-spectra of 1 to 3 physical fields of the model's current state, formed on the device.  May be called wherever
    isotropic_spectra may; reads the state and writes only buffers of its own and planes that are free between steps."""
    names = _validate(m, names)
    if getattr(m, "_any_size", False):
        return _result(m, names, _any_size_table(m, names))
    m._ctx._cospec_owner = None
    return _result(m, names, m._ctx.cospectra([_CODES[n] for n in names]))


class Accumulator(object):
    """Time means over several states: add() forms the current state's table and adds it to the running sums (on the device for
    the fused contexts: nothing is downloaded and the host does not wait; on the host for the any-size path), result() returns the
    CrossSpectra of the means with n, reset() starts over."""

    def __init__(self, m, names):
        self.m, self.names = m, _validate(m, names)
        self.any_size = bool(getattr(m, "_any_size", False))
        self.n, self.sum = 0, None

    def add(self):
        if self.any_size:
            t = _any_size_table(self.m, self.names)
            self.sum = t if self.n == 0 else self.sum + t
        else:
            ctx = self.m._ctx
            if self.n and getattr(ctx, "_cospec_owner", None) is not self:
                raise RuntimeError("Accumulator.add: the context's tables were used by another call since the last add(); reset() first")
            ctx._cospec_owner = self
            ctx.cospectra([_CODES[n] for n in self.names], accumulate=self.n > 0, download=False)
        self.n += 1

    def result(self):
        if self.n == 0:
            raise RuntimeError("Accumulator.result: nothing added yet")
        if self.any_size:
            return _result(self.m, self.names, self.sum, self.n)
        ctx = self.m._ctx
        if getattr(ctx, "_cospec_owner", None) is not self:
            raise RuntimeError("Accumulator.result: the context's tables were used by another call since the last add()")
        n, raw = ctx.cospectra_read()
        assert n == self.n, (n, self.n)
        return _result(self.m, self.names, raw, n)

    def reset(self):
        self.n, self.sum = 0, None
