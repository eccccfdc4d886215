"""Time-mean spectra, spectral transfer and flux, accumulated on the device inside the step.

    from niwqg_amd import timespectra
    T = timespectra.attach(m, spectra=True, transfer=True, every=10)
    m.run()                                   # every 10th step ends with one sample, batched nq_step(n) included
    R = T.result()                            # one download of the small tables
    R.n; R.steps; R.k; R.k_edge
    R.mean("ens"); R.mean_transfer("ens"); R.mean_flux("ens")
    R.variance("ke_qg"); R.variance_transfer("ens"); R.variance_flux("ens")
    R.raw_spectra; R.raw_transfer; R.raw_cumulative       # fused contexts: the sequential sums themselves, (32, nb), (6, nb), (6, nb)
    T.sample()                                # add the current state now
    T.reset()                                 # zero the sums and n (not the step counter)
    T.detach()

A sample is what ``spectra.isotropic_spectra(m)`` and ``transfer.spectral_transfer(m)`` are made of at that point: on a fused
context the raw shell tables of ``nq_diagnostics_binned`` (32 x nb) and ``nq_transfer_binned`` (6 x nb), bit for bit -- the same
passes on the same state, forced and re-inverted where a forcing is attached, with the quirk-Q1 gradients of UnCoupledModel and
YBJModel and the mean of the two q-hat copies of a dual-copy context -- left on the device.  With both bodies attached each of the
tick's two products passes runs once per sample and serves the two tables.  A sample is taken after every ``every``-th step since
attach (``every = 0``: never automatically), after the forcing, the particles, the recorder and the averages.  Attach itself takes
none.

The accumulation rule (``accumulate`` restates it in numpy): for every raw element x of a sample S1 <- S1 + x, S2 <- S2 + x x;
for every transfer row the running sum c[b] = sum_{b' <= b} x[b'], added in shell order one after the other as ``np.cumsum``
does, then P1 <- P1 + c, P2 <- P2 + c c.  Everything is fp64, in sample order, without atomics: two runs are bit-identical and a
first-moment table is the sequential fp64 sum exactly.  The device may contract S2 + x x into one fused multiply-add, one rounding
less per sample than numpy's, so second moments are not promised to equal numpy's bit for bit.

The named results are formed on the host from the sums: the formulas of ``spectra._named`` and ``transfer.ROWS`` applied to
S1 / n, the flux of ``name`` as -factor P1 / n, variances by the raw-moment formula S2 / n - (S1 / n)^2, which loses digits
where the mean squared is much larger than the variance.  A spectrum that is a combination of several raw rows (``ep_psi``,
``ep_phi``, ``chi_phi``, ``ep_c``, ``chi_c``) has no variance here: that needs the covariances of its rows, which are not kept.

On the any-size path a sample takes ``m._spectra`` and ``m._transfer`` after the step and the same rule is applied to the named
values on the host; ``raw_*`` are None there.
"""
import numpy as np

from . import _attach, _lib, spectra as _spectra, transfer as _transfer

SPEC_ROWS = 32
MULTI_ROW = ("ep_psi", "ep_phi", "chi_phi", "ep_c", "chi_c")      # spectra formed from more than one raw row
# the raw row of every other spectrum (spectra._named): its value is that row times a constant
SINGLE_ROW = dict(ke_qg=11, ens=6, ke_niw=0, pe_niw=1, chi_q=7, gamma_r=28, gamma_a=24, xi_r=27, xi_a=31, C2=16, gradC2=17)
TABLES = ("S1", "S2", "T1", "T2", "P1", "P2")


def tables(spec_rows, transfer_rows, nb):
    """zeroed sums: S1, S2 (spec_rows, nb), T1, T2, P1, P2 (transfer_rows, nb)"""
    out = {k: np.zeros((spec_rows, nb)) for k in ("S1", "S2")}
    out.update({k: np.zeros((transfer_rows, nb)) for k in ("T1", "T2", "P1", "P2")})
    return out


def accumulate(sums, spectra=None, transfer=None):
    """THE accumulation rule in numpy: one sample -- ``spectra`` (rows, nb) and / or ``transfer`` (rows, nb) -- added to ``sums``
    (``tables``), in place: S1 += x, S2 += x x for every element of either; per transfer row c = cumsum(x), P1 += c, P2 += c c.
    Returns ``sums``."""
    if spectra is not None:
        x = np.asarray(spectra, dtype=np.float64)
        sums["S1"] += x
        sums["S2"] += x * x
    if transfer is not None:
        x = np.asarray(transfer, dtype=np.float64)
        sums["T1"] += x
        sums["T2"] += x * x
        c = np.cumsum(x, axis=1)
        sums["P1"] += c
        sums["P2"] += c * c
    return sums


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check(spectra=True, transfer=True, every=1):
    """the arguments of ``attach``; returns (spectra, transfer, every).  Every error is a ValueError, raised before anything
    reaches the library."""
    for name, v in (("spectra", spectra), ("transfer", transfer)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("timespectra.attach: %s = %r; valid: True or False" % (name, v))
    if not (spectra or transfer):
        raise ValueError("timespectra.attach: spectra = transfer = False; valid: at least one of the two")
    if not _integer(every) or every < 0:
        raise ValueError("timespectra.attach: every = %r; valid: an integer >= 0" % (every,))
    return bool(spectra), bool(transfer), int(every)


class TimeSpectra(object):
    """What ``result()`` returns: n samples, steps since attach, shell, k = shell dk, k_edge = (shell + 1/2) dk, modes, k_iso_max
    as ``spectra.IsotropicSpectra`` has them, ``sums`` {"S1", "S2", "T1", "T2", "P1", "P2"} and the statistics formed from them.

    Fused contexts: the sums are the raw tables (``raw_spectra`` = S1, ``raw_transfer`` = T1, ``raw_cumulative`` = P1; rows as
    nq_diagnostics_binned / nq_transfer_binned) and every named result applies the tree's formula to them.  Any-size path: the
    rows of the sums are the named values themselves (``spectra_names``, ``transfer_names``) and ``raw_*`` are None.  Variances
    are raw-moment formulas, S2 / n - (S1 / n)^2: they lose digits where |mean|^2 >> variance."""

    def __init__(self, m, n, steps, sums, spectra_names, transfer_names, raw):
        nb = _spectra.shell_count(m.nx)
        self._m, self.n, self.steps, self.sums = m, n, steps, sums
        self.spectra_names, self.transfer_names, self._raw = list(spectra_names), list(transfer_names), raw
        self.shell = np.arange(nb, dtype=np.int64)
        self.dk = float(m.dk)
        self.k = self.shell * self.dk
        self.k_edge = (self.shell + 0.5) * self.dk
        self.modes = _spectra.shell_modes(m.nx)
        self.k_iso_max = 0.5 * m.nx * self.dk
        self.raw_spectra = sums["S1"] if raw and spectra_names else None
        self.raw_transfer = sums["T1"] if raw and transfer_names else None
        self.raw_cumulative = sums["P1"] if raw and transfer_names else None

    def __repr__(self):
        return "TimeSpectra(n=%d, spectra=%s, transfer=%s)" % (self.n, self.spectra_names, self.transfer_names)

    # ---- names
    def _spectrum_name(self, name):
        valid = _spectra.available(self._m)
        if name not in valid:
            raise ValueError("isotropic_spectra: %r not available for %s; valid names: %s" % (name, type(self._m).__module__, ", ".join(valid)))
        if not self.spectra_names:
            raise KeyError("timespectra: the spectra were not accumulated (attach with spectra=True)")

    def _transfer_name(self, name):
        valid = _transfer.available(self._m)
        if name not in valid:
            raise ValueError("spectral_transfer: %r not available for %s; valid names: %s" % (name, type(self._m).__module__, ", ".join(valid)))
        if not self.transfer_names:
            raise KeyError("timespectra: the transfer was not accumulated (attach with transfer=True)")

    def _M2(self):
        return (float(self._m.nx) * self._m.ny) ** 2

    def _transfer_row(self, name, first, second=None):
        """(scale, first-moment row, second-moment row) of transfer ``name`` in the tables ``first`` / ``second``"""
        if self._raw:
            row, factor = _transfer.ROWS[name]
            scale = factor
        else:
            row, scale = self.transfer_names.index(name), None
        return scale, self.sums[first][row], (self.sums[second][row] if second else None)

    # ---- first moments
    def mean(self, name):
        """time mean of the spectrum ``name`` (``spectra.available(m)``)"""
        self._spectrum_name(name)
        if self._raw:
            return _spectra._named(self._m, self.sums["S1"] / self.n, [name])[name]
        return self.sums["S1"][self.spectra_names.index(name)] / self.n

    def mean_transfer(self, name):
        """time mean of the transfer T(b) of ``name`` (``transfer.available(m)``)"""
        self._transfer_name(name)
        scale, S, _ = self._transfer_row(name, "T1")
        return S / self.n if scale is None else scale * (S / self.n) / self._M2()

    def mean_flux(self, name):
        """time mean of the flux Pi(b) = -sum_{b' <= b} T(b') of ``name`` through k_edge"""
        self._transfer_name(name)
        scale, P, _ = self._transfer_row(name, "P1")
        return -(P / self.n) if scale is None else -scale * (P / self.n) / self._M2()

    # ---- second moments
    def _var(self, S1, S2):
        mean = S1 / self.n
        return S2 / self.n - mean * mean

    def variance(self, name):
        """variance over the samples of the spectrum ``name``; ValueError for a spectrum formed from several raw rows"""
        self._spectrum_name(name)
        if name in MULTI_ROW:
            raise ValueError("timespectra: %s combines several raw rows of the tick: its variance needs the covariances of those rows, "
                             "which are not kept (variances: %s)" % (name, ", ".join(n for n in _spectra.available(self._m) if n not in MULTI_ROW)))
        if not self._raw:
            i = self.spectra_names.index(name)
            return self._var(self.sums["S1"][i], self.sums["S2"][i])
        row = SINGLE_ROW[name]
        unit = np.zeros(SPEC_ROWS)
        unit[row] = 1.0
        c = float(_spectra._named(self._m, unit, [name])[name])          # the constant of the formula
        return c * c * self._var(self.sums["S1"][row], self.sums["S2"][row])

    def variance_transfer(self, name):
        """variance over the samples of the transfer of ``name``"""
        self._transfer_name(name)
        scale, S1, S2 = self._transfer_row(name, "T1", "T2")
        c = 1.0 if scale is None else scale / self._M2()
        return c * c * self._var(S1, S2)

    def variance_flux(self, name):
        """variance over the samples of the flux of ``name``"""
        self._transfer_name(name)
        scale, P1, P2 = self._transfer_row(name, "P1", "P2")
        c = 1.0 if scale is None else scale / self._M2()
        return c * c * self._var(P1, P2)


class Accumulator(_attach.Attachment):
    """Time-mean spectra attached to one model (``attach``); see the module's doc"""
    SLOT, LABEL = "_timespectra", "timespectra"
    ALREADY = (RuntimeError, "timespectra.attach: this model has time-mean spectra attached already (detach them first)")
    NO_SLAB = ("timespectra.attach: slab-decomposed models have no time-mean spectra yet (every rank would sum the shells of the "
               "columns it owns and the tables would be added in rank order at read-out; DESIGN.md section 7)")

    def __init__(self, m, spectra, transfer, every):
        self.m, self.spectra, self.transfer, self.every = m, spectra, transfer, every

    def info(self):
        """{"n": samples in the sums, "steps": steps since attach}"""
        self._check()
        n, steps = self._info()
        return {"n": n, "steps": steps}

    def sample(self):
        """adds the current state to the sums now"""
        self._check()
        self._sample()

    def reset(self):
        """zeroes the sums and n; the step counter (and so the phase of ``every``) stays"""
        self._check()
        self._reset()

    def result(self):
        """One download of the tables -> TimeSpectra (n, steps, the sums and the statistics formed from them on the host)"""
        self._check()
        n, steps = self._info()
        if n == 0:
            raise RuntimeError("timespectra.result: no sample taken yet")
        sums, snames, tnames, raw = self._read()
        return TimeSpectra(self.m, n, steps, sums, snames, tnames, raw)


class _Fused(Accumulator):
    """fused contexts: the tables live in the library and nq_step adds to them (nq_tspec_*)"""

    def __init__(self, m, spectra, transfer, every):
        Accumulator.__init__(self, m, spectra, transfer, every)
        self.ctx = m._ctx
        self.ctx.tspec_attach((_lib.TSPEC_SPECTRA if spectra else 0) | (_lib.TSPEC_TRANSFER if transfer else 0), every)

    def _info(self):
        return self.ctx.tspec_info()[:2]

    def _sample(self):
        self.ctx.tspec_sample()

    def _reset(self):
        self.ctx.tspec_reset()

    def _read(self):
        sums = {k: self.ctx.tspec_read(getattr(_lib, "TSPEC_" + k)) for k in TABLES}
        return (sums, _spectra.available(self.m) if self.spectra else [], _transfer.available(self.m) if self.transfer else [], True)

    def _detach(self):
        self.ctx.tspec_detach()


class _AnySize(Accumulator):
    """any-size path: the model's _step_etdrk4 calls _after_step; a sample takes the named spectra and transfers the path forms
    (m._spectra, m._transfer) and adds them to host tables whose rows are those names"""

    def __init__(self, m, spectra, transfer, every):
        Accumulator.__init__(self, m, spectra, transfer, every)
        self.snames = _spectra.available(m) if spectra else []
        self.tnames = _transfer.available(m) if transfer else []
        self.rg = _attach.Ring(1, every)
        self.sums = self._zero()

    def _zero(self):
        return tables(len(self.snames), len(self.tnames), _spectra.shell_count(self.m.nx))

    def _info(self):
        return self.rg.count, self.rg.steps

    def _sample(self):
        s = t = None
        if self.snames:
            v = self.m._spectra(self.snames)
            s = np.array([v[n] for n in self.snames], dtype=np.float64)
        if self.tnames:
            v = self.m._transfer(self.tnames)
            t = np.array([v[n] for n in self.tnames], dtype=np.float64)
        accumulate(self.sums, s, t)
        self.rg.count += 1

    def _after_step(self):
        if self.rg.tick():
            self._sample()

    def _reset(self):
        self.sums = self._zero()
        self.rg.count = 0

    def _read(self):
        return {k: v.copy() for k, v in self.sums.items()}, self.snames, self.tnames, False

    def _detach(self):
        self.sums = None


def attach(m, spectra=True, transfer=True, every=1):
    """Attach running sums of the spectra and / or the spectral transfer to model m (one set per model), zero at attach, a sample
    after every ``every``-th step (0: only ``sample()``).  The tables are (2 x 32 + 4 x 6) x nb doubles, under 5 MB at 8192^2.
    Argument errors raise ValueError before the device is touched, a second attach RuntimeError, slab-decomposed models
    NotImplementedError."""
    spectra, transfer, every = check(spectra, transfer, every)
    return _attach.attach(m, _AnySize, _Fused, spectra, transfer, every)
