"""Lagrangian frequency spectra, velocity autocovariance and dispersion of the particle records, formed on the device
(DESIGN.md section 5r).

    from niwqg_amd import particles, lagrangian
    P = particles.attach(m, x, y, record_every=4, capacity=1024, record=("u", "v", "phi"))
    m.run()
    S = lagrangian.spectrum(P, groups=labels)           # .omega (F,), .values {"uv": (F, G), "phi": (F, G)}, .counts (G,)
    R = lagrangian.autocovariance(P, "uv")              # .lag (K + 1,), .values (K + 1,); R.diffusivity()
    D = lagrangian.dispersion(P, pairs=(i, j))          # .t (T,), .A2, .D2, ...; D.kurtosis(), D.pair_kurtosis()
    S = lagrangian.stretching(P, groups=labels)         # stretch mode: .mean_lnsigma, .var_lnsigma, .mean_det, .var_det; S.ftle()
    lam = lagrangian.ftle(P)                            # (n,) ln sigma_1 / (t - t0) of every particle now

Only the small tables leave the device; ``P.trajectory()``, which downloads the whole ring, is not called.

With the T >= 2 held records of a series x_n(i) (particle i, record n, oldest first), Delta = record_every dt and a real window w_n:

    X_p(i) = sum_n w_n x'_n(i) e^{+2 pi i p n / F},     x' = x minus the particle's own time mean (``demean``), or x
    P(p, g) = 1/2 sum_{i in group g} |X_p(i)|^2 / (count_g F sum w^2),      omega_p = 2 pi fftfreq(F, Delta), sorted ascending

F = ``nfft`` >= T (default T; the records are followed by zeros).  The convention is ``frequency.py``'s: a series turning as
e^{-i omega t} appears at +omega.  By Parseval sum_p P(p, g) is the group mean of 1/2 sum_n w_n^2 |x'_n|^2 / sum_n w_n^2.  Series:
"q", "u", "v", "uw", "vw" (real), "phi" (complex), "uv" (u + i v: the rotary spectrum) -- whatever was recorded -- and, with the
wave velocity columns of section 5s, "uvw" (uw + i vw) and "uvt" ((u + uw) + i (v + vw): what a drifter's rotary spectrum shows).

    R(k) = mean_i (T - k)^-1 sum_n conj(x'_n(i)) x'_{n+k}(i),  k = 0 .. max_lag        (the unbiased autocovariance)

comes from the same device pass with a boxcar window and F = 2 T, and a transform of the small table on the host.

Dispersion, with d = r_n(i) - r_0(i) of the unwrapped positions, per record n and group: the means of dx, dy, A_xx = <dx^2>, A_yy,
A_xy, A2 = A_xx + A_yy and <|d|^4>; with pairs (i, j) and s = r_n(i) - r_n(j): D_xx = <sx^2>, D_yy, D_xy, D2 = <|s|^2>, <|s|^4>.

Stretching (stretch mode of the particles; "f11", "f12", "f21", "f22" recorded): per record and group the mean
and the variance (the mean square minus the squared mean) of ln sigma_1, the ln of the largest singular value of the deformation
gradient F, and of det F; ``ftle()`` = <ln sigma_1> / (t - t0), t0 the time F was last the identity (the attach, or the last
``P.reset_deformation()``; every held record must be later than that reset).  These are no series of ``spectrum``.

A particle whose coordinate went non-finite has NaN records (section 5g); the tables of its group are NaN.  An empty group has
count 0 and NaN tables.  ``reference_spectrum``, ``reference_autocovariance`` and ``reference_dispersion`` are the same definitions
in numpy on a ``particles.Trajectory``.
"""
import numpy as np

from . import frequency

SERIES = ("u", "v", "q", "phi", "uv", "uw", "vw", "uvw", "uvt")       # ids of the library (include/niwqg_amd.h: nq_lagr_spectrum)
COMPOSITES = {"uv": ("u", "v"), "uvw": ("uw", "vw"), "uvt": ("u", "v", "uw", "vw")}      # the columns a composite is made of
REAL = ("u", "v", "q", "uw", "vw")
MAX_GROUPS = 256


# ---- checks that need no model and no library (the CPU tests drive them) -----------------------------------------------------
def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def available(record):
    """series names the recorded columns give: the columns themselves, "uv" first in place of u and v when both are there,
    likewise "uvw" in place of uw and vw, and "uvt" when all four are; the columns of ray mode ("k", "l", "zeta", "omega":
    particles.py) are no series here"""
    record = list(record)
    made = [c for c in ("uv", "uvw", "uvt") if all(n in record for n in COMPOSITES[c])]
    used = set(n for c in made for n in COMPOSITES[c])
    return made + [n for n in record if n not in used and n in SERIES]


def check_names(record, names, what="spectrum"):
    """``names`` (None: ``available(record)``) as a list, each one a recorded column or a composite ("uv", "uvw", "uvt") with all
    its columns recorded"""
    if names is None:
        names = available(record)
    names = [names] if isinstance(names, str) else list(names)
    if not names:
        raise ValueError("lagrangian.%s: no names; recorded: %s" % (what, ", ".join(record) or "nothing"))
    for n in names:
        if n == "uv":
            if "u" not in record or "v" not in record:
                raise ValueError("lagrangian.%s: 'uv' needs both 'u' and 'v' recorded; recorded: %s" % (what, ", ".join(record) or "nothing"))
        elif isinstance(n, str) and n in COMPOSITES:
            if any(c not in record for c in COMPOSITES[n]):
                raise ValueError("lagrangian.%s: %r needs %s recorded; recorded: %s"
                                 % (what, n, " and ".join(repr(c) for c in COMPOSITES[n]), ", ".join(record) or "nothing"))
        elif n not in SERIES:
            raise ValueError("lagrangian.%s: unknown name %r; valid names: %s" % (what, n, ", ".join(SERIES)))
        elif n not in record:
            raise ValueError("lagrangian.%s: %r is not recorded; recorded: %s" % (what, n, ", ".join(record) or "nothing"))
    return names


def check_records(record_every, held, what="spectrum"):
    if record_every <= 0:
        raise ValueError("lagrangian.%s: the particles were attached with record_every = 0" % what)
    if held < 2:
        raise ValueError("lagrangian.%s: %d record held (at least 2)" % (what, held))
    return int(held)


def check_window(window, T):
    """the window as T float64 values: "boxcar", "hann" (periodic) or T finite reals: frequency.py's rule"""
    return frequency.check_window(window, T, "lagrangian.spectrum")


def check_nfft(nfft, T):
    """the transform length: T by default, any length from T to 8192, or 16384 (what the any-length transform takes)"""
    if nfft is None:
        nfft = T
    if not _integer(nfft) or nfft < T:
        raise ValueError("lagrangian.spectrum: nfft = %r (an integer >= T = %d)" % (nfft, T))
    if nfft > 8192 and nfft != 16384:
        raise ValueError("lagrangian.spectrum: nfft = %d (the transform takes lengths up to 8192, and 16384)" % nfft)
    return int(nfft)


def check_groups(groups, n, what="spectrum"):
    """(order, offsets, counts, G): the stable-sorted index list of the labels -- group g is order[offsets[g]:offsets[g + 1]] --
    from n integer labels in [0, G); G = max label + 1, at most 256.  None: one group of everything."""
    if groups is None:
        return np.arange(n, dtype=np.int32), np.array([0, n], np.int32), np.array([n], np.int64), 1
    g = np.asarray(groups)
    if g.shape != (n,) or g.dtype.kind not in "iu":
        raise ValueError("lagrangian.%s: groups must be %d integer labels (got shape %s, dtype %s)" % (what, n, g.shape, g.dtype))
    g = g.astype(np.int64)
    if g.min() < 0 or g.max() >= MAX_GROUPS:
        raise ValueError("lagrangian.%s: group labels must lie in [0, %d) (got %d .. %d)" % (what, MAX_GROUPS, g.min(), g.max()))
    G = int(g.max()) + 1
    counts = np.bincount(g, minlength=G).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return np.argsort(g, kind="stable").astype(np.int32), offsets, counts, G


def check_pairs(pairs, n):
    """(i, j) as int32 arrays of equal length, indices in [0, n), i != j; None stays None"""
    if pairs is None:
        return None
    try:
        i, j = pairs
        i, j = np.asarray(i), np.asarray(j)
    except (TypeError, ValueError):
        raise ValueError("lagrangian.dispersion: pairs must be two integer arrays (i, j)")
    if i.ndim != 1 or i.shape != j.shape or i.size < 1 or i.dtype.kind not in "iu" or j.dtype.kind not in "iu":
        raise ValueError("lagrangian.dispersion: pairs must be two integer arrays of one length >= 1 (got %s %s, %s %s)"
                         % (i.shape, i.dtype, j.shape, j.dtype))
    if min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= n:
        raise ValueError("lagrangian.dispersion: a pair index lies outside [0, %d)" % n)
    if np.any(i == j):
        raise ValueError("lagrangian.dispersion: a pair names one particle twice (i = j)")
    return np.ascontiguousarray(i, np.int32), np.ascontiguousarray(j, np.int32)


def check_max_lag(max_lag, T):
    if max_lag is None:
        return T - 1
    if not _integer(max_lag) or not 0 <= max_lag <= T - 1:
        raise ValueError("lagrangian.autocovariance: max_lag = %r (an integer, 0 <= max_lag <= T - 1 = %d)" % (max_lag, T - 1))
    return int(max_lag)


def _omega(F, dt_rec):
    f = np.fft.fftfreq(F, float(dt_rec))
    order = np.argsort(f, kind="stable")
    return order, 2.0 * np.pi * f[order]


def _per_group(sums, counts, grouped):
    """sums (..., G) over each group -> means; an empty group: NaN.  Without groups the last axis goes."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = sums / np.where(counts > 0, counts, np.nan)
    return out if grouped else out[..., 0]


def _autocov_from_table(sums, counts, T, K, real, grouped):
    """R(k), k = 0..K, from the (2T, G) boxcar table of sums S(p, g) = 1/2 sum_i |X_p|^2 / (2T T) in FFT order:
    sum_p |X_p|^2 e^{-2 pi i p k / F} = F sum_n conj(x_n) x_{n+k}  (F = 2T: the zeros keep the lags apart)"""
    C = 2.0 * T * np.fft.fft(sums, axis=0)[:K + 1]
    C = C / (T - np.arange(K + 1))[:, None]
    R = _per_group(C, counts, grouped)
    return np.ascontiguousarray(R.real) if real else R


# ---- the public objects ----------------------------------------------------------------------------------------------------
class LagrangianSpectra(object):
    """omega (F,) ascending, values {name: (F,) or (F, G) float64}, counts (G,) particles per group, step (T,) of the records"""

    def __init__(self, omega, values, counts, step):
        self.omega, self.values, self.counts, self.step = omega, values, counts, step

    def __repr__(self):
        return "LagrangianSpectra(F=%d, G=%d, names=%s)" % (len(self.omega), len(self.counts), sorted(self.values))


class Autocovariance(object):
    """lag (K + 1,) in time units, values (K + 1,) or (K + 1, G): float64 for a real series, complex128 for "phi", "uv", "uvw", "uvt";
    counts (G,)"""

    def __init__(self, name, lag, values, counts):
        self.name, self.lag, self.values, self.counts = name, lag, values, counts

    def diffusivity(self):
        """the cumulative trapezoid of Re R over the lag: int_0^tau R for a real series, 1/2 int_0^tau Re R for "uv" (and "phi"),
        so that a velocity's is the single-component diffusivity either way; [0] = 0"""
        r = np.real(self.values) * (1.0 if self.name in REAL else 0.5)
        d = np.diff(self.lag)
        d = d.reshape((-1,) + (1,) * (r.ndim - 1))
        out = np.zeros_like(r)
        out[1:] = np.cumsum(0.5 * (r[1:] + r[:-1]) * d, axis=0)
        return out


class Dispersion(object):
    """per record (T,) or per record and group (T, G): dx, dy (mean displacement), A_xx, A_yy, A_xy, A2, M4 = <|d|^4>; with pairs,
    per record (T,): D_xx, D_yy, D_xy, D2, S4 = <|s|^4> (else None); t, step (T,), counts (G,), npairs"""

    def __init__(self, t, step, counts, single, pair, npairs, grouped):
        self.t, self.step, self.counts, self.npairs = t, step, counts, npairs
        m = _per_group(np.moveaxis(single, 1, 2), counts, grouped)          # (T, 6, G) -> means
        self.dx, self.dy, self.A_xx, self.A_yy, self.A_xy, self.M4 = (np.ascontiguousarray(m[:, k]) for k in range(6))
        self.A2 = self.A_xx + self.A_yy
        self.D_xx = self.D_yy = self.D_xy = self.D2 = self.S4 = None
        if pair is not None:
            self.D_xx, self.D_yy, self.D_xy, self.D2, self.S4 = (pair[:, k] / npairs for k in range(5))

    def kurtosis(self):
        """<|d|^4> / <|d|^2>^2 of the displacements (NaN where A2 = 0: the first record)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.M4 / self.A2 ** 2

    def pair_kurtosis(self):
        """<|s|^4> / <|s|^2>^2 of the pair separations"""
        if self.D2 is None:
            raise ValueError("lagrangian.dispersion: no pairs were given")
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.S4 / self.D2 ** 2


# ---- the device passes ---------------------------------------------------------------------------------------------------------
def _records(P, what):
    """(T, steps since attach (T,)) of the held records after the checks that need the particles"""
    P._check()
    T = check_records(P.record_every, P._held(), what)
    return T, P._record_steps()


def spectrum(P, names=None, window="hann", demean=True, groups=None, nfft=None, chunk=0):
    """Lagrangian frequency spectra of the recorded series of particles ``P``, per group; see the module's doc.  ``chunk``: the
    particles per pass through the work plane (0: the library's rule).  Argument errors raise ValueError before the device is
    touched."""
    T, step = _records(P, "spectrum")
    names = check_names(P.record, names)
    w = check_window(window, T)
    F = check_nfft(nfft, T)
    order, offsets, counts, G = check_groups(groups, P.n)
    if not _integer(chunk) or chunk < 0:
        raise ValueError("lagrangian.spectrum: chunk = %r (an integer >= 0)" % (chunk,))
    perm, omega = _omega(F, P.record_every * float(P.m.dt))
    values = {}
    for n in names:
        sums = P._lagr_spectrum(n, T, F, w, bool(demean), G, order, offsets, int(chunk))
        values[n] = _per_group(sums, counts, groups is not None)[perm]
    return LagrangianSpectra(omega, values, counts, step + P.tc0)


def autocovariance(P, name, max_lag=None, demean=True, groups=None, chunk=0):
    """the unbiased autocovariance R(k), k = 0..max_lag (default T - 1), of one recorded series, per group; see the module's doc"""
    T, _ = _records(P, "autocovariance")
    name, = check_names(P.record, [name] if isinstance(name, str) else name, "autocovariance")
    K = check_max_lag(max_lag, T)
    check_nfft(2 * T, T)
    order, offsets, counts, G = check_groups(groups, P.n, "autocovariance")
    sums = P._lagr_spectrum(name, T, 2 * T, np.ones(T), bool(demean), G, order, offsets, int(chunk))
    R = _autocov_from_table(sums, counts, T, K, name in REAL, groups is not None)
    return Autocovariance(name, np.arange(K + 1) * (P.record_every * float(P.m.dt)), R, counts)


def dispersion(P, pairs=None, groups=None):
    """absolute dispersion per group and, with ``pairs = (i, j)``, relative dispersion of those pairs, at every held record
    relative to the oldest; see the module's doc"""
    T, step = _records(P, "dispersion")
    order, offsets, counts, G = check_groups(groups, P.n, "dispersion")
    pairs = check_pairs(pairs, P.n)
    single, pair = P._lagr_dispersion(T, G, order, offsets, pairs)
    return Dispersion(P._times(step), step + P.tc0, counts, single, pair, 0 if pairs is None else len(pairs[0]), groups is not None)


class Stretching(object):
    """per record (T,) or per record and group (T, G): mean_lnsigma, var_lnsigma, mean_det, var_det; t, step (T,), t0 the time at
    which F was last set, counts (G,)"""

    def __init__(self, t, step, t0, counts, sums, grouped):
        self.t, self.step, self.t0, self.counts = t, step, t0, counts
        m = _per_group(np.moveaxis(sums, 1, 2), counts, grouped)            # (T, 4, G) -> means
        self.mean_lnsigma, ms, self.mean_det, md = (np.ascontiguousarray(m[:, k]) for k in range(4))
        self.var_lnsigma = ms - self.mean_lnsigma ** 2
        self.var_det = md - self.mean_det ** 2

    def ftle(self):
        """<ln sigma_1> / (t - t0), the finite-time Lyapunov exponent of each group; NaN at t = t0"""
        T = (self.t - self.t0).reshape((-1,) + (1,) * (self.mean_lnsigma.ndim - 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(T != 0.0, self.mean_lnsigma / np.where(T != 0.0, T, np.nan), np.nan)


STRETCH_COLUMNS = ("f11", "f12", "f21", "f22")


def _stretch_t0(P):
    """the time of the particle step at which F was last set, on the clock of ``trajectory().t``"""
    return float(P._times(np.array([P.stretch_step0], np.int64))[0])


def stretching(P, groups=None):
    """stretching statistics of stretch mode per group at every held record, from the device tables alone; see the module's doc"""
    P._check()
    if not getattr(P, "stretch", False):
        raise ValueError("lagrangian.stretching: the particles were attached without stretch=")
    T, step = _records(P, "stretching")
    if any(c not in P.record for c in STRETCH_COLUMNS):
        raise ValueError("lagrangian.stretching: needs %s recorded; recorded: %s" % (", ".join(map(repr, STRETCH_COLUMNS)), ", ".join(P.record) or "nothing"))
    order, offsets, counts, G = check_groups(groups, P.n, "stretching")
    sums = P._lagr_stretching(T, G, order, offsets)
    return Stretching(P._times(step), step + P.tc0, _stretch_t0(P), counts, sums, groups is not None)


def ftle(P):
    """ln sigma_1 / (t - t0) of every particle now, (n,), from one ``sample(("lnsigma",))``; NaN at t = t0"""
    P._check()
    if not getattr(P, "stretch", False):
        raise ValueError("lagrangian.ftle: the particles were attached without stretch=")
    ls = P.sample(("lnsigma",))["lnsigma"]
    steps = P._steps_now()
    dt = float(P._times(np.array([steps], np.int64))[0]) - _stretch_t0(P)
    return ls / dt if dt != 0.0 else np.full_like(ls, np.nan)


def reference_stretching(tr, groups=None):
    """``stretching`` in numpy on a ``particles.Trajectory`` that holds the four f-columns: a dict of mean_lnsigma, var_lnsigma,
    mean_det, var_det, each (T,) or (T, G), and counts"""
    from . import particles
    v = tr.values
    F = np.stack([np.stack([v["f11"], v["f12"]], -1), np.stack([v["f21"], v["f22"]], -1)], -2)          # (T, n, 2, 2)
    T, n = F.shape[:2]
    order, offsets, counts, G = check_groups(groups, n, "reference_stretching")
    ls, dt = particles.ln_sigma(F), particles.det(F)
    out = {}
    for key, a in (("mean_lnsigma", ls), ("ms", ls * ls), ("mean_det", dt), ("md", dt * dt)):
        sums = np.zeros((T, G))
        for g in range(G):
            sums[:, g] = a[:, order[offsets[g]:offsets[g + 1]]].sum(axis=1)
        out[key] = _per_group(sums, counts, groups is not None)
    out["var_lnsigma"] = out.pop("ms") - out["mean_lnsigma"] ** 2
    out["var_det"] = out.pop("md") - out["mean_det"] ** 2
    out["counts"] = counts
    return out


# ---- the same definitions in numpy, on a downloaded trajectory (tests use them) -----------------------------------------------------
def _compose(tr, name):
    if name == "uv":
        if "u" not in tr.values or "v" not in tr.values:
            raise ValueError("lagrangian: 'uv' needs both 'u' and 'v' in the trajectory")
        return tr.values["u"] + 1j * tr.values["v"]
    if isinstance(name, str) and name in COMPOSITES:
        if any(c not in tr.values for c in COMPOSITES[name]):
            raise ValueError("lagrangian: %r needs %s in the trajectory" % (name, " and ".join(repr(c) for c in COMPOSITES[name])))
        v = tr.values
        return v["uw"] + 1j * v["vw"] if name == "uvw" else (v["u"] + v["uw"]) + 1j * (v["v"] + v["vw"])
    if name not in tr.values:
        raise ValueError("lagrangian: %r is not in the trajectory; it holds: %s" % (name, ", ".join(sorted(tr.values))))
    return np.asarray(tr.values[name])


def _dt_rec(tr, dt_rec):
    return (tr.t[-1] - tr.t[0]) / (len(tr.t) - 1) if dt_rec is None else float(dt_rec)


def _transform(y, F):
    """X_p = sum_n y_n e^{+2 pi i p n / F}, p = 0..F-1, along axis 0 of y (T <= F rows); extended precision by the definition"""
    T = y.shape[0]
    if y.dtype != np.clongdouble:
        return F * np.fft.ifft(y, n=F, axis=0)
    pn = (np.arange(F)[:, None] * np.arange(T)[None, :]) % F                 # the angle reduced exactly
    a = 2 * np.arccos(np.longdouble(-1)) * pn.astype(np.longdouble) / F        # (np.pi is a double)
    return np.tensordot(np.cos(a) + 1j * np.sin(a), y, axes=(1, 0))


def reference_spectrum(tr, name, window="hann", demean=True, groups=None, nfft=None, dt_rec=None):
    """``spectrum`` in numpy on a ``particles.Trajectory``: returns (omega (F,), P (F,) or (F, G), counts (G,)).  ``dt_rec``: the
    time between records (default: from ``tr.t``).  A series of ``longdouble`` / ``clongdouble`` is worked in extended precision
    throughout, with a direct DFT."""
    x = _compose(tr, name)
    ext = x.dtype in (np.longdouble, np.clongdouble)
    real = np.longdouble if ext else np.float64
    x = x.astype(np.clongdouble if ext else np.complex128)
    T, n = x.shape
    check_records(1, T, "reference_spectrum")
    w = check_window(window, T).astype(real)
    F = check_nfft(nfft, T)
    order, offsets, counts, G = check_groups(groups, n, "reference_spectrum")
    if demean:
        x = x - x.mean(axis=0)[None]
    X = _transform(w[:, None] * x, F)
    a = X.real ** 2 + X.imag ** 2
    sums = np.zeros((F, G), real)
    for g in range(G):
        sums[:, g] = a[:, order[offsets[g]:offsets[g + 1]]].sum(axis=1)
    sums *= real(0.5) / (F * (w * w).sum())
    perm, omega = _omega(F, _dt_rec(tr, dt_rec))
    return omega, _per_group(sums, counts, groups is not None)[perm], counts


def reference_autocovariance(tr, name, max_lag=None, demean=True, groups=None, dt_rec=None):
    """``autocovariance`` in numpy by its definition, the direct sums: returns (lag (K + 1,), R (K + 1,) or (K + 1, G), counts)"""
    x = _compose(tr, name)
    isreal = not np.iscomplexobj(x)
    x = x.astype(np.complex128)
    T, n = x.shape
    check_records(1, T, "reference_autocovariance")
    K = check_max_lag(max_lag, T)
    order, offsets, counts, G = check_groups(groups, n, "reference_autocovariance")
    if demean:
        x = x - x.mean(axis=0)[None]
    per = np.array([(np.conj(x[:T - k]) * x[k:]).sum(axis=0) / (T - k) for k in range(K + 1)])       # (K + 1, n)
    sums = np.zeros((K + 1, G), np.complex128)
    for g in range(G):
        sums[:, g] = per[:, order[offsets[g]:offsets[g + 1]]].sum(axis=1)
    R = _per_group(sums, counts, groups is not None)
    return np.arange(K + 1) * _dt_rec(tr, dt_rec), (np.ascontiguousarray(R.real) if isreal else R), counts


def reference_dispersion(tr, pairs=None, groups=None):
    """``dispersion`` in numpy: a dict of the arrays of ``Dispersion`` (dx, dy, A_xx, A_yy, A_xy, A2, M4; with pairs D_xx, D_yy,
    D_xy, D2, S4), each (T,) or (T, G), and counts"""
    x, y = np.asarray(tr.x, np.float64), np.asarray(tr.y, np.float64)
    T, n = x.shape
    check_records(1, T, "reference_dispersion")
    order, offsets, counts, G = check_groups(groups, n, "reference_dispersion")
    pairs = check_pairs(pairs, n)
    dx, dy = x - x[0][None], y - y[0][None]
    terms = dict(dx=dx, dy=dy, A_xx=dx * dx, A_yy=dy * dy, A_xy=dx * dy, M4=(dx * dx + dy * dy) ** 2)
    out = {}
    for key, v in terms.items():
        sums = np.zeros((T, G))
        for g in range(G):
            sums[:, g] = v[:, order[offsets[g]:offsets[g + 1]]].sum(axis=1)
        out[key] = _per_group(sums, counts, groups is not None)
    out["A2"] = out["A_xx"] + out["A_yy"]
    if pairs is not None:
        i, j = pairs
        sx, sy = x[:, i] - x[:, j], y[:, i] - y[:, j]
        r2 = sx * sx + sy * sy
        out.update(D_xx=(sx * sx).mean(axis=1), D_yy=(sy * sy).mean(axis=1), D_xy=(sx * sy).mean(axis=1), D2=r2.mean(axis=1),
                   S4=(r2 * r2).mean(axis=1))
    out["counts"] = counts
    return out
