"""PDFs of the field increments, binned on the device per separation.

    from niwqg_amd import increments
    P = increments.pdfs(m, names=("u", "v", "q_psi"), separations=None, bins=256, ranges=None, width=8.0)
    P.r, P.x                     # separations in grid points and in length
    P.counts["u"]                # (nsep, bins) int64;  P.edges["u"] (nsep, bins + 1);  P.below / P.above / P.nan ["u"]: (nsep,) int64
    z, p = P.standardised("u")   # centres / sigma_r and density * sigma_r: the curves one plots together on a semilog axis
    P.moment("u", 4), P.flatness("u"), P.tail("u", 4.0)
    A = increments.Accumulator(m, ("u", "phi"), separations=[1, 2, 4, 8]); A.add(); ...; A.result(); A.reset(); A.ranges
    P2 = increments.pdfs2d(m, names=("u", "v"), vectors=None, project=("u", "v"))
    P2.vectors, P2.length, P2.angle; P2.along("y"); r, counts, nvec = P2.isotropic("u")

The increments are those of ``structure``: d_r a(x, y) = a((x + r) mod nx, y) - a(x, y), or at a lattice vector (r_x, r_y) for
``pdfs2d``, where the ``project`` pair is first rotated onto the separation vector exactly as ``structure.functions2d`` rotates
it (``structure.unit_vectors``, d_L = c_x d_a + c_y d_b, d_T = -c_y d_a + c_x d_b).  A real name is binned signed, ``"phi"`` as
|d phi| over [0, hi].  Names, their number per call and every refusal are ``structure``'s.

Ranges are per (separation, name), since sigma_r varies by orders of magnitude over the separations.  ``ranges=None``: a range pass
on the device forms <d> and <d^2> of the current state; the range is +-width sqrt<d^2> ([0, width sqrt<|d phi|^2>] for ``"phi"``),
or (-1, 1) ([0, 1]) where <d^2> is zero or not finite.  Explicit: ``{name: (lo, hi)}`` for every separation or ``{name: array
(nsep, 2)}``.  The bin rule is ``pdfs.bin_index``; the edges are lo + (hi - lo) arange(bins + 1) / bins of the very lo, hi handed
to the device.  Counts are integers: two calls on one state return the same tables.

``reference`` is the specification in numpy (``structure.increments``, ``structure.increments2d``, ``pdfs.bin_index``).
"""
import ctypes

import numpy as np

from . import _lib, structure
from . import pdfs as _pdfs

MAX_BINS = _lib.IPDF_MAX_BINS
PHI = structure.PHI
_CODES = structure._CODES


def _check_bins(bins, what):
    if not (isinstance(bins, (int, np.integer)) and 1 <= bins <= MAX_BINS):
        raise ValueError("%s: bins = %r; valid: 1 to %d (the LDS tables of a workgroup)" % (what, bins, MAX_BINS))
    return int(bins)


def _check_width(width, what):
    width = float(width)
    if not (np.isfinite(width) and width > 0):
        raise ValueError("%s: width = %r; valid: a positive number (the range is width sigma_r)" % (what, width))
    return width


def _check_ranges(names, n, ranges, what):
    """{name: (n, 2) float64} of the names that have an explicit range; every ValueError before any device call"""
    out = {}
    for name, r in dict(ranges or {}).items():
        if name not in names:
            raise ValueError("%s: ranges given for %r; the binned names are %s" % (what, name, ", ".join(names)))
        try:
            r = np.array(r, np.float64)
        except Exception:
            raise ValueError("%s: range of %r must be (lo, hi) or an array (%d, 2), got %r" % (what, name, n, r)) from None
        if r.shape == (2,):
            r = np.tile(r, (n, 1))
        if r.shape != (n, 2):
            raise ValueError("%s: range of %r has shape %r; valid: (lo, hi), or one pair per row: (%d, 2)" % (what, name, r.shape, n))
        if not np.all(np.isfinite(r)) or not np.all(r[:, 0] < r[:, 1]):
            raise ValueError("%s: range of %r must be finite with lo < hi in every row, got %r" % (what, name, r.tolist()))
        out[name] = r
    return out


def auto_ranges(names, sums, points, width):
    """the default ranges from the range pass: sums (n, names, 2) = (sum d, sum d^2) per row and name (``"phi"``: sum |d phi|, sum
    |d phi|^2) of ``points`` points -> {name: (n, 2)}"""
    out = {}
    for i, name in enumerate(names):
        m2 = np.asarray(sums[:, i, 1], np.float64) / float(points)
        ok = np.isfinite(m2) & (m2 > 0)
        with np.errstate(invalid="ignore"):
            top = np.where(ok, width * np.sqrt(np.where(ok, m2, 1.0)), 1.0)
        out[name] = np.stack([np.zeros_like(top) if name == PHI else -top, top], axis=1)
    return out


def _edges(r, bins):
    lo, hi = r[:, :1], r[:, 1:]
    return lo + (hi - lo) * np.arange(bins + 1) / bins


class IncrementPDFs(object):
    """names, r (separations in grid points), x = r dx (None without a grid spacing); per name: counts (nsep, bins) int64, edges
    (nsep, bins + 1), below / above / nan (nsep,) int64, ranges (nsep, 2); samples: states added, points: nx ny"""

    def __init__(self, names, r, tab, ranges, samples, points, dx=None):
        self.names, self.r = list(names), None if r is None else np.asarray(r, np.int64)
        tab = np.asarray(tab).astype(np.int64)
        self.bins = tab.shape[2] - 3
        self.samples, self.points = int(samples), int(points)
        self.ranges = {n: np.array(ranges[n], np.float64) for n in self.names}
        self.counts = {n: tab[:, i, :self.bins].copy() for i, n in enumerate(self.names)}
        self.below = {n: tab[:, i, self.bins].copy() for i, n in enumerate(self.names)}
        self.above = {n: tab[:, i, self.bins + 1].copy() for i, n in enumerate(self.names)}
        self.nan = {n: tab[:, i, self.bins + 2].copy() for i, n in enumerate(self.names)}
        self.edges = {n: _edges(self.ranges[n], self.bins) for n in self.names}
        self.x = None if dx is None or self.r is None else self.r * float(dx)

    def __repr__(self):
        return "%s(names=%s, %d rows, %d bins, samples=%d)" % (type(self).__name__, self.names, len(self.counts[self.names[0]]), self.bins, self.samples)

    def _table(self):
        """(rows, names, bins + 3) as the device lays it out"""
        return np.stack([np.concatenate([self.counts[n], self.below[n][:, None], self.above[n][:, None], self.nan[n][:, None]], axis=1)
                         for n in self.names], axis=1)

    def _name(self, name):
        if name not in self.names:
            raise ValueError("increments: no name %r in this result (%s)" % (name, ", ".join(self.names)))
        return name

    def centres(self, name):
        e = self.edges[self._name(name)]
        return 0.5 * (e[:, :-1] + e[:, 1:])

    def density(self, name):
        """counts / (in-range total * bin width): integrates to one over each row's range"""
        n, e = self.counts[self._name(name)], self.edges[name]
        with np.errstate(invalid="ignore", divide="ignore"):
            return n / (n.sum(axis=1, keepdims=True).astype(np.float64) * np.diff(e, axis=1))

    def moment(self, name, p):
        """<d^p>(r) of the in-range points, from the bin centres (``"phi"``: <|d phi|^p>)"""
        n, c = self.counts[self._name(name)].astype(np.float64), self.centres(name)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (n * c ** p).sum(axis=1) / n.sum(axis=1)

    def sigma(self, name):
        """sigma_r = sqrt<d^2>(r), from the counts"""
        return np.sqrt(self.moment(name, 2))

    def standardised(self, name):
        """(centres / sigma_r, density * sigma_r): unit second moment in every row"""
        s = self.sigma(name)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.centres(name) / s, self.density(name) * s

    def flatness(self, name):
        """<d^4> / <d^2>^2 from the bin centres"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.moment(name, 4) / self.moment(name, 2) ** 2

    def tail(self, name, z):
        """the fraction of the points (NaN excluded) with |d| > z sigma_r: the bins whose centre lies beyond, and everything out of
        range; exact whenever z sigma_r is an edge"""
        n, c = self.counts[self._name(name)], self.centres(name)
        beyond = (n * (np.abs(c) > float(z) * self.sigma(name)[:, None])).sum(axis=1) + self.below[name] + self.above[name]
        with np.errstate(invalid="ignore", divide="ignore"):
            return beyond / (n.sum(axis=1) + self.below[name] + self.above[name]).astype(np.float64)


class IncrementPDFs2d(IncrementPDFs):
    """IncrementPDFs with one row per lattice vector: vectors (n, 2), length, angle (as in StructureFunctions2d), project: the
    rotated pair (its first name holds the longitudinal, its second the transverse increment) or None, proj: the (c_x, c_y) used"""

    def __init__(self, names, vectors, tab, ranges, samples, points, dx=None, dy=None, project=None, proj=None, ring=None):
        IncrementPDFs.__init__(self, names, None, tab, ranges, samples, points)
        self.vectors = np.asarray(vectors, np.int64).reshape(-1, 2)
        self.dx = 1.0 if dx is None else float(dx)
        self.dy = self.dx if dy is None else float(dy)
        X, Y = self.vectors[:, 0] * self.dx, self.vectors[:, 1] * self.dy
        self.length, self.angle = np.hypot(X, Y), np.arctan2(Y, X)
        self.x = self.length
        self.project, self.proj, self.ring = project, proj, ring

    def along(self, direction):
        """the rows with r_y = 0 (r_x > 0), for "x", or with r_x = 0, for "y", ordered by separation, as an IncrementPDFs"""
        if direction not in ("x", "y"):
            raise ValueError("increments.along: direction = %r; valid: \"x\", \"y\"" % (direction,))
        rx, ry = self.vectors[:, 0], self.vectors[:, 1]
        rows = np.flatnonzero((ry == 0) & (rx > 0)) if direction == "x" else np.flatnonzero((rx == 0) & (ry > 0))
        r = (rx if direction == "x" else ry)[rows]
        rows = rows[np.argsort(r, kind="stable")]
        r = (rx if direction == "x" else ry)[rows]
        return IncrementPDFs(self.names, r, self._table()[rows], {n: self.ranges[n][rows] for n in self.names}, self.samples, self.points,
                             dx=self.dx if direction == "x" else self.dy)

    def isotropic(self, name):
        """(radius, counts (rings, bins + 3): the bins, below, above, nan, vectors per ring): the counts of the vectors of one ring
        (of a vectors=None call; else of one length) added.  Adding counts needs equal edges within a ring: explicit ranges."""
        self._name(name)
        key = self.ring if self.ring is not None else self.length
        _, which = np.unique(key, return_inverse=True)
        tab = self._table()[:, self.names.index(name)]
        radius, counts, nvec = [], [], []
        for b in range(which.max() + 1):
            rows = np.flatnonzero(which == b)
            if np.any(self.ranges[name][rows] != self.ranges[name][rows[0]]):
                raise ValueError("increments.isotropic: the vectors of the ring at %g have different ranges for %r; counts add only "
                                 "under equal edges: give explicit ranges" % (self.length[rows].mean(), name))
            radius.append(self.length[rows].mean())
            counts.append(tab[rows].sum(axis=0))
            nvec.append(len(rows))
        return np.array(radius), np.array(counts, np.int64), np.array(nvec, np.int64)


# ---- the specification in numpy -----------------------------------------------------------------------------------------------------
def _count(x, lo, hi, bins):
    """bins + 3 counts of one plane of values under the bin rule: the bins, below, above, nan"""
    i = _pdfs.bin_index(x, lo, hi, bins).ravel()
    i = np.where(i < 0, bins, np.where(i == bins, bins + 1, np.where(i == bins + 1, bins + 2, i)))
    return np.bincount(i, minlength=bins + 3)


def binned_values(fields, r, project=None, c=None):
    """{name: (ny, nx) plane of the values that are binned} at one separation: r an integer (along x) or a pair (r_x, r_y); the
    increments of the real names (the ``project`` pair rotated by c = (c_x, c_y) first), |d phi| for ``"phi"``"""
    if np.ndim(r) == 0:
        d = {n: structure.increments(np.asarray(fields[n]), r) for n in fields}
    else:
        d = {n: structure.increments2d(np.asarray(fields[n]), r[0], r[1]) for n in fields}
    if project is not None:
        a, b = project
        cx, cy = c
        da, db = d[a], d[b]
        d[a], d[b] = cx * da + cy * db, -cy * da + cx * db
    return {n: (np.abs(d[n]) if n == PHI else d[n]) for n in d}


def reference(fields, where=None, bins=256, ranges=None, project=None, width=8.0, proj=None):
    """THE definitions in numpy, from a dict {name: (ny, nx) plane} (``"phi"``: the complex plane).  where: separations along x (one
    dimension; None: structure.default_separations) or lattice vectors (n, 2); ranges as in pdfs (None: +-width sqrt<d^2> of these
    planes); project, proj: the rotation, for vectors, as in structure.reference2d.  Returns an IncrementPDFs / IncrementPDFs2d."""
    what = "increments.reference"
    names = list(fields)
    planes = {n: np.asarray(fields[n]) for n in names}
    shapes = set(p.shape for p in planes.values())
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError("%s: the planes must share one (ny, nx) shape, got %r" % (what, sorted(shapes)))
    for n, p in planes.items():
        if np.iscomplexobj(p) != (n == PHI):
            raise ValueError("%s: %r must be a %s plane" % (what, n, "complex" if n == PHI else "real"))
    ny, nx = next(iter(shapes))
    bins, width = _check_bins(bins, what), _check_width(width, what)
    two = where is not None and np.ndim(where) == 2
    if two:
        names, _, _ = structure._check_lists(names, [1], (), nx, what)
        vec = structure._check_vectors(where, nx, ny, what)
        project = structure._check_project(names, project, what)
        if project is not None:
            proj = structure.unit_vectors(vec) if proj is None else structure._check_proj(proj, len(vec), what)
        rows = len(vec)
    else:
        if project is not None:
            raise ValueError("%s: project = %r with separations along x; the rotation goes with lattice vectors" % (what, project))
        names, sep, _ = structure._check_lists(names, where, (), nx, what)
        rows = len(sep)
    given = _check_ranges(names, rows, ranges, what)

    def values(s):
        return binned_values(planes, vec[s] if two else sep[s], project, proj[s] if project is not None else None)

    rng = dict(given)
    if len(rng) < len(names):
        sums = np.zeros((rows, len(names), 2))
        for s in range(rows):
            v = values(s)
            for i, n in enumerate(names):
                sums[s, i] = v[n].sum(), (v[n] * v[n]).sum()
        for n, r in auto_ranges(names, sums, nx * ny, width).items():
            rng.setdefault(n, r)
    tab = np.zeros((rows, len(names), bins + 3), np.int64)
    for s in range(rows):
        v = values(s)
        for i, n in enumerate(names):
            tab[s, i] = _count(v[n], rng[n][s, 0], rng[n][s, 1], bins)
    if two:
        return IncrementPDFs2d(names, vec, tab, rng, 1, nx * ny, project=project, proj=proj if project else None)
    return IncrementPDFs(names, sep, tab, rng, 1, nx * ny)


# ---- the device -----------------------------------------------------------------------------------------------------------------------
def _iarr(v):
    return np.ascontiguousarray(v, np.int32)


def _lohi(names, rng):
    """the (rows, names) arrays of lo and of hi the library takes"""
    r = np.stack([rng[n] for n in names], axis=1)
    return np.ascontiguousarray(r[:, :, 0]), np.ascontiguousarray(r[:, :, 1])


def _ullp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))


class _Fused(object):
    """the fused contexts: nq_increment_range* / nq_increment_hist* / nq_increment_hist_read, the counts stay on the device"""

    def __init__(self, m, names, sep=None, vec=None, pair=(-1, -1), proj=None):
        self.ctx, self.names = m._ctx, names
        self.codes = _iarr([_CODES[n] for n in names])
        self.sep, self.vec = None if sep is None else _iarr(sep), None if vec is None else _iarr(vec)
        self.rows = len(sep) if vec is None else len(vec)
        self.pair, self.proj = pair, proj
        self.bins = 0

    def sums(self):
        c, out = self.ctx, np.empty((self.rows, len(self.names), 2))
        pj = None if self.proj is None else _lib._dptr(self.proj)
        if self.vec is None:
            c._chk(c.L.nq_increment_range(c.h, len(self.codes), _lib._iptr(self.codes), self.rows, _lib._iptr(self.sep), _lib._dptr(out)), "nq_increment_range")
        else:
            c._chk(c.L.nq_increment_range2(c.h, len(self.codes), _lib._iptr(self.codes), self.rows, _lib._iptr(self.vec), pj, self.pair[0], self.pair[1],
                                           _lib._dptr(out)), "nq_increment_range2")
        return out

    def bin(self, rng, bins, accumulate):
        c = self.ctx
        lo, hi = _lohi(self.names, rng)
        pj = None if self.proj is None else _lib._dptr(self.proj)
        if self.vec is None:
            c._chk(c.L.nq_increment_hist(c.h, len(self.codes), _lib._iptr(self.codes), self.rows, _lib._iptr(self.sep), _lib._dptr(lo), _lib._dptr(hi),
                                         bins, int(bool(accumulate))), "nq_increment_hist")
        else:
            c._chk(c.L.nq_increment_hist2(c.h, len(self.codes), _lib._iptr(self.codes), self.rows, _lib._iptr(self.vec), pj, self.pair[0], self.pair[1],
                                          _lib._dptr(lo), _lib._dptr(hi), bins, int(bool(accumulate))), "nq_increment_hist2")
        self.bins = bins

    def read(self):
        c = self.ctx
        n, out = ctypes.c_longlong(0), np.zeros((self.rows, len(self.names), self.bins + 3), np.uint64)
        c._chk(c.L.nq_increment_hist_read(c.h, ctypes.byref(n), _ullp(out)), "nq_increment_hist_read")
        return out, int(n.value)


class _AnySize(object):
    """grids without a fused plan: the path's own planes through nq_any_increments* (the range pass) and nq_any_increment_hist; several
    states are summed here, in integers.  Separations along x go as the vectors (r, 0)."""

    def __init__(self, m, names, sep=None, vec=None, pair=(-1, -1), proj=None):
        self.m, self.names = m, names
        self.sep = None if sep is None else _iarr(sep)
        self.vec = _iarr(vec) if vec is not None else _iarr(np.stack([np.asarray(sep), np.zeros(len(sep), np.int64)], axis=1))
        self.rows = len(self.vec)
        self.pair, self.proj = pair, proj
        self.tab, self.n = None, 0

    def _planes(self):
        m = self.m
        real = [n for n in self.names if n != PHI]
        planes = m._pdf_planes(real) if real else {}
        keep, what = [], []
        for n in self.names:
            pl, w = (m._d["phi"], 2) if n == PHI else (planes[n][0], 0)
            if n != PHI and planes[n][1] == 1:             # phi2: as a plane, as in structure._AnySize
                pl = pl.abs2()
            keep.append(pl)                                # the planes live until the synchronous call returns
            what.append(w)
        return keep, (ctypes.c_void_p * len(keep))(*[p.ptr for p in keep]), _lib._iptr(_iarr(what))

    def sums(self):
        e = self.m._eng
        keep, ptrs, what = self._planes()
        ny, nx = keep[0].shape
        nf = len(self.names)
        out = np.empty((self.rows, structure.COLS * nf))
        pj = None if self.proj is None else _lib._dptr(self.proj)
        if self.sep is not None:
            e.chk(e.L.nq_any_increments(e.h, nf, ptrs, what, int(ny), int(nx), self.rows, _lib._iptr(self.sep), 0, None, _lib._dptr(out)), "nq_any_increments")
        else:
            e.chk(e.L.nq_any_increments2(e.h, nf, ptrs, what, int(ny), int(nx), self.rows, _lib._iptr(self.vec), pj, self.pair[0], self.pair[1], 0, None,
                                         _lib._dptr(out)), "nq_any_increments2")
        return np.ascontiguousarray(out.reshape(self.rows, nf, structure.COLS)[:, :, :2])

    def bin(self, rng, bins, accumulate):
        e = self.m._eng
        keep, ptrs, what = self._planes()
        ny, nx = keep[0].shape
        lo, hi = _lohi(self.names, rng)
        tab = np.zeros((self.rows, len(self.names), bins + 3), np.uint64)
        pj = None if self.proj is None else _lib._dptr(self.proj)
        e.chk(e.L.nq_any_increment_hist(e.h, len(self.names), ptrs, what, int(ny), int(nx), self.rows, _lib._iptr(self.vec), pj, self.pair[0], self.pair[1],
                                        _lib._dptr(lo), _lib._dptr(hi), bins, _ullp(tab)), "nq_any_increment_hist")
        if accumulate and self.tab is not None:
            self.tab, self.n = self.tab + tab, self.n + 1
        else:
            self.tab, self.n = tab, 1

    def read(self):
        return self.tab.copy(), self.n


class _Call(object):
    """what pdfs, pdfs2d and Accumulator share: the validated call, its backend, its ranges and its result"""

    def __init__(self, m, names, separations, vectors, project, bins, ranges, width, two, what):
        self.m, self.two, self.what = m, two, what
        self.dx, self.dy = getattr(m, "dx", None), getattr(m, "dy", None)
        self.project = self.proj = self.ring = self.sep = self.vec = None
        pair = (-1, -1)
        if two:
            call = structure._Call2d(m, names, vectors, (), project, None, what)
            self.names, self.vec, self.project, self.proj, self.ring = call.names, call.vec, call.project, call.proj, call.ring
            if self.project:
                pair = (self.names.index(self.project[0]), self.names.index(self.project[1]))
        else:
            self.names, self.sep, _ = structure._validate(m, names, separations, (), "x", what)
        self.rows = len(self.vec) if two else len(self.sep)
        self.bins, self.width = _check_bins(bins, what), _check_width(width, what)
        self.given = _check_ranges(self.names, self.rows, ranges, what)
        self.be = (_AnySize if getattr(m, "_any_size", False) else _Fused)(m, self.names, self.sep, self.vec, pair, self.proj)

    def ranges(self):
        """the explicit ranges, the others from a range pass of the current state"""
        rng = dict(self.given)
        if len(rng) < len(self.names):
            for n, r in auto_ranges(self.names, self.be.sums(), self.m.nx * self.m.ny, self.width).items():
                rng.setdefault(n, r)
        return rng

    def result(self, tab, samples, rng):
        points = self.m.nx * self.m.ny
        if self.two:
            return IncrementPDFs2d(self.names, self.vec, tab, rng, samples, points, dx=self.dx, dy=self.dy, project=self.project, proj=self.proj, ring=self.ring)
        return IncrementPDFs(self.names, self.sep, tab, rng, samples, points, dx=self.dx)

    def once(self):
        rng = self.ranges()
        if isinstance(self.be, _Fused):
            self.be.ctx._ipdf_owner = None
        self.be.bin(rng, self.bins, False)
        tab, n = self.be.read()
        return self.result(tab, n, rng)


def pdfs(m, names=("u", "v", "q_psi"), separations=None, bins=256, ranges=None, width=8.0):
    """PDFs of the x-increments of the model's current physical fields, counted on the device.
    names, separations: as structure.functions takes them; bins: 1 to MAX_BINS; ranges: {name: (lo, hi)} or {name: (nsep, 2)}, names
    without an entry get +-width sigma_r from a range pass on the device.  May be called wherever structure.functions may; reads the
    state and writes only buffers of its own (structure's tables and Accumulators are not disturbed)."""
    return _Call(m, names, separations, None, None, bins, ranges, width, False, "increments.pdfs").once()


def pdfs2d(m, names=("u", "v"), vectors=None, project=("u", "v"), bins=256, ranges=None, width=8.0):
    """The same at lattice vectors (r_x, r_y) (default: structure.ring_vectors(nx)), with the ``project`` pair rotated onto each
    separation vector first (first name: longitudinal, second: transverse; None: no rotation; the default pair is dropped when the
    call does not name both).  Every combination of names works at every size: the values go through physical planes."""
    return _Call(m, names, None, vectors, project, bins, ranges, width, True, "increments.pdfs2d").once()


class Accumulator(object):
    """Counts of several states under fixed ranges: the first add() fixes the ranges from that state (or takes the explicit ones) and
    shows them as ``ranges``; add() bins the current state on top of the table (on the device for the fused contexts: one read at
    result(); in integers on the host for the any-size path); result() returns the IncrementPDFs; reset() starts over and frees the
    ranges again.  A context has one count table: a pdfs / pdfs2d call (or another Accumulator's add) on the same model in between
    takes it over, and the next add() raises instead of mixing counts."""

    def __init__(self, m, names=("u", "v", "q_psi"), separations=None, bins=256, ranges=None, width=8.0):
        self.call = _Call(m, names, separations, None, None, bins, ranges, width, False, "increments.Accumulator")
        self.be, self.n, self.ranges = self.call.be, 0, None

    def _owned(self):
        return not isinstance(self.be, _Fused) or getattr(self.be.ctx, "_ipdf_owner", None) is self

    def add(self):
        if self.n and not self._owned():
            raise RuntimeError("Accumulator.add: the context's table was used by another call since the last add(); reset() first")
        if self.ranges is None:
            self.ranges = self.call.ranges()
        if isinstance(self.be, _Fused):
            self.be.ctx._ipdf_owner = self
        self.be.bin(self.ranges, self.call.bins, self.n > 0)
        self.n += 1

    def result(self):
        if self.n == 0:
            raise RuntimeError("Accumulator.result: nothing added yet")
        if not self._owned():
            raise RuntimeError("Accumulator.result: the context's table was used by another call since the last add()")
        tab, n = self.be.read()
        return self.call.result(tab, n, self.ranges)

    def reset(self):
        self.n, self.ranges = 0, None
        if isinstance(self.be, _AnySize):
            self.be.tab, self.be.n = None, 0
