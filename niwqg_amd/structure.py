"""Structure functions of the physical fields, formed on the device.

    from niwqg_amd import structure
    S = structure.functions(m, names=("u", "v", "q_psi"), mixed=(("u", "v", "v"), ("u", "q_psi", "q_psi")))
    S.r, S.x                     # separations in grid points and in length
    S.moment("u", 3)             # <du^3>(r);  S.abs_moment("u", 3) = <|du|^3>(r)
    S.third_order("u", "v")      # <du_L (du_L^2 + du_T^2)>(r): along x, u is the longitudinal and v the transverse component
    S.flatness("u")              # S4 / S2^2

Definitions (``reference`` restates them in numpy).  For a field a on the (ny, nx) grid and an integer separation r along x,
periodic, d_r a(x, y) = a((x + r) mod nx, y) - a(x, y).  Per name and separation nine plane means (sum over all points / nx ny):

    a real name    column p - 1 = <d^p>, p = 1 .. 6;      columns 6, 7, 8 = <|d|>, <|d|^3>, <|d|^5>
    "phi"          column p - 1 = <|d phi|^p>, p = 1 .. 6; columns 6, 7 = <Re d phi>, <Im d phi>; column 8 = 0

and one mean per mixed triple (a, b, c) of the call's names: <d_a d_b d_c>.  ``"phi"``, the complex wave field, may only be the
last two entries together: (a, "phi", "phi") = <d_a |d phi|^2>.  Powers are successive products, d^p = d^(p-1) d, and
|d|^3 = |d^3|, on the device and in ``reference`` alike.

Names: on CoupledModel, UnCoupledModel and YBJModel everything ``pdfs.available(m)`` and ``flow.available(m)`` list, plus
``"phi"``; on QGModel ``q``, ``c`` and, on the any-size path, its flow names: what the PDFs accept.  The values are those the PDFs
bin (the last inversion's rows).  At most three real names per call, or two and ``"phi"``: the LDS rows of a 4096-point row
pass (3 x 32 KB, or 2 x 32 KB + 64 KB).  On the fused grids the Kernel family runs ONE row pass for all names
(``k_x_flow_sf``: the row's values go to LDS rows and every separation is read from there); QGModel and the any-size path run
``k_sf_plane`` on their planes.  Only the table of sums leaves the GPU.  The sums are deterministic: two calls on one state return
the same bits.

Refused: slab-decomposed models; increments along y (``direction="y"``); more names than above;
separations outside [1, nx - 1] or not strictly increasing, or more than ``MAX_SEPS``; names the model lacks; at nx = 8192,
where every name runs in a launch of its own, a triple of different names and ``"phi"`` together with a real name.
"""
import ctypes

import numpy as np

from . import _lib, flow, pdfs

COLS, MAX_SEPS, MAX_FIELDS, MAX_TRIPLES = _lib.SF_COLS, _lib.SF_MAX_SEPS, _lib.SF_MAX_FIELDS, _lib.SF_MAX_TRIPLES
PHI = "phi"
_CODES = dict(pdfs._CODES)
_CODES[PHI] = _lib.SF_PHI


def default_separations(nx):
    """1, 2, 3, 4, 6, 8, 12, ...: powers of two and their 3/2 multiples, up to nx / 2"""
    out, p = [], 1
    while p <= nx // 2:
        out.append(p)
        if p >= 2 and 3 * p // 2 <= nx // 2:
            out.append(3 * p // 2)
        p *= 2
    return np.array(sorted(out), np.int64)


def available(m):
    """the names functions(m) takes"""
    out = pdfs.available(m) + flow.available(m)
    return out if pdfs._is_qg(m) else out + [PHI]


def _powers(d):
    p = [d]
    for _ in range(5):
        p.append(p[-1] * d)
    return p


def increments(a, r):
    """d_r a = a((x + r) mod nx, y) - a(x, y) of a (ny, nx) plane"""
    return np.roll(a, -int(r), axis=1) - a


def _columns(a, r):
    """the nine columns of one plane at one separation -> (sums, sums of the absolute values)"""
    d = increments(a, r)
    if np.iscomplexobj(a):
        m2 = d.real * d.real + d.imag * d.imag
        m1 = np.sqrt(m2)
        m4 = m2 * m2
        s = [m1.sum(), m2.sum(), (m2 * m1).sum(), m4.sum(), (m4 * m1).sum(), (m4 * m2).sum(), d.real.sum(), d.imag.sum(), 0.0]
        return s, s[:6] + [np.abs(d.real).sum(), np.abs(d.imag).sum(), 0.0]
    p = _powers(d)
    s = [x.sum() for x in p] + [np.abs(d).sum(), np.abs(p[2]).sum(), np.abs(p[4]).sum()]
    return s, [s[6], s[1], s[7], s[3], s[8], s[5], s[6], s[7], s[8]]       # |d^p| = |d|^p: the odd powers' are columns 6, 7, 8


def _triple(fields, t, r):
    a, b, c = t
    da = increments(fields[a], r)
    if b == PHI:
        d = increments(fields[PHI], r)
        col = da * (d.real * d.real + d.imag * d.imag)
    else:
        col = da * increments(fields[b], r) * increments(fields[c], r)
    return col.sum(), np.abs(col).sum()


def _check_lists(names, separations, mixed, nx, what):
    """the checks that need no model -> (names, separations int64, mixed)"""
    names = [names] if isinstance(names, str) else list(names)
    if not names or len(set(names)) != len(names):
        raise ValueError("%s: names %r; valid: one to three different names" % (what, names))
    real = [n for n in names if n != PHI]
    if len(real) > MAX_FIELDS or len(names) > MAX_FIELDS:
        raise ValueError("%s: %d real names%s; valid: at most three real names per call, or two and \"phi\" (the LDS rows of a "
                         "4096-point row pass: 3 x 32 KB, or 2 x 32 KB + 64 KB)" % (what, len(real), " and \"phi\"" if PHI in names else ""))
    sep = default_separations(nx) if separations is None else np.asarray(separations)
    if sep.ndim != 1 or sep.size < 1 or sep.size > MAX_SEPS:
        raise ValueError("%s: %d separations; valid: 1 to %d" % (what, sep.size, MAX_SEPS))
    if not np.issubdtype(sep.dtype, np.integer):
        if not np.all(sep == np.round(sep)):
            raise ValueError("%s: separations %r; valid: integers (grid points)" % (what, sep))
    sep = sep.astype(np.int64)
    if sep.min() < 1 or sep.max() > nx - 1 or np.any(np.diff(sep) <= 0):
        raise ValueError("%s: separations %r; valid: integers in [1, nx - 1 = %d], strictly increasing" % (what, sep.tolist(), nx - 1))
    mixed = [tuple(t) for t in (mixed or ())]
    if len(mixed) > MAX_TRIPLES:
        raise ValueError("%s: %d mixed triples; valid: at most %d" % (what, len(mixed), MAX_TRIPLES))
    for t in mixed:
        if len(t) != 3 or any(n not in names for n in t):
            raise ValueError("%s: mixed triple %r; valid: three names out of %s" % (what, t, ", ".join(names)))
        if t[0] == PHI or (t[1] == PHI) != (t[2] == PHI):
            raise ValueError("%s: mixed triple %r; \"phi\" may only be the last two entries together: (a, \"phi\", \"phi\") = "
                             "<d_a |d phi|^2>" % (what, t))
    if len(set(mixed)) != len(mixed):
        raise ValueError("%s: mixed triples %r; each once" % (what, mixed))
    return names, sep, mixed


def reference(fields, separations=None, mixed=()):
    """THE definitions in numpy, from a dict {name: (ny, nx) plane} (``"phi"``: the complex plane): a StructureFunctions with the
    raw sums in ``sums`` (nsep, 9 names + triples) and the sums of the ABSOLUTE values of the same terms in ``abs_sums`` (what the
    error bound of a summation is stated against)."""
    names = list(fields)
    planes = {n: np.asarray(fields[n]) for n in names}
    shapes = set(p.shape for p in planes.values())
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError("structure.reference: the planes must share one (ny, nx) shape, got %r" % sorted(shapes))
    for n, p in planes.items():
        if np.iscomplexobj(p) != (n == PHI):
            raise ValueError("structure.reference: %r must be a %s plane" % (n, "complex" if n == PHI else "real"))
    ny, nx = next(iter(shapes))
    names, sep, mixed = _check_lists(names, separations, mixed, nx, "structure.reference")
    nout = COLS * len(names) + len(mixed)
    sums, asums = np.zeros((sep.size, nout)), np.zeros((sep.size, nout))
    rows = max(1, (1 << 18) // nx)                          # blocks of whole rows that stay in cache; their sums are added in order
    for y0 in range(0, ny, rows):
        block = {n: p[y0:y0 + rows] for n, p in planes.items()}
        for s, r in enumerate(sep):
            for i, n in enumerate(names):
                a, b = _columns(block[n], r)
                sums[s, COLS * i:COLS * (i + 1)] += a
                asums[s, COLS * i:COLS * (i + 1)] += b
            for k, t in enumerate(mixed):
                a, b = _triple(block, t, r)
                sums[s, COLS * len(names) + k] += a
                asums[s, COLS * len(names) + k] += b
    return StructureFunctions(names, sep, mixed, sums, 1, nx * ny, abs_sums=asums)


class StructureFunctions(object):
    """names, r (separations in grid points), x = r dx (None without a grid spacing), mixed: {triple: <d_a d_b d_c>(r)};
    sums: the raw sums (nsep, 9 names + triples) of `samples` states of `points` points each; table = sums / (samples points)"""

    def __init__(self, names, r, triples, sums, samples, points, dx=None, abs_sums=None):
        self.names, self.r, self.triples = list(names), np.asarray(r, np.int64), list(triples)
        self.sums, self.samples, self.points, self.abs_sums = sums, int(samples), int(points), abs_sums
        self.table = sums / (float(max(self.samples, 1)) * float(points))
        self.x = None if dx is None else self.r * float(dx)
        self.mixed = {t: self.table[:, COLS * len(self.names) + k] for k, t in enumerate(self.triples)}

    def __repr__(self):
        return "StructureFunctions(names=%s, %d separations, mixed=%s, samples=%d)" % (self.names, self.r.size, self.triples, self.samples)

    def _col(self, name, k):
        if name not in self.names:
            raise ValueError("structure: no name %r in this result (%s)" % (name, ", ".join(self.names)))
        return self.table[:, COLS * self.names.index(name) + k]

    def moment(self, name, p):
        """<d^p>(r), p = 1 .. 6 (``"phi"``: <|d phi|^p>)"""
        if p not in (1, 2, 3, 4, 5, 6):
            raise ValueError("structure.moment: p = %r; valid: 1 to 6" % (p,))
        return self._col(name, p - 1)

    def abs_moment(self, name, p):
        """<|d|^p>(r), p = 1 .. 6"""
        if p not in (1, 2, 3, 4, 5, 6):
            raise ValueError("structure.abs_moment: p = %r; valid: 1 to 6" % (p,))
        if name == PHI or p % 2 == 0:
            return self._col(name, p - 1)
        return self._col(name, 6 + p // 2)

    def mean_increment(self):
        """<d phi>(r), complex"""
        return self._col(PHI, 6) + 1j * self._col(PHI, 7)

    def flatness(self, name):
        """S4 / S2^2"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.moment(name, 4) / self.moment(name, 2) ** 2

    def third_order(self, longitudinal="u", transverse="v"):
        """<d u_L (d u_L^2 + d u_T^2)>(r) = moment(L, 3) + mixed[(L, T, T)]"""
        t = (longitudinal, transverse, transverse)
        if t not in self.mixed:
            raise ValueError("structure.third_order: the call needs mixed=(%r,)" % (t,))
        return self.moment(longitudinal, 3) + self.mixed[t]


def _validate(m, names, separations, mixed, direction, what):
    if direction != "x":
        raise NotImplementedError("%s: direction = %r; only increments along x exist: the row pass holds rows, not columns (a column "
                                  "pass over physical planes would close this; DESIGN.md section 7)" % (what, direction))
    any_size = getattr(m, "_any_size", False)
    if not any_size and not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("%s: slab-decomposed models have no structure functions yet (a row's increments are local, the sums "
                                  "would have to be added over the ranks; DESIGN.md section 7); use a single-GPU model" % what)
    names, sep, mixed = _check_lists(names, separations, mixed, m.nx, what)
    if pdfs._is_qg(m) and not any_size and any(n in flow.NAMES for n in names):
        flow.refuse(m, what)
    valid = available(m)
    bad = [n for n in names if n not in valid]
    if bad:
        raise ValueError("%s: names %r; valid names for %s: %s" % (what, bad, type(m).__module__, ", ".join(valid)))
    if not any_size and m.nx >= flow.ONE_VALUE_NX:
        if any(len(set(t)) > 1 for t in mixed) or (PHI in names and len(names) > 1):
            raise NotImplementedError("%s: no triple of different names and no \"phi\" beside a real name at nx = %d yet: a device thread "
                                      "of that row plan holds one value, so every name gets a launch of its own (DESIGN.md section 7); "
                                      "single names, \"phi\" alone and (a, a, a) work" % (what, m.nx))
    return names, sep, mixed


def _iarr(v):
    return np.ascontiguousarray(v, np.int32)


class _Fused(object):
    """the fused contexts: nq_structure / nq_structure_read, running sums on the device"""

    def __init__(self, m, names, sep, mixed):
        self.ctx = m._ctx
        self.codes, self.sep = _iarr([_CODES[n] for n in names]), _iarr(sep)
        self.tri = _iarr([[names.index(n) for n in t] for t in mixed]).reshape(-1)
        self.nout = COLS * len(names) + len(mixed)

    def add(self, accumulate):
        c = self.ctx
        c._chk(c.L.nq_structure(c.h, len(self.codes), _lib._iptr(self.codes), len(self.sep), _lib._iptr(self.sep), len(self.tri) // 3,
                                _lib._iptr(self.tri) if len(self.tri) else None, int(bool(accumulate))), "nq_structure")

    def read(self):
        c = self.ctx
        n, out = ctypes.c_longlong(0), np.empty((len(self.sep), self.nout))
        c._chk(c.L.nq_structure_read(c.h, ctypes.byref(n), _lib._dptr(out)), "nq_structure_read")
        return out, int(n.value)


class _AnySize(object):
    """grids without a fused plan: nq_any_increments on the path's own planes; several states are summed here, in float64"""

    def __init__(self, m, names, sep, mixed):
        self.m, self.names, self.sep = m, names, _iarr(sep)
        self.tri = _iarr([[names.index(n) for n in t] for t in mixed]).reshape(-1)
        self.nout = COLS * len(names) + len(mixed)
        self.sums, self.n = None, 0

    def add(self, accumulate):
        e, m = self.m._eng, self.m
        real = [n for n in self.names if n != PHI]
        planes = m._pdf_planes(real) if real else {}
        ptrs, what = [], []
        for n in self.names:
            pl, w = (m._d["phi"], 2) if n == PHI else (planes[n][0], 0)
            if n != PHI and planes[n][1] == 1:             # phi2: the PDFs form |phi|^2 from the phi plane as they bin; here as a plane
                pl = pl.abs2()
            ptrs.append(pl)
            what.append(w)
        keep = ptrs                                        # the planes live until the synchronous call returns
        ny, nx = keep[0].shape
        out = np.empty((len(self.sep), self.nout))
        e.chk(e.L.nq_any_increments(e.h, len(self.names), (ctypes.c_void_p * len(keep))(*[p.ptr for p in keep]), _lib._iptr(_iarr(what)),
                                    int(ny), int(nx), len(self.sep), _lib._iptr(self.sep), len(self.tri) // 3,
                                    _lib._iptr(self.tri) if len(self.tri) else None, _lib._dptr(out)), "nq_any_increments")
        if accumulate and self.sums is not None:
            self.sums, self.n = self.sums + out, self.n + 1
        else:
            self.sums, self.n = out, 1

    def read(self):
        return self.sums.copy(), self.n


def _backend(m, names, sep, mixed):
    return (_AnySize if getattr(m, "_any_size", False) else _Fused)(m, names, sep, mixed)


def _result(m, names, sep, mixed, sums, n):
    dx = getattr(m, "dx", None)
    return StructureFunctions(names, sep, mixed, sums, n, m.nx * m.ny, dx=dx)


def functions(m, names=("u", "v", "q_psi"), separations=None, mixed=(), direction="x"):
    """Structure functions of the model's current physical fields along x, summed on the device.
    names: up to three of available(m) (two beside "phi"); separations: integers in [1, nx - 1], strictly increasing (default:
    default_separations(nx)); mixed: up to four triples of the names.  May be called wherever pdfs.field_pdfs may; reads the
    state and writes only buffers of its own."""
    names, sep, mixed = _validate(m, names, separations, mixed, direction, "structure.functions")
    be = _backend(m, names, sep, mixed)
    if isinstance(be, _Fused):
        be.ctx._sf_owner = None
    be.add(False)
    sums, n = be.read()
    return _result(m, names, sep, mixed, sums, n)


class Accumulator(object):
    """Sums of several states: add() adds the current state's sums to the running table (on the device for the fused contexts:
    one download at result(); in float64 on the host for the any-size path), result() returns the StructureFunctions of all
    states added, reset() starts over.  A context has one table: a functions() call (or another Accumulator's add) on the same
    model in between takes it over, and the next add() raises instead of mixing sums."""

    def __init__(self, m, names=("u", "v", "q_psi"), separations=None, mixed=(), direction="x"):
        self.m = m
        self.names, self.sep, self.mixed = _validate(m, names, separations, mixed, direction, "structure.Accumulator")
        self.be = _backend(m, self.names, self.sep, self.mixed)
        self.n = 0

    def _owned(self):
        return not isinstance(self.be, _Fused) or getattr(self.be.ctx, "_sf_owner", None) is self

    def add(self):
        if self.n and not self._owned():
            raise RuntimeError("Accumulator.add: the context's table was used by another call since the last add(); reset() first")
        if isinstance(self.be, _Fused):
            self.be.ctx._sf_owner = self
        self.be.add(self.n > 0)
        self.n += 1

    def result(self):
        if self.n == 0:
            sums = np.zeros((len(self.sep), COLS * len(self.names) + len(self.mixed)))
            return _result(self.m, self.names, self.sep, self.mixed, sums, 0)
        if not self._owned():
            raise RuntimeError("Accumulator.result: the context's table was used by another call since the last add()")
        sums, n = self.be.read()
        return _result(self.m, self.names, self.sep, self.mixed, sums, n)

    def reset(self):
        self.n = 0
        if isinstance(self.be, _AnySize):
            self.be.sums, self.be.n = None, 0
