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

Two-dimensional separations: ``functions2d`` / ``Accumulator2d`` take lattice vectors (r_x, r_y) instead of
separations along x, rotate (u, v) onto each separation vector on the device and return a ``StructureFunctions2d``:

    S = structure.functions2d(m, names=("u", "v", "q_psi"), mixed=(("u", "v", "v"),))     # ring_vectors(nx): 8 angles per radius
    S.vectors, S.length, S.angle  # per table row
    S.third_order("u", "v")      # <dL (dL^2 + dT^2)> per vector: u holds the longitudinal, v the transverse increment
    radius, table, count = S.isotropic()
    S.along("y")                 # the rows (0, r) as a StructureFunctions
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


# ---- two-dimensional separations ----------------------------------------------------------------------------
# Increments at lattice vectors r = (r_x, r_y), d_r a(x, y) = a((x + r_x) mod nx, (y + r_y) mod ny) - a(x, y); the same nine columns
# and triples per name and vector.  Optionally one ordered pair (a, b) of the call's real names is rotated per vector before
# anything is summed, d_L = c_x d_a + c_y d_b, d_T = -c_y d_a + c_x d_b: the columns and triples of a then hold L (the component
# along the separation) and those of b hold T.  (c_x, c_y) is formed HERE, in numpy (default: the unit vector of (r_x dx, r_y dy)),
# and handed to the library, so that reference2d and the device use the same bits.
MAX_VECS = _lib.SF2_MAX_VECS


def increments2d(a, rx, ry):
    """d_r a = a((x + r_x) mod nx, (y + r_y) mod ny) - a(x, y) of a (ny, nx) plane"""
    return np.roll(np.roll(a, -int(rx), axis=1), -int(ry), axis=0) - a


def axis_vectors(nx, direction, separations=None):
    """(r, 0) for "x" or (0, r) for "y", r out of separations (default: default_separations(nx))"""
    if direction not in ("x", "y"):
        raise ValueError("structure.axis_vectors: direction = %r; valid: \"x\", \"y\"" % (direction,))
    sep = default_separations(nx) if separations is None else np.asarray(separations, np.int64).reshape(-1)
    zero = np.zeros_like(sep)
    return np.stack([sep, zero] if direction == "x" else [zero, sep], axis=1).astype(np.int64)


def _rings(nx, radii, angles):
    """ring_vectors and, per vector, the radius of the ring that brought it"""
    angles = int(angles)
    if angles < 1:
        raise ValueError("structure.ring_vectors: angles = %r; valid: at least 1" % (angles,))
    thin = radii is None
    radii = default_separations(nx) if thin else np.asarray(radii, np.float64).reshape(-1)
    if thin and radii.size * angles > MAX_VECS:                # every n-th radius, the largest kept
        step = -(-radii.size * angles // MAX_VECS)
        radii = radii[::-1][::step][::-1]
    if radii.size < 1 or np.any(radii < 1) or np.any(radii > nx - 1):
        raise ValueError("structure.ring_vectors: radii %r; valid: in [1, nx - 1 = %d]" % (np.asarray(radii).tolist(), nx - 1))
    seen, out, ring = set(), [], []
    for rho in radii:
        for k in range(angles):
            th = k * np.pi / angles
            rx, ry = int(np.rint(rho * np.cos(th))), int(np.rint(rho * np.sin(th)))
            if ry == 0 and rx < 0:                             # the same increments as (-r_x, 0), up to the sign of the odd columns
                rx = -rx
            if (rx, ry) == (0, 0) or (rx, ry) in seen:
                continue
            seen.add((rx, ry))
            out.append((rx, ry))
            ring.append(float(rho))
    if len(out) > MAX_VECS:
        raise ValueError("structure.ring_vectors: %d vectors; valid: at most %d (fewer radii or angles)" % (len(out), MAX_VECS))
    return np.array(out, np.int64).reshape(-1, 2), np.array(ring)


def ring_vectors(nx, radii=None, angles=8):
    """The lattice vectors nearest to radius rho at the angles k pi / angles, k = 0 .. angles - 1 (the half-plane r_y >= 0:
    d_{-r} has the same L and T moments), for every rho of radii (default: default_separations(nx), thinned to fit MAX_VECS);
    duplicates removed, | |r| - rho | <= sqrt(2) / 2."""
    return _rings(nx, radii, angles)[0]


def _check_vectors(vectors, nx, ny, what):
    v = np.asarray(vectors)
    if v.ndim != 2 or v.shape[1] != 2 or v.shape[0] < 1 or v.shape[0] > MAX_VECS:
        raise ValueError("%s: vectors of shape %r; valid: (n, 2) integers (r_x, r_y), n = 1 to %d" % (what, v.shape, MAX_VECS))
    if not np.issubdtype(v.dtype, np.integer):
        if not np.all(v == np.round(v)):
            raise ValueError("%s: vectors %r; valid: integers (grid points)" % (what, v.tolist()))
    v = v.astype(np.int64)
    bad = (np.abs(v[:, 0]) > nx - 1) | (v[:, 1] < 0) | (v[:, 1] > ny - 1) | ((v[:, 0] == 0) & (v[:, 1] == 0))
    if np.any(bad):
        raise ValueError("%s: vectors %r; valid: r_x in [-(nx - 1), nx - 1], r_y in [0, ny - 1] (the half-plane: d_{-r} has the same "
                         "moments), not (0, 0)" % (what, v[bad].tolist()))
    keys = set()
    for rx, ry in v:
        k = (int(rx) % nx, int(ry))
        if k in keys:
            raise ValueError("%s: vector (%d, %d) is listed twice, or beside its periodic image (r_x -+ nx)" % (what, rx, ry))
        keys.add(k)
    return v


def _check_project(names, project, what):
    """None, or the pair of real names the call rotates"""
    if project is None:
        return None
    project = tuple(project)
    if len(project) != 2 or project[0] == project[1]:
        raise ValueError("%s: project = %r; valid: None, or two different real names of the call" % (what, project))
    if PHI in project:
        raise ValueError("%s: project = %r; \"phi\" is complex: the rotation takes two real names (a vector's components)" % (what, project))
    if any(n not in names for n in project):
        if project == ("u", "v"):                              # the default pair: off when the call does not have it
            return None
        raise ValueError("%s: project = %r; valid: two of the call's names (%s)" % (what, project, ", ".join(names)))
    return project


def unit_vectors(vectors, dx=1.0, dy=1.0):
    """(c_x, c_y) = (r_x dx, r_y dy) / |(r_x dx, r_y dy)| per vector, float64 (n, 2): the default projection"""
    v = np.asarray(vectors, np.float64) * np.array([float(dx), float(dy)])
    return np.ascontiguousarray(v / np.hypot(v[:, 0], v[:, 1])[:, None])


def _check_proj(proj, nvec, what):
    proj = np.ascontiguousarray(proj, np.float64)
    if proj.shape != (nvec, 2) or not np.all(np.isfinite(proj)):
        raise ValueError("%s: proj of shape %r; valid: (%d, 2) finite numbers (c_x, c_y), one pair per vector" % (what, proj.shape, nvec))
    return proj


def _abs_columns(m):
    """the columns of the sums of absolute values from the magnitude m >= |d| of the terms"""
    p = _powers(m)
    s = [x.sum() for x in p]
    return [s[0], s[1], s[2], s[3], s[4], s[5], s[0], s[2], s[4]]


def _columns2d(d, mag=None):
    """_columns of the increments d themselves; mag: what majorises |d| (a rotated component), or None: |d|"""
    if np.iscomplexobj(d):
        m2 = d.real * d.real + d.imag * d.imag
        m1 = np.sqrt(m2)
        m4 = m2 * m2
        s = [m1.sum(), m2.sum(), (m2 * m1).sum(), m4.sum(), (m4 * m1).sum(), (m4 * m2).sum(), d.real.sum(), d.imag.sum(), 0.0]
        return s, s[:6] + [np.abs(d.real).sum(), np.abs(d.imag).sum(), 0.0]
    p = _powers(d)
    s = [x.sum() for x in p] + [np.abs(d).sum(), np.abs(p[2]).sum(), np.abs(p[4]).sum()]
    if mag is not None:
        return s, _abs_columns(mag)
    return s, [s[6], s[1], s[7], s[3], s[8], s[5], s[6], s[7], s[8]]


def reference2d(fields, vectors, mixed=(), project=None, proj=None):
    """THE definitions in numpy, from a dict {name: (ny, nx) plane} (``"phi"``: the complex plane) and (n, 2) integer vectors:
    a StructureFunctions2d with the raw sums in ``sums`` (n, 9 names + triples) and, in ``abs_sums``, the sums of the absolute
    values of the same terms (what the error bound of a summation is stated against).  project = (a, b): the rotation, with
    proj (n, 2) = (c_x, c_y) per vector (default: the unit vectors of the lattice vectors, dx = dy); the terms of the rotated
    names are majorised by (|c_x d_a| + |c_y d_b|)^p, resp. (|c_y d_a| + |c_x d_b|)^p, in the columns and inside the triples."""
    what = "structure.reference2d"
    names = list(fields)
    planes = {n: np.asarray(fields[n]) for n in names}
    shapes = set(p.shape for p in planes.values())
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError("%s: the planes must share one (ny, nx) shape, got %r" % (what, sorted(shapes)))
    for n, p in planes.items():
        if np.iscomplexobj(p) != (n == PHI):
            raise ValueError("%s: %r must be a %s plane" % (what, n, "complex" if n == PHI else "real"))
    ny, nx = next(iter(shapes))
    names, _, mixed = _check_lists(names, [1], mixed, nx, what)
    vec = _check_vectors(vectors, nx, ny, what)
    project = _check_project(names, project, what)
    if project is not None:
        proj = unit_vectors(vec) if proj is None else _check_proj(proj, len(vec), what)
    nout = COLS * len(names) + len(mixed)
    sums, asums = np.zeros((len(vec), nout)), np.zeros((len(vec), nout))
    rows = max(1, (1 << 18) // nx)                          # the row blocks of ``reference``: (r, 0) gives its bits
    for s, (rx, ry) in enumerate(vec):
        d = {n: increments2d(planes[n], rx, ry) for n in names}
        mag = {n: (d[n].real * d[n].real + d[n].imag * d[n].imag if n == PHI else np.abs(d[n])) for n in names}   # phi: |d phi|^2
        rotated = ()
        if project is not None:
            a, b = project
            cx, cy = proj[s]
            da, db = d[a], d[b]
            d[a], d[b] = cx * da + cy * db, -cy * da + cx * db
            mag[a], mag[b] = np.abs(cx * da) + np.abs(cy * db), np.abs(cy * da) + np.abs(cx * db)
            rotated = project
        for y0 in range(0, ny, rows):
            sl = slice(y0, y0 + rows)
            for i, n in enumerate(names):
                x, y = _columns2d(d[n][sl], mag[n][sl] if n in rotated else None)
                sums[s, COLS * i:COLS * (i + 1)] += x
                asums[s, COLS * i:COLS * (i + 1)] += y
            for k, (a, b, c) in enumerate(mixed):
                if b == PHI:
                    col, top = d[a][sl] * mag[PHI][sl], mag[a][sl] * mag[PHI][sl]
                else:
                    col, top = d[a][sl] * d[b][sl] * d[c][sl], mag[a][sl] * mag[b][sl] * mag[c][sl]
                sums[s, COLS * len(names) + k] += col.sum()
                asums[s, COLS * len(names) + k] += top.sum()
    return StructureFunctions2d(names, vec, mixed, sums, 1, nx * ny, abs_sums=asums, project=project, proj=proj if project else None)


class StructureFunctions2d(StructureFunctions):
    """names, vectors (n, 2) in grid points, length = |(r_x dx, r_y dy)| and angle = atan2(r_y dy, r_x dx) per vector, project: the
    rotated pair (its first name holds the longitudinal, its second the transverse component) or None, proj: the (c_x, c_y) used;
    sums, samples, points, table, mixed and the derived quantities as in StructureFunctions, one row per vector"""

    def __init__(self, names, vectors, triples, sums, samples, points, dx=None, dy=None, abs_sums=None, project=None, proj=None, ring=None):
        self.names, self.triples = list(names), list(triples)
        self.vectors = np.asarray(vectors, np.int64).reshape(-1, 2)
        self.sums, self.samples, self.points, self.abs_sums = sums, int(samples), int(points), abs_sums
        self.table = sums / (float(max(self.samples, 1)) * float(points))
        self.dx = 1.0 if dx is None else float(dx)
        self.dy = self.dx if dy is None else float(dy)
        X, Y = self.vectors[:, 0] * self.dx, self.vectors[:, 1] * self.dy
        self.length, self.angle = np.hypot(X, Y), np.arctan2(Y, X)
        self.r, self.x = None, self.length
        self.project, self.proj, self.ring = project, proj, ring
        self.mixed = {t: self.table[:, COLS * len(self.names) + k] for k, t in enumerate(self.triples)}

    def __repr__(self):
        return "StructureFunctions2d(names=%s, %d vectors, mixed=%s, project=%s, samples=%d)" % (self.names, len(self.vectors), self.triples,
                                                                                                 self.project, self.samples)

    def along(self, direction):
        """the rows with r_y = 0 (r_x > 0), for "x", or with r_x = 0, for "y", ordered by separation, as a StructureFunctions.
        (With the rotation on, the first projected name holds the component along that axis: u along x, v along y.)"""
        if direction not in ("x", "y"):
            raise ValueError("structure.along: direction = %r; valid: \"x\", \"y\"" % (direction,))
        rx, ry = self.vectors[:, 0], self.vectors[:, 1]
        rows = np.flatnonzero((ry == 0) & (rx > 0)) if direction == "x" else np.flatnonzero((rx == 0) & (ry > 0))
        r = (rx if direction == "x" else ry)[rows]
        rows = rows[np.argsort(r, kind="stable")]
        r = (rx if direction == "x" else ry)[rows]
        return StructureFunctions(self.names, r, self.triples, self.sums[rows], self.samples, self.points,
                                  dx=self.dx if direction == "x" else self.dy, abs_sums=None if self.abs_sums is None else self.abs_sums[rows])

    def isotropic(self, edges=None):
        """(radius, table, count): the equal-weight average of the table rows over the vectors whose length falls in a bin.
        edges: bin edges in length, [lo, hi) each; default: one bin per ring of ring_vectors (of a vectors=None call), else one per
        distinct length.  radius is the mean length in the bin; empty bins are dropped."""
        if edges is None:
            key = self.ring if self.ring is not None else self.length
            _, which = np.unique(key, return_inverse=True)
        else:
            edges = np.asarray(edges, np.float64)
            if edges.ndim != 1 or edges.size < 2 or np.any(np.diff(edges) <= 0):
                raise ValueError("structure.isotropic: edges %r; valid: at least two, increasing" % (edges.tolist(),))
            which = np.searchsorted(edges, self.length, side="right") - 1
            which = np.where((which >= 0) & (which < edges.size - 1), which, -1)
        bins = [b for b in np.unique(which) if b >= 0]
        radius = np.array([self.length[which == b].mean() for b in bins])
        table = np.array([self.table[which == b].mean(axis=0) for b in bins]).reshape(len(bins), self.table.shape[1])
        count = np.array([int((which == b).sum()) for b in bins], np.int64)
        return radius, table, count


def _validate2d(m, names, vectors, mixed, project, what):
    """-> (names, vectors int64 (n, 2), mixed, project or None, ring radii or None)"""
    any_size = getattr(m, "_any_size", False)
    if not any_size and not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("%s: slab-decomposed models have no structure functions yet (a row's increments are local, the sums "
                                  "would have to be added over the ranks; DESIGN.md section 7); use a single-GPU model" % what)
    names, _, mixed = _check_lists(names, [1], mixed, m.nx, what)
    if pdfs._is_qg(m) and not any_size and any(n in flow.NAMES for n in names):
        flow.refuse(m, what)
    valid = available(m)
    bad = [n for n in names if n not in valid]
    if bad:
        raise ValueError("%s: names %r; valid names for %s: %s" % (what, bad, type(m).__module__, ", ".join(valid)))
    ring = None
    if vectors is None:
        vectors, ring = _rings(m.nx, None, 8)
    vec = _check_vectors(vectors, m.nx, m.ny, what)
    return names, vec, mixed, _check_project(names, project, what), ring


class _Fused2d(object):
    """the fused contexts: nq_structure2 / nq_structure2_read, running sums on the device"""

    def __init__(self, m, names, vec, mixed, project, proj):
        self.ctx = m._ctx
        self.codes, self.vec = _iarr([_CODES[n] for n in names]), _iarr(vec)
        self.tri = _iarr([[names.index(n) for n in t] for t in mixed]).reshape(-1)
        self.pair = (names.index(project[0]), names.index(project[1])) if project else (-1, -1)
        self.proj = proj if project else None
        self.nout = COLS * len(names) + len(mixed)

    def add(self, accumulate):
        c = self.ctx
        c._chk(c.L.nq_structure2(c.h, len(self.codes), _lib._iptr(self.codes), len(self.vec), _lib._iptr(self.vec),
                                 None if self.proj is None else _lib._dptr(self.proj), self.pair[0], self.pair[1], len(self.tri) // 3,
                                 _lib._iptr(self.tri) if len(self.tri) else None, int(bool(accumulate))), "nq_structure2")

    def read(self):
        c = self.ctx
        n, out = ctypes.c_longlong(0), np.empty((len(self.vec), self.nout))
        c._chk(c.L.nq_structure2_read(c.h, ctypes.byref(n), _lib._dptr(out)), "nq_structure2_read")
        return out, int(n.value)


class _AnySize2d(object):
    """grids without a fused plan: nq_any_increments2 on the path's own planes; several states are summed here, in float64"""

    def __init__(self, m, names, vec, mixed, project, proj):
        self.m, self.names, self.vec = m, names, _iarr(vec)
        self.tri = _iarr([[names.index(n) for n in t] for t in mixed]).reshape(-1)
        self.pair = (names.index(project[0]), names.index(project[1])) if project else (-1, -1)
        self.proj = proj if project else None
        self.nout = COLS * len(names) + len(mixed)
        self.sums, self.n = None, 0

    def add(self, accumulate):
        e, m = self.m._eng, self.m
        real = [n for n in self.names if n != PHI]
        planes = m._pdf_planes(real) if real else {}
        keep, what = [], []
        for n in self.names:
            pl, w = (m._d["phi"], 2) if n == PHI else (planes[n][0], 0)
            if n != PHI and planes[n][1] == 1:             # phi2: as a plane, as in _AnySize
                pl = pl.abs2()
            keep.append(pl)                                # the planes live until the synchronous call returns
            what.append(w)
        ny, nx = keep[0].shape
        out = np.empty((len(self.vec), self.nout))
        e.chk(e.L.nq_any_increments2(e.h, len(self.names), (ctypes.c_void_p * len(keep))(*[p.ptr for p in keep]), _lib._iptr(_iarr(what)),
                                     int(ny), int(nx), len(self.vec), _lib._iptr(self.vec), None if self.proj is None else _lib._dptr(self.proj),
                                     self.pair[0], self.pair[1], len(self.tri) // 3, _lib._iptr(self.tri) if len(self.tri) else None,
                                     _lib._dptr(out)), "nq_any_increments2")
        if accumulate and self.sums is not None:
            self.sums, self.n = self.sums + out, self.n + 1
        else:
            self.sums, self.n = out, 1

    def read(self):
        return self.sums.copy(), self.n


class _Call2d(object):
    """what functions2d and Accumulator2d share: the validated call, its projection and its backend"""

    def __init__(self, m, names, vectors, mixed, project, proj, what):
        self.m = m
        self.names, self.vec, self.mixed, self.project, self.ring = _validate2d(m, names, vectors, mixed, project, what)
        self.dx, self.dy = getattr(m, "dx", None), getattr(m, "dy", None)
        self.proj = None
        if self.project is not None:
            self.proj = (unit_vectors(self.vec, 1.0 if self.dx is None else self.dx, 1.0 if self.dy is None else self.dy)
                         if proj is None else _check_proj(proj, len(self.vec), what))
        self.be = (_AnySize2d if getattr(m, "_any_size", False) else _Fused2d)(m, self.names, self.vec, self.mixed, self.project, self.proj)

    def result(self, sums, n):
        return StructureFunctions2d(self.names, self.vec, self.mixed, sums, n, self.m.nx * self.m.ny, dx=self.dx, dy=self.dy,
                                    project=self.project, proj=self.proj, ring=self.ring)


def functions2d(m, names=("u", "v", "q_psi"), vectors=None, mixed=(), project=("u", "v"), proj=None):
    """Structure functions of the model's current physical fields at two-dimensional separations, summed on the device.
    names, mixed: as in functions (every combination works at every size: the values go through physical planes); vectors: (n, 2)
    integers (r_x, r_y), r_x in [-(nx - 1), nx - 1], r_y in [0, ny - 1], at most MAX_VECS (default: ring_vectors(nx));
    project: the pair of real names rotated onto each separation vector (first name: longitudinal, second: transverse), None:
    no rotation; the default pair is dropped when the call does not name both; proj: (n, 2) numbers (c_x, c_y) in place of the
    unit vectors of (r_x dx, r_y dy).  Reads the state and writes only buffers of its own; an x-Accumulator is not disturbed."""
    call = _Call2d(m, names, vectors, mixed, project, proj, "structure.functions2d")
    if isinstance(call.be, _Fused2d):
        call.be.ctx._sf2_owner = None
    call.be.add(False)
    return call.result(*call.be.read())


class Accumulator2d(object):
    """Accumulator at two-dimensional separations: add(), result(), reset().  The context's 2-D table is separate from the one of
    functions / Accumulator; a functions2d call (or another Accumulator2d's add) on the same model in between takes it over, and
    the next add() raises instead of mixing sums."""

    def __init__(self, m, names=("u", "v", "q_psi"), vectors=None, mixed=(), project=("u", "v"), proj=None):
        self.call = _Call2d(m, names, vectors, mixed, project, proj, "structure.Accumulator2d")
        self.be, self.n = self.call.be, 0

    def _owned(self):
        return not isinstance(self.be, _Fused2d) or getattr(self.be.ctx, "_sf2_owner", None) is self

    def add(self):
        if self.n and not self._owned():
            raise RuntimeError("Accumulator2d.add: the context's table was used by another call since the last add(); reset() first")
        if isinstance(self.be, _Fused2d):
            self.be.ctx._sf2_owner = self
        self.be.add(self.n > 0)
        self.n += 1

    def result(self):
        if self.n == 0:
            return self.call.result(np.zeros((len(self.call.vec), COLS * len(self.call.names) + len(self.call.mixed))), 0)
        if not self._owned():
            raise RuntimeError("Accumulator2d.result: the context's table was used by another call since the last add()")
        return self.call.result(*self.be.read())

    def reset(self):
        self.n = 0
        if isinstance(self.be, _AnySize2d):
            self.be.sums, self.be.n = None, 0
