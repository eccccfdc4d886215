"""Vortex census: the connected regions of a thresholded field, labelled and summed on the device.

    from niwqg_amd import vortices
    C = vortices.census(m)                       # Kernel family: OW < -0.2 sigma_OW, 4-connectivity, sums of q_psi and |phi|^2
    C.n, C.total, C.truncated, C.points_in_set   # rows of the table, components found, total > capacity, points in the set
    C.label, C.area, C.x, C.y, C.radius          # per component: smallest linear index, points, periodic centroid, sqrt(area dx dy / pi)
    C.inertia(), C.axes()                        # central second moments (n, 2, 2); semi-axes and orientation of the equivalent ellipse
    C.crit_min, C.crit_max, C.sum("phi2"), C.integral("phi2"), C.mean("phi2"), C.cyclonic
    A = C.select(C.cyclonic < 0); A.share("phi2")   # the wave energy inside anticyclones, as a fraction of the plane's
    C.size_distribution([1, 4, 16, 64, 256])
    C = vortices.census(m, "q", 1.5, units="sigma", mode="abs_above", sums=("q", "phi2"), connectivity=8, labels=True); C.labels

A call names one to three different real fields (``structure.available(m)`` without ``"phi"``): the criterion and the ``sums``.
Point (y, x) is in the set when the criterion a satisfies the mode against the finite threshold t: ``below`` a < t, ``above``
a > t, ``abs_above`` |a| > t; NaN is never in the set.  ``units="sigma"`` multiplies the threshold by the standard deviation of
the criterion's plane (a range pass of its own before the census: one more store pass and one small download), ``"abs"`` passes
it through.  The components are those of the set under 4- or 8-connectivity on the doubly periodic grid; a component's label is
the smallest linear index y nx + x of its points.  The table (``Census.table``, int64, one row per component in ascending label order):

    0 label | 1 area | 2, 3 sum dx, sum dy | 4, 5, 6 sum dx^2, sum dy^2, sum dx dy | 7, 8 bits of min, max of the criterion | 9 + f sums

with dx = ((x - x0 + nx/2) mod nx) - nx/2 (dy likewise), the periodic offsets from the label's own point (y0, x0) in [-n/2, n/2):
centroid and second moments follow exactly.  A component wider than half the domain gets what this formula gives: offsets beyond
n/2 fold over, and its centroid and axes are not those of the unfolded shape.  Field sums are fixed-point integers, sum
rint(a 2^s) with s = ``fixed_point_scale(max |a|, nx ny)``: no sum over any subset of the plane can leave int64, a component's
sum is sum a to within area 2^(-s - 1), and nothing depends on the order of arrival, so two calls return the same bytes.
``capacity`` rows are kept (the first in label order); the points of later components are labelled, not summed.

``reference`` is the specification in numpy on a dict of planes; it returns the same ``Census``.
"""
import ctypes
import math

import numpy as np

from . import _lib, flow, structure
from . import pdfs as _pdfs

COLS, MAX_CAPACITY, MAX_FIELDS = _lib.VX_COLS, _lib.VX_MAX_CAPACITY, _lib.SF_MAX_FIELDS
MODES = {"below": _lib.VX_BELOW, "above": _lib.VX_ABOVE, "abs_above": _lib.VX_ABS_ABOVE}
UNITS = ("sigma", "abs")
_CODES = _pdfs._CODES
_SIGN = np.uint64(1 << 63)


def fixed_point_scale(maxabs, points):
    """s = 61 - ceil(log2(points)) - e for maxabs = m 2^e, m in [0.5, 1) (``math.frexp``); 0 for a plane of zeros (or without a
    finite value).  Every |rint(a 2^s)| is then below 2^(61 - ceil(log2 points)): no sum of ``points`` terms leaves int64."""
    maxabs = float(maxabs)
    if not (np.isfinite(maxabs) and maxabs > 0):
        return 0
    return 61 - (int(points) - 1).bit_length() - math.frexp(maxabs)[1]


def _key(a):
    """order-preserving uint64 key of float64 values (-0 < +0)"""
    b = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _SIGN)


def _in_set(a, mode, t):
    with np.errstate(invalid="ignore"):
        return a < t if mode == "below" else (a > t if mode == "above" else np.abs(a) > t)


def label_plane(mask, connectivity=4):
    """(ny, nx) int64: the smallest linear index of the component of every set point of the boolean plane on the doubly periodic
    grid, -1 outside.  A minimum-propagation fixpoint with np.roll; between sweeps every point takes its label's label."""
    mask = np.asarray(mask, bool)
    ny, nx = mask.shape
    big = ny * nx
    lab = np.where(mask, np.arange(big, dtype=np.int64).reshape(ny, nx), big)
    shifts = [(0, 1), (0, -1), (1, 0), (-1, 0)]
    if connectivity == 8:
        shifts += [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    flat_mask = mask.ravel()
    while True:
        new = lab
        for sy, sx in shifts:
            new = np.minimum(new, np.roll(lab, (sy, sx), axis=(0, 1)))
        new = np.where(mask, new, big)
        flat = new.ravel()
        for _ in range(4):
            flat[flat_mask] = flat[flat[flat_mask]]
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1)


def _offsets(d, n):
    return (d + n // 2) % n - n // 2


class Census(object):
    """names (the fields, criterion first unless the caller ordered them), criterion, mode, connectivity, threshold (absolute),
    scales {name: s}, table (n, 9 + fields) int64, n, total, truncated, points_in_set, nonfinite, plane_sums {name: sum over the
    plane}, labels ((ny, nx) int32 ranks into the table, -1 outside the set, -2 for components beyond the capacity; None unless
    requested); per component: label, area, x, y, radius, crit_min, crit_max, cyclonic"""

    def __init__(self, names, criterion, mode, connectivity, threshold, scales, table, total, points_in_set, nonfinite, shape, dx=1.0, dy=1.0,
                 plane_sums=None, labels=None, capacity=None):
        self.names, self.criterion, self.mode, self.connectivity = list(names), criterion, mode, int(connectivity)
        self.threshold = float(threshold)
        self.scales = {n: int(s) for n, s in zip(self.names, scales)}
        self.table = np.ascontiguousarray(table, np.int64).reshape(-1, COLS + len(self.names))
        self.n, self.total, self.points_in_set, self.nonfinite = len(self.table), int(total), int(points_in_set), int(nonfinite)
        self.truncated = self.total > self.n
        self.capacity = capacity
        self.ny, self.nx = int(shape[0]), int(shape[1])
        self.dx, self.dy = float(dx), float(dy)
        self.plane_sums = dict(plane_sums or {})
        self.labels = labels
        t = self.table
        self.label, self.area = t[:, 0].copy(), t[:, 1].copy()
        self.crit_min, self.crit_max = t[:, 7].copy().view(np.float64), t[:, 8].copy().view(np.float64)

    def __repr__(self):
        return "Census(%s %s %g, %d-connectivity: %d of %d components, %d points)" % (self.criterion, self.mode, self.threshold, self.connectivity, self.n,
                                                                                       self.total, self.points_in_set)

    def info(self):
        """the seven entries nq_vortex_read returns"""
        s = [self.scales[n] for n in self.names] + [0] * (MAX_FIELDS - len(self.names))
        return np.array([self.total, self.n, self.points_in_set, self.nonfinite] + s, np.int64)

    # ---- geometry, exact from the integer moments
    def _mean_offsets(self):
        a = self.area.astype(np.float64)
        return self.table[:, 2] / a, self.table[:, 3] / a

    @property
    def x(self):
        mx, _ = self._mean_offsets()
        return ((self.label % self.nx + mx) % self.nx) * self.dx

    @property
    def y(self):
        _, my = self._mean_offsets()
        return ((self.label // self.nx + my) % self.ny) * self.dy

    @property
    def radius(self):
        return np.sqrt(self.area * (self.dx * self.dy / np.pi))

    def inertia(self):
        """(n, 2, 2): [[<dx dx>, <dx dy>], [<dx dy>, <dy dy>]] about the centroid, in length units squared"""
        a = self.area.astype(np.float64)
        mx, my = self._mean_offsets()
        t = self.table
        xx = (t[:, 4] / a - mx * mx) * self.dx ** 2
        yy = (t[:, 5] / a - my * my) * self.dy ** 2
        xy = (t[:, 6] / a - mx * my) * self.dx * self.dy
        return np.stack([np.stack([xx, xy], axis=1), np.stack([xy, yy], axis=1)], axis=1)

    def axes(self):
        """(a, b, angle): semi-axes a >= b of the ellipse with these second moments (a uniform ellipse has variance a^2 / 4 along
        its major axis) and the angle of the major axis from x, in (-pi/2, pi/2]"""
        I = self.inertia()
        xx, yy, xy = I[:, 0, 0], I[:, 1, 1], I[:, 0, 1]
        mean, diff = 0.5 * (xx + yy), np.hypot(0.5 * (xx - yy), xy)
        return 2.0 * np.sqrt(np.maximum(mean + diff, 0.0)), 2.0 * np.sqrt(np.maximum(mean - diff, 0.0)), 0.5 * np.arctan2(2.0 * xy, xx - yy)

    # ---- the sums
    def _index(self, name):
        if name not in self.names:
            raise ValueError("vortices: no field %r in this census (%s)" % (name, ", ".join(self.names)))
        return self.names.index(name)

    def sum(self, name):
        """sum of the field over each component: the fixed-point sums times 2^-s"""
        f = self._index(name)
        return np.ldexp(self.table[:, COLS + f].astype(np.float64), -self.scales[name])

    def integral(self, name):
        return self.sum(name) * (self.dx * self.dy)

    def mean(self, name):
        return self.sum(name) / self.area

    @property
    def cyclonic(self):
        """the sign of the component's sum of q_psi (of q where the census has no q_psi): +1 cyclonic, -1 anticyclonic"""
        for name in ("q_psi", "q"):
            if name in self.names:
                return np.sign(self.table[:, COLS + self.names.index(name)]).astype(np.int64)
        raise ValueError("vortices: cyclonic needs q_psi or q among the fields of the census (%s)" % ", ".join(self.names))

    def _which(self, which):
        if which is None:
            return np.ones(self.n, bool)
        which = np.asarray(which)
        if which.dtype == bool:
            if which.shape != (self.n,):
                raise ValueError("vortices: a mask of shape %r for %d components" % (which.shape, self.n))
            return which
        keep = np.zeros(self.n, bool)
        keep[which.astype(np.int64)] = True
        return keep

    def select(self, mask_or_min_area):
        """the Census of the chosen components: a boolean mask or an index array over the rows, or a number: area >= it.  total,
        points_in_set and plane_sums stay those of the plane; labels are renumbered, the dropped components become -1."""
        if np.ndim(mask_or_min_area) == 0 and not isinstance(mask_or_min_area, (bool, np.bool_)):
            keep = self.area >= mask_or_min_area
        else:
            keep = self._which(mask_or_min_area)
        labels = None
        if self.labels is not None:
            new = np.append(np.where(keep, np.cumsum(keep) - 1, -1), [-2, -1]).astype(np.int32)     # new[-2] = -2, new[-1] = -1
            labels = new[self.labels]
        out = Census(self.names, self.criterion, self.mode, self.connectivity, self.threshold, [self.scales[n] for n in self.names], self.table[keep],
                     self.total, self.points_in_set, self.nonfinite, (self.ny, self.nx), self.dx, self.dy, self.plane_sums, labels, self.capacity)
        out.truncated = self.truncated
        return out

    def share(self, name, which=None):
        """the fraction of the plane's sum of ``name`` held by the chosen components (all of them by default)"""
        self._index(name)
        if name not in self.plane_sums:
            raise ValueError("vortices: no plane sum of %r in this census" % name)
        return float(self.sum(name)[self._which(which)].sum() / self.plane_sums[name])

    def size_distribution(self, edges):
        """components per bin of area in points: edges as numpy.histogram takes them -> int64 counts"""
        return np.histogram(self.area, bins=np.asarray(edges))[0].astype(np.int64)


def _ranks(lab, labels_in_table):
    """the label plane as ranks into the table: -1 outside the set, -2 for a component that is not in the table"""
    lab = np.asarray(lab, np.int64)
    n = len(labels_in_table)
    r = np.searchsorted(labels_in_table, lab)
    hit = r < n
    hit[hit] = labels_in_table[r[hit]] == lab[hit]
    return np.where(lab < 0, -1, np.where(hit, r, -2)).astype(np.int32)


# ---- the specification in numpy -----------------------------------------------------------------------------------------------------
def reference(fields, criterion, mode, threshold, connectivity=4, capacity=None):
    """THE definitions in numpy, from a dict {name: (ny, nx) real plane}: every field is summed, ``criterion`` names the one that is
    thresholded (absolute threshold).  Returns a Census with labels; capacity None: every component."""
    what = "vortices.reference"
    names = list(fields)
    planes = {n: np.asarray(fields[n], np.float64) for n in names}
    shapes = set(p.shape for p in planes.values())
    if not 1 <= len(names) <= MAX_FIELDS or len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError("%s: 1 to %d planes of one (ny, nx) shape, got %r" % (what, MAX_FIELDS, sorted(shapes)))
    if criterion not in names:
        raise ValueError("%s: criterion %r is not among the fields (%s)" % (what, criterion, ", ".join(names)))
    _check_call(mode, threshold, "abs", connectivity, MAX_CAPACITY if capacity is None else capacity, what)
    ny, nx = next(iter(shapes))
    a = planes[criterion]
    mask = _in_set(a, mode, float(threshold))
    lab = label_plane(mask, connectivity)
    scales, sums, nonfinite = [], {}, 0
    for n in names:
        ok = np.isfinite(planes[n])
        nonfinite += int(ok.size - ok.sum())
        scales.append(fixed_point_scale(np.abs(planes[n][ok]).max() if ok.any() else 0.0, nx * ny))
        sums[n] = float(planes[n][ok].sum())
    at = np.flatnonzero(mask.ravel())
    l = lab.ravel()[at]
    order = np.argsort(l, kind="stable")
    at, l = at[order], l[order]
    labels, starts = np.unique(l, return_index=True)
    total = len(labels)
    tab = np.zeros((total, COLS + len(names)), np.int64)
    if total:
        dx = _offsets(at % nx - l % nx, nx)
        dy = _offsets(at // nx - l // nx, ny)
        red = lambda v: np.add.reduceat(np.asarray(v, np.int64), starts)
        tab[:, 0] = labels
        tab[:, 1] = red(np.ones(len(at)))
        tab[:, 2], tab[:, 3] = red(dx), red(dy)
        tab[:, 4], tab[:, 5], tab[:, 6] = red(dx * dx), red(dy * dy), red(dx * dy)
        k = _key(a.ravel()[at])
        lo, hi = np.minimum.reduceat(k, starts), np.maximum.reduceat(k, starts)
        unkey = lambda k: np.where(k >> np.uint64(63) != 0, k & ~_SIGN, ~k)
        tab[:, 7], tab[:, 8] = unkey(lo).view(np.int64), unkey(hi).view(np.int64)
        for f, n in enumerate(names):
            v = planes[n].ravel()[at]
            with np.errstate(invalid="ignore", over="ignore"):
                term = np.where(np.isfinite(v), np.rint(np.ldexp(np.where(np.isfinite(v), v, 0.0), scales[f])), 0.0)
            tab[:, COLS + f] = red(term.astype(np.int64))
    keep = total if capacity is None else min(total, int(capacity))
    return Census(names, criterion, mode, connectivity, threshold, scales, tab[:keep], total, len(at), nonfinite, (ny, nx), plane_sums=sums,
                  labels=_ranks(lab, tab[:keep, 0]), capacity=capacity)


# ---- the device -----------------------------------------------------------------------------------------------------------------------
def _check_call(mode, threshold, units, connectivity, capacity, what):
    if mode not in MODES:
        raise ValueError("%s: mode = %r; valid: %s" % (what, mode, ", ".join(MODES)))
    if units not in UNITS:
        raise ValueError("%s: units = %r; valid: \"sigma\" (threshold times the plane's standard deviation), \"abs\"" % (what, units))
    try:
        ok = np.ndim(threshold) == 0 and np.isfinite(float(threshold))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: threshold = %r; valid: a finite number" % (what, threshold))
    if connectivity not in (4, 8) or isinstance(connectivity, (bool, np.bool_)):
        raise ValueError("%s: connectivity = %r; valid: 4 (edges) or 8 (edges and corners)" % (what, connectivity))
    if not (isinstance(capacity, (int, np.integer)) and not isinstance(capacity, (bool, np.bool_)) and 1 <= capacity <= MAX_CAPACITY):
        raise ValueError("%s: capacity = %r; valid: 1 to %d rows of the table" % (what, capacity, MAX_CAPACITY))


def available(m):
    """the names census(m) takes: structure.available(m) without the complex "phi\""""
    return [n for n in structure.available(m) if n != structure.PHI]


def _validate(m, criterion, threshold, units, mode, sums, connectivity, capacity, what="vortices.census"):
    """every ValueError / NotImplementedError of the contract, before any device call -> (names, criterion, mode, threshold)"""
    any_size = getattr(m, "_any_size", False)
    if not any_size and not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("%s: slab-decomposed models have no vortex census yet (a component crosses the slabs: the labels would have "
                                  "to be united over the ranks; DESIGN.md section 7); use a single-GPU model" % what)
    qg = _pdfs._is_qg(m)
    if criterion is None:
        criterion = "q" if qg else "ow"
        if threshold == -0.2 and qg:
            threshold = 1.0
    if mode is None:
        mode = "abs_above" if qg else "below"
    if sums is None:
        sums = () if qg else ("q_psi", "phi2")
    sums = [sums] if isinstance(sums, str) else list(sums)
    if not isinstance(criterion, str) or any(not isinstance(n, str) for n in sums):
        raise ValueError("%s: criterion and sums are field names, got %r and %r" % (what, criterion, sums))
    if len(set(sums)) != len(sums):
        raise ValueError("%s: sums = %r names a field twice" % (what, sums))
    names = [criterion] + [n for n in sums if n != criterion]
    if structure.PHI in names:
        raise ValueError("%s: \"phi\" is complex: a census thresholds and sums real fields (\"phi2\" is |phi|^2; DESIGN.md section 7)" % what)
    if len(names) > MAX_FIELDS:
        raise ValueError("%s: %d different fields (%s); valid: 1 to %d per call, the criterion included" % (what, len(names), ", ".join(names), MAX_FIELDS))
    if qg and not any_size and any(n in flow.NAMES for n in names):
        flow.refuse(m, what)
    valid = available(m)
    bad = [n for n in names if n not in valid]
    if bad:
        raise ValueError("%s: names %r; valid names for %s: %s" % (what, bad, type(m).__module__, ", ".join(valid)))
    _check_call(mode, threshold, units, connectivity, capacity, what)
    return names, criterion, mode, float(threshold)


def _llp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))


class _Fused(object):
    """the fused contexts: nq_vortex_range / nq_vortex_census / nq_vortex_read / nq_vortex_labels; the table stays on the device
    until it is read"""

    def __init__(self, m, names):
        self.ctx, self.names = m._ctx, names
        self.codes = np.ascontiguousarray([_CODES[n] for n in names], np.int32)
        self.shape = (m.ny, m.nx)

    def range(self):
        c, out = self.ctx, np.empty((len(self.names), 4))
        c._chk(c.L.nq_vortex_range(c.h, len(self.codes), _lib._iptr(self.codes), _lib._dptr(out)), "nq_vortex_range")
        return out[:, 2], out[:, 3]

    def run(self, crit, mode, threshold, connectivity, capacity, labels):
        c, nf = self.ctx, len(self.names)
        c._chk(c.L.nq_vortex_census(c.h, nf, _lib._iptr(self.codes), crit, MODES[mode], threshold, connectivity, capacity), "nq_vortex_census")
        info = np.zeros(7, np.int64)
        c._chk(c.L.nq_vortex_read(c.h, _llp(info), None), "nq_vortex_read")           # the rows first: the table is sized by them
        tab = np.zeros((int(info[1]), COLS + nf), np.int64)
        if len(tab):
            c._chk(c.L.nq_vortex_read(c.h, _llp(info), _llp(tab)), "nq_vortex_read")
        stats = np.empty((nf, 4))
        c._chk(c.L.nq_vortex_stats(c.h, _lib._dptr(stats)), "nq_vortex_stats")        # the plane sums of the census's own range pass
        lab = None
        if labels:
            lab = np.empty(self.shape, np.int32)
            c._chk(c.L.nq_vortex_labels(c.h, _lib._iptr(lab)), "nq_vortex_labels")
        return info, tab, lab, stats[:, 2]


class _AnySize(object):
    """grids without a fused plan: the path's own planes through nq_any_components (the same kernels)"""

    def __init__(self, m, names):
        self.m, self.names = m, names
        self.shape = (m.ny, m.nx)

    def _planes(self):
        planes = self.m._pdf_planes(self.names)
        return [planes[n][0].abs2() if planes[n][1] == 1 else planes[n][0] for n in self.names]      # phi2: as a plane

    def range(self):
        keep = self._planes()
        s = np.array([complex(p.sum()).real for p in keep])
        ss = np.array([(p if p.isreal else p.real).sumabs2() for p in keep])
        return s, ss

    def run(self, crit, mode, threshold, connectivity, capacity, labels):
        e, nf = self.m._eng, len(self.names)
        keep = self._planes()                                  # the planes live until the synchronous call returns
        ny, nx = keep[0].shape
        info, tab = np.zeros(7, np.int64), np.zeros((capacity, COLS + nf), np.int64)
        lab = np.empty((ny, nx), np.int32) if labels else None
        e.chk(e.L.nq_any_components(e.h, nf, (ctypes.c_void_p * nf)(*[p.ptr for p in keep]), int(ny), int(nx), crit, MODES[mode], threshold,
                                    connectivity, capacity, _llp(info), _llp(tab), None if lab is None else _lib._iptr(lab)), "nq_any_components")
        return info, tab[:info[1]].copy(), lab, self.range()[0]


def census(m, criterion=None, threshold=-0.2, units="sigma", mode=None, sums=None, connectivity=4, capacity=65536, labels=False):
    """The census of the model's current state.  Kernel family defaults: criterion "ow", mode "below", sums ("q_psi", "phi2"): the
    classical OW < -0.2 sigma_OW; QGModel defaults: criterion "q", mode "abs_above", threshold 1.0 (sigma), no further sums (the
    signature's -0.2 becomes 1.0 there only while the criterion is left to the default too).
    Reads the state and writes only buffers of its own and the plane pool of structure.functions2d.  A non-finite value in a field
    of the call raises FloatingPointError after the read."""
    names, criterion, mode, threshold = _validate(m, criterion, threshold, units, mode, sums, connectivity, capacity)
    be = (_AnySize if getattr(m, "_any_size", False) else _Fused)(m, names)
    points = m.nx * m.ny
    if units == "sigma":
        s, ss = be.range()
        mean = s[0] / points
        threshold = threshold * math.sqrt(max(ss[0] / points - mean * mean, 0.0))
        if not np.isfinite(threshold):
            raise FloatingPointError("vortices.census: the standard deviation of %r is not finite" % criterion)
    info, tab, lab, s = be.run(0, mode, float(threshold), int(connectivity), int(capacity), bool(labels))
    if info[3]:
        raise FloatingPointError("vortices.census: %d non-finite values in the fields %s" % (info[3], ", ".join(names)))
    return Census(names, criterion, mode, connectivity, threshold, info[4:4 + len(names)], tab, info[0], info[2], info[3], (m.ny, m.nx),
                  getattr(m, "dx", 1.0), getattr(m, "dy", 1.0), dict(zip(names, s)), None if lab is None else _ranks(lab, tab[:, 0]), int(capacity))
