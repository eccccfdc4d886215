"""PDFs and joint PDFs of the physical fields, binned on the device.

``field_pdfs(m)`` counts the values of q, q_psi and |phi|^2 (QGModel: q and its passive scalar c) of the model's current state
into uniform bins: the row pass of the diagnostics tick holds exactly these values in registers (``k_x_diag``), and
``k_x_hist`` bins them there instead of summing them.  Only the integer tables leave the GPU, a few KB instead of three
planes, and no physical plane is written on the device either.  Counts are integers, so the result is bit-reproducible.

The bin rule (``bin_index`` restates it in numpy; host and device use fp64): with s = bins / (hi - lo), a value x goes to
NaN if x != x, below if x < lo, above if x > hi, else bin min(int(floor((x - lo) * s)), bins - 1); x == hi is in the last bin.
This is ``numpy.histogram``'s result except for values within a few ulp of an edge, where numpy's own rule (a search in the
edge array) may decide the other way.

``q``, ``q_psi`` and phi are what the tick's physical sums see: the rows of the last inversion (dual-copy contexts: the mean
of the two q-hat copies, whose real field is ``m.q``), so ``set_phi`` after ``set_q`` leaves ``q_psi`` wave-free until the
first step exactly as it does ``m.q_psi`` (quirk Q2).  UnCoupledModel and YBJModel have q_psi = q.

``conditional_mean`` comes from the joint table and b's bin centres, so it is accurate to half a bin of b.
"""
import numpy as np

from . import _lib, flow

KERNEL_NAMES = ("q", "q_psi", "phi2")
MAX_BINS, MAX_JOINT_BINS = _lib.PDF_MAX_BINS, _lib.PDF_MAX_JOINT_BINS
_CODES = {"q": _lib.PDF_Q, "q_psi": _lib.PDF_QPSI, "phi2": _lib.PDF_PHI2, "c": _lib.PDF_C}
_CODES.update(flow.CODES)           # the flow fields (flow.py): taken by name only, never a default


def bin_index(x, lo, hi, bins):
    """the bin rule in numpy: bin of every x (int64), below = -1, above = bins, NaN = bins + 1"""
    x = np.asarray(x, np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    s = np.float64(bins) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (x >= lo) & (x <= hi)
        i = np.floor((np.where(ok, x, lo) - lo) * s).astype(np.int64)
    i = np.minimum(i, bins - 1)
    i = np.where(x < lo, -1, i)
    i = np.where(x > hi, bins, i)
    return np.where(x != x, bins + 1, i)


def _is_qg(m):
    from .QGModel import Model as QG
    return isinstance(m, QG)


def available(m):
    """names of the fields field_pdfs(m) can bin for this model"""
    if _is_qg(m):
        return ["q", "c"] if m.passive_scalar else ["q"]
    return list(KERNEL_NAMES)


class JointTable(object):
    """names (a, b); counts (joint_bins, joint_bins) int64 indexed [bin of b][bin of a]; edges_a, edges_b; outside: points with
    either value out of its range or NaN"""

    def __init__(self, names, counts, edges_a, edges_b, outside):
        self.names, self.counts, self.edges_a, self.edges_b, self.outside = names, counts, edges_a, edges_b, outside


class ConditionalMean(object):
    """mean: E[b | a in bin] per a-bin (NaN where the a-bin is empty), from b's bin centres: accurate to half a bin of b;
    counts: points per a-bin; centres: the a-bin centres"""

    def __init__(self, mean, counts, centres):
        self.mean, self.counts, self.centres = mean, counts, centres


class FieldPDFs(object):
    """counts / edges / below / above / nan: dicts by field name (see the module text); joint: a JointTable or None"""

    def __init__(self, counts, edges, below, above, nan, joint=None):
        self.counts, self.edges, self.below, self.above, self.nan, self.joint = counts, edges, below, above, nan, joint

    def __repr__(self):
        return "FieldPDFs(names=%s, joint=%s)" % (sorted(self.counts), self.joint.names if self.joint else None)

    def centres(self, name):
        e = self.edges[name]
        return 0.5 * (e[:-1] + e[1:])

    def density(self, name):
        """counts / (in-range total * bin width): integrates to one over [lo, hi]"""
        n, e = self.counts[name], self.edges[name]
        return n / (float(n.sum()) * np.diff(e))

    def moments(self, name):
        """(mean, variance, skewness, kurtosis) of the in-range points, from the bin centres"""
        n, c = self.counts[name].astype(np.float64), self.centres(name)
        tot = n.sum()
        mean = (n * c).sum() / tot
        d = c - mean
        var = (n * d ** 2).sum() / tot
        with np.errstate(invalid="ignore", divide="ignore"):
            return mean, var, (n * d ** 3).sum() / tot / var ** 1.5, (n * d ** 4).sum() / tot / var ** 2

    def conditional_mean(self):
        """E[b | a-bin] of the joint pair (a, b)"""
        if self.joint is None:
            raise ValueError("conditional_mean: no joint table (field_pdfs(..., joint=(a, b)))")
        J = self.joint
        n = J.counts.astype(np.float64)
        cb = 0.5 * (J.edges_b[:-1] + J.edges_b[1:])
        per_a = J.counts.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (n * cb[:, None]).sum(axis=0) / per_a
        return ConditionalMean(mean, per_a, 0.5 * (J.edges_a[:-1] + J.edges_a[1:]))


def _check_range(name, r):
    try:
        lo, hi = float(r[0]), float(r[1])
    except Exception:
        raise ValueError("field_pdfs: range of %r must be (lo, hi), got %r" % (name, r))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("field_pdfs: range of %r must be finite with lo < hi, got (%r, %r)" % (name, lo, hi))
    return lo, hi


def _validate(m, names, bins, ranges, joint, joint_bins, need_ranges=False):
    """every ValueError / NotImplementedError of the contract, before any device call -> (names, ranges dict, joint)"""
    valid = available(m)
    if names is None:
        names = list(valid)
    else:
        names = [names] if isinstance(names, str) else list(names)
    if any(n in flow.NAMES for n in names if isinstance(n, str)):
        flow.refuse(m, "field_pdfs", linked=joint is not None and len(names) > 1)
    by_name = flow.available(m)
    bad = [n for n in names if n not in valid and n not in by_name]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError("field_pdfs: names %r; valid names for %s (each once): %s%s" % (names, type(m).__module__, ", ".join(valid),
                         "; by name only (flow.py): " + ", ".join(by_name) if by_name else ""))
    if len(names) > 3:
        raise ValueError("field_pdfs: %d names; valid: 1 to 3 per call (the value registers of the row pass)" % len(names))
    if not (isinstance(bins, (int, np.integer)) and 1 <= bins <= MAX_BINS):
        raise ValueError("field_pdfs: bins = %r; valid: 1 to %d (the LDS tables of a workgroup)" % (bins, MAX_BINS))
    if joint is not None:
        joint = tuple(joint)
        if len(joint) != 2 or joint[0] == joint[1] or any(n not in names for n in joint):
            raise ValueError("field_pdfs: joint = %r; valid: an ordered pair of two different names out of %s" % (joint, ", ".join(names)))
        if not (isinstance(joint_bins, (int, np.integer)) and 1 <= joint_bins <= MAX_JOINT_BINS):
            raise ValueError("field_pdfs: joint_bins = %r; valid: 1 to %d (the LDS tables of a workgroup)" % (joint_bins, MAX_JOINT_BINS))
    ranges = dict(ranges or {})
    unknown = [n for n in ranges if n not in names]
    if unknown:
        raise ValueError("field_pdfs: ranges given for %r; the binned names are %s" % (unknown, ", ".join(names)))
    ranges = {n: _check_range(n, r) for n, r in ranges.items()}
    if need_ranges and any(n not in ranges for n in names):
        raise ValueError("Accumulator: explicit ranges are mandatory for every name (%s): counts of several states need fixed edges"
                         % ", ".join(names))
    if not getattr(m, "_any_size", False) and not isinstance(m._ctx, _lib.Context):
        raise NotImplementedError("field_pdfs: slab-decomposed models have no PDFs yet (the tables would have to be summed over the "
                                  "ranks); use a single-GPU model")
    return names, ranges, joint


class _Fused(object):
    """the fused contexts: nq_field_minmax / nq_field_hist / nq_field_hist_read"""

    def __init__(self, m):
        self.ctx = m._ctx

    def minmax(self, names):
        return dict(zip(names, self.ctx.field_minmax([_CODES[n] for n in names])))

    def bin(self, names, ranges, bins, joint, joint_bins, accumulate):
        self.ctx.field_hist([_CODES[n] for n in names], [ranges[n][0] for n in names], [ranges[n][1] for n in names], bins,
                            None if joint is None else (_CODES[joint[0]], _CODES[joint[1]]), joint_bins if joint else 0, accumulate)

    def read(self, names, bins, joint, joint_bins):
        return self.ctx.field_hist_read(len(names), bins, joint_bins if joint else 0)


class _AnySize(object):
    """grids without a fused plan: the path's own planes through nq_any_minmax / nq_any_hist / nq_any_hist2.  The engine's calls
    return their tables, so several states are summed here, in integers."""

    def __init__(self, m):
        self.m = m
        self.tab = self.jtab = None

    def minmax(self, names):
        import ctypes
        e, out = self.m._eng, {}
        for n, (pl, what) in self.m._pdf_planes(names).items():
            v = np.empty(2)
            e.chk(e.L.nq_any_minmax(e.h, ctypes.c_void_p(pl.ptr), pl.size, what, _lib._dptr(v)), "nq_any_minmax")
            out[n] = (float(v[0]), float(v[1]))
        return out

    def bin(self, names, ranges, bins, joint, joint_bins, accumulate):
        import ctypes
        ullp = ctypes.POINTER(ctypes.c_ulonglong)
        e = self.m._eng
        planes = self.m._pdf_planes(names)
        tab = np.zeros((len(names), bins + 3), np.uint64)
        for i, n in enumerate(names):
            pl, what = planes[n]
            e.chk(e.L.nq_any_hist(e.h, ctypes.c_void_p(pl.ptr), pl.size, what, ranges[n][0], ranges[n][1], bins,
                                  tab[i].ctypes.data_as(ullp)), "nq_any_hist")
        jtab = None
        if joint is not None:
            (pa, wa), (pb, wb) = planes[joint[0]], planes[joint[1]]
            lo2 = np.array([ranges[joint[0]][0], ranges[joint[1]][0]])
            hi2 = np.array([ranges[joint[0]][1], ranges[joint[1]][1]])
            jtab = np.zeros(joint_bins * joint_bins + 1, np.uint64)
            e.chk(e.L.nq_any_hist2(e.h, ctypes.c_void_p(pa.ptr), ctypes.c_void_p(pb.ptr), pa.size, wa, wb, _lib._dptr(lo2),
                                   _lib._dptr(hi2), joint_bins, jtab.ctypes.data_as(ullp)), "nq_any_hist2")
        if accumulate and self.tab is not None:
            tab += self.tab
            if jtab is not None:
                jtab += self.jtab
        self.tab, self.jtab = tab, jtab

    def read(self, names, bins, joint, joint_bins):
        return self.tab, self.jtab


def _backend(m):
    return _AnySize(m) if getattr(m, "_any_size", False) else _Fused(m)


def _default_ranges(be, names, ranges):
    missing = [n for n in names if n not in ranges]
    if missing:
        for n, (lo, hi) in be.minmax(missing).items():
            if not (np.isfinite(lo) and np.isfinite(hi)):
                raise ValueError("field_pdfs: field %r is not finite (min %r, max %r); give an explicit range to count its NaNs and "
                                 "infinities" % (n, lo, hi))
            ranges[n] = (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)
    return ranges


def _result(names, ranges, bins, joint, joint_bins, tab, jtab):
    tab = tab.astype(np.int64)
    counts = {n: tab[i, :bins].copy() for i, n in enumerate(names)}
    below = {n: int(tab[i, bins]) for i, n in enumerate(names)}
    above = {n: int(tab[i, bins + 1]) for i, n in enumerate(names)}
    nan = {n: int(tab[i, bins + 2]) for i, n in enumerate(names)}
    edges = {n: np.linspace(ranges[n][0], ranges[n][1], bins + 1) for n in names}
    J = None
    if joint is not None:
        jt = jtab.astype(np.int64)
        a, b = joint
        J = JointTable((a, b), jt[:-1].reshape(joint_bins, joint_bins).copy(), np.linspace(ranges[a][0], ranges[a][1], joint_bins + 1),
                       np.linspace(ranges[b][0], ranges[b][1], joint_bins + 1), int(jt[-1]))
    return FieldPDFs(counts, edges, below, above, nan, J)


def field_pdfs(m, names=None, bins=256, ranges=None, joint=None, joint_bins=64):
    """Histograms (and one optional joint table) of the model's current physical fields, counted on the device.
    names: a subset of available(m) (default: all); ranges: {name: (lo, hi)}, names without an entry get the field's exact
    minimum and maximum from a device pass of their own; joint: an ordered pair (a, b) of the binned names.
    May be called wherever isotropic_spectra may; reads the state and writes only buffers of its own."""
    names, ranges, joint = _validate(m, names, bins, ranges, joint, joint_bins)
    be = _backend(m)
    ranges = _default_ranges(be, names, ranges)
    if isinstance(be, _Fused):
        be.ctx._hist_owner = None
    be.bin(names, ranges, int(bins), joint, int(joint_bins), False)
    tab, jtab = be.read(names, int(bins), joint, int(joint_bins))
    return _result(names, ranges, int(bins), joint, int(joint_bins), tab, jtab)


class Accumulator(object):
    """Counts of several states with fixed edges: add() bins the current state on top of what the tables hold (on the device for
    the fused contexts: one read at result(); summed in integers on the host for the any-size path), result() returns the
    FieldPDFs, reset() starts over.  A context has one set of tables: a field_pdfs call (or another Accumulator's add) on the
    same model in between takes them over, and the next add() raises instead of mixing counts."""

    def __init__(self, m, ranges, names=None, bins=256, joint=None, joint_bins=64):
        self.names, self.ranges, self.joint = _validate(m, names, bins, ranges, joint, joint_bins, need_ranges=True)
        self.bins, self.joint_bins = int(bins), int(joint_bins)
        self.be = _backend(m)
        self.n = 0

    def add(self):
        be = self.be
        if isinstance(be, _Fused):
            if self.n and getattr(be.ctx, "_hist_owner", None) is not self:
                raise RuntimeError("Accumulator.add: the context's tables were used by another call since the last add(); reset() first")
            be.ctx._hist_owner = self
        be.bin(self.names, self.ranges, self.bins, self.joint, self.joint_bins, self.n > 0)
        self.n += 1

    def result(self):
        if self.n == 0:
            raise RuntimeError("Accumulator.result: nothing added yet")
        be = self.be
        if isinstance(be, _Fused) and getattr(be.ctx, "_hist_owner", None) is not self:
            raise RuntimeError("Accumulator.result: the context's tables were used by another call since the last add()")
        tab, jtab = be.read(self.names, self.bins, self.joint, self.joint_bins)
        return _result(self.names, self.ranges, self.bins, self.joint, self.joint_bins, tab, jtab)

    def reset(self):
        self.n = 0
        if isinstance(self.be, _AnySize):
            self.be.tab = self.be.jtab = None
