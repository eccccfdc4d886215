"""PDFs of the field increments on the device (niwqg_amd/increments.py, csrc/nq_ipdf.hpp): the counts of
every route against ``increments.reference`` on the device's own planes and against the independent restatement ``flow.reference``,
the large LDS plans, QGModel and the any-size path, two-dimensional separations with and without the rotation, determinism,
accumulation, isolation from ``structure`` and ``pdfs``, zero and NaN fields, and the refusals.

The condition (the form of tests/test_gpu_pdfs.py): per (name, separation) the L1 distance of [below, counts, above] to the
reference is at most 2 n_near, n_near = the increments within 1e-11 (hi - lo) of an edge (plus what a test adds for its own
value tolerance); n_near <= 8 or the case is declared badly posed and fails; ``nan`` is 0 and the row closes on nx ny exactly.
The allowance covers |d phi| = sqrt(dr^2 + di^2) against numpy's ``abs`` and the compiler's freedom to contract; where the values
are bit-identical L1 is 0.

Expected n_near: points x edges x 2e-11 x the density at an edge, about 1e-5 per table of ``make``'s continuous random states
under sigma-scaled ranges.  Confirmed once on the CPU: ``make``-like planes (filtered Gaussian noise) at 128^2, the three name
groups, separations(128), 64 bins, +-8 sigma: n_near = 0 in all 72 tables, so the reference alone stays far inside the cap."""
import ctypes

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs
from test_gpu_flow import make, advance, device_values, KINDS, SIZES
from test_gpu_structure import separations, own_planes, GROUPS, qg_with_scalar

pytestmark = pytest.mark.gpu

BINS = 64


def near_edges(x, lo, hi, bins, delta):
    """points of x within delta of one of the bins + 1 edges"""
    t = (np.ravel(x) - lo) * (bins / (hi - lo))
    k = np.clip(np.rint(t), 0, bins)
    return int((np.abs(np.ravel(x) - (lo + (hi - lo) * k / bins)) <= delta).sum())


def check(P, planes, tag, extra=None, samples=1, points=None):
    """the condition of the module text for every (name, row) of P; extra(name, values): what a test adds to the edge tolerance"""
    from niwqg_amd import increments
    two = isinstance(P, increments.IncrementPDFs2d)
    where = P.vectors if two else P.r
    fields = {n: planes[n] for n in P.names}
    R = increments.reference(fields, where, bins=P.bins, ranges=P.ranges, project=P.project if two else None, proj=P.proj if two else None)
    points = points or next(iter(fields.values())).size
    worst_near = worst_l1 = 0
    for s in range(len(where)):
        v = increments.binned_values(fields, where[s], P.project if two else None, P.proj[s] if two and P.project else None)
        for n in P.names:
            lo, hi = P.ranges[n][s]
            assert np.array_equal(P.edges[n][s], lo + (hi - lo) * np.arange(P.bins + 1) / P.bins)
            near = near_edges(v[n], lo, hi, P.bins, 1e-11 * (hi - lo) + (extra(n, v[n]) if extra else 0.0))
            assert near <= 8, "badly posed: %s %s row %d: %d increments within the tolerance of an edge" % (tag, n, s, near)
            got = np.concatenate([[P.below[n][s]], P.counts[n][s], [P.above[n][s]]])
            ref = np.concatenate([[R.below[n][s]], R.counts[n][s], [R.above[n][s]]])
            l1 = int(np.abs(got - ref).sum())
            worst_near, worst_l1 = max(worst_near, near), max(worst_l1, l1)
            assert l1 <= 2 * near, (tag, n, s, l1, near)
            assert P.nan[n][s] == 0 and got.sum() == samples * points, (tag, n, s, P.nan[n][s], got.sum())
            assert (P.counts[n][s] > 0).sum() >= min(3, P.bins), (tag, n, s)         # several bins are populated
    assert P.samples == samples and P.points == points
    print("%s: max n_near %d, max L1 %d" % (tag, worst_near, worst_l1))
    return R


# ---- 1. counts against the device's own planes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_counts_equal_numpy_on_the_device_planes(kind, nx):
    from niwqg_amd import increments
    m = make(kind, nx)
    sep = separations(nx)
    for state in ("set", "3 steps"):
        if state != "set":
            advance(m, 3, batched=True)
        for names, _ in GROUPS:
            P = increments.pdfs(m, names=names, separations=sep, bins=BINS)
            check(P, device_values(m, names), "%s %d %s %s" % (kind, nx, state, "/".join(names)))


# ---- 2. against the independent restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("ybj", 512), ("uncoupled", 1024)])
def test_against_the_restatement(kind, nx):
    from niwqg_amd import flow, increments, structure
    m = make(kind, nx)
    advance(m, 2, batched=True)
    names, sep = ("u", "v", "q_psi"), separations(nx)
    ref = flow.reference(m, ("u", "v"))
    ref["q_psi"] = np.array(m.q_psi, np.float64)
    S = structure.reference({n: ref[n] for n in names}, sep)
    ranges = {n: np.stack([-6 * np.sqrt(S.moment(n, 2)), 6 * np.sqrt(S.moment(n, 2))], axis=1) for n in names}
    P = increments.pdfs(m, names=names, separations=sep, bins=BINS, ranges=ranges)
    top = {n: np.abs(ref[n]).max() for n in names}
    check(P, ref, "%s %d restatement" % (kind, nx), extra=lambda n, v: 2e-12 * top[n])


# ---- 3. large plans ----------------------------------------------------------------------------------------------------------------
def test_rows_of_4096_points():
    from niwqg_amd import increments
    m = make("coupled", 4096)
    names = ("u", "v", "q_psi")                                                 # three rows of 32 KB and the largest tables in LDS
    P = increments.pdfs(m, names=names, separations=[1, 511, 512, 2048], bins=increments.MAX_BINS)
    check(P, device_values(m, names), "coupled 4096 %d bins" % increments.MAX_BINS)
    names = ("u", "q_psi", "phi")                                               # 2 x 32 KB + 64 KB
    P = increments.pdfs(m, names=names, separations=[1, 512], bins=BINS)
    check(P, device_values(m, names), "coupled 4096 with phi")


def test_rows_of_8192_points():
    from niwqg_amd import increments
    m = make("coupled", 8192)
    names = ("u", "v", "q_psi")                                                 # ONE call: a launch per name fills one table
    P = increments.pdfs(m, names=names, separations=[1, 1023], bins=BINS)
    check(P, device_values(m, names), "coupled 8192 three names")
    P = increments.pdfs(m, names=("phi",), separations=[1, 1023], bins=BINS)    # a row of 128 KB and a table
    check(P, device_values(m, ("phi",)), "coupled 8192 phi")


# ---- 4. other routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 256])
def test_qgmodel_on_the_fused_grids(nx):
    from niwqg_amd import increments
    m = qg_with_scalar(nx)
    advance(m, 2)
    P = increments.pdfs(m, names=("q", "c"), separations=separations(nx), bins=BINS)
    check(P, device_values(m, ("q", "c")), "qg %d" % nx)
    P = increments.pdfs(m, names=("c",), separations=separations(nx), bins=BINS)
    check(P, device_values(m, ("c",)), "qg %d c" % nx)


@pytest.mark.parametrize("kind, nx, names", [("coupled", 96, ("u", "q_psi", "phi")), ("coupled", 192, ("phi", "ow", "v")), ("qg", 96, ("u", "v", "q")),
                                             ("qg", 192, ("q",))])
def test_any_size(kind, nx, names):
    from niwqg_amd import increments
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    advance(m, 2)
    sep = [1, 2, 3, nx // 2 - 1, nx // 2, nx - 1]
    planes = own_planes(m, names)
    P = increments.pdfs(m, names=names, separations=sep, bins=BINS)
    check(P, planes, "%s %d any-size" % (kind, nx))


# ---- 5. two-dimensional separations --------------------------------------------------------------------------------------------------
def vectors(nx):
    T = nx // 8
    return [(0, 1), (0, nx - 1), (1, 1), (-3, 2), (T, T + 1), (nx - 1, nx // 2)]


@pytest.mark.parametrize("project", [None, ("u", "v")])
@pytest.mark.parametrize("nx", [64, 128, 1024])
def test_pdfs2d(nx, project):
    from niwqg_amd import increments
    m = make("coupled", nx)
    advance(m, 2, batched=True)
    names = ("u", "v", "phi")
    P = increments.pdfs2d(m, names=names, vectors=vectors(nx), project=project, bins=BINS)
    assert P.project == project and (P.proj is None) == (project is None)
    planes = device_values(m, names)
    # the rotation's rounding: each of the two products and their sum within 2^-53 of max |d|, doubled for a contracted form
    check(P, planes, "coupled %d 2-D project=%s" % (nx, project), extra=(lambda n, v: 4 * 2.0 ** -53 * np.abs(v).max()) if project else None)
    Y = P.along("y")
    assert np.array_equal(Y.r, [1, nx - 1])
    for n in names:
        assert np.array_equal(Y.counts[n], P.counts[n][:2]) and np.array_equal(Y.edges[n], P.edges[n][:2])


@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("qg", 64), ("coupled", 96)])
def test_x_and_2d_calls_count_alike(kind, nx):
    """two kernels (the row pass and the plane kernel on the fused Kernel family), one definition: identical counts"""
    from niwqg_amd import increments
    m = make(kind, nx, "filter")
    advance(m, 1)
    names = ("q",) if kind == "qg" and nx == 64 else ("u", "q_psi", "phi")
    sep = separations(nx)
    A = increments.pdfs(m, names=names, separations=sep, bins=BINS)
    B = increments.pdfs2d(m, names=names, vectors=[(r, 0) for r in sep], project=None, bins=BINS, ranges=A.ranges)
    for n in names:
        assert np.array_equal(A.counts[n], B.counts[n]) and np.array_equal(A.below[n], B.below[n]) and np.array_equal(A.above[n], B.above[n])
        assert np.array_equal(B.along("x").counts[n], A.counts[n])


# ---- 6. determinism, accumulation, isolation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("coupled", 96)])
def test_determinism_accumulation_and_reset(kind, nx):
    from niwqg_amd import increments
    m, twin = make(kind, nx, "filter"), make(kind, nx, "filter")             # the twin takes the single calls (one table per context)
    names, sep = ("u", "v", "phi"), separations(nx)
    a, b = increments.pdfs(m, names=names, separations=sep, bins=BINS), increments.pdfs(m, names=names, separations=sep, bins=BINS)
    for n in names:
        assert np.array_equal(a.counts[n], b.counts[n]) and np.array_equal(a.ranges[n], b.ranges[n])
    A = increments.Accumulator(m, names, separations=sep, bins=BINS)
    assert A.ranges is None
    with pytest.raises(RuntimeError, match="nothing added"):
        A.result()
    singles = []
    for _ in range(3):
        advance(m, 1)
        advance(twin, 1)
        A.add()
        singles.append(increments.pdfs(twin, names=names, separations=sep, bins=BINS, ranges=A.ranges))
    R = A.result()
    assert R.samples == 3 and R.points == nx * nx
    for n in names:
        assert np.array_equal(R.ranges[n], A.ranges[n]) and np.array_equal(R.ranges[n], singles[0].ranges[n])
        assert np.array_equal(R.counts[n], sum(s.counts[n] for s in singles))
        assert np.array_equal(R.below[n], sum(s.below[n] for s in singles)) and np.array_equal(R.above[n], sum(s.above[n] for s in singles))
        assert np.all(R.counts[n].sum(axis=1) + R.below[n] + R.above[n] == 3 * nx * nx)
    if not getattr(m, "_any_size", False):
        increments.pdfs(m, names=names, separations=sep, bins=BINS)            # takes the context's table over
        with pytest.raises(RuntimeError, match="another call"):
            A.add()
    A.reset()
    assert A.ranges is None
    A.add()
    one = increments.pdfs(twin, names=names, separations=sep, bins=BINS, ranges=A.ranges)
    assert A.result().samples == 1 and all(np.array_equal(A.result().counts[n], one.counts[n]) for n in names)


def test_accumulate_needs_the_configuration_that_zeroed_the_table():
    from niwqg_amd import _lib
    m = make("coupled", 64)
    L, h = m._ctx.L, m._ctx.h
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    n, out = ctypes.c_longlong(0), (ctypes.c_ulonglong * (2 * 11))()
    assert L.nq_increment_hist_read(h, ctypes.byref(n), out) == -4                                          # no table yet
    hist = lambda lo, hi, bins, acc, f=_lib.FLOW_U: L.nq_increment_hist(h, 1, ints(f), 2, ints(1, 5), dbl(*lo), dbl(*hi), bins, acc)
    assert hist((-1, -1), (1, 1), 8, 1) == -1                                                               # accumulate before any call
    assert hist((-1, -1), (1, 1), 8, 0) == 0
    assert hist((-1, -1), (1, 2), 8, 1) == -1 and b"ranges" in L.nq_last_error(h)                           # other ranges
    assert hist((-1, -1), (1, 1), 16, 1) == -1                                                              # other bins
    assert hist((-1, -1), (1, 1), 8, 1, _lib.FLOW_V) == -1                                                  # another field
    assert L.nq_increment_hist2(h, 1, ints(_lib.FLOW_U), 2, ints(1, 0, 5, 0), None, -1, -1, dbl(-1, -1), dbl(1, 1), 8, 1) == -1     # the other kind of call
    assert hist((-1, -1), (1, 1), 8, 1) == 0
    assert L.nq_increment_hist_read(h, ctypes.byref(n), out) == 0 and n.value == 2 and sum(out) == 2 * 2 * 64 * 64
    assert hist((-1, -1), (1, np.inf), 8, 0) == -1 and hist((1, -1), (1, 1), 8, 0) == -1                    # ranges: finite, lo < hi
    assert hist((-1, -1), (1, 1), 0, 0) == -1 and hist((-1, -1), (1, 1), _lib.IPDF_MAX_BINS + 1, 0) == -1
    assert L.nq_increment_hist_read(h, ctypes.byref(n), out) == 0 and n.value == 2                          # refused calls change nothing


def test_structure_accumulators_are_not_disturbed():
    from niwqg_amd import increments, structure
    a, b = make("coupled", 128, "filter"), make("coupled", 128, "filter")
    kw = dict(names=("u", "v", "phi"), separations=separations(128), mixed=(("u", "v", "v"),))
    kw2 = dict(names=("u", "v", "q_psi"), vectors=vectors(128), mixed=(("u", "v", "v"),))
    A, B = structure.Accumulator(a, **kw), structure.Accumulator(b, **kw)
    A2, B2 = structure.Accumulator2d(a, **kw2), structure.Accumulator2d(b, **kw2)
    for acc in (A, B, A2, B2):
        acc.add()
    increments.pdfs(a)                                                          # auto ranges: the range pass runs structure's kernels
    increments.pdfs2d(a, names=("u", "v", "phi"))
    increments.pdfs(a, names=("q_psi", "phi"), separations=[1, 2])
    advance(a, 1)
    advance(b, 1)
    for acc in (A, B, A2, B2):
        acc.add()                                                               # must not raise RuntimeError
    assert A.result().samples == 2 and A.result().sums.tobytes() == B.result().sums.tobytes()
    assert A2.result().samples == 2 and A2.result().sums.tobytes() == B2.result().sums.tobytes()


def test_increment_calls_leave_the_run_alone():
    from niwqg_amd import increments, pdfs, _lib
    a, b = make("coupled", 128, "filter"), make("coupled", 128, "filter")
    ranges = {"q_psi": (-1e-4, 1e-4), "phi2": (0.0, 1.0)}
    H = pdfs.Accumulator(a, ranges, names=("q_psi", "phi2"), bins=32)
    H.add()
    before = H.result()
    bytes0 = None
    for m in (a, b):
        m._ctx.take_budget_increments()
    for k in range(6):
        a._ctx.step(1)
        b._ctx.step(1)
        increments.pdfs(a, names=("u", "q_psi", "phi"), bins=increments.MAX_BINS if k == 0 else BINS)
        increments.pdfs2d(a, bins=increments.MAX_BINS if k == 0 else BINS)    # the largest tables of this test first: no growth afterwards
        if k == 0:
            bytes0 = a._ctx.device_bytes()
    assert a._ctx.device_bytes() == bytes0
    for fid in (_lib.F_QH, _lib.F_PHIH, _lib.F_PH, _lib.F_QWH):
        assert a._ctx.field(fid).tobytes() == b._ctx.field(fid).tobytes(), fid
    assert a._ctx.take_budget_increments() == b._ctx.take_budget_increments()       # the budget series of the six steps
    after = H.result()
    for n in ("q_psi", "phi2"):
        assert np.array_equal(before.counts[n], after.counts[n])


def test_device_bytes_stay_within_the_declared_bound():
    from niwqg_amd import _lib, increments, structure
    m = make("coupled", 128)
    structure.functions(m, names=("u", "v", "phi"))                             # the shared partials and the 2-D planes are structure's
    structure.functions2d(m, names=("u", "v", "phi"))
    before = m._ctx.device_bytes()
    increments.pdfs(m, names=("u", "v", "phi"), bins=increments.MAX_BINS)
    increments.pdfs2d(m, names=("u", "v", "phi"), bins=increments.MAX_BINS)
    grown = m._ctx.device_bytes() - before
    print("nq_device_bytes grew by %d of at most %d" % (grown, _lib.IPDF_DEVICE_BYTES))
    assert 0 < grown <= _lib.IPDF_DEVICE_BYTES


def test_zero_fields():
    """q = 0 and phi = const on a coupled model.  A plane that is exactly constant on the device (phi is: the transforms of a constant
    are exact; u, v and q_psi of the wave-free inversion) has zero increments: the default range is (-1, 1) ([0, 1] for phi) and
    every increment falls in the bin that holds 0.  A plane that is the round-off of its partner's transform (q shares a packed
    transform with q_w: 1e-22 here) is an ordinary field with sigma-scaled ranges: no NaN and the rows close."""
    from niwqg_amd import increments
    nx = 64
    m = make("coupled", nx)
    m.set_q(np.zeros((nx, nx)))
    m.set_phi(np.full((nx, nx), 0.3 + 0.1j))
    exact = set()
    for P in (increments.pdfs(m, names=("q", "u", "phi"), separations=separations(nx), bins=BINS),
              increments.pdfs2d(m, names=("u", "v", "phi"), vectors=vectors(nx), bins=BINS)):
        planes = device_values(m, P.names)
        for n in P.names:
            assert np.all(P.nan[n] == 0) and np.all(P.counts[n].sum(axis=1) + P.below[n] + P.above[n] == nx * nx)
            if np.all(planes[n] == planes[n][0, 0]):
                exact.add(n)
                assert np.all(P.below[n] + P.above[n] == 0)
                assert np.array_equal(P.ranges[n], [[0.0 if n == "phi" else -1.0, 1.0]] * len(P.counts[n])), n
                assert np.all(P.counts[n][:, 0 if n == "phi" else BINS // 2] == nx * nx), n     # the bin that holds 0
        rest = [n for n in P.names if n not in exact]
        print("zero fields: exactly constant on the device: %s; round-off planes: %s" % (sorted(exact), rest))
    assert "phi" in exact


def test_nan_in_the_state_lands_in_nan():
    from niwqg_amd import increments
    nx = 64
    m = make("coupled", nx)
    q = np.array(m.q, np.float64)
    q[5, 7] = np.nan
    m.set_q(q)                                                                  # read only: nothing is stepped
    sep = [1, 9]
    P = increments.pdfs(m, names=("q",), separations=sep, bins=BINS, ranges={"q": (-1e-3, 1e-3)})
    plane = device_values(m, ("q",))["q"]
    assert np.isnan(plane).any()
    for s, r in enumerate(sep):
        want = int(np.isnan(np.roll(plane, -r, axis=1) - plane).sum())
        assert want > 0 and P.nan["q"][s] == want
        assert P.counts["q"][s].sum() + P.below["q"][s] + P.above["q"][s] + want == nx * nx
    A = increments.pdfs(m, names=("q",), separations=sep, bins=BINS)            # auto ranges of a NaN field: (-1, 1)
    assert np.array_equal(A.ranges["q"], [[-1, 1]] * 2) and np.array_equal(A.nan["q"], P.nan["q"])


def test_refusals():
    import niwqg_amd
    from niwqg_amd import increments, _lib
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    k = make("coupled", 64)
    with pytest.raises(ValueError, match="three real names"):
        increments.pdfs(k, names=("u", "v", "q", "q_psi"))
    for bins in (0, increments.MAX_BINS + 1):
        with pytest.raises(ValueError, match="bins"):
            increments.pdfs(k, bins=bins)
    with pytest.raises(ValueError, match="listed twice"):
        increments.pdfs2d(k, vectors=[(1, 2), (1, 2)])
    with pytest.raises(ValueError, match="range"):
        increments.pdfs(k, ranges={"u": (1.0, 1.0)})
    L, h = k._ctx.L, k._ctx.h
    assert L.nq_increment_hist2(h, 1, ints(_lib.FLOW_U), 2, ints(1, 2, 1, 2), None, -1, -1, dbl(-1, -1), dbl(1, 1), 8, 0) == -1
    assert L.nq_increment_hist(h, 4, ints(_lib.FLOW_U, _lib.FLOW_V, _lib.PDF_Q, _lib.PDF_QPSI), 1, ints(1), dbl(-1, -1, -1, -1), dbl(1, 1, 1, 1), 8, 0) == -1
    g = make("qg", 64)
    with pytest.raises(NotImplementedError, match="QGModel"):
        increments.pdfs(g, names=("u",))
    with pytest.raises(ValueError, match="valid names"):
        increments.pdfs(g, names=("q", "phi"))
    out = (ctypes.c_double * 2)()
    assert L.nq_increment_range(g._ctx.h, 1, ints(_lib.FLOW_U), 1, ints(1), out) == -1 and b"QGModel" in L.nq_last_error(g._ctx.h)
    assert L.nq_increment_hist(g._ctx.h, 1, ints(_lib.SF_PHI), 1, ints(1), dbl(0), dbl(1), 8, 0) == -1
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        increments.pdfs(s, names=("u",))
    with pytest.raises(NotImplementedError, match="slab"):
        increments.pdfs2d(s)
    hs = s._ctx.sim.ranks[0].h
    n, tab = ctypes.c_longlong(0), (ctypes.c_ulonglong * 11)()
    assert L.nq_increment_hist(hs, 1, ints(_lib.FLOW_U), 1, ints(1), dbl(-1), dbl(1), 8, 0) == -4 and len(L.nq_last_error(hs)) > 0
    assert L.nq_increment_hist2(hs, 1, ints(_lib.FLOW_U), 1, ints(1, 0), None, -1, -1, dbl(-1), dbl(1), 8, 0) == -4
    assert L.nq_increment_range(hs, 1, ints(_lib.FLOW_U), 1, ints(1), out) == -4
    assert L.nq_increment_range2(hs, 1, ints(_lib.FLOW_U), 1, ints(1, 0), None, -1, -1, out) == -4
    assert L.nq_increment_hist_read(hs, ctypes.byref(n), tab) == -4
