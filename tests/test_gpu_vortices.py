"""Vortex census on the device (niwqg_amd/vortices.py, csrc/nq_vortex.hpp): the label plane and the whole
int64 table equal the numpy specification ``vortices.reference`` bit for bit -- on crafted sets (rings round the torus, seams,
long equivalence chains, wave and thread-stride boundaries, random masks) for the fused Kernel family, QGModel and the any-size
path, and on physical states of every model kind against the device's own planes; the capacity cuts the table, not the labels;
two calls return the same bytes; a census disturbs neither the accumulators that share its planes nor the run; a NaN is counted,
kept out of the set and raised; the refusals carry the documented codes.

No census kernel sizes its grid by the CU count (one workgroup per row, a fixed 1024 for the range pass), so there is no case
under NIWQG_AMD_NUM_CU.  The crafted sets are those of tests/test_vortices_host.py."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_flow import make, advance, device_values, KINDS
from test_vortices_host import cases

pytestmark = pytest.mark.gpu


def same(C, R, tag):
    """the census C equals the reference R in every integer it returns"""
    assert np.array_equal(C.info(), R.info()), (tag, C.info(), R.info())
    assert C.scales == R.scales, (tag, C.scales, R.scales)
    assert C.table.shape == R.table.shape and C.table.tobytes() == R.table.tobytes(), (tag, np.argwhere(C.table != R.table)[:8])
    if C.labels is not None:
        assert C.labels.dtype == np.int32 and np.array_equal(C.labels, R.labels), (tag, np.argwhere(C.labels != R.labels)[:8])


def point_labels(C):
    """the plane of component labels (smallest linear index, -1 outside the set) of a census with labels"""
    return np.where(C.labels >= 0, np.append(C.label, -1)[C.labels], -1)


@functools.lru_cache(maxsize=None)
def exact_labels(n, name, connectivity):
    from niwqg_amd import vortices
    return vortices.label_plane(cases(n, n)[name], connectivity)


# ---- 1. crafted sets, compared exactly -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("coupled", 128), ("qg", 64), ("coupled", 12), ("coupled", 96)])
def test_crafted_sets(kind, nx):
    from niwqg_amd import vortices
    m = make(kind, nx)
    assert bool(getattr(m, "_any_size", False)) == (nx in (12, 96))
    if kind != "qg":
        m.set_phi(np.zeros((nx, nx), complex))
    for name, mask in cases(nx, nx).items():
        m.set_q(mask.astype(np.float64))
        q = device_values(m, ["q"])["q"]
        assert np.array_equal(q > 0.5, mask) and np.abs(q - mask).max() < 1e-12, name      # the round trip moves the values, not the set
        for conn in (4, 8):
            tag = "%s %d %s %d" % (kind, nx, name, conn)
            C = vortices.census(m, "q", 0.5, units="abs", mode="above", sums=("q",), connectivity=conn, labels=True)
            same(C, vortices.reference({"q": q}, "q", "above", 0.5, conn, 65536), tag)
            want = exact_labels(nx, name, conn)
            assert not C.truncated and np.array_equal(point_labels(C), want), tag
            assert C.points_in_set == int(mask.sum()) and int(C.area.sum()) == C.points_in_set, tag
    full = vortices.census(m, "q", -1.0, units="abs", mode="above", sums=("q",))               # the last q, every point
    assert full.n == 1 and full.label[0] == 0 and full.area[0] == nx * nx


# ---- 2. physical states -----------------------------------------------------------------------------------------------------------------
def crosses_a_seam(labels):
    a = (labels[:, 0] >= 0) & (labels[:, 0] == labels[:, -1])
    b = (labels[0, :] >= 0) & (labels[0, :] == labels[-1, :])
    return bool(a.any() or b.any())


def check_state(m, names, tag, capacity=65536, **kw):
    """the census of the current state, both connectivities, against the reference on the device's own planes"""
    from niwqg_amd import vortices
    planes = device_values(m, names)
    seam = False
    for conn in (4, 8):
        C = vortices.census(m, names[0], sums=names[1:], connectivity=conn, labels=True, capacity=capacity, **kw)
        R = vortices.reference({n: planes[n] for n in C.names}, C.criterion, C.mode, C.threshold, conn, capacity)
        same(C, R, "%s %d" % (tag, conn))
        assert C.total > 1, tag
        seam = seam or crosses_a_seam(C.labels)
        print("%s, %d-connectivity: %d components, %.3f of the plane, threshold %.4g" % (tag, conn, C.total, C.points_in_set / C.labels.size, C.threshold))
    return seam


@pytest.mark.parametrize("nx", [64, 128, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_physical_states(kind, nx):
    from niwqg_amd import vortices
    m = make(kind, nx)
    names = ["ow", "q_psi", "phi2"]
    D = vortices.census(m)                                                    # the defaults are this very call
    assert D.names == names and D.criterion == "ow" and D.mode == "below" and D.connectivity == 4 and D.threshold < 0
    seam = check_state(m, names, "%s %d at set" % (kind, nx))
    advance(m, 3, batched=True)
    seam = check_state(m, names, "%s %d after 3 steps" % (kind, nx)) or seam
    assert seam or nx < 128, "no component crosses a seam: the case proves little"


def test_physical_state_1024():
    """more components than the default capacity: a capacity that holds them all, so that every row of the table is compared"""
    from niwqg_amd import vortices
    m = make("coupled", 1024)
    names = ["ow", "q_psi", "phi2"]
    assert check_state(m, names, "coupled 1024 at set", capacity=1 << 19)
    advance(m, 3, batched=True)
    assert check_state(m, names, "coupled 1024 after 3 steps", capacity=1 << 19)
    C = vortices.census(m)
    assert 65536 < C.total < (1 << 19) and C.n == 65536 and C.truncated               # and the default capacity cuts this state


def test_any_size_and_qg_states():
    from niwqg_amd import vortices
    m = make("coupled", 96, "filter")
    assert m._any_size
    advance(m, 2)
    assert check_state(m, ["ow", "q_psi", "phi2"], "coupled 96 (any size)")
    from test_gpu_structure import qg_with_scalar
    g = qg_with_scalar(64)
    D = vortices.census(g)
    assert D.names == ["q"] and D.mode == "abs_above" and D.threshold > 0
    check_state(g, ["q", "c"], "qg 64 (q, c)", threshold=1.0, mode="abs_above")
    advance(g, 3, batched=True)
    check_state(g, ["c", "q"], "qg 64 (c, q) after 3 steps", threshold=0.5, mode="above")


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_the_table_not_the_labels():
    from niwqg_amd import vortices
    m = make("coupled", 64)
    m.set_phi(np.zeros((64, 64), complex))
    board = cases(64, 64)["checkerboard"]
    m.set_q(board.astype(np.float64))
    call = dict(criterion="q", threshold=0.5, units="abs", mode="above", sums=("q",), connectivity=4, labels=True)
    whole = vortices.census(m, **call)
    cut = vortices.census(m, capacity=1024, **call)
    assert whole.total == whole.n == 2048 and not whole.truncated
    assert cut.total == 2048 and cut.n == 1024 and cut.truncated and cut.points_in_set == 2048
    assert cut.table.tobytes() == whole.table[:1024].tobytes()
    assert np.array_equal(cut.labels, np.where(whole.labels >= 1024, -2, whole.labels)) and (cut.labels == -2).sum() == 1024
    same(cut, vortices.reference({"q": device_values(m, ["q"])["q"]}, "q", "above", 0.5, 4, 1024), "capacity 1024")


# ---- 4. determinism and isolation ----------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes():
    from niwqg_amd import vortices
    m = make("coupled", 128)
    advance(m, 2, batched=True)
    a = vortices.census(m, connectivity=8, labels=True)
    b = vortices.census(m, connectivity=8, labels=True)
    assert a.table.tobytes() == b.table.tobytes() and a.labels.tobytes() == b.labels.tobytes() and np.array_equal(a.info(), b.info())
    assert a.threshold == b.threshold and a.plane_sums == b.plane_sums
    held = a.share("phi2", a.cyclonic < 0)
    print("share of |phi|^2 inside anticyclones: %.4f (%d of %d components)" % (held, int((a.cyclonic < 0).sum()), a.n))
    assert 0.0 <= held <= 1.0


def test_a_census_disturbs_neither_the_accumulators_nor_the_run():
    from niwqg_amd import _lib, increments, structure, vortices
    a, b = make("coupled", 128, "filter"), make("coupled", 128, "filter")
    S = [structure.Accumulator2d(m, names=("u", "v", "q_psi")) for m in (a, b)]
    P = [increments.Accumulator(m, ("u", "q_psi"), separations=[1, 2, 8]) for m in (a, b)]
    for k in range(2):
        for i, m in enumerate((a, b)):
            S[i].add()
            P[i].add()
            if i == 0:
                vortices.census(m, labels=True)
                vortices.census(m, "q", 1.0, mode="abs_above", sums=("u", "v"), connectivity=8)
            m._ctx.step(2)
            m._after_steps()
    ra, rb = S[0].result(), S[1].result()
    assert ra.samples == rb.samples == 2 and ra.sums.tobytes() == rb.sums.tobytes()
    pa, pb = P[0].result(), P[1].result()
    for n in ("u", "q_psi"):
        assert np.array_equal(pa.counts[n], pb.counts[n]) and np.array_equal(pa.ranges[n], pb.ranges[n])
    for fid in (_lib.F_QH, _lib.F_PHIH, _lib.F_PH, _lib.F_QWH):
        assert a._ctx.field(fid).tobytes() == b._ctx.field(fid).tobytes(), fid


def test_device_bytes_are_the_feature_s_own_buffers():
    from niwqg_amd import vortices
    n = 128
    m = make("coupled", n)
    call = dict(criterion="q", threshold=1.0, mode="abs_above", sums=("q_psi",))
    before = m._ctx.device_bytes()
    vortices.census(m, capacity=1000, **call)
    first = m._ctx.device_bytes()
    pool = 2 * n * n * 8                                                     # two real planes of the shared pool, allocated here
    small = 2 * (1024 * 3 * 6 * 8 + 120 + 7 * 8 + 3 * 4 * n)                 # range partials, range results, info, three ints per row: the census's and the range call's
    table = lambda cap: cap * 12 * 8
    assert first - before == pool + 2 * 4 * n * n + small + table(1000), (first - before, small)
    vortices.census(m, capacity=1000, **call)
    vortices.census(m, capacity=10, **call)
    assert m._ctx.device_bytes() == first
    vortices.census(m, capacity=5000, **call)
    assert m._ctx.device_bytes() == first + table(5000) - table(1000)
    m._ctx.close()
    assert m._ctx.h is None


def test_close_gives_the_buffers_back():
    """nq_device_bytes cannot be asked of a closed context, so the device's free memory is: closing a context that ran a census
    frees at least every byte the context counted, the label and rank planes and the table among them (1024^2: 8 MB of planes and
    50 MB of table, far above the allocation granularity)."""
    import torch
    from niwqg_amd import vortices
    m = make("coupled", 1024)
    quiet = make("coupled", 1024)                                            # a twin that never runs a census: what a context counts without one
    vortices.census(m, capacity=1 << 19)
    counted, own = m._ctx.device_bytes(), m._ctx.device_bytes() - quiet._ctx.device_bytes()
    assert own >= 2 * 4 * 1024 * 1024 + (1 << 19) * 12 * 8
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    m._ctx.close()
    freed = torch.cuda.mem_get_info()[0] - before
    print("close() freed %d bytes, the context counted %d, %d of them the census's" % (freed, counted, own))
    assert freed >= counted


# ---- 5. non-finite values -------------------------------------------------------------------------------------------------------------------
def test_a_nan_is_counted_kept_out_and_raised():
    from niwqg_amd import _lib, vortices
    n = 64
    m = make("coupled", n)
    good = device_values(m, ["q"])["q"]
    bad = good.copy()
    bad[7, 9] = np.nan
    m.set_q(bad)                                                             # the transform spreads it over the plane
    with pytest.raises(FloatingPointError, match="non-finite"):
        vortices.census(m, "q", 0.5, units="abs", mode="abs_above", sums=("q",))
    c = m._ctx
    info = np.zeros(7, np.int64)
    ll = ctypes.POINTER(ctypes.c_longlong)
    assert c.L.nq_vortex_read(c.h, info.ctypes.data_as(ll), None) == 0
    assert info[3] == n * n and info[0] == info[1] == info[2] == 0 and info[4] == 0
    lab = np.zeros((n, n), np.int32)
    assert c.L.nq_vortex_labels(c.h, _lib._iptr(lab)) == 0 and (lab == -1).all()
    m.set_q(good)
    q = device_values(m, ["q"])["q"]
    C = vortices.census(m, "q", 0.5, units="sigma", mode="abs_above", sums=("q",), labels=True)
    same(C, vortices.reference({"q": q}, "q", "abs_above", C.threshold, 4, 65536), "after the NaN")
    assert C.total > 1 and C.nonfinite == 0


# ---- 6. return codes ------------------------------------------------------------------------------------------------------------------------
def test_return_codes():
    import niwqg_amd
    from niwqg_amd import _lib
    from test_oracle_golden import notebook_kwargs
    L = _lib.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    ll = ctypes.POINTER(ctypes.c_longlong)
    info, four = np.zeros(7, np.int64), np.zeros(12)
    k = make("coupled", 64)
    h = k._ctx.h
    Q, OW, PHI2 = _lib.PDF_Q, _lib.FLOW_OW, _lib.PDF_PHI2
    assert L.nq_vortex_read(h, info.ctypes.data_as(ll), None) == -4 and b"census" in L.nq_last_error(h)     # a read before a census
    assert L.nq_vortex_labels(h, _lib._iptr(np.zeros((64, 64), np.int32))) == -4 and L.nq_vortex_stats(h, _lib._dptr(four)) == -4
    ok = lambda *a: L.nq_vortex_census(h, *a)
    assert ok(1, ints(OW), 0, _lib.VX_BELOW, 0.0, 4, 100) == 0                                             # OW < 0: a good census
    assert ok(0, ints(OW), 0, _lib.VX_BELOW, -1.0, 4, 100) == -1
    assert ok(4, ints(OW, Q, PHI2, _lib.FLOW_U), 0, _lib.VX_BELOW, -1.0, 4, 100) == -1
    assert ok(2, ints(OW, OW), 0, _lib.VX_BELOW, -1.0, 4, 100) == -1 and b"twice" in L.nq_last_error(h)
    assert ok(2, ints(OW, _lib.SF_PHI), 0, _lib.VX_BELOW, -1.0, 4, 100) == -1 and b"complex" in L.nq_last_error(h)
    assert ok(1, ints(_lib.PDF_C), 0, _lib.VX_BELOW, -1.0, 4, 100) == -1                                    # a field the model lacks
    assert ok(1, ints(OW), 1, _lib.VX_BELOW, -1.0, 4, 100) == -1                                            # crit outside the list
    assert ok(1, ints(OW), 0, 3, -1.0, 4, 100) == -1
    assert ok(1, ints(OW), 0, _lib.VX_BELOW, float("nan"), 4, 100) == -1 and ok(1, ints(OW), 0, _lib.VX_BELOW, float("inf"), 4, 100) == -1
    assert ok(1, ints(OW), 0, _lib.VX_BELOW, -1.0, 6, 100) == -1
    assert ok(1, ints(OW), 0, _lib.VX_BELOW, -1.0, 4, 0) == -1 and ok(1, ints(OW), 0, _lib.VX_BELOW, -1.0, 4, _lib.VX_MAX_CAPACITY + 1) == -1
    assert L.nq_vortex_range(h, 1, ints(_lib.SF_PHI), _lib._dptr(four)) == -1
    assert L.nq_vortex_read(h, info.ctypes.data_as(ll), None) == 0 and info[0] >= info[1] >= 1             # the good census is still there
    kept = info.copy()
    assert L.nq_vortex_range(h, 2, ints(Q, PHI2), _lib._dptr(four)) == 0 and four[0] < four[1]                 # a range call keeps results of its own
    assert L.nq_vortex_read(h, info.ctypes.data_as(ll), None) == 0 and np.array_equal(info, kept)
    assert L.nq_vortex_stats(h, _lib._dptr(four)) == 0 and four[0] < 0 < four[1]                               # OW of the census, not q of the range call
    g = make("qg", 64)
    assert L.nq_vortex_census(g._ctx.h, 1, ints(OW), 0, _lib.VX_BELOW, -1.0, 4, 100) == -1 and b"QGModel" in L.nq_last_error(g._ctx.h)
    assert L.nq_vortex_census(g._ctx.h, 1, ints(_lib.PDF_C), 0, _lib.VX_ABOVE, 0.0, 4, 100) == -1           # no passive scalar here
    assert L.nq_vortex_census(g._ctx.h, 1, ints(Q), 0, _lib.VX_ABS_ABOVE, 0.0, 8, 100) == 0
    fresh = niwqg_amd.CoupledModel.Model(**notebook_kwargs(64, False))
    assert L.nq_vortex_census(fresh._ctx.h, 1, ints(OW), 0, _lib.VX_BELOW, -1.0, 4, 100) == -4              # nothing set yet
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    hs = s._ctx.sim.ranks[0].h
    assert L.nq_vortex_census(hs, 1, ints(OW), 0, _lib.VX_BELOW, -1.0, 4, 100) == -4 and len(L.nq_last_error(hs)) > 0
    assert L.nq_vortex_range(hs, 1, ints(OW), _lib._dptr(four)) == -4
    from niwqg_amd import vortices
    with pytest.raises(NotImplementedError, match="slab"):
        vortices.census(s)
    e = make("coupled", 96)._eng
    planes = (ctypes.c_void_p * 1)(None)
    tab = np.zeros((4, 10), np.int64)
    assert L.nq_any_components(e.h, 1, planes, 96, 96, 0, 0, 0.0, 4, 4, info.ctypes.data_as(ll), tab.ctypes.data_as(ll), None) == -1
    assert L.nq_any_components(e.h, 1, planes, 95, 96, 0, 0, 0.0, 4, 4, info.ctypes.data_as(ll), tab.ctypes.data_as(ll), None) == -1
