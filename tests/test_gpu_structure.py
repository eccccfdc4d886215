"""Structure functions on the device (niwqg_amd/structure.py, csrc/nq_sf.hpp): every column of the device's
table equals ``structure.reference`` applied to the device's own planes to the bound of the summation alone, and to the
independent restatement ``flow.reference`` to the standing 1e-12 of two routes; the 96 KB and 128 KB LDS rows of the large plans,
the plane kernel of QGModel and the any-size path, determinism and accumulation, a run that is left alone, and the refusals.

Bound of a sum (test 1 of the feature): |device - numpy| <= 2 nx 2^-53 sum |term|.  The values are bit-identical by the row pass's
construction; the longest addition chain on either side is under nx + 40 terms (the device: 8 points of a thread, 10 adds of a
wave, up to 16 waves, then at most nx workgroup slots, in runs) and the p-th power costs p roundings, together under 2 nx for
nx >= 64."""
import ctypes

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs
from test_gpu_flow import make, advance, device_values, KINDS, SIZES

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GROUPS = ((("u", "v", "q_psi"), (("u", "v", "v"), ("u", "q_psi", "q_psi"), ("u", "u", "u"))),
          (("ow", "gradphi2", "phi2"), ()),
          (("u", "q_psi", "phi"), (("u", "phi", "phi"),)))


def thread_stride(nx):
    """T = nx / P of the row plan (csrc/nq_generic.hpp: XPlanT: 8 points per thread)"""
    return nx // 8


def separations(nx):
    T = thread_stride(nx)
    return sorted(set(r for r in (1, 2, 3, T - 1, T, T + 1, nx // 2, nx - 1) if 1 <= r <= nx - 1))


def check(S, planes, sep, mixed, nx, tag, factor=1.0, samples=1):
    """every column of the device's raw sums against the numpy sums of the same planes"""
    from niwqg_amd import structure
    R = structure.reference(planes, sep, mixed) if not isinstance(planes, structure.StructureFunctions) else planes
    assert S.names == R.names and S.triples == R.triples and np.array_equal(S.r, R.r) and S.samples == samples
    err, tol = np.abs(S.sums - R.sums), factor * 2 * nx * U * R.abs_sums
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print("%s: max |device - numpy| / bound = %.3g" % (tag, worst))
    assert np.all(err <= tol), (tag, np.argwhere(err > tol)[:4].tolist(), worst)
    assert np.abs(R.sums[:, 1]).min() > 0
    return R


def own_planes(m, names):
    """{name: plane} of the device's own values: the averages' single sample on the fused grids, the any-size path's planes"""
    if not getattr(m, "_any_size", False):
        return device_values(m, names)
    real = m._pdf_planes([n for n in names if n != "phi"])
    out = {}
    for n in names:
        x = m._d["phi"].get() if n == "phi" else real[n][0].get()
        out[n] = x if n == "phi" else np.ascontiguousarray(x.real)
    return out


# ---- 1. sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sums_equal_numpy_on_the_device_planes(kind, nx):
    from niwqg_amd import structure
    m = make(kind, nx)
    sep = separations(nx)
    for state in ("set", "3 steps"):
        if state != "set":
            advance(m, 3, batched=True)
        for names, mixed in GROUPS:
            S = structure.functions(m, names=names, separations=sep, mixed=mixed)
            check(S, device_values(m, names), sep, mixed, nx, "%s %d %s %s" % (kind, nx, state, "/".join(names)))


# ---- 2. against the independent restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("ybj", 512), ("uncoupled", 1024)])
def test_against_the_restatement(kind, nx):
    from niwqg_amd import flow, structure
    m = make(kind, nx)
    advance(m, 2, batched=True)
    names, sep = ("u", "v", "q_psi"), separations(nx)
    ref = flow.reference(m, ("u", "v"))
    ref["q_psi"] = np.array(m.q_psi, np.float64)
    R = structure.reference({n: ref[n] for n in names}, sep)
    S = structure.functions(m, names=names, separations=sep)
    power = (1, 2, 3, 4, 5, 6, 1, 3, 5)                                      # of column k
    for i, n in enumerate(names):
        top = np.abs(ref[n]).max()
        for k, p in enumerate(power):
            # each increment is within 2e-12 max|a| of the restatement's, so d^p moves by p |d|^(p-1) times that, summed over the plane
            lower = np.full(len(sep), float(nx * nx)) if p == 1 else R.abs_sums[:, 9 * i + p - 2]
            tol = p * 2e-12 * top * lower + 2 * nx * U * R.abs_sums[:, 9 * i + k]
            err = np.abs(S.sums[:, 9 * i + k] - R.sums[:, 9 * i + k])
            print("%s %d %s column %d: %.3g of the bound" % (kind, nx, n, k, (err / tol).max()))
            assert np.all(err <= tol), (n, k, err, tol)


# ---- 3. large plans --------------------------------------------------------------------------------------------------------------
def test_rows_of_4096_points():
    from niwqg_amd import structure
    m = make("coupled", 4096)
    names, mixed, sep = ("u", "v", "q_psi"), (("u", "v", "v"),), [1, 511, 512, 2048]
    S = structure.functions(m, names=names, separations=sep, mixed=mixed)       # three rows of 32 KB in LDS
    check(S, device_values(m, names), sep, mixed, 4096, "coupled 4096")


def test_rows_of_8192_points():
    from niwqg_amd import structure
    m = make("coupled", 8192)
    sep = [1, 1023, 4096]
    for names in (("u",), ("phi",)):                                            # one value per thread; phi: a row of 128 KB in LDS
        S = structure.functions(m, names=names, separations=sep)
        check(S, device_values(m, names), sep, (), 8192, "coupled 8192 %s" % names[0])
    with pytest.raises(NotImplementedError, match="8192"):
        structure.functions(m, names=("u", "v"), separations=sep, mixed=(("u", "v", "v"),))
    L, h = m._ctx.L, m._ctx.h
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    from niwqg_amd import _lib
    assert L.nq_structure(h, 2, ints(_lib.FLOW_U, _lib.FLOW_V), 1, ints(1), 1, ints(0, 1, 1), 0) == -1 and b"8192" in L.nq_last_error(h)
    assert L.nq_structure(h, 2, ints(_lib.FLOW_U, _lib.SF_PHI), 1, ints(1), 0, None, 0) == -1 and b"8192" in L.nq_last_error(h)


# ---- 4. other routes ---------------------------------------------------------------------------------------------------------------
def qg_with_scalar(nx):
    import niwqg_amd
    kw = notebook_kwargs(nx, False)
    for k in ("m", "N", "f", "nu4w", "nuw", "muw"):
        kw.pop(k)
    kw.update(mu=2e-8, nu=0.0, use_filter=False, passive_scalar=True, nu4c=3e9, nuc=2.0, muc=1e-8)
    m = niwqg_amd.QGModel.Model(**kw)
    rng = np.random.default_rng(nx)
    q, c = rng.standard_normal((2, nx, nx))
    m.set_q(1e-5 * (q - q.mean()))
    m.set_c(c - c.mean())
    return m


@pytest.mark.parametrize("nx", [64, 256])
def test_qgmodel_on_the_fused_grids(nx):
    from niwqg_amd import structure
    m = qg_with_scalar(nx)
    advance(m, 2)
    names, mixed, sep = ("q", "c"), (("q", "c", "c"), ("c", "c", "c")), separations(nx)
    assert structure.available(m) == ["q", "c"]
    S = structure.functions(m, names=names, separations=sep, mixed=mixed)
    check(S, device_values(m, names), sep, mixed, nx, "qg %d" % nx)
    S = structure.functions(m, names=("c",), separations=sep)                   # the scalar alone: plane b in slot 0
    check(S, device_values(m, ("c",)), sep, (), nx, "qg %d c" % nx)


@pytest.mark.parametrize("kind, nx, names, mixed", [("coupled", 96, ("u", "q_psi", "phi"), (("u", "phi", "phi"), ("u", "q_psi", "q_psi"))),
                                                     ("coupled", 96, ("phi", "ow", "v"), (("v", "phi", "phi"),)),
                                                     ("qg", 48, ("u", "v", "q"), (("u", "v", "v"),))])
def test_any_size(kind, nx, names, mixed):
    from niwqg_amd import structure
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    advance(m, 2)
    sep = [1, 2, 3, nx // 2 - 1, nx // 2, nx - 1]
    planes = own_planes(m, names)
    S = structure.functions(m, names=names, separations=sep, mixed=mixed)
    check(S, planes, sep, mixed, nx, "%s %d any-size" % (kind, nx))


# ---- 5. determinism and accumulation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("coupled", 96), ("qg", 64)])
def test_determinism_and_reset(kind, nx):
    from niwqg_amd import structure
    m = make(kind, nx, "filter")
    fused = not getattr(m, "_any_size", False)
    advance(m, 1)
    kw = dict(names=("q",), mixed=(("q", "q", "q"),)) if kind == "qg" else dict(names=("u", "q_psi", "phi"), mixed=(("u", "phi", "phi"), ("u", "q_psi", "q_psi")))
    kw["separations"] = separations(nx)
    a, b = structure.functions(m, **kw), structure.functions(m, **kw)
    assert a.sums.tobytes() == b.sums.tobytes() and np.all(a.moment(kw["names"][0], 2) > 0)
    A = structure.Accumulator(m, **kw)
    assert np.all(A.result().sums == 0) and A.result().samples == 0
    A.add()
    A.add()
    R = A.result()
    assert R.samples == 2 and R.sums.tobytes() == (2 * a.sums).tobytes()      # x + x is exact
    assert R.table.tobytes() == (2 * a.sums / (2.0 * nx * nx)).tobytes()
    if fused:
        structure.functions(m, **kw)                                          # takes the context's table over
        with pytest.raises(RuntimeError, match="another call"):
            A.add()
        with pytest.raises(RuntimeError, match="another call"):
            A.result()
    A.reset()
    assert np.all(A.result().sums == 0)
    A.add()
    assert A.result().samples == 1 and A.result().sums.tobytes() == a.sums.tobytes()


@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("coupled", 96)])
def test_accumulator_is_the_sum_of_single_calls(kind, nx):
    from niwqg_amd import structure
    m, twin = make(kind, nx, "filter"), make(kind, nx, "filter")             # the twin takes the single calls (one table per context)
    kw = dict(names=("u", "v", "phi"), separations=separations(nx), mixed=(("u", "v", "v"), ("u", "phi", "phi")))
    A = structure.Accumulator(m, **kw)
    singles, bound = [], 0.0
    for _ in range(3):
        advance(m, 1)
        advance(twin, 1)
        A.add()
        singles.append(structure.functions(twin, **kw))
        ref = check(singles[-1], own_planes(twin, kw["names"]), kw["separations"], kw["mixed"], nx, "%s %d single" % (kind, nx))
        bound = bound + 2 * nx * U * ref.abs_sums
    R = A.result()
    assert R.samples == 3 and R.points == nx * nx
    total = sum(s.sums for s in singles)
    assert np.all(np.abs(R.sums - total) <= 3 * bound)
    assert np.allclose(R.moment("u", 2), total[:, 1] / (3.0 * nx * nx), rtol=1e-12)


# ---- 6. leaves the run alone -------------------------------------------------------------------------------------------------------
def test_structure_calls_leave_the_run_alone():
    from niwqg_amd import averages, pdfs, structure
    a, b = make("coupled", 128, "filter"), make("coupled", 128, "filter")
    ranges = {"q_psi": (-1e-4, 1e-4), "phi2": (0.0, 1.0)}
    P = pdfs.Accumulator(a, ranges, names=("q_psi", "phi2"), bins=32)
    P.add()
    A = averages.attach(a, ("u", "phi"), every=0)
    A.sample()
    before_pdf, before_avg = P.result(), {n: A.result().sums[n].copy() for n in ("u", "phi")}
    for _ in range(4):
        advance(a, 1)
        advance(b, 1)
        structure.functions(a, names=("u", "q_psi", "phi"), mixed=(("u", "phi", "phi"),))
        structure.functions(a, names=("ow", "gradphi2", "phi2"), separations=[1, 5])
    for n in ("qh", "phih", "ph"):
        assert np.array(getattr(a, n)).tobytes() == np.array(getattr(b, n)).tobytes(), n
    after_pdf, after_avg = P.result(), A.result()
    for n in ("q_psi", "phi2"):
        assert np.array_equal(before_pdf.counts[n], after_pdf.counts[n])
    assert after_avg.n == 1 and all(before_avg[n].tobytes() == after_avg.sums[n].tobytes() for n in before_avg)
    A.detach()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import niwqg_amd
    from niwqg_amd import structure, _lib
    L = _lib.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    k = make("coupled", 64)
    h = k._ctx.h
    with pytest.raises(ValueError, match="three real names"):
        structure.functions(k, names=("u", "v", "q", "q_psi"))
    with pytest.raises(ValueError, match="three real names"):
        structure.functions(k, names=("u", "v", "q", "phi"))
    for bad in ([0, 1], [1, 64]):
        with pytest.raises(ValueError, match="separations"):
            structure.functions(k, separations=bad)
    with pytest.raises(NotImplementedError, match="along x"):
        structure.functions(k, direction="y")
    out, n = np.zeros(64 * 31), ctypes.c_longlong(0)
    assert L.nq_structure_read(h, ctypes.byref(n), _lib._dptr(out)) == -4                                   # no table yet
    assert L.nq_structure(h, 4, ints(_lib.FLOW_U, _lib.FLOW_V, _lib.PDF_Q, _lib.PDF_QPSI), 1, ints(1), 0, None, 0) == -1
    assert L.nq_structure(h, 3, ints(_lib.FLOW_U, _lib.SF_PHI, _lib.SF_PHI), 1, ints(1), 0, None, 0) == -1
    for seps in ((0,), (64,), (2, 2), (3, 1)):
        assert L.nq_structure(h, 1, ints(_lib.FLOW_U), len(seps), ints(*seps), 0, None, 0) == -1 and b"separation" in L.nq_last_error(h)
    assert L.nq_structure(h, 1, ints(_lib.FLOW_U), 65, ints(*range(1, 66)), 0, None, 0) == -1
    assert L.nq_structure(h, 2, ints(_lib.FLOW_U, _lib.SF_PHI), 1, ints(1), 1, ints(1, 0, 0), 0) == -1     # phi first in a triple
    assert L.nq_structure(h, 2, ints(_lib.FLOW_U, _lib.SF_PHI), 1, ints(1), 1, ints(0, 0, 1), 0) == -1     # phi once
    assert L.nq_structure(h, 1, ints(_lib.FLOW_U), 1, ints(1), 1, ints(0, 0, 1), 0) == -1                  # an index past the list
    assert L.nq_structure(h, 1, ints(_lib.FLOW_U), 1, ints(1), 0, None, 1) == -1                           # accumulate before any call
    assert L.nq_structure(h, 1, ints(_lib.FLOW_U), 1, ints(1), 0, None, 0) == 0
    assert L.nq_structure(h, 1, ints(_lib.FLOW_V), 1, ints(1), 0, None, 1) == -1                           # another configuration
    assert L.nq_structure(h, 1, ints(_lib.FLOW_U), 1, ints(1), 0, None, 1) == 0
    assert L.nq_structure_read(h, ctypes.byref(n), _lib._dptr(out)) == 0 and n.value == 2 and out[1] > 0
    g = make("qg", 64)
    with pytest.raises(NotImplementedError, match="QGModel"):
        structure.functions(g, names=("u",))
    with pytest.raises(ValueError, match="valid names"):
        structure.functions(g, names=("q", "phi"))
    with pytest.raises(ValueError, match="valid names"):
        structure.functions(g, names=("q", "c"))                                                            # no passive scalar here
    assert L.nq_structure(g._ctx.h, 1, ints(_lib.FLOW_U), 1, ints(1), 0, None, 0) == -1 and b"QGModel" in L.nq_last_error(g._ctx.h)
    assert L.nq_structure(g._ctx.h, 1, ints(_lib.SF_PHI), 1, ints(1), 0, None, 0) == -1
    assert L.nq_structure(g._ctx.h, 1, ints(_lib.PDF_C), 1, ints(1), 0, None, 0) == -1
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        structure.functions(s, names=("u",))
    hs = s._ctx.sim.ranks[0].h
    assert L.nq_structure(hs, 1, ints(_lib.FLOW_U), 1, ints(1), 0, None, 0) == -4 and len(L.nq_last_error(hs)) > 0
    assert L.nq_structure_read(hs, ctypes.byref(n), _lib._dptr(out)) == -4
