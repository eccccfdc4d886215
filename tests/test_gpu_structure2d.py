"""Structure functions at two-dimensional separations on the device (niwqg_amd/structure.py: functions2d, csrc/nq_sf2.hpp; DESIGN.md
section 5w): every column of the device's table equals ``structure.reference2d`` applied to the device's own planes, with the
(c_x, c_y) the device was handed, to the bound of the summation; the row route and the global route of the plane kernel, QGModel
and the any-size path, the closed form of a plane wave, the x-pass, determinism and accumulation, a run that is left alone, and
the return codes.

Bound of a sum: |device - numpy| <= max(2 nx, nx + 64) 2^-53 sum |term|.  The values are bit-identical (the store pass writes what
the averages' pass adds to zero); the longest addition chain on either side is under nx + 40 terms (the device: up to 8 points of
a thread, 10 adds of a wave, up to 16 waves, the rows of a workgroup, then at most nx workgroup slots, in runs), the p-th power
costs p <= 6 roundings and the rotation three roundings per factor, each weighted by p; a contraction of the rotation into a fused
multiply-add is one rounding fewer.  ``abs_sums`` majorises the rotated terms by (|c_x d_a| + |c_y d_b|)^p."""
import ctypes

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs
from test_gpu_flow import make, advance, device_values, KINDS, SIZES
from test_gpu_structure import GROUPS, own_planes, qg_with_scalar, separations

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def vectors(nx):
    """the edges of the ranges, both signs of r_x, the row plan's thread stride, three vectors that share r_y = 1 (one row in LDS
    serves them), deliberately not sorted by r_y"""
    T = nx // 8
    return [(1, 0), (0, 1), (nx - 1, nx - 1), (-1, 1), (T, 0), (0, T + 1), (-(T - 1), nx // 2), (nx // 2, nx // 2), (3, nx - 1), (5, 1), (T, 1)]


def check(S, planes, nx, tag, samples=1):
    """every column of the device's raw sums against the numpy sums of the same planes, rotated with the same (c_x, c_y)"""
    from niwqg_amd import structure
    R = structure.reference2d({n: planes[n] for n in S.names}, S.vectors, S.triples, project=S.project, proj=S.proj)
    assert S.names == R.names and S.triples == R.triples and S.samples == samples and S.sums.shape == R.sums.shape
    err, tol = np.abs(S.sums - R.sums), max(2 * nx, nx + 64) * U * R.abs_sums
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print("%s: max |device - numpy| / bound = %.3g" % (tag, worst))
    assert np.all(err <= tol), (tag, np.argwhere(err > tol)[:4].tolist(), worst)
    assert np.abs(R.sums[:, 1]).min() > 0
    return R


# ---- 1. sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sums_equal_numpy_on_the_device_planes(kind, nx):
    from niwqg_amd import structure
    m = make(kind, nx)
    vec = vectors(nx)
    for state in ("set", "3 steps"):
        if state != "set":
            advance(m, 3, batched=True)
        names_all = sorted(set(n for names, _ in GROUPS for n in names))
        planes = device_values(m, names_all)
        for names, mixed in GROUPS:
            S = structure.functions2d(m, names=names, vectors=vec, mixed=mixed)
            assert (S.project == ("u", "v")) == ("v" in names)
            check(S, planes, nx, "%s %d %s %s" % (kind, nx, state, "/".join(names)))
        S = structure.functions2d(m, names=GROUPS[0][0], vectors=vec, mixed=GROUPS[0][1], project=None)
        assert S.project is None and S.proj is None
        check(S, planes, nx, "%s %d %s unrotated" % (kind, nx, state))
    S = structure.functions2d(m, names=("u", "q_psi", "v"), vectors=vec, project=("q_psi", "u"), proj=np.tile([0.6, -0.8], (len(vec), 1)))
    check(S, planes, nx, "%s %d another pair, given numbers" % (kind, nx))


# ---- 2. large rows ---------------------------------------------------------------------------------------------------------------
def workgroups(nx, nvec, names=3):
    """csrc/nq_lib.hip: sf2_grid: one workgroup per row while workgroups x vectors x columns x 8 B fit NQ_SF_PART_MAX_BYTES"""
    from niwqg_amd import _lib
    return min(nx, _lib.SF_PART_MAX_BYTES // (nvec * {1: 10, 2: 22, 3: 31}[names] * 8))


def majorant(S0, proj):
    """From the UNROTATED table S0 of (u, v, third name) with the triple (u, v, v): what majorises ``abs_sums`` of the same call
    rotated with proj (None: unrotated), column by column, without a numpy pass over the planes.  A_p = sum |d|^p of a name are
    its columns 6, 1, 7, 3, 8, 5.  Rotated, |d_L| <= |c_x d_u| + |c_y d_v|, so by Minkowski (sum |d_L|^p)^(1/p) <= |c_x| A_p(u)^(1/p)
    + |c_y| A_p(v)^(1/p), and likewise T; a triple is bounded by Hoelder, sum |a b c| <= (A_3(a) A_3(b) A_3(c))^(1/3)."""
    A = [S0.sums[:, 9 * i:9 * i + 9][:, [6, 1, 7, 3, 8, 5]] for i in range(3)]
    if proj is not None:
        p = np.arange(1, 7)[None, :]
        cx, cy = np.abs(proj[:, :1]), np.abs(proj[:, 1:])
        ru, rv = A[0] ** (1.0 / p), A[1] ** (1.0 / p)
        A[0], A[1] = (cx * ru + cy * rv) ** p * (1 + 1e-12), (cy * ru + cx * rv) ** p * (1 + 1e-12)
    out = np.zeros_like(S0.sums)
    for i in range(3):
        out[:, 9 * i:9 * i + 9] = A[i][:, [0, 1, 2, 3, 4, 5, 0, 2, 4]]
    out[:, 27] = np.cbrt(A[0][:, 2] * A[1][:, 2] * A[1][:, 2]) * (1 + 1e-12)
    return out


def check_rows_shared_by_a_workgroup(m, nx, vec, chunk, tag):
    """A list so long that a workgroup of the plane kernel owns SEVERAL rows (it adds each row to its partial slot, in row order)
    against the same vectors in chunks short enough for one workgroup per row, the path the other tests hold against numpy: both
    are within the bound of their own summation of the exact sums, so they differ by at most the two bounds together."""
    from niwqg_amd import structure
    names, mixed = ("u", "v", "q_psi"), (("u", "v", "v"),)
    vec = np.array(vec)
    assert workgroups(nx, len(vec)) < nx <= workgroups(nx, chunk)
    plain = None
    for project in (None, ("u", "v")):
        kw = dict(names=names, mixed=mixed, project=project)
        S = structure.functions2d(m, vectors=vec, **kw)
        again = structure.functions2d(m, vectors=vec, **kw)
        assert S.sums.tobytes() == again.sums.tobytes()
        parts = [structure.functions2d(m, vectors=vec[i:i + chunk], **kw) for i in range(0, len(vec), chunk)]
        C = np.concatenate([p.sums for p in parts])
        if project is None:
            plain = parts
        else:
            assert np.array_equal(S.proj, np.concatenate([p.proj for p in parts]))
        top = np.concatenate([majorant(p0, p.proj) for p0, p in zip(plain, parts)])
        err, tol = np.abs(S.sums - C), 2 * max(2 * nx, nx + 64) * U * top
        print("%s, %d vectors on %d workgroups, %s: %.3g of the two bounds" % (tag, len(vec), workgroups(nx, len(vec)), project,
                                                                                (err / np.where(tol > 0, tol, 1.0)).max()))
        assert np.all(err <= tol) and np.all(C[:, 1] > 0)
        assert np.all(np.abs(S.sums) <= top * (1 + 1e-9))                       # the majorant is one


def test_rows_of_4096_points():
    from niwqg_amd import structure
    m = make("coupled", 4096)
    names, mixed, vec = ("u", "v", "q_psi"), (("u", "v", "v"),), [(1, 0), (-511, 1), (512, 1), (2048, 4095)]
    S = structure.functions2d(m, names=names, vectors=vec, mixed=mixed)         # three rows of 32 KB in LDS: the row route at its largest
    check(S, device_values(m, names), 4096, "coupled 4096")
    # 80 vectors on four r_y, not sorted: 3276 workgroups for 4096 rows, 820 of them with two rows (the row route)
    vec = [(rx, ry) for rx in range(-10, 11) if rx for ry in (7, 0, 4095, 1)]
    check_rows_shared_by_a_workgroup(m, 4096, vec, 40, "coupled 4096")


def test_rows_of_8192_points():
    from niwqg_amd import structure
    m = make("coupled", 8192)
    vec = [(1, 0), (-1023, 1), (4096, 1), (3, 8191)]
    planes = device_values(m, ("u", "v", "q_psi", "phi"))
    S = structure.functions2d(m, names=("u",), vectors=vec)                      # the row route: one row of 64 KB
    check(S, planes, 8192, "coupled 8192 u")
    # the global route, and the combinations the x-pass refuses at this size
    S = structure.functions2d(m, names=("u", "v", "q_psi"), vectors=vec, mixed=(("u", "v", "v"),))
    check(S, planes, 8192, "coupled 8192 u/v/q_psi")
    S = structure.functions2d(m, names=("phi", "u"), vectors=vec, mixed=(("u", "phi", "phi"),))
    check(S, planes, 8192, "coupled 8192 phi/u")
    # 40 vectors of three names: 6553 workgroups for 8192 rows (the global route)
    vec = [(rx, ry) for rx in (-1000, -3, -1, 1, 2, 5, 64, 1024, 4096, 8190) for ry in (3, 0, 8191, 1)]
    check_rows_shared_by_a_workgroup(m, 8192, vec, 20, "coupled 8192")


# ---- 3. other routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 256])
def test_qgmodel_on_the_fused_grids(nx):
    from niwqg_amd import structure
    m = qg_with_scalar(nx)
    advance(m, 2)
    names, mixed = ("q", "c"), (("q", "c", "c"), ("c", "c", "c"))
    S = structure.functions2d(m, names=names, vectors=vectors(nx), mixed=mixed)
    assert S.project is None
    planes = device_values(m, names)
    check(S, planes, nx, "qg %d" % nx)
    S = structure.functions2d(m, names=("c", "q"), vectors=vectors(nx), project=("c", "q"))     # any pair of real names may be rotated
    check(S, planes, nx, "qg %d c/q rotated" % nx)
    S = structure.functions2d(m, names=("c",), vectors=vectors(nx))             # the scalar alone: plane b in slot 0
    check(S, planes, nx, "qg %d c" % nx)


@pytest.mark.parametrize("kind, nx, names, mixed", [("coupled", 96, ("u", "q_psi", "phi"), (("u", "phi", "phi"), ("u", "q_psi", "q_psi"))),
                                                     ("coupled", 96, ("phi", "v", "u"), (("v", "phi", "phi"), ("u", "v", "v"))),
                                                     ("qg", 48, ("u", "v", "q"), (("u", "v", "v"),))])
def test_any_size(kind, nx, names, mixed):
    from niwqg_amd import structure
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    advance(m, 2)
    planes = own_planes(m, names)
    S = structure.functions2d(m, names=names, vectors=vectors(nx), mixed=mixed)
    assert (S.project == ("u", "v")) == ("v" in names)
    check(S, planes, nx, "%s %d any-size" % (kind, nx))


# ---- 4. a plane wave ---------------------------------------------------------------------------------------------------------------
def test_plane_wave_on_qgmodel():
    from niwqg_amd import structure
    nx, A, k0, l0 = 64, 3e-5, 3, 5
    m = make("qg", nx)
    x = 2 * np.pi * np.arange(nx) / nx
    m.set_q(A * np.cos(k0 * x[None, :] + l0 * x[:, None]))
    vec = np.array(vectors(nx))
    S = structure.functions2d(m, names=("q",), vectors=vec)
    # <(d q)^2> = A^2 (1 - cos(k r_x dx + l r_y dy)), k dx = 2 pi k0 / nx
    want = A * A * (1 - np.cos(2 * np.pi * (k0 * vec[:, 0] + l0 * vec[:, 1]) / nx))
    assert np.abs(S.moment("q", 2) - want).max() <= 1e-12 * A * A
    assert np.allclose(S.length, np.hypot(vec[:, 0] * m.dx, vec[:, 1] * m.dy)) and S.project is None


# ---- 5. the x-pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("coupled", 96), ("qg", 64)])
def test_along_x_is_the_x_pass(kind, nx):
    from niwqg_amd import structure
    m = make(kind, nx, "filter")
    advance(m, 1)
    sep = separations(nx)
    names, mixed = (("q",), (("q", "q", "q"),)) if kind == "qg" else (("u", "v", "phi"), (("u", "v", "v"), ("u", "phi", "phi")))
    X = structure.functions(m, names=names, separations=sep, mixed=mixed)
    vec = np.concatenate([structure.axis_vectors(nx, "x", sep)[::-1], [(0, 1), (2, 3)]])
    S2 = structure.functions2d(m, names=names, vectors=vec, mixed=mixed)
    A = S2.along("x")
    assert A.names == X.names and np.array_equal(A.r, X.r) and A.triples == X.triples
    R = structure.reference(own_planes(m, names) if kind != "qg" else device_values(m, names), sep, mixed)
    tol = (2 * nx + max(2 * nx, nx + 64)) * U * R.abs_sums                      # the two kernels add in different orders: both bounds
    err = np.abs(A.sums - X.sums)
    print("%s %d along x: %.3g of the two bounds" % (kind, nx, (err / np.where(tol > 0, tol, 1.0)).max()))
    assert np.all(err <= tol)
    assert S2.along("y").r.tolist() == [1]


# ---- 6. determinism and accumulation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("coupled", 96), ("qg", 64)])
def test_determinism_accumulation_and_the_two_tables(kind, nx):
    from niwqg_amd import structure
    m = make(kind, nx, "filter")
    fused = not getattr(m, "_any_size", False)
    advance(m, 1)
    kw = dict(names=("q",), mixed=(("q", "q", "q"),)) if kind == "qg" else dict(names=("u", "v", "phi"), mixed=(("u", "phi", "phi"), ("u", "v", "v")))
    xkw = dict(kw, separations=separations(nx))
    kw["vectors"] = vectors(nx)
    a, b = structure.functions2d(m, **kw), structure.functions2d(m, **kw)
    assert a.sums.tobytes() == b.sums.tobytes() and np.all(a.moment(kw["names"][0], 2) > 0)
    A = structure.Accumulator2d(m, **kw)
    assert np.all(A.result().sums == 0) and A.result().samples == 0
    A.add()
    X = structure.Accumulator(m, **xkw)                                        # an x-accumulator in progress beside it
    X.add()
    A.add()
    X.add()
    R, XR = A.result(), X.result()
    assert R.samples == 2 and R.sums.tobytes() == (2 * a.sums).tobytes()      # x + x is exact
    assert R.table.tobytes() == (2 * a.sums / (2.0 * nx * nx)).tobytes()
    assert XR.samples == 2
    if fused:
        single = structure.functions2d(m, **kw)                               # takes the 2-D table over, not the x-table
        assert single.sums.tobytes() == a.sums.tobytes()
        X.add()
        assert X.result().samples == 3 and X.result().sums.tobytes() == (1.5 * XR.sums).tobytes()
        with pytest.raises(RuntimeError, match="another call"):
            A.add()
        with pytest.raises(RuntimeError, match="another call"):
            A.result()
        A.reset()
        A.add()
        once = structure.functions(m, **xkw)                                  # and the other way round
        assert once.sums.tobytes() == (XR.sums / 2).tobytes()
        A.add()
        assert A.result().samples == 2 and A.result().sums.tobytes() == (2 * a.sums).tobytes()
        L, h = m._ctx.L, m._ctx.h                                              # another vector list with accumulate = 1
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        from niwqg_amd import _lib
        code = _lib.PDF_Q if kind == "qg" else _lib.FLOW_U
        assert L.nq_structure2(h, 1, ints(code), 2, ints(1, 0, 0, 1), None, -1, -1, 0, None, 0) == 0
        assert L.nq_structure2(h, 1, ints(code), 2, ints(1, 0, 0, 2), None, -1, -1, 0, None, 1) == -1 and b"accumulate" in L.nq_last_error(h)
        assert L.nq_structure2(h, 1, ints(code), 2, ints(0, 1, 1, 0), None, -1, -1, 0, None, 1) == -1
        assert L.nq_structure2(h, 1, ints(code), 2, ints(1, 0, 0, 1), None, -1, -1, 0, None, 1) == 0
    A.reset()
    assert np.all(A.result().sums == 0)
    A.add()
    assert A.result().samples == 1 and A.result().sums.tobytes() == a.sums.tobytes()


# ---- 7. leaves the run alone -------------------------------------------------------------------------------------------------------
def test_calls_leave_the_run_alone_and_the_memory_they_take():
    from niwqg_amd import structure
    a, b = make("coupled", 128, "filter"), make("coupled", 128, "filter")
    before = a._ctx.device_bytes()
    vec = [(1, 0), (0, 1), (-5, 7)]
    structure.functions2d(a, names=("u", "v", "q_psi"), vectors=vec)
    table = 256 * 31 * 8 + 256 * 16 + 256 * 2 * 8                               # the table, the vectors and their (c_x, c_y)
    partials = 128 * 3 * 31 * 8                                                 # one workgroup per row x vectors x columns
    planes = 3 * 128 * 128 * 8
    assert a._ctx.device_bytes() - before == table + partials + planes
    structure.functions2d(a, names=("u", "v", "q_psi"), vectors=vec)
    structure.functions2d(a, names=("u",), vectors=vec[:2])
    assert a._ctx.device_bytes() - before == table + partials + planes          # nothing grows for a smaller call
    structure.functions2d(a, names=("u", "v", "phi"), vectors=vec)              # two real planes and a complex one
    assert a._ctx.device_bytes() - before == table + partials + planes + 128 * 128 * 8
    for _ in range(4):
        advance(a, 1)
        advance(b, 1)
        structure.functions2d(a, names=("u", "q_psi", "phi"), mixed=(("u", "phi", "phi"),))
        structure.functions2d(a, names=("ow", "gradphi2", "phi2"), vectors=[(1, 1), (5, 0)])
    for n in ("qh", "phih", "ph"):
        assert np.array(getattr(a, n)).tobytes() == np.array(getattr(b, n)).tobytes(), n


# ---- 8. return codes ---------------------------------------------------------------------------------------------------------------
def test_return_codes():
    import niwqg_amd
    from niwqg_amd import structure, _lib
    L = _lib.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    k = make("coupled", 64)
    h = k._ctx.h
    out, n = np.zeros(256 * 31), ctypes.c_longlong(0)
    uv = ints(_lib.FLOW_U, _lib.FLOW_V)
    assert L.nq_structure2_read(h, ctypes.byref(n), _lib._dptr(out)) == -4                                   # no table yet
    call = lambda nf, f, nv, v, proj=None, pa=-1, pb=-1, nt=0, t=None, acc=0: L.nq_structure2(h, nf, f, nv, v, proj, pa, pb, nt, t, acc)
    for bad in ((0, 0), (1, 0, 1, 0), (1, -1), (64, 0), (-64, 0), (0, 64), (3, 2, 3 - 64, 2)):
        assert call(2, uv, len(bad) // 2, ints(*bad)) == -1 and b"vector" in L.nq_last_error(h), bad
    assert call(2, uv, 257, ints(*[v for i in range(257) for v in (i % 60 + 1, i // 60)])) == -1
    assert call(2, uv, 1, ints(1, 0), dbl(float("nan"), 1.0), 0, 1) == -1 and b"finite" in L.nq_last_error(h)
    assert call(2, uv, 1, ints(1, 0), dbl(float("inf"), 0.0), 0, 1) == -1
    assert call(2, ints(_lib.FLOW_U, _lib.SF_PHI), 1, ints(1, 0), dbl(1.0, 0.0), 0, 1) == -1 and b"complex" in L.nq_last_error(h)
    assert call(2, uv, 1, ints(1, 0), dbl(1.0, 0.0), 0, 0) == -1 and b"twice" in L.nq_last_error(h)
    assert call(2, uv, 1, ints(1, 0), dbl(1.0, 0.0), 0, 2) == -1                                            # an index past the list
    assert call(2, uv, 1, ints(1, 0), dbl(1.0, 0.0), -1, -1) == -1 and call(2, uv, 1, ints(1, 0), None, 0, 1) == -1
    assert call(4, ints(_lib.FLOW_U, _lib.FLOW_V, _lib.PDF_Q, _lib.PDF_QPSI), 1, ints(1, 0)) == -1
    assert call(2, ints(_lib.FLOW_U, _lib.SF_PHI), 1, ints(1, 0), nt=1, t=ints(1, 0, 0)) == -1               # phi first in a triple
    assert call(2, uv, 1, ints(1, 0), acc=1) == -1                                                          # accumulate before any call
    assert L.nq_structure2_read(h, ctypes.byref(n), _lib._dptr(out)) == -4
    assert call(2, uv, 2, ints(0, 1, 1, 0), dbl(0.0, 1.0, 1.0, 0.0), 0, 1) == 0
    assert call(2, uv, 2, ints(0, 1, 1, 0), dbl(0.0, 1.0, 1.0, 1e-300), 0, 1, acc=1) == -1                   # other numbers
    assert call(2, uv, 2, ints(0, 1, 1, 0), dbl(0.0, 1.0, 1.0, 0.0), 1, 0, acc=1) == -1                      # the other order of the pair
    assert call(2, uv, 2, ints(0, 1, 1, 0), dbl(0.0, 1.0, 1.0, 0.0), 0, 1, acc=1) == 0
    assert L.nq_structure2_read(h, ctypes.byref(n), _lib._dptr(out)) == 0 and n.value == 2 and out[1] > 0
    assert L.nq_structure_read(h, ctypes.byref(n), _lib._dptr(out)) == -4                                    # the x-table is another one
    g = make("qg", 64)
    with pytest.raises(NotImplementedError, match="QGModel"):
        structure.functions2d(g, names=("u",))
    with pytest.raises(ValueError, match="valid names"):
        structure.functions2d(g, names=("q", "c"))                                                           # no passive scalar here
    assert L.nq_structure2(g._ctx.h, 1, ints(_lib.FLOW_U), 1, ints(1, 0), None, -1, -1, 0, None, 0) == -1 and b"QGModel" in L.nq_last_error(g._ctx.h)
    assert L.nq_structure2(g._ctx.h, 1, ints(_lib.SF_PHI), 1, ints(1, 0), None, -1, -1, 0, None, 0) == -1
    with pytest.raises(ValueError, match="vectors"):
        structure.functions2d(k, vectors=[(0, 0)])
    with pytest.raises(ValueError, match="complex"):
        structure.functions2d(k, names=("u", "phi"), project=("u", "phi"))
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        structure.functions2d(s, names=("u",))
    with pytest.raises(NotImplementedError, match="slab"):
        structure.Accumulator2d(s, names=("u",))
    hs = s._ctx.sim.ranks[0].h
    assert L.nq_structure2(hs, 1, ints(_lib.FLOW_U), 1, ints(1, 0), None, -1, -1, 0, None, 0) == -4 and len(L.nq_last_error(hs)) > 0
    assert L.nq_structure2_read(hs, ctypes.byref(n), _lib._dptr(out)) == -4
