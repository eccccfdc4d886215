"""Structure functions at two-dimensional separations (niwqg_amd/structure.py), the parts that need no GPU:
the numpy restatement ``structure.reference2d`` against a brute-force loop, its agreement with ``structure.reference`` along x (bit
for bit) and along y (by transposition), the vector sets, the angle average, every refusal, and the header's declarations."""

import numpy as np
import pytest

from niwqg_amd import _abi, _lib, structure
from test_structure_host import fake


def planes(ny=6, nx=8, seed=5):
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal((2, ny, nx))
    phi = rng.standard_normal((ny, nx)) + 1j * rng.standard_normal((ny, nx))
    return u, v, phi


def brute(fields, vec, mixed, project, proj):
    """the definitions as a triple loop over vectors, rows and columns"""
    names = list(fields)
    ny, nx = fields[names[0]].shape
    out = np.zeros((len(vec), 9 * len(names) + len(mixed)))
    for s, (rx, ry) in enumerate(vec):
        for y in range(ny):
            for x in range(nx):
                d = {n: fields[n][(y + ry) % ny, (x + rx) % nx] - fields[n][y, x] for n in names}
                if project:
                    a, b = project
                    cx, cy = proj[s]
                    d[a], d[b] = cx * d[a] + cy * d[b], -cy * d[a] + cx * d[b]
                for i, n in enumerate(names):
                    if n == "phi":
                        m = abs(d[n])
                        col = [m, m ** 2, m ** 3, m ** 4, m ** 5, m ** 6, d[n].real, d[n].imag, 0.0]
                    else:
                        col = [d[n] ** p for p in range(1, 7)] + [abs(d[n]), abs(d[n]) ** 3, abs(d[n]) ** 5]
                    out[s, 9 * i:9 * i + 9] += col
                for k, (a, b, c) in enumerate(mixed):
                    out[s, 9 * len(names) + k] += d[a] * abs(d["phi"]) ** 2 if b == "phi" else d[a] * d[b] * d[c]
    return out


VECTORS = [(1, 0), (0, 1), (-3, 2), (7, 5), (0, 5)]


@pytest.mark.parametrize("project", [None, ("u", "v")])
def test_reference2d_against_a_brute_force_loop(project):
    u, v, phi = planes()
    fields = {"u": u, "v": v, "phi": phi}
    mixed = (("u", "v", "v"), ("u", "phi", "phi"), ("v", "v", "v"))
    R = structure.reference2d(fields, VECTORS, mixed=mixed, project=project)
    assert (R.proj is None) == (project is None)
    if project:
        assert np.array_equal(R.proj, structure.unit_vectors(VECTORS)) and np.allclose(np.hypot(R.proj[:, 0], R.proj[:, 1]), 1, rtol=1e-15)
    want = brute(fields, VECTORS, mixed, project, R.proj)
    scale = np.maximum(np.abs(want), R.abs_sums)
    assert np.all(np.abs(R.sums - want) <= 1e-13 * scale), np.abs(R.sums - want).max()
    assert np.all(R.abs_sums >= np.abs(R.sums) * (1 - 1e-14)) and np.all(R.sums[:, 26] == 0)
    assert R.samples == 1 and R.points == 48 and np.array_equal(R.vectors, VECTORS)


def test_x_vectors_give_the_bits_of_reference():
    rng = np.random.default_rng(6)
    u, v, q = rng.standard_normal((3, 40, 96))
    fields, mixed, sep = {"u": u, "v": v, "q": q}, (("u", "v", "v"), ("u", "q", "q")), [1, 2, 17, 48, 95]
    X = structure.reference(fields, sep, mixed)
    for project in (None, ("u", "v")):
        R = structure.reference2d(fields, structure.axis_vectors(96, "x", sep), mixed=mixed, project=project)
        assert R.sums.tobytes() == X.sums.tobytes() and R.abs_sums.tobytes() == X.abs_sums.tobytes(), project
        A = R.along("x")
        assert isinstance(A, structure.StructureFunctions) and np.array_equal(A.r, sep) and A.table.tobytes() == X.table.tobytes()
        assert R.along("y").r.size == 0
    # tall planes (more than one row block of reference's summation)
    w = rng.standard_normal((600, 512))
    assert structure.reference2d({"w": w}, [(5, 0)]).sums.tobytes() == structure.reference({"w": w}, [5]).sums.tobytes()


def test_y_vectors_by_transposition():
    # along (0, r) the unit vector is (0, 1): L = d v and T = -d u, the x-increments of the transposed planes
    rng = np.random.default_rng(7)
    u, v = rng.standard_normal((2, 24, 40))
    sep = [1, 3, 11, 23]
    R = structure.reference2d({"u": u, "v": v}, structure.axis_vectors(40, "y", sep), mixed=(("u", "v", "v"),), project=("u", "v"))
    assert np.array_equal(R.proj, [[0.0, 1.0]] * 4)
    # the rotated increments themselves are exact: 0 d_u + 1 d_v = d_v and -1 d_u + 0 d_v = -d_u, bit for bit, at every point
    for r in sep:
        du, dv = structure.increments2d(u, 0, r), structure.increments2d(v, 0, r)
        cx, cy = R.proj[0]
        assert np.array_equal(cx * du + cy * dv, dv) and np.array_equal(-cy * du + cx * dv, -du)
        assert np.array_equal(dv.T, structure.increments(np.ascontiguousarray(v.T), r))      # and they are v.T's x-increments
    # The SUMS are not bitwise those of the transposed planes: numpy adds a (ny, nx) block pairwise in memory order, and the
    # transposed array presents the same terms in another order.  Every column, the even ones included, is therefore held to
    # 1e-13 of the sum of the absolute values of its terms (the odd columns of T with the sign of -u).
    L, T =structure.reference({"a": np.ascontiguousarray(v.T)}, sep), structure.reference({"a": np.ascontiguousarray(-u.T)}, sep)
    for i, X in enumerate((L, T)):
        got = R.sums[:, 9 * i:9 * i + 9]
        assert np.all(np.abs(got - X.sums) <= 1e-13 * X.abs_sums), i
    # the triple (u, v, v) holds L T T = d v (d u)^2
    for s, r in enumerate(sep):
        du, dv = np.roll(u, -r, axis=0) - u, np.roll(v, -r, axis=0) - v
        assert np.isclose(R.sums[s, 18], (dv * du * du).sum(), rtol=1e-12, atol=1e-12)
    A = R.along("y")
    assert np.array_equal(A.r, sep) and np.array_equal(A.sums, R.sums)
    # without the rotation the columns are those of the planes themselves: u.T, with its sign
    P = structure.reference2d({"u": u, "v": v}, structure.axis_vectors(40, "y", sep), project=None)
    Ut = structure.reference({"a": np.ascontiguousarray(u.T)}, sep)
    assert np.all(np.abs(P.sums[:, :9] - Ut.sums) <= 1e-13 * Ut.abs_sums)
    odd = [0, 2, 4]
    assert np.all(np.abs(R.sums[:, 9:18][:, odd] + Ut.sums[:, odd]) <= 1e-13 * Ut.abs_sums[:, odd])       # T = -d u: odd columns change sign


def test_ring_vectors():
    for nx, angles in ((64, 8), (4096, 8), (8192, 16), (256, 5)):
        radii = structure.default_separations(nx)
        v, ring = structure._rings(nx, None, angles)
        assert np.array_equal(v, structure.ring_vectors(nx, angles=angles))
        assert 0 < len(v) <= structure.MAX_VECS and np.all(v[:, 1] >= 0) and np.all(np.abs(v[:, 0]) <= nx - 1)
        assert len(set(map(tuple, v.tolist()))) == len(v) and not np.any((v[:, 0] == 0) & (v[:, 1] == 0))
        assert not np.any((v[:, 1] == 0) & (v[:, 0] < 0))
        assert np.all(np.abs(np.hypot(v[:, 0], v[:, 1]) - ring) <= np.sqrt(2) / 2 + 1e-12)
        assert set(ring.tolist()) <= set(radii.astype(float).tolist()) and ring.max() == radii.max()
        structure._check_vectors(v, nx, nx, "test")
    assert structure.ring_vectors(64, radii=[1, 5, 20], angles=2).tolist() == [[1, 0], [0, 1], [5, 0], [0, 5], [20, 0], [0, 20]]
    assert structure.ring_vectors(64, radii=[10], angles=4).tolist() == [[10, 0], [7, 7], [0, 10], [-7, 7]]
    assert structure.axis_vectors(64, "y", [1, 4]).tolist() == [[0, 1], [0, 4]] and len(structure.axis_vectors(4096, "x")) == 22
    with pytest.raises(ValueError, match="radii"):
        structure.ring_vectors(64, radii=[64])
    with pytest.raises(ValueError, match="at most"):
        structure.ring_vectors(4096, radii=np.arange(100, 200), angles=8)
    with pytest.raises(ValueError, match="direction"):
        structure.axis_vectors(64, "z")


def test_isotropic_average_of_a_single_mode():
    # a = cos(k (x + y)): d_r a = -2 sin(k (r_x + r_y) / 2) sin(k (x + y) + ...), so <d^2> = 1 - cos(k (r_x + r_y)) per vector
    n, k0 = 64, 3
    k = 2 * np.pi * k0 / n
    x = np.arange(n)
    a = np.cos(k * (x[None, :] + x[:, None]))
    v, ring = structure._rings(n, [2, 5, 12], 8)
    R = structure.reference2d({"a": a}, v)
    want = 1 - np.cos(k * (v[:, 0] + v[:, 1]))
    assert np.abs(R.moment("a", 2) - want).max() <= 1e-12
    R.ring = ring
    radius, table, count = R.isotropic()
    assert len(radius) == 3 and count.sum() == len(v) and table.shape == (3, 9)
    for b, rho in enumerate((2.0, 5.0, 12.0)):
        assert count[b] == (ring == rho).sum()
        assert np.isclose(table[b, 1], want[ring == rho].mean(), rtol=0, atol=1e-12)
        assert np.isclose(radius[b], np.hypot(v[ring == rho, 0], v[ring == rho, 1]).mean())
    # explicit edges: [0, 3.5), [3.5, 20); and without rings one bin per distinct length
    radius, table, count = R.isotropic(edges=[0, 3.5, 20])
    inner = np.hypot(v[:, 0], v[:, 1]) < 3.5
    assert count.tolist() == [int(inner.sum()), int((~inner).sum())] and np.isclose(table[0, 1], want[inner].mean(), atol=1e-12)
    R.ring = None
    assert R.isotropic()[2].sum() == len(v) and len(R.isotropic()[0]) == len(np.unique(R.length))
    with pytest.raises(ValueError, match="edges"):
        R.isotropic(edges=[1])
    S = structure.StructureFunctions2d(["a"], [(3, 4), (-3, 0)], [], np.ones((2, 9)), 2, 50, dx=0.5, dy=0.25)
    assert np.allclose(S.length, [np.hypot(1.5, 1.0), 1.5]) and np.allclose(S.angle, [np.arctan2(1.0, 1.5), np.pi]) and np.all(S.table == 0.01)
    assert np.allclose(structure.unit_vectors([(3, 4)], 0.5, 0.25), [[1.5 / np.hypot(1.5, 1), 1 / np.hypot(1.5, 1)]])


def test_refusals():
    V = lambda m, names=("u", "v"), vec=((1, 0),), mixed=(), project=("u", "v"): structure._validate2d(m, names, vec, mixed, project, "structure.functions2d")
    k = fake()
    names, vec, mixed, project, ring = V(k, ("u", "v", "phi"), [(1, 0), (-63, 63), (0, 5)], (("u", "phi", "phi"),))
    assert names == ["u", "v", "phi"] and vec.tolist() == [[1, 0], [-63, 63], [0, 5]] and project == ("u", "v") and ring is None
    assert V(k, ("u", "q_psi"))[3] is None and V(k, project=None)[3] is None                # the default pair: off without both names
    assert V(k, ("v", "u", "q"), project=("q", "v"))[3] == ("q", "v")
    d = V(k, vec=None)
    assert len(d[1]) == len(structure.ring_vectors(64)) and len(d[4]) == len(d[1])
    with pytest.raises(NotImplementedError, match="slab"):
        V(fake(any_size=False))
    with pytest.raises(NotImplementedError, match="QGModel"):
        V(fake("qg", any_size=False, _ctx=_lib.Context.__new__(_lib.Context)), ("u",))
    assert V(fake("qg"), ("q", "c", "u"))[0] == ["q", "c", "u"]
    for bad in ([(0, 0)], [(64, 0)], [(-64, 1)], [(1, -1)], [(1, 64)], [(1, 0), (1, 0)], [(3, 2), (3 - 64, 2)], [(1.5, 0)], [], [1, 2],
                [(i, 1) for i in range(-60, 60)] + [(i, 2) for i in range(-60, 60)] + [(i, 3) for i in range(20)]):
        with pytest.raises(ValueError, match="vectors|vector "):
            V(fake(nx=128) if len(bad) > 100 else k, vec=bad)
    with pytest.raises(ValueError, match="valid names"):
        V(k, ("zeta",))
    with pytest.raises(ValueError, match="valid names"):
        V(fake("qg"), ("q", "phi"))
    with pytest.raises(ValueError, match="three real names"):
        V(k, ("u", "v", "q", "q_psi"))
    for bad in ((("u", "v"),), (("phi", "u", "u"),), (("u", "u", "phi"),), (("u", "u", "u"),) * 2):
        with pytest.raises(ValueError, match="mixed"):
            V(k, ("u", "v", "phi"), mixed=bad)
    for bad in (("u", "phi"), ("phi", "u")):
        with pytest.raises(ValueError, match="complex"):
            V(k, ("u", "v", "phi"), project=bad)
    for bad in (("u", "q"), ("u", "u"), ("u",), ("q", "q_psi")):
        with pytest.raises(ValueError, match="project"):
            V(k, project=bad)
    for bad in (np.zeros((2, 2)), [[np.nan, 1.0]], [[np.inf, 0.0]], [1.0, 0.0]):
        with pytest.raises(ValueError, match="proj"):
            structure._check_proj(bad, 1, "structure.functions2d")
    big = fake(nx=8192, any_size=False, _ctx=_lib.Context.__new__(_lib.Context))         # what the x-pass refuses at this size
    assert V(big, ("u", "v", "phi"), mixed=(("u", "v", "v"), ("u", "phi", "phi")))[2] == [("u", "v", "v"), ("u", "phi", "phi")]
    with pytest.raises(NotImplementedError, match="along x"):                             # the x-call keeps refusing y
        structure._validate(k, ("u",), None, (), "y", "structure.functions")
    with pytest.raises(ValueError, match="complex"):
        structure.reference2d({"phi": np.zeros((4, 8))}, [(1, 0)])
    with pytest.raises(ValueError, match="shape"):
        structure.reference2d({"a": np.zeros((4, 8)), "b": np.zeros((4, 6))}, [(1, 0)])
    with pytest.raises(ValueError, match="vectors"):
        structure.reference2d({"a": np.zeros((4, 8))}, [(0, 4)])


def test_the_header_declares_the_entry_points():
    protos, consts, _ = _abi.read(open(_lib.HEADER).read())
    by_name = {n: (ret, params) for n, ret, params in protos}
    assert [t for t, _ in by_name["nq_structure2"][1]] == ["nq_ctx*", "int", "const int*", "int", "const int*", "const double*", "int", "int", "int",
                                                          "const int*", "int"]
    assert [t for t, _ in by_name["nq_structure2_read"][1]] == ["nq_ctx*", "long long*", "double*"]
    assert [t for t, _ in by_name["nq_any_increments2"][1]] == ["nq_any*", "int", "const void* const*", "const int*", "int", "int", "int", "const int*",
                                                               "const double*", "int", "int", "int", "const int*", "double*"]
    for n in ("nq_structure2", "nq_structure2_read", "nq_any_increments2"):
        assert by_name[n][0] == "int" and n in _lib.EXPORTS
        _lib.signature((n,) + by_name[n])
    assert consts["NQ_SF2_MAX_VECS"] == 256 == structure.MAX_VECS
    assert 64 * consts["NQ_SF2_MAX_VECS"] * 31 * 8 <= consts["NQ_SF_PART_MAX_BYTES"]
