"""Structure functions (niwqg_amd/structure.py), the parts that need no GPU: the numpy restatement
``structure.reference`` against closed forms of a cosine, the periodicity and the autocorrelation closure, the derived
quantities and the normalisation, every validation error, and the header's declarations."""

import numpy as np
import pytest

from niwqg_amd import _abi, _lib, structure


def cosine(nx=96, ny=40, k0=3, A=1.7, seed=1):
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0, 2 * np.pi, ny)
    x = 2 * np.pi * np.arange(nx) / nx
    return A * np.cos(k0 * x[None, :] + theta[:, None]), 2 * np.pi * k0 / nx, A


def col(S, name, k):
    return S.table[:, structure.COLS * S.names.index(name) + k]


def test_moments_of_a_cosine():
    # d = A cos(k0 (x + r) + th) - A cos(k0 x + th) = -2 A sin(k0 r / 2) sin(k0 x + th + k0 r / 2): over whole periods in x the mean of
    # sin^2 is 1/2 and of sin^4 is 3/8, so <d^2> = 2 A^2 sin^2(k0 r / 2) = A^2 (1 - cos k0 r) and <d^4> = 6 A^4 sin^4(k0 r / 2)
    a, k0, A = cosine()
    r = np.array([1, 2, 5, 17, 48, 95])
    S = structure.reference({"a": a}, r)
    for p in (1, 3, 5):
        assert np.abs(S.moment("a", p)).max() <= 1e-13 * A ** p, p
    assert np.abs(S.moment("a", 2) - A ** 2 * (1 - np.cos(k0 * r))).max() <= 1e-13 * A ** 2
    assert np.abs(S.moment("a", 4) - 6 * A ** 4 * np.sin(k0 * r / 2) ** 4).max() <= 1e-13 * A ** 4
    assert np.abs(S.abs_moment("a", 2) - S.moment("a", 2)).max() == 0 and np.all(S.abs_moment("a", 3) > 0)


def test_periodicity():
    rng = np.random.default_rng(2)
    a = rng.standard_normal((12, 64))
    phi = rng.standard_normal((12, 64)) + 1j * rng.standard_normal((12, 64))
    r = np.array([1, 7, 31])
    S, R = structure.reference({"a": a, "phi": phi}, r), structure.reference({"a": a, "phi": phi}, (64 - r)[::-1])
    for p in range(1, 7):
        top = np.abs(a).max() ** p * 2 ** p
        assert np.abs(S.moment("a", p) - (-1) ** p * R.moment("a", p)[::-1]).max() <= 1e-13 * top, p
        assert np.abs(S.moment("phi", p) - R.moment("phi", p)[::-1]).max() <= 1e-13 * top * 2 ** p, p
    assert np.abs(S.mean_increment() + R.mean_increment()[::-1]).max() <= 1e-13
    assert np.all(col(S, "phi", 8) == 0)


def test_closure_against_the_autocorrelation():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((20, 128))
    r = structure.default_separations(128)
    S = structure.reference({"a": a}, r)
    ah = np.fft.fft(a, axis=1)
    corr = np.fft.ifft(np.abs(ah) ** 2, axis=1).real.sum(axis=0)              # sum_xy a(x) a(x + r)
    want = 2 * ((a * a).sum() - corr[r])
    assert np.abs(S.sums[:, 1] - want).max() <= 1e-12 * (a * a).sum()


def test_derived_quantities_and_normalisation():
    rng = np.random.default_rng(4)
    u, v = rng.standard_normal((2, 10, 32))
    phi = rng.standard_normal((10, 32)) + 1j * rng.standard_normal((10, 32))
    r = [1, 3, 16]
    S = structure.reference({"u": u, "v": v, "phi": phi}, r, mixed=(("u", "v", "v"), ("u", "phi", "phi"), ("u", "u", "u")))
    assert S.samples == 1 and S.points == 320 and np.array_equal(S.table, S.sums / 320.0) and S.x is None
    for s, rr in enumerate(r):
        du, dv, dp = (np.roll(f, -rr, axis=1) - f for f in (u, v, phi))
        assert np.isclose(S.mixed[("u", "v", "v")][s], (du * dv * dv).mean(), rtol=1e-13, atol=1e-15)
        assert np.isclose(S.mixed[("u", "phi", "phi")][s], (du * np.abs(dp) ** 2).mean(), rtol=1e-12, atol=1e-15)
        assert np.isclose(S.mixed[("u", "u", "u")][s], S.moment("u", 3)[s], rtol=1e-12, atol=1e-15)
        assert np.isclose(S.third_order("u", "v")[s], (du * (du * du + dv * dv)).mean(), rtol=1e-12, atol=1e-15)
        assert np.isclose(S.flatness("u")[s], (du ** 4).mean() / (du ** 2).mean() ** 2, rtol=1e-12)
        assert np.isclose(S.abs_moment("u", 5)[s], (np.abs(du) ** 5).mean(), rtol=1e-12)
        assert np.isclose(S.moment("phi", 3)[s], (np.abs(dp) ** 3).mean(), rtol=1e-12)
        assert np.isclose(S.abs_sums[s, 2], (np.abs(du) ** 3).sum(), rtol=1e-12)
    with pytest.raises(ValueError, match="mixed="):
        S.third_order("v", "u")
    with pytest.raises(ValueError, match="1 to 6"):
        S.moment("u", 7)
    T = structure.StructureFunctions(["u"], [1, 2], [], np.ones((2, 9)), 4, 100, dx=0.5)
    assert np.all(T.table == 1.0 / 400) and np.array_equal(T.x, [0.5, 1.0])


def test_default_separations():
    assert structure.default_separations(64).tolist() == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32]
    assert structure.default_separations(96).tolist() == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48]
    d = structure.default_separations(4096)
    assert d[-1] == 2048 and d.size == 22 and np.all(np.diff(d) > 0)
    assert structure.default_separations(8192).size <= structure.MAX_SEPS


def fake(kind="coupled", nx=64, any_size=True, **kw):
    """a model as far as the validation looks at one (no library is loaded)"""
    from niwqg_amd import CoupledModel, QGModel
    cls = QGModel.Model if kind == "qg" else CoupledModel.Model
    m = cls.__new__(cls)
    m.__dict__.update(dict(nx=nx, ny=nx, _any_size=any_size, passive_scalar=True, _ctx=object()), **kw)
    return m


def test_validation_errors():
    V = lambda m, names=("u",), sep=None, mixed=(), direction="x": structure._validate(m, names, sep, mixed, direction, "structure.functions")
    k = fake()
    assert V(k, ("u", "q_psi", "phi"), [1, 63], (("u", "phi", "phi"),))[0] == ["u", "q_psi", "phi"]
    assert structure.available(k)[-1] == "phi" and "ow" in structure.available(k) and "q_psi" in structure.available(k)
    with pytest.raises(NotImplementedError, match="slab"):
        V(fake(any_size=False))
    with pytest.raises(NotImplementedError, match="along x"):
        V(k, direction="y")
    with pytest.raises(ValueError, match="three real names"):
        V(k, ("u", "v", "q", "q_psi"))
    with pytest.raises(ValueError, match="three real names"):
        V(k, ("u", "v", "q", "phi"))
    for bad in ([0, 1], [1, 64], [2, 2], [3, 1], [], list(range(1, 63)) + [63, 64, 65], [1.5]):
        with pytest.raises(ValueError, match="separations"):
            V(fake(nx=128) if len(bad) > 60 else k, sep=bad)
    with pytest.raises(ValueError, match="valid names"):
        V(k, ("zeta",))
    with pytest.raises(ValueError, match="valid names"):
        V(fake("qg"), ("q", "phi"))
    with pytest.raises(ValueError, match="valid names"):
        V(fake("qg"), ("gradphi2",))
    with pytest.raises(NotImplementedError, match="QGModel"):
        V(fake("qg", any_size=False, _ctx=_lib.Context.__new__(_lib.Context)), ("u",))
    assert V(fake("qg"), ("q", "c", "u"))[0] == ["q", "c", "u"]
    for bad in ((("u", "v"),), (("u", "v", "w"),), (("phi", "u", "u"),), (("u", "phi", "u"),), (("u", "u", "phi"),), (("u", "u", "u"),) * 2,
                tuple(("u", "u", n) for n in ("u", "v", "q_psi")) + (("v", "v", "v"), ("v", "u", "u"))):
        with pytest.raises(ValueError, match="mixed"):
            V(k, ("u", "v", "q_psi") if "phi" not in str(bad) else ("u", "v", "phi"), mixed=bad)
    big = fake(nx=8192, any_size=False, _ctx=_lib.Context.__new__(_lib.Context))
    with pytest.raises(NotImplementedError, match="8192"):
        V(big, ("u", "v"), mixed=(("u", "v", "v"),))
    with pytest.raises(NotImplementedError, match="8192"):
        V(big, ("u", "phi"))
    assert V(big, ("u", "v"), mixed=(("u", "u", "u"),))[2] == [("u", "u", "u")] and V(big, ("phi",))[0] == ["phi"]
    with pytest.raises(ValueError, match="complex"):
        structure.reference({"phi": np.zeros((4, 8))}, [1])
    with pytest.raises(ValueError, match="shape"):
        structure.reference({"a": np.zeros((4, 8)), "b": np.zeros((4, 6))}, [1])


def test_the_header_declares_the_entry_points():
    protos, consts, _ = _abi.read(open(_lib.HEADER).read())
    by_name = {n: (ret, params) for n, ret, params in protos}
    assert [t for t, _ in by_name["nq_structure"][1]] == ["nq_ctx*", "int", "const int*", "int", "const int*", "int", "const int*", "int"]
    assert [t for t, _ in by_name["nq_structure_read"][1]] == ["nq_ctx*", "long long*", "double*"]
    assert [t for t, _ in by_name["nq_any_increments"][1]] == ["nq_any*", "int", "const void* const*", "const int*", "int", "int", "int", "const int*",
                                                              "int", "const int*", "double*"]
    for n in ("nq_structure", "nq_structure_read", "nq_any_increments"):
        assert by_name[n][0] == "int" and n in _lib.EXPORTS
        _lib.signature((n,) + by_name[n])
    assert (consts["NQ_SF_MAX_SEPS"], consts["NQ_SF_MAX_FIELDS"], consts["NQ_SF_MAX_TRIPLES"], consts["NQ_SF_COLS"]) == (64, 3, 4, 9)
    others = [v for k, v in consts.items() if k.startswith(("NQ_PDF_Q", "NQ_PDF_C", "NQ_PDF_PHI2", "NQ_FLOW_", "NQ_AVG_"))]
    assert len(others) >= 12 and consts["NQ_SF_PHI"] not in others
    assert consts["NQ_SF_PART_MAX_BYTES"] == 4096 * 64 * 31 * 8
    assert structure._CODES["phi"] == consts["NQ_SF_PHI"] and structure.MAX_SEPS == 64
