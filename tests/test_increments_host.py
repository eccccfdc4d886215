"""PDFs of the field increments (niwqg_amd/increments.py), the parts that need no GPU: the numpy
specification ``increments.reference`` against a loop of ``pdfs.bin_index`` and ``np.bincount``, the closure of the result class
with bounds derived from the bin width, the default ranges, every ValueError of the contract, ``along`` and ``isotropic``, and the
header's declarations.

Closure bounds (ranges that contain every increment, bin width h, so |c - x| <= h / 2 for every point x and its bin centre c):
|<c> - <x>| <= h / 2, and |<c^2> - <x^2>| = |<(c - x)(c + x)>| <= <|c - x| (2 |x| + |c - x|)> <= h <|x|> + h^2 / 4."""
import numpy as np
import pytest

from niwqg_amd import _abi, _lib, increments, pdfs, structure
from test_structure_host import fake

SEPS = [1, 2, 5, 11]
VECTORS = [(1, 0), (0, 1), (-3, 2), (7, 5), (0, 5)]


def planes(ny=12, nx=16, seed=3):
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal((2, ny, nx))
    phi = rng.standard_normal((ny, nx)) + 1j * rng.standard_normal((ny, nx))
    return {"u": u, "v": 0.3 * v, "phi": phi}


def loop_counts(values, lo, hi, bins):
    """[bins, below, above, nan] by the bin rule, one np.bincount per class"""
    i = pdfs.bin_index(values, lo, hi, bins).ravel()
    return np.concatenate([np.bincount(i[(i >= 0) & (i < bins)], minlength=bins), [(i == -1).sum(), (i == bins).sum(), (i == bins + 1).sum()]])


def check_against_loop(R, values, bins):
    """values(s) -> {name: plane of the binned values of row s}"""
    for s in range(len(R.counts[R.names[0]])):
        v = values(s)
        for n in R.names:
            lo, hi = R.ranges[n][s]
            want = loop_counts(v[n], lo, hi, bins)
            got = np.concatenate([R.counts[n][s], [R.below[n][s], R.above[n][s], R.nan[n][s]]])
            assert np.array_equal(got, want), (n, s)
            assert got.sum() == v[n].size
            assert np.array_equal(R.edges[n][s], lo + (hi - lo) * np.arange(bins + 1) / bins)


def test_reference_along_x_equals_a_loop_of_bin_index():
    f = planes()
    for ranges in (None, {"u": (-0.5, 0.7), "v": np.array([[-1, 1], [-2, 2], [-0.1, 0.1], [-3, 4.0]]), "phi": (0.0, 1.5)}):
        R = increments.reference(f, SEPS, bins=16, ranges=ranges)
        assert isinstance(R, increments.IncrementPDFs) and R.names == ["u", "v", "phi"] and np.array_equal(R.r, SEPS)
        assert R.samples == 1 and R.points == 12 * 16 and R.counts["u"].shape == (4, 16) and R.edges["phi"].shape == (4, 17)
        check_against_loop(R, lambda s: {n: (np.abs(structure.increments(f[n], SEPS[s])) if n == "phi" else structure.increments(f[n], SEPS[s])) for n in f}, 16)
    assert (R.below["u"] + R.above["u"]).min() > 0 and np.all(R.below["phi"] == 0)      # the narrow explicit ranges leave points outside


@pytest.mark.parametrize("project", [None, ("u", "v")])
def test_reference_at_vectors_equals_a_loop_of_bin_index(project):
    f = planes()
    R = increments.reference(f, VECTORS, bins=8, project=project)
    assert isinstance(R, increments.IncrementPDFs2d) and np.array_equal(R.vectors, VECTORS) and (R.proj is None) == (project is None)

    def values(s):
        rx, ry = VECTORS[s]
        d = {n: structure.increments2d(f[n], rx, ry) for n in f}
        if project:
            cx, cy = structure.unit_vectors(VECTORS)[s]
            d["u"], d["v"] = cx * d["u"] + cy * d["v"], -cy * d["u"] + cx * d["v"]
        d["phi"] = np.abs(d["phi"])
        return d
    check_against_loop(R, values, 8)
    assert np.allclose(R.length, np.hypot(*np.array(VECTORS).T)) and R.x is R.length
    X = increments.reference(f, [(r, 0) for r in SEPS], bins=8, project=None)
    A = increments.reference(f, SEPS, bins=8)
    for n in f:                                                                         # (r, 0) is the separation r: one definition
        assert np.array_equal(X.counts[n], A.counts[n]) and np.array_equal(X.ranges[n], A.ranges[n])


def test_closure_of_the_result_class():
    f = {k: v for k, v in planes(32, 64, 7).items() if k != "phi"}
    bins = 64
    d = {n: np.array([structure.increments(f[n], r) for r in SEPS]) for n in f}
    top = {n: 1.01 * np.abs(d[n]).max(axis=(1, 2)) for n in f}
    ranges = {n: np.stack([-top[n], top[n]], axis=1) for n in f}          # contain every increment; symmetric: -e is an edge where e is
    R = increments.reference(f, SEPS, bins=bins, ranges=ranges)
    S = structure.reference(f, SEPS)
    for n in f:
        assert np.all(R.below[n] + R.above[n] + R.nan[n] == 0) and np.all(R.counts[n].sum(axis=1) == 32 * 64)
        h = (ranges[n][:, 1] - ranges[n][:, 0]) / bins
        m1, m2, a1 = S.moment(n, 1), S.moment(n, 2), S.abs_moment(n, 1)
        assert np.all(np.abs(R.moment(n, 1) - m1) <= h / 2)
        bound = h * a1 + h * h / 4
        assert np.all(np.abs(R.moment(n, 2) - m2) <= bound)
        assert np.all(np.abs(R.sigma(n) ** 2 - m2) <= bound)
        width = np.diff(R.edges[n], axis=1)
        assert np.all(np.abs((R.density(n) * width).sum(axis=1) - 1) <= 1e-12)
        z, p = R.standardised(n)
        dz = np.diff(R.edges[n], axis=1) / R.sigma(n)[:, None]
        assert np.all(np.abs((p * dz).sum(axis=1) - 1) <= 1e-12)
        second = (p * z * z * dz).sum(axis=1)                                           # of the standardised curve: <c^2> / sigma^2
        assert np.all(np.abs(second - m2 / R.sigma(n) ** 2) <= bound / R.sigma(n) ** 2 + 1e-12)
        assert np.all(np.abs(R.flatness(n) - R.moment(n, 4) / R.moment(n, 2) ** 2) == 0)
        for s in range(len(SEPS)):                                                      # z sigma_r on an edge: the tail is a counted fraction
            e = R.edges[n][s]
            edge = e[np.searchsorted(e, 1.5 * R.sigma(n)[s])]
            want = (np.abs(d[n][s]) > edge).mean()
            assert R.tail(n, edge / R.sigma(n)[s])[s] == want, (n, s)


def test_tail_counts_what_is_out_of_range():
    f = {"u": planes(32, 64, 7)["u"]}
    R = increments.reference(f, [3], bins=8, ranges={"u": (-1.0, 1.0)})
    d = structure.increments(f["u"], 3)
    assert R.below["u"][0] + R.above["u"][0] == (np.abs(d) > 1).sum() > 0
    assert R.tail("u", 1.0 / R.sigma("u")[0])[0] == (np.abs(d) > 1).mean()             # the edge at hi: only the out-of-range points


def test_default_ranges():
    f = planes()
    R = increments.reference(f, SEPS, bins=8, width=5.0)
    for n in ("u", "v"):
        s2 = np.array([(structure.increments(f[n], r) ** 2).mean() for r in SEPS])
        assert np.array_equal(R.ranges[n][:, 1], 5.0 * np.sqrt(s2)) and np.array_equal(R.ranges[n][:, 0], -R.ranges[n][:, 1])
    s2 = np.array([(np.abs(structure.increments(f["phi"], r)) ** 2).mean() for r in SEPS])
    assert np.all(R.ranges["phi"][:, 0] == 0) and np.array_equal(R.ranges["phi"][:, 1], 5.0 * np.sqrt(s2))
    const = {"u": np.full((4, 8), 2.5), "phi": np.full((4, 8), 1 + 2j)}
    Z = increments.reference(const, [1, 3], bins=8)
    assert np.array_equal(Z.ranges["u"], [[-1, 1]] * 2) and np.array_equal(Z.ranges["phi"], [[0, 1]] * 2)
    assert np.all(Z.counts["u"][:, 4] == 32) and np.all(Z.counts["phi"][:, 0] == 32)      # the bin that holds 0; bin 0 of |d phi|
    bad = {"u": np.full((4, 8), np.nan)}
    N = increments.reference(bad, [1], bins=8)
    assert np.array_equal(N.ranges["u"], [[-1, 1]]) and N.nan["u"][0] == 32 and N.counts["u"].sum() == 0
    one = np.zeros((4, 8))
    one[1, 2] = np.nan                                                                  # one NaN: the two increments that touch it
    E = increments.reference({"u": one}, [1], bins=8, ranges={"u": (-1, 1)})
    assert E.nan["u"][0] == 2 and E.counts["u"][0, 4] == 30
    sums = np.array([[[0.0, 4.0], [0.0, np.inf]], [[0.0, 0.0], [0.0, np.nan]]])
    A = increments.auto_ranges(["u", "phi"], sums, 4, 8.0)
    assert np.array_equal(A["u"], [[-8, 8], [-1, 1]]) and np.array_equal(A["phi"], [[0, 1], [0, 1]])


def test_value_errors_need_no_device():
    k = fake()
    C = lambda **kw: increments._Call(k, kw.pop("names", ("u",)), kw.pop("separations", [1, 2]), None, None, kw.pop("bins", 16), kw.pop("ranges", None),
                                      kw.pop("width", 8.0), False, "increments.pdfs")
    assert C(names=("u", "q_psi", "phi")).names == ["u", "q_psi", "phi"]
    for bins in (0, increments.MAX_BINS + 1, 2.5, -1):
        with pytest.raises(ValueError, match="bins"):
            C(bins=bins)
    assert increments.MAX_BINS == _lib.IPDF_MAX_BINS == pdfs.MAX_BINS
    for r in ({"u": (1.0, 1.0)}, {"u": (2.0, 1.0)}, {"u": (0.0, np.inf)}, {"u": (np.nan, 1.0)}, {"u": np.zeros((3, 2))}, {"u": (1, 2, 3)},
              {"u": np.array([[-1, 1], [1, 1.0]])}, {"v": (-1, 1)}):
        with pytest.raises(ValueError, match="range"):
            C(ranges=r)
    assert np.array_equal(C(ranges={"u": (-1, 2)}).given["u"], [[-1, 2], [-1, 2]])
    for w in (0, -1, np.nan):
        with pytest.raises(ValueError, match="width"):
            C(width=w)
    with pytest.raises(ValueError, match="three real names"):                            # structure's own checks, reused
        C(names=("u", "v", "q", "q_psi"))
    with pytest.raises(ValueError, match="three real names"):
        C(names=("u", "v", "q", "phi"))
    with pytest.raises(ValueError, match="separations"):
        C(separations=[0, 1])
    with pytest.raises(ValueError, match="valid names"):
        C(names=("nope",))
    with pytest.raises(NotImplementedError, match="slab"):
        increments._Call(fake(any_size=False), ("u",), [1], None, None, 16, None, 8.0, False, "increments.pdfs")
    with pytest.raises(NotImplementedError, match="QGModel"):
        increments._Call(fake("qg", any_size=False, _ctx=_lib.Context.__new__(_lib.Context)), ("u",), [1], None, None, 16, None, 8.0, False, "increments.pdfs")
    D = lambda **kw: increments._Call(k, kw.pop("names", ("u", "v")), None, kw.pop("vectors", [(1, 0), (0, 2)]), kw.pop("project", ("u", "v")), 16,
                                      kw.pop("ranges", None), 8.0, True, "increments.pdfs2d")
    assert D().project == ("u", "v") and D(names=("u", "q")).project is None and D().proj.shape == (2, 2)
    with pytest.raises(ValueError, match="listed twice"):
        D(vectors=[(1, 2), (1, 2)])
    with pytest.raises(ValueError, match="vectors"):
        D(vectors=[(0, 0)])
    with pytest.raises(ValueError, match="project"):
        D(names=("u", "phi"), project=("u", "phi"))
    with pytest.raises(ValueError, match="range"):
        D(ranges={"u": np.zeros((3, 2))})
    with pytest.raises(ValueError, match="project"):
        increments.reference(planes(), SEPS, project=("u", "v"))
    with pytest.raises(ValueError, match="complex"):
        increments.reference({"phi": np.zeros((4, 4))}, [1])


def test_along_and_isotropic():
    f = planes()
    vec = [(0, 1), (3, 0), (0, 3), (1, 0), (2, 2), (-2, 2)]
    rng = {"u": (-4.0, 4.0), "phi": (0.0, 6.0)}
    R = increments.reference({"u": f["u"], "phi": f["phi"]}, vec, bins=8, ranges=rng)
    Y = R.along("y")
    assert isinstance(Y, increments.IncrementPDFs) and np.array_equal(Y.r, [1, 3])
    for n in ("u", "phi"):
        assert np.array_equal(Y.counts[n], R.counts[n][[0, 2]]) and np.array_equal(Y.edges[n], R.edges[n][[0, 2]]) and np.array_equal(Y.nan[n], R.nan[n][[0, 2]])
    X = R.along("x")
    assert np.array_equal(X.r, [1, 3]) and np.array_equal(X.counts["u"], R.counts["u"][[3, 1]])
    A = increments.reference({"u": f["u"], "phi": f["phi"]}, [1, 3], bins=8, ranges=rng)
    assert np.array_equal(X.counts["u"], A.counts["u"]) and np.array_equal(X.counts["phi"], A.counts["phi"])
    with pytest.raises(ValueError, match="direction"):
        R.along("z")
    radius, counts, nvec = R.isotropic("u")
    assert np.allclose(radius, [1, np.hypot(2, 2), 3]) and np.array_equal(nvec, [2, 2, 2]) and counts.shape == (3, 11)
    assert np.array_equal(counts[0, :8], R.counts["u"][0] + R.counts["u"][3]) and np.all(counts.sum(axis=1) == 2 * 12 * 16)
    assert np.array_equal(counts[1, 8], R.below["u"][4] + R.below["u"][5])
    auto = increments.reference({"u": f["u"]}, vec, bins=8)
    with pytest.raises(ValueError, match="equal edges"):
        auto.isotropic("u")
    with pytest.raises(ValueError, match="no name"):
        R.isotropic("v")


def test_the_header_declares_the_entry_points():
    protos, consts, _ = _abi.read(open(_lib.HEADER).read())
    names = [p[0] for p in protos]
    for fn in ("nq_increment_range", "nq_increment_range2", "nq_increment_hist", "nq_increment_hist2", "nq_increment_hist_read", "nq_any_increment_hist"):
        assert fn in names
    assert consts["NQ_IPDF_MAX_BINS"] == consts["NQ_PDF_MAX_BINS"] == 1024
    table = consts["NQ_SF2_MAX_VECS"] * consts["NQ_SF_MAX_FIELDS"] * (consts["NQ_IPDF_MAX_BINS"] + 3) * 8
    assert table < consts["NQ_IPDF_DEVICE_BYTES"] < table + (1 << 17)
