"""Vortex census without a device (niwqg_amd/vortices.py): the numpy specification labels like
scipy.ndimage.label with the two seams united, the fixed-point sums never leave int64 and stay within their stated bound, discs and
ellipses come back with their geometry, every refusal is raised before any library call, and the result class's selections are
those of a hand-made table.  ``patterns`` and ``random_mask`` are shared with tests/test_gpu_vortices.py."""
import math

import numpy as np
import pytest


# ---- the crafted sets ------------------------------------------------------------------------------------------------------------------
def spiral(ny, nx):
    """a rectangular spiral, one pixel wide with one pixel between its arms, wound inwards from (0, 0)"""
    m = np.zeros((ny, nx), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    lo_y, hi_y, lo_x, hi_x = 0, ny - 1, 0, nx - 2           # the last column stays empty: the arms must not meet across the x seam
    hi_y -= 1                                               # nor the last row across the y seam
    turns = 0
    while turns < 2:
        ty, tx = y + dy, x + dx
        ahead2y, ahead2x = y + 2 * dy, x + 2 * dx
        blocked = not (lo_y <= ty <= hi_y and lo_x <= tx <= hi_x) or m[ty, tx] or \
            (lo_y <= ahead2y <= hi_y and lo_x <= ahead2x <= hi_x and m[ahead2y, ahead2x])
        if blocked:
            dy, dx = dx, -dy
            turns += 1
            continue
        turns = 0
        y, x = ty, tx
        m[y, x] = True
    return m


def patterns(ny, nx):
    """{name: (ny, nx) boolean set}"""
    yy, xx = np.mgrid[0:ny, 0:nx]
    z = lambda: np.zeros((ny, nx), bool)
    out = {"empty": z(), "full": np.ones((ny, nx), bool)}
    p = z(); p[0, 0] = True; out["point_first"] = p
    p = z(); p[ny - 1, nx - 1] = True; out["point_last"] = p
    p = z(); p[ny // 3, :] = True; out["row_ring"] = p
    p = z(); p[:, nx // 3] = True; out["column_ring"] = p
    out["diagonal"] = yy == xx
    out["checkerboard"] = (yy + xx) % 2 == 0
    p = z(); p[2:, ::2] = True; p[ny - 1, :] = True; out["comb"] = p
    out["spiral"] = spiral(ny, nx)
    p = z()
    for k in range(ny // 2):
        p[2 * k, nx - 3:] = True
        p[2 * k, :3] = True
        p[2 * k + 1, 2 if k % 2 == 0 else nx - 3] = True
    out["serpentine"] = p
    p = z(); p[5:9, :3] = True; p[5:9, nx - 3:] = True; out["blobs_x_seam"] = p
    c = nx // 2
    p = z(); p[:2, c:c + 3] = True; p[ny - 2:, c:c + 3] = True; out["blobs_y_seam"] = p
    p = z(); p[ny // 2, nx // 8 - 1:nx // 8 + 1] = True
    if nx > 64:
        p[ny // 2 + 2, 63:65] = True
    out["boundary_runs"] = p
    return out


def random_mask(ny, nx, density, seed=0):
    return np.random.default_rng(seed).random((ny, nx)) < density


DENSITIES = (0.3, 0.55, 0.7)


def cases(ny, nx):
    out = dict(patterns(ny, nx))
    out.update({"random_%g" % d: random_mask(ny, nx, d) for d in DENSITIES})
    return out


# ---- 1. the labelling against scipy -----------------------------------------------------------------------------------------------------
def scipy_labels(mask, connectivity):
    """scipy's labels without wrap-around, united across the two seams by a small union-find, renamed to the minimum index"""
    ndimage = pytest.importorskip("scipy.ndimage")
    ny, nx = mask.shape
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int) if connectivity == 8 else None)
    parent = list(range(n + 1))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    steps = (0,) if connectivity == 4 else (-1, 0, 1)
    for y in range(ny):
        for s in steps:
            if mask[y, nx - 1] and mask[(y + s) % ny, 0]:
                unite(lab[y, nx - 1], lab[(y + s) % ny, 0])
    for x in range(nx):
        for s in steps:
            if mask[ny - 1, x] and mask[0, (x + s) % nx]:
                unite(lab[ny - 1, x], lab[0, (x + s) % nx])
    root = np.array([find(i) for i in range(n + 1)])
    lab = root[lab]
    idx = np.arange(ny * nx).reshape(ny, nx)
    smallest = np.full(n + 1, ny * nx)
    np.minimum.at(smallest, lab[mask], idx[mask])
    return np.where(mask, smallest[lab], -1)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("n", [12, 64])
def test_reference_labels_equal_scipy(n, connectivity):
    from niwqg_amd import vortices
    for name, mask in cases(n, n).items():
        want = scipy_labels(mask, connectivity)
        got = vortices.label_plane(mask, connectivity)
        assert np.array_equal(got, want), (name, n, connectivity)
        C = vortices.reference({"a": mask.astype(float)}, "a", "above", 0.5, connectivity)
        assert C.total == C.n == len(np.unique(want[want >= 0])) and C.points_in_set == int(mask.sum()), name
        assert np.array_equal(C.label, np.unique(want[want >= 0])), name
        assert np.array_equal(C.labels >= 0, mask) and np.array_equal(C.label[C.labels[mask]], want[mask]), name
        assert np.array_equal(C.area, np.bincount(C.labels[mask], minlength=C.n)), name


def test_crafted_sets_are_what_they_claim():
    from niwqg_amd import vortices
    n = 64
    P = patterns(n, n)
    count = lambda name, conn: len(np.unique(vortices.label_plane(P[name], conn))) - (0 if P[name].all() else 1)
    assert count("empty", 4) == 0 and count("full", 4) == 1 and count("row_ring", 4) == 1 and count("column_ring", 8) == 1
    assert count("diagonal", 4) == n and count("diagonal", 8) == 1
    assert count("checkerboard", 4) == n * n // 2 and count("checkerboard", 8) == 1
    assert count("comb", 4) == 1 and count("spiral", 4) == 1 and count("spiral", 8) == 1 and P["spiral"].sum() > n * n // 3
    assert count("serpentine", 4) == 1
    assert count("blobs_x_seam", 4) == 1 and count("blobs_y_seam", 4) == 1 and count("boundary_runs", 8) == 1
    wide = patterns(128, 128)["boundary_runs"]                            # the run over x = 63, 64 exists from 128 columns on
    assert wide[66, 63] and wide[66, 64] and wide[64, 15] and wide[64, 16] and wide.sum() == 4


# ---- 2. the fixed-point sums ------------------------------------------------------------------------------------------------------------
def test_fixed_point_scale_is_the_rule():
    from niwqg_amd.vortices import fixed_point_scale
    assert fixed_point_scale(0.0, 4096) == 0 and fixed_point_scale(float("nan"), 64) == 0
    assert fixed_point_scale(1.0, 64 * 64) == 61 - 12 - 1 and fixed_point_scale(0.75, 64 * 64) == 61 - 12
    assert fixed_point_scale(1.0, 96 * 96) == 61 - 14 - 1                  # ceil(log2 9216) = 14
    assert fixed_point_scale(2.0 ** -40, 4096 ** 2) == 61 - 24 + 39


@pytest.mark.parametrize("exponent", [-300, -5, 0, 7, 300])
def test_fixed_point_sums_stay_in_int64_and_within_their_bound(exponent):
    from niwqg_amd import vortices
    n = 64
    rng = np.random.default_rng(exponent + 1000)
    a = rng.standard_normal((n, n)) * 10.0 ** exponent
    a[3, 5] = np.abs(a).max() * 1.999                                      # a lone maximum: the mantissa next to 1
    s = vortices.fixed_point_scale(np.abs(a).max(), n * n)
    terms = np.rint(np.ldexp(a, s))
    limit = 2.0 ** (61 - 12)
    assert np.abs(terms).max() < limit and np.abs(terms).sum() < 2.0 ** 63
    full = np.ones((n, n))
    C = vortices.reference({"w": full, "a": a}, "w", "above", 0.5)
    assert C.n == 1 and C.area[0] == n * n and C.scales["a"] == s
    exact = math.fsum(a.ravel())
    got = C.sum("a")[0]
    bound = n * n * 2.0 ** (-s - 1) + abs(exact) * 2.0 ** -52                # the terms' rounding, then the conversion of the integer
    print("exponent %d: |sum - fsum| = %.3g, bound %.3g" % (exponent, abs(got - exact), bound))
    assert abs(got - exact) <= bound
    blobs = vortices.reference({"a": a}, "a", "abs_above", np.abs(a).mean())
    for r in range(blobs.n):
        pts = blobs.labels == r
        part = math.fsum(a[pts])
        assert abs(blobs.sum("a")[r] - part) <= blobs.area[r] * 2.0 ** (-s - 1) + abs(part) * 2.0 ** -52


def test_planes_of_zeros_and_non_finite_values():
    from niwqg_amd import vortices
    z = np.zeros((12, 12))
    C = vortices.reference({"a": z}, "a", "above", -1.0)
    assert C.scales["a"] == 0 and C.n == 1 and C.table[0, 9] == 0 and C.area[0] == 144
    z[2, 3] = np.nan
    z[4, 4] = np.inf
    C = vortices.reference({"a": z}, "a", "above", -1.0)
    assert C.nonfinite == 2 and C.points_in_set == 143 and C.labels[2, 3] == -1 and C.table[0, 9] == 0
    assert C.crit_max[0] == np.inf and C.crit_min[0] == 0.0


# ---- 3. geometry --------------------------------------------------------------------------------------------------------------------------
def test_a_disc_across_both_seams_is_the_disc_mid_domain():
    from niwqg_amd import vortices
    n, r = 64, 9.3
    yy, xx = np.mgrid[0:n, 0:n]
    disc = ((yy - 32) ** 2 + (xx - 32) ** 2 <= r * r).astype(float)
    mid = vortices.reference({"a": disc}, "a", "above", 0.5)
    seam = vortices.reference({"a": np.roll(disc, (-32, -32), axis=(0, 1))}, "a", "above", 0.5)
    assert mid.n == seam.n == 1 and mid.area[0] == seam.area[0]
    assert mid.x[0] == 32.0 and mid.y[0] == 32.0 and seam.x[0] == 0.0 and seam.y[0] == 0.0
    assert seam.radius[0] == mid.radius[0] and abs(mid.radius[0] - r) < 0.5      # a lattice disc's area is pi r^2 to within its rim
    assert np.allclose(seam.inertia(), mid.inertia(), rtol=0, atol=1e-12)
    a, b, _ = seam.axes()
    assert abs(a[0] - b[0]) < 1e-9 and abs(a[0] - r) < 0.5


def test_an_ellipse_returns_its_axes_and_angle():
    """A pixel is in when its centre is: every point of the rim is displaced by at most half a pixel diagonal, 0.71, so the
    semi-axes of the moments' ellipse lie within 0.71 of (A, B); the major axis of such a shape turns by at most
    atan(0.71 / A) ... the bound used is that angle for the displacement acting at the tip of the major axis."""
    from niwqg_amd import vortices
    n, A, B, theta = 128, 30.0, 12.0, 0.6
    yy, xx = np.mgrid[0:n, 0:n]
    u = (xx - 60.0) * math.cos(theta) + (yy - 70.0) * math.sin(theta)
    v = -(xx - 60.0) * math.sin(theta) + (yy - 70.0) * math.cos(theta)
    e = ((u / A) ** 2 + (v / B) ** 2 <= 1.0).astype(float)
    e = np.roll(e, (50, -70), axis=(0, 1))                                  # across both seams
    C = vortices.reference({"a": e}, "a", "above", 0.5, connectivity=8)
    assert C.n == 1
    a, b, angle = C.axes()
    half_diagonal = math.sqrt(0.5)
    print("ellipse: a = %.3f (%.1f), b = %.3f (%.1f), angle = %.4f (%.2f)" % (a[0], A, b[0], B, angle[0], theta))
    assert abs(a[0] - A) <= half_diagonal and abs(b[0] - B) <= half_diagonal
    assert abs(angle[0] - theta) <= math.atan(half_diagonal / A)
    assert abs(C.x[0] - (60.0 - 70.0) % n) <= half_diagonal and abs(C.y[0] - (70.0 + 50.0) % n) <= half_diagonal


# ---- 4. refusals, before any library call ------------------------------------------------------------------------------------------------
class Untouchable(object):
    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


def stub(kind="coupled", nx=64):
    import niwqg_amd
    from niwqg_amd import _lib
    cls = {"coupled": niwqg_amd.CoupledModel.Model, "qg": niwqg_amd.QGModel.Model}[kind]
    m = cls.__new__(cls)
    m.nx = m.ny = nx
    m.dx = m.dy = 1.0
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.L, ctx.h = Untouchable(), None
    m._ctx = ctx
    if kind == "qg":
        m.passive_scalar = True
    return m


def test_refusals_come_before_any_device_call():
    from niwqg_amd import vortices
    m = stub()
    bad = [dict(criterion="zeta"), dict(sums=("q", "nope")), dict(criterion="phi"), dict(sums=("phi",)), dict(sums=("q", "q")),
           dict(sums=("q", "u", "v")), dict(mode="inside"), dict(units="percent"), dict(threshold=float("nan")), dict(threshold=float("inf")),
           dict(threshold="low"), dict(connectivity=6), dict(capacity=0), dict(capacity=vortices.MAX_CAPACITY + 1), dict(capacity=2.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            vortices.census(m, **kw)
    g = stub("qg")
    with pytest.raises(NotImplementedError, match="QGModel"):
        vortices.census(g, "ow")
    with pytest.raises(ValueError):
        vortices.census(g, "q_psi")
    s = stub()
    s._ctx = object()                                                        # not a single-GPU context
    with pytest.raises(NotImplementedError, match="slab"):
        vortices.census(s)
    with pytest.raises(ValueError):
        vortices.reference({"a": np.zeros((4, 4))}, "b", "above", 0.0)
    with pytest.raises(ValueError):
        vortices.reference({"a": np.zeros((4, 4))}, "a", "above", 0.0, connectivity=5)


def test_available_names():
    from niwqg_amd import vortices
    assert "phi" not in vortices.available(stub()) and {"q", "q_psi", "phi2", "ow"} <= set(vortices.available(stub()))


# ---- 5. the result class on a hand-made table ----------------------------------------------------------------------------------------------
def test_select_share_and_size_distribution():
    from niwqg_amd import vortices
    bits = lambda v: np.array([v]).view(np.int64)[0]
    #        label area sdx sdy sdx2 sdy2 sdxdy  min        max        ow   q_psi<<4  phi2<<2
    rows = [[0,    4,   2,  2,  2,   2,   1,     bits(-2.), bits(-1.), -6,  16 * 3,   4 * 10],
            [9,    1,   0,  0,  0,   0,   0,     bits(-5.), bits(-5.), -5,  -16 * 2,  4 * 1],
            [20,   16,  0,  0,  0,   0,   0,     bits(-3.), bits(-1.), -40, -16 * 8,  4 * 5],
            [33,   2,   1,  0,  1,   0,   0,     bits(-4.), bits(-2.), -6,  0,        4 * 4]]
    lab = np.full((8, 8), -1, np.int32)
    lab[0, 0] = 0; lab[1, 1] = 1; lab[2, 4] = 2; lab[4, 1] = 3; lab[7, 7] = -2
    C = vortices.Census(["ow", "q_psi", "phi2"], "ow", "below", 4, -0.5, [0, 4, 2], rows, 5, 24, 0, (8, 8), 0.5, 0.5,
                        {"ow": -40.0, "q_psi": 1.0, "phi2": 40.0}, lab, 4)
    assert C.n == 4 and C.total == 5 and C.truncated and C.points_in_set == 24
    assert np.array_equal(C.sum("q_psi"), [3.0, -2.0, -8.0, 0.0]) and np.array_equal(C.sum("phi2"), [10.0, 1.0, 5.0, 4.0])
    assert np.array_equal(C.cyclonic, [1, -1, -1, 0]) and np.array_equal(C.crit_min, [-2.0, -5.0, -3.0, -4.0])
    assert np.array_equal(C.mean("phi2"), [2.5, 1.0, 5.0 / 16, 2.0]) and np.array_equal(C.integral("phi2"), np.array([10.0, 1.0, 5.0, 4.0]) * 0.25)
    assert np.array_equal(C.x, [0.25, 0.5, 2.0, 0.75]) and np.array_equal(C.y, [0.25, 0.5, 1.0, 2.0])
    assert C.share("phi2") == 0.5 and C.share("phi2", C.cyclonic < 0) == 6.0 / 40.0 and C.share("phi2", [0, 3]) == 14.0 / 40.0
    A = C.select(C.cyclonic < 0)
    assert A.n == 2 and np.array_equal(A.label, [9, 20]) and A.share("phi2") == 6.0 / 40.0 and A.total == 5 and A.truncated
    assert A.labels[1, 1] == 0 and A.labels[2, 4] == 1 and A.labels[0, 0] == -1 and A.labels[4, 1] == -1 and A.labels[7, 7] == -2 and A.labels[3, 3] == -1
    big = C.select(2)
    assert np.array_equal(big.label, [0, 20, 33]) and np.array_equal(C.select([2]).area, [16])
    assert np.array_equal(C.size_distribution([1, 2, 4, 8, 32]), [1, 1, 1, 1])
    with pytest.raises(ValueError):
        C.sum("u")
    assert np.array_equal(C.info(), [5, 4, 24, 0, 0, 4, 2])
    I = C.inertia()
    assert I.shape == (4, 2, 2) and np.array_equal(I[0], np.array([[0.25, 0.0], [0.0, 0.25]]) * 0.25)
