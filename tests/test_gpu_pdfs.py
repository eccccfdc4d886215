"""PDFs and joint PDFs of the physical fields, binned on the device (niwqg_amd/pdfs.py, nq_field_hist, nq_any_hist): the
engine's counts equal the numpy restatement of the bin rule exactly; on models the counts close on nx^2, agree with the
restatement applied to the fields the model hands out (up to the points within 1e-11 of an edge, which the test counts),
with the real reference's fields, and with the tick's own sums within bounds derived from the bin width; the joint table's
marginals are the 1-D counts; the Accumulator adds states exactly; the call leaves the run alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs, U0
from test_gpu_spectra import make, steps, CASES, ATOMIC, LEFTOVERS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULLP = ctypes.POINTER(ctypes.c_ulonglong)


def pd():
    from niwqg_amd import pdfs
    return pdfs


def restated(x, lo, hi, bins):
    """[below, counts..., above, nan] of the numpy restatement"""
    return np.bincount(pd().bin_index(np.ravel(x), lo, hi, bins) + 1, minlength=bins + 3)


def vector(h, n):
    return np.concatenate([[h.below[n]], h.counts[n], [h.above[n]], [h.nan[n]]])


def near_edges(x, edges, delta):
    x = np.ravel(x)
    i = np.clip(np.searchsorted(edges, x), 1, len(edges) - 1)
    return int((np.minimum(np.abs(x - edges[i - 1]), np.abs(x - edges[i])) <= delta).sum())


def host_field(m, n):
    if n == "phi2":
        p = m.phi
        return p.real * p.real + p.imag * p.imag
    return np.array(getattr(m, n))


# ---- 1. engine level: exact ---------------------------------------------------------------------------------------------------
def cplx(x, y):
    """x + i y without arithmetic (1j * inf would put a NaN into the real part)"""
    z = np.empty((1, len(x)), np.complex128)
    z.real, z.imag = x, y
    return z


def engine_data(n, lo, hi, bins, seed):
    rng = np.random.default_rng(seed)
    e = np.linspace(lo, hi, bins + 1)
    special = np.concatenate([[lo, hi, np.nan, np.inf, -np.inf, -0.0, 0.0, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)], e])
    x = rng.standard_normal(n) * 0.4 * (hi - lo) + 0.5 * (lo + hi)
    k = min(n, len(special))
    x[rng.permutation(n)[:k]] = special[:k]
    return x


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 2 ** 20 + 3])
def test_engine_counts_equal_the_restatement_exactly(n):
    from niwqg_amd._anysize import Engine
    eng = Engine(0)
    L = eng.L
    for lo, hi, bins in ((-1.0, 1.0, 64), (-0.3, 0.1, 10), (-2.5, 7.0, 1024), (0.0, 1.0, 1)):
        x = engine_data(n, lo, hi, bins, n + bins)
        y = engine_data(n, lo, hi, bins, n + bins + 1)
        pl = eng.plane(cplx(x, y))
        out = np.zeros(bins + 3, np.uint64)
        eng.chk(L.nq_any_hist(eng.h, ctypes.c_void_p(pl.ptr), n, 0, lo, hi, bins, out.ctypes.data_as(ULLP)), "nq_any_hist")
        ref = restated(x, lo, hi, bins)
        assert np.array_equal(out[:bins], ref[1:bins + 1]) and (out[bins], out[bins + 1], out[bins + 2]) == (ref[0], ref[bins + 1], ref[bins + 2])
        assert out.sum() == n
        # what = 1: |a|^2 of exactly representable products (no rounding, fma or not)
        xi = np.round(x[np.isfinite(x)] * 8)
        yi = np.arange(len(xi)) % 5.0
        if len(xi):
            p2 = eng.plane(cplx(xi, yi))
            o2 = np.zeros(bins + 3, np.uint64)
            eng.chk(L.nq_any_hist(eng.h, ctypes.c_void_p(p2.ptr), len(xi), 1, lo, hi + 30.0, bins, o2.ctypes.data_as(ULLP)), "nq_any_hist")
            r2 = restated(xi * xi + yi * yi, lo, hi + 30.0, bins)
            assert np.array_equal(o2, np.concatenate([r2[1:bins + 1], [r2[0]], r2[bins + 1:]]))
        # the joint form: Re(a) against Im-free second plane
        jb = min(bins, 128)
        pb = eng.plane(cplx(y, np.zeros(n)))
        lo2, hi2 = np.array([lo, lo - 0.25]), np.array([hi, hi + 0.5])
        oj = np.zeros(jb * jb + 1, np.uint64)
        eng.chk(L.nq_any_hist2(eng.h, ctypes.c_void_p(pl.ptr), ctypes.c_void_p(pb.ptr), n, 0, 0, lo2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                               hi2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), jb, oj.ctypes.data_as(ULLP)), "nq_any_hist2")
        ia, ib = pd().bin_index(x, lo2[0], hi2[0], jb), pd().bin_index(y, lo2[1], hi2[1], jb)
        ok = (ia >= 0) & (ia < jb) & (ib >= 0) & (ib < jb)
        refj = np.bincount(ib[ok] * jb + ia[ok], minlength=jb * jb)
        assert np.array_equal(oj[:-1], refj) and oj[-1] == n - ok.sum()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 2 ** 20 + 3])
def test_engine_minmax(n):
    from niwqg_amd._anysize import Engine
    eng = Engine(0)
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    pl = eng.plane((x + 1j * y).reshape(1, n))
    out = np.zeros(2)
    dp = ctypes.POINTER(ctypes.c_double)
    eng.chk(eng.L.nq_any_minmax(eng.h, ctypes.c_void_p(pl.ptr), n, 0, out.ctypes.data_as(dp)), "nq_any_minmax")
    assert out.tobytes() == np.array([x.min(), x.max()]).tobytes()
    xi, yi = np.round(x * 16), np.round(y * 16)                       # |a|^2 without rounding
    pl = eng.plane((xi + 1j * yi).reshape(1, n))
    eng.chk(eng.L.nq_any_minmax(eng.h, ctypes.c_void_p(pl.ptr), n, 1, out.ctypes.data_as(dp)), "nq_any_minmax")
    a2 = xi * xi + yi * yi
    assert out.tobytes() == np.array([a2.min(), a2.max()]).tobytes()
    for bad in (np.nan, np.inf, -np.inf):                 # non-finite data is reported as such, as numpy.min / max report it
        z = x.copy()
        z[(7 * n) // 11] = bad
        pl = eng.plane(cplx(z, np.zeros(n)))
        eng.chk(eng.L.nq_any_minmax(eng.h, ctypes.c_void_p(pl.ptr), n, 0, out.ctypes.data_as(dp)), "nq_any_minmax")
        assert np.array_equal(out, [z.min(), z.max()], equal_nan=True), (bad, out)


# ---- 2, 3, 6: closure, the model's own fields, marginals --------------------------------------------------------------------
def joint_of(names):
    return ("q_psi", "phi2") if "phi2" in names else (("q", "c") if "c" in names else None)


def check_closure(m, h, names, default_ranges):
    M = m.nx * m.nx
    for n in names:
        assert h.below[n] + int(h.counts[n].sum()) + h.above[n] + h.nan[n] == M, n
        assert h.counts[n].dtype == np.int64 and h.edges[n].shape == (len(h.counts[n]) + 1,)
        if default_ranges:
            assert h.below[n] == h.above[n] == h.nan[n] == 0, n
            assert h.counts[n][0] > 0 and h.counts[n][-1] > 0, n
    if h.joint is not None:
        assert int(h.joint.counts.sum()) + h.joint.outside == M


def check_marginals(h, bins, jb):
    """joint_bins divides bins by a power of two: (x - lo) * s doubles exactly, so the coarse bin is the fine one >> k"""
    a, b = h.joint.names
    g = bins // jb
    assert h.joint.outside == 0
    assert np.array_equal(h.joint.counts.sum(axis=0), h.counts[a].reshape(jb, g).sum(axis=1))
    assert np.array_equal(h.joint.counts.sum(axis=1), h.counts[b].reshape(jb, g).sum(axis=1))


def check_against_fields(m, h, names, bins, drop_extremes):
    """L1 distance of [below, counts, above] to the restatement on the host fields <= 2 n_near, n_near <= 8 or the case is badly posed"""
    for n in names:
        x = host_field(m, n)
        e = h.edges[n]
        near = near_edges(x, e, 1e-11 * (e[-1] - e[0]))
        assert near <= 8, "badly posed: %d points of %s within 1e-11 of an edge" % (near, n)
        if not drop_extremes:
            assert near >= 2                       # the field's own minimum and maximum sit on the outer edges
        ref = restated(x, e[0], e[-1], bins)
        l1 = int(np.abs(vector(h, n)[:-1] - ref[:-1]).sum())
        print("%s: n_near %d, L1 %d" % (n, near, l1))
        assert l1 <= 2 * near, (n, l1, near)
        assert h.nan[n] == ref[-1] == 0


def widened(m, names):
    out = {}
    for n in names:
        x = host_field(m, n)
        span = x.max() - x.min()
        out[n] = (x.min() - 0.01 * span, x.max() + 0.01 * span)
    return out


def model_checks(m, kind, with_fields):
    P = pd()
    names = P.available(m)
    assert names == {"qg": ["q"], "qgc": ["q", "c"]}.get(kind, ["q", "q_psi", "phi2"])
    bins, jb = 256, 64
    for nsteps in (0, 2, 6):
        steps(m, nsteps)
        h = P.field_pdfs(m, bins=bins, joint=joint_of(names), joint_bins=jb)
        check_closure(m, h, names, True)
        if h.joint is not None:
            check_marginals(h, bins, jb)
        if with_fields:
            check_against_fields(m, h, names, bins, False)
            r = widened(m, names)
            h2 = P.field_pdfs(m, bins=bins, ranges=r, joint=joint_of(names), joint_bins=jb)
            check_closure(m, h2, names, False)
            assert all(h2.below[n] == h2.above[n] == 0 for n in names)
            check_against_fields(m, h2, names, bins, True)
    # two calls on one state are identical; a subset of the names and another bin count give the same field's counts regrouped
    h3 = P.field_pdfs(m, bins=bins, joint=joint_of(names), joint_bins=jb)
    assert all(np.array_equal(h.counts[n], h3.counts[n]) for n in names)
    assert h.joint is None or np.array_equal(h.joint.counts, h3.joint.counts)
    one = P.field_pdfs(m, names=[names[-1]], bins=bins // 4, ranges={names[-1]: (h.edges[names[-1]][0], h.edges[names[-1]][-1])})
    assert np.array_equal(one.counts[names[-1]], h.counts[names[-1]].reshape(-1, 4).sum(axis=1))


@pytest.mark.parametrize("nx", [64, 128, 512])
@pytest.mark.parametrize("kind,mask", CASES)
def test_closure_fields_and_marginals(kind, mask, nx):
    model_checks(make(kind, nx, mask), kind, with_fields=(nx == 128))


@pytest.mark.parametrize("nx", [96, 192])
@pytest.mark.parametrize("kind", ["coupled", "qgc"])
def test_any_size_closure_fields_and_marginals(kind, nx):
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    model_checks(m, kind, with_fields=True)
    check_accumulator(m, kind)


# ---- 4. the real reference ------------------------------------------------------------------------------------------------
def check_golden(m, q_ref, phi_ref):
    P = pd()
    a_ref = np.abs(phi_ref) ** 2
    r = {}
    for n, x in (("q", q_ref), ("phi2", a_ref)):
        span = x.max() - x.min()
        r[n] = (x.min() - 0.01 * span, x.max() + 0.01 * span)
    for bins in (64, 256):
        h = P.field_pdfs(m, names=["q", "phi2"], bins=bins, ranges=r, joint=("q", "phi2"), joint_bins=64)
        for n, x in (("q", q_ref), ("phi2", a_ref)):
            near = near_edges(x, h.edges[n], 1e-9 * (r[n][1] - r[n][0]))
            ref = restated(x, r[n][0], r[n][1], bins)
            l1 = int(np.abs(vector(h, n) - ref).sum())
            print("golden %s, %d bins: n_near %d, L1 %d" % (n, bins, near, l1))
            assert l1 <= 2 * near, (n, bins, l1, near)
        ia, ib = P.bin_index(q_ref.ravel(), r["q"][0], r["q"][1], 64), P.bin_index(a_ref.ravel(), r["phi2"][0], r["phi2"][1], 64)
        near = near_edges(q_ref, h.joint.edges_a, 1e-9 * (r["q"][1] - r["q"][0])) + near_edges(a_ref, h.joint.edges_b, 1e-9 * (r["phi2"][1] - r["phi2"][0]))
        refj = np.bincount(ib * 64 + ia, minlength=64 * 64).reshape(64, 64)
        assert int(np.abs(h.joint.counts - refj).sum()) <= 2 * near and h.joint.outside == 0


def test_against_the_real_reference_128():
    import niwqg_amd
    g = np.load(os.path.join(GOLDEN, "g2_coupled_128_filter.npz"))
    m = niwqg_amd.CoupledModel.Model(**notebook_kwargs(128, True))
    m.set_q(g["q0"])
    m.set_phi(g["phi0"])
    steps(m, 100)
    for bins in (64, 256):          # the condition of the comparison, on the golden alone
        for x in (g["q_100"], np.abs(g["phi_100"]) ** 2):
            span = x.max() - x.min()
            assert near_edges(x, np.linspace(x.min() - 0.01 * span, x.max() + 0.01 * span, bins + 1), 1e-9 * 1.02 * span) == 0
    check_golden(m, g["q_100"], g["phi_100"])


def test_against_the_real_reference_any_size_192():
    import niwqg_amd
    g = np.load(os.path.join(GOLDEN, "g17_non_power_of_two.npz"))
    m = niwqg_amd.CoupledModel.Model(**notebook_kwargs(192, True))
    m.set_q(g["c192_q0"])
    m.set_phi((np.ones((192, 192)) + 1j) * (2 * U0) / np.sqrt(2))
    steps(m, 100)
    check_golden(m, g["c192_s100_q"], g["c192_s100_phi"])


# ---- 5. against the tick: no shared restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "filter"), ("ybj", "none")])
def test_against_the_tick(kind, mask):
    m = make(kind, 128, mask)
    steps(m, 6)
    s = m._ctx.diagnostic_sums()
    h = pd().field_pdfs(m, bins=1024)
    M = float(m.nx * m.nx)
    abar = s[0] / (M * M)

    def cw(n):
        e = h.edges[n]
        return 0.5 * (e[:-1] + e[1:]), (e[-1] - e[0]) / 1024, h.counts[n].astype(np.float64), max(abs(e[0]), abs(e[-1]))

    c, w, n, mx = cw("q_psi")
    assert abs((n * c).sum() / M - s[15]) <= w / 2
    assert abs((n * c * c).sum() - s[17]) <= M * (w * mx + w * w / 4)
    c, w, n, mx = cw("q")
    assert abs((n * c * c).sum() - s[16]) <= M * (w * mx + w * w / 4)
    c, w, n, _ = cw("phi2")
    mx = max(abs(h.edges["phi2"][0] - abar), abs(h.edges["phi2"][-1] - abar))
    assert abs((n * (c - abar) ** 2).sum() - s[20]) <= M * (w * mx + w * w / 4)


# ---- 6. the Accumulator ----------------------------------------------------------------------------------------------------------
def test_accumulator_equals_the_sum_of_single_calls():
    P = pd()
    for kind in ("coupled", "qgc"):
        a, b = make(kind, 128, "filter"), make(kind, 128, "filter")
        names = P.available(a)
        r = {n: (lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo)) for n, (lo, hi) in widened(a, names).items()}
        j = joint_of(names)
        acc = P.Accumulator(a, ranges=r, bins=128, joint=j, joint_bins=32)
        tot, totj, outside = {n: np.zeros(131, np.int64) for n in names}, np.zeros((32, 32), np.int64), 0
        for k in range(3):
            steps(a, 2 * (k + 1))
            steps(b, 2 * (k + 1))
            acc.add()
            h = P.field_pdfs(b, bins=128, ranges=r, joint=j, joint_bins=32)
            for n in names:
                tot[n] += vector(h, n)
            totj += h.joint.counts
            outside += h.joint.outside
        res = acc.result()
        for n in names:
            assert np.array_equal(vector(res, n), tot[n]), n
            assert int(vector(res, n).sum()) == 3 * 128 * 128
        assert np.array_equal(res.joint.counts, totj) and res.joint.outside == outside
        acc.reset()
        with pytest.raises(RuntimeError):
            acc.result()
        acc.add()
        one = acc.result()
        assert all(np.array_equal(vector(one, n), vector(h, n)) for n in names)
        # a field_pdfs call on the same model takes the context's tables over: the next add() refuses to mix counts
        P.field_pdfs(a, bins=16)
        with pytest.raises(RuntimeError, match="reset"):
            acc.add()


def check_accumulator(m, kind):
    """the any-size form: the same identity on one model (its counts are summed on the host, so field_pdfs may run in between)"""
    P = pd()
    names = P.available(m)
    r = {n: (lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo)) for n, (lo, hi) in widened(m, names).items()}
    j = joint_of(names)
    acc = P.Accumulator(m, ranges=r, bins=128, joint=j, joint_bins=32)
    tot, totj = {n: np.zeros(131, np.int64) for n in names}, np.zeros((32, 32), np.int64)
    for k in range(3):
        steps(m, m.tc + 1)
        acc.add()
        h = P.field_pdfs(m, bins=128, ranges=r, joint=j, joint_bins=32)
        for n in names:
            tot[n] += vector(h, n)
        totj += h.joint.counts
    res = acc.result()
    assert all(np.array_equal(vector(res, n), tot[n]) for n in names) and np.array_equal(res.joint.counts, totj)
    acc.reset()
    acc.add()
    assert all(np.array_equal(vector(acc.result(), n), vector(h, n)) for n in names)


# ---- 7. leaves the run alone ----------------------------------------------------------------------------------------------------
def _run(kind, call, mask):
    from niwqg_amd.spectra import isotropic_spectra
    m = make(kind, 64, mask, tdiags=3)
    m.twrite = 5
    names = pd().available(m)
    qs = []
    while m.tc < 30:
        m._step_forward()
        if call:
            pd().field_pdfs(m, joint=joint_of(names))
        qs.append(np.array(m.q))
    out = {"q": np.array(qs), "qh": np.array(m.qh), "ph": np.array(m.ph)}
    out.update({"diag:" + n: np.array(d['value']) for n, d in m.diagnostics.items() if 'value' in d})
    if kind != "qgc":
        out["phi"] = np.array(m.phi)
        out["phih"] = np.array(m.phih)
    for name in LEFTOVERS[kind]:
        out[name] = np.array(getattr(m, name))
    sp = isotropic_spectra(m)
    out.update({"spec:" + n: v for n, v in sp.values.items()})
    return out


@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "dual"), ("uncoupled", "filter"), ("uncoupled", "dual"),
                                       ("ybj", "filter"), ("qgc", "filter")])
def test_pdfs_leave_the_run_alone(kind, mask):
    """30 steps, ticks every 3, status lines every 5, with and without a field_pdfs call (joint on, default ranges) after every
    step: bit-identical state, leftovers, spectra and diagnostics series; the atomically reduced scalars (test_gpu_spectra.ATOMIC)
    at 1e-12"""
    a, b = _run(kind, False, mask), _run(kind, True, mask)
    assert set(a) == set(b)
    for n in a:
        if n in ATOMIC and not (n in ("diag:ep_phi", "diag:chi_phi") and kind == "coupled"):
            assert np.allclose(a[n], b[n], rtol=1e-12, atol=0), n
        else:
            assert np.array_equal(a[n], b[n], equal_nan=True), n


# ---- 8. sizes and refusals -----------------------------------------------------------------------------------------------------
BIG = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from test_gpu_spectra import make
from niwqg_amd import pdfs
nx = %d
m = make("coupled", nx, "filter")
h = pdfs.field_pdfs(m, bins=512, joint=("q_psi", "phi2"), joint_bins=64)
for n in ("q", "q_psi", "phi2"):
    assert h.below[n] == h.above[n] == h.nan[n] == 0 and int(h.counts[n].sum()) == nx * nx, n
    assert h.counts[n][0] > 0 and h.counts[n][-1] > 0
assert int(h.joint.counts.sum()) == nx * nx and h.joint.outside == 0
assert np.array_equal(h.joint.counts.sum(axis=0), h.counts["q_psi"].reshape(64, 8).sum(axis=1))
assert np.array_equal(h.joint.counts.sum(axis=1), h.counts["phi2"].reshape(64, 8).sum(axis=1))
print("closure ok at", nx)
"""


@pytest.mark.parametrize("nx", [4096, 8192])
def test_closure_at_size(nx, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "big.py"
    script.write_text(BIG % (root, os.path.join(root, "tests"), nx))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "closure ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("kind", ["coupled", "qgc"])
def test_device_bytes_grow_by_the_tables_only(kind):
    from niwqg_amd import _lib
    m = make(kind, 1024, "filter")
    names = pd().available(m)
    b0 = m._ctx.device_bytes()
    pd().field_pdfs(m, joint=joint_of(names))
    b1 = m._ctx.device_bytes()
    assert b1 - b0 == _lib.PDF_DEVICE_BYTES == (3 * 1027 + 128 * 128 + 1) * 8 + 6 * 8192 * 8
    assert _lib.PDF_DEVICE_BYTES < 8 * 1024 * 1024 // 8            # far less than a plane
    pd().field_pdfs(m, bins=1024, joint=joint_of(names), joint_bins=128)
    assert m._ctx.device_bytes() == b1


def test_refusals():
    m = make("coupled", 64, "filter")
    with pytest.raises(ValueError, match="1 to 1024"):
        pd().field_pdfs(m, bins=2048)
    with pytest.raises(ValueError, match="q, q_psi, phi2"):
        pd().field_pdfs(m, names=["zeta"])
    with pytest.raises(ValueError, match="valid names"):
        pd().field_pdfs(make("qg", 64, "filter"), names=["c"])
    sl = make("coupled", 128, "filter", slab=2)
    with pytest.raises(NotImplementedError):
        pd().field_pdfs(sl)
    # the library refuses on its own, too: out-of-range bins, a slab context
    c = (ctypes.c_int * 1)(0)
    lo, hi = np.zeros(1), np.ones(1)
    dp = ctypes.POINTER(ctypes.c_double)
    L = m._ctx.L
    assert L.nq_field_hist(m._ctx.h, 1, c, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 2048, -1, -1, 0, 0) == -1
    assert b"1 to 1024" in L.nq_last_error(m._ctx.h)
    assert L.nq_field_hist(m._ctx.h, 1, c, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 16, -1, -1, 0, 1) == -1     # nothing to add to
    r0 = sl._ctx.sim.ranks[0]
    mm = np.zeros(2)
    assert r0.L.nq_field_hist(r0.h, 1, c, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), 16, -1, -1, 0, 0) == -4
    assert r0.L.nq_field_minmax(r0.h, 1, c, mm.ctypes.data_as(dp)) == -4
    assert r0.L.nq_field_hist_read(r0.h, np.zeros(19, np.uint64).ctypes.data_as(ULLP)) == -4
    import niwqg_amd
    fresh = niwqg_amd.CoupledModel.Model(**notebook_kwargs(64, True))
    with pytest.raises(RuntimeError, match="set_phi"):
        pd().field_pdfs(fresh)


def test_non_finite_fields():
    m = make("coupled", 64, "filter")
    q = np.array(m.q)
    q[3, 5] = np.nan
    q[7, 9] = np.inf
    m.set_q(q)                              # the spectrum of such a field is NaN everywhere: every value of q is NaN
    with pytest.raises(ValueError, match="'q'"):
        pd().field_pdfs(m, names=["q"])
    h = pd().field_pdfs(m, names=["q", "phi2"], ranges={"q": (-1.0, 1.0)})
    assert h.nan["q"] == 64 * 64 and h.counts["q"].sum() == 0
    assert h.nan["phi2"] == 0 and h.counts["phi2"].sum() == 64 * 64
