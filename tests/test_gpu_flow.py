"""Velocity, strain, Okubo-Weiss and wave-gradient fields in the PDFs and the averages (niwqg_amd/flow.py, csrc/nq_flow.hpp;
DESIGN.md section 5m): the device values equal the numpy restatement ``flow.reference`` to the standing 1e-12 of two routes to
one quantity, the strain components equal the textbook spectral forms, the PDFs close, agree with the restatement and leave the
old names' tables alone, the averages in the step are the sequential sums of the per-step values, nothing disturbs the run, the
any-size path agrees, and the models without flow fields refuse.

Grids: 64 (eight rows per workgroup), 128 (four), 512 (one row, one wave), 1024 (two waves per row: the plan's LDS outgrows the
default tables); 256, 2048, 4096 and 8192, the two-pass tiles at 64 ... 512 and another column split at 1024 are in
tests/test_gpu_plan_ladder_analysis.py and the children of tests/test_gpu_plan_ladder.py, through ``check_values`` and
``check_pdf_calls`` of this module.  States: broadband q and phi with a white part, so the Nyquist row and column carry energy."""
import ctypes
import types

import numpy as np
import pytest

from test_oracle_golden import notebook_kwargs, K0, U0

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MASKS = {"filter": dict(use_filter=True), "none": dict(use_filter=False)}
KINDS = ("coupled", "uncoupled", "ybj")
SIZES = (64, 128, 512, 1024)
TRIPLES = (("u", "v", "sn"), ("ss", "strain2", "ow"), ("gradphi2",))


def make(kind, nx, mask="none", seed=0, bandlimit=False):
    import niwqg_amd
    kw = notebook_kwargs(nx, False)
    kw.update(MASKS[mask])
    if kind == "qg":
        for k in ("m", "N", "f", "nu4w", "nuw", "muw"):
            kw.pop(k)
        kw.update(mu=2e-8, nu=0.0)
        m = niwqg_amd.QGModel.Model(**kw)
    else:
        kw.update(nu4w=3e9 * (128.0 / nx) ** 4, muw=1e-7, mu=2e-8)
        m = {"coupled": niwqg_amd.CoupledModel, "uncoupled": niwqg_amd.UnCoupledModel, "ybj": niwqg_amd.YBJModel}[kind].Model(**kw)
    rng = np.random.default_rng(seed + nx)
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    kap = np.sqrt(n[None, :] ** 2.0 + n[:, None] ** 2.0)

    def noise(cplx):
        z = rng.standard_normal((nx, nx)) + (1j * rng.standard_normal((nx, nx)) if cplx else 0)
        zh = np.fft.fft2(z)
        w = (kap <= nx // 4) * np.exp(-(kap / 8.0) ** 2) if bandlimit else np.exp(-(kap / 8.0) ** 2) + 0.05     # + white: Nyquist lines
        z = np.fft.ifft2(zh * w)
        z = z if cplx else z.real
        return z - z.mean()
    q = noise(False)
    m.set_q(U0 * K0 * q / q.std())
    if kind != "qg":
        p = noise(True)
        m.set_phi(0.2 * (1 + 0.5j) / np.sqrt(2) + 0.05 * p / np.abs(p).std())
    return m


def advance(m, n, batched=False):
    if batched and not getattr(m, "_any_size", False):
        m._ctx.step(n)
        m._after_steps()
    else:
        for _ in range(n):
            m._step_forward()


def device_values(m, names):
    """{name: plane} of one sample of the averages on zeroed sums (0 + x = x exactly)"""
    from niwqg_amd import averages
    out = {}
    names = list(names)
    for i in range(0, len(names), 3):
        A = averages.attach(m, names[i:i + 3], every=0)
        A.sample()
        R = A.result()
        assert R.n == 1
        out.update({n: R.mean(n) for n in names[i:i + 3]})
        A.detach()
    return out


def check_values(m, names, tag, ref=None):
    from niwqg_amd import flow
    ref = flow.reference(m, names) if ref is None else ref
    got = device_values(m, names)
    for n in names:
        err, top = np.abs(got[n] - ref[n]).max(), np.abs(ref[n]).max()
        print("%s %s: max |device - reference| / max |field| = %.3g" % (tag, n, err / top))
        assert top > 0 and err <= 1e-12 * top, (tag, n, err, top)


# ---- 2. values ---------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(k, nx, "none") for k in KINDS for nx in SIZES] + [("coupled", nx, "filter") for nx in SIZES]


@pytest.mark.parametrize("kind, nx, mask", VALUE_CASES)
def test_device_values_equal_the_reference(kind, nx, mask):
    from niwqg_amd import flow
    m = make(kind, nx, mask)
    assert flow.available(m) == list(flow.NAMES)
    check_values(m, flow.NAMES, "%s %d %s set" % (kind, nx, mask))
    advance(m, 3, batched=True)                       # the rows are now the step's own inversion's
    check_values(m, flow.NAMES, "%s %d %s 3 steps" % (kind, nx, mask))


# ---- 3. the strain components against their textbook forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx", SIZES)
def test_strain_identity(nx):
    m = make("coupled", nx, "filter", bandlimit=True)
    advance(m, 2, batched=True)
    ph = np.array(m.ph)
    k, l = np.array(m.k), np.array(m.l)
    want = {"ss": np.fft.ifft2((l * l - k * k) * ph).real, "sn": 2 * np.fft.ifft2(k * l * ph).real}
    got = device_values(m, ("ss", "sn"))
    for n in want:
        err, top = np.abs(got[n] - want[n]).max(), np.abs(want[n]).max()
        print("%d %s: %.3g" % (nx, n, err / top))
        assert err <= 1e-10 * top, (n, err, top)


# ---- 4. PDFs -------------------------------------------------------------------------------------------------------------------------
def restated(x, lo, hi, bins):
    from niwqg_amd import pdfs
    return np.bincount(pdfs.bin_index(np.ravel(x), lo, hi, bins) + 1, minlength=bins + 3)


def vector(h, n):
    return np.concatenate([[h.below[n]], h.counts[n], [h.above[n]], [h.nan[n]]])


def near_edges(x, edges, delta):
    x = np.ravel(x)
    i = np.clip(np.searchsorted(edges, x), 1, len(edges) - 1)
    return int((np.minimum(np.abs(x - edges[i - 1]), np.abs(x - edges[i])) <= delta).sum())


def wide(x):
    lo, hi = float(x.min()), float(x.max())
    return lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo)


def reference_with_old(m, names):
    from niwqg_amd import flow
    ref = flow.reference(m, [n for n in names if n in flow.NAMES])
    for n in names:
        if n == "phi2":
            p = np.array(m.phi)
            ref[n] = p.real * p.real + p.imag * p.imag
        elif n not in ref:
            ref[n] = np.array(getattr(m, n))
    return ref


PDF_CALLS = [(("q_psi", "ow", "gradphi2"), ("ow", "gradphi2")), (("ss", "phi2"), ("ss", "phi2")), (("u", "v", "strain2"), ("v", "u")),
             (("sn",), None)]


@pytest.mark.parametrize("kind, nx, mask", [("coupled", 64, "none"), ("uncoupled", 128, "none"), ("ybj", 512, "none"),
                                            ("coupled", 1024, "none"), ("coupled", 128, "filter")])
def test_pdfs_close_and_equal_the_restatement(kind, nx, mask):
    m = make(kind, nx, mask)
    advance(m, 2, batched=True)
    check_pdf_calls(m, kind, nx)


def check_pdf_calls(m, kind, nx, calls=None):
    """every call of ``calls`` (PDF_CALLS): the counts close, equal the restatement up to the points near an edge, the joint table's
    marginals are the 1-D counts, the default edges are the exact extremes"""
    from niwqg_amd import pdfs
    bins, jb = 96, 24
    for names, joint in (PDF_CALLS if calls is None else calls):
        ref = reference_with_old(m, names)
        ranges = {n: wide(ref[n]) for n in names}
        h = pdfs.field_pdfs(m, names=names, bins=bins, ranges=ranges, joint=joint, joint_bins=bins)
        for n in names:
            assert h.below[n] + int(h.counts[n].sum()) + h.above[n] + h.nan[n] == nx * nx, n
            lo, hi = ranges[n]
            n_near = near_edges(ref[n], h.edges[n], 1e-11 * (hi - lo))
            l1 = int(np.abs(vector(h, n) - restated(ref[n], lo, hi, bins)).sum())
            print("%s %d %s: L1 %d, near an edge %d" % (kind, nx, n, l1, n_near))
            assert n_near <= 8, "badly posed"
            assert l1 <= 2 * n_near, (n, l1, n_near)
        if joint:                                        # marginals at equal bins
            a, b = joint
            assert h.joint.names == (a, b) and h.joint.counts.sum() + h.joint.outside == nx * nx
            assert h.joint.outside == 0
            assert np.array_equal(h.joint.counts.sum(axis=0), h.counts[a]) and np.array_equal(h.joint.counts.sum(axis=1), h.counts[b])
        d = pdfs.field_pdfs(m, names=names, bins=jb)     # default ranges: the exact extremes
        dv = device_values(m, names)
        for n in names:
            top = np.abs(dv[n]).max()                     # the averages' pass: another route to the same extremes
            assert abs(d.edges[n][0] - dv[n].min()) <= 1e-12 * top and abs(d.edges[n][-1] - dv[n].max()) <= 1e-12 * top, n
            assert d.below[n] == d.above[n] == d.nan[n] == 0 and d.counts[n].sum() == nx * nx
            assert d.counts[n][0] > 0 and d.counts[n][-1] > 0
        # the edges are the EXACT extremes of the values the counting pass sees: nothing outside them (above), and one ulp inside
        # them leaves a point out on either side
        inside = {n: (np.nextafter(d.edges[n][0], np.inf), np.nextafter(d.edges[n][-1], -np.inf)) for n in names}
        t = pdfs.field_pdfs(m, names=names, bins=jb, ranges=inside)
        for n in names:
            assert t.below[n] >= 1 and t.above[n] >= 1 and t.nan[n] == 0, n


def test_old_names_tables_are_untouched_by_flow_calls():
    from niwqg_amd import pdfs
    m = make("coupled", 128)
    advance(m, 2)
    kw = dict(names=("q", "q_psi", "phi2"), bins=64, joint=("q_psi", "phi2"), joint_bins=32)
    before = pdfs.field_pdfs(m, **kw)
    pdfs.field_pdfs(m, names=("ow", "q_psi", "gradphi2"), joint=("gradphi2", "ow"))
    after = pdfs.field_pdfs(m, **kw)
    for n in kw["names"]:
        assert np.array_equal(before.counts[n], after.counts[n]) and np.array_equal(before.edges[n], after.edges[n])
    assert np.array_equal(before.joint.counts, after.joint.counts)
    acc = pdfs.Accumulator(m, {"ow": (-1e-6, 1e-6), "phi2": (0.0, 1.0)}, names=("ow", "phi2"), bins=32, joint=("ow", "phi2"), joint_bins=8)
    acc.add()
    advance(m, 1)
    acc.add()
    r = acc.result()
    assert all(r.below[n] + r.counts[n].sum() + r.above[n] + r.nan[n] == 2 * 128 * 128 for n in ("ow", "phi2"))


# ---- 5. averages in the step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("uncoupled", 128), ("coupled", 1024)])
def test_averages_in_the_step(kind, nx):
    from niwqg_amd import averages, flow
    fields, products = ("q_psi", "strain2", "gradphi2", "phi"), (("strain2", "gradphi2"), ("q_psi", "strain2"), ("gradphi2", "gradphi2"))
    nsteps = 12 if nx < 1024 else 4                   # 12 steps at 64 and 128; 1024 repeats the same code on two waves per row: 4 keep it quick
    runs = []
    for batches in ((1,) * nsteps, (nsteps // 4, nsteps - nsteps // 4), (1,) * nsteps):
        m = make(kind, nx)
        A = averages.attach(m, fields, products, every=1)
        sums = {n: np.zeros((nx, nx)) for n in fields[:3]}
        sums.update({"%s*%s" % p: np.zeros((nx, nx)) for p in products})
        tops = {k: 0.0 for k in sums}
        follow = len(runs) == 0                           # the restatement follows the first run step by step
        for b in batches:
            advance(m, b, batched=True)
            if follow:
                vals = reference_with_old(m, fields[:3])
                averages.accumulate(sums, vals)
                for k in sums:
                    x = vals[k] if "*" not in k else vals[k.split("*")[0]] * vals[k.split("*")[1]]
                    tops[k] = max(tops[k], float(np.abs(x).max()))
        R = A.result()
        assert R.n == nsteps
        if follow:
            for k in sums:
                err = np.abs(R.sums[k] - sums[k]).max()
                # first moments: the standing 1e-12 per sample; products: the same on each factor plus the contraction's one
                # rounding per sample (section 5l), 2e-12 + 2^-53 of the largest product, times n samples
                tol = (1e-12 if "*" not in k else 2e-12 + 2 * U) * nsteps * tops[k]
                print("%s %d %s: %.3g of %.3g" % (kind, nx, k, err, tol))
                assert err <= tol, (k, err, tol)
        runs.append({k: R.sums[k].copy() for k in list(sums) + ["phi"]})
        A.detach()
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), ("batched", k)
        assert runs[0][k].tobytes() == runs[2][k].tobytes(), ("rerun", k)


# ---- 6. non-interference -----------------------------------------------------------------------------------------------------------
def test_flow_calls_leave_the_run_alone():
    from niwqg_amd import averages, pdfs
    a, b = make("coupled", 128, "filter"), make("coupled", 128, "filter")
    for m in (a, b):
        pdfs.field_pdfs(m, names=("q",))                  # the PDFs' own buffers exist before the byte count
    b0, c0 = a._ctx.device_bytes(), b._ctx.device_bytes()
    planes = (1 + 1 + 2 + 1) * 8 * 128 * 128             # ow, gradphi2, phi (complex) and one product
    A = averages.attach(a, ("ow", "gradphi2", "phi"), (("ow", "gradphi2"),), every=1)
    assert a._ctx.device_bytes() - b0 == planes
    for _ in range(20):
        advance(a, 1)
        advance(b, 1)
        pdfs.field_pdfs(a, names=("u", "ss", "gradphi2"), joint=("ss", "gradphi2"))
    grown = b._ctx.device_bytes() - c0                    # what stepping itself allocates on first use
    assert a._ctx.device_bytes() - b0 == planes + grown
    for n in ("qh", "phih", "ph"):
        assert np.array(getattr(a, n)).tobytes() == np.array(getattr(b, n)).tobytes(), n
    assert A.result().n == 20
    A.detach()
    assert a._ctx.device_bytes() == b0 + grown


# ---- 7. any-size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [96, 100])
@pytest.mark.parametrize("kind", ["coupled", "qg"])
def test_any_size(kind, nx):
    from niwqg_amd import flow, pdfs
    m = make(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    names = flow.available(m)
    assert names == ([n for n in flow.NAMES if n != "gradphi2"] if kind == "qg" else list(flow.NAMES))
    advance(m, 2)
    d = m._d
    src = types.SimpleNamespace(nx=nx, kk=m.kk, ll=m.ll, ph=d["ph"].get(), q_psi=m._pdf_planes(["q" if kind == "qg" else "q_psi"]).popitem()[1][0].get(),
                                phih=d["phih"].get() if kind != "qg" else None)
    ref = flow.reference(src, names)
    check_values(m, names, "%s %d" % (kind, nx), ref)
    pick = ("u", "ow", "ss")
    ranges = {n: wide(ref[n]) for n in pick}
    h = pdfs.field_pdfs(m, names=pick, bins=48, ranges=ranges, joint=("ow", "ss"), joint_bins=48)
    for n in pick:
        lo, hi = ranges[n]
        assert h.below[n] + int(h.counts[n].sum()) + h.above[n] + h.nan[n] == nx * nx
        n_near = near_edges(ref[n], h.edges[n], 1e-11 * (hi - lo))
        assert n_near <= 8 and int(np.abs(vector(h, n) - restated(ref[n], lo, hi, 48)).sum()) <= 2 * n_near, n
    assert np.array_equal(h.joint.counts.sum(axis=0), h.counts["ow"]) and np.array_equal(h.joint.counts.sum(axis=1), h.counts["ss"])


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import niwqg_amd
    from niwqg_amd import averages, flow, pdfs, _lib
    L = _lib.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    two = np.zeros(2)
    g = make("qg", 64)
    assert flow.available(g) == []
    with pytest.raises(NotImplementedError, match="QGModel"):
        pdfs.field_pdfs(g, names=("ow",))
    with pytest.raises(NotImplementedError, match="QGModel"):
        averages.attach(g, ("q", "u"))
    h = g._ctx.h
    assert L.nq_field_minmax(h, 1, ints(_lib.FLOW_OW), _lib._dptr(two)) == -1 and b"QGModel" in L.nq_last_error(h)
    assert L.nq_field_hist(h, 1, ints(_lib.FLOW_U), _lib._dptr(two[:1]), _lib._dptr(two[1:] + 1), 8, -1, -1, 0, 0) == -1
    assert L.nq_avg_attach(h, 1, ints(_lib.FLOW_SN), 0, None, 1) == -1 and b"QGModel" in L.nq_last_error(h)
    assert L.nq_avg_detach(h) == -4
    k = make("coupled", 64)
    assert L.nq_avg_attach(k._ctx.h, 4, ints(_lib.AVG_Q, _lib.FLOW_U, _lib.FLOW_V, _lib.FLOW_OW), 0, None, 1) == -1     # four real fields
    assert L.nq_field_minmax(k._ctx.h, 1, ints(23), _lib._dptr(two)) == -1                                                # past the last code
    with pytest.raises(ValueError, match="q, q_psi, phi2"):
        pdfs.field_pdfs(k, names=("zeta",))
    s = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        pdfs.field_pdfs(s, names=("ow",))
    with pytest.raises(NotImplementedError, match="slab"):
        averages.attach(s, ("ow",))
    hs = s._ctx.sim.ranks[0].h
    assert L.nq_field_minmax(hs, 1, ints(_lib.FLOW_OW), _lib._dptr(two)) == -4 and len(L.nq_last_error(hs)) > 0
    assert L.nq_avg_attach(hs, 1, ints(_lib.FLOW_OW), 0, None, 1) == -4
