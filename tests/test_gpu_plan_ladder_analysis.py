"""The analysis features of DESIGN.md sections 5m to 5q on every fused plan, and on fields that vanish (section 6, "features x
plans"): flow names in the PDFs and the averages, time-mean spectra, coarse-grained flux maps, shell-to-shell transfers, co-spectra.

tests/test_gpu_plan_ladder.py walks the ladder for the older features; this module is its sibling for the newer ones, and the
two-pass tiles at 64 ... 512 and NIWQG_AMD_Y_SPLIT are in that module's children (``check_analysis``).  Every check is one the
feature's own test makes at another size, through the same helpers and with the same bound: flow values 1e-12 of the field's maximum,
coarse maps 1e-12 of the product of the factors' maxima (identity 1e-12 (mean |map| + sum |T|)), shell-to-shell rows 1e-10 sum |T|
against numpy and 1e-12 sum |T| for closure and antisymmetry, co-spectra 1e-12 sum_shell |A||B| / M^2 on the resolved shells,
time-mean spectra bit for bit in the first moments.

Grids.  1: the row plans the feature tests skip (256: two rows per workgroup; 2048: four waves per row; 1024 for the shell-to-shell
rows, whose own test stops at 512), states of test_gpu_flow.make (white part: the Nyquist lines carry energy).  2: 4096 (eight
waves per row, the dual-stream step) and 8192 (even/odd rows, one flow value per thread), the ladder's white-noise model after two
steps; host transforms only where stated.  3: 64 and 1024 with a field that is exactly zero or uniform."""
import time

import numpy as np
import pytest

from test_gpu_plan_ladder import big, rough_model, check_averages, check_coarse, check_s2s_rows, check_qgc_cospectra      # noqa: F401 (big: a fixture)
from test_gpu_spectra import steps
import test_gpu_flow as flow_t
import test_gpu_coarse as coarse_t
import test_gpu_shelltoshell as s2s_t
import test_gpu_cospectra as cospec_t
import test_gpu_timespectra as tspec_t
from test_gpu_flow import make, advance, device_values, check_values

pytestmark = pytest.mark.gpu


# ---- 1. the row plans the feature tests skip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", [("coupled", 256, "none"), ("coupled", 2048, "none"), ("uncoupled", 256, "none"),
                                            ("ybj", 2048, "none"), ("coupled", 2048, "filter")])
def test_flow_values_equal_the_reference(kind, nx, mask):
    from niwqg_amd import flow
    m = make(kind, nx, mask)
    check_values(m, flow.NAMES, "%s %d %s set" % (kind, nx, mask))
    advance(m, 3, batched=True)
    check_values(m, flow.NAMES, "%s %d %s 3 steps" % (kind, nx, mask))
    if kind == "coupled" and mask == "none":              # one PDF call with a joint table
        flow_t.check_pdf_calls(m, kind, nx, flow_t.PDF_CALLS[:1])
    m._ctx.close()


@pytest.mark.parametrize("kind, nx, mask", [("coupled", 256, "none"), ("coupled", 2048, "filter"), ("qg", 256, "none"), ("qgc", 256, "none")])
def test_coarse_maps_equal_the_reference(kind, nx, mask):
    from niwqg_amd import coarse
    m = cospec_t.make_qg(nx, True) if kind == "qgc" else make(kind, nx, mask)
    names = coarse.available(m)
    print("coarse %s %d: names %s" % (kind, nx, names))
    if not names:
        pytest.skip("coarse.available has no names for %s" % kind)
    advance(m, 3, batched=True)
    shells = [nx // 8] if nx >= 2048 else sorted({B for n in names for B in coarse_t.cuts(nx, n)})
    tab = np.array([coarse.sharp(m, B) for B in shells] + [coarse.gaussian(m, coarse_t.length(m))])
    R = coarse.flux_maps(m, table=tab)
    tag = "%s %d %s" % (kind, nx, mask)
    coarse_t.check_maps(m, R, tab, coarse.reference(m, tab, names), tag)
    if nx >= 2048:
        coarse_t.check_mean_closes(m, R, shells, tag, cut_list=shells)
    else:
        coarse_t.check_mean_closes(m, R, shells, tag)
    coarse_t.check_moments(R, nx, len(tab))
    m._ctx.close()


S2S_CASES = [(k, 1024, "none") for k in s2s_t.KINDS] + [("coupled", 1024, "filter"), ("coupled", 256, "none"), ("coupled", 2048, "filter")]


@pytest.mark.parametrize("kind, nx, mask", S2S_CASES)
def test_shell_to_shell_rows_equal_the_reference(kind, nx, mask):
    m = make(kind, nx, mask)
    advance(m, 3, batched=True)
    edges = [0, 16, nx // 16, nx // 2] if nx >= 2048 else s2s_t.edges(nx)
    check_s2s_rows(m, edges, "%s %d %s" % (kind, nx, mask))
    m._ctx.close()


@pytest.mark.parametrize("kind, nx, mask", [("coupled", 256, "none"), ("uncoupled", 256, "none"), ("coupled", 2048, "none"),
                                            ("coupled", 2048, "filter")])
def test_cospectra_rows_equal_the_reference(kind, nx, mask):
    m = make(kind, nx, mask)
    cospec_t.check_lists(m, nx, "%s %d %s set" % (kind, nx, mask), only_ends=mask == "none")
    advance(m, 3, batched=True)
    cospec_t.check_lists(m, nx, "%s %d %s 3 steps" % (kind, nx, mask))
    m._ctx.close()


@pytest.mark.parametrize("kind, nx", [("coupled", 128), ("coupled", 256), ("qgc", 512), ("coupled", 2048)])
def test_time_mean_spectra_bit_identity(kind, nx):
    A, B = tspec_t.twin(kind, nx, "filter")
    tspec_t.check_bit_identity(A, B, kind, 4)
    A._ctx.close()
    B._ctx.close()


# ---- 2. the large plans ----------------------------------------------------------------------------------------------------------
def timed(what, t0):
    print("%s: %.1f s" % (what, time.time() - t0))


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_flow_values_4096(big):
    from niwqg_amd import flow
    t0 = time.time()
    steps(big, 2)
    check_values(big, flow.NAMES, "coupled 4096 rough")
    timed("flow values 4096", t0)


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_cospectra_rows_4096(big):
    t0 = time.time()
    steps(big, 2)
    cospec_t.check_lists(big, 4096, "coupled 4096 rough", lists=(("q_psi", "phi2"), ("q_psi", "ow", "gradphi2")))
    timed("co-spectra rows 4096", t0)


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_coarse_identity_and_moments_4096(big):
    from niwqg_amd import coarse
    t0 = time.time()
    steps(big, 2)
    B = 4096 // 8
    R = coarse.flux_maps(big, [B])
    coarse_t.check_mean_closes(big, R, [B], "coupled 4096 rough", cut_list=[B])
    coarse_t.check_moments(R, 4096, 1)
    timed("coarse identity and moments 4096", t0)


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_shell_to_shell_closure_on_a_broadband_state_4096(big):
    """the closure of test_closure_after_steps_with_the_filter on white noise the filter has passed twice: every row transform
    sees a full spectrum below the filter's cut (the feature's own large case is band-limited to nx/8)"""
    from niwqg_amd import shelltoshell
    t0 = time.time()
    steps(big, 2)
    nx = 4096
    R = shelltoshell.shell_to_shell(big, [0, 16, nx // 16, nx // 2])
    assert R.raw.shape[0] == 3
    s2s_t.check_closure(big, R, shelltoshell.NAMES, "coupled 4096 rough")
    s2s_t.check_antisymmetry(R, "ke_niw_ref", "coupled 4096 rough")
    timed("shell-to-shell closure 4096", t0)


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_flow_averages_of_explicit_samples_4096(big):
    """k_x_flow_moments on XPlan<4096>, explicit samples BETWEEN steps (every=0): one sample equals flow.reference
    (test_gpu_averages.own reads a flow name through it), and two samples are x1 + x2 bit for bit.  Nothing is sampled inside a
    step here: that is the next test."""
    t0 = time.time()
    check_averages(big, "coupled", ("ow", "gradphi2", "u"), (("ow", "gradphi2"),))
    timed("flow averages, explicit samples 4096", t0)


def test_flow_averages_sampled_inside_the_dual_stream_step_4096():
    """In-step sampling behind the second stream.  A: flow names attached with every=1, ONE batched nq_step(4): the hook fires
    inside the call after every step, and the next step's q update on the second stream follows each sample.  B, the same state:
    single steps, and after each an explicit sample on zeroed sums, added up on the host in the same order.  First moments are the
    same additions: bit for bit.  The product plane: each product may round once on either side (the device may contract it into the
    addition) and each of the n additions once, at most 2^-53 of sum_i |a_i b_i| each time: 2 (n + 1) 2^-53 sum_i |a_i b_i|."""
    import ctypes
    from niwqg_amd import averages, _lib
    t0 = time.time()
    nx, n = 4096, 4
    fields, products = ("ow", "gradphi2", "u"), (("ow", "gradphi2"),)
    A, B = rough_model(nx), rough_model(nx)
    try:
        info = (ctypes.c_int * 3)()
        assert A._ctx.L.nq_overlap_info(A._ctx.h, info) == 0
        want = _lib.lib().nq_overlap_default_cus(nx)
        assert want > 0 and info[0] >= want, (want, list(info))          # the default step here IS the dual-stream step
        for m in (A, B):
            m._ctx.step(2)                                               # (the filter has taken the Nyquist content away)
        SA, SB = averages.attach(A, fields, products, every=1), averages.attach(B, fields, products, every=0)
        A._ctx.step(n)
        assert SA.info() == {"n": n, "steps": n} and SB.info() == {"n": 0, "steps": 0}
        sums, mag = None, None
        for _ in range(n):
            B._ctx.step(1)
            SB.reset()
            SB.sample()
            R = SB.result()
            assert R.n == 1
            x = {k: np.array(v) for k, v in R.sums.items()}
            ab = np.abs(x["ow"] * x["gradphi2"])
            sums = x if sums is None else {k: sums[k] + x[k] for k in x}
            mag = ab if mag is None else mag + ab
        got = SA.result()
        assert got.n == n
        for k in fields:
            assert np.any(sums[k] != 0) and np.array_equal(got.sums[k], sums[k]), (k, np.abs(got.sums[k] - sums[k]).max())
        k = "ow*gradphi2"
        err = np.abs(got.sums[k] - sums[k])
        print("in-step flow averages 4096: first moments bit for bit; %s: max err / bound = %.3g"
              % (k, (err / np.maximum(2 * (n + 1) * 2.0 ** -53 * mag, 1e-300)).max()))
        assert np.all(err <= 2 * (n + 1) * 2.0 ** -53 * mag), k
        tspec_t.same_state(A, B, "coupled")
    finally:
        A._ctx.close()
        B._ctx.close()
    timed("flow averages sampled inside the step 4096", t0)


@pytest.mark.parametrize("big", [4096, 8192], indirect=True)
def test_cospectra_closure_at_size(big):
    """test_gpu_cospectra.test_closure on the old names, no host transform: the plane means of the products, the tick's sum, and
    auto[q] against 2 x the enstrophy spectrum (from q-hat, no row transform: independent of k_x_cross); two calls bit for bit"""
    from niwqg_amd import cospectra
    t0 = time.time()
    nx = big.nx
    steps(big, 2)
    cospec_t.check_closure(big, "coupled", nx, lists=(("q", "q_psi", "phi2"),), host_transform=False)
    one, two = (cospectra.cross_spectra(big, ("q", "q_psi", "phi2")).raw for _ in range(2))
    assert np.array_equal(one, two) and one.any()
    if nx >= 8192:
        with pytest.raises(NotImplementedError, match="flow names"):
            cospectra.cross_spectra(big, ("q", "ow"))
    timed("co-spectra closure %d" % nx, t0)


@pytest.mark.parametrize("big", [8192], indirect=True)
def test_flow_values_and_pdfs_8192(big):
    """One flow value per thread and one launch per name (flow_nv<8192>() == 1).  (a) u, v against the model's own reads; (b) sn,
    ss, gradphi2 against references formed with the model's ifft2 seam (pinned at this size against pocketfft by
    test_gpu_at_size.test_fft_seam_8192_against_numpy) and numpy multiplies: nothing of x_flow_values or x_row_values is in them;
    (c) strain2 and ow point-wise from the planes of (b).  Then the 1-D PDFs of two names, and the refusals."""
    from niwqg_amd import averages, pdfs
    t0 = time.time()
    m, nx = big, 8192
    steps(m, 2)

    def close(got, want, n):
        err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
        print("coupled 8192 %s: max |device - reference| / max |field| = %.3g" % (n, err / top))
        assert top > 0 and err <= 1e-12 * top, (n, err, top)
    got = device_values(m, ("u", "v"))
    m.jacobian_psi_q()                    # leaves the u, v of the CURRENT psi behind (after a step m.u, m.v are the fourth stage's)
    for n in ("u", "v"):                                                             # (a)
        close(got[n], np.array(getattr(m, n)), n)
    del got
    kk, ll = np.asarray(m.kk, np.float64), np.asarray(m.ll, np.float64)
    ik, il = 1j * kk[None, :], 1j * ll[:, None]
    ph = np.array(m.ph)
    q_psi = np.array(m.q_psi, np.float64)
    sn = 2.0 * np.asarray(m.ifft(ik * (-il * ph))).real                              # (b)
    ss = 2.0 * np.asarray(m.ifft(ik * (ik * ph))).real - q_psi
    del ph
    phih = np.array(m.phih)
    px, py = np.asarray(m.ifft(ik * phih)), np.asarray(m.ifft(il * phih))
    del phih
    grad = px.real ** 2 + px.imag ** 2 + py.real ** 2 + py.imag ** 2
    del px, py
    got = device_values(m, ("sn", "ss", "gradphi2"))
    close(got["sn"], sn, "sn")
    close(got["ss"], ss, "ss")
    close(got["gradphi2"], grad, "gradphi2")
    del got
    strain2 = sn * sn + ss * ss                                                     # (c)
    got = device_values(m, ("strain2", "ow"))
    close(got["strain2"], strain2, "strain2")
    close(got["ow"], strain2 - q_psi * q_psi, "ow")
    del got, strain2, q_psi
    # 1-D PDFs of two names: they close, and equal the restatement on the planes of (b) up to the points near an edge
    ref = {"sn": sn, "gradphi2": grad}
    ranges = {n: flow_t.wide(ref[n]) for n in ref}
    bins = 96
    h = pdfs.field_pdfs(m, names=("sn", "gradphi2"), bins=bins, ranges=ranges)
    for n in ref:
        assert h.below[n] + int(h.counts[n].sum()) + h.above[n] + h.nan[n] == nx * nx, n
        lo, hi = ranges[n]
        n_near = flow_t.near_edges(ref[n], h.edges[n], 1e-11 * (hi - lo))
        l1 = int(np.abs(flow_t.vector(h, n) - flow_t.restated(ref[n], lo, hi, bins)).sum())
        print("coupled 8192 %s: L1 %d, near an edge %d" % (n, l1, n_near))
        assert n_near <= 8, "badly posed"
        assert l1 <= 2 * n_near, (n, l1, n_near)
    with pytest.raises(NotImplementedError, match="joint"):
        pdfs.field_pdfs(m, names=("sn", "gradphi2"), joint=("sn", "gradphi2"))
    with pytest.raises(NotImplementedError, match="product"):
        averages.attach(m, ("sn", "gradphi2"), (("sn", "gradphi2"),), every=0)
    with pytest.raises(NotImplementedError, match="product"):              # a flow name with an old name
        averages.attach(m, ("sn", "q_psi"), (("sn", "q_psi"),), every=0)
    timed("flow values and PDFs 8192", t0)


@pytest.mark.parametrize("big", [8192], indirect=True)
def test_time_mean_spectra_8192(big):
    """two steps, both bodies, against the two host calls.  The twin: a second white-noise model, and BOTH models take the
    fixture's current q and phi through set_phi and set_q, so the two start from the same bits; closed straight afterwards"""
    t0 = time.time()
    B = rough_model(8192)
    q, phi = np.array(big.q), np.array(big.phi)
    for m in (big, B):
        m.set_phi(phi)
        m.set_q(q)
    del q, phi
    try:
        tspec_t.same_state(big, B, "coupled")
        tspec_t.check_bit_identity(big, B, "coupled", 2)
    finally:
        B._ctx.close()
    big._after_steps()
    timed("time-mean spectra 8192", t0)


# ---- 3. fields that vanish -------------------------------------------------------------------------------------------------------
def zero_rows(cs, zero, tag):
    """the rows of the names in `zero` are exactly 0.0 and every coherence with them NaN; the others have content"""
    for a in cs.names:
        if a in zero:
            assert np.array_equal(cs.auto[a], np.zeros_like(cs.auto[a])), (tag, a, float(np.abs(cs.auto[a]).max()))
        else:
            assert (cs.auto[a][1:] > 0).all(), (tag, a)
        for b in cs.names:
            if a != b and (a in zero or b in zero):
                co, coh = cs.co[(a, b)], cs.coherence(a, b)
                assert np.array_equal(co, np.zeros_like(co)), (tag, a, b, float(np.abs(co).max()))
                assert np.isnan(coh).all(), (tag, a, b, coh[~np.isnan(coh)][:4])


def zero_waves(kind, nx):
    """make's q under phi = 0 exactly (set_phi first: set_q then inverts with it)"""
    m = make(kind, nx)
    q = np.array(m.q)
    m.set_phi(np.zeros((nx, nx), complex))
    m.set_q(q)
    return m


@pytest.mark.parametrize("nx", [64, 1024])
def test_cospectra_of_zero_waves(nx):
    """phi = 0 exactly: packed with q_psi, the split part of |phi|^2 is the round-off of q_psi's transform; it must come out as
    exact zeros (k_cospec_scale hands BinCross the factor 0 for a field whose maximum is 0), in either position of the list"""
    from niwqg_amd import cospectra
    m = zero_waves("coupled", nx)
    for stage in ("set", "2 steps"):
        assert not np.asarray(m.phi).any()
        alone = cospectra.cross_spectra(m, ("q_psi",))
        for names in (("q_psi", "phi2"), ("q_psi", "phi2", "gradphi2"), ("phi2", "q_psi"), ("gradphi2", "q_psi", "phi2")):
            tag = "zero waves %d %s %s" % (nx, stage, "/".join(names))
            cs = cospectra.cross_spectra(m, names)
            zero_rows(cs, ("phi2", "gradphi2"), tag)
            same = np.array_equal(cs.auto["q_psi"], alone.auto["q_psi"])
            print("%s: auto[q_psi] equals the one-name call bit for bit: %s (max difference %.3g of the row's maximum)"
                  % (tag, same, np.abs(cs.auto["q_psi"] - alone.auto["q_psi"]).max() / alone.auto["q_psi"].max()))
            assert same, tag
            assert np.array_equal(cospectra.cross_spectra(m, names).raw, cs.raw), tag        # two calls
        advance(m, 2, batched=True)
    m._ctx.close()


def test_cospectra_of_zero_pv_under_waves():
    """q = 0 exactly under waves (test_gpu_magnitudes.test_zero_pv_under_waves's state): by the same rule, the rows of a plane that
    is exactly zero are exact zeros; a plane that is the round-off of its partner's transform (q shares q_w's after a step) is an
    ordinary field and its rows equal numpy's on the plane the averages sample"""
    from niwqg_amd import cospectra
    from test_magnitudes_host import degenerate_states, make_device, start
    kind, kw, f = degenerate_states()["q_zero"]
    m = start(make_device(kind, kw), f)
    nx = m.nx
    for stage in ("set", "4 steps"):
        names = ("q", "phi2")
        planes = device_values(m, names)
        exact = not planes["q"].any()
        print("zero PV %s: max |q| of the sampled plane = %.3g" % (stage, np.abs(planes["q"]).max()))
        for lst in (names, names[::-1]):
            cs = cospectra.cross_spectra(m, lst)
            if exact:
                zero_rows(cs, ("q",), "zero PV %s" % stage)
                assert np.array_equal(cs.auto["phi2"], cospectra.cross_spectra(m, ("phi2",)).auto["phi2"]), lst
            else:
                cospec_t.check_rows(cs, cospec_t.transforms(planes), planes, nx, "zero PV %s" % stage)
        for _ in range(4):
            m._step_forward()
    m._ctx.close()


def test_cospectra_of_uniform_waves():
    """phi uniform: |phi|^2 is a constant, all of auto[phi2] sits in shell 0 and the shells >= 1 hold at most the round-off of the
    packed transform (cospectra.transform_rounding, packed)"""
    from niwqg_amd import cospectra
    nx = 64
    m = make("coupled", nx)
    q = np.array(m.q)
    m.set_phi(np.full((nx, nx), 0.2 + 0.1j))
    m.set_q(q)
    names = ("q_psi", "phi2")
    planes = device_values(m, names)
    T = cospec_t.transforms(planes)
    cs = cospectra.cross_spectra(m, names)
    cospec_t.check_rows(cs, T, planes, nx, "uniform waves")
    a, A = planes["phi2"], T["phi2"]
    rounding = cospectra.transform_rounding(A, A, a, a, nx, packed=True)
    want = cospectra.bin_shells(np.abs(A) ** 2, nx) / float(nx) ** 4
    print("uniform waves: auto[phi2][0] = %.17g, mean^2 = %.17g; shells >= 1: max %.3g, bound %.3g"
          % (cs.auto["phi2"][0], a.mean() ** 2, cs.auto["phi2"][1:].max(), (want + rounding)[1:].max()))
    assert abs(cs.auto["phi2"][0] - a.mean() ** 2) <= 1e-12 * a.mean() ** 2
    assert (cs.auto["phi2"][1:] <= (want + rounding)[1:]).all()
    m._ctx.close()


def test_flow_coarse_and_shell_to_shell_of_zero_waves():
    """phi = 0 exactly: gradphi2 and the wave rows and maps are exact zeros, the other flow values equal flow.reference, and the
    balanced rows and maps (ens, ke_qg) are those of an UnCoupledModel on the same q and equal their references"""
    from niwqg_amd import coarse, flow, shelltoshell
    nx = 64
    m, u = zero_waves("coupled", nx), zero_waves("uncoupled", nx)
    for stage in ("set", "3 steps"):
        tag = "zero waves %d %s" % (nx, stage)
        assert not device_values(m, ["gradphi2"])["gradphi2"].any()
        check_values(m, [n for n in flow.NAMES if n != "gradphi2"], tag)
        edges, cuts = [0, 4, nx // 8, nx // 2], [2, nx // 8]
        R, Ru = (shelltoshell.shell_to_shell(x, edges) for x in (m, u))
        for n in ("ke_niw_adv", "ke_niw_ref"):
            assert not R.rows[n].any(), (tag, n)
        check_s2s_rows(m, edges, tag, names=("ke_qg", "ens"))
        C, Cu = (coarse.flux_maps(x, cuts) for x in (m, u))
        assert not C.maps["ke_niw_adv"].any() and not C.sums["ke_niw_adv"].any() and not C.sumsq["ke_niw_adv"].any(), tag
        check_coarse(m, cuts, tag, names=["ke_qg", "ens"])
        for n in ("ke_qg", "ens"):
            same = (np.array_equal(R.rows[n], Ru.rows[n]), np.array_equal(C.maps[n], Cu.maps[n]))
            print("%s %s: bit for bit the UnCoupledModel's rows: %s, maps: %s" % (tag, n, same[0], same[1]))
            assert all(same), (tag, n, same)
        advance(m, 3, batched=True)
        advance(u, 3, batched=True)
    m._ctx.close()
    u._ctx.close()
