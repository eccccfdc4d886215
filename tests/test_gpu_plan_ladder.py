"""The step attachments and the binned diagnostics on every fused plan ("features x plans").

The feature tests pin values on a few plans each; this module walks the ladder.  Row plans: XPlan<N> is one instantiation per
size (64: eight rows per workgroup, 128: four, 256: two, 512: one row in one wave, 1024 / 2048 / 4096: 2 / 4 / 8 waves, 8192: 16
waves and a 128 KB exchange).  Column plans: single-pass columns up to 512 on one rank, the two-pass tiles (32,32), (32,64),
(64,64), (64,128) from 1024 on, and, with NIWQG_AMD_SINGLE_PASS=0, the two-pass tiles (8,8) ... (16,32) on 64 ... 512.  The
dual-stream step is CoupledModel 4096^2 by default.

Every check is one the feature's own test makes at another size, through the same helpers and with the same bound:
1e-12 relative L2 between two states, 1e-12 of the field's maximum between two device routes to one plane, 1e-10 per shell over
sum |ref| for spectra against numpy, 1e-11 sum |S| for closure, equality for counts, ring records and first-moment sums.

The analysis features that came after this module (flow names, time-mean spectra, coarse-grained maps, shell-to-shell transfers,
co-spectra) have their row plans, large plans and zero fields in the sibling tests/test_gpu_plan_ladder_analysis.py; the children of
this module under NIWQG_AMD_SINGLE_PASS=0 and NIWQG_AMD_Y_SPLIT run them too (``check_analysis``).

4096^2 and 8192^2 states are seeded white noise in physical space (the scaling of test_gpu_at_size's rough-field step, filter
on): no host transform is needed to build them.  One model per size lives in a module-scoped fixture; its checks read it or step
it forward, none depends on the step count another left behind."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_oracle_golden import rel
from test_gpu_at_size import rough_kwargs
from test_gpu_spectra import make, steps, np_shell, restated, check_raw_closure
from test_gpu_transfer import restated as ref
from test_gpu_pdfs import check_against_fields, check_closure, check_marginals, joint_of, widened
from test_gpu_averages import own, attach_all, one_sample, advance
from test_gpu_frequency import state_blocks, model as recorder_model
from test_gpu_forcing import pair, amplitudes, full_hermitian, restated as restated_increment
import test_gpu_flow as flow_t
import test_gpu_coarse as coarse_t
import test_gpu_shelltoshell as s2s_t
import test_gpu_cospectra as cospec_t
import test_gpu_timespectra as tspec_t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
KERNEL = ("coupled", "uncoupled", "ybj")
SWITCHES = ("NIWQG_AMD_SINGLE_PASS", "NIWQG_AMD_SMALL_QG", "NIWQG_AMD_Y_SPLIT")


# ---- states ------------------------------------------------------------------------------------------------------------------
def rough_model(nx, seed=11):
    """CoupledModel on white noise in physical space: every mode of the grid is populated, nothing is transformed on the host"""
    import niwqg_amd
    m = niwqg_amd.CoupledModel.Model(**rough_kwargs(nx))
    rng = np.random.default_rng(seed)
    m.set_q(1e-5 * rng.standard_normal((nx, nx)))
    m.set_phi(0.05 * (rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx))))
    return m


@pytest.fixture(scope="module")
def big(request):
    """the one white-noise model of a large size; closed at the end so that the next size does not start beside it"""
    m = rough_model(request.param)
    yield m
    m._ctx.close()


@pytest.fixture(scope="module")
def stepped():
    """(kind, nx, mask) -> make(...) after ten steps: stepped once, only read afterwards"""
    cache = {}

    def get(kind, nx, mask="filter"):
        key = (kind, nx, mask)
        if key not in cache:
            cache[key] = make(kind, nx, mask)
            steps(cache[key], 10)
        return cache[key]
    yield get
    for m in cache.values():
        m._ctx.close()


def state_of(m):
    out = dict(q=m.q, qh=m.qh, ph=m.ph)
    if hasattr(m, "phih"):
        out.update(phi=m.phi, phih=m.phih)
    if getattr(m, "passive_scalar", False):
        out.update(c=m.c, ch=m.ch)
    return {k: np.array(v) for k, v in out.items()}


def record_budgets(m):
    """the increments every later step hands to Ke, Pw, Kw (QGModel: Ke, and the scalar's variance), as the step hands them over:
    the totals themselves start from atomically reduced sums whose last bits differ between any two runs"""
    from niwqg_amd import _lib
    log, c = [], m._ctx
    if hasattr(m, "phih"):
        take = c.take_budget_increments

        def taking():
            d = take()
            log.append(d)
            return d
        c.take_budget_increments = taking
    else:
        scalar = c.scalar

        def reading(sid):
            v = scalar(sid)
            if sid in (_lib.S_KE, _lib.S_PW):
                log.append(v)
            return v
        c.scalar = reading
    return log


# ---- the checks, each in the form of its feature's own test ---------------------------------------------------------------------
def check_averages(m, kind, fields=None, products=()):
    """test_gpu_averages.test_one_sample_is_the_field, then a second sample from a later step: S = x1 + x2 bit for bit"""
    from niwqg_amd import averages
    nx = m.nx
    A = attach_all(m, kind, 0) if fields is None else averages.attach(m, fields, products, every=0)
    advance(m, 3)
    assert A.info() == {"n": 0, "steps": 3}
    A.sample()
    R = A.result()
    assert R.n == 1 and R.steps == 3
    same_plane = kind in ("qg", "qgc")                         # the sample reads the very plane the model's read returns
    for n in A.fields:
        got, want = R.sums[n], own(m, n)
        assert got.shape == (nx, nx) and got.dtype == (np.complex128 if n == "phi" else np.float64) and np.any(want != 0)
        err, top = np.abs(got - want).max(), np.abs(want).max()
        print("averages %s %d %s: max |S - field| / max |field| = %.3g" % (kind, nx, n, err / top))
        if same_plane:
            assert np.array_equal(got, want), n
        else:                                                  # two device routes to one quantity: the standing 1e-12
            assert err <= 1e-12 * top, (n, err, top)
    for a, b in A.products:
        x, y = R.sums[a], R.sums[b]
        assert np.all(np.abs(R.sums[a + "*" + b] - x * y) <= 2 * U * np.abs(x * y)), (a, b)
    x1 = {n: R.sums[n] for n in A.fields}
    advance(m, 1)
    A.sample()
    S = A.result()
    assert S.n == 2 and S.steps == 4
    two = {n: S.sums[n] for n in A.fields}
    x2 = one_sample(A)
    for n in A.fields:
        assert np.any(x2[n] != x1[n]) or (kind == "ybj" and n in ("q", "q_psi")), n        # (the state moved)
        assert np.array_equal(two[n], x1[n] + x2[n]), (n, np.abs(two[n] - (x1[n] + x2[n])).max())
    A.detach()


def check_pdfs(m, kind, bins=256, jb=64):
    """test_gpu_pdfs.model_checks on one state: the default-range pass, the widened-range pass and the marginals"""
    from niwqg_amd import pdfs
    names = pdfs.available(m)
    h = pdfs.field_pdfs(m, bins=bins, joint=joint_of(names), joint_bins=jb)
    check_closure(m, h, names, True)
    if h.joint is not None:
        check_marginals(h, bins, jb)
    check_against_fields(m, h, names, bins, False)
    h2 = pdfs.field_pdfs(m, bins=bins, ranges=widened(m, names), joint=joint_of(names), joint_bins=jb)
    check_closure(m, h2, names, False)
    assert all(h2.below[n] == h2.above[n] == 0 for n in names)
    check_against_fields(m, h2, names, bins, True)


def check_spectra_numpy(m, tag=""):
    from niwqg_amd.spectra import isotropic_spectra, shell_modes
    sp = isotropic_spectra(m)
    assert np.array_equal(sp.modes, shell_modes(m.nx)) and sp.modes.sum() == m.nx ** 2
    want = restated(m)
    worst = 0.0
    for name, v in sp.values.items():
        err = np.abs(v - want[name]).max() / np.abs(want[name]).sum()
        worst = max(worst, err)
        assert err <= 1e-10, (name, err)
    print("spectra %s %d: worst shell error / sum |ref| = %.3g" % (tag, m.nx, worst))
    return sp


def check_transfer_numpy(m, tag=""):
    from niwqg_amd.transfer import spectral_transfer, available
    st = spectral_transfer(m)
    want = ref(m)
    assert set(st.transfer) == set(available(m)) == set(want)
    worst = 0.0
    for name, t in st.transfer.items():
        err = np.abs(t - want[name]).max() / np.abs(want[name]).sum()
        worst = max(worst, err)
        assert err <= 1e-10, (name, err)
        assert np.array_equal(st.flux[name], -np.cumsum(t))
    print("transfer %s %d: worst shell error / sum |ref| = %.3g" % (tag, m.nx, worst))


def check_transfer_identities(m, kind):
    """test_refraction_transfer_sums_to_zero and test_balanced_energy_transfer_sums_to_zero_with_the_filter"""
    from niwqg_amd.transfer import spectral_transfer
    for name in (["ke_niw_ref"] if kind in KERNEL else []) + (["ke_qg"] if kind != "ybj" else []):
        t = spectral_transfer(m, names=[name]).transfer[name]
        print("transfer identity %s %d %s: |sum| / sum |t| = %.3g" % (kind, m.nx, name, abs(t.sum()) / np.abs(t).sum()))
        assert np.abs(t).sum() > 0
        assert abs(t.sum()) <= 1e-12 * np.abs(t).sum(), (name, t.sum(), np.abs(t).sum())


SPECTRAL = ("ens", "ke_qg", "chi_q", "ke_niw", "pe_niw", "ep_phi", "chi_phi")


def restated_spectral(m):
    """the rows of test_gpu_spectra.restated that need q-hat, psi-hat and phi-hat only, from the downloaded spectra themselves"""
    nx, M2 = m.nx, float(m.nx) ** 4
    b = np_shell(nx).ravel()
    nb = int(b.max()) + 1
    k = np.fft.fftfreq(nx, 1.0 / nx) * m.dk
    wv2 = k[None, :] ** 2 + k[:, None] ** 2
    wv4 = wv2 ** 2

    def binned(x):
        return np.bincount(b, weights=np.ravel(x), minlength=nb)
    q2, p2, a2 = np.abs(m.qh) ** 2, np.abs(m.ph) ** 2, np.abs(m.phih) ** 2
    return dict(ens=binned(0.5 * q2) / M2, ke_qg=binned(0.5 * wv2 * p2) / M2, chi_q=-m.nu4 * binned(wv4 * q2) / M2,
                ke_niw=binned(0.5 * a2) / M2, pe_niw=binned(0.25 * wv2 * a2) / M2 / m.kappa2,
                ep_phi=(-m.nu4w * binned(wv4 * a2) - m.muw * binned(a2) - m.nuw * binned(wv2 * a2)) / M2,
                chi_phi=(-0.5 * m.nu4w * binned(wv4 * wv2 * a2) - 0.5 * m.nuw * binned(wv4 * a2)
                         - 0.5 * m.muw * binned(wv2 * a2)) / M2 / m.kappa2)


def check_spectral_rows(m, sp=None):
    from niwqg_amd.spectra import isotropic_spectra
    sp = sp or isotropic_spectra(m, names=list(SPECTRAL))
    want = restated_spectral(m)
    for name in SPECTRAL:
        err = np.abs(sp.values[name] - want[name]).max() / np.abs(want[name]).sum()
        print("spectral rows %d %s: shell error / sum |ref| = %.3g" % (m.nx, name, err))
        assert np.abs(want[name]).sum() > 0 and err <= 1e-10, (name, err)


def check_ring(m, kind, K, nsteps):
    """test_gpu_frequency.test_ring_is_the_state: every record is the block of the downloads, bit for bit"""
    from niwqg_amd import frequency
    R = frequency.attach(m, K, length=16)
    assert R.fields == {"qg": ("q", "psi"), "ybj": ("phi",)}.get(kind, ("phi", "q", "psi"))
    for step in range(nsteps + 1):
        if step:
            m._step_forward()
        want = state_blocks(m, R.fields, K)
        for n in R.fields:
            ts = R.series(n)
            assert ts.values.shape == (step + 1, 2 * K + 1, 2 * K + 1 if n == "phi" else K + 1) and ts.values.dtype == np.complex128
            assert np.array_equal(ts.step, np.arange(step + 1))
            assert np.any(ts.values[-1] != 0)
            assert np.array_equal(ts.values[-1], want[n]), (n, step, np.abs(ts.values[-1] - want[n]).max())
            if step:
                assert not np.array_equal(ts.values[-1], ts.values[-2]), n
    assert R.info() == {"written": nsteps + 1, "held": nsteps + 1, "steps": nsteps}
    R.detach()


def check_forced_twin(A, B, kind, seed=21):
    """Twin models on one state, A forced, one step: A - B is the restated increment.  Then B takes A's forced state through
    set_phi and set_q, A's forcing goes, and three steps of both agree in the state, psi-hat, u, v and the budget increments: what
    the forcing tail left behind (the re-emitted phi and phi_y, the re-inversion, the spectral sums carried into the next step's
    slot 0) is what set_phi and set_q leave."""
    from niwqg_amd import forcing
    nx, wave = A.nx, kind in KERNEL
    tag = "forced twin %s %d" % (kind, nx)
    Aq, Aphi = amplitudes(nx, "q+phi" if wave else "q")
    F = forcing.attach(A, q=Aq, phi=Aphi, seed=seed)
    A._step_forward()
    B._step_forward()
    # The bound of test_increment_is_the_restated_noise, 1e-13 max A, plus what the comparison through the state adds: the device
    # rounds state + D once and the difference of the two downloads rounds once more, each by at most 2^-53 of the forced value
    for name, amp, stream in (("qh", Aq, 0), ("phih", Aphi, 1)):
        if amp is None:
            continue
        a = np.array(getattr(A, name))
        d = a - np.array(getattr(B, name))
        want = restated_increment(nx, A.dt, amp, 0, stream, seed)
        if want.shape != d.shape:
            want = full_hermitian(want)
        err = np.abs(d - want)
        print("%s %s: max |A - B - D| = %.3e, bound 1e-13 max A = %.3e" % (tag, name, err.max(), 1e-13 * amp.max()))
        assert np.all(err <= 1e-13 * amp.max() + 2 * U * np.abs(a)), name
        assert np.abs(d).max() > 0.1 * np.sqrt(A.dt) * amp.max()
    assert F.state()["step"] == 1
    F.detach()
    if wave:
        B.set_phi(np.array(A.phi))
    if kind == "qgc":
        B.set_c(np.array(A.c))
    B.set_q(np.array(A.q))
    logs = [record_budgets(x) for x in (A, B)]
    for _ in range(3):
        A._step_forward()
        B._step_forward()
    for name in ("q", "ph", "u", "v") + (("phi",) if wave else ()) + (("c",) if kind == "qgc" else ()):
        e = rel(np.array(getattr(A, name)), np.array(getattr(B, name)))
        print("%s %s: %.2e" % (tag, name, e))
        assert e <= 1e-12, (name, e)
    a, b = (np.array(x, float).reshape(3, -1) for x in logs)
    assert np.isfinite(b).all() and np.all(np.abs(b).max(axis=0) > 0)
    for j in range(b.shape[1]):
        e = np.linalg.norm(a[:, j] - b[:, j]) / np.linalg.norm(b[:, j])
        print("%s budget %d: %.2e" % (tag, j, e))
        assert e <= 1e-12, (j, a[:, j], b[:, j])


def check_coarse(m, shells, tag, gaussian=False, names=None):
    """test_gpu_coarse's three value checks on the sharp cuts `shells` (and one Gaussian): the maps equal coarse.reference, the
    plane means close on the spectral flux, the moments agree with the downloaded maps"""
    from niwqg_amd import coarse
    tab = np.array([coarse.sharp(m, B) for B in shells] + ([coarse.gaussian(m, coarse_t.length(m))] if gaussian else []))
    R = coarse.flux_maps(m, table=tab, names=names)
    coarse_t.check_maps(m, R, tab, coarse.reference(m, tab, list(R.names)), tag)
    if names is None:
        coarse_t.check_mean_closes(m, R, list(shells), tag, cut_list=list(shells))
    coarse_t.check_moments(R, m.nx, len(tab))
    return R


def check_s2s_rows(m, edges, tag, names=None):
    """test_gpu_shelltoshell.test_rows_equal_the_reference on the bands between `edges`"""
    from niwqg_amd import shelltoshell
    R = shelltoshell.shell_to_shell(m, edges, names=names)
    assert R.raw.shape[0] == len(edges) - 1
    s2s_t.check_rows(m, R, tag, m.nx, "")
    return R


def check_qgc_cospectra(m, tag):
    """test_gpu_cospectra.test_qgmodel's value check: QGModel bins q-hat and c-hat as they are"""
    from niwqg_amd import cospectra
    planes = {n: np.array(getattr(m, n), np.float64) for n in ("q", "c")}
    T = cospec_t.transforms(planes)
    for lst in (("q", "c"), ("c", "q")):
        cospec_t.check_rows(cospectra.cross_spectra(m, lst), T, planes, m.nx, tag, packed=False)


def check_analysis(m, kind, tag, cuts, edges, lists):
    """the analysis features of sections 5m to 5q on one state of a coupled or a qgc model, against numpy: what a child under
    a column-plan switch adds to its battery"""
    from niwqg_amd import flow
    if kind == "coupled":
        flow_t.check_values(m, flow.NAMES, tag)
        cospec_t.check_lists(m, m.nx, tag, lists=lists)
    else:
        check_qgc_cospectra(m, tag)
    check_coarse(m, cuts, tag)
    check_s2s_rows(m, edges, tag)


# ---- 1. averages on every row plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask", [("coupled", 128, "filter"), ("coupled", 256, "filter"), ("coupled", 2048, "filter"),
                                            ("uncoupled", 256, "filter"), ("uncoupled", 2048, "filter"), ("ybj", 1024, "filter"),
                                            ("coupled", 1024, "mask")])
def test_averages_one_sample_is_the_field(kind, nx, mask):
    m = make(kind, nx, mask)
    assert m._dual == (mask == "mask")
    check_averages(m, kind)
    m._ctx.close()


@pytest.mark.parametrize("big", [4096, 8192], indirect=True)
def test_averages_one_sample_is_the_field_at_size(big):
    check_averages(big, "coupled", ("q_psi", "phi2", "phi"), (("q_psi", "phi2"),))


# ---- 2. PDFs against the fields on every row plan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 64), ("coupled", 256), ("coupled", 512), ("coupled", 1024), ("coupled", 2048),
                                      ("uncoupled", 512)])
def test_pdfs_against_the_fields(kind, nx):
    m = make(kind, nx)
    steps(m, 2)
    check_pdfs(m, kind)
    m._ctx.close()


CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_plan_ladder as T
res = T.%(call)s
if res is not None:
    np.savez(sys.argv[1], **res)
print("child ok")
"""


def run_child(tmp_path, call, env=None):
    """T.<call> in a fresh process: the switches are read when a context is created"""
    script, out = tmp_path / "child.py", tmp_path / "child.npz"
    script.write_text(CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "call": call})
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env or {})
    r = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=420, env=e, cwd=str(tmp_path))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    print(r.stdout[-3000:])
    return np.load(str(out)) if out.exists() else None


def pdfs_at_size(nx):
    m = rough_model(nx)
    steps(m, 2)
    check_pdfs(m, "coupled")


def test_pdfs_against_the_fields_4096(tmp_path):
    run_child(tmp_path, "pdfs_at_size(4096)")


# ---- 3. spectra and transfer on two-pass columns and multi-wave rows ------------------------------------------------------------------
NUMPY_CASES = [("coupled", 1024, "filter"), ("coupled", 2048, "filter"), ("uncoupled", 1024, "filter"), ("ybj", 1024, "filter"),
               ("qg", 1024, "filter"), ("qgc", 1024, "filter"), ("coupled", 1024, "dual")]


@pytest.mark.parametrize("kind, nx, mask", NUMPY_CASES)
def test_spectra_against_numpy(stepped, kind, nx, mask):
    m = stepped(kind, nx, mask)
    sp = check_spectra_numpy(m, "%s %s" % (kind, mask))
    if kind == "coupled" and mask == "filter":                 # the host-transform-free form of the 4096 test, where both exist
        check_spectral_rows(m, sp)


@pytest.mark.parametrize("kind, nx, mask", NUMPY_CASES)
def test_transfer_against_numpy(stepped, kind, nx, mask):
    check_transfer_numpy(stepped(kind, nx, mask), "%s %s" % (kind, mask))


@pytest.mark.parametrize("kind, nx", [("coupled", 1024), ("coupled", 2048), ("qgc", 2048)])
def test_closure_and_transfer_identities(stepped, kind, nx):
    m = stepped(kind, nx)
    check_raw_closure(m, kind)
    check_transfer_identities(m, kind)


@pytest.mark.parametrize("big", [4096, 8192], indirect=True)
def test_closure_and_transfer_identities_at_size(big):
    steps(big, 2)                                              # (the filter has taken the Nyquist content away)
    check_raw_closure(big, "coupled")
    check_transfer_identities(big, "coupled")


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_spectral_rows_4096(big):
    steps(big, 2)
    check_spectral_rows(big)


# ---- 4. two-pass tiles at small sizes, and the other switches ---------------------------------------------------------------------------
def a_subpasses_of_one_step(m):
    c = m._ctx
    c.profile_enable(c.KERNEL_CLASSES["y_A"])
    c.step(1)
    n, _ = c.profile_read()
    c.profile_enable(-1)
    return n


def battery(nx):
    """what a child under a switch runs: a coupled and a qgc model, ten steps each, the value checks of every feature in this
    process, the states for the parent"""
    out = {}
    for kind in ("coupled", "qgc"):
        m = make(kind, nx)
        steps(m, 10)
        out.update({kind + ":" + k: v for k, v in state_of(m).items()})
        check_spectra_numpy(m, kind)
        check_transfer_numpy(m, kind)
        check_pdfs(m, kind)
        check_averages(m, kind)
        twins = [make(kind, nx) for _ in range(4)]
        check_forced_twin(twins[0], twins[1], kind)
        check_analysis(m, kind, "%s %d two-pass" % (kind, nx), sorted({2, nx // 8}), [0, 4, nx // 8, nx // 2], cospec_t.LISTS[:2])
        tspec_t.check_bit_identity(twins[2], twins[3], kind, 4)
        for t in twins:
            t._ctx.close()
        out[kind + ":a_subpasses"] = np.array(a_subpasses_of_one_step(m))
    return out


def assert_same_states(got, want, prefix=""):
    for k, v in want.items():
        e = rel(got[prefix + k], v)
        print("%s%s: %.2e" % (prefix, k, e))
        assert e <= 1e-12, (prefix + k, e)


@pytest.mark.parametrize("nx", [64, 128, 256, 512])
def test_two_pass_tiles_at_small_sizes(tmp_path, nx):
    got = run_child(tmp_path, "battery(%d)" % nx, {"NIWQG_AMD_SINGLE_PASS": "0"})
    for kind in ("coupled", "qgc"):
        m = make(kind, nx)
        steps(m, 10)
        assert_same_states(got, state_of(m), kind + ":")
        assert got[kind + ":a_subpasses"] > 0 and a_subpasses_of_one_step(m) == 0       # the child really ran the A sub-passes
        m._ctx.close()


def qg_run(nx):
    m = make("qg", nx)
    log = record_budgets(m)
    steps(m, 10)
    return dict(state_of(m), budgets=np.array(log))


@pytest.mark.parametrize("nx", [128, 256])
def test_separate_q_and_invert_kernels_of_small_qg(tmp_path, nx):
    got, want = run_child(tmp_path, "qg_run(%d)" % nx, {"NIWQG_AMD_SMALL_QG": "0"}), qg_run(nx)
    assert want["budgets"].shape == (10,) and np.all(want["budgets"] != 0)
    assert_same_states(got, want)


def split_run():
    m = make("coupled", 1024)
    steps(m, 10)
    check_spectra_numpy(m, "coupled 16,64")
    check_transfer_numpy(m, "coupled 16,64")
    check_analysis(m, "coupled", "coupled 1024 split 16,64", [1024 // 8], [0, 16, 1024 // 16, 1024 // 2], cospec_t.LISTS[1:2])
    return state_of(m)


def test_another_y_split_at_1024(tmp_path, stepped):
    got = run_child(tmp_path, "split_run()", {"NIWQG_AMD_Y_SPLIT": "16,64"})
    assert_same_states(got, state_of(stepped("coupled", 1024)))


def test_y_split_alone_is_refused_on_single_pass_grids(monkeypatch):
    monkeypatch.delenv("NIWQG_AMD_SINGLE_PASS", raising=False)
    monkeypatch.setenv("NIWQG_AMD_Y_SPLIT", "8,16")
    with pytest.raises(RuntimeError, match="NIWQG_AMD_Y_SPLIT has no effect on a single-rank grid <= 512"):
        make("coupled", 128)


# ---- 5. forcing beyond single-pass columns ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx", [("coupled", 1024), ("coupled", 2048), ("coupled", 4096), ("qg", 1024)])
def test_forced_twin(kind, nx):
    A, _, init, kw = pair(kind, nx, "filter", oracle=False)
    B = type(A)(**kw)
    init(A)
    init(B)
    check_forced_twin(A, B, kind)
    A._ctx.close()
    B._ctx.close()


# ---- 6. the recorder on the large plans ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask, K", [("coupled", 1024, "filter", 16), ("coupled", 1024, "mask", 8), ("qg", 2048, "filter", 8)])
def test_ring_is_the_state(kind, nx, mask, K):
    m = recorder_model(kind, nx, mask)
    assert bool(getattr(m, "_dual", False)) == (mask == "mask")
    check_ring(m, kind, K, 6)
    m._ctx.close()


@pytest.mark.parametrize("big", [4096], indirect=True)
def test_ring_is_the_state_4096(big):
    check_ring(big, "coupled", 8, 3)


def test_batching_and_wrap_1024():
    from niwqg_amd import frequency
    A, B = recorder_model("coupled", 1024), recorder_model("coupled", 1024)
    RA, RB = (frequency.attach(m, 8, every=3, length=4) for m in (A, B))
    A._ctx.step(11)
    for _ in range(11):
        B._step_forward()
    assert RA.info() == RB.info() == {"written": 4, "held": 4, "steps": 11}
    for n in RA.fields:
        a, b = RA.series(n), RB.series(n)
        assert np.array_equal(a.step, [0, 3, 6, 9]) and np.array_equal(b.step, [0, 3, 6, 9])
        assert np.array_equal(a.values, b.values), n
    A._ctx.step(4)                                             # the fifth and sixth record wrap the ring
    for _ in range(4):
        B._step_forward()
    for n in RA.fields:
        a, b = RA.series(n), RB.series(n)
        assert np.array_equal(a.step, [6, 9, 12, 15]) and np.array_equal(a.values, b.values), n
    assert np.array_equal(RB.series("phi").values[-1], state_blocks(B, ("phi",), 8)["phi"])
    assert RA.info() == {"written": 6, "held": 4, "steps": 15}
    A._ctx.close()
    B._ctx.close()
