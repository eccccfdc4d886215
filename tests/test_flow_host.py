"""The flow fields' numpy restatement (niwqg_amd/flow.py: reference) against the analytic fields of a single Fourier mode, its own
identities, and the parts of the PDFs' and the averages' contracts the flow names must leave alone.  No GPU."""
import types

import numpy as np
import pytest


def shim(nx, L, ph, phih, q_psi):
    dk = 2 * np.pi / L
    kk = dk * np.append(np.arange(0., nx / 2), np.arange(-nx / 2, 0.))
    return types.SimpleNamespace(nx=nx, kk=kk, ll=kk.copy(), ph=ph, phih=phih, q_psi=q_psi)


@pytest.mark.parametrize("nx, a, b", [(32, 3, 5), (48, 7, 2), (32, 4, 0), (32, 0, 6)])
def test_reference_on_a_single_fourier_mode(nx, a, b):
    from niwqg_amd import flow
    L = 2 * np.pi * 3.0
    dk = 2 * np.pi / L
    x = np.arange(nx) * L / nx
    X, Y = np.meshgrid(x, x)
    k, l, A, th0 = a * dk, b * dk, 0.7, 0.3
    th = k * X + l * Y + th0
    psi = A * np.cos(th)
    qbar = 0.25                                          # a plane mean of q_psi, which psi does not carry: ss carries minus it, as stated
    q_psi = -(k * k + l * l) * psi + qbar
    c, p, r, B = 2 * dk, -3 * dk, 0.4, 1.3 - 0.6j        # phi = B exp(i (c x + p y)) + r
    phi = B * np.exp(1j * (c * X + p * Y)) + r
    m = shim(nx, L, np.fft.fft2(psi), np.fft.fft2(phi), q_psi)
    R = flow.reference(m)
    assert sorted(R) == sorted(flow.NAMES) and all(v.shape == (nx, nx) and v.dtype == np.float64 for v in R.values())
    s = np.sin(th)
    want = {"u": A * l * s, "v": -A * k * s, "sn": 2 * A * k * l * np.cos(th), "ss": (l * l - k * k) * psi - qbar}
    want["strain2"] = want["sn"] ** 2 + want["ss"] ** 2
    want["ow"] = want["strain2"] - q_psi ** 2
    want["gradphi2"] = np.full((nx, nx), (c * c + p * p) * abs(B) ** 2)
    for n in flow.NAMES:
        # ow is a difference of squares of size (A kappa^2 + qbar)^2: its rounding scales with those, not with its own maximum
        scale = A * (k * k + l * l) + abs(qbar) + 1
        assert np.abs(R[n] - want[n]).max() <= 1e-13 * (scale * scale if n in ("strain2", "ow") else max(np.abs(want[n]).max(), scale)), n
    assert list(flow.reference(m, ["ow"])) == ["ow"] and np.array_equal(flow.reference(m, "ow")["ow"], R["ow"])
    with pytest.raises(ValueError, match="valid"):
        flow.reference(m, ["zeta"])


def test_okubo_weiss_and_strain_identity():
    """ow is strain2 - q_psi^2 of the very planes returned: bit for bit.  Read the other way, ow + q_psi^2 returns to strain2 up
    to the two roundings of (s - p) + p, 2 ulp of max(s, p) (in floating point that sum is not exact for arbitrary data)."""
    from niwqg_amd import flow
    nx, L = 64, 2 * np.pi
    rng = np.random.default_rng(3)
    psi = rng.standard_normal((nx, nx))
    ph = np.fft.fft2(psi)
    kk = shim(nx, L, None, None, None).kk
    q_psi = np.fft.ifft2(-(kk[None, :] ** 2 + kk[:, None] ** 2) * ph).real
    m = shim(nx, L, ph, np.fft.fft2(rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx))), q_psi)
    R = flow.reference(m)
    assert np.array_equal(R["ow"], R["strain2"] - q_psi * q_psi)
    assert np.array_equal(R["strain2"], R["sn"] * R["sn"] + R["ss"] * R["ss"])
    p = q_psi * q_psi
    assert np.all(np.abs((R["ow"] + p) - R["strain2"]) <= 2 * 2.0 ** -52 * np.maximum(R["strain2"], p))
    assert (R["strain2"] >= 0).all() and (R["gradphi2"] >= 0).all()


class _Kernel(object):
    pass


def test_linked_calls_are_refused_where_a_thread_holds_one_value():
    """at nx = 8192 every flow name runs in a launch of its own: a joint table or a product of two different names is refused,
    everything else is not"""
    from niwqg_amd import _lib, flow
    m = _Kernel()
    m._ctx = _lib.Context.__new__(_lib.Context)          # a single-GPU context as far as isinstance goes; never opened
    m._ctx.h = None
    for nx, linked, refused in ((8192, True, True), (8192, False, False), (4096, True, False), (64, True, False)):
        m.nx = nx
        if refused:
            with pytest.raises(NotImplementedError, match="8192"):
                flow.refuse(m, "field_pdfs", linked=linked)
        else:
            flow.refuse(m, "field_pdfs", linked=linked)
    m.nx = 8192
    from niwqg_amd import averages, pdfs
    with pytest.raises(NotImplementedError, match="joint table"):
        pdfs._validate(m, ["ow", "phi2"], 16, None, ("ow", "phi2"), 8)
    assert pdfs._validate(m, ["ow", "phi2"], 16, None, None, 8)[0] == ["ow", "phi2"]
    with pytest.raises(NotImplementedError, match="product"):
        averages.attach(m, ("ow", "phi2"), (("ow", "phi2"),))


def test_available_lists_are_unchanged_and_flow_names_are_by_name_only():
    from niwqg_amd import averages, flow, pdfs
    m = _Kernel()
    assert pdfs.available(m) == ["q", "q_psi", "phi2"]
    assert averages.available(m) == ["q", "q_psi", "phi2", "phi"]
    assert flow.available(m) == list(flow.NAMES) == ["u", "v", "sn", "ss", "strain2", "ow", "gradphi2"]
    assert not set(flow.NAMES) & set(pdfs.available(m)) and "zeta" not in flow.NAMES
    from niwqg_amd import _lib
    assert [flow.CODES[n] for n in flow.NAMES] == list(range(16, 23)) == [_lib.FLOW_U, _lib.FLOW_V, _lib.FLOW_SN, _lib.FLOW_SS,
                                                                          _lib.FLOW_STRAIN2, _lib.FLOW_OW, _lib.FLOW_GRADPHI2]
    assert pdfs._CODES["ow"] == averages._CODES["ow"] == 21


def test_unknown_name_errors_keep_their_text():
    from niwqg_amd import averages, pdfs
    m = _Kernel()
    with pytest.raises(ValueError, match="q, q_psi, phi2") as e:
        pdfs._validate(m, ["zeta"], 16, None, None, 8)
    assert "ow" in str(e.value)
    a = _Kernel()
    a._any_size = True
    with pytest.raises(ValueError, match="1 to 3"):
        pdfs._validate(a, ["q", "u", "v", "ow"], 16, None, None, 8)
    assert pdfs._validate(a, ["ss", "phi2"], 16, None, ("ss", "phi2"), 8)[0] == ["ss", "phi2"]
    with pytest.raises(ValueError, match="q, q_psi, phi2"):
        averages.check(averages.available(m), ["zeta"])
    with pytest.raises(ValueError, match="at most 3 real"):
        averages.check(averages.available(m) + list(__import__("niwqg_amd").flow.NAMES), ["q", "u", "v", "ow", "phi"])
    f, p, e = averages.check(averages.available(m) + ["ow", "gradphi2"], ["ow", "gradphi2", "phi"], [("ow", "gradphi2")], 2)
    assert f == ("ow", "gradphi2", "phi") and p == (("ow", "gradphi2"),) and e == 2
