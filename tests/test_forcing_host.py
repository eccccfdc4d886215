"""CPU-only checks of the stochastic-forcing module (niwqg_amd/forcing.py): the generator's known answers, the statistics and the
Hermitian rule of the numpy restatement of the noise, the normalisation of ``ring``, every refusal raised before the device is
touched, and the C entries exported, typed and declared in the header."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# counter, key -> output of Philox4x32-10
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_scalar(counter, key):
    """Philox4x32-10 on Python integers, written from the paper independently of the package"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return tuple(c)


def gaussian_scalar(x):
    n = (x[0] >> 5) * 2 ** 26 + (x[1] >> 6)
    u1 = 1.0 - n * 2.0 ** -53
    u2 = (x[2] + 0.5) * 2.0 ** -32
    return np.sqrt(-np.log(u1)) * (np.cos(2 * np.pi * u2) + 1j * np.sin(2 * np.pi * u2))


def _fake(module, **attrs):
    cls = __import__("niwqg_amd." + module, fromlist=["Model"]).Model
    m = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


class _NoDevice(object):
    """a context any use of which fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the device was touched: %s" % name)


def _grid(n=16, L=2 * np.pi * 200e3):
    dk = 2 * np.pi / L
    ll = dk * np.append(np.arange(0., n / 2), np.arange(-n / 2, 0.))
    return dict(nx=n, ny=n, L=L, kk=ll.copy(), ll=ll, dk=dk, M=n * n)


def _models(n=16):
    return [_fake(mod, _ctx=_NoDevice(), tc=0, t=0.0, **_grid(n)) for mod in ("CoupledModel", "UnCoupledModel", "YBJModel", "QGModel")]


def test_known_answers():
    from niwqg_amd import forcing
    for counter, key, want in KNOWN:
        assert philox_scalar(counter, key) == want
        got = forcing.philox(counter, key)
        assert tuple(int(v) for v in got) == want


def test_noise_is_the_contracts_function_of_the_philox_words():
    from niwqg_amd import forcing
    seed = (0x299f31d0 << 32) | 0xa4093822
    for l, k, s, stream in ((0, 0, 0, 0), (3, 7, 2, 1), (127, 64, 2 ** 31, 0), (5, 0, 4294967295, 1)):
        x = philox_scalar((l, k, s, stream), (seed & 0xFFFFFFFF, seed >> 32))
        z = complex(forcing.noise(l, k, s, stream, seed))
        assert abs(z - gaussian_scalar(x)) <= 1e-15 * max(1.0, abs(z))
    # vectorised draws are the scalar ones
    l, k = np.arange(5)[:, None], np.arange(4)[None, :]
    z = forcing.noise(l, k, 9, 1, 77)
    assert z.shape == (5, 4)
    assert z[3, 2] == forcing.noise(3, 2, 9, 1, 77)
    # u1 = 1 (n = 0) is finite: xi = 0
    assert np.isfinite(gaussian_scalar((0, 0, 0, 0)))


def test_noise_statistics():
    from niwqg_amd import forcing
    l, k = np.arange(128)[:, None], np.arange(65)[None, :]
    for step, stream, seed in ((0, 0, 0), (1, 1, 1), (2 ** 31, 0, 2 ** 63 + 5)):
        z = forcing.noise(l, k, step, stream, seed)
        n = z.size
        assert abs(np.mean(np.abs(z) ** 2) - 1.0) <= 4.0 / np.sqrt(n)
        assert abs(np.mean(z)) <= 4.0 / np.sqrt(n)
    # different steps, streams and seeds give different planes
    a = forcing.noise(l, k, 0, 0, 0)
    for other in (forcing.noise(l, k, 1, 0, 0), forcing.noise(l, k, 0, 1, 0), forcing.noise(l, k, 0, 0, 1), forcing.noise(l, k, 0, 0, 1 << 32)):
        assert not np.any(a == other)


def test_hermitian_rule():
    from niwqg_amd import forcing
    n = 32
    z = forcing.noise_plane(n, 3, 0, 11)
    assert z.shape == (n, n // 2 + 1)
    assert not z[n // 2, :].any() and not z[:, n // 2].any() and z[0, 0] == 0
    raw = forcing.noise(np.arange(n)[:, None], np.arange(n // 2 + 1)[None, :], 3, 0, 11)
    for l in range(1, n // 2):
        assert z[l, 0] == raw[l, 0]
        assert z[n - l, 0] == np.conj(raw[l, 0])
    assert np.array_equal(z[:n // 2, 1:n // 2], raw[:n // 2, 1:n // 2]) and np.array_equal(z[n // 2 + 1:, 1:n // 2], raw[n // 2 + 1:, 1:n // 2])
    # the Hermitian extension is a real field
    full = np.zeros((n, n), complex)
    full[:, :n // 2 + 1] = z
    full[:, n // 2 + 1:] = np.conj(np.roll(z[::-1, 1:n // 2], 1, axis=0))[:, ::-1]
    f = np.fft.ifft2(full)
    assert np.max(np.abs(f.imag)) <= 1e-15 * np.max(np.abs(f.real))
    w = forcing.noise_plane(n, 3, 1, 11)
    assert w.shape == (n, n) and np.all(w != 0)


@pytest.mark.parametrize("n", [64, 96, 128])
def test_ring_normalisation(n):
    from niwqg_amd import forcing
    m = _models(n)[0]
    dk, M2 = m.dk, float(n * n) ** 2
    eps = 3.7e-9
    A = forcing.ring(m, 16 * dk, 2 * dk, eps)
    assert A.shape == (n, n // 2 + 1) and np.all(A >= 0) and np.all(np.isfinite(A))
    assert not A[n // 2, :].any() and not A[:, n // 2].any() and A[0, 0] == 0
    assert np.array_equal(A[1:n // 2, 0], A[n // 2 + 1:, 0][::-1])
    wv2 = m.kk[None, :n // 2 + 1] ** 2 + m.ll[:, None] ** 2
    wv2[0, 0] = 1.0
    w = np.full(n // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    assert abs(0.5 * (w * A ** 2 / wv2).sum() / M2 - eps) <= 1e-13 * eps
    kap = np.sqrt(wv2)
    assert not A[np.abs(kap - 16 * dk) > 6 * dk * (1 + 1e-12)].any() and A[0, 16] > 0
    B = forcing.ring(m, 16 * dk, 2 * dk, eps, field="phi")
    assert B.shape == (n, n)
    assert not B[n // 2, :].any() and not B[:, n // 2].any() and B[0, 0] == 0
    assert abs(0.5 * (B ** 2).sum() / M2 - eps) <= 1e-13 * eps
    for bad in (dict(kf=-1.0), dict(width=0.0), dict(eps=np.nan), dict(field="c"), dict(kf=1e-3 * dk, width=1e-4 * dk)):
        kw = dict(kf=16 * dk, width=2 * dk, eps=eps)
        kw.update(bad)
        with pytest.raises(ValueError):
            forcing.ring(m, **kw)


def _planes(n):
    q = np.zeros((n, n // 2 + 1))
    q[2, 3] = 1.0
    phi = np.zeros((n, n))
    phi[1, 1] = 1.0
    return q, phi


def test_argument_errors_are_raised_before_the_device():
    from niwqg_amd import forcing
    n = 16
    q, phi = _planes(n)
    co, un, yb, qg = _models(n)
    for m in (co, un, yb, qg):
        with pytest.raises(ValueError, match="q, phi or both"):
            forcing.attach(m)
    for m in (co, un):
        for kw, match in ((dict(q=q[:, :-1]), "shape"), (dict(phi=phi[:-1]), "shape"), (dict(q=-q), ">= 0"), (dict(phi=np.full((n, n), np.nan)), "finite"),
                          (dict(q=np.full((n, n // 2 + 1), np.inf)), "finite"), (dict(q="x"), "real array"), (dict(q=q, seed=-1), "seed"),
                          (dict(q=q, seed=2 ** 64), "seed"), (dict(q=q, seed=1.5), "seed"), (dict(q=q, step0=-1), "step0"),
                          (dict(q=q, step0=0.5), "step0")):
            with pytest.raises(ValueError, match=match):
                forcing.attach(m, **kw)
        lop = q.copy()
        lop[3, 0] = 1.0                       # row 3 of column 0 without its mirror row
        with pytest.raises(ValueError, match="column 0"):
            forcing.attach(m, q=lop)
    with pytest.raises(ValueError, match="YBJModel"):
        forcing.attach(yb, q=q)
    with pytest.raises(ValueError, match="YBJModel"):
        forcing.attach(yb, q=q, phi=phi)
    with pytest.raises(ValueError, match="QGModel"):
        forcing.attach(qg, phi=phi)
    with pytest.raises(ValueError, match="QGModel"):
        forcing.attach(qg, q=q, phi=phi)


def test_second_attach_is_refused():
    from niwqg_amd import forcing
    m = _models()[0]
    m.__dict__["_forcing"] = object()
    with pytest.raises(ValueError, match="attached already"):
        forcing.attach(m, q=_planes(16)[0])


def test_slab_models_are_refused():
    from niwqg_amd import forcing
    from niwqg_amd.slab import SlabContext
    q, phi = _planes(16)
    for mod, kw in (("CoupledModel", dict(q=q, phi=phi)), ("QGModel", dict(q=q)), ("YBJModel", dict(phi=phi))):
        m = _fake(mod, _ctx=SlabContext.__new__(SlabContext), tc=0, t=0.0, **_grid(16))
        with pytest.raises(NotImplementedError, match="slab"):
            forcing.attach(m, **kw)
        assert "_forcing" not in m.__dict__


def test_forcing_entries_are_exported_and_typed():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    names = ("nq_forcing_attach", "nq_forcing_detach", "nq_forcing_apply", "nq_forcing_increment", "nq_forcing_state", "nq_any_forcing")
    header = open(os.path.join(ROOT, "include", "niwqg_amd.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert L.nq_forcing_attach.argtypes[3] is ctypes.c_ulonglong
    assert L.nq_forcing_attach.argtypes[4] is ctypes.c_longlong
    assert L.nq_any_forcing.argtypes[1] is ctypes.c_void_p and L.nq_any_forcing.argtypes[9] is ctypes.c_double
    # null contexts and engines are refused without a device
    x = (ctypes.c_double * 4)()
    assert L.nq_forcing_attach(None, x, None, 0, 0) != 0
    assert L.nq_forcing_detach(None) != 0
    assert L.nq_forcing_apply(None) != 0
    assert L.nq_forcing_increment(None, 0, 0, x) != 0
    assert L.nq_forcing_state(None, x) != 0
    assert L.nq_any_forcing(None, None, None, 8, 8, 1, 0, 0, 1, 1.0, None, None) == -1


def test_module_is_importable_like_particles():
    from niwqg_amd import forcing
    for name in ("attach", "ring", "noise", "noise_plane", "philox", "Forcing"):
        assert hasattr(forcing, name)
