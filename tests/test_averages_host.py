"""Time-mean and covariance maps, host side (niwqg_amd/averages.py): the accumulation rule's numpy restatement and the
statistics of ``result()`` against numpy's own mean and covariance, every refusal of the contract before any device call, and
the C ABI's names in the header and in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

from niwqg_amd import _lib, averages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = ["q", "q_psi", "phi2", "phi"]


class FakeKernelModel(object):
    """enough of a model for the argument checks: they must all fire before anything touches a context"""
    _ctx = None
    nx = 64


def random_samples(n=9, shape=(5, 7), seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        phi = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        q = 3.0 + rng.standard_normal(shape)
        out.append(dict(q=q, q_psi=q - 0.3 * np.abs(phi) ** 2, phi2=np.abs(phi) ** 2, phi=phi))
    return out


def test_accumulate_and_statistics_against_numpy():
    xs = random_samples()
    fields = ("q", "q_psi", "phi2", "phi")
    products = (("q_psi", "phi2"), ("phi2", "phi2"), ("q_psi", "q_psi"), ("q", "q"))
    shape = xs[0]["q"].shape
    sums = {n: np.zeros(shape, np.complex128 if n == "phi" else np.float64) for n in fields}
    sums.update({averages.product_key(a, b): np.zeros(shape) for a, b in products})
    for x in xs:
        assert averages.accumulate(sums, x) is sums
    # the rule itself: S <- S + x and S <- S + x y in sample order, bit for bit
    S, Sp = np.zeros(shape), np.zeros(shape)
    for x in xs:
        S = S + x["q_psi"]
        Sp = Sp + x["q_psi"] * x["phi2"]
    assert np.array_equal(S, sums["q_psi"]) and np.array_equal(Sp, sums["q_psi*phi2"])
    full = dict(sums)
    full.update({averages.product_key(b, a): sums[averages.product_key(a, b)] for a, b in products})
    R = averages.Averages(len(xs), 9, fields, products, full)
    stack = {n: np.array([x[n] for x in xs]) for n in fields}

    top = {n: np.abs(stack[n]).max() for n in fields}

    def close(got, want, scale):                       # 1e-13 relative to the largest magnitude that enters the statistic
        assert np.abs(got - want).max() <= 1e-13 * scale

    for n in fields:
        close(R.mean(n), stack[n].mean(axis=0), top[n])
    for n in ("q", "q_psi", "phi2"):
        close(R.variance(n), stack[n].var(axis=0), top[n] ** 2)
        assert np.array_equal(R.covariance(n, n), R.variance(n))
    a, b = stack["q_psi"].reshape(len(xs), -1), stack["phi2"].reshape(len(xs), -1)
    cov = np.array([np.cov(a[:, i], b[:, i], bias=True)[0, 1] for i in range(a.shape[1])]).reshape(shape)
    close(R.covariance("q_psi", "phi2"), cov, top["q_psi"] * top["phi2"])
    assert np.array_equal(R.covariance("phi2", "q_psi"), R.covariance("q_psi", "phi2"))
    # correlation = cov / sqrt(va vb): the three absolute errors above over the smallest variance product
    corr = np.array([np.corrcoef(a[:, i], b[:, i])[0, 1] for i in range(a.shape[1])]).reshape(shape)
    vmin = min(np.sqrt(a.var(axis=0) * b.var(axis=0)).min(), a.var(axis=0).min(), b.var(axis=0).min())
    close(R.correlation("q_psi", "phi2"), corr, 3 * max(top["q_psi"], top["phi2"]) ** 2 / vmin)
    assert R.sums["phi2*q_psi"] is R.sums["q_psi*phi2"]


def test_correlation_is_nan_where_a_variance_is_not_positive():
    one = np.ones((2, 2))
    R = averages.Averages(2, 2, ("q", "c"), (("q", "q"), ("c", "c"), ("q", "c")),
                          {"q": 2 * one, "c": np.array([[2.0, 4.0], [0.0, 6.0]]), "q*q": 2 * one, "c*c": np.array([[4.0, 10.0], [2.0, 20.0]]),
                           "q*c": 2 * one, "c*q": 2 * one})
    assert np.all(R.variance("q") == 0.0) and np.all(np.isnan(R.correlation("q", "c")))


def test_statistics_whose_sums_were_not_kept_raise_key_error():
    z = np.zeros((2, 2))
    R = averages.Averages(1, 1, ("q", "phi2"), (("q", "phi2"),), {"q": z, "phi2": z, "q*phi2": z, "phi2*q": z})
    R.covariance("phi2", "q")
    with pytest.raises(KeyError, match="products"):
        R.variance("q")
    with pytest.raises(KeyError, match="products"):
        R.correlation("q", "phi2")
    with pytest.raises(KeyError, match="fields"):
        R.mean("q_psi")


@pytest.mark.parametrize("kw", [
    dict(fields=["zeta"]), dict(fields=["q", "c"]), dict(fields=[]), dict(fields=["q", "q"]),
    dict(fields=["q"], products=[("q", "phi2")]), dict(fields=["q", "phi"], products=[("q", "phi")]),
    dict(fields=["phi"], products=[("phi", "phi")]), dict(fields=["q"], products=[("q",)]), dict(fields=["q"], products=["q"]),
    dict(fields=["q", "phi2"], products=[("q", "phi2"), ("phi2", "q")]), dict(fields=["q"], products=[("q", "q"), ("q", "q")]),
    dict(fields=["q"], every=-1), dict(fields=["q"], every=1.5), dict(fields=["q"], every=True), dict(fields=["q"], every="2"),
])
def test_value_errors_before_any_device_call(kw):
    with pytest.raises(ValueError, match="valid"):
        averages.attach(FakeKernelModel(), **kw)
    args = dict(products=(), every=1)
    args.update(kw)
    with pytest.raises(ValueError, match="averages.attach"):
        averages.check(KERNEL, **args)


def test_check_normalises_and_allows_the_largest_configuration():
    pairs = [(a, b) for i, a in enumerate(KERNEL[:3]) for b in KERNEL[i:3]]
    assert len(pairs) == averages.MAX_PRODUCTS
    f, p, e = averages.check(KERNEL, KERNEL, pairs, 0)
    assert f == tuple(KERNEL) and p == tuple(pairs) and e == 0
    assert averages.check(["q", "c"], "q", [["q", "q"]], np.int64(3)) == (("q",), (("q", "q"),), 3)


def test_available_slab_refusal_second_attach_and_detached_use():
    m = FakeKernelModel()
    assert averages.available(m) == KERNEL
    # a model whose context is not the single-GPU one (a slab-decomposed simulation's facade) is refused, after the argument checks
    with pytest.raises(NotImplementedError, match="slab"):
        averages.attach(m, fields=["q"])
    with pytest.raises(ValueError):
        averages.attach(m, fields=["q"], every=-1)
    # a second attach: refused before the path is even looked at
    m.__dict__["_averages"] = object()
    with pytest.raises(RuntimeError, match="already"):
        averages.attach(m, fields=["q"])
    # use after detach: Attachment._check, before anything else
    A = averages.Accumulator(None, ("q",), (), 1)
    for call in (A.sample, A.reset, A.result, A.info):
        with pytest.raises(RuntimeError, match="^averages: detached$"):
            call()
    A.detach()                                        # idempotent


def test_result_without_a_sample_raises():
    class NoSample(averages.Accumulator):
        def _info(self):
            return 0, 5

    with pytest.raises(RuntimeError, match="no sample"):
        NoSample(FakeKernelModel(), ("q",), (), 0).result()


def test_result_docstring_states_the_raw_moment_caveat():
    assert "raw-moment" in averages.Accumulator.result.__doc__ and "lose digits" in averages.Accumulator.result.__doc__


def test_after_step_order_ends_with_the_averages():
    import inspect
    from niwqg_amd import _attach
    assert '("_forcing", "_particles", "_frequency", "_averages")' in inspect.getsource(_attach.after_step)


def test_abi_names_in_header_and_library():
    L = _lib.lib()
    names = ("nq_avg_attach", "nq_avg_detach", "nq_avg_sample", "nq_avg_reset", "nq_avg_info", "nq_avg_read", "nq_any_moments")
    header = open(os.path.join(ROOT, "include", "niwqg_amd.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    for i, n in enumerate(("NQ_AVG_Q", "NQ_AVG_QPSI", "NQ_AVG_PHI2", "NQ_AVG_C", "NQ_AVG_PHI")):
        assert re.search(r"\b%s = %d\b" % (n, i), header) and getattr(_lib, n[3:]) == i
    # null contexts and engines are refused without a device
    f = (ctypes.c_int * 2)(0, 0)
    i3 = (ctypes.c_longlong * 3)()
    d = (ctypes.c_double * 4)()
    assert L.nq_avg_attach(None, 1, f, 1, f, 1) != 0
    assert L.nq_avg_detach(None) != 0
    assert L.nq_avg_sample(None) != 0
    assert L.nq_avg_reset(None) != 0
    assert L.nq_avg_info(None, i3) != 0
    assert L.nq_avg_read(None, 0, d) != 0
    assert L.nq_any_moments(None, 4, 1, None, f, None, 0, None, None) != 0
