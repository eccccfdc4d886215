"""PDFs of the physical fields, host side (niwqg_amd/pdfs.py): the bin rule's numpy restatement against numpy.histogram (away
from the edges, where the two rules may differ by design) and on the real reference's fields, the arithmetic of density /
moments / conditional_mean on hand-made tables, and every ValueError of the contract before any device call."""
import os

import numpy as np
import pytest

from niwqg_amd import pdfs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def near_edges(x, lo, hi, bins, delta):
    """how many values lie within delta of an edge of np.linspace(lo, hi, bins + 1)"""
    e = np.linspace(lo, hi, bins + 1)
    i = np.clip(np.searchsorted(e, x), 1, bins)
    return int((np.minimum(np.abs(x - e[i - 1]), np.abs(x - e[i])) <= delta).sum())


def counts_of(x, lo, hi, bins):
    """[below, counts..., above, nan] by the restatement"""
    return np.bincount(pdfs.bin_index(np.ravel(x), lo, hi, bins) + 1, minlength=bins + 3)


def test_bin_index_rule():
    lo, hi, bins = -1.0, 3.0, 8
    x = np.array([-1.0, 3.0, -1.0000001, 3.0000001, np.nan, np.inf, -np.inf, 0.0, -0.0, 2.9999999, -0.5, 1.0])
    assert pdfs.bin_index(x, lo, hi, bins).tolist() == [0, 7, -1, 8, 9, 8, -1, 2, 2, 7, 1, 4]
    assert pdfs.bin_index(x, lo, hi, bins).dtype == np.int64
    # every interior edge belongs to the bin on its right here (exact arithmetic: powers of two)
    e = np.linspace(lo, hi, bins + 1)
    assert pdfs.bin_index(e, lo, hi, bins).tolist() == list(range(bins)) + [bins - 1]
    # a product that rounds up to `bins` is clamped into the last bin: s = 10 / 0.1 is rounded up, and so is x * s for x just below hi
    lo, hi, bins = 0.0, 0.1, 10
    x = np.nextafter(0.1, 0.0)
    assert x < hi and np.floor((x - lo) * (bins / (hi - lo))) == bins
    assert pdfs.bin_index(x, lo, hi, bins) == bins - 1
    assert pdfs.bin_index(np.float64(0.25), 0.0, 1.0, 1) == 0            # one bin


@pytest.mark.parametrize("bins", [1, 7, 64, 256, 1024])
def test_bin_index_equals_numpy_histogram_away_from_edges(bins):
    rng = np.random.default_rng(11)
    x = rng.standard_normal(100000)
    span = x.max() - x.min()
    lo, hi = x.min() - 0.01 * span, x.max() + 0.01 * span
    e = np.linspace(lo, hi, bins + 1)
    i = np.clip(np.searchsorted(e, x), 1, bins)
    far = np.minimum(np.abs(x - e[i - 1]), np.abs(x - e[i])) > 1e-9 * (hi - lo)
    assert far.sum() > 99000
    ref = np.searchsorted(e, x[far], side="right") - 1                   # numpy.histogram's rule for interior values
    assert np.array_equal(pdfs.bin_index(x[far], lo, hi, bins), ref)
    assert np.array_equal(np.bincount(ref, minlength=bins), np.histogram(x[far], bins=bins, range=(lo, hi))[0])


@pytest.mark.parametrize("bins", [64, 256])
def test_restatement_on_the_reference_fields(bins):
    g = np.load(os.path.join(GOLDEN, "g2_coupled_128_filter.npz"))
    for x in (g["q_100"], np.abs(g["phi_100"]) ** 2):
        span = x.max() - x.min()
        lo, hi = x.min() - 0.01 * span, x.max() + 0.01 * span
        assert near_edges(x.ravel(), lo, hi, bins, 1e-9 * (hi - lo)) == 0
        c = counts_of(x, lo, hi, bins)
        assert c[0] == c[-2] == c[-1] == 0
        assert np.array_equal(c[1:-2], np.histogram(x, bins=bins, range=(lo, hi))[0])


def hand_made():
    counts = {"a": np.array([1, 3, 0, 4], np.int64)}
    edges = {"a": np.linspace(0.0, 8.0, 5)}
    J = pdfs.JointTable(("a", "b"), np.array([[1, 0, 2], [3, 0, 0]], np.int64).repeat(1, axis=0), np.linspace(0.0, 3.0, 4),
                        np.linspace(10.0, 14.0, 3), 5)
    return pdfs.FieldPDFs(counts, edges, {"a": 2}, {"a": 0}, {"a": 1}, J)


def test_density_moments_conditional_mean():
    h = hand_made()
    d = h.density("a")
    assert np.allclose(d, np.array([1, 3, 0, 4]) / (8.0 * 2.0))
    assert abs((d * np.diff(h.edges["a"])).sum() - 1.0) < 1e-15
    c = np.array([1.0, 3.0, 5.0, 7.0])
    n = np.array([1.0, 3.0, 0.0, 4.0])
    mean = (n * c).sum() / 8
    var = (n * (c - mean) ** 2).sum() / 8
    mo = h.moments("a")
    assert np.allclose(mo, [mean, var, (n * (c - mean) ** 3).sum() / 8 / var ** 1.5, (n * (c - mean) ** 4).sum() / 8 / var ** 2])
    cm = h.conditional_mean()
    # joint counts [index of b][index of a]: a-bin 0 holds 1 point at b = 11 and 3 at b = 13; a-bin 1 is empty; a-bin 2: 2 at 11
    assert cm.counts.tolist() == [4, 0, 2]
    assert cm.mean[0] == (1 * 11.0 + 3 * 13.0) / 4 and np.isnan(cm.mean[1]) and cm.mean[2] == 11.0
    assert np.allclose(cm.centres, [0.5, 1.5, 2.5])
    h.joint = None
    with pytest.raises(ValueError):
        h.conditional_mean()


class FakeKernelModel(object):
    """enough of a model for the argument checks: they must all fire before anything touches a context"""
    _ctx = None
    nx = 64


@pytest.mark.parametrize("kw", [
    dict(names=["zeta"]), dict(names=["q", "c"]), dict(names=[]), dict(names=["q", "q"]),
    dict(bins=0), dict(bins=1025), dict(bins=2048), dict(bins=12.5),
    dict(joint=("q_psi", "phi2"), joint_bins=0), dict(joint=("q_psi", "phi2"), joint_bins=129),
    dict(joint=("q", "q")), dict(joint=("q", "c")), dict(joint=("q",)), dict(names=["q"], joint=("q", "phi2")),
    dict(ranges={"q": (1.0, 1.0)}), dict(ranges={"q": (2.0, 1.0)}), dict(ranges={"q": (0.0, np.inf)}),
    dict(ranges={"q": (np.nan, 1.0)}), dict(ranges={"q": 3.0}), dict(ranges={"zeta": (0.0, 1.0)}),
    dict(names=["q"], ranges={"phi2": (0.0, 1.0)}),
])
def test_value_errors_before_any_device_call(kw):
    with pytest.raises(ValueError) as e:
        pdfs.field_pdfs(FakeKernelModel(), **kw)
    assert "valid" in str(e.value) or "range" in str(e.value)
    args = dict(kw)
    args.setdefault("ranges", {"q": (0.0, 1.0), "q_psi": (0.0, 1.0), "phi2": (0.0, 1.0)})
    with pytest.raises(ValueError):
        pdfs.Accumulator(FakeKernelModel(), **args)


def test_accumulator_needs_every_range():
    with pytest.raises(ValueError) as e:
        pdfs.Accumulator(FakeKernelModel(), ranges={"q": (0.0, 1.0)})
    assert "mandatory" in str(e.value)
    with pytest.raises(ValueError):
        pdfs.Accumulator(FakeKernelModel(), ranges=None, names=["q"])


def test_available_and_slab_refusal():
    assert pdfs.available(FakeKernelModel()) == ["q", "q_psi", "phi2"]
    # a model whose context is not the single-GPU one (a slab-decomposed simulation's facade) is refused, after the argument checks
    with pytest.raises(NotImplementedError):
        pdfs.field_pdfs(FakeKernelModel())
    with pytest.raises(ValueError):
        pdfs.field_pdfs(FakeKernelModel(), bins=0)
