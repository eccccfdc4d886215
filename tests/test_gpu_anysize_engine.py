"""The any-size engine's C ABI (include/niwqg_amd.h: nq_any_*; csrc/nq_anysize.hpp) against numpy in float64 / complex128.

The model classes only ever drive the engine with one square length; these tests call its primitives directly: element counts
between the grid-stride caps, aliased operands, non-finite data, non-square planes, several transform lengths on one engine, the
fallback code paths, the helper kernels and the limits.
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
COUNTS = [1, 255, 257, 256 * 4096 - 1, 256 * 4096 + 3]          # the last crosses k_any_ew's 4096-block grid-stride cap
RCOUNTS = COUNTS + [256 * 1024 + 7]                             # ... and k_any_reduce1's 1024-block cap
# (rows, cols, axis): every plan kind along axis 0 and axis 1 of non-square planes
#   Bluestein (M = 64 .. 512): 2, 3, 7, 127, 250;  direct: 64, 4096, 8192;  split 3 m / 5 m: 192, 320, 6144;
#   Bluestein on four-step 16384 rows: 4097, 8191
FFT_CASES = [(2, 96, 1), (96, 2, 0), (3, 100, 1), (7, 3000, 0), (3000, 7, 1), (127, 40, 0), (96, 250, 1), (250, 96, 0),
             (64, 18, 0), (10, 64, 1), (4096, 3, 0), (5, 4096, 1), (8192, 2, 0), (2, 8192, 1), (192, 33, 0), (9, 192, 1),
             (320, 12, 0), (17, 320, 1), (6144, 6, 0), (6, 6144, 1), (4097, 2, 0), (3, 4097, 1), (8191, 2, 0), (2, 8191, 1)]


def fft_bound(n):
    return 5e-15 * max(1.0, np.log2(max(n, 2)) / 4)


@pytest.fixture(scope="module")
def eng():
    from niwqg_amd import _anysize
    e = _anysize.Engine(0)
    yield e
    e.close()


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _raw(e, elems):
    """a bare device plane of this engine (freed with the engine)"""
    p = ctypes.c_void_p()
    e.chk(e.L.nq_any_alloc(e.h, int(elems), ctypes.byref(p)), "nq_any_alloc")
    return p.value


def _up(e, ptr, a):
    from niwqg_amd import _lib
    buf = np.ascontiguousarray(a, np.complex128)
    e.chk(e.L.nq_any_upload(e.h, ptr, _lib._dptr(buf.view(np.float64)), buf.size), "nq_any_upload")


def _down(e, ptr, shape):
    from niwqg_amd import _lib
    out = np.empty(shape, np.complex128)
    e.chk(e.L.nq_any_download(e.h, ptr, _lib._dptr(out.view(np.float64)), out.size), "nq_any_download")
    return out


def _sc(s0=1.0, s1=0.0, s2=0.0):
    return (ctypes.c_double * 6)(s0.real, s0.imag, s1.real, s1.imag, s2.real, s2.imag)


def _rel_rows(got, want, axis):
    """error of the 1-D transforms relative to the plane's norm (the measure of test_gpu_anysize.py)"""
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


# ---- B1: nq_any_ew ------------------------------------------------------------------------------------------------------
EW = ["COPY", "MUL", "MULCONJ", "AXPBY", "AXPBYPCZ", "REAL", "ABS2", "SCALE", "CONJ", "ADDS", "IMAG", "MULADD", "FILL"]
EXACT = {"COPY", "CONJ", "REAL", "IMAG", "FILL", "ADDS"}      # one rounding (or none): bit-exact


class _X(object):
    """complex values as (re, im) in long double: the numpy restatement of an op rounds far below the device's double"""

    def __init__(self, re, im):
        self.re, self.im = re, im

    @staticmethod
    def of(z):
        z = np.asarray(z, np.complex128)
        return _X(z.real.astype(np.longdouble), z.imag.astype(np.longdouble))

    def __mul__(self, o):
        return _X(self.re * o.re - self.im * o.im, self.re * o.im + self.im * o.re)

    def __add__(self, o):
        return _X(self.re + o.re, self.im + o.im)

    def conj(self):
        return _X(self.re, -self.im)

    def c128(self):
        return self.re.astype(np.float64) + 1j * self.im.astype(np.float64)


def _ew_numpy(op, a, b, c, s0, s1, s2):
    """the formula of include/niwqg_amd.h (exact ops in complex128, the others in long double), and the magnitude of its terms
    (for the rounding bound)"""
    A, B, C = np.abs(a), np.abs(b), np.abs(c)
    xa, xb, xc, x0, x1, x2 = _X.of(a), _X.of(b), _X.of(c), _X.of(s0), _X.of(s1), _X.of(s2)
    r = {"COPY": (a, A), "MUL": (x0 * (xa * xb), abs(s0) * A * B), "MULCONJ": (x0 * (xa.conj() * xb), abs(s0) * A * B),
         "AXPBY": (x0 * xa + x1 * xb, abs(s0) * A + abs(s1) * B),
         "AXPBYPCZ": (x0 * xa + x1 * xb + x2 * xc, abs(s0) * A + abs(s1) * B + abs(s2) * C),
         "REAL": (a.real + 0j, A), "ABS2": (_X(xa.re * xa.re + xa.im * xa.im, 0 * xa.re), A * A), "SCALE": (x0 * xa, abs(s0) * A),
         "CONJ": (np.conj(a), A), "ADDS": (a + s0, A + abs(s0)), "IMAG": (a.imag + 0j, A),
         "MULADD": (x0 * (xa * xb) + x1 * xc, abs(s0) * A * B + abs(s1) * C),
         "FILL": (np.full_like(a, s0), np.full(a.shape, abs(s0)))}
    want, mag = r[op]
    return (want.c128() if isinstance(want, _X) else want), mag


@pytest.mark.parametrize("n", COUNTS)
def test_elementwise_ops_against_numpy_with_aliasing(eng, n):
    """all 13 ops on random operands; the output separate and aliased to a, b and c (the header promises it): bit-exact where the
    op is one rounding, otherwise within 4 eps of the operand magnitudes (the device may contract into FMAs)"""
    e, L = eng, eng.L
    rng = np.random.default_rng(n)
    a, b, c = _rand(rng, n), _rand(rng, n), _rand(rng, n)
    s0, s1, s2 = complex(*rng.standard_normal(2)), complex(*rng.standard_normal(2)), complex(*rng.standard_normal(2))
    pa, pb, pc, pd = (_raw(e, n) for _ in range(4))
    for op_i, op in enumerate(EW):
        want, mag = _ew_numpy(op, a, b, c, s0, s1, s2)
        for alias in ("none", "a", "b", "c"):
            _up(e, pa, a)
            _up(e, pb, b)
            _up(e, pc, c)
            d = {"none": pd, "a": pa, "b": pb, "c": pc}[alias]
            e.chk(L.nq_any_ew(e.h, op_i, d, pa, pb, pc, n, _sc(s0, s1, s2)), "nq_any_ew")
            got = _down(e, d, n)
            if op in EXACT:
                assert np.array_equal(got.view(np.float64), want.view(np.float64)), (op, alias, n)
            else:
                err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
                assert np.all(err <= 4 * EPS * mag), (op, alias, n, float(np.max(err / mag)))
    # EW_FILL never reads a: a plane full of NaN becomes the fill value
    _up(e, pa, np.full(n, np.nan + 1j * np.nan))
    e.chk(L.nq_any_ew(e.h, EW.index("FILL"), pa, pa, None, None, n, _sc(2.5 - 1j)), "nq_any_ew")
    assert np.all(_down(e, pa, n) == 2.5 - 1j)
    e.sync()


# ---- B2: nq_any_reduce --------------------------------------------------------------------------------------------------
RD = ["SUM", "SUMABS2", "DOT", "DOTC", "MAXABS", "WSUMABS2", "MAXABSRE"]


def _rd_terms(op, a, b):
    return {"SUM": a, "SUMABS2": np.abs(a) ** 2 + 0j, "DOT": a * b, "DOTC": np.conj(a) * b,
            "WSUMABS2": b.real * (a.real * a.real + a.imag * a.imag) + 0j}[op]


def _rd_mag(op, a, b):
    """the magnitudes of each term's products, real and imaginary parts apart (the rounding bound under cancellation)"""
    ar, ai, br, bi = np.abs(a.real), np.abs(a.imag), np.abs(b.real), np.abs(b.imag)
    return {"SUM": (ar, ai), "SUMABS2": (ar * ar + ai * ai, 0 * ar), "DOT": (ar * br + ai * bi, ar * bi + ai * br),
            "DOTC": (ar * br + ai * bi, ar * bi + ai * br), "WSUMABS2": (br * (ar * ar + ai * ai), 0 * ar)}[op]


def _reduce(e, op, pa, pb, n):
    out = np.zeros(2)
    from niwqg_amd import _lib
    e.chk(e.L.nq_any_reduce(e.h, RD.index(op), pa, pb, n, _lib._dptr(out)), "nq_any_reduce")
    return out


@pytest.mark.parametrize("n", RCOUNTS)
def test_reductions_against_fsum_and_numpy_propagation(eng, n):
    """sums and dots within 4 log2(n) eps sum|terms| of math.fsum (real and imaginary parts apart), maxima exact, two calls
    bit-identical; NaN, +inf and -inf at the first, the last index and in the tail block follow numpy's propagation"""
    e = eng
    rng = np.random.default_rng(1000 + n)
    a, b = _rand(rng, n), _rand(rng, n)
    pa, pb = _raw(e, n), _raw(e, n)
    _up(e, pa, a)
    _up(e, pb, b)
    for op in RD:
        got = _reduce(e, op, pa, pb, n)
        assert np.array_equal(got, _reduce(e, op, pa, pb, n)), op
        if op == "MAXABS":              # (sqrt(x^2 + y^2) on the device, hypot in numpy: the same element, within an ulp)
            assert abs(got[0] - np.max(np.abs(a))) <= 2 * EPS * got[0], op
        elif op == "MAXABSRE":
            assert got[0] == np.max(np.abs(a.real)), op
        else:
            t = _rd_terms(op, a, b)
            bound = 4 * max(1.0, math.log2(n)) * EPS
            mr, mi = _rd_mag(op, a, b)
            assert abs(got[0] - math.fsum(t.real)) <= bound * math.fsum(mr), op
            assert abs(got[1] - math.fsum(t.imag)) <= bound * math.fsum(mi), op
    # non-finite values: numpy's propagation (a NaN term makes every sum and maximum NaN; an inf an inf)
    for idx in sorted({0, n - 1, max(0, n - 100)}):
        for bad in (np.nan, np.inf, -np.inf):
            x = a.copy()
            x[idx] = bad + 0j if not np.isnan(bad) else complex(np.nan, 0.0)
            _up(e, pa, x)
            with np.errstate(all="ignore"):
                for op in RD:
                    got = _reduce(e, op, pa, pb, n)
                    if op == "MAXABS":
                        want = (np.max(np.abs(x)), 0.0)
                    elif op == "MAXABSRE":
                        want = (np.max(np.abs(x.real)), 0.0)
                    else:
                        t = _rd_terms(op, x, b)
                        want = (np.sum(t.real), np.sum(t.imag))
                    for g, w in zip(got, want):
                        assert np.isnan(g) == np.isnan(w), (op, idx, bad, got, want)
                        if not np.isnan(w) and np.isinf(w):
                            assert g == w, (op, idx, bad, got, want)
    e.sync()


# ---- B3: nq_any_fft -----------------------------------------------------------------------------------------------------
FFT_WORKER = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from niwqg_amd import _anysize
import test_gpu_anysize_engine as T
e = _anysize.Engine(0)
T.fft_matrix(e)
print("fft matrix agrees with numpy")
'''


def fft_matrix(e):
    """every case of FFT_CASES, forward and inverse, in place and out of place, against numpy.fft along that axis"""
    rng = np.random.default_rng(7)
    for rows, cols, axis in FFT_CASES:
        n = rows if axis == 0 else cols
        x = _rand(rng, (rows, cols))
        src, dst = _raw(e, rows * cols), _raw(e, rows * cols)
        for inverse in (0, 1):
            want = (np.fft.ifft if inverse else np.fft.fft)(x, axis=axis)
            for inplace in (False, True):
                _up(e, src, x)
                out = src if inplace else dst
                e.chk(e.L.nq_any_fft(e.h, out, src, rows, cols, axis, inverse), "nq_any_fft")
                got = _down(e, out, (rows, cols))
                err = _rel_rows(got, want, axis)
                assert err < fft_bound(n), (rows, cols, axis, inverse, inplace, err)
                if not inplace:
                    assert np.array_equal(_down(e, src, (rows, cols)), x), "out-of-place transform wrote its source"
        for p in (src, dst):
            e.chk(e.L.nq_any_free(e.h, p, rows * cols), "nq_any_free")


def test_transforms_of_every_plan_kind_on_non_square_planes(eng):
    fft_matrix(eng)


@pytest.mark.parametrize("switch", ["NIWQG_AMD_ANY_FUSED", "NIWQG_AMD_ANY_SPLIT"])
def test_transforms_on_the_fallback_code_paths(tmp_path, switch):
    """the unfused five-launch Bluestein form (NIWQG_AMD_ANY_FUSED=0) and Bluestein for 3 m / 5 m (NIWQG_AMD_ANY_SPLIT=0): the
    switches are read once into a static, hence a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "fft_fallback.py"
    script.write_text(FFT_WORKER % (root, os.path.join(root, "tests")))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **{switch: "0"}))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert "fft matrix agrees with numpy" in out.stdout


# ---- B4: transform lengths interleaved on one engine ------------------------------------------------------------------------
def test_a_new_length_after_a_queued_transform_leaves_it_intact():
    """an axis-0 transform of a 3000 x 3000 plane is queued (no sync), then the first transform of a length the engine has never
    seen (its plan build writes the engine's work rows), then the first result is downloaded: it must be numpy's.  Each new
    length once."""
    from niwqg_amd import _anysize
    e = _anysize.Engine(0)
    rng = np.random.default_rng(11)
    n = 3000
    x = _rand(rng, (n, n))
    want = np.fft.fft(x, axis=0)
    big, out = _raw(e, n * n), _raw(e, n * n)
    small = _raw(e, 4 * 8191)
    for new in (127, 250, 4097, 8191):
        _up(e, big, x)
        e.chk(e.L.nq_any_fft(e.h, out, big, n, n, 0, 0), "nq_any_fft")        # queued; its kernels read the work rows
        e.chk(e.L.nq_any_fft(e.h, small, small, 4, new, 1, 0), "nq_any_fft")  # a new plan: it must not write the work rows under it
        got = _down(e, out, (n, n))
        err = _rel_rows(got, want, 0)
        assert err < fft_bound(n), (new, err)
    e.close()


# ---- B6: helper kernels -----------------------------------------------------------------------------------------------
def _expand_numpy(half, n, project):
    rows, nh = half.shape
    full = np.empty((rows, n), np.complex128)
    lm = np.arange(rows) if project == 2 else (-np.arange(rows)) % rows
    full[:, :nh] = half
    if project:
        for k in (0, n // 2):
            m = half[lm, k]
            full[:, k] = 0.5 * (half[:, k].real + m.real) + 1j * (0.5 * (half[:, k].imag - m.imag))
    for k in range(nh, n):
        full[:, k] = np.conj(half[lm, n - k])
    return full


@pytest.mark.parametrize("rows,n", [(6, 10), (96, 250), (7, 4)])
def test_helper_kernels_against_their_header_comments(eng, rows, n):
    """nq_any_expand_half with project 0, 1, 2 on half planes whose self-mirrored columns are NOT Hermitian; nq_any_take_cols;
    nq_any_set_elem at the last index"""
    e = eng
    rng = np.random.default_rng(rows * n)
    nh = n // 2 + 1
    half = _rand(rng, (rows, nh))
    ph, pf = _raw(e, rows * nh), _raw(e, rows * n)
    _up(e, ph, half)
    for project in (0, 1, 2):
        e.chk(e.L.nq_any_expand_half(e.h, pf, ph, rows, n, project), "nq_any_expand_half")
        got = _down(e, pf, (rows, n))
        assert np.array_equal(got, _expand_numpy(half, n, project)), project
    src = _rand(rng, (rows, n))
    _up(e, pf, src)
    for dcols in (1, nh, n):
        pd = _raw(e, rows * dcols)
        e.chk(e.L.nq_any_take_cols(e.h, pd, pf, rows, n, dcols), "nq_any_take_cols")
        assert np.array_equal(_down(e, pd, (rows, dcols)), src[:, :dcols]), dcols
    e.chk(e.L.nq_any_set_elem(e.h, pf, rows * n - 1, 1.25, -3.5), "nq_any_set_elem")
    want = src.copy()
    want.flat[-1] = 1.25 - 3.5j
    assert np.array_equal(_down(e, pf, (rows, n)), want)


# ---- B7: limits fail loudly; B8: length 1 -------------------------------------------------------------------------------
def test_lengths_beyond_the_engine_fail_loudly_and_leave_it_usable(eng):
    e = eng
    rng = np.random.default_rng(3)
    p = _raw(e, 2 * 16385)
    for n in (8193, 12288, 16385):
        rc = e.L.nq_any_fft(e.h, p, p, 2, n, 1, 0)
        assert rc != 0, n
        assert str(n) in e.L.nq_any_last_error(e.h).decode(), n
        rc = e.L.nq_any_fft(e.h, p, p, n, 2, 0, 1)
        assert rc != 0, n
    assert e.L.nq_any_fft(e.h, p, p, 0, 5, 1, 0) != 0
    assert e.L.nq_any_fft(e.h, p, p, -3, 5, 0, 0) != 0
    x = _rand(rng, (3, 250))
    _up(e, p, x)
    e.chk(e.L.nq_any_fft(e.h, p, p, 3, 250, 1, 0), "nq_any_fft")
    assert _rel_rows(_down(e, p, (3, 250)), np.fft.fft(x, axis=1), 1) < fft_bound(250)


def test_length_one_is_the_identity(eng):
    """numpy.fft of length 1 is the identity; Kernel.fft of a (1, n) array reaches it"""
    e = eng
    rng = np.random.default_rng(5)
    for rows, cols, axis in ((1, 7, 0), (9, 1, 1), (1, 1, 0), (1, 1, 1)):
        x = _rand(rng, (rows, cols))
        src, dst = _raw(e, rows * cols), _raw(e, rows * cols)
        for inverse in (0, 1):
            _up(e, src, x)
            e.chk(e.L.nq_any_fft(e.h, dst, src, rows, cols, axis, inverse), "nq_any_fft")
            assert np.array_equal(_down(e, dst, (rows, cols)), x)
            e.chk(e.L.nq_any_fft(e.h, src, src, rows, cols, axis, inverse), "nq_any_fft")
            assert np.array_equal(_down(e, src, (rows, cols)), x)
    import niwqg_amd
    m = niwqg_amd.UnCoupledModel.Model(nx=96)
    a = _rand(rng, (1, 10))
    f = m.fft(a)
    assert np.abs(f - np.fft.fft2(a)).max() <= 1e-14 * np.abs(a).sum()
    assert np.abs(m.ifft(f) - a).max() <= 1e-14 * np.abs(a).sum()


# ---- two engines on two devices ---------------------------------------------------------------------------------------
def test_two_engines_on_two_devices_interleaved():
    """calls alternate between an engine on device 0 and one on device 1: every entry makes its own device current"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    from niwqg_amd import _anysize
    e0, e1 = _anysize.Engine(0), _anysize.Engine(1)
    rng = np.random.default_rng(9)
    xs = [_rand(rng, (96, 250)) for _ in range(2)]
    ps = [_raw(e, 96 * 250) for e in (e0, e1)]
    for e, p, x in zip((e0, e1), ps, xs):
        _up(e, p, x)
    for e, p in zip((e0, e1), ps):
        e.chk(e.L.nq_any_fft(e.h, p, p, 96, 250, 1, 0), "nq_any_fft")
        e.chk(e.L.nq_any_ew(e.h, EW.index("SCALE"), p, p, None, None, 96 * 250, _sc(2.0)), "nq_any_ew")
    for e, p, x in zip((e0, e1), ps, xs):
        assert _rel_rows(_down(e, p, (96, 250)), 2.0 * np.fft.fft(x, axis=1), 1) < fft_bound(250)
        assert _reduce(e, "MAXABS", p, None, 96 * 250)[0] == np.max(np.abs(_down(e, p, (96, 250))))
    e0.close()
    e1.close()
