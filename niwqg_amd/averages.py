"""Time-mean and covariance maps of the physical fields, accumulated on the device inside the step.

    from niwqg_amd import averages
    A = averages.attach(m, fields=("q_psi", "phi2"), products=(("q_psi", "phi2"), ("phi2", "phi2")), every=1)
    m.run()                                   # every `every`-th step ends with one sample, batched or not
    R = A.result()                            # one download of the sum planes
    R.n; R.mean("phi2"); R.variance("phi2"); R.covariance("q_psi", "phi2"); R.correlation("q_psi", "phi2"); R.sums["q_psi*phi2"]
    A.sample()                                # add the current state now
    A.reset()                                 # zero the sums and n (not the step counter)
    A.detach()

Fields: ``q``, ``q_psi``, ``phi2`` (= |phi|^2) and ``phi`` (complex, as ``m.phi``) on CoupledModel, UnCoupledModel and YBJModel;
``q`` and, with its passive scalar, ``c`` on QGModel (``available(m)``).  The values are those ``pdfs.field_pdfs`` bins: the rows of
the last inversion (dual-copy contexts: the mean of the two q-hat copies), so ``set_phi`` after ``set_q`` leaves ``q_psi``
wave-free until the first step exactly as it does ``m.q_psi`` (quirk Q2); after a forced step they are the forced, re-inverted
state.  ``products`` are unordered pairs of real field names, each of which must also be in ``fields`` (a pair of one name: its
second moment); ``phi`` takes no part in them.

The accumulation rule (``accumulate`` restates it in numpy): every sample does S <- S + x, products S <- S + x y, in fp64, in
sample order, one device thread per point.  No atomics and no reduction: two runs are bit-identical and a first-moment plane is
the sequential fp64 sum exactly.  The device may contract S + x y into one fused multiply-add, one rounding less per sample
than numpy's, so product planes are not promised to equal numpy's bit for bit.  Non-finite values propagate as IEEE addition
does; nothing is checked per sample.

A sample is taken after every ``every``-th step since attach (``every = 0``: never automatically), after the forcing, the
particles and the recorder.  Attach itself takes none.
"""
import ctypes

import numpy as np

from . import _attach, _lib, flow, pdfs

_CODES = {"q": _lib.AVG_Q, "q_psi": _lib.AVG_QPSI, "phi2": _lib.AVG_PHI2, "c": _lib.AVG_C, "phi": _lib.AVG_PHI}
_CODES.update(flow.CODES)           # the flow fields (flow.py): taken by name only
MAX_PRODUCTS = 6
MAX_REAL = 3                        # real fields of one attachment: the value registers of the row pass


def available(m):
    """names of the fields attach(m) can average for this model"""
    names = pdfs.available(m)
    return names if pdfs._is_qg(m) else names + ["phi"]


def product_key(a, b):
    """the key of the pair (a, b) in ``Averages.sums``, as given; the reversed key names the same plane"""
    return "%s*%s" % (a, b)


def accumulate(sums, values):
    """THE accumulation rule in numpy: one sample ``values`` {name: array} added to ``sums`` {name or "a*b": array}, in place:
    S <- S + x for a field, S <- S + x y for a product.  Returns ``sums``."""
    for key, S in sums.items():
        if "*" in key:
            a, b = key.split("*")
            S += np.asarray(values[a]) * np.asarray(values[b])
        else:
            S += np.asarray(values[key])
    return sums


def _integer(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check(valid, fields, products=(), every=1):
    """the arguments of ``attach`` checked against the names a model takes (``available(m)``); returns (fields, products, every)
    as tuples of names / of name pairs.  Every error is a ValueError, raised before anything reaches the library."""
    valid = list(valid)
    fields = [fields] if isinstance(fields, str) else list(fields)
    bad = [n for n in fields if n not in valid]
    if bad or not fields or len(set(fields)) != len(fields):
        raise ValueError("averages.attach: fields %r; valid names (each once): %s" % (fields, ", ".join(valid)))
    if len([n for n in fields if n != "phi"]) > MAX_REAL:
        raise ValueError("averages.attach: fields %r; valid: at most %d real fields (and phi)" % (fields, MAX_REAL))
    pairs, seen = [], set()
    for p in products:
        p = tuple(p) if not isinstance(p, str) else (p,)
        if len(p) != 2 or any(not isinstance(n, str) for n in p):
            raise ValueError("averages.attach: product %r; valid: a pair of names out of %s" % (p, ", ".join(fields)))
        if "phi" in p:
            raise ValueError("averages.attach: product %r; valid: pairs of real fields (phi is complex and takes no part in products)" % (p,))
        missing = [n for n in p if n not in fields]
        if missing:
            raise ValueError("averages.attach: product %r names %s, not in fields; valid: pairs out of %s"
                             % (p, ", ".join(map(repr, missing)), ", ".join(fields)))
        if frozenset(p) in seen:
            raise ValueError("averages.attach: the pair %r is listed twice; valid: every unordered pair once" % (p,))
        seen.add(frozenset(p))
        pairs.append(p)
    if not _integer(every) or every < 0:
        raise ValueError("averages.attach: every = %r; valid: an integer >= 0" % (every,))
    return tuple(fields), tuple(pairs), int(every)


class Averages(object):
    """What ``result()`` returns: n samples, steps since attach, ``sums`` {name: (ny, nx) float64 (phi: complex128), "a*b": the
    product plane (either order of the names)}.  The statistics are formed here from the sums by the raw-moment formulas

        mean = S / n        cov(a, b) = S_ab / n - (S_a / n)(S_b / n)        correlation = cov / sqrt(var var)

    which lose digits where |mean|^2 >> variance (the difference of two nearly equal numbers): a point whose field varies by one
    part in 10^8 around its mean has no correct digit left in its variance."""

    def __init__(self, n, steps, fields, products, sums):
        self.n, self.steps, self.fields, self.products, self.sums = n, steps, fields, products, sums

    def __repr__(self):
        return "Averages(n=%d, fields=%s, products=%s)" % (self.n, list(self.fields), list(self.products))

    def _field(self, name):
        if name not in self.fields:
            raise KeyError("averages: %r was not averaged; add it to fields (averaged: %s)" % (name, ", ".join(self.fields)))
        return self.sums[name]

    def _product(self, a, b):
        self._field(a)
        self._field(b)
        S = self.sums.get(product_key(a, b))
        if S is None:
            raise KeyError("averages: the sum of %s * %s was not kept; add (%r, %r) to products" % (a, b, a, b))
        return S

    def mean(self, name):
        return self._field(name) / self.n

    def covariance(self, a, b):
        return self._product(a, b) / self.n - self.mean(a) * self.mean(b)

    def variance(self, name):
        return self.covariance(name, name)

    def correlation(self, a, b):
        """cov / sqrt(var var); NaN where a variance is <= 0"""
        cov, va, vb = self.covariance(a, b), self.variance(a), self.variance(b)
        ok = (va > 0) & (vb > 0)
        out = np.full(cov.shape, np.nan)
        out[ok] = cov[ok] / np.sqrt(va[ok] * vb[ok])
        return out


class Accumulator(_attach.Attachment):
    """Averages attached to one model (``attach``); see the module's doc"""
    SLOT, LABEL = "_averages", "averages"
    ALREADY = (RuntimeError, "averages.attach: this model has averages attached already (detach them first)")
    NO_SLAB = ("averages.attach: slab-decomposed models have no averages yet (every rank would keep the rows it owns and the "
               "planes would be assembled at read-out; DESIGN.md section 7)")

    def __init__(self, m, fields, products, every):
        self.m, self.fields, self.products, self.every = m, fields, products, every

    def info(self):
        """{"n": samples in the sums, "steps": steps since attach}"""
        self._check()
        n, steps = self._info()
        return {"n": n, "steps": steps}

    def sample(self):
        """adds the current state to the sums now"""
        self._check()
        self._sample()

    def reset(self):
        """zeroes the sums and n; the step counter (and so the phase of ``every``) stays"""
        self._check()
        self._reset()

    def result(self):
        """One download of the sum planes -> Averages (n, steps, sums and the statistics formed from them on the host).  Those are
        raw-moment formulas, cov(a, b) = S_ab / n - (S_a / n)(S_b / n): they lose digits where |mean|^2 >> variance."""
        self._check()
        n, steps = self._info()
        if n == 0:
            raise RuntimeError("averages.result: no sample taken yet")
        planes = self._read()
        sums = dict(zip(self.fields, planes))
        for (a, b), S in zip(self.products, planes[len(self.fields):]):
            sums[product_key(a, b)] = sums[product_key(b, a)] = S
        return Averages(n, steps, self.fields, self.products, sums)


class _Fused(Accumulator):
    """fused contexts: the planes live in the library and nq_step adds to them (nq_avg_*)"""

    def __init__(self, m, fields, products, every):
        Accumulator.__init__(self, m, fields, products, every)
        self.ctx = m._ctx
        self.ctx.avg_attach([_CODES[n] for n in fields], [(_CODES[a], _CODES[b]) for a, b in products], every)

    def _info(self):
        return self.ctx.avg_info()[:2]

    def _sample(self):
        self.ctx.avg_sample()

    def _reset(self):
        self.ctx.avg_reset()

    def _read(self):
        return [self.ctx.avg_read(i, n == "phi") for i, n in enumerate(self.fields)] + \
               [self.ctx.avg_read(len(self.fields) + p) for p in range(len(self.products))]

    def _detach(self):
        self.ctx.avg_detach()


class _AnySize(Accumulator):
    """any-size path: the sums are engine planes; the model's _step_etdrk4 calls _after_step, a sample is one nq_any_moments
    launch on the planes ``field_pdfs`` reads there (m._pdf_planes) and on the model's phi"""

    def __init__(self, m, fields, products, every):
        Accumulator.__init__(self, m, fields, products, every)
        e = self.eng = m._eng
        self.size = int(m.nx) * int(m.nx)
        half = (self.size + 1) // 2                         # engine planes are complex: a real sum plane takes half the elements
        self.sums = [e.zeros((1, self.size if n == "phi" else half)) for n in fields]
        self.psums = [e.zeros((1, half)) for _ in products]
        self.rg = _attach.Ring(1, every)
        nf, npr = len(fields), len(products)
        self._sums_c = (ctypes.c_void_p * nf)(*[p.ptr for p in self.sums])
        self._psums_c = (ctypes.c_void_p * max(1, npr))(*[p.ptr for p in self.psums])
        self._pairs_c = (ctypes.c_int * max(1, 2 * npr))(*[fields.index(n) for p in products for n in p])

    def _info(self):
        return self.rg.count, self.rg.steps

    def _sample(self):
        e, m, nf = self.eng, self.m, len(self.fields)
        real = m._pdf_planes([n for n in self.fields if n != "phi"])
        src = [(m._d["phi"], 2) if n == "phi" else real[n] for n in self.fields]
        e.chk(e.L.nq_any_moments(e.h, self.size, nf, (ctypes.c_void_p * nf)(*[p.ptr for p, _ in src]), (ctypes.c_int * nf)(*[w for _, w in src]),
                                 self._sums_c, len(self.products), self._pairs_c, self._psums_c), "nq_any_moments")
        self.rg.count += 1

    def _after_step(self):
        if self.rg.tick():
            self._sample()

    def _reset(self):
        from ._anysize import EW_FILL
        for p in self.sums + self.psums:
            p._ew(EW_FILL, p, s0=0.0)
        self.rg.count = 0

    def _read(self):
        nx = int(self.m.nx)
        out = []
        for n, p in zip(self.fields + ("",) * len(self.psums), self.sums + self.psums):
            v = p.get()
            out.append(v.reshape(nx, nx) if n == "phi" else np.ascontiguousarray(v.view(np.float64).ravel()[:self.size].reshape(nx, nx)))
        return out

    def _detach(self):
        self.eng.sync()
        self.sums, self.psums = [], []


def attach(m, fields, products=(), every=1):
    """Attach running sums to model m (one set per model): a plane per name in ``fields`` (out of ``available(m)``) and per pair in
    ``products``, zero at attach, a sample after every ``every``-th step (0: only ``sample()``).  The largest configuration, four
    fields and six products, is eleven real planes: 88 bytes per grid point.  Argument errors raise ValueError before the device
    is touched, a second attach RuntimeError, slab-decomposed models NotImplementedError."""
    if any(n in flow.NAMES for n in ([fields] if isinstance(fields, str) else fields) if isinstance(n, str)):
        flow.refuse(m, "averages.attach", linked=any(len(set(p)) > 1 for p in products if not isinstance(p, str)))
    fields, products, every = check(available(m) + flow.available(m), fields, products, every)
    return _attach.attach(m, _AnySize, _Fused, fields, products, every)

