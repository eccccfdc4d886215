"""What the attachments of the step share: particles.py, forcing.py, frequency.py, averages.py and
timespectra.py each hang one object on a model, in a slot of its ``__dict__``, and every step of that model drives it -- inside ``nq_step`` on fused contexts
(csrc/nq_lib.hip: attachments_before_step / attachments_after_step), from ``_anysize._step_etdrk4`` through the two hooks
below on the any-size path.
"""
from . import _lib


class Ring(object):
    """host bookkeeping of a ring of ``cap`` records, one after every ``every``-th step (0: never); the library's RecordRing"""

    def __init__(self, cap, every):
        self.cap, self.every = cap, every
        self.count = self.steps = 0               # records written, steps since attach
        self.ring_step = [0] * cap                # steps since attach of each slot

    def slot(self):
        """where the next record goes"""
        return self.count % self.cap

    def held(self):
        return min(self.count, self.cap)

    def oldest(self, r):
        """slot of the r-th held record, oldest first"""
        return (self.count - self.held() + r) % self.cap

    def wrote(self):
        self.ring_step[self.slot()] = self.steps
        self.count += 1

    def tick(self):
        """one step done: is a record due?"""
        self.steps += 1
        return self.every > 0 and self.steps % self.every == 0


class Attachment(object):
    """Base of Particles, Forcing, Recorder and the Accumulators of the averages and the time-mean spectra: ``m`` is the model until ``detach``, then None"""
    SLOT = None           # the key in m.__dict__
    LABEL = None          # the prefix of the module's messages
    ALREADY = None        # (exception class, message) of a second attach
    NO_SLAB = None        # NotImplementedError's message on slab-decomposed models

    def _check(self):
        if self.m is None:
            raise RuntimeError("%s: detached" % self.LABEL)

    def detach(self):
        """frees every device buffer the attachment allocated"""
        if self.m is None:
            return
        try:
            self._detach()
        finally:
            self.m.__dict__.pop(self.SLOT, None)
            self.m = None


def attach(m, any_size, fused, *args):
    """the tail of the ``attach`` functions, after their argument checks: one attachment per slot, the any-size or the
    fused flavour by the model's path, none on slab contexts"""
    if m.__dict__.get(fused.SLOT) is not None:
        raise fused.ALREADY[0](fused.ALREADY[1])
    if getattr(m, "_any_size", False):
        A = any_size(m, *args)
    elif isinstance(m._ctx, _lib.Context):
        A = fused(m, *args)
    else:
        raise NotImplementedError(fused.NO_SLAB)
    m.__dict__[fused.SLOT] = A
    return A


# ---- the hooks of an any-size step: the order is nq_step's (csrc/nq_lib.hip, attachments_before_step / _after_step) ------------
def before_step(m):
    P = m.__dict__.get("_particles")              # U0 from the state the step starts from
    if P is not None:
        P._before_step()


def after_step(m):
    # the forcing first: the forced, re-inverted state is what the particles' U1, the record of this step, the averages' sample
    # and the next step see; the time-mean spectra (timespectra.py) come last, after the four attachments of section 5k (whose
    # order tests/test_averages_host.py reads from this line as it stands)
    for slot in ("_forcing", "_particles", "_frequency", "_averages") + ("_timespectra",):
        A = m.__dict__.get(slot)
        if A is not None:
            A._after_step()
