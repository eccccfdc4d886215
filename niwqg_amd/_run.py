"""The run loop of niwqg_amd.Kernel.Kernel and niwqg_amd.QGModel.Model: the reference's sequence of steps, diagnostics ticks,
status lines and snapshots, with the steps between two host-visible events batched into one nq_step call.  The class supplies
``_step_forward``, ``_after_steps``, ``_print_status`` and ``_snapshot_fields``.
"""
import numpy as np

from .Saving import save_snapshots, save_diagnostics, flush_snapshots, flush_pending_quietly


class RunLoop(object):

    def _quiet_steps(self, n_left):
        """How many of the next ``n_left`` steps need no host attention before the first one that
        does: a diagnostics tick fires after a step when tc_before % tdiags == 0 (Diagnostics.py:43),
        a status line when (tc_before + 1) % twrite == 0 (Kernel.py:587-590)."""
        for j in range(n_left):
            tcb = self.tc + j
            if (tcb % self.tdiags) == 0 or ((tcb + 1) % self.twrite) == 0:
                return j
            if self.save_to_disk and ((tcb + 1) % self.tsnaps) == 0:      # a snapshot after this step (Saving.py:70)
                return j
        return n_left - 1

    def _steps_left(self, cap=1 << 30):
        """Replays the reference's float clock ``while t < tmax: t += dt`` (Kernel.py:198,:588)."""
        t, n = self.t, 0
        while t < self.tmax and n < cap:
            t += self.dt
            n += 1
        return n

    def run(self):
        """ref: niwqg/Kernel.py:183-203, niwqg/QGModel.py:184-207.  Steps between host-visible events are batched into one
        nq_step call; the sequence of diagnostics ticks and status lines is the reference's."""
        self._defer_snapshots = True              # snapshots are written while the next batch of steps runs
        try:
            if self.save_to_disk:                     # the initial condition (Kernel.py:194-195)
                save_snapshots(self, fields=self._snapshot_fields())
            while self.t < self.tmax:
                quiet = self._quiet_steps(self._steps_left(4096))
                if quiet > 0:
                    self._ctx.step(quiet)             # asynchronous: a pending snapshot is written while these steps run
                    flush_snapshots(self)
                    for _ in range(quiet):
                        self.tc += 1
                        self.t += self.dt
                    self._after_steps()
                self._step_forward()
            flush_snapshots(self)
            if self.save_to_disk:                     # Kernel.py:202-203
                save_diagnostics(self)
        finally:
            self._defer_snapshots = False
            flush_pending_quietly(self)      # (a failure in here must not mask the exception that is already on its way)

    def run_with_snapshots(self, tsnapstart=0., tsnapint=432000.):
        """ref: niwqg/Kernel.py:161-181"""
        tsnapints = np.ceil(tsnapint / self.dt)
        while self.t < self.tmax:
            self._step_forward()
            if self.t >= tsnapstart and (self.tc % tsnapints) == 0:
                yield self.t
        return
