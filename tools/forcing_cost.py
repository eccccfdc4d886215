"""Cost of stochastic forcing inside the step.

CoupledModel at nx (default 4096) with a broadband state and a ring at kf = 32 dk, all in one run: (a) ms per unforced step,
(b) per step with q forced, (c) with q and phi forced, (d) one nq_invert call alone, (e) the device part of set_phi (the emit
kernel plus the inverse column pass, NQ_PH_EMIT_PHI).  Each step leg runs one warm-up call, then --steps steps timed with
perf_counter around a synchronous call; (d) and (e) are the mean of --reps synchronous calls.  The expectation checked:
(b) <= (a + d) 1.05 and (c) <= (a + d + e) 1.05.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd import forcing
    from niwqg_amd.slab import PH_EMIT_PHI
    nx, L = a.nx, 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    ctx = m._ctx

    def step_ms():
        ctx.step(2)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.step(a.steps)
        ctx.sync()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def call_ms(fn):
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    def emit():
        ctx._chk(ctx.L.nq_phase(ctx.h, PH_EMIT_PHI, 0), "nq_phase")

    dk = m.dk
    eps = 1e-12
    Aq, Aphi = forcing.ring(m, 32 * dk, 2 * dk, eps), forcing.ring(m, 32 * dk, 2 * dk, eps, field="phi")
    out = dict(nx=nx, steps=a.steps, reps=a.reps, forced_modes_q=int((Aq > 0).sum()), forced_modes_phi=int((Aphi > 0).sum()))
    out["a_unforced_ms"] = step_ms()
    out["d_invert_ms"] = call_ms(ctx.invert)
    out["e_emit_phi_ms"] = call_ms(emit)
    b0 = ctx.device_bytes()
    F = forcing.attach(m, q=Aq, seed=1)
    out["b_forced_q_ms"] = step_ms()
    out["bytes_q"] = ctx.device_bytes() - b0
    F.detach()
    F = forcing.attach(m, q=Aq, phi=Aphi, seed=1)
    out["c_forced_q_phi_ms"] = step_ms()
    out["bytes_q_phi"] = ctx.device_bytes() - b0
    F.detach()
    out["a_unforced_again_ms"] = step_ms()
    a_ms = 0.5 * (out["a_unforced_ms"] + out["a_unforced_again_ms"])
    out["b_over_a_plus_d"] = out["b_forced_q_ms"] / (a_ms + out["d_invert_ms"])
    out["c_over_a_plus_d_plus_e"] = out["c_forced_q_phi_ms"] / (a_ms + out["d_invert_ms"] + out["e_emit_phi_ms"])
    out["within_expectation"] = bool(out["b_over_a_plus_d"] <= 1.05 and out["c_over_a_plus_d_plus_e"] <= 1.05)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
