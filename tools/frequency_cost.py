"""Cost of the low-mode recorder inside the step and of one spectrum call.

CoupledModel at nx (default 4096) with a broadband state, all in one run: (a) ms per step without a recorder, (b) per step with
phi, q and psi recorded at kmax (default 256) after every step, (c) without again; each leg one warm-up call, then --steps steps
timed with perf_counter around a synchronous call.  Then a ring of --length (default 1024) records filled by stepping, and
--reps spectrum calls (Hann) timed after a first one that allocates the work plane and builds the transform plan.  The
expectation checked: |b - a| within the 1.5 % run-to-run spread of the step.  Prints one JSON line."""
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
    ap.add_argument("--kmax", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--length", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd import frequency
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

    K = a.kmax
    R = 2 * K + 1
    out = dict(nx=nx, kmax=K, steps=a.steps, length=a.length, record_bytes=16 * R * (R + 2 * (K + 1)))
    out["a_unattached_ms"] = step_ms()
    b0 = ctx.device_bytes()
    rec = frequency.attach(m, K, every=1, length=a.length)
    out["b_recording_ms"] = step_ms()
    out["ring_bytes"] = ctx.device_bytes() - b0
    held = rec.info()["held"]
    ctx.step(max(0, a.length - held))                     # fill the ring
    ctx.sync()
    t0 = time.perf_counter()
    S = rec.spectrum("hann")
    out["spectrum_first_call_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for _ in range(a.reps):
        S = rec.spectrum("hann")
    out["spectrum_ms"] = (time.perf_counter() - t0) / a.reps * 1e3
    out["spectrum_T"] = len(S.omega)
    out["spectrum_shells"] = len(S.shell)
    out["bytes_with_spectrum"] = ctx.device_bytes() - b0
    rec.detach()
    out["bytes_after_detach"] = ctx.device_bytes() - b0
    out["a_unattached_again_ms"] = step_ms()
    a_ms = 0.5 * (out["a_unattached_ms"] + out["a_unattached_again_ms"])
    out["b_over_a"] = out["b_recording_ms"] / a_ms
    out["within_spread"] = bool(abs(out["b_over_a"] - 1.0) <= 0.015)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
