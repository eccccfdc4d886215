"""Cost of the time-mean spectra's sample inside the step.

    python tools/timespectra_cost.py --cost 4096     # ms per sample and per host call against the bare step, one JSON line

CoupledModel at nx with a broadband state.  One run times, alternating --reps times: the bare step (nothing attached), the step
with the attachment at every = 1 for the spectra only, the transfer only and both, and single steps each followed by the host
call(s) the sample replaces (``nq_diagnostics_binned``, ``nq_transfer_binned``, both).  Every configuration takes --steps steps
between two host synchronisations and is timed on the host clock around them (the host calls synchronise anyway); the medians are
reported, a cost is the difference to the bare step, and ``spread_ms`` is the largest max - min of any configuration's
repetitions.  The two requirements of section 5n are evaluated at the end: the combined sample is cheaper than the two separate
ones by more than the spread (the shared products passes), and a sample costs no more than its host call plus the spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SAMPLES = {"spectra": (True, False), "transfer": (False, True), "both": (True, True)}


def model(nx):
    import niwqg_amd
    L = 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    return m


def cost(nx, steps, reps):
    from niwqg_amd import timespectra
    m = model(nx)
    c = m._ctx
    c.step(2)
    c.diagnostic_sums_binned()                        # the context-owned planes of the two calls exist before anything is timed
    c.transfer_sums_binned()

    def in_step():
        c.step(steps)

    def host(spectra, transfer):
        def go():
            for _ in range(steps):
                c.step(1)
                if spectra:
                    c.diagnostic_sums_binned()
                if transfer:
                    c.transfer_sums_binned()
        return go

    def timed(go):
        c.sync()
        t0 = time.perf_counter()
        go()
        c.sync()
        return (time.perf_counter() - t0) * 1e3 / steps

    configs = ["bare"] + ["step_" + k for k in SAMPLES] + ["host_" + k for k in SAMPLES]
    runs = {k: [] for k in configs}
    for _ in range(reps):
        for k in configs:
            kind, _, what = k.partition("_")
            T = timespectra.attach(m, *SAMPLES[what], every=1) if kind == "step" else None
            go = host(*SAMPLES[what]) if kind == "host" else in_step
            timed(go)                                 # warm-up of this configuration
            runs[k].append(timed(go))
            if T:
                assert T.info()["n"] == 2 * steps
                T.detach()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = max(max(v) - min(v) for v in runs.values())
    out = dict(nx=nx, steps=steps, reps=reps, bare_step_ms=round(med["bare"], 4), spread_ms=round(spread, 4))
    for k in configs:
        out[k + "_ms_all"] = [round(v, 4) for v in runs[k]]
    for what in SAMPLES:
        out["ms_per_sample_" + what] = round(med["step_" + what] - med["bare"], 4)
        out["ms_per_host_call_" + what] = round(med["host_" + what] - med["bare"], 4)
    saving = out["ms_per_sample_spectra"] + out["ms_per_sample_transfer"] - out["ms_per_sample_both"]
    out["shared_pass_saving_ms"] = round(saving, 4)
    out["combined_cheaper_than_separate_by_more_than_spread"] = bool(saving > spread)
    out["sample_no_dearer_than_host_call"] = {w: bool(out["ms_per_sample_" + w] <= out["ms_per_host_call_" + w] + spread) for w in SAMPLES}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX", required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cost(a.cost, a.steps, a.reps)


if __name__ == "__main__":
    main()
