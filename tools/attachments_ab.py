"""The three attachments of the step together: digests for an A/B between two builds, and their cost.

Default: CoupledModel at 64 (fused context) and at 96 (any-size path) and QGModel at 96, each with forcing, 37 recording
particles (a record every 2 steps, 3 kept) and a recorder (kmax 4, a record every 2 steps, 3 kept), 8 steps, the first three in
one call where the path batches.  Prints one line per case with the sha256 of q-hat, phi-hat, the particle positions, the
trajectory, the recorder's series, its spectrum table and the forcing's work: two builds that compute the same print the same.

--cost NX: ms per step at NX (one warm-up call, then --steps steps timed with perf_counter around a synchronous call) with
nothing attached, with all three (the particles and the recorder recording every second step), and with nothing again.
Prints one JSON line."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model(kind, nx):
    import niwqg_amd
    L = 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    kw = dict(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9, use_filter=True, U=-0.1,
              nu4=5e11 * (128.0 / nx) ** 4, nu=20)
    if kind == "qg":
        m = niwqg_amd.QGModel.Model(**kw)
    else:
        m = niwqg_amd.CoupledModel.Model(f=1e-4, N=0.01, m=2 * np.pi / 280.0, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7, **kw)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    if kind != "qg":
        m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    return m


def attach_all(m, kind, n=37, every=2, keep=3, kmax=4):
    from niwqg_amd import forcing, frequency, particles
    qg = kind == "qg"
    dk = m.dk
    F = forcing.attach(m, q=forcing.ring(m, 4 * dk, 2 * dk, 1e-12),
                       phi=None if qg else forcing.ring(m, 4 * dk, 2 * dk, 1e-12, field="phi"), seed=11)
    rng = np.random.default_rng(5)
    P = particles.attach(m, rng.uniform(0, m.L, n), rng.uniform(0, m.W, n), record_every=every, capacity=keep,
                         record=("q",) if qg else ("q", "phi"))
    R = frequency.attach(m, kmax, every=every, length=keep, fields=("q", "psi") if qg else None)
    return F, P, R


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def digests(kind, nx):
    m = model(kind, nx)
    F, P, R = attach_all(m, kind)
    if getattr(m, "_any_size", False):
        for _ in range(3):
            m._step_forward()
    else:
        m._ctx.step(3)
        m._after_steps()
    for _ in range(5):
        m._step_forward()
    tr, S, w = P.trajectory(), R.spectrum("boxcar"), F.work()
    out = dict(case="%s-%d" % (kind, nx), qh=sha(m.qh), phih=sha(m.phih) if kind != "qg" else None, positions=sha(*P.positions()),
               trajectory=sha(tr.step, tr.x, tr.y, *[tr.values[n] for n in sorted(tr.values)]),
               series=sha(*[a for n in R.fields for a in (R.series(n).step, R.series(n).values)]),
               spectrum=sha(S.omega, *[S.values[n] for n in R.fields]), work=sha(np.array([w["q"], w["phi"]])),
               forcing_step=F.state()["step"], records=R.info()["written"])
    for a in (R, P, F):
        a.detach()
    print(json.dumps(out))


def cost(nx, steps):
    m = model("coupled", nx)
    ctx = m._ctx

    def step_ms():
        ctx.step(2)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.step(steps)
        ctx.sync()
        return (time.perf_counter() - t0) / steps * 1e3

    out = dict(nx=nx, steps=steps, bare_ms=step_ms())
    b0 = ctx.device_bytes()
    att = attach_all(m, "coupled", n=100000, keep=8, kmax=32)
    out["attached_ms"] = step_ms()
    out["bytes"] = ctx.device_bytes() - b0
    for a in att:
        a.detach()
    out["bare_again_ms"] = step_ms()
    out["attached_over_bare"] = out["attached_ms"] / (0.5 * (out["bare_ms"] + out["bare_again_ms"]))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, default=0, metavar="NX")
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    if a.cost:
        cost(a.cost, a.steps)
    else:
        for kind, nx in (("coupled", 64), ("coupled", 96), ("qg", 96)):
            digests(kind, nx)


if __name__ == "__main__":
    main()
