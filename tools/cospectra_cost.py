"""Cost and large-grid check of the co-spectra of the physical fields.

    python tools/cospectra_cost.py --cost 4096              # ms per call, one JSON line
    python tools/cospectra_cost.py --check 2048 4096 8192   # against the numpy route, one JSON line per grid

--cost: CoupledModel at nx with a broadband state; four calls alternate --reps times in one run, each timed with device events
after a warm-up call, and the medians are reported: cross_spectra on (q_psi, phi2) and on (q_psi, ow, gradphi2), both without
download, spectral_transfer(m)'s device call, and the flow-names field_pdfs call of tools/flow_cost.py.
--check: the instantiations the feature's own test does not reach (tests/test_gpu_plan_ladder_analysis.py does since).  Every row of every list against numpy's fft2 of the planes one averages
sample returns for the same names, per shell, in units of the tests' bar (tests/test_gpu_cospectra.py: the issue's 1e-12 of the
shell's content on every resolved shell): ok means <= 1.  At 8192 a
list with a flow name must be refused and the three old names are checked."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from averages_cost import model          # noqa: E402  (tools/averages_cost.py: the broadband state of the averages' cost tool)

PAIR = ("q_psi", "phi2")
TRIPLE = ("q_psi", "ow", "gradphi2")
LISTS = (("q", "q_psi", "phi2"), TRIPLE, ("u", "v"), ("strain2",))
FLOW = dict(names=TRIPLE, joint=("ow", "gradphi2"))


def cost(nx, reps):
    from niwqg_amd import cospectra, pdfs
    m = model(nx)
    c = m._ctx
    c.step(2)
    h = pdfs.field_pdfs(m, **FLOW)
    ranges = {n: (h.edges[n][0], h.edges[n][-1]) for n in TRIPLE}

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()
    codes = lambda names: [cospectra._CODES[n] for n in names]
    calls = {"cross_pair_ms": lambda: c.cospectra(codes(PAIR), download=False),
             "cross_triple_ms": lambda: c.cospectra(codes(TRIPLE), download=False),
             "spectral_transfer_ms": lambda: c.transfer_sums_binned(),
             "flow_pdfs_ms": lambda: pdfs._Fused(m).bin(list(TRIPLE), ranges, 256, FLOW["joint"], 64, False)}
    runs = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
    out = dict(nx=nx, reps=reps, pair=list(PAIR), triple=list(TRIPLE))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_all"] = [round(x, 4) for x in v]
    out["pair_over_transfer"] = round(out["cross_pair_ms"] / out["spectral_transfer_ms"], 2)
    out["triple_over_transfer"] = round(out["cross_triple_ms"] / out["spectral_transfer_ms"], 2)
    print(json.dumps(out), flush=True)


def worst_ratio(cs, planes, nx):
    """(largest |device - numpy| over the issue's bar 1e-12 sum_shell |A||B| / M^2 on the resolved shells of every row, number of
    shells that are not resolved -- the reference's own round-off bound, cospectra.transform_rounding, above 5 % of that bar --, the
    largest error there over that bar plus the round-off bound of the packed route)"""
    from niwqg_amd import cospectra
    M2, worst, nother, worst_other = float(nx) ** 4, 0.0, 0, 0.0
    T = {n: np.fft.fft2(planes[n]) for n in cs.names}
    for i, a in enumerate(cs.names):
        for b in cs.names[i:]:
            A, B = T[a], T[b]
            want = cospectra.bin_shells(A.real * B.real + A.imag * B.imag, nx) / M2
            bar = 1e-12 * cospectra.bin_shells(np.abs(A) * np.abs(B), nx) / M2
            resolved = cospectra.transform_rounding(A, B, planes[a], planes[b], nx) <= 0.05 * bar      # the reference's own round-off
            rounding = cospectra.transform_rounding(A, B, planes[a], planes[b], nx, packed=True)        # the device's packed route
            got = cs.auto[a] if a == b else cs.co[(a, b)]
            err = np.abs(got - want)
            worst = max(worst, float((err / bar)[resolved].max()))
            if not resolved.all():
                nother += int((~resolved).sum())
                worst_other = max(worst_other, float((err / (bar + rounding))[~resolved].max()))
    return worst, nother, worst_other


def check(nx):
    from niwqg_amd import averages, cospectra, flow
    m = model(nx)
    m._ctx.step(1)
    m._after_steps()
    out = dict(nx=nx)
    for names in LISTS:
        key = "/".join(names)
        if nx >= flow.ONE_VALUE_NX and any(n in flow.NAMES for n in names):
            try:
                cospectra.cross_spectra(m, names)
                out[key] = "not refused"
            except NotImplementedError:
                out[key] = "refused"
            continue
        A = averages.attach(m, names, every=0)
        A.sample()
        R = A.result()
        planes = {n: R.mean(n) for n in names}
        A.detach()
        out[key], out["not resolved " + key], out["their worst " + key] = worst_ratio(cospectra.cross_spectra(m, names), planes, nx)
    out["ok"] = bool(all(v == "refused" or (not isinstance(v, str) and v <= 1.0) for k, v in out.items() if k != "nx" and not k.startswith("not resolved")))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX")
    ap.add_argument("--check", type=int, nargs="+", metavar="NX")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.cost is None and a.check is None:
        ap.error("one of --cost NX, --check NX [NX ...]")
    if a.cost is not None:
        cost(a.cost, a.reps)
    for nx in a.check or ():
        check(nx)


if __name__ == "__main__":
    main()
