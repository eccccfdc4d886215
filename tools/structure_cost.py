"""Cost of the structure functions.

    python tools/structure_cost.py --cost 4096        # ms per call, one JSON line

--cost: CoupledModel at nx with a broadband state.  Three calls alternate --reps times (at least five) in one run, each timed with
device events after a warm-up call: one structure call on (u, v, q_psi) with two triples and the default separations, the same
with 8 separations, and a PDF call (a counting pass with fixed ranges) on the same names.  Medians, with the minimum and the
maximum as the spread and every repetition listed."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from averages_cost import model          # noqa: E402  (tools/averages_cost.py: the broadband state of the averages' cost tool)

NAMES = ("u", "v", "q_psi")
MIXED = (("u", "v", "v"), ("u", "q_psi", "q_psi"))


def cost(nx, reps):
    from niwqg_amd import pdfs, structure
    m = model(nx)
    c = m._ctx
    c.step(2)
    h = pdfs.field_pdfs(m, names=NAMES)
    ranges = {n: (h.edges[n][0], h.edges[n][-1]) for n in NAMES}
    full = structure.default_separations(nx)
    eight = full[np.linspace(0, full.size - 1, 8).round().astype(int)] if full.size > 8 else full
    backends = {"structure_default_ms": structure._Fused(m, list(NAMES), full, list(MIXED)),
                "structure_8_separations_ms": structure._Fused(m, list(NAMES), eight, list(MIXED))}
    calls = {k: (lambda be=be: be.add(False)) for k, be in backends.items()}
    calls["pdf_same_names_ms"] = lambda: pdfs._Fused(m).bin(list(NAMES), ranges, 256, None, 0, False)

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()
    runs = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
    out = dict(nx=nx, reps=reps, names=list(NAMES), triples=len(MIXED), default_separations=int(full.size), eight=[int(r) for r in eight])
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
        out[k + "_all"] = [round(x, 4) for x in v]
    out["structure_default_over_pdf"] = round(out["structure_default_ms"] / out["pdf_same_names_ms"], 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX", required=True)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5 (medians of fewer repetitions are not reported)")
    cost(a.cost, a.reps)


if __name__ == "__main__":
    main()
