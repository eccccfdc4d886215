"""Cost of the PDFs of the increments.

    python tools/increment_pdfs_cost.py --cost 4096        # ms per call, JSON lines

--cost: CoupledModel at nx with a broadband state (tools/averages_cost.py).  The calls alternate --reps times (at least five) in one
run, each timed with device events after a warm-up call, on (u, v, q_psi):
  increments_default_ms / increments_8_separations_ms   the counting pass (k_x_flow_ipdf, 256 bins, fixed ranges) at the default
                                                        separations and at eight of them
  range_pass_default_ms                                 the range pass alone (structure's kernels, its table read back)
  pdfs_call_default_ms                                  increments.pdfs as a user calls it: range pass, counting pass, read
  pdfs2d_y_axis_ms                                      the counting pass of pdfs2d on the vectors (0, r) (store pass + k_ipdf_plane)
  structure_default_ms, pdf_same_names_ms               the yardsticks of tools/structure_cost.py: one structure call (two triples)
                                                        and one pdfs.field_pdfs counting pass
One line with the medians (minimum and maximum as the spread), one line per call with every repetition."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from averages_cost import model          # noqa: E402
from structure_cost import NAMES, MIXED  # noqa: E402

BINS = 256


def cost(nx, reps):
    from niwqg_amd import increments, pdfs, structure
    m = model(nx)
    c = m._ctx
    c.step(2)
    h = pdfs.field_pdfs(m, names=NAMES)
    ranges = {n: (h.edges[n][0], h.edges[n][-1]) for n in NAMES}
    full = structure.default_separations(nx)
    eight = full[np.linspace(0, full.size - 1, 8).round().astype(int)] if full.size > 8 else full
    first = increments.pdfs(m, names=NAMES, bins=BINS)
    C = lambda sep, vec=None: increments._Call(m, NAMES, sep, vec, ("u", "v") if vec is not None else None, BINS, None, 8.0, vec is not None, "cost")
    cd, c8, cy = C(full), C(eight), C(None, structure.axis_vectors(nx, "y"))
    r8 = {n: first.ranges[n][np.searchsorted(full, eight)] for n in NAMES}
    ry = cy.ranges()
    sf = structure._Fused(m, list(NAMES), full, list(MIXED))
    calls = {"increments_default_ms": lambda: cd.be.bin(first.ranges, BINS, False),
             "increments_8_separations_ms": lambda: c8.be.bin(r8, BINS, False),
             "range_pass_default_ms": lambda: cd.be.sums(),
             "pdfs_call_default_ms": lambda: increments.pdfs(m, names=NAMES, bins=BINS),
             "pdfs2d_y_axis_ms": lambda: cy.be.bin(ry, BINS, False),
             "structure_default_ms": lambda: sf.add(False),
             "pdf_same_names_ms": lambda: pdfs._Fused(m).bin(list(NAMES), ranges, BINS, None, 0, False)}

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()
    runs = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
    out = dict(nx=nx, reps=reps, names=list(NAMES), bins=BINS, default_separations=int(full.size), eight=[int(r) for r in eight], triples_of_structure=len(MIXED))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    out["increments_default_over_structure_default"] = round(out["increments_default_ms"] / out["structure_default_ms"], 2)
    out["increments_default_over_pdf"] = round(out["increments_default_ms"] / out["pdf_same_names_ms"], 2)
    print(json.dumps(out))
    for k, v in runs.items():
        print(json.dumps({"call": k, "all_ms": [round(x, 4) for x in v]}))


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
