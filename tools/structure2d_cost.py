"""Cost of the structure functions at two-dimensional separations.

    python tools/structure2d_cost.py --cost 4096        # ms per call, one JSON line

--cost: CoupledModel at nx with a broadband state, (u, v, q_psi) with the two usual triples and the rotation of (u, v).  The calls
alternate --reps times (at least five) in one run, each timed with device events after a warm-up call: (a) functions2d at the
default separations along y, (b) at the default ring set, (c) at ONE vector, which is the store pass, one base and one shifted row
read and the totals, an upper bound of the store pass alone (the library has no entry that runs it alone), (d) the same with TWO
vectors of one r_y, so that (d) - (c) is one more vector out of LDS and 2 (c) - (d) estimates the store pass; beside them
structure.functions on the same names at the same separations along x, and a PDF call (a counting pass with fixed ranges).
Medians, with the minimum and the maximum as the spread and every repetition listed; the bytes the layout implies for (a) and the
read rate that follows from the median."""
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
    sep = structure.default_separations(nx)
    sets = {"y_separations": structure.axis_vectors(nx, "y", sep), "ring_set": structure.ring_vectors(nx),
            "one_vector": np.array([(1, 0)]), "two_vectors_one_row": np.array([(1, 0), (2, 0)])}
    calls = {}
    for k, vec in sets.items():
        call = structure._Call2d(m, NAMES, vec, MIXED, ("u", "v"), None, "structure2d_cost")
        calls[k + "_ms"] = lambda be=call.be: be.add(False)
    xpass = structure._Fused(m, list(NAMES), sep, list(MIXED))
    calls["x_pass_same_separations_ms"] = lambda: xpass.add(False)
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
    ring = sets["ring_set"]
    out = dict(nx=nx, reps=reps, names=list(NAMES), triples=len(MIXED), y_separations=int(sep.size), ring_vectors=int(len(ring)),
               ring_distinct_ry=int(np.unique(ring[:, 1]).size))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
        out[k + "_all"] = [round(x, 4) for x in v]
    out["store_pass_estimate_ms"] = round(2 * out["one_vector_ms"] - out["two_vectors_one_row_ms"], 4)
    plane = nx * nx * 8.0
    read = (1 + sep.size) * len(NAMES) * plane                                  # the base rows once, a shifted row per distinct r_y
    out["y_plane_kernel_bytes_read"] = read
    out["y_store_bytes_written"] = len(NAMES) * plane
    out["y_read_rate_GBps_whole_call"] = round(read / (out["y_separations_ms"] * 1e-3) / 1e9, 1)
    rest = out["y_separations_ms"] - out["store_pass_estimate_ms"]
    out["y_read_rate_GBps_without_store_estimate"] = round(read / (rest * 1e-3) / 1e9, 1) if rest > 0 else None
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
