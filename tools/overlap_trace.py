#!/usr/bin/env python
"""What the dual-stream step does in time, from a rocprofv3 kernel trace (csv) of `python bench.py`:
    python tools/overlap_trace.py run_kernel_trace.csv
Per ETDRK4 stage (steady half of the trace): the wall span of [wave-PV row kernel U q branch] = from the start of the first of
{k_x_wavepv2, k_s_q, the k_y_A launch in front of k_s_q} to the end of the last (only meaningful when they run side by side: in
the serial step the wave kernels lie between them, there the sum of the three is the cost); how long each of them takes;
how long they overlap; and the median time per launch of the kernels that must not move (k_s_phi, k_x_products, k_s_invert,
every other k_y_A)."""
import csv, re, sys, statistics as st

rows = [r for r in csv.DictReader(open(sys.argv[1])) if r["Kernel_Name"].startswith(("void nq::", "nq::"))]
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["n"] = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("nq::", "")
rows.sort(key=lambda r: r["s"])
rows = rows[len(rows) // 2:]
short = lambda n: re.sub(r"<.*", "", n)
wpv = [r for r in rows if short(r["n"]).startswith("k_x_wavepv")]
sq = [r for r in rows if short(r["n"]) == "k_s_q"]
inv = [r for r in rows if short(r["n"]) == "k_s_invert"]
span, dw, dq, da, lead, ovl = [], [], [], [], [], []
used = set()
for w in wpv:
    nxt = [r for r in inv if r["s"] >= w["s"]]
    if not nxt:
        continue
    end = nxt[0]["s"]
    qs = [r for r in sq if w["s"] - 2_000_000 < r["s"] < end]          # the k_s_q of this stage (before it when serial)
    if not qs:
        continue
    q = qs[-1]
    ya = [r for r in rows if short(r["n"]) == "k_y_A" and r["e"] <= q["s"] + 1000 and r["s"] >= q["s"] - 400_000 and "false" in r["n"]][-1:]
    parts = [w, q] + ya
    used.update(id(r) for r in parts)
    span.append((max(r["e"] for r in parts) - min(r["s"] for r in parts)) / 1e3)
    dw.append((w["e"] - w["s"]) / 1e3); dq.append((q["e"] - q["s"]) / 1e3); da.append(sum(r["e"] - r["s"] for r in ya) / 1e3)
    lead.append((min(r["s"] for r in [q] + ya) - w["s"]) / 1e3)
    ovl.append(max(0, min(w["e"], q["e"]) - max(w["s"], min(r["s"] for r in [q] + ya))) / 1e3)
print("stages: %d" % len(span))
for name, v in (("span [wavepv U q branch]", span), ("k_x_wavepv", dw), ("k_s_q", dq), ("k_y_A of the q branch", da), ("sum of the three (the serial cost)", [a + b + c for a, b, c in zip(dw, dq, da)]),
                ("q branch start - wavepv start", lead), ("time both run", ovl)):
    if v:
        print("%-36s median %8.1f us   min %8.1f   max %8.1f" % (name, st.median(v), min(v), max(v)))
other = {}
for r in rows:
    if id(r) in used:
        continue
    key = r["n"][:60]
    other.setdefault(key, []).append((r["e"] - r["s"]) / 1e3)
print("launches outside the overlapped pair:")
for k, v in sorted(other.items(), key=lambda kv: -sum(kv[1])):
    if len(v) >= 8:
        print("  %-60s n=%5d median %8.1f us  total %9.1f us" % (k, len(v), st.median(v), sum(v)))
tot = (rows[-1]["e"] - rows[0]["s"]) / 1e3
print("trace window %.1f us, %d wave-PV launches -> %.3f ms per step" % (tot, len(wpv), tot / max(1, len(wpv)) * 4 / 1e3))
