#!/usr/bin/env python
"""Kernel boundaries of the dense layer step out of a rocprofv3 --kernel-trace run of scripts/layer_one.py (csv output):
for every repetition the six kernels of the step in dispatch order

    k_fft2d_fwd3 (xhat) -> k_modegemm_dma (yhat) -> k_fft2d_inv3 | k_fft2d_fwd3 (ghat) -> k_modegemm_dma_bwd (gxhat) -> k_fft2d_inv3

and the gap (start of the consumer - end of the producer) behind each of the four spectrum writers.  The boundary
between the two C calls (inverse -> adjoint) and the one between repetitions contain host work and are left out.
Prints the MEDIAN over the repetitions (the first two are warm-up) of every gap and every kernel duration, in us, and
the spread (iqr: the interquartile range of the per-repetition sum of the two calls' spans; with BOUNDARY_SITES=1 the
span producer start -> consumer end of every store site and its interquartile range) so that a difference can be set
against the noise.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/layer_one.py
    python scripts/boundary_table.py DIR [label]

Sites are switched with LAYER_FLAGS=1024 (SC_PLAN_PLAIN_CACHE_POLICY) on the product library, or one by one on the
diagnostic build (scripts/build_diag.py) with SC_POLICY_SITES=<mask> / SC_POLICY_NT=<mask> (csrc/sc_engine.cpp)."""
import csv
import glob
import os
import statistics
import sys

ORDER = ["k_fft2d_fwd3", "k_modegemm_dma<", "k_fft2d_inv3", "k_fft2d_fwd3", "k_modegemm_dma_bwd", "k_fft2d_inv3"]
NAMES = ["fwd", "gemm", "inv", "adj", "pair", "inv2"]
GAPS = [(0, 1, "fwd>gemm"), (1, 2, "gemm>inv"), (3, 4, "adj>pair"), (4, 5, "pair>inv")]


def load(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return [r for r in rows if any(k in r[2] for k in ("k_fft2d_", "k_modegemm_"))]


def steps(rows):
    out, i = [], 0
    while i + 6 <= len(rows):
        if all(ORDER[j] in rows[i + j][2] for j in range(6)):
            out.append(rows[i:i + 6])
            i += 6
        else:
            i += 1
    return out


def table(d):
    st = steps(load(d))[2:]
    if not st:
        raise SystemExit(f"{d}: no complete layer step in the trace")
    med = {}
    for a, b, name in GAPS:
        med[name] = statistics.median((s[b][0] - s[a][1]) / 1e3 for s in st)
    for j, name in enumerate(NAMES):
        med[name] = statistics.median((s[j][1] - s[j][0]) / 1e3 for s in st)
    # per store site: producer + gap + consumer (start of the producer to end of the consumer), median and interquartile range
    for a, b, name in GAPS:
        span = [(s[b][1] - s[a][0]) / 1e3 for s in st]
        qs = statistics.quantiles(span, n=4) if len(span) >= 4 else [min(span), 0, max(span)]
        med["S:" + name] = statistics.median(span)
        med["I:" + name] = qs[2] - qs[0]
    fwd_call = [(s[2][1] - s[0][0]) / 1e3 for s in st]          # first dispatch to last end of sc_layer_forward
    bwd_call = [(s[5][1] - s[3][0]) / 1e3 for s in st]
    both = [f + b for f, b in zip(fwd_call, bwd_call)]
    med["calls"] = statistics.median(both)
    q = statistics.quantiles(both, n=4) if len(both) >= 4 else [min(both), med["calls"], max(both)]
    med["iqr"] = q[2] - q[0]
    med["n"] = len(st)
    return med


COLS = [g[2] for g in GAPS] + NAMES + ["calls", "iqr", "n"]
if os.environ.get("BOUNDARY_SITES"):       # the per-site view: S = producer + gap + consumer, I = its interquartile range
    COLS = [p + g[2] for g in GAPS for p in ("S:", "I:")] + ["calls", "iqr", "n"]

if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    m = table(sys.argv[1])
    label = sys.argv[2] if len(sys.argv) > 2 else os.path.basename(os.path.normpath(sys.argv[1]))
    if os.environ.get("BOUNDARY_HEADER"):
        print(f"{'variant':<22}" + "".join(f"{c:>11}" for c in COLS))
    print(f"{label:<22}" + "".join(f"{m[c]:>11.2f}" if c != "n" else f"{m[c]:>11d}" for c in COLS), flush=True)
