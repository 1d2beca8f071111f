#!/usr/bin/env python
"""Split the time of bench.py's dependent loop from a rocprofv3 --kernel-trace CSV (profiles/r7/NOTES.md).

    rocprofv3 --kernel-trace -f csv -d DIR -- python bench.py --full --steps 200 --warmup 20 --spinup-steps 1500 ...
    python scripts/trace_gaps.py DIR/.../*_kernel_trace.csv --skip 1520 --steps 200 --out summary.json --steps-csv steps.csv

Kernels of one hardware queue are taken in start order and cut into SEGMENTS wherever the queue stood idle for more than
--cut-us (a pass of bench.py ends with a device synchronise and the next one starts with Python work) and wherever the PASS
changes: the convolution's instantiation (the context launches the unit-table form, the pre-planned passes the plain one) or
whether a k_policy_token follows each convolution.  A segment whose convolution launches alternate with k_policy_token is a
dependent pass; a `conv_only` segment of the unit-table instantiation on the dependent pass's queue is the context's
single-stream pass (its gap_to_next_conv_us is the conv -> conv gap).  Per step: kernel durations, the gap conv end -> token
start, and the gap token end -> next conv start, both also by the step's position in its ring group (step index mod 4: the ring
used to record its completion event behind the last step of a group).  Gaps over --max-gap-us are host stalls: counted, listed by
step, left out of the medians.
All times in microseconds."""
import argparse
import csv
import json
import sys

import numpy as np


def q3(v):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return None
    return {"n": int(v.size), "p10": round(float(np.quantile(v, 0.1)), 3), "median": round(float(np.median(v)), 3),
            "p90": round(float(np.quantile(v, 0.9)), 3)}


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            kind = "token" if "k_policy_token" in name else ("conv" if "k_conv" in name else None)
            if kind is None:
                continue
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, name, r.get("Queue_Id", "0")))
    rows.sort()
    return rows


def segments(rows, cut_ns):
    by_q = {}
    for r in rows:
        by_q.setdefault(r[4], []).append(r)
    segs = []
    for q, rs in by_q.items():
        # the pass a kernel belongs to: (instantiation of the convolution, a token follows it)
        mode = [None] * len(rs)
        for i, r in enumerate(rs):
            if r[2] == "conv":
                mode[i] = (r[3], i + 1 < len(rs) and rs[i + 1][2] == "token")
        for i in range(len(rs)):                        # a token belongs to the convolution in front of it
            if mode[i] is None:
                mode[i] = mode[i - 1] if i else (rs[i][3], True)
        cur = [rs[0]]
        for i in range(1, len(rs)):
            a, b = rs[i - 1], rs[i]
            if b[0] - a[1] > cut_ns or (b[2] == "conv" and mode[i] != mode[i - 1] and
                                        i + 1 < len(rs) and mode[i + 1] == mode[i]):      # (two in a row: not a pass's last step)
                segs.append((q, cur))
                cur = []
            cur.append(b)
        segs.append((q, cur))
    segs.sort(key=lambda s: s[1][0][0])
    return segs


def steps_of(seg):
    """dependent pass: [(conv, token, next conv)]; single-stream pass: [(conv, None, next conv)]"""
    out = []
    i = 0
    while i < len(seg):
        if seg[i][2] != "conv":
            i += 1
            continue
        if i + 2 < len(seg) and seg[i + 1][2] == "token" and seg[i + 2][2] == "conv":
            out.append((seg[i], seg[i + 1], seg[i + 2]))
            i += 2
        elif i + 1 < len(seg) and seg[i + 1][2] == "conv":
            out.append((seg[i], None, seg[i + 1]))
            i += 1
        else:
            i += 1
    return out


def table(steps, skip, n, max_gap_us):
    st = steps[skip:skip + n] if n > 0 else steps[skip:]
    us = 1e-3
    conv = [(c[1] - c[0]) * us for c, _, _ in st]
    tok = [(t[1] - t[0]) * us for _, t, _ in st if t]
    g_ct = [(t[0] - c[1]) * us for c, t, _ in st if t]
    g_ct_pos = [((t[0] - c[1]) * us, (skip + i) % 4) for i, (c, t, _) in enumerate(st) if t]
    g_next = [((nx[0] - (t[1] if t else c[1])) * us, (skip + i) % 4) for i, (c, t, nx) in enumerate(st)]
    g_ok = [(g, ph) for g, ph in g_next if g <= max_gap_us]          # (a host stall is not a launch gap: counted, not averaged)
    res = {"steps": len(st), "conv_us": q3(conv), "token_us": q3(tok), "gap_conv_to_token_us": q3(g_ct),
           "gap_to_next_conv_us": q3([g for g, _ in g_ok]),
           "gap_to_next_conv_by_position_us": {str(ph): q3([g for g, p in g_ok if p == ph]) for ph in range(4)},
           "gap_conv_to_token_by_position_us": {str(ph): q3([g for g, p in g_ct_pos if p == ph]) for ph in range(4)},
           "gaps_to_next_conv_over_2_us": sum(1 for g, _ in g_ok if g > 2.0),
           "host_stalls_over_%g_us" % max_gap_us: len(g_next) - len(g_ok),
           "host_stall_us": [round(g, 1) for g, _ in g_next if g > max_gap_us][:64]}
    if st:
        res["step_period_us"] = q3([(b[0][0] - a[0][0]) * us for a, b in zip(st, st[1:])])
    return res, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--cut-us", type=float, default=1000.0)
    ap.add_argument("--skip", type=int, default=1520, help="steps of a segment in front of the timed region (spin-up + warm-up)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--max-gap-us", type=float, default=50.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps-csv", default=None, help="per-step rows of the first dependent segment's timed region")
    a = ap.parse_args()
    rows = load(a.csv)
    segs = segments(rows, a.cut_us * 1e3)
    summary = {"segments": []}
    first_dep = None
    for q, seg in segs:
        n_conv = sum(1 for r in seg if r[2] == "conv")
        n_tok = len(seg) - n_conv
        if n_conv < a.skip + 50:
            continue
        names = sorted({r[3] for r in seg if r[2] == "conv"})
        kind = "dependent" if n_tok > n_conv // 2 else "conv_only"
        steps = steps_of(seg)
        res, st = table(steps, a.skip, a.steps, a.max_gap_us)
        rest, _ = table(steps, a.skip, 0, a.max_gap_us)
        summary["segments"].append({"queue": q, "kind": kind, "convs": n_conv, "tokens": n_tok, "conv_kernels": names,
                                    "t0_ms": round((seg[0][0] - rows[0][0]) * 1e-6, 2), "timed_region": res, "whole_after_skip": rest})
        if kind == "dependent" and first_dep is None:
            first_dep = st
    txt = json.dumps(summary, indent=1)
    if a.out:
        open(a.out, "w").write(txt + "\n")
    print(txt)
    if a.steps_csv and first_dep:
        t0 = first_dep[0][0][0]
        with open(a.steps_csv, "w") as f:
            f.write("step,position_in_group,conv_start_us,conv_us,gap_conv_to_token_us,token_us,gap_token_to_next_conv_us\n")
            for i, (c, t, nx) in enumerate(first_dep):
                f.write(f"{i},{(a.skip + i) % 4},{(c[0] - t0) * 1e-3:.3f},{(c[1] - c[0]) * 1e-3:.3f},{(t[0] - c[1]) * 1e-3:.3f},"
                        f"{(t[1] - t[0]) * 1e-3:.3f},{(nx[0] - t[1]) * 1e-3:.3f}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
