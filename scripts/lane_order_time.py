"""How long the filler of tests/test_lane_order.py has to run: the host time of every writer of shared state while all
lanes are idle, the time of one filler product, and the filler time the test derives from them (ten times the longest
host time, 0.2 s at the most).  With --case NAME the ordered run of that case follows, and the script says whether R was
the old result and R' the new one; with $ARTP_LIB pointing at another build of the library (the parent commit's) that
is the evidence that the filler makes the test sensitive.  Only the motion-cost cases may run against a library without
the ordering: a torn sampler table can send the column search out of bounds.
Output: one text table (profiles/lane_order.txt).
Usage: python scripts/lane_order_time.py [--out FILE] [--reps N] [--case NAME]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_lane_order as T  # noqa: E402
from lane_busy import CEILING_S, Busy  # noqa: E402

SAFE_WITHOUT_ORDERING = [n for n in T.CASES if n.startswith("cost_query-")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", default=None, choices=list(T.CASES))
    ap.add_argument("--only-case", action="store_true", help="time the writers of --case's family only (another library)")
    a = ap.parse_args()
    from art_planner_amd import _capi
    lines = [f"library: {os.path.relpath(_capi.LIB_PATH, ROOT)}", ""]
    names = SAFE_WITHOUT_ORDERING if a.only_case else list(T.CASES)
    lines.append(f"host time of W, all lanes idle (ms; median and min .. max of {a.reps} fresh contexts)")
    longest, seq = 0.0, {}
    for name in names:
        ts = []
        for _ in range(a.reps):
            r = T.run_case(name)
            r["case"].close()
            ts.append(r["host_seconds"])
            seq[name] = (r["old"], r["new"])
        ts.sort()
        longest = max(longest, ts[len(ts) // 2])
        lines.append(f"  {name:44s} {ts[len(ts) // 2] * 1e3:9.3f}   {ts[0] * 1e3:9.3f} .. {ts[-1] * 1e3:9.3f}")
    busy = Busy(T.DEV)
    fill = min(CEILING_S, T.MARGIN * longest)
    lines += ["", f"one filler product ({busy.a.shape[0]}^3, float32): {busy.seconds_per_product * 1e3:.3f} ms",
              f"filler: {T.MARGIN:g} x {longest * 1e3:.3f} ms, ceiling {CEILING_S * 1e3:.0f} ms -> {fill * 1e3:.1f} ms = "
              f"{busy.repeats(fill)} products"]
    if a.case:
        old, new = seq[a.case]
        r = T.run_case(a.case, busy, fill)
        r["case"].close()
        r_old, r_new = np.array_equal(r["old"], old), np.array_equal(r["new"], new)
        lines += ["", f"ordered run of {a.case}:",
                  f"  lane 1 busy before W: {r['busy_before']}, after W: {r['busy_after']}, W host {r['host_seconds'] * 1e3:.3f} ms, "
                  f"filler product as expected: {r['filler_ok']}",
                  f"  R  == result under the old state: {r_old}   (elements equal to the NEW result: "
                  f"{float((r['old'] == new).mean()):.3f})",
                  f"  R' == result under the new state: {r_new}",
                  f"  the test would {'PASS' if r_old and r_new and r['busy_before'] and r['filler_ok'] else 'FAIL'}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
