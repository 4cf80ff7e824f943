"""The MC pre-phase's two chains in a rocprofv3 kernel trace of bench.py (development tool, no GPU needed).

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 1 --warmup 1 --no-kernel-timers
  python tools/prephase_trace.py DIR/**/*kernel_trace.csv

Takes the LAST sampling call of the trace.  A call launches four time tables (time_embed_kernel): two at the start of
the pre-phase, one per chain, and two at the start of the guided loop.  Every Euler step of a chain ends with one
conv_out_kernel, so a chain is the launches of one stream up to its last conv_out_kernel before the guided loop.
Prints when each chain starts and ends, the step rate of the chain that ends last while the other runs beside it and
after the other has ended, and the idle time (gaps between consecutive launches) of that solo part."""
import csv
import sys
from collections import defaultdict


def main(path, column="Stream_Id"):
    rows = []
    for r in csv.DictReader(open(path)):
        key = r.get(column) or r["Queue_Id"]
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], key, r["Queue_Id"]))
    rows.sort()
    tables = [r for r in rows if "time_embed_kernel" in r[2]]
    if len(tables) < 4:
        raise SystemExit(f"{len(tables)} time-table launches: not a trace of a whole sampling call")
    t0, t_main = min(tables[-4][0], tables[-3][0]), tables[-2][0]
    chains = defaultdict(list)
    for r in rows:
        if t0 <= r[0] < t_main:
            chains[r[3]].append(r)
    ends = {}
    for key, ks in chains.items():
        outs = [i for i, k in enumerate(ks) if "conv_out_kernel" in k[2]]
        if outs:
            chains[key] = ks = ks[:outs[-1] + 1]
            ends[key] = (ks[-1][1], len(outs), sum(k[1] - k[0] for k in ks))
    if len(ends) != 2 and column != "Queue_Id":  # (a profiler version without stream ids)
        return main(path, "Queue_Id")
    if len(ends) != 2:
        raise SystemExit(f"{len(ends)} streams with Euler steps in the pre-phase (expected 2): {sorted(ends)}")
    short, long_ = sorted(ends, key=lambda k: ends[k][2])
    ms = 1e-6
    length = (max(e[0] for e in ends.values()) - t0) * ms
    for name, key in (("short", short), ("long", long_)):
        e = ends[key]
        print(f"{name} chain (stream {key}, hardware queue {chains[key][0][4]}): {e[1]} steps, {len(chains[key])} launches, "
              f"kernel time {e[2] * ms:.1f} ms, first launch starts at {(chains[key][0][0] - t0) * ms:.1f} ms, "
              f"last launch ends at {(e[0] - t0) * ms:.1f} ms")
    gap = abs(ends[long_][0] - ends[short][0]) * ms
    print(f"pre-phase length {length:.1f} ms; the chains end {gap:.1f} ms apart = {100 * gap / length:.1f} % of it")
    early, late = sorted(ends, key=lambda k: ends[k][0])
    name = "long" if late == long_ else "short"
    t_early = ends[early][0]
    ks = chains[late]
    step_ends = [k[1] for k in ks if "conv_out_kernel" in k[2]]
    co = [t for t in step_ends if t <= t_early]
    solo = [t for t in step_ends if t > t_early]
    if len(co) > 1:
        span = (co[-1] - co[0]) * ms
        print(f"{name} chain beside the other: {len(co) - 1} steps in {span:.1f} ms = {span / (len(co) - 1):.3f} ms/step")
    if len(solo) > 1:
        span = (solo[-1] - solo[0]) * ms
        print(f"{name} chain solo: {len(solo) - 1} steps in {span:.1f} ms = {span / (len(solo) - 1):.3f} ms/step")
        tail = [k for k in ks if k[0] >= t_early]
        idle = sum(max(0, b[0] - a[1]) for a, b in zip(tail, tail[1:])) * ms
        print(f"  solo tail after the other chain's end: {(ends[late][0] - t_early) * ms:.1f} ms; idle between its launches "
              f"{idle:.2f} ms over {len(tail)} launches = {1e3 * idle / max(len(tail) - 1, 1):.2f} us per launch")
    else:
        print(f"no solo tail to speak of: {len(solo)} step(s) of the {name} chain end after the other chain")

if __name__ == "__main__":
    main(sys.argv[1])
