"""A rocprofv3 kernel trace of tools/relaybench.py taken apart call by call:
per shape (told by the grid of the plan's first kernel) and per call (the
echo's, the relay's in one room, the relay's in many rooms, in the order the
tool issues them), the median duration in microseconds of the reply's
k_msg_gather, the relay's (the launch behind k_relay_finalize) and each relay
plan kernel.

usage: python tools/relay_trace_split.py RUN_kernel_trace.csv
"""
import csv
import statistics
import sys
from collections import defaultdict


def main(path):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("wsg::", "")
        took = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if name.startswith(("k_msg_scan_local", "k_rfc_scan_local")):   # a call's first kernel
            cur = {"k": {}, "frames": int(r["Grid_Size_X"]), "last": ""}
            calls.append(cur)
        if cur is None:
            continue
        if name.startswith("k_msg_gather"):
            cur["k"]["gather_relay" if cur["last"].startswith("k_relay_finalize") else "gather_reply"] = took
        elif name.startswith("k_relay"):
            cur["k"][name] = took
        cur["last"] = name
    groups, nth = defaultdict(list), defaultdict(int)
    for c in calls:
        if not any(k.startswith("k_relay") for k in c["k"]):
            kind, nth[c["frames"]] = "echo", 0
        else:
            nth[c["frames"]] += 1
            kind = "relay_one_room" if nth[c["frames"]] == 1 else "relay_many_rooms"
        groups[(c["frames"], kind)].append(c["k"])
    for (frames, kind), calls_ in sorted(groups.items()):
        names = sorted({k for c in calls_ for k in c})
        print("plan grid %d  %-16s calls %d  " % (frames, kind, len(calls_)) + "  ".join(
            "%s %.2f" % (n, statistics.median(c[n] for c in calls_ if n in c) / 1e3) for n in names))


if __name__ == "__main__":
    main(sys.argv[1])
