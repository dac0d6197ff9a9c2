"""The launch stream of a `rocprofv3 --kernel-trace -f csv` run as text.  A launch is the line
    <kernel name> grid=<x,y,z> wg=<x,y,z> lds=<bytes> q=<hardware queue>
(grid in work-items, as the profiler reports it; the kernel's parameter list is dropped from its name; the queue stands for the stream — the
profiler's own stream label is not stable for a stream's first launch).  Per host thread, in dispatch order — threads in the order of their
first dispatch, the busiest one, the thread that runs the tests, as "main" — the default output is the whole list, one line per run of equal
launches (`<repeats> x <launch>`): two builds whose host code enqueues the same kernels in the same shapes on the same streams give the same
text, and `diff` says where they do not.  --digest prints, per thread, the number of launches and the SHA-256 of that ordered list, and for
the main thread a table `<launches> x <kernel> wg lds q grids=<distinct grids>`: small enough to keep, and equal hashes are equal lists.
--no-runtime-copies leaves out the runtime's own copy and fill kernels (__amd_rocclr_*: hipMemcpyAsync / hipMemsetAsync).
Usage: python tools/dev/kernel_trace_list.py [--digest] [--no-runtime-copies] <directory of *kernel_trace.csv[.gz]> > launches.txt"""
import collections
import csv
import glob
import gzip
import hashlib
import os
import re
import sys


def rows_of(path):
    with (gzip.open(path, "rt", newline="") if path.endswith(".gz") else open(path, newline="")) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            yield (int(r["Dispatch_Id"]), r["Thread_Id"],
                   f'{name} grid={r["Grid_Size_X"]},{r["Grid_Size_Y"]},{r["Grid_Size_Z"]} '
                   f'wg={r["Workgroup_Size_X"]},{r["Workgroup_Size_Y"]},{r["Workgroup_Size_Z"]} lds={r["LDS_Block_Size"]} q={r["Queue_Id"]}')


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    skip_copies, digest = "--no-runtime-copies" in sys.argv, "--digest" in sys.argv
    files = sorted(glob.glob(os.path.join(args[0], "**", "*kernel_trace.csv*"), recursive=True))
    for path in files:
        rows = sorted(r for r in rows_of(path) if not (skip_copies and r[2].startswith("__amd_rocclr_")))
        threads = collections.OrderedDict()
        for _, tid, line in rows:
            threads.setdefault(tid, []).append(line)
        busiest = max(threads, key=lambda t: len(threads[t]))
        print(f"# {os.path.basename(path)}: {len(rows)} launches on {len(threads)} host threads")
        for k, (tid, lines) in enumerate(threads.items()):
            head = f"# thread {k}{' (main)' if tid == busiest else ''}: {len(lines)} launches"
            if digest:
                print(f"{head}, ordered list sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
                if tid == busiest:
                    count, grids = collections.Counter(), collections.defaultdict(set)
                    for line in lines:
                        shape = re.sub(r" grid=\S+", "", line)
                        count[shape] += 1
                        grids[shape].add(line)
                    for shape in sorted(count):
                        print(f"{count[shape]} x {shape} grids={len(grids[shape])}")
                continue
            print(head)
            run, last = 0, None
            for line in lines + [None]:
                if line != last and last is not None:
                    print(f"{run} x {last}")
                    run = 0
                last = line
                run += 1


if __name__ == "__main__":
    main()
