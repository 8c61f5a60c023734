"""Step-by-step timeline of the last Lanczos fit in rocprofv3 kernel traces of tools/lanczos_step_time.py's child:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/lanczos_step_time.py --child centred --fits 1
    python tools/lanczos_step_timeline.py LABEL=OUT/.../N_kernel_trace.csv [LABEL=...]

Prints the kernels of step 20 and, for steps 1..40 and 40..79, the start-to-start time of a step and the mean duration of
each kernel: fits that take different numbers of steps are compared at EQUAL step indices (a step's re-orthogonalisation and
convergence check grow with the size of the basis)."""
import collections
import csv
import re
import statistics
import sys


def steps_of_last_fit(path):
    rows = []
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\((?!anonymous).*", "", r["Kernel_Name"]).replace("void ", "")
        name = name.replace("sapca::(anonymous namespace)::", "").replace("sapca::k::(anonymous namespace)::", "k::")
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    first = [i for i, r in enumerate(rows) if "count_kept" in r[2]][-1]   # (the mask compaction opens a masked fit)
    fit = [r for r in rows[first:] if "at::" not in r[2] and "rocprim" not in r[2] and "rocclr" not in r[2]]
    at = [i for i, r in enumerate(fit) if r[2].startswith("spmv_ldsx")]
    return [fit[at[j]:at[j + 1]] for j in range(len(at) - 1)]


def main():
    fits = {}
    for arg in sys.argv[1:]:
        label, path = arg.split("=", 1)
        fits[label] = steps_of_last_fit(path)
        print(f"{label}: {len(fits[label]) + 1} steps")
    print("\nstep 20")
    for label, st in fits.items():
        print(label)
        for a, b, n in st[20]:
            print("   %-50s start %7.1f us  duration %6.1f us" % (n[:50], (a - st[20][0][0]) / 1e3, (b - a) / 1e3))
    for lo, hi in ((1, 40), (40, 79)):
        for label, all_steps in fits.items():
            st = all_steps[lo:hi]
            if len(st) < 2:
                continue
            wall = [(st[i + 1][0][0] - st[i][0][0]) / 1e3 for i in range(len(st) - 1)]
            print(f"\n{label}, steps {lo}..{lo + len(st) - 1}: start to start median {statistics.median(wall):.1f} us, mean {statistics.mean(wall):.1f} us")
            per = collections.defaultdict(list)
            for s in st:
                for a, b, n in s:
                    per[n[:50]].append((b - a) / 1e3)
            for n, v in per.items():
                print("   %-50s %.2f per step, mean %6.1f us" % (n, len(v) / len(st), statistics.mean(v)))


if __name__ == "__main__":
    main()
