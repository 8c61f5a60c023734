"""The Lanczos step of the C3 workload (bench.py: masked 200k x 30k f64, 60 % mask, k = 30), uncentred and with the opt-in
centring (sapca_options.lanczos_center), across library builds on ONE box: boxes differ by +-4 %, builds are compared interleaved.

    python tools/lanczos_step_time.py [--rounds 4] [--fits 5] [build ...]

A build is `default` (the tree's library) or a name N / a path, as in tools/ab_libs.sh (lib/exp/libsapca_N.so).  Every round
runs one fresh process per (build, uncentred | centred); builds other than `default` (older libraries, which ignore the option's
byte) run uncentred only.
Prints every run and the medians: ms per step = lanczos_ms / lanczos_steps (HIP events on the library stream), and the whole
fit, where a centred fit also pays for the column statistics that no longer run beside its iterations."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(centred, fits):
    sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
    import torch
    import sapca
    from sapca import synth
    m, n, density, k = 200_000, 30_000, 0.03, 30
    ptr, idx, val = synth.gapped_csr(m, n, density, k, seed=42, centred=False, dtype=torch.float64, device="cuda")
    x = sapca.DeviceCsr(ptr, idx, val, (m, n))
    b = (sapca.MaskedSparsePCABuilder.new().n_components(k).mask(synth.bernoulli_mask(n, 0.6, 7).numpy()).collect_timings(True)
         .svd_method(sapca.SVDMethod.Lanczos()))
    if centred:
        b = b.lanczos_center()
    est = b.build()
    for _ in range(2):
        est.fit(x)
    lz, steps, total, stats = 0.0, 0, 0.0, 0.0
    for _ in range(fits):
        est.fit(x)
        t = est.timings()
        lz += t.lanczos_ms
        steps += int(t.lanczos_steps)
        total += t.fit_total_ms
        stats += t.stats_ms
    print(json.dumps({"step_ms": lz / steps, "steps_per_fit": steps / fits, "lanczos_ms": lz / fits, "fit_total_ms": total / fits,
                      "stats_ms": stats / fits}), flush=True)


def lib_path(name):
    if name == "default":
        return os.path.join(ROOT, "single-algebra_amd", "lib", "libsapca.so")
    return name if os.path.isfile(name) else os.path.join(ROOT, "single-algebra_amd", "lib", "exp", f"libsapca_{name}.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("builds", nargs="*", default=["default"])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--fits", type=int, default=5)
    ap.add_argument("--child", choices=["uncentred", "centred"])
    a = ap.parse_args()
    if a.child:
        return child(a.child == "centred", a.fits)
    runs = {}
    for r in range(a.rounds):
        for build in a.builds:
            path = lib_path(build)
            # (only the tree's build is known to have the option; an older library ignores the byte)
            for mode in ("uncentred", "centred") if build == "default" else ("uncentred",):
                env = dict(os.environ, SAPCA_LIB_PATH=path)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--fits", str(a.fits)], env=env,
                                   capture_output=True, text=True, timeout=300)
                if p.returncode != 0:   # a failed run ends the comparison: nothing more is started on the device
                    sys.exit(f"{build} {mode}: exit {p.returncode}\n{p.stderr[-2000:]}")
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                runs.setdefault((build, mode), []).append(rec)
                print(f"round {r} {build:10s} {mode:10s} " + "  ".join(f"{k} {v:.4f}" for k, v in rec.items()), flush=True)
    print("\nmedians of %d runs" % a.rounds)
    for (build, mode), recs in runs.items():
        print(f"{build:10s} {mode:10s} " + "  ".join(f"{k} {statistics.median(x[k] for x in recs):.4f}" for k in recs[0]))


if __name__ == "__main__":
    main()
