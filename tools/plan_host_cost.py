#!/usr/bin/env python3
"""What planning a ph_run_programs call costs its caller's thread: the host time of an eight-job call of each kind of shared launch, in
a dry run (ph_trace_begin(1): every check is made, every launch chosen, nothing enqueued), in microseconds per call.  Two builds of the
library side by side - this tree's and another (the parent commit's, built as a variant) - in fresh processes that alternate:
  python tools/plan_host_cost.py parent=<libphaneron_hip.so of the other build> [runs=5] [calls=2000] [out=profiles/plan_host_cost.jsonl]
Kinds (ph_run_programs' numbering), eight jobs without a hazard each, so every job is held against every job before it in its launch:
  1 chan_compose_v210_1, 2 fused_v210_combine_2, 3 compose_up_write_v210_1 - tests/test_call_order_gpu.py's rig, 384 x 54;
  4 chan_compose_v210_1 with outPacking yuv422p8 (option chan_batch_outs) - tests/test_chan_batch_out_gpu.py's named_jobs;
  5 fused_v210_combine_multi_2 for three consumers (option fused_multi_batch) - tests/test_fused_multi_gpu.py's three_outputs, 384 x 6;
  6 clip_compose_multi_1 for two consumers (option clip_batch) - tests/test_clip_multi_gpu.py's clip_params.
One JSON line per kind: both builds' runs, medians, the parent's spread (max - min of its runs) and whether this build's median stays
within the parent's median plus that spread.  `python tools/plan_host_cost.py run [calls]` is one process's run of the build that
PHANERON_HIP_LIB names: one JSON line {kind: us per call}."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHUNK = 10  # calls per trace: the route of a trace stays short


def calls_of():
    """{kind: (context, jobs)} - the eight-job calls"""
    import numpy as np
    import call_order as co
    import frames
    from phaneron_amd import capi
    from test_call_order_gpu import Rig, upload
    from test_chan_batch_out_gpu import named_jobs
    from test_chan_multi_gpu import ByName
    from test_clip_multi_gpu import SH, SW, clip_params
    from test_fused_multi_gpu import layer_words, three_outputs
    ctx = capi.Context(0)
    rig = Rig(ctx)
    words = frames.v210_random(co.W, co.IMAGE_BYTES // (co.W * 8 // 3), 170)
    # buffers 0-7: images (layer images of the compositor), 8-15: frames (v210 sources), 16-23: outputs - no job touches another's
    pool = [upload(ctx, words, dims=(co.SW, co.SH) if i < 8 else None) for i in range(24)]
    ctx.wait(capi.QUEUE_LOAD)
    kinds = {1: (ctx, [rig.job(co.job("chan", 1, [8 + i], 16 + i, small=[True]), pool) for i in range(8)]),
             2: (ctx, [rig.job(co.job("fused", 2, [8 + i, 8 + (i + 1) % 8], 16 + i), pool) for i in range(8)]),
             3: (ctx, [rig.job(co.job("up", 1, [i], 16 + i), pool) for i in range(8)])}
    b = ByName(384, 54)
    b.progs = []
    b.ctx.set_option("chan_batch_outs", 1)
    b.ctx.set_option("clip_batch", 1)
    kinds[4] = (b.ctx, named_jobs(b, ["yuv422p8"] * 8, 2400)[0])
    clip = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [b.w, b.h])
    kinds[6] = (b.ctx, [(clip, clip_params(b, frames.pack_random("yuv420p", SW, SH, 3900 + j))[0]) for j in range(8)])
    f = ByName(384, 6)
    f.ctx.set_option("fused_multi_batch", 1)
    multi = f.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [f.w, f.h])
    kinds[5] = (f.ctx, [(multi, three_outputs(f, [f.upload(l, svm="coarse") for l in layer_words(f.w, f.h, 2, 60 + j)])[0]) for j in range(8)])
    for c in (b.ctx, f.ctx):
        c.wait(capi.QUEUE_LOAD)
    return kinds


def run(calls):
    import ctypes as C
    from phaneron_amd import capi
    lib = capi.lib()
    route = C.create_string_buffer(1 << 16)
    result, routes = {}, {}
    for kind, (ctx, jobs) in sorted(calls_of().items()):
        marshalled = [ctx._args(params) for _, params in jobs]
        progs = (C.c_void_p * len(jobs))(*[p.h for p, _ in jobs])
        args = (C.POINTER(capi.PhArg) * len(jobs))(*[C.cast(a, C.POINTER(capi.PhArg)) for a, _ in marshalled])
        counts = (C.c_int * len(jobs))(*[len(params) for _, params in jobs])

        def chunk():
            capi.check(lib.ph_trace_begin(1))
            for _ in range(CHUNK):
                rc = lib.ph_run_programs(ctx.h, len(jobs), progs, args, counts, capi.QUEUE_PROCESS)
            capi.check(lib.ph_trace_end(route, len(route)))
            capi.check(rc, ctx.h)
        for _ in range(20):
            chunk()
        launches = route.value.decode().split("+")
        routes[kind] = "+".join(launches[:len(launches) // CHUNK])  # one call's
        t0 = time.perf_counter()
        for _ in range(calls // CHUNK):
            chunk()
        result[kind] = round(1e6 * (time.perf_counter() - t0) / (calls // CHUNK * CHUNK), 3)
    print(json.dumps({"us_per_call": result, "routes": routes}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        return run(int(sys.argv[2]) if len(sys.argv) > 2 else 2000)
    kw = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    runs, calls = int(kw.get("runs", 5)), int(kw.get("calls", 2000))
    path = kw.get("out", os.path.join(ROOT, "profiles", "plan_host_cost.jsonl"))
    libs = {"parent": os.path.abspath(kw["parent"]), "this": os.path.join(ROOT, "phaneron_amd", "lib", "libphaneron_hip.so")}
    us, routes = {k: {} for k in libs}, {}
    for _ in range(runs):  # the builds alternate, a fresh process each
        for build, lib in libs.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(calls)], env=dict(os.environ, PHANERON_HIP_LIB=lib), capture_output=True,
                                 text=True, timeout=600)
            if out.returncode != 0:
                sys.exit("the %s build's run failed:\n%s%s" % (build, out.stdout, out.stderr))
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            for kind, v in rec["us_per_call"].items():
                us[build].setdefault(kind, []).append(v)
            routes.setdefault(build, rec["routes"])
    lines = []
    for kind in sorted(us["this"]):
        p, t = us["parent"][kind], us["this"][kind]
        spread = max(p) - min(p)
        line = {"bench": "plan_host_cost", "kind": int(kind), "jobs": 8, "calls_per_run": calls, "unit": "us per ph_run_programs call (dry run)", "route": routes["this"][kind],
                "same_route": routes["this"][kind] == routes["parent"][kind], "parent_us": p, "this_us": t, "parent_median_us": round(statistics.median(p), 3),
                "this_median_us": round(statistics.median(t), 3), "parent_spread_us": round(spread, 3),
                "within_parent_spread": statistics.median(t) <= statistics.median(p) + spread}
        print(json.dumps(line), flush=True)
        lines.append(line)
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
