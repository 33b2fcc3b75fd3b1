#!/usr/bin/env python3
"""720p channels (1280 x 720: every v210 line ends in a tail quad) with SDI's v210 frame among several consumers: the context option
"up_v210_tails" = 1 - the v210 output stays inside its writer table's launch of the several-outputs kernels - against the option's
default 0, where it is made on its own; timed with device events, in microseconds per call.  Sides:
  opt0  the entry with the option at 0 (today's routes)
  opt1  the same call with the option at 1
The sides alternate on warmed shapes inside every round.  The baseline of record is a build of the PARENT commit, run in the same session:
run this file with mode=parent and PHANERON_HIP_LIB=<the parent's library> (it then never names the option) twice - in front of this
build's run and again behind it - and give both files to this build's run of record as parent=<file>,<file>; their rounds are merged per
shape.  opt0 must equal the parent within the spreads (the record says whether it does).  The sources are seeded, so every process makes
the same frames: a record carries the SHA-256 of the output planes, and this build compares opt1's bytes with opt0's byte for byte and
with the parent's digest BEFORE it times a shape; a difference ends the run.
  python tools/up_tails_bench.py [reps=200] [rounds=7] [out=profiles/up_tails_bench.jsonl] [mode=both|parent] [parent=<jsonl>[,<jsonl>]]
One JSON line per shape: every side's median over the rounds, its spread (max - min over the rounds) and its route from a dry-run trace;
whether the option wins, loses or ties beyond the larger of the two spreads."""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    pos = [a for a in sys.argv[1:] if "=" not in a]
    kw = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    reps = int(pos[0]) if len(pos) > 0 else 200
    rounds = int(pos[1]) if len(pos) > 1 else 7
    path = pos[2] if len(pos) > 2 else os.path.join(ROOT, "profiles", "up_tails_bench.jsonl")
    parent_only = kw.get("mode", "both") == "parent"
    parent, parent_sha = {}, {}
    for f in [p for p in kw.get("parent", "").split(",") if p]:
        for line in open(f):
            rec = json.loads(line)
            parent.setdefault(rec["shape"], []).extend(rec["rounds_opt0_us"])
            parent_sha.setdefault(rec["shape"], set()).add(rec["sha256"])
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    formats = ("v210", "yuv422p8", "yuv420p", "nv12", "rgba8")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE[f])) for f in formats}
    rd_own = dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE["yuv420p"]))
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of frames: no source is read from the cache the launch before left it in
    gen = torch.Generator(device="cuda")
    W, H = 1280, 720

    def planes(fmt, w, h, random=False):
        sizes = [capi.v210_pitch_bytes(w) * h] if fmt == "v210" else capi.pack_plane_bytes(fmt, w, h)
        if random:  # (codes of any value: only the time counts)
            return [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen) for n in sizes]
        return [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in sizes]

    def outputs_of(outs):
        dst = [planes(fmt, W, H) for fmt in outs]
        return dst, [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]

    def clip_layers(sw, sh):
        p = planes("yuv420p", sw, sh, random=True)
        return [dict(src=(tuple(p), sw, sh, capi.transform_matrix(W, H), "yuv420p", rd_own), transition="cut", mix=0.0)]

    # (name, kind, source size, outputs, jobs)
    shapes = [("720p yuv420p under the default fill -> v210 + rgba8", "clip", (1280, 720), ["v210", "rgba8"], 1),
              ("720p yuv420p under the default fill -> v210 + yuv422p8 + rgba8", "clip", (1280, 720), ["v210", "yuv422p8", "rgba8"], 1),
              ("720 x 576 yuv420p filling the channel -> v210 + nv12", "clip", (720, 576), ["v210", "nv12"], 1),
              ("four channels of 720p yuv420p -> v210 + rgba8, ph_clip_compose_batch_out", "batch", (1280, 720), ["v210", "rgba8"], 4),
              ("two 720 x 576 packed-RGB fields per frame -> v210 + rgba8, ph_compose_up_write_multi jobs = 2", "up", (720, 576), ["v210", "rgba8"], 2)]
    lines = []
    for index, (name, kind, (sw, sh), outs, jobs) in enumerate(shapes):
        gen.manual_seed(20261022 + index)
        per_job = [outputs_of(outs) for _ in range(jobs)]
        all_planes = [p for dst, _ in per_job for d in dst for p in d]
        keep, calls = [], []
        for _ in range(R):
            if kind == "clip":
                layers = clip_layers(sw, sh)
                keep.append(layers)
                calls.append(ctx.clip_compose_multi(layers, per_job[0][1], W, H, *rd, prepare_only=True))
            elif kind == "batch":
                js = [(clip_layers(sw, sh), per_job[j][1]) for j in range(jobs)]
                keep.append(js)
                calls.append(ctx.clip_compose_batch_out(js, W, H, *rd, prepare_only=True))
            else:
                sets = [[(torch.rand(sw * sh * 3, dtype=torch.float32, device="cuda", generator=gen), sw, sh, capi.transform_matrix(W, H))] for _ in range(jobs)]
                keep.append(sets)
                calls.append(ctx.compose_up_write_multi(sets, [per_job[j][1] for j in range(jobs)], W, H, rgb=True, prepare_only=True))
        torch.cuda.synchronize()

        def side(value):
            def run(i):
                if not parent_only:
                    ctx.set_option("up_v210_tails", value)
                calls[i]()
            return run
        sides = {"opt0": side(0)} if parent_only else {"opt0": side(0), "opt1": side(1)}

        def frame_of(fn):
            for p in all_planes:
                p.fill_(0x5A)
            torch.cuda.synchronize()
            fn(0)
            ctx.wait()
            torch.cuda.synchronize()
            return [p.cpu().numpy().tobytes() for p in all_planes]

        def sha(frame):
            hsh = hashlib.sha256()
            for b in frame:
                hsh.update(b)
            return hsh.hexdigest()

        frames = {k: frame_of(fn) for k, fn in sides.items()}
        digest = sha(frames["opt0"])
        if not parent_only:
            assert frames["opt1"] == frames["opt0"], "%s: the planes with the option at 1 differ from those with 0" % name
            assert not parent_sha.get(name) or parent_sha[name] == {digest}, "%s: the bytes differ from the parent build's (%s against %s)" % (name, digest, parent_sha[name])
        routes = {}
        for k, fn in sides.items():
            with capi.trace(dry_run=True) as t:
                fn(0)
            routes[k] = t.route

        def timed(k):
            fn = sides[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                fn(i % R)
            e1.record(stream)
            ctx.wait()
            return 1e3 * e0.elapsed_time(e1) / reps
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # until every shape is warm and the clocks have settled
            for k in sides:
                for i in range(R):
                    sides[k](i)
            ctx.wait()
        us = {k: [] for k in sides}
        for _ in range(rounds):  # the sides alternate inside a round
            for k in sides:
                us[k].append(timed(k))
        if not parent_only:
            ctx.set_option("up_v210_tails", 0)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        line = {"bench": "up_tails", "shape": name, "source": [sw, sh], "width": W, "height": H, "outputs": outs, "jobs": jobs, "reps": reps, "rounds": rounds,
                "unit": "us per call", "routes": routes, "sha256": digest, "opt0_us": round(med["opt0"], 2), "opt0_spread_us": round(spread["opt0"], 2),
                "rounds_opt0_us": [round(v, 2) for v in us["opt0"]]}
        if not parent_only:
            line.update({"opt1_us": round(med["opt1"], 2), "opt1_spread_us": round(spread["opt1"], 2), "rounds_opt1_us": [round(v, 2) for v in us["opt1"]]})
            base, base_spread, which = med["opt0"], spread["opt0"], "opt0 (this build)"
            if name in parent:
                base, base_spread, which = statistics.median(parent[name]), max(parent[name]) - min(parent[name]), "parent build, same session"
                gap = med["opt0"] - base
                line.update({"parent_us": round(base, 2), "parent_spread_us": round(base_spread, 2), "rounds_parent_us": parent[name], "bytes_equal_parent": True,
                             "opt0_minus_parent_us": round(gap, 2), "opt0_equals_parent_within_spread": abs(gap) <= max(spread["opt0"], base_spread)})
            worst = max(spread["opt1"], base_spread)
            saved = base - med["opt1"]
            line.update({"baseline": which, "saved_us": round(saved, 2), "verdict": "wins" if saved > worst else "loses" if -saved > worst else "ties"})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del keep, calls, per_job, all_planes
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
