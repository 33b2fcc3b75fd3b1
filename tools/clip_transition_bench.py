#!/usr/bin/env python3
"""File playback through a MIX or WIPE: ph_clip_compose_transition_multi against what the same frames cost without it, timed with device
events, in microseconds per frame.  Sides:
  trans  the new entry - once with the context option "chan_enlarged" = 1 (one launch of clip_up_trans_kernel per writer table) and once
         with 2 (never the one-launch form: the format readers, then compose_up_trans)
  multi  ph_clip_compose_multi on the same arguments: a layer in a transition sends it to the channel kernel - what these frames took
         before the entry existed
The sides alternate on warmed shapes inside every round.  The baseline of record is the multi side of a build of the PARENT commit, run in
the same session from a directory of its own: run this file there with mode=baseline (it then never names the new entry) in front of and
behind the run of this build, and give both files to this build's run as parent=<file>,<file>; their rounds are merged per shape.
The clips are seeded, so every process makes the same frames: a baseline record carries the SHA-256 of its output planes, and this build
compares the new entry's planes with it - and, byte for byte, with its own multi side - BEFORE it times a shape; a difference ends the run.
Shapes, each for both routes: two 1080p yuv420p files dissolving on a 1080p channel -> nv12, and -> v210 + rgba8; a 720p file dissolving
into a 1080p one -> nv12; two 1080p p010 files on a 2160p channel -> yuv422p10; a wipe of two 1080p yuv420p files through a 960 x 540 v210
mask clip -> nv12.
  python tools/clip_transition_bench.py [reps=200] [rounds=7] [out=profiles/clip_transition_bench.jsonl] [mode=both|baseline] [parent=<jsonl>[,<jsonl>]]
One JSON line per shape and route: every side's median over the rounds, its spread (max - min over the rounds) and its route from a
dry-run trace; whether the entry wins, loses or equals the baseline beyond the baseline's spread (or its own, where that is larger)."""
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
    path = pos[2] if len(pos) > 2 else os.path.join(ROOT, "profiles", "clip_transition_bench.jsonl")
    baseline_only = kw.get("mode", "both") == "baseline"
    parent, parent_sha = {}, {}
    for f in [p for p in kw.get("parent", "").split(",") if p]:
        for line in open(f):
            rec = json.loads(line)
            parent.setdefault(rec["shape"], []).extend(rec["rounds_multi_us"])
            parent_sha.setdefault(rec["shape"], set()).add(rec["sha256"])
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    formats = ("v210", "yuv422p10", "yuv420p", "nv12", "rgba8", "p010")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE[f])) for f in formats}
    rd_own = {f: dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE[f])) if capi.FORMAT_RANGE[f] and capi.FORMAT_RANGE[f][0] == 8 else None for f in formats}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of frames: no clip is read from the cache the launch before left it in
    gen = torch.Generator(device="cuda")

    def planes(fmt, w, h, random=False):
        sizes = [capi.v210_pitch_bytes(w) * h] if fmt == "v210" else capi.pack_plane_bytes(fmt, w, h)
        if random and fmt == "v210":  # (10-bit codes of any value in whole words: only the time counts)
            return [(torch.randint(0, 1 << 30, (n // 4,), dtype=torch.int32, device="cuda", generator=gen)).view(torch.uint8) for n in sizes]
        if random:  # (8-bit codes of any value)
            return [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen) for n in sizes]
        return [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in sizes]

    HD, UHD, P720, QHD = (1920, 1080), (3840, 2160), (1280, 720), (960, 540)
    # (name, kind, [(clip format, clip size)]: src, incoming, mask; channel size, outputs)
    shapes = [("two 1080p yuv420p dissolving -> nv12", "dissolve", [("yuv420p", HD), ("yuv420p", HD)], HD, ["nv12"]),
              ("two 1080p yuv420p dissolving -> v210+rgba8", "dissolve", [("yuv420p", HD), ("yuv420p", HD)], HD, ["v210", "rgba8"]),
              ("720p yuv420p dissolving into 1080p -> nv12", "dissolve", [("yuv420p", P720), ("yuv420p", HD)], HD, ["nv12"]),
              ("two 1080p p010 dissolving on 2160p -> yuv422p10", "dissolve", [("p010", HD), ("p010", HD)], UHD, ["yuv422p10"]),
              ("two 1080p yuv420p wiping through a 960x540 v210 mask -> nv12", "wipe", [("yuv420p", HD), ("yuv420p", HD), ("v210", QHD)], HD, ["nv12"])]
    lines = []
    for index, (name, kind, clips, (w, h), outs) in enumerate(shapes):
        gen.manual_seed(20261021 + index)
        ring = []
        for _ in range(R):
            imgs = []
            for fmt, (sw, sh) in clips:
                p = planes(fmt, sw, sh, random=True)
                imgs.append((p[0], sw, sh, capi.transform_matrix(w, h)) if fmt == "v210" else (tuple(p), sw, sh, capi.transform_matrix(w, h), fmt, rd_own[fmt]))
            ring.append([dict(zip(("src", "incoming", "mask"), imgs), transition=kind, mix=0.5)])
        dst = [planes(fmt, w, h) for fmt in outs]
        torch.cuda.synchronize()
        outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
        multi = [ctx.clip_compose_multi(ring[s], outputs, w, h, *rd, prepare_only=True) for s in range(R)]
        trans = None if baseline_only else [ctx.clip_compose_transition_multi(ring[s], outputs, w, h, *rd, prepare_only=True) for s in range(R)]

        def frame_of(fn):
            """the output planes of frame 0 of the ring, as bytes"""
            for d in dst:
                for p in d:
                    p.fill_(0x5A)
            torch.cuda.synchronize()
            fn(0)
            ctx.wait()
            torch.cuda.synchronize()
            return [p.cpu().numpy().tobytes() for d in dst for p in d]

        def sha(frame):
            hsh = hashlib.sha256()
            for b in frame:
                hsh.update(b)
            return hsh.hexdigest()

        for option in ([1] if baseline_only else [1, 2]):
            shape = name if baseline_only else "%s [chan_enlarged=%d]" % (name, option)
            sides = {"multi": lambda i: multi[i]()}
            if not baseline_only:
                sides["trans"] = lambda i: trans[i]()
            # the bytes first: nothing is timed that does not make the baseline's frame
            ctx.set_option("chan_enlarged", option)
            frames = {k: frame_of(fn) for k, fn in sides.items()}
            digest = sha(frames["multi"])
            if not baseline_only:
                assert frames["trans"] == frames["multi"], "%s: the entry's planes differ from ph_clip_compose_multi's" % shape
                assert not parent_sha.get(name) or parent_sha[name] == {digest}, "%s: the planes differ from the parent build's (%s against %s)" % (shape, digest, parent_sha[name])
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
            ctx.set_option("chan_enlarged", 1)
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = {k: max(v) - min(v) for k, v in us.items()}
            line = {"bench": "clip_transition", "shape": shape if not baseline_only else name, "kind": kind, "clips": [[fmt, sw, sh] for fmt, (sw, sh) in clips], "width": w, "height": h,
                    "outputs": outs, "reps": reps, "rounds": rounds, "unit": "us per frame", "routes": routes, "sha256": digest, "multi_us": round(med["multi"], 2),
                    "multi_spread_us": round(spread["multi"], 2), "rounds_multi_us": [round(v, 2) for v in us["multi"]]}
            if not baseline_only:
                line.update({"chan_enlarged": option, "trans_us": round(med["trans"], 2), "trans_spread_us": round(spread["trans"], 2), "rounds_trans_us": [round(v, 2) for v in us["trans"]]})
                base, base_spread, which = med["multi"], spread["multi"], "multi (this build)"
                if name in parent:
                    base, base_spread, which = statistics.median(parent[name]), max(parent[name]) - min(parent[name]), "multi (parent build, same session)"
                    line.update({"parent_multi_us": round(base, 2), "parent_multi_spread_us": round(base_spread, 2), "rounds_parent_multi_us": parent[name],
                                 "bytes_equal_parent": True})
                worst = max(spread["trans"], base_spread)
                saved = base - med["trans"]
                line.update({"baseline": which, "saved_us": round(saved, 2), "verdict": "wins" if saved > worst else "loses" if -saved > worst else "equal within spread"})
            print(json.dumps(line), flush=True)
            lines.append(line)
        del ring, dst, multi, trans
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
