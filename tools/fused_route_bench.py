#!/usr/bin/env python3
"""A routed channel's frame - f32 RGBA images among the plain v210 layers, the combined image beside the consumers' frames: ONE
ph_fused_v210_route_multi call against the chain that made such a frame before, through entry points this change does not touch -
ph_v210_read_batch + ph_combine + ph_pack_write_multi (ph_v210_write for one v210 frame), or, where no image is wanted,
ph_chan_compose_multi - in one process, the sides alternating on warmed shapes, timed with device events.  The layers cycle over a ring
of frame sets larger than the 256 MiB Infinity Cache, as bench.py's headline does; the chain's intermediate images are one set.
  python tools/fused_route_bench.py [reps=1000] [rounds=7] [out=profiles/fused_route_bench.jsonl] [only=<shape name>]
One JSON line per shape: the median of the rounds for both sides and each side's spread (max - min over the rounds).  The new call
counts as faster only if it wins by more than the chain side's spread; a shape that loses says so (with image_out there is no other
route to go back to).  One device only: nothing here was measured on more than one."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

CACHE_BYTES = 256 << 20
# per shape: its name, the number of v210 layers, whether a routed image lies on top, whether the image is written, the outputs
SHAPES = [("config 5: 3 v210 + routed image -> image + v210", 3, True, True, ["v210"]),
          ("3 v210 + routed image -> image + v210 + rgba8", 3, True, True, ["v210", "rgba8"]),
          ("source only: 4 v210 -> image + v210", 4, False, True, ["v210"]),
          ("sink only: 3 v210 + routed image -> v210 + yuv422p8", 3, True, False, ["v210", "yuv422p8"]),
          ("image alone: 3 v210 + routed image -> image", 3, True, True, [])]


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "fused_route_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    lib, hnd, ptr, q = capi.lib(), ctx.h, capi._ptr, capi.QUEUE_PROCESS
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rspec, wspec = "709", "2020"
    rd_lut_h, wr_lut_h = capi.gamma2linear_lut(rspec), capi.linear2gamma_lut(wspec)
    rd = (dev(capi.ycbcr2rgb_matrix(rspec)), dev(rd_lut_h), dev(np.concatenate([capi.rgb2rgb_matrix(rspec, wspec), np.zeros(3, np.float32)])))
    wr_lut = dev(wr_lut_h)
    fmts = ("v210", "yuv422p8", "rgba8")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix(wspec, *capi.FORMAT_RANGE[f])) for f in fmts}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], rd_lut_h)
    ctx.register_lut(wr_lut, wr_lut_h)

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h, dtype=torch.uint8, device="cuda")]
        return [torch.empty(b, dtype=torch.uint8, device="cuda") for b in capi.pack_plane_bytes(fmt, w, h)]

    def call(fn, *args):  # the C call alone, its arguments made once
        def job(_keep=args):
            capi.check(fn(*args), hnd)
        return job

    lines = []
    for size, w, h in [("2160p", 3840, 2160), ("1080p", 1920, 1080)]:
        frame_bytes = capi.v210_pitch_bytes(w) * h
        ring = CACHE_BYTES // (4 * frame_bytes) + 2
        gen = torch.Generator(device="cuda").manual_seed(5)
        words = lambda: torch.randint(0, 2 ** 31 - 1, (frame_bytes // 4,), dtype=torch.int32, device="cuda", generator=gen) & 0x3FFFFFFF
        sets = [[words() for _ in range(4)] for _ in range(ring)]
        routed = [torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=gen) for _ in range(ring)]
        rgba = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(4)]  # the chain's images of its v210 layers
        image_new, image_chain = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        for shape, n_v210, has_image, wants_image, outs in SHAPES:
            name = "%s %s" % (size, shape)
            if only and only != name:
                continue
            dst = [frame(fmt, w, h) for fmt in outs]
            torch.cuda.synchronize()
            outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
            n = n_v210 + (1 if has_image else 0)
            new, chain = [], []
            for s in range(ring):
                layers = sets[s][:n_v210] + ([dict(data=routed[s], format="rgba")] if has_image else [])
                new.append(ctx.fused_v210_route_multi(layers, image_new if wants_image else None, outputs, w, h, *rd, prepare_only=True))
                if not wants_image:
                    cl = [dict(src=(t, w, h, None), transition="cut", mix=0.0) for t in sets[s][:n_v210]] + [dict(src=(routed[s], w, h, None, "rgba"), transition="cut", mix=0.0)]
                    chain.append([ctx.chan_compose_multi(cl, outputs, w, h, *rd, prepare_only=True)])
                    continue
                ins = (C.c_void_p * n_v210)(*[ptr(t).value for t in sets[s][:n_v210]])
                mids = (C.c_void_p * n_v210)(*[ptr(t).value for t in rgba[:n_v210]])
                imgs = (C.c_void_p * n)(*([ptr(t).value for t in rgba[:n_v210]] + ([ptr(routed[s]).value] if has_image else [])))
                jobs = [call(lib.ph_v210_read_batch, hnd, q, n_v210, ins, mids, w, h, ptr(rd[0]), ptr(rd[1]), ptr(rd[2])),
                        call(lib.ph_combine, hnd, q, n, imgs, w, h, ptr(image_chain))]
                if outs == ["v210"]:
                    jobs.append(call(lib.ph_v210_write, hnd, q, ptr(image_chain), ptr(dst[0][0]), w, h, 0, ptr(wr_cm["v210"]), ptr(wr_lut)))
                elif outs:
                    jobs.append(ctx.pack_write_multi(image_chain, outputs, w, h, prepare_only=True))
                chain.append(jobs)
            base = "chan_compose_multi" if not wants_image else "v210_read_batch + combine" + (" + v210_write" if outs == ["v210"] else " + pack_write_multi" if outs else "")
            sides = {"new": [[j] for j in new], "chain": chain}
            routes = {}
            for k, side in sides.items():
                with capi.trace(dry_run=True) as t:
                    for job in side[0]:
                        job()
                routes[k] = t.route

            def timed(side):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(reps):
                    for job in side[i % ring]:
                        job()
                e1.record(stream)
                ctx.wait()
                return 1e3 * e0.elapsed_time(e1) / reps
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:  # until every side is warm and the clocks have settled
                for side in sides.values():
                    for jobs in side:
                        for job in jobs:
                            job()
                ctx.wait()
            us = {k: [] for k in sides}
            for _ in range(rounds):  # the sides alternate inside a round
                for k, side in sides.items():
                    us[k].append(timed(side))
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = {k: max(v) - min(v) for k, v in us.items()}
            saved = med["chain"] - med["new"]
            line = {"bench": "fused_route", "shape": name, "width": w, "height": h, "v210_layers": n_v210, "image_layer": has_image, "image_out": wants_image, "frame_sets": ring,
                    "outputs": outs, "reps": reps, "rounds": rounds, "routes": routes, "new_us": round(med["new"], 2), "new_spread_us": round(spread["new"], 2), "chain": base,
                    "chain_us": round(med["chain"], 2), "chain_spread_us": round(spread["chain"], 2), "saved_us": round(saved, 2),
                    "verdict": "wins" if saved > spread["chain"] else "loses" if -saved > spread["chain"] else "within the spread",
                    "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del dst, sides, new, chain
        del sets, routed, rgba, image_new, image_chain
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
