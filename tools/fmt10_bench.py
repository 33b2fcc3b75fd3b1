"""Timings of the 10-bit 4:2:0 decoder formats (yuv420p10le, p010le) beside the formats they are measured against, in one process:
the standalone reader and writer at 3840 x 2160 (against yuv422p10, yuv420p, nv12) and a channel frame of one clip (f1: a 1080p clip
under the Mixer's default fill; f2: a 720p clip filling 1080p) in each 4:2:0 format.  HIP events around `reps` launches over a ring of
frames; the formats take turns round by round, so a clock or thermal drift spreads over all of them.  Prints one JSON line per case
(median of the rounds, and the spread), and with --out writes them to that file (profiles/fmt10_bench.jsonl is such a record).

    python tools/fmt10_bench.py [--rounds 7] [--reps 50] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from phaneron_amd import capi  # noqa: E402

RING = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    args = ap.parse_args()
    ctx = capi.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(1)
    luts = {}

    def lut(kind, spec):
        if (kind, spec) not in luts:
            host = capi.gamma2linear_lut(spec) if kind == "r" else capi.linear2gamma_lut(spec)
            luts[(kind, spec)] = dev(host)
            torch.cuda.synchronize()
            ctx.register_lut(luts[(kind, spec)], host)
        return luts[(kind, spec)]

    def rd(fmt):
        return (dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE[fmt])), lut("r", "709"),
                dev(np.concatenate([capi.rgb2rgb_matrix("709", "2020"), np.zeros(3, np.float32)])))

    def wr(fmt):
        return dev(capi.rgb2ycbcr_matrix("2020", *capi.FORMAT_RANGE[fmt])), lut("w", "2020")

    def planes(fmt, w, h):
        return [torch.from_numpy(rng.integers(0, 1 << 16, n // 2, dtype=np.uint16).view(np.uint8)).cuda() for n in capi.pack_plane_bytes(fmt, w, h)]

    stream = ctx.torch_stream()
    cases = {}
    W, H = 3840, 2160
    img = [torch.rand(W * H * 4, device="cuda") for _ in range(RING)]
    for fmt in ("yuv422p10", "yuv420p", "nv12", "yuv420p10", "p010"):
        src = [planes(fmt, W, H) for _ in range(RING)]
        dst = [planes(fmt, W, H) for _ in range(RING)]
        r, w_ = rd(fmt), wr(fmt)
        nbytes = sum(capi.pack_plane_bytes(fmt, W, H))
        cases["read 2160p " + fmt] = (lambda i, fmt=fmt, src=src, r=r: ctx.pack_read(fmt, src[i % RING], img[i % RING], W, H, *r), nbytes + W * H * 16)
        cases["write 2160p " + fmt] = (lambda i, fmt=fmt, dst=dst, w_=w_: ctx.pack_write(fmt, img[i % RING], dst[i % RING], W, H, 0, *w_), nbytes + W * H * 16)
    ow, oh = 1920, 1080
    out = [torch.zeros(capi.v210_pitch_bytes(ow) * oh // 4, dtype=torch.int32, device="cuda") for _ in range(RING)]
    crd, cwr = rd("v210"), wr("v210")
    fill = capi.transform_matrix(ow, oh)
    for shape, (sw, sh) in (("f1", (1920, 1080)), ("f2", (1280, 720))):
        for fmt in ("yuv420p", "yuv420p10", "nv12", "p010"):
            own = None if fmt in ("yuv420p10", "p010") else dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE[fmt]))
            src = [planes(fmt, sw, sh) for _ in range(RING)]
            layers = [[dict(src=(tuple(p), sw, sh, fill, fmt, own))] for p in src]
            with capi.trace(dry_run=True) as t:
                ctx.chan_compose_v210(layers[0], out[0], ow, oh, 0, *crd, *cwr)
            cases["%s %s" % (shape, fmt)] = (lambda i, layers=layers: ctx.chan_compose_v210(layers[i % RING], out[i % RING], ow, oh, 0, *crd, *cwr), t.route)
    torch.cuda.synchronize()

    def timed(fn):
        for i in range(3):
            fn(i)
        ctx.wait()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(args.reps):
            fn(i)
        e1.record(stream)
        ctx.wait()
        return 1e3 * e0.elapsed_time(e1) / args.reps

    samples = {k: [] for k in cases}
    for _ in range(args.rounds):
        for name, (fn, _) in cases.items():
            samples[name].append(timed(fn))
    lines = []
    for name, (_, extra) in cases.items():
        s = sorted(samples[name])
        rec = {"case": name, "us": round(s[len(s) // 2], 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2), "rounds": args.rounds, "reps": args.reps}
        if isinstance(extra, int):
            rec["bytes"], rec["GBps"] = extra, round(extra / s[len(s) // 2] / 1e3, 1)
        else:
            rec["route"] = extra
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    med = {json.loads(l)["case"]: json.loads(l)["us"] for l in lines}
    for shape in ("f1", "f2"):
        for ten, eight in (("yuv420p10", "yuv420p"), ("p010", "nv12")):
            lines.append(json.dumps({"case": "%s %s / %s" % (shape, ten, eight), "ratio": round(med["%s %s" % (shape, ten)] / med["%s %s" % (shape, eight)], 3)}))
            print(lines[-1])
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
