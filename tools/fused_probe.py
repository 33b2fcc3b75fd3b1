#!/usr/bin/env python3
"""Where the headline kernel's time goes, measured inside the real kernel: builds lib/libphaneron_hip_probe.so
(-DPH_PROBE=1: wave 0 of every workgroup stamps s_memtime / s_memrealtime at the phase boundaries), runs the
bench workload once per variant and prints the sustained shader clock and the per-phase share.
It also stamps the kernel's entry and the far side of the barrier that ends the tile: `head_us` is kernel entry -> first
table DMA issued, `tail_wait_us` is what wave 0 waits for the slowest wave before it may end (profiles/launch_head_*.jsonl).
usage: python tools/fused_probe.py [--out FILE] [--label NAME]   (on the GPU box; PH_FUSED_PIPE=0|1 selects the variant;
       --build / --build-only (re)build the probe library, PH_PROBE_LIB=PATH runs an already built one)"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from phaneron_amd import build  # noqa: E402

# PH_PROBE_ABLATE=1|8: also build in the timing experiments of ph_ldslut.h (1 = no LDS reads, 8 = conflict-free reads;
# WRONG results, timing only) to see what the VALU stream costs on its own
ablate = os.environ.get("PH_PROBE_ABLATE", "")
variant = "probe" + ablate
lib_path = os.environ.get("PH_PROBE_LIB") or build.variant_path(variant)
if not os.path.exists(lib_path) or "--build" in sys.argv:
    build.build(variant=variant, extra_flags=["-DPH_PROBE=1"] + (["-DPH_ABLATE=" + ablate] if ablate else []))
if "--build-only" in sys.argv:
    sys.exit(0)
os.environ["PHANERON_HIP_LIB"] = lib_path
import numpy as np  # noqa: E402
import torch  # noqa: E402
from phaneron_amd import capi  # noqa: E402


def opt(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv[:-1] else None


out_path, label = opt("--out"), opt("--label")  # --out FILE appends the result line to FILE, --label NAME tags it
sys.argv = [sys.argv[0]]
import bench  # noqa: E402

w, h, n = 3840, 2160, 4
ctx = capi.Context(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")),
      dev(np.concatenate([capi.rgb2rgb_matrix("709", "2020"), np.zeros(3, np.float32)]))]
wr = [dev(capi.rgb2ycbcr_matrix("2020")), dev(capi.linear2gamma_lut("2020"))]
torch.cuda.synchronize()
ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
ctx.register_lut(wr[1], capi.linear2gamma_lut("2020"))
ring = [[bench.synth_v210(torch, w, h, 0x5EED0000 + 16 * r + l, torch.device("cuda", 0)) for l in range(n)] for r in range(8)]
out = torch.empty(capi.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
heads = []                                  # the launch head and tail of several launches, each read out on its own
for rep in range(5):
    for i in range(400 if rep == 0 else 50):
        ctx.fused_v210_combine(ring[i % 8], out, w, h, *rd, *wr)
    ctx.wait()
    probe = np.zeros(256 * 16, np.uint64)
    rc = capi.lib().__getattr__("ph_debug_fused_probe")(probe.ctypes.data_as(C.c_void_p), probe.size)
    assert rc == 0, rc
    s = probe.reshape(256, 8, 2).astype(np.float64)  # stamps 0..4 phase boundaries, 5 kernel entry, 6 behind the last barrier
    heads.append({"head_cycles_median": int(np.median(s[:, 0, 0] - s[:, 5, 0])),
                  "head_us_median": round(float(np.median(s[:, 0, 1] - s[:, 5, 1])) / 100.0, 3),
                  "head_us_max": round(float((s[:, 0, 1] - s[:, 5, 1]).max()) / 100.0, 3),
                  "entry_skew_us": round(float(s[:, 5, 1].max() - s[:, 5, 1].min()) / 100.0, 2),
                  "tail_wait_cycles_median": int(np.median(s[:, 6, 0] - s[:, 4, 0])),
                  "tail_wait_us_median": round(float(np.median(s[:, 6, 1] - s[:, 4, 1])) / 100.0, 3),
                  "entry_to_end_us_median": round(float(np.median(s[:, 6, 1] - s[:, 5, 1])) / 100.0, 2),
                  "first_entry_to_last_end_us": round(float(s[:, 6, 1].max() - s[:, 5, 1].min()) / 100.0, 2)})
p = s[:, :5]
cyc = p[:, 1:, 0] - p[:, :-1, 0]           # per workgroup: table load, phase 1, table swap, phase 2 (shader cycles)
real = p[:, -1, 1] - p[:, 0, 1]            # 100 MHz ticks
total = p[:, -1, 0] - p[:, 0, 0]
ghz = total / real * 0.1
names = ["reader table -> LDS", "phase 1 (unpack, CSC, LUT, gamut, combine)", "barrier + writer table -> LDS", "phase 2 (LUT, CSC, pack, store)"]
res = {"pipe": os.environ.get("PH_FUSED_PIPE", "0"), "ablate": ablate or "0", "workgroups": 256, "shader_ghz_median": round(float(np.median(ghz)), 3),
       "tile_cycles_median": int(np.median(total)), "tile_us_median": round(float(np.median(real)) / 100.0, 2),
       "phases": {nm: {"cycles_median": int(np.median(cyc[:, i])), "share": round(float(np.median(cyc[:, i]) / np.median(total)), 3)}
                  for i, nm in enumerate(names)},
       "start_skew_us": round(float(p[:, 0, 1].max() - p[:, 0, 1].min()) / 100.0, 2),
       "end_skew_us": round(float(p[:, -1, 1].max() - p[:, -1, 1].min()) / 100.0, 2),
       # kernel entry -> first table DMA issued (the scalar head), wave 0's wait at the last barrier, and the whole launch
       # as the stamps see it; per-workgroup medians of five launches, and the median of those
       "launch_head": heads,
       "head_us": round(float(np.median([x["head_us_median"] for x in heads])), 3),
       "tail_wait_us": round(float(np.median([x["tail_wait_us_median"] for x in heads])), 3)}
if label:
    res = dict(label=label, **res)
print(json.dumps(res))
if out_path:
    with open(out_path, "a") as f:
        f.write(json.dumps(res) + "\n")
ctx.close()
