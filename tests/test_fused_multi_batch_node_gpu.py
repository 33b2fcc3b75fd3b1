"""The `fusedBatch` option through the node layer on the GPU (node/test/fused_batch_run.js): four channels per tick, each a headline-shaped
frame for SDI (v210) and the screen (bgra8).  With `fusedWriters` and `fusedBatch` a tick's trace is exactly one
"fused_v210_combine_multi x2j4" launch; without `fusedBatch` it is four "fused_v210_combine_multi x2" launches; either way every consumer
sees the launch-as-posted context's bytes."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_four_channels_frames_share_a_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "fused_batch_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    on, off = res["scenarios"]
    assert (on["name"], off["name"]) == ("fusedBatch: true", "fusedBatch off (the default)")
    assert on["planes"] == off["planes"] == 16  # 2 ticks x 4 channels x (v210 + bgra8)
    assert on["routes"] == ["fused_v210_combine_multi x2j4"] * 2, on["routes"]
    assert off["routes"] == ["+".join(["fused_v210_combine_multi x2"] * 4)] * 2, off["routes"]
    assert on["deferred"]["batched"] == 8 and not off["deferred"].get("batched")
