"""The `fusedWriters` option through the node layer on the GPU (node/test/fused_writers_run.js): recorded streams of a headline-shaped frame
with a yuv422p8 write, and with v210 + bgra8 sibling writes.  With the option off the launches are the parent's (the channel kernel's);
with it on a tick is one fused_v210_combine_multi launch; either way the frames equal the launch-as-posted context's byte for byte."""
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
def test_headline_shaped_frames_for_other_consumers():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "fused_writers_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["yuv422p8 alone", "v210 + bgra8"]
    assert all(s["frames"] > 0 for s in res["scenarios"])
    assert all(route.startswith("fused_v210_combine_multi x") for s in res["scenarios"] for route in s["on"])
