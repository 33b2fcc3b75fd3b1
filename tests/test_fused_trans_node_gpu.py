"""The `fusedTransitions` option through the node layer on the GPU (node/test/fused_trans_run.js): recorded streams of a headline-shaped
frame whose top layer dissolves, wipes by an f32 mask image and wipes by a v210 mask frame, for SDI's v210 write alone and with the
screen's bgra8 write beside it.  With the option off the launches are today's (the channel kernel's); with it on a tick is one
fused_v210_trans_multi launch; either way the frames equal the launch-as-posted context's byte for byte."""
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
def test_a_transition_between_plain_layers_takes_the_headline_kernels_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "fused_trans_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["v210 alone", "v210 + bgra8"]
    assert [s["frames"] for s in res["scenarios"]] == [3, 6]
    assert [s["on"] for s in res["scenarios"]] == [["fused_v210_trans_multi x1"] * 3, ["fused_v210_trans_multi x2"] * 3]
    assert all(route.startswith("chan_compose_") for s in res["scenarios"] for route in s["off"])
