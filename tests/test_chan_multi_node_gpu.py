"""Several consumers on one channel through the node layer on the GPU (node/test/multi_out_run.js): the recording context makes the
writes of a tick with one launch of the channel kernel, the plain context with a launch per operator - every consumer sees the same
bytes; the option off, a sibling posted late and a refused launch give today's launches."""
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
def test_consumers_of_one_channel_share_a_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "multi_out_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["v210 + bgra8", "v210 + yuv422p8 + rgba8", "v210 field + rgba8 frame", "multiWriter: false", "a sibling posted late",
                                                     "a refused multi launch falls back"]
    assert all(s["frames"] > 0 for s in res["scenarios"])
