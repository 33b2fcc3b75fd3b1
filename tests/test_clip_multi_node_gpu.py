"""File playback for several consumers through the node addon on the GPU (node/test/clip_multi_run.js): program clip_compose_multi_1,
made and run by name, sends a yuv420p clip to nv12 + rgba8 in one launch of the clip kernel; the bytes are chan_compose_multi_1's on the
same buffers."""
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
def test_a_clip_for_two_consumers_by_name():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "clip_multi_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert res["route"] == "clip_up_multi<rgb>x2", res["route"]
    assert res["baseline"].startswith("chan_compose_multi<") and res["bytes"] > 0
