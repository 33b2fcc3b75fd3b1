"""File playback through a MIX through the node addon on the GPU (node/test/clip_trans_run.js): program clip_compose_trans_1, posted by
name on a recording context (with and without clipBatch) and on a plain context, makes every tick of a dissolve between two yuv420p clips
for nv12 + rgba8 in one launch of the transition clip kernel; the bytes are the library's channel kernel's on the same arguments."""
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
def test_a_dissolve_between_two_clips_by_name():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "clip_trans_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["a recording context", "a recording context, clipBatch: true", "a plain context"]
    for s in res["scenarios"]:
        assert s["routes"] == ["clip_up_trans<rgb>x2"] * 3, s
