"""A routed channel's file playback through the node addon on the GPU (node/test/clip_route_run.js): program clip_compose_route_1, posted
by name on a recording context (with and without clipBatch) and on a plain context, makes every tick's nv12 and rgba8 frames and the
combined f32 RGBA image in one launch of the route clip kernel; the bytes are those of the posted chain - read, transform, a write per
consumer.  The image alone is posted too."""
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
def test_a_routed_clip_by_name():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "clip_route_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["a recording context", "a recording context, clipBatch: true", "a plain context", "a plain context, the image alone"]
    for s in res["scenarios"][:3]:
        assert s["routes"] == ["clip_up_route<rgb>x2"] * 3, s
    assert res["scenarios"][3]["routes"] == ["clip_up_route<rgb>x0"] * 3, res["scenarios"][3]
