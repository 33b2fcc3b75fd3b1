"""The `imageWriters` option through the node layer on the GPU (node/test/image_writers_run.js): a recording context with the option and the
plain context post the same job stream - a routed image consumed by v210 (both field modes), p010 and rgba8 writers - and every consumer
sees the same bytes; the option off, a sibling posted late and a refused launch give today's launches; a 1280 x 720 channel."""
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
def test_consumers_of_one_image_share_a_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "image_writers_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["v210 fields + p010 + rgba8", "imageWriters off", "a sibling posted late", "a refused launch falls back", "1280 x 720"]
    assert all(s["frames"] > 0 for s in res["scenarios"])
