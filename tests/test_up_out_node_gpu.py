"""Consumers of a 1080i-source channel through the node layer on the GPU (node/test/up_out_run.js): the recording context makes a tick's
frames for a consumer that is not SDI, and for several consumers, with one launch of the 2 x 2-block compositor's several-outputs form
from the packed fields, the plain context with a launch per operator - every consumer sees the same bytes; the option off, the
default, a sibling posted late and a refused launch likewise."""
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
def test_consumers_of_a_field_channel_share_the_compositors_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "up_out_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["yuv422p8 alone", "v210 + bgra8", "v210 + yuv420p + rgba8", "upWriters: false", "the default", "a sibling posted late",
                                                     "a refused launch falls back"]
    assert all(s["frames"] > 0 for s in res["scenarios"])
