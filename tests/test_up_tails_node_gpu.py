"""A 1280 x 10 channel of two enlarged packed fields with SDI + the screen through the node layer on the GPU (node/test/up_tails_run.js):
the plain context, the recording context and the recording context with `upTails: true` give every consumer the same bytes, and with
`upTails` a tick is one kernel fewer - the v210 frames come out of the several-outputs launch."""
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
def test_sdi_and_screen_of_a_720p_wide_channel_share_a_launch_with_up_tails():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "up_tails_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["a plain context", "a recording context", "a recording context, upTails: true"]
    assert all(s["frames"] == 4 for s in res["scenarios"])
    assert len(res["scenarios"][2]["kernels"]) == len(res["scenarios"][1]["kernels"]) - 1
