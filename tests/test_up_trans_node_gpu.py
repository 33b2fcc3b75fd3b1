"""A 1080i-source channel in a transition through the node layer on the GPU (node/test/up_trans_run.js): a recorded stream with a layer
that dissolves, then wipes, to another source.  With `upTransitions: true` the recording context makes the frames with
compose_up_trans_<n> - the dissolve from the packed fields, no channel kernel; with the option off, and by default, it launches what it
launches without the route.  Every frame is the same bytes on the plain context, the recording one, and whatever the option says."""
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
def test_a_transition_on_a_field_channel_takes_the_compositors_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "up_trans_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["upTransitions: true", "upTransitions: false", "the default"]
    assert all(s["frames"] == 6 for s in res["scenarios"])
    on = res["scenarios"][0]
    assert "compose_up_trans_2" in on["programs"] and not on["deferred"].get("unpacked")
