"""Several channels' file playback through the node addon on the GPU (node/test/clip_batch_run.js): four channels post program
clip_compose_multi_1 (nv12 + rgba8) per tick for three ticks on a recording context.  With `clipBatch: true` a tick is one launch,
clip_up_multi<rgb>x2j4; with the option off it is four launches; both ways every consumer sees chan_compose_multi_1's bytes."""
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
def test_four_channels_clips_of_a_tick_share_a_launch():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "clip_batch_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    on, off = res["scenarios"]
    assert on["routes"] == ["clip_up_multi<rgb>x2j4"] * 3, on["routes"]
    assert off["routes"] == ["+".join(["clip_up_multi<rgb>x2"] * 4)] * 3, off["routes"]
    assert on["deferred"]["batched"] == 12, on["deferred"]
