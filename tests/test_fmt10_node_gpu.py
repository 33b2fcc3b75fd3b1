"""The 10-bit 4:2:0 decoder frames through the node layer on the GPU (node/test/fmt10_run.js): Readers made by tag, recorded job streams
against launch-as-posted ones (same bytes, as many launches as for yuv420p / nv12), and the write job and Yadif window that fall back
to separate launches."""
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
def test_recorded_job_streams_of_10bit_420_frames():
    from phaneron_amd import build as hipbuild
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(ROOT, "node", "build.py")], check=True)
    r = subprocess.run([NODE, os.path.join(ROOT, "node", "test", "fmt10_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert len(res["scenarios"]) == 12
