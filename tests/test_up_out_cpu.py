"""CPU-side checks of ph_compose_up_write_multi's surface: the symbol and its binding, the by-name program's resolution, the ABI number
(the call is additive within 8)."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi


def test_the_symbol_is_exported_and_bound():
    assert "ph_compose_up_write_multi" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(build.build()), "ph_compose_up_write_multi")
    fn = capi.lib().ph_compose_up_write_multi
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, ci, ctypes.POINTER(ctypes.POINTER(capi.PhImageLayer)), ci, ctypes.POINTER(capi.PhChanOutput), cu, cu]
    assert callable(capi.Context.compose_up_write_multi)


def test_the_program_resolves_for_every_layer_count():
    for n in range(1, 9):
        name = "compose_up_multi_%d" % n
        assert capi.resolve_program("phaneron:up", name) == (name, None, "tag")
        assert capi.resolve_program("", name) == (name, None, "name")
    for name, needle in (("compose_up_multi_", "plain layer count"), ("compose_up_multi_9", "layers are built"), ("compose_up_multi_0", "layers are built"),
                         ("compose_up_multi_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)
    assert capi.resolve_program("", "compose_up_write_v210_4") == ("compose_up_write_v210_4", None, "name")


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_plans_with_the_compositors_several_outputs_form():
    """node/defer.js against a counting stand-in for the addon (node/test/up_out_defer_check.js): a yuv422p8 write of de-interlaced fields
    is one compose_up_multi_1 launch told packedRgb; v210 + bgra8 siblings of both fields fold into one; the option off, a late sibling
    and a refused launch give today's launches; a field unpacked between plan and commit makes the frame be planned again"""
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    r = subprocess.run([shutil.which("node"), os.path.join(root, "node", "test", "up_out_defer_check.js")], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 30
