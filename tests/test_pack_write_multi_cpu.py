"""CPU-side checks of ph_pack_write_multi's surface: the symbol and its binding, the by-name program's resolution, the ABI number (the
call is additive within 8), and the recording context's `imageWriters` option against a counting stand-in for the addon."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi


def test_the_symbol_is_exported_and_bound():
    assert "ph_pack_write_multi" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(build.build()), "ph_pack_write_multi")
    fn = capi.lib().ph_pack_write_multi
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, vp, ci, ctypes.POINTER(capi.PhChanOutput), cu, cu]
    assert callable(capi.Context.pack_write_multi)
    assert ctypes.sizeof(capi.PhChanOutput) == 56  # (ph_chan_output is as it was)


def test_the_program_resolves_for_one_to_four_outputs():
    for n in range(1, 5):
        name = "pack_write_multi_%d" % n
        assert capi.resolve_program("phaneron:pack", name) == (name, None, "tag")
        assert capi.resolve_program("", name) == (name, None, "name")
    for name, needle in (("pack_write_multi_0", "1..4 outputs are built"), ("pack_write_multi_5", "1..4 outputs are built"),
                         ("pack_write_multi_2x", "plain output count"), ("pack_write_multi_", "plain output count")):
        with pytest.raises(capi.PhaneronError, match=needle) as e:
            capi.resolve_program("", name)
        assert "error -4:" in str(e.value)  # PH_E_UNKNOWN_KERNEL, as its siblings
    # the siblings' words are as they were
    with pytest.raises(capi.PhaneronError, match="1..8 layers are built"):
        capi.resolve_program("", "chan_compose_multi_9")
    with pytest.raises(capi.PhaneronError, match="plain layer count"):
        capi.resolve_program("", "compose_up_multi_2x")


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_folds_the_writes_of_one_image():
    """node/defer.js against a counting stand-in for the addon (node/test/image_writers_check.js): three writes (v210 + p010 + rgba8) of an
    already-made image fold into one pack_write_multi_3; the option off gives three `write` launches; a late sibling and a refused launch
    fall back; two writes into one buffer never share a launch"""
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    r = subprocess.run([shutil.which("node"), os.path.join(root, "node", "test", "image_writers_check.js")], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 30
