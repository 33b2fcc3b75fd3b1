"""CPU-side checks of ph_fused_v210_combine_multi's surface: the symbol and its binding, the by-name program's resolution in front of
fused_v210_combine_<n>'s prefix, the ABI number (the call is additive within 8), the NULL-context answers and the option's name."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_the_symbol_is_exported_and_bound():
    assert "ph_fused_v210_combine_multi" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(build.build()), "ph_fused_v210_combine_multi")
    fn = capi.lib().ph_fused_v210_combine_multi
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, ctypes.POINTER(vp), ci, ctypes.POINTER(capi.PhChanOutput), cu, cu, vp, vp, vp]
    assert callable(capi.Context.fused_v210_combine_multi)
    assert ctypes.sizeof(capi.PhChanOutput) == 56  # (ph_chan_output is as it was)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


def test_the_program_resolves_in_front_of_the_headline_prefix():
    assert capi.resolve_program("phaneron:fused", "fused_v210_combine_multi_3") == ("fused_v210_combine_multi_3", None, "tag")
    for n in range(1, 9):
        name = "fused_v210_combine_multi_%d" % n
        assert capi.resolve_program("", name) == (name, None, "name")
    # the headline program resolves as before
    assert capi.resolve_program("", "fused_v210_combine_4") == ("fused_v210_combine_4", None, "name")
    assert capi.resolve_program("phaneron:fused", "fused_v210_combine_8") == ("fused_v210_combine_8", None, "tag")
    for name, needle in (("fused_v210_combine_multi_0", "1..8 layers are built"), ("fused_v210_combine_multi_9", "1..8 layers are built"),
                         ("fused_v210_combine_multi_2x", "plain layer count"), ("fused_v210_combine_multi_", "plain layer count"),
                         ("fused_v210_combine_9", "1..8 layers are built"), ("fused_v210_combine_x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle) as e:
            capi.resolve_program("", name)
        assert "error -4:" in str(e.value)  # PH_E_UNKNOWN_KERNEL, as its siblings


def test_null_context_answers():
    l = capi.lib()
    layers = (ctypes.c_void_p * 1)(0x1000)
    outs = (capi.PhChanOutput * 1)()
    one = ctypes.c_void_p(0x1000)
    assert l.ph_fused_v210_combine_multi(None, 1, 1, layers, 1, outs, 48, 2, one, one, one) == -1
    assert "NULL" in l.ph_last_error(None).decode(), l.ph_last_error(None)
    assert l.ph_ctx_set_option(None, b"fused_multi_wgs", 1) == -1
    assert "NULL" in l.ph_last_error(None).decode(), l.ph_last_error(None)


def test_the_option_is_named_in_the_header():
    text = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    assert '"fused_multi_wgs"' in text and "ph_fused_v210_combine_multi" in text


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_takes_headline_shaped_frames_to_the_new_program():
    """node/defer.js against a counting stand-in for the addon (node/test/fused_writers_check.js): with `fusedWriters` a headline-shaped
    frame for a consumer that is not a v210 frame, or for several consumers, is one fused_v210_combine_multi_<n> job; one v210 frame stays
    the headline kernel's; the option off gives the channel kernel's launches; a refused launch falls back"""
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "node", "test", "fused_writers_check.js")], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 10
