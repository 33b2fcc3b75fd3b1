"""CPU-side checks of ph_fused_v210_combine_multi_batch's surface: the symbol and its binding, the ABI number (the call is additive
within 8), the NULL-context answers, the option's and the entry point's place in the header, and - device-free - the recording
context's `fusedBatch` option."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_the_symbol_is_exported_and_bound():
    assert "ph_fused_v210_combine_multi_batch" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(build.build()), "ph_fused_v210_combine_multi_batch")
    fn = capi.lib().ph_fused_v210_combine_multi_batch
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, ci, ctypes.POINTER(vp), ci, ctypes.POINTER(capi.PhChanOutput), cu, cu, vp, vp, vp]
    assert callable(capi.Context.fused_v210_combine_multi_batch)
    assert ctypes.sizeof(capi.PhChanOutput) == 56  # (ph_chan_output is as it was)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


def test_null_context_answers():
    l = capi.lib()
    layers = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    outs = (capi.PhChanOutput * 2)()
    one = ctypes.c_void_p(0x1000)
    assert l.ph_fused_v210_combine_multi_batch(None, 1, 2, 1, layers, 1, outs, 48, 2, one, one, one) == -1
    assert "NULL" in l.ph_last_error(None).decode(), l.ph_last_error(None)
    assert l.ph_ctx_set_option(None, b"fused_multi_batch", 1) == -1
    assert "NULL" in l.ph_last_error(None).decode(), l.ph_last_error(None)


def test_the_option_and_the_entry_point_stand_in_the_header():
    text = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    assert '"fused_multi_batch"' in text
    assert "int ph_fused_v210_combine_multi_batch(ph_ctx *ctx, int queue, int jobs, int n, const void *const *layers" in text
    assert "#define PH_ABI_VERSION 8" in text


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_puts_four_channels_frames_into_one_call():
    """node/defer.js against a counting stand-in for the addon (node/test/fused_batch_check.js): with `fusedBatch` four channels'
    headline-shaped frames of a tick are one runPrograms call of four fused_v210_combine_multi_<n> jobs; with it off, four calls; a
    refused batch falls back plan by plan"""
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "node", "test", "fused_batch_check.js")], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 12
