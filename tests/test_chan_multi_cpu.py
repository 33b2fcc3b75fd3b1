"""CPU-side checks of ph_chan_compose_multi's surface: the symbol, the struct's layout as the header's compiler sees it, the by-name
program's resolution, the ABI number (the call is additive within 8)."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_the_symbol_is_exported_and_bound():
    assert "ph_chan_compose_multi" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(build.build()), "ph_chan_compose_multi")
    fn = capi.lib().ph_chan_compose_multi
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[5] == ctypes.POINTER(capi.PhChanOutput)
    assert callable(capi.Context.chan_compose_multi)


def test_the_struct_is_the_headers(tmp_path):
    """sizeof and every offset of ph_chan_output, from a program compiled against include/phaneron_hip.h"""
    fields = ["format", "planes", "interlace", "wr_col_matrix12", "wr_gamma_lut"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "phaneron_hip.h"\nint main() {\n  printf("%zu", sizeof(ph_chan_output));\n' +
                   "".join('  printf(" %%zu", offsetof(ph_chan_output, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(capi.PhChanOutput)
    assert got[1:] == [getattr(capi.PhChanOutput, f).offset for f in fields]
    assert [n for n, _ in capi.PhChanOutput._fields_] == fields


def test_the_program_resolves_for_every_layer_count():
    for n in range(1, 9):
        name = "chan_compose_multi_%d" % n
        assert capi.resolve_program("phaneron:chan", name) == (name, None, "tag")
        assert capi.resolve_program("", name) == (name, None, "name")
    for name, needle in (("chan_compose_multi_", "plain layer count"), ("chan_compose_multi_9", "layers are built"), ("chan_compose_multi_0", "layers are built"),
                         ("chan_compose_multi_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_folds_sibling_writes():
    """node/defer.js against a counting stand-in for the addon (node/test/multi_defer_check.js): the writes of several consumers on one
    combined image are one chan_compose_multi_<n> launch; the option off, a late sibling and a refused launch give a launch per write"""
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "node", "test", "multi_defer_check.js")], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 30
