"""CPU-side checks of ph_chan_compose_batch_out's surface: the symbol and its binding, the job struct's layout as the header's compiler
sees it, the ABI number (the call is additive within 8), the context option's name in the header, and the answer without a device."""
import ctypes
import os
import subprocess

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_the_symbol_is_exported_and_bound():
    assert "ph_chan_compose_batch_out" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(build.build()), "ph_chan_compose_batch_out")
    fn = capi.lib().ph_chan_compose_batch_out
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[3] == ctypes.POINTER(capi.PhChanJobOut)
    assert callable(capi.Context.chan_compose_batch_out)


def test_the_struct_is_the_headers(tmp_path):
    """sizeof and every offset of ph_chan_job_out, from a program compiled against include/phaneron_hip.h"""
    fields = ["n", "layers", "n_out", "outs"]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "phaneron_hip.h"\nint main() {\n  printf("%zu", sizeof(ph_chan_job_out));\n' +
                   "".join('  printf(" %%zu", offsetof(ph_chan_job_out, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(capi.PhChanJobOut)
    assert got[1:] == [getattr(capi.PhChanJobOut, f).offset for f in fields]
    assert [n for n, _ in capi.PhChanJobOut._fields_] == fields
    assert capi.PhChanJobOut.outs.size == ctypes.sizeof(ctypes.c_void_p) and capi.PhChanJobOut._fields_[3][1] == ctypes.POINTER(capi.PhChanOutput)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    assert "#define PH_ABI_VERSION 8" in header and "ph_chan_compose_batch_out (ph_chan_job_out)" in header.split("#define PH_ABI_VERSION")[0]


def test_without_a_device_the_call_says_so():
    """no context can exist without a device (ph_ctx_create: PH_E_NO_DEVICE), and the call gives the same answer for the context that is
    not there; with a device a NULL context is an argument fault like any other"""
    import torch
    jobs = (capi.PhChanJobOut * 1)()
    rc = capi.lib().ph_chan_compose_batch_out(None, capi.QUEUE_PROCESS, 1, jobs, 384, 8, None, None, None)
    assert rc == (-1 if torch.cuda.is_available() else -2), rc
    text = capi.lib().ph_last_error(None).decode()
    assert ("NULL argument" if torch.cuda.is_available() else "no HIP device") in text, text
