"""CPU-side checks of ph_fused_v210_route_multi's surface: ph_route_layer as the header and the binding lay it out, the symbol, the
by-name program's resolution, the ABI number (the call is additive within 8), and every refusal - the entry point looks at its context
last, so these are answered without a device and before anything could be launched."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIELDS = ["data", "format"]
FN = "ph_fused_v210_route_multi"


def test_the_struct_is_laid_out_as_the_header_says(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "phaneron_hip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(ph_route_layer));']
    lines += ['  printf("%%zu\\n", offsetof(ph_route_layer, %s));' % f for f in FIELDS]
    lines += ['  printf("%d %d\\n", PH_SRC_V210, PH_SRC_RGBA_F32);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    T = capi.PhRouteLayer
    want = [C.sizeof(T)] + [getattr(T, f).offset for f in FIELDS]
    assert [int(x) for x in got[:len(want)]] == want
    assert [f for f, _ in T._fields_] == FIELDS
    assert got[len(want)].split() == [str(x) for x in (capi.SRC_V210, capi.SRC_RGBA_F32)]
    assert C.sizeof(capi.PhChanOutput) == 56  # (the struct beside it is as it was)


def test_the_symbol_is_exported_and_bound():
    assert FN in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), FN)
    fn = getattr(capi.lib(), FN)
    ci, cu, vp = C.c_int, C.c_uint32, C.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, C.POINTER(capi.PhRouteLayer), vp, ci, C.POINTER(capi.PhChanOutput), cu, cu, vp, vp, vp]
    assert callable(capi.Context.fused_v210_route_multi)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


def test_the_program_resolves_for_every_layer_count():
    assert capi.resolve_program("", "fused_v210_route_3") == ("fused_v210_route_3", None, "name")
    for n in range(1, 9):
        name = "fused_v210_route_%d" % n
        assert capi.resolve_program("phaneron:fused", name) == (name, None, "tag")
        for sibling in ("fused_v210_combine_multi_%d" % n, "fused_v210_trans_%d" % n):
            assert capi.resolve_program("phaneron:fused", sibling) == (sibling, None, "tag")  # the siblings are as they were
    for name, needle in (("fused_v210_route_", "plain layer count"), ("fused_v210_route_9", "layers are built"), ("fused_v210_route_0", "layers are built"),
                         ("fused_v210_route_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)


# ---- refusals: no context, device pointers that are never followed ---------------------------------------------------------------
W, H = 384, 6
FAKE = 0x10000  # a device address that nothing reads
IMAGE_OUT = FAKE * 400


def good_layers():
    """three v210 frames under a routed image"""
    arr = (capi.PhRouteLayer * 9)()
    for i in range(4):
        arr[i].data, arr[i].format = FAKE * (1 + i), capi.SRC_RGBA_F32 if i == 3 else capi.SRC_V210
    return arr


def good_outputs(fmts=("v210", "rgba8")):
    outs = (capi.PhChanOutput * max(len(fmts), 5))()
    for k, f in enumerate(fmts):
        o = outs[k]
        o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
        for p in range(3):
            o.planes[p] = FAKE * (200 + 4 * k + p)
    return outs


def answer(layers, outs, n=4, n_out=2, w=W, h=H, rd=(FAKE * 300, FAKE * 301, FAKE * 302), queue=None, image_out=IMAGE_OUT):
    rc = getattr(capi.lib(), FN)(None, capi.QUEUE_PROCESS if queue is None else queue, n, layers, image_out, n_out, outs, w, h, *rd)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    for kw in ({}, {"h": 0}, {"image_out": None}, {"n": 1}, {"n_out": 1}):
        rc, text = answer(good_layers(), good_outputs(), **kw)
        assert rc == -1 and "ctx is NULL" in text, (kw, text)  # every check of the arguments passed
    layers = good_layers()
    for i in range(4, 8):
        layers[i].data, layers[i].format = FAKE * (1 + i), capi.SRC_RGBA_F32
    rc, text = answer(layers, good_outputs(), n=8)
    assert rc == -1 and "ctx is NULL" in text, text


def test_no_output_with_an_image_is_accepted_as_far_as_the_context():
    rc, text = answer(good_layers(), good_outputs(), n_out=0)
    assert rc == -1 and "ctx is NULL" in text, text
    rc, text = answer(good_layers(), None, n_out=0)  # no outputs: no list of them is needed
    assert rc == -1 and "ctx is NULL" in text, text


def broken(change, fmts=("v210", "rgba8"), **kw):
    layers, outs = good_layers(), good_outputs(fmts)
    change(layers, outs)
    kw.setdefault("n_out", len(fmts))
    rc, text = answer(layers, outs, **kw)
    assert rc == -1, text  # PH_E_INVALID
    assert FN in text and "ctx is NULL" not in text, text
    return text


def test_every_refusal_names_its_cause():
    # the layers
    assert "1..8 layers" in broken(lambda l, o: None, n=0)
    assert "1..8 layers" in broken(lambda l, o: None, n=9)
    assert "layer 2 is NULL" in broken(lambda l, o: setattr(l[2], "data", None))
    assert "layer 3 is NULL" in broken(lambda l, o: setattr(l[3], "data", None))
    assert "layer 1: format 0 " in broken(lambda l, o: setattr(l[1], "format", 0))  # PH_SRC_NONE
    assert "layer 3: format 7 " in broken(lambda l, o: setattr(l[3], "format", capi.SRC_RGBA8))
    assert "PH_SRC_RGBA_F32" in broken(lambda l, o: setattr(l[0], "format", capi.SRC_YUV422P10))
    # the outputs' number, and nothing to make
    assert "0..4 outputs (-1)" in broken(lambda l, o: None, n_out=-1)
    assert "0..4 outputs (5)" in broken(lambda l, o: None, n_out=5)
    assert "nothing to make" in broken(lambda l, o: None, n_out=0, image_out=None)
    # the image beside what the call reads and writes
    assert "image_out is layer 3's data" in broken(lambda l, o: setattr(l[3], "data", IMAGE_OUT))
    assert "image_out is layer 0's data" in broken(lambda l, o: setattr(l[0], "data", IMAGE_OUT))
    assert "image_out is output 1's first plane" in broken(lambda l, o: o[1].planes.__setitem__(0, IMAGE_OUT))
    assert "image_out is output 0's first plane" in broken(lambda l, o: o[0].planes.__setitem__(0, IMAGE_OUT))
    # everything ph_fused_v210_combine_multi refuses about outputs and geometry
    assert "NULL argument" in answer(None, good_outputs())[1] and answer(None, good_outputs())[0] == -1
    assert "NULL argument" in answer(good_layers(), None)[1] and answer(good_layers(), None)[0] == -1
    for i in range(3):
        rd = [FAKE * 300, FAKE * 301, FAKE * 302]
        rd[i] = None
        assert "NULL argument" in broken(lambda l, o: None, rd=tuple(rd))
        assert "NULL argument" in broken(lambda l, o: None, rd=tuple(rd), n_out=0)
    assert "queue" in broken(lambda l, o: None, queue=99)
    assert "queue" in broken(lambda l, o: None, queue=99, n_out=0)
    assert "width 0" in broken(lambda l, o: None, w=0)
    assert "width 0" in broken(lambda l, o: None, w=0, n_out=0)
    assert "output 1: format 99 is not a PH_FMT_" in broken(lambda l, o: setattr(o[1], "format", 99))
    assert "output 1: interlace must be 0, 1 or 3" in broken(lambda l, o: setattr(o[1], "interlace", 2))
    assert "output 0: NULL argument" in broken(lambda l, o: o[0].planes.__setitem__(0, None))
    assert "output 1: NULL argument" in broken(lambda l, o: setattr(o[1], "wr_gamma_lut", None))
    assert "output 0: the writer's RGB -> YCbCr matrix is missing" in broken(lambda l, o: setattr(o[0], "wr_col_matrix12", None))
    assert "output 1: a planar output needs its three planes" in broken(lambda l, o: o[1].planes.__setitem__(2, None), fmts=("rgba8", "yuv422p8"))
    assert "output 1: a planar output needs its three planes" in broken(lambda l, o: o[1].planes.__setitem__(1, None), fmts=("rgba8", "nv12"))
    assert "output 1: a 4:2:0 frame needs an even height" in broken(lambda l, o: None, fmts=("rgba8", "yuv420p"), h=7)
    assert "output 0: width 383" in broken(lambda l, o: None, w=383)
    assert "multiple of 8" in broken(lambda l, o: None, fmts=("rgba8", "yuv422p8"), w=100)
    assert "outputs 0 and 1 name the same plane" in broken(lambda l, o: o[1].planes.__setitem__(0, o[0].planes[0]))
    # ... whatever the layers are: with plain layers and no image the refusals are still this entry's, made without a context
    def plain(l, o):
        l[3].format = capi.SRC_V210
        o[1].interlace = 2
    assert "output 1: interlace must be 0, 1 or 3" in broken(plain, image_out=None)


def test_the_10_bit_420_outputs_are_refused_with_the_siblings_message():
    sibling = capi.lib().ph_fused_v210_transition_multi
    for fmt in ("yuv420p10", "p010"):
        for k, n_out in ((1, 2), (0, 1)):
            text = broken(lambda l, o: setattr(o[k], "format", capi.FORMATS[fmt]), n_out=n_out)
            assert fmt in text
            cuts = (capi.PhFusedLayer * 4)()
            for i in range(4):
                cuts[i].v210 = FAKE * (1 + i)
            outs = good_outputs()
            outs[k].format = capi.FORMATS[fmt]
            assert sibling(None, capi.QUEUE_PROCESS, 4, cuts, n_out, outs, W, H, FAKE * 300, FAKE * 301, FAKE * 302) == -1
            theirs = capi.lib().ph_last_error(None).decode()
            assert text.replace(FN, "ph_fused_v210_transition_multi") == theirs
