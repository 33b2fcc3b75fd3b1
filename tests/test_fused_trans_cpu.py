"""CPU-side checks of ph_fused_v210_transition_multi's surface: ph_fused_layer as the header and the binding lay it out, the symbol, the
by-name program's resolution, the ABI number (the call is additive within 8), and every refusal - the entry point looks at its context
last, so these are answered without a device and before anything could be launched."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIELDS = ["v210", "transition", "mix", "incoming_v210", "mask", "mask_format"]
FN = "ph_fused_v210_transition_multi"


def test_the_struct_is_laid_out_as_the_header_says(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "phaneron_hip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(ph_fused_layer));']
    lines += ['  printf("%%zu\\n", offsetof(ph_fused_layer, %s));' % f for f in FIELDS]
    lines += ['  printf("%d %d %d %d %d\\n", PH_TRANSITION_CUT, PH_TRANSITION_DISSOLVE, PH_TRANSITION_WIPE, PH_SRC_V210, PH_SRC_RGBA_F32);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    T = capi.PhFusedLayer
    want = [C.sizeof(T)] + [getattr(T, f).offset for f in FIELDS]
    assert [int(x) for x in got[:len(want)]] == want
    assert [f for f, _ in T._fields_] == FIELDS
    assert got[len(want)].split() == [str(x) for x in (capi.TRANSITION_CUT, capi.TRANSITION_DISSOLVE, capi.TRANSITION_WIPE, capi.SRC_V210, capi.SRC_RGBA_F32)]
    assert C.sizeof(capi.PhChanOutput) == 56  # (the struct beside it is as it was)


def test_the_symbol_is_exported_and_bound():
    assert FN in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), FN)
    fn = getattr(capi.lib(), FN)
    ci, cu, vp = C.c_int, C.c_uint32, C.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, C.POINTER(capi.PhFusedLayer), ci, C.POINTER(capi.PhChanOutput), cu, cu, vp, vp, vp]
    assert callable(capi.Context.fused_v210_transition_multi)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


def test_the_program_resolves_for_every_layer_count():
    assert capi.resolve_program("", "fused_v210_trans_3") == ("fused_v210_trans_3", None, "name")
    for n in range(1, 9):
        name = "fused_v210_trans_%d" % n
        assert capi.resolve_program("phaneron:fused", name) == (name, None, "tag")
        sibling = "fused_v210_combine_multi_%d" % n
        assert capi.resolve_program("phaneron:fused", sibling) == (sibling, None, "tag")  # the sibling is as it was
    for name, needle in (("fused_v210_trans_", "plain layer count"), ("fused_v210_trans_9", "layers are built"), ("fused_v210_trans_0", "layers are built"),
                         ("fused_v210_trans_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)
    assert capi.resolve_program("", "fused_v210_combine_4") == ("fused_v210_combine_4", None, "name")


# ---- refusals: no context, device pointers that are never followed ---------------------------------------------------------------
W, H = 384, 6
FAKE = 0x10000  # a device address that nothing reads


def good_layers():
    """a cut under a dissolve under a wipe by a v210 mask under a wipe by an f32 mask"""
    arr = (capi.PhFusedLayer * 8)()
    kinds = (capi.TRANSITION_CUT, capi.TRANSITION_DISSOLVE, capi.TRANSITION_WIPE, capi.TRANSITION_WIPE)
    for i, kind in enumerate(kinds):
        arr[i].v210, arr[i].transition, arr[i].mix = FAKE * (1 + 4 * i), kind, 0.25
        if kind != capi.TRANSITION_CUT:
            arr[i].incoming_v210 = FAKE * (2 + 4 * i)
        if kind == capi.TRANSITION_WIPE:
            arr[i].mask, arr[i].mask_format = FAKE * (3 + 4 * i), capi.SRC_V210 if i == 2 else capi.SRC_RGBA_F32
    return arr


def good_outputs(fmts=("v210", "rgba8")):
    outs = (capi.PhChanOutput * max(len(fmts), 5))()
    for k, f in enumerate(fmts):
        o = outs[k]
        o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
        for p in range(3):
            o.planes[p] = FAKE * (200 + 4 * k + p)
    return outs


def answer(layers, outs, n=4, n_out=2, w=W, h=H, rd=(FAKE * 300, FAKE * 301, FAKE * 302), queue=None):
    rc = getattr(capi.lib(), FN)(None, capi.QUEUE_PROCESS if queue is None else queue, n, layers, n_out, outs, w, h, *rd)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    rc, text = answer(good_layers(), good_outputs())
    assert rc == -1 and "ctx is NULL" in text, text  # every check of the arguments passed
    rc, text = answer(good_layers(), good_outputs(), h=0)
    assert rc == -1 and "ctx is NULL" in text, text
    layers = good_layers()
    layers[0].incoming_v210 = layers[0].mask = None  # what a cut layer says beside its frame is not looked at
    layers[0].mask_format, layers[1].mask_format = 77, 77  # nor a dissolve's mask
    rc, text = answer(layers, good_outputs())
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
    # the transitions
    assert "layer 1: transition 3 is not" in broken(lambda l, o: setattr(l[1], "transition", 3))
    assert "layer 0: transition -1 is not" in broken(lambda l, o: setattr(l[0], "transition", -1))
    assert "layer 1: a layer in a transition needs its incoming frame" in broken(lambda l, o: setattr(l[1], "incoming_v210", None))
    assert "layer 3: a layer in a transition needs its incoming frame" in broken(lambda l, o: setattr(l[3], "incoming_v210", None))
    assert "layer 2: a wipe needs its mask" in broken(lambda l, o: setattr(l[2], "mask", None))
    assert "layer 3: mask format 0" in broken(lambda l, o: setattr(l[3], "mask_format", 0))  # PH_SRC_NONE
    assert "layer 2: mask format 7" in broken(lambda l, o: setattr(l[2], "mask_format", capi.SRC_RGBA8))
    # everything ph_fused_v210_combine_multi refuses
    assert "NULL argument" in answer(None, good_outputs())[1] and answer(None, good_outputs())[0] == -1
    assert "NULL argument" in answer(good_layers(), None)[1] and answer(good_layers(), None)[0] == -1
    for i in range(3):
        rd = [FAKE * 300, FAKE * 301, FAKE * 302]
        rd[i] = None
        assert "NULL argument" in broken(lambda l, o: None, rd=tuple(rd))
    assert "layer 2 is NULL" in broken(lambda l, o: setattr(l[2], "v210", None))
    assert "1..8 layers" in broken(lambda l, o: None, n=0)
    assert "1..8 layers" in broken(lambda l, o: None, n=9)
    assert "1..4 outputs (0)" in broken(lambda l, o: None, n_out=0)
    assert "1..4 outputs (5)" in broken(lambda l, o: None, n_out=5)
    assert "queue" in broken(lambda l, o: None, queue=99)
    assert "width 0" in broken(lambda l, o: None, w=0)
    assert "output 1: format 99 is not a PH_FMT_" in broken(lambda l, o: setattr(o[1], "format", 99))
    for fmt in ("yuv420p10", "p010"):
        assert "%s" % fmt in broken(lambda l, o: setattr(o[1], "format", capi.FORMATS[fmt]))
        assert "%s" % fmt in broken(lambda l, o: setattr(o[0], "format", capi.FORMATS[fmt]), n_out=1)
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
    # ... whatever the layers are: with every layer a cut the refusals are still this entry's, made without a context
    def cuts(l, o):
        for i in range(4):
            l[i].transition = capi.TRANSITION_CUT
        o[1].interlace = 2
    assert "output 1: interlace must be 0, 1 or 3" in broken(cuts)
