"""CPU-side checks of ph_clip_compose_multi's surface: the symbol and its binding, the by-name program's resolution, the ABI number (the
call is additive within 8), and every refusal decided from the arguments - the entry point looks at its context last, so these are
answered without a device and before anything could be launched."""
import ctypes as C
import os
import re

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FN = "ph_clip_compose_multi"
W, H = 384, 6
FAKE = 0x10000  # a device address that nothing reads


def test_the_symbol_is_exported_and_bound():
    assert FN in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), FN)
    fn = getattr(capi.lib(), FN)
    ci, cu, vp = C.c_int, C.c_uint32, C.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, C.POINTER(capi.PhChanLayer), ci, C.POINTER(capi.PhChanOutput), cu, cu, vp, vp, vp]
    assert list(fn.argtypes) == list(capi.lib().ph_chan_compose_multi.argtypes)  # the sibling's signature
    assert callable(capi.Context.clip_compose_multi)


def test_the_abi_is_still_8_and_the_header_names_the_entry_in_its_history():
    assert capi.lib().ph_abi_version() == 8
    text = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    define = text.index("#define PH_ABI_VERSION 8")
    history = text[text.index("ABI history"):define]
    assert FN in history and '"clip_compose_multi_<n>"' in history
    assert re.search(r"int %s\(ph_ctx \*ctx, int queue, int n, const ph_chan_layer \*layers, int n_out, const ph_chan_output \*outs," % FN, text[define:])


def test_the_program_resolves_for_every_layer_count():
    assert capi.resolve_program("", "clip_compose_multi_3") == ("clip_compose_multi_3", None, "name")
    for n in range(1, 9):
        name = "clip_compose_multi_%d" % n
        assert capi.resolve_program("phaneron:chan", name) == (name, None, "tag")
        sibling = "chan_compose_multi_%d" % n
        assert capi.resolve_program("phaneron:chan", sibling) == (sibling, None, "tag")  # the sibling is as it was
    for name, needle in (("clip_compose_multi_", "plain layer count"), ("clip_compose_multi_9", "layers are built"), ("clip_compose_multi_0", "layers are built"),
                         ("clip_compose_multi_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)


# ---- refusals: no context, device pointers that are never followed ---------------------------------------------------------------
IDENTITY = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)


def good_layers(n=9):
    """yuv420p clips of half the channel's size, placed by a matrix"""
    arr = (capi.PhChanLayer * 9)()
    for i in range(n):
        s = arr[i].src
        s.data, s.data_u, s.data_v = FAKE * (1 + 3 * i), FAKE * (2 + 3 * i), FAKE * (3 + 3 * i)
        s.format, s.width, s.height = capi.SRC_YUV420P, W // 2, 4
        s.matrix9_host = C.cast(IDENTITY, C.POINTER(C.c_float))
        arr[i].transition = 0
    return arr


def good_outputs(fmts=("v210", "rgba8")):
    outs = (capi.PhChanOutput * max(len(fmts), 5))()
    for k, f in enumerate(fmts):
        o = outs[k]
        o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
        for p in range(3):
            o.planes[p] = FAKE * (200 + 4 * k + p)
    return outs


def answer(layers, outs, n=1, n_out=2, w=W, h=H, rd=(FAKE * 300, FAKE * 301, FAKE * 302), queue=None, fn=FN):
    rc = getattr(capi.lib(), fn)(None, capi.QUEUE_PROCESS if queue is None else queue, n, layers, n_out, outs, w, h, *rd)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    for kw in ({}, {"h": 0}, {"n": 8}, {"n_out": 1}):
        rc, text = answer(good_layers(), good_outputs(), **kw)
        assert rc == -1 and "%s: ctx is NULL" % FN in text, (kw, text)  # every check of the arguments passed
    for fmts in (("yuv420p", "nv12", "yuv422p8", "yuv422p10"), ("bgra8",), ("v210", "v210")):
        outs = good_outputs(fmts)
        outs[1].interlace = 3
        rc, text = answer(good_layers(), outs, n_out=len(fmts))
        assert rc == -1 and "%s: ctx is NULL" % FN in text, (fmts, text)


def broken(change, fmts=("v210", "rgba8"), **kw):
    layers, outs = good_layers(), good_outputs(fmts)
    change(layers, outs)
    kw.setdefault("n_out", len(fmts))
    rc, text = answer(layers, outs, **kw)
    assert rc == -1, text  # PH_E_INVALID
    assert "ctx is NULL" not in text, text
    return text


def test_every_refusal_names_its_cause():
    assert "NULL argument" in answer(None, good_outputs())[1] and answer(None, good_outputs())[0] == -1
    assert "NULL argument" in answer(good_layers(), None)[1] and answer(good_layers(), None)[0] == -1
    for i in range(3):
        rd = [FAKE * 300, FAKE * 301, FAKE * 302]
        rd[i] = None
        assert FN + ": NULL argument" in broken(lambda l, o: None, rd=tuple(rd))
    assert "1..8 layers" in broken(lambda l, o: None, n=0)
    assert "1..8 layers" in broken(lambda l, o: None, n=9)
    assert "1..4 outputs (0)" in broken(lambda l, o: None, n_out=0)
    assert "1..4 outputs (5)" in broken(lambda l, o: None, n_out=5)
    assert "queue" in broken(lambda l, o: None, queue=99)
    assert "width 0" in broken(lambda l, o: None, w=0)
    assert "output 1: format 99 is not a PH_FMT_" in broken(lambda l, o: setattr(o[1], "format", 99))
    assert "output 0: format 99 is not a PH_FMT_" in broken(lambda l, o: setattr(o[0], "format", 99), n_out=1)
    assert "output 1: interlace must be 0, 1 or 3" in broken(lambda l, o: setattr(o[1], "interlace", 2))
    assert "output 0: NULL argument" in broken(lambda l, o: o[0].planes.__setitem__(0, None))
    assert "output 1: NULL argument" in broken(lambda l, o: setattr(o[1], "wr_gamma_lut", None))
    assert "output 0: the writer's RGB -> YCbCr matrix is missing" in broken(lambda l, o: setattr(o[0], "wr_col_matrix12", None))
    assert "output 1: a planar output needs its three planes" in broken(lambda l, o: o[1].planes.__setitem__(2, None), fmts=("rgba8", "yuv422p8"))
    assert "output 1: a planar output needs its three planes" in broken(lambda l, o: o[1].planes.__setitem__(1, None), fmts=("rgba8", "nv12"))
    assert "output 1: a 4:2:0 frame needs an even height" in broken(lambda l, o: None, fmts=("rgba8", "yuv420p"), h=7)
    assert "output 0: a 4:2:0 frame needs an even height" in broken(lambda l, o: None, fmts=("nv12",), h=7)
    assert "output 0: width 383" in broken(lambda l, o: None, w=383)
    assert "multiple of 8" in broken(lambda l, o: None, fmts=("rgba8", "yuv422p8"), w=100)
    assert "outputs 0 and 1 name the same plane" in broken(lambda l, o: o[1].planes.__setitem__(0, o[0].planes[0]))
    # the layers, as the channel kernel's entries refuse them
    assert "layer 0: the source is empty" in broken(lambda l, o: setattr(l[0].src, "data", None))
    assert "layer 0: transition 7" in broken(lambda l, o: setattr(l[0], "transition", 7))
    assert "layer 1: the source is a yuv420p frame" in broken(lambda l, o: setattr(l[1].src, "data_v", None), n=2)


def test_the_10_bit_420_outputs_are_refused_with_the_channel_kernels_message():
    for fmt in ("yuv420p10", "p010"):
        for k, n_out in ((1, 2), (0, 1)):
            text = broken(lambda l, o: setattr(o[k], "format", capi.FORMATS[fmt]), n_out=n_out)
            assert fmt in text and "ph_pack_write" in text
    # ... which is ph_chan_compose_multi's own text for the same call, under its own name (it wants its context first: compare through a sibling
    # that checks its arguments as this entry does)
    sibling = capi.lib().ph_fused_v210_transition_multi
    cuts = (capi.PhFusedLayer * 4)()
    for i in range(4):
        cuts[i].v210 = FAKE * (1 + i)
    for fmt in ("yuv420p10", "p010"):
        outs = good_outputs()
        outs[1].format = capi.FORMATS[fmt]
        assert sibling(None, capi.QUEUE_PROCESS, 4, cuts, 2, outs, W, H, FAKE * 300, FAKE * 301, FAKE * 302) == -1
        theirs = capi.lib().ph_last_error(None).decode()
        rc, mine = answer(good_layers(), outs)
        assert rc == -1 and mine.replace(FN, "ph_fused_v210_transition_multi") == theirs
