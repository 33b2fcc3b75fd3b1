"""CPU-side checks of ph_clip_compose_transition_multi's surface: the symbol and its binding, the by-name program's resolution, the ABI
number (the call is additive within 8), the header's declaration, and every refusal decided from the arguments - the entry point looks
at its context last, so these are answered without a device and before anything could be launched."""
import ctypes as C
import os
import re

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FN = "ph_clip_compose_transition_multi"
W, H = 384, 6
FAKE = 0x10000  # a device address that nothing reads


def test_the_symbol_is_exported_and_bound():
    assert FN in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), FN)
    fn = getattr(capi.lib(), FN)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == list(capi.lib().ph_clip_compose_multi.argtypes)
    assert callable(capi.Context.clip_compose_transition_multi)


def test_the_abi_is_still_8_and_the_header_declares_the_entry():
    assert capi.lib().ph_abi_version() == 8
    text = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    define = text.index("#define PH_ABI_VERSION 8")
    history = text[text.index("ABI history"):define]
    assert FN in history and '"clip_compose_trans_<n>"' in history
    assert re.search(r"int %s\(ph_ctx \*ctx, int queue, int n, const ph_chan_layer \*layers, int n_out, const ph_chan_output \*outs," % FN, text[define:])


def test_the_program_resolves_for_every_layer_count():
    assert capi.resolve_program("", "clip_compose_trans_3") == ("clip_compose_trans_3", None, "name")
    for n in range(1, 9):
        name = "clip_compose_trans_%d" % n
        assert capi.resolve_program("phaneron:chan", name) == (name, None, "tag")
        sibling = "clip_compose_multi_%d" % n
        assert capi.resolve_program("phaneron:chan", sibling) == (sibling, None, "tag")  # the sibling is as it was
    for name, needle in (("clip_compose_trans_", "plain layer count"), ("clip_compose_trans_9", "layers are built"), ("clip_compose_trans_0", "layers are built"),
                         ("clip_compose_trans_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)


# ---- refusals: no context, device pointers that are never followed ---------------------------------------------------------------
IDENTITY = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)


def clip_source(s, i):
    """a yuv420p clip of half the channel's size, placed by a matrix"""
    s.data, s.data_u, s.data_v = FAKE * (1 + 3 * i), FAKE * (2 + 3 * i), FAKE * (3 + 3 * i)
    s.format, s.width, s.height = capi.SRC_YUV420P, W // 2, 4
    s.matrix9_host = C.cast(IDENTITY, C.POINTER(C.c_float))


def good_layers(transition=1, n=9):
    """layers in a dissolve (1) or a wipe (2), each with the partners the transition needs"""
    arr = (capi.PhChanLayer * 9)()
    for i in range(n):
        clip_source(arr[i].src, 3 * i)
        arr[i].transition, arr[i].mix = transition, 0.25
        if transition >= 1:
            clip_source(arr[i].incoming, 3 * i + 1)
        if transition == 2:
            clip_source(arr[i].mask, 3 * i + 2)
    return arr


def good_outputs(fmts=("v210", "rgba8")):
    outs = (capi.PhChanOutput * max(len(fmts), 5))()
    for k, f in enumerate(fmts):
        o = outs[k]
        o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
        for p in range(3):
            o.planes[p] = FAKE * (200 + 4 * k + p)
    return outs


def answer(layers, outs, n=1, n_out=2, w=W, h=H, rd=(FAKE * 300, FAKE * 301, FAKE * 302), queue=None):
    rc = getattr(capi.lib(), FN)(None, capi.QUEUE_PROCESS if queue is None else queue, n, layers, n_out, outs, w, h, *rd)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    for transition in (0, 1, 2):
        for kw in ({}, {"h": 0}, {"n": 8}, {"n_out": 1}):
            rc, text = answer(good_layers(transition), good_outputs(), **kw)
            assert rc == -1 and "%s: ctx is NULL" % FN in text, (transition, kw, text)  # every check of the arguments passed
    for fmts in (("yuv420p", "nv12", "yuv422p8", "yuv422p10"), ("bgra8",), ("v210", "v210")):
        outs = good_outputs(fmts)
        outs[1].interlace = 3
        rc, text = answer(good_layers(2), outs, n_out=len(fmts))
        assert rc == -1 and "%s: ctx is NULL" % FN in text, (fmts, text)


def broken(change, fmts=("v210", "rgba8"), transition=1, **kw):
    layers, outs = good_layers(transition), good_outputs(fmts)
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
    assert "output 1: interlace must be 0, 1 or 3" in broken(lambda l, o: setattr(o[1], "interlace", 2))
    assert "output 0: NULL argument" in broken(lambda l, o: o[0].planes.__setitem__(0, None))
    assert "output 0: the writer's RGB -> YCbCr matrix is missing" in broken(lambda l, o: setattr(o[0], "wr_col_matrix12", None))
    assert "output 1: a planar output needs its three planes" in broken(lambda l, o: o[1].planes.__setitem__(2, None), fmts=("rgba8", "yuv422p8"))
    assert "output 1: a 4:2:0 frame needs an even height" in broken(lambda l, o: None, fmts=("rgba8", "yuv420p"), h=7)
    assert "multiple of 8" in broken(lambda l, o: None, fmts=("rgba8", "yuv422p8"), w=100)
    # two outputs on one first plane
    assert "outputs 0 and 1 name the same plane" in broken(lambda l, o: o[1].planes.__setitem__(0, o[0].planes[0]))
    # the layers and their transitions, as the channel kernel's entries refuse them
    assert "layer 0: the source is empty" in broken(lambda l, o: setattr(l[0].src, "data", None))
    assert "layer 0: transition 7" in broken(lambda l, o: setattr(l[0], "transition", 7))
    assert "layer 0: transition 3" in broken(lambda l, o: setattr(l[0], "transition", 3))
    assert "layer 0: transition -1" in broken(lambda l, o: setattr(l[0], "transition", -1))
    assert "layer 0: the transition's incoming source is empty" in broken(lambda l, o: setattr(l[0].incoming, "data", None))  # a dissolve without `incoming`
    assert "layer 1: the transition's incoming source is empty" in broken(lambda l, o: setattr(l[1].incoming, "data", None), transition=2, n=2)
    assert "layer 0: the wipe's mask is empty" in broken(lambda l, o: setattr(l[0].mask, "data", None), transition=2)  # a wipe without a mask
    assert "layer 0: the wipe's mask is a yuv420p frame" in broken(lambda l, o: setattr(l[0].mask, "data_v", None), transition=2)


def test_the_10_bit_420_outputs_are_refused_with_the_channel_kernels_message():
    for fmt in ("yuv420p10", "p010"):
        for k, n_out in ((1, 2), (0, 1)):
            text = broken(lambda l, o: setattr(o[k], "format", capi.FORMATS[fmt]), n_out=n_out)
            assert fmt in text and "does not write" in text and "ph_pack_write" in text
    # ... which is ph_clip_compose_multi's own text for the same call, under its own name
    sibling = capi.lib().ph_clip_compose_multi
    for fmt in ("yuv420p10", "p010"):
        outs = good_outputs()
        outs[1].format = capi.FORMATS[fmt]
        assert sibling(None, capi.QUEUE_PROCESS, 1, good_layers(), 2, outs, W, H, FAKE * 300, FAKE * 301, FAKE * 302) == -1
        theirs = capi.lib().ph_last_error(None).decode()
        rc, mine = answer(good_layers(), outs)
        assert rc == -1 and mine.replace(FN, "ph_clip_compose_multi") == theirs
