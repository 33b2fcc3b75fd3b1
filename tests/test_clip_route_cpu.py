"""CPU-side checks of ph_clip_compose_route_multi's surface: the symbol and its binding, the by-name program's resolution, the ABI
number (the call is additive within 8), the header's declaration, and every refusal decided from the arguments - the entry point looks
at its context last, so these are answered without a device and before anything could be launched."""
import ctypes as C
import os
import re

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FN = "ph_clip_compose_route_multi"
W, H = 384, 6
FAKE = 0x10000  # a device address that nothing reads; the buffers below lie 64 KiB apart, more than any of them holds
IMAGE = FAKE * 400
CHAIN = ("ph_pack_read", "ph_transform", "ph_combine", "ph_pack_write_multi")


def test_the_symbol_is_exported_and_bound():
    assert FN in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), FN)
    fn = getattr(capi.lib(), FN)
    assert fn.restype is C.c_int
    sibling = list(capi.lib().ph_clip_compose_multi.argtypes)
    assert list(fn.argtypes) == sibling[:4] + [C.c_void_p] + sibling[4:]  # image_out between the layers and the outputs
    assert callable(capi.Context.clip_compose_route_multi)


def test_the_abi_is_still_8_and_the_header_declares_the_entry():
    assert capi.lib().ph_abi_version() == 8
    text = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    define = text.index("#define PH_ABI_VERSION 8")
    history = text[text.index("ABI history"):define]
    assert FN in history and '"clip_compose_route_<n>"' in history
    assert re.search(r"int %s\(ph_ctx \*ctx, int queue, int n, const ph_chan_layer \*layers, void \*image_out, int n_out,\s+const ph_chan_output \*outs," % FN,
                     text[define:])


def test_the_program_resolves_for_every_layer_count():
    assert capi.resolve_program("", "clip_compose_route_3") == ("clip_compose_route_3", None, "name")
    for n in range(1, 9):
        name = "clip_compose_route_%d" % n
        assert capi.resolve_program("phaneron:chan", name) == (name, None, "tag")
        sibling = "clip_compose_multi_%d" % n
        assert capi.resolve_program("phaneron:chan", sibling) == (sibling, None, "tag")  # the sibling is as it was
    for name, needle in (("clip_compose_route_", "plain layer count"), ("clip_compose_route_9", "layers are built"), ("clip_compose_route_0", "layers are built"),
                         ("clip_compose_route_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)


# ---- refusals: no context, device pointers that are never followed ---------------------------------------------------------------
IDENTITY = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
ROTATED = (C.c_float * 9)(0.9, 0.1, 0, -0.1, 0.9, 0, 0, 0, 1)
MIRRORED = (C.c_float * 9)(-1, 0, 0, 0, 1, 0, 0, 0, 1)


def clip_source(s, i, w=W // 2, h=4, matrix=IDENTITY):
    """a yuv420p clip of half the channel's size, placed by a matrix"""
    s.data, s.data_u, s.data_v = FAKE * (1 + 3 * i), FAKE * (2 + 3 * i), FAKE * (3 + 3 * i)
    s.format, s.width, s.height = capi.SRC_YUV420P, w, h
    s.matrix9_host = C.cast(matrix, C.POINTER(C.c_float))


def good_layers(n=9):
    arr = (capi.PhChanLayer * 9)()
    for i in range(n):
        clip_source(arr[i].src, i)
    return arr


def good_outputs(fmts=("v210", "rgba8")):
    outs = (capi.PhChanOutput * max(len(fmts), 5))()
    for k, f in enumerate(fmts):
        o = outs[k]
        o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
        for p in range(3):
            o.planes[p] = FAKE * (200 + 4 * k + p)
    return outs


def answer(layers, outs, n=1, n_out=2, w=W, h=H, rd=(FAKE * 300, FAKE * 301, FAKE * 302), queue=None, image=IMAGE):
    rc = getattr(capi.lib(), FN)(None, capi.QUEUE_PROCESS if queue is None else queue, n, layers, image, n_out, outs, w, h, *rd)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    for kw in ({}, {"h": 0}, {"n": 8}, {"n_out": 1}, {"n_out": 0}, {"n_out": 0, "n": 3}):
        rc, text = answer(good_layers(), good_outputs(), **kw)
        assert rc == -1 and "%s: ctx is NULL" % FN in text, (kw, text)  # every check of the arguments passed
    rc, text = answer(good_layers(), None, n_out=0)  # no output: no list of outputs either
    assert rc == -1 and "%s: ctx is NULL" % FN in text, text
    for fmts in (("yuv420p", "nv12", "yuv422p8", "yuv422p10"), ("bgra8",), ("v210", "v210"), ("v210",)):
        outs = good_outputs(fmts)
        outs[len(fmts) - 1].interlace = 3
        rc, text = answer(good_layers(), outs, n_out=len(fmts))
        assert rc == -1 and "%s: ctx is NULL" % FN in text, (fmts, text)
    # a frame of the channel's size under the default fill; an f32 image as a layer
    layers = good_layers()
    clip_source(layers[0].src, 0, W, H)
    layers[1].src.format, layers[1].src.data_u, layers[1].src.data_v = capi.SRC_RGBA_F32, None, None
    rc, text = answer(layers, good_outputs(), n=2)
    assert rc == -1 and "%s: ctx is NULL" % FN in text, text


def test_without_the_image_the_call_is_ph_clip_compose_multi():
    sibling = capi.lib().ph_clip_compose_multi
    for kw in ({}, {"n": 9}, {"w": 0}, {"n_out": 1}):
        rc, mine = answer(good_layers(), good_outputs(), image=None, **kw)
        assert sibling(None, capi.QUEUE_PROCESS, kw.get("n", 1), good_layers(), kw.get("n_out", 2), good_outputs(), kw.get("w", W), H, FAKE * 300, FAKE * 301, FAKE * 302) == rc == -1
        assert mine == capi.lib().ph_last_error(None).decode() and "ph_clip_compose_multi: " in mine


def broken(change, fmts=("v210", "rgba8"), **kw):
    layers, outs = good_layers(), good_outputs(fmts)
    change(layers, outs)
    kw.setdefault("n_out", len(fmts))
    rc, text = answer(layers, outs, **kw)
    assert rc == -1, text  # PH_E_INVALID
    assert "ctx is NULL" not in text, text
    return text


def names_the_chain(text):
    return all(step in text for step in CHAIN)


def test_every_refusal_names_its_cause():
    assert "NULL argument" in answer(None, good_outputs())[1] and answer(None, good_outputs())[0] == -1
    assert "NULL argument" in answer(good_layers(), None)[1] and answer(good_layers(), None)[0] == -1
    for i in range(3):
        rd = [FAKE * 300, FAKE * 301, FAKE * 302]
        rd[i] = None
        assert FN + ": NULL argument" in broken(lambda l, o: None, rd=tuple(rd))
    assert "1..8 layers" in broken(lambda l, o: None, n=0)
    assert "1..8 layers" in broken(lambda l, o: None, n=9)
    assert "0..4 outputs (-1)" in broken(lambda l, o: None, n_out=-1)
    assert "0..4 outputs (5)" in broken(lambda l, o: None, n_out=5)
    assert "0..4 outputs (5)" in broken(lambda l, o: None, n_out=5, image=None)
    assert "nothing to make: no output and image_out is NULL" in broken(lambda l, o: None, n_out=0, image=None)
    assert "queue" in broken(lambda l, o: None, queue=99)
    assert "width 0" in broken(lambda l, o: None, w=0)
    assert "width 0" in broken(lambda l, o: None, w=0, n_out=0)
    assert "output 1: format 99 is not a PH_FMT_" in broken(lambda l, o: setattr(o[1], "format", 99))
    assert "output 1: interlace must be 0, 1 or 3" in broken(lambda l, o: setattr(o[1], "interlace", 2))
    assert "output 0: NULL argument" in broken(lambda l, o: o[0].planes.__setitem__(0, None))
    assert "output 0: the writer's RGB -> YCbCr matrix is missing" in broken(lambda l, o: setattr(o[0], "wr_col_matrix12", None))
    assert "output 1: a planar output needs its three planes" in broken(lambda l, o: o[1].planes.__setitem__(2, None), fmts=("rgba8", "yuv422p8"))
    assert "output 1: a 4:2:0 frame needs an even height" in broken(lambda l, o: None, fmts=("rgba8", "yuv420p"), h=7)
    assert "multiple of 8" in broken(lambda l, o: None, fmts=("rgba8", "yuv422p8"), w=100)
    assert "outputs 0 and 1 name the same plane" in broken(lambda l, o: o[1].planes.__setitem__(0, o[0].planes[0]))
    # the layers, as the channel kernel's entries refuse them (their texts, under their name)
    assert "layer 0: the source is empty" in broken(lambda l, o: setattr(l[0].src, "data", None))
    assert "layer 0: transition 7" in broken(lambda l, o: setattr(l[0], "transition", 7))
    assert "layer 0: the transition's incoming source is empty" in broken(lambda l, o: setattr(l[0], "transition", 1))


def test_what_the_read_once_routes_do_not_take_is_refused_with_the_chain_to_run():
    def dissolve(l, o):
        l[1].transition, l[1].mix = 1, 0.25
        clip_source(l[1].incoming, 5)
    text = broken(dissolve, n=2)
    assert "layer 1 is in a transition" in text and names_the_chain(text), text
    for what, change in (("shrunk", lambda l, o: clip_source(l[0].src, 0, 2 * W, 2 * H)), ("as large as the channel but for a line", lambda l, o: clip_source(l[0].src, 0, W, H - 2)),
                         ("rotated", lambda l, o: clip_source(l[0].src, 0, matrix=ROTATED)), ("mirrored", lambda l, o: clip_source(l[0].src, 0, matrix=MIRRORED))):
        text = broken(change)
        assert "layer 0 is neither enlarged" in text and "default fill" in text and names_the_chain(text), (what, text)
    text = broken(lambda l, o: clip_source(l[2].src, 2, W + 2, H), n=3, n_out=0)
    assert "layer 2 is neither enlarged" in text and names_the_chain(text), text
    text = broken(lambda l, o: None, fmts=("rgba8",), w=W + 1)
    assert "odd" in text and names_the_chain(text), text


def test_image_out_may_overlap_nothing_the_call_reads_or_writes():
    image_bytes = W * H * 16
    # every plane of the clip, by either end of the image
    for plane in ("data", "data_u", "data_v"):
        for image in (lambda p: p, lambda p: p - image_bytes + 1, lambda p: p + 1):
            layers = good_layers()
            at = getattr(layers[0].src, plane)
            rc, text = answer(layers, good_outputs(), image=image(at))
            assert rc == -1 and "image_out overlaps a layer's source" in text, (plane, text)
    # ... and what lies right beside them is fine
    layers = good_layers()
    rc, text = answer(layers, good_outputs(), image=layers[0].src.data - image_bytes)
    assert "ctx is NULL" in text, text
    # an f32 layer image
    layers = good_layers()
    layers[1].src.format, layers[1].src.data_u, layers[1].src.data_v = capi.SRC_RGBA_F32, None, None
    rc, text = answer(layers, good_outputs(), n=2, image=layers[1].src.data + 16)
    assert rc == -1 and "image_out overlaps a layer's source" in text, text
    # every plane of every output
    for fmts in (("v210", "rgba8"), ("yuv422p10", "nv12"), ("yuv420p",)):
        for k in range(len(fmts)):
            for p in range(3 if fmts[k].startswith("yuv") else 2 if fmts[k] == "nv12" else 1):
                outs = good_outputs(fmts)
                rc, text = answer(good_layers(), outs, n_out=len(fmts), image=outs[k].planes[p] + 8)
                assert rc == -1 and "image_out overlaps an output's plane" in text, (fmts, k, p, text)


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
