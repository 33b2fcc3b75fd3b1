"""CPU-side checks of ph_clip_compose_batch_out's surface: the symbol and its binding, the ABI number (the call is additive within 8), and
every refusal decided from the arguments - the entry point looks at its context last, so these are answered with a context pointer that
is never followed, without a device and before anything could be launched.  The texts are ph_chan_compose_batch_out's with the function
name replaced (that entry wants its context first: its texts are spelled out here, and tests/test_clip_batch_gpu.py compares the two
entries' answers on a device)."""
import ctypes as C
import os
import re

import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FN = "ph_clip_compose_batch_out"
SIBLING = "ph_chan_compose_batch_out"
W, H = 384, 6
FAKE = 0x10000  # a device address that nothing reads
FAKE_CTX = 0x7000  # a context that nothing follows
IDENTITY = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)


def test_the_symbol_is_exported_and_bound_with_the_siblings_argtypes():
    assert FN in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), FN)
    fn = getattr(capi.lib(), FN)
    ci, cu, vp = C.c_int, C.c_uint32, C.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, C.POINTER(capi.PhChanJobOut), cu, cu, vp, vp, vp]
    assert list(fn.argtypes) == list(getattr(capi.lib(), SIBLING).argtypes)
    assert callable(capi.Context.clip_compose_batch_out)


def test_the_abi_is_still_8_and_the_header_names_the_entry_in_its_history():
    assert capi.lib().ph_abi_version() == 8
    text = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    define = text.index("#define PH_ABI_VERSION 8")
    history = text[text.index("ABI history"):define]
    assert FN + " (ph_chan_job_out)" in history and '"clip_batch"' in history
    assert re.search(r"int %s\(ph_ctx \*ctx, int queue, int n_jobs, const ph_chan_job_out \*jobs, uint32_t out_width, uint32_t out_height," % FN, text[define:])


def layers_of(job):
    """a yuv420p clip of half the channel's width, placed by a matrix"""
    arr = (capi.PhChanLayer * 2)()
    for i in range(2):
        s = arr[i].src
        s.data, s.data_u, s.data_v = FAKE * (1 + 8 * job + 3 * i), FAKE * (2 + 8 * job + 3 * i), FAKE * (3 + 8 * job + 3 * i)
        s.format, s.width, s.height = capi.SRC_YUV420P, W // 2, 4
        s.matrix9_host = C.cast(IDENTITY, C.POINTER(C.c_float))
        arr[i].transition = 0
    return arr


def outputs_of(job, fmts):
    outs = (capi.PhChanOutput * max(len(fmts), 5))()
    for k, f in enumerate(fmts):
        o = outs[k]
        o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
        for p in range(3):
            o.planes[p] = FAKE * (200 + 16 * job + 4 * k + p)
    return outs


def good_jobs(n=3, fmts=("v210", "rgba8")):
    keep = [(layers_of(j), outputs_of(j, fmts)) for j in range(n)]
    arr = (capi.PhChanJobOut * n)()
    for j, (la, outs) in enumerate(keep):
        arr[j].n, arr[j].layers, arr[j].n_out, arr[j].outs = 1, la, len(fmts), outs
    return arr, keep


def answer(jobs, n_jobs=3, w=W, h=H, rd=(FAKE * 300, FAKE * 301, FAKE * 302), queue=None, ctx=FAKE_CTX):
    rc = getattr(capi.lib(), FN)(ctx, capi.QUEUE_PROCESS if queue is None else queue, n_jobs, jobs, w, h, *rd)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    for fmts in (("v210", "rgba8"), ("nv12",), ("yuv420p", "nv12", "yuv422p8", "yuv422p10"), ("v210",)):
        for kw in ({}, {"h": 0}, {"n_jobs": 1}):
            jobs, keep = good_jobs(fmts=fmts)
            rc, text = answer(jobs, ctx=None, **kw)
            assert rc == -1 and text == "%s: ctx is NULL" % FN, (fmts, kw, text)  # every check of the arguments passed


def refused(change=lambda arr, keep: None, fmts=("v210", "rgba8"), own_name=True, **kw):
    jobs, keep = good_jobs(fmts=fmts)
    change(jobs, keep)
    rc, text = answer(jobs, **kw)  # (a context pointer that would fault if it were followed)
    assert rc == -1, text  # PH_E_INVALID
    assert text.startswith(FN + ": ") or not own_name, text
    return text.replace(FN, SIBLING)


def test_every_refusal_is_the_siblings_text_under_this_name():
    assert answer(None) == (-1, "%s: NULL argument" % FN)
    for i in range(3):
        rd = [FAKE * 300, FAKE * 301, FAKE * 302]
        rd[i] = None
        assert refused(rd=tuple(rd)) == SIBLING + ": NULL argument"
    assert refused(n_jobs=0) == SIBLING + ": no jobs"
    assert refused(n_jobs=-2) == SIBLING + ": no jobs"
    assert refused(w=0) == SIBLING + ": width 0"
    assert "queue" in refused(queue=99)
    assert refused(lambda a, k: setattr(a[1], "layers", None)) == SIBLING + ": job 1: NULL argument"
    assert refused(lambda a, k: setattr(a[2], "outs", None)) == SIBLING + ": job 2: NULL argument"
    assert refused(lambda a, k: setattr(a[0], "n_out", 0)) == SIBLING + ": job 0: 1..4 outputs (0)"
    assert refused(lambda a, k: setattr(a[1], "n_out", 5)) == SIBLING + ": job 1: 1..4 outputs (5)"
    assert refused(lambda a, k: setattr(a[1], "n", 0)) == SIBLING + ": job 1: 1..8 layers"
    assert refused(lambda a, k: setattr(a[1], "n", 9)) == SIBLING + ": job 1: 1..8 layers"
    assert refused(lambda a, k: setattr(k[2][1][1], "format", 99)) == SIBLING + ": job 2: output 1: format 99 is not a PH_FMT_*"
    assert refused(lambda a, k: setattr(k[1][1][0], "interlace", 2)) == SIBLING + ": job 1: output 0: interlace must be 0, 1 or 3"
    assert refused(lambda a, k: k[1][1][0].planes.__setitem__(0, None)) == SIBLING + ": job 1: output 0: NULL argument"
    assert refused(lambda a, k: setattr(k[0][1][0], "wr_col_matrix12", None)) == SIBLING + ": job 0: output 0: the writer's RGB -> YCbCr matrix is missing"
    assert refused(lambda a, k: k[1][1][1].planes.__setitem__(2, None), fmts=("rgba8", "yuv422p8")) == \
        SIBLING + ": job 1: output 1: a planar output needs its three planes (nv12: Y and the interleaved CbCr plane)"
    assert refused(fmts=("rgba8", "yuv420p"), h=7) == SIBLING + ": job 0: output 1: a 4:2:0 frame needs an even height (7)"
    # two outputs of a job naming one first plane - of any job
    for j in range(3):
        assert refused(lambda a, k: k[j][1][1].planes.__setitem__(0, k[j][1][0].planes[0])) == SIBLING + ": job %d: outputs 0 and 1 name the same plane" % j
    # an odd width; a planar output at width % 8 != 0
    width = ": job 0: output %d: width %d (a v210 frame needs an even width, a planar one a multiple of 8); run the separate kernels"
    assert refused(w=383) == SIBLING + width % (0, 383)
    assert refused(fmts=("rgba8", "yuv422p8"), w=100) == SIBLING + width % (1, 100)
    # the layers, as the channel kernel's entries refuse them (under that kernel's name, in the sibling too)
    assert refused(lambda a, k: setattr(k[1][0][0].src, "data", None), own_name=False) == "ph_chan_compose_v210: layer 0: the source is empty"
    assert "layer 0: transition 7" in refused(lambda a, k: setattr(k[2][0][0], "transition", 7), own_name=False)


def test_the_10_bit_420_outputs_are_refused_with_the_channel_kernels_message():
    for fmt in ("yuv420p10", "p010"):
        for j, k in ((0, 0), (2, 1)):
            text = refused(lambda a, keep: setattr(keep[j][1][k], "format", capi.FORMATS[fmt]))
            assert text == SIBLING + ": the channel kernel does not write %s frames - run the separate kernels: the channel's frame as an image, then the format's writer (ph_pack_write)" % fmt
    assert "does not write p010 frames" in refused(lambda a, keep: setattr(keep[1][1][0], "format", capi.FORMATS["p010"]))


def test_the_option_takes_0_or_1():
    """(the value is refused before the context is touched)"""
    set_option = capi.lib().ph_ctx_set_option
    for value in (2, -1, 7):
        assert set_option(FAKE_CTX, b"clip_batch", value) == -1
        text = capi.lib().ph_last_error(None).decode()
        assert text == "clip_batch: 0 (a launch per such job) or 1 (shared launches)", text
    header = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    assert '"clip_batch" (default 0)' in header
