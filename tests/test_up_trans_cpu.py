"""CPU-side checks of ph_compose_up_transition_multi's surface: ph_image_trans_layer as the header and the binding lay it out, the symbol,
the by-name program's resolution, the ABI number (the call is additive within 8), and every refusal the arguments alone decide - the
entry point looks at its context last, so these are answered without a device and before anything could be launched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from phaneron_amd import build, capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIELDS = ["src", "src.data", "src.format", "src.width", "src.height", "src.matrix9_host", "transition", "mix", "incoming", "mask"]


def test_the_struct_is_laid_out_as_the_header_says(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "phaneron_hip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(ph_image_trans_layer));']
    lines += ['  printf("%%zu\\n", offsetof(ph_image_trans_layer, %s));' % f for f in FIELDS]
    lines += ['  printf("%d %d %d\\n", PH_TRANSITION_CUT, PH_TRANSITION_DISSOLVE, PH_TRANSITION_WIPE);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    T, L = capi.PhImageTransLayer, capi.PhImageLayer
    want = [C.sizeof(T)]
    for f in FIELDS:
        outer, _, inner = f.partition(".")
        want.append(getattr(T, outer).offset + (getattr(L, inner).offset if inner else 0))
    assert [int(x) for x in got[:len(want)]] == want
    assert got[len(want)].split() == [str(capi.TRANSITION_CUT), str(capi.TRANSITION_DISSOLVE), str(capi.TRANSITION_WIPE)]
    assert C.sizeof(L) == 32 and C.sizeof(capi.PhChanOutput) == 56  # (the structs it is made of are as they were)


def test_the_symbol_is_exported_and_bound():
    assert "ph_compose_up_transition_multi" in capi.EXPORTS
    assert hasattr(C.CDLL(build.build()), "ph_compose_up_transition_multi")
    fn = capi.lib().ph_compose_up_transition_multi
    ci, cu, vp = C.c_int, C.c_uint32, C.c_void_p
    assert fn.restype is ci
    assert list(fn.argtypes) == [vp, ci, ci, ci, C.POINTER(C.POINTER(capi.PhImageTransLayer)), ci, C.POINTER(capi.PhChanOutput), cu, cu]
    assert callable(capi.Context.compose_up_transition_multi)


def test_the_abi_is_still_8():
    assert capi.lib().ph_abi_version() == 8


def test_the_program_resolves_for_every_layer_count():
    assert capi.resolve_program("", "compose_up_trans_3") == ("compose_up_trans_3", None, "name")
    for n in range(1, 9):
        name = "compose_up_trans_%d" % n
        assert capi.resolve_program("phaneron:up", name) == (name, None, "tag")
    for name, needle in (("compose_up_trans_", "plain layer count"), ("compose_up_trans_9", "layers are built"), ("compose_up_trans_0", "layers are built"),
                         ("compose_up_trans_2x", "plain layer count")):
        with pytest.raises(capi.PhaneronError, match=needle):
            capi.resolve_program("", name)
    assert capi.resolve_program("", "compose_up_multi_4") == ("compose_up_multi_4", None, "name")  # the sibling is as it was


# ---- refusals: no context, device pointers that are never followed ---------------------------------------------------------------
OW, OH = 192, 54
FAKE = 0x10000  # a device address that nothing reads
_keep = []


def matrix(*six):
    m = np.array(list(six or (1, 0, 0, 0, 1, 0)) + [0, 0, 1], np.float32)
    _keep.append(m)
    return m.ctypes.data_as(C.POINTER(C.c_float))


def image(dst, w=96, h=13, six=(), data=FAKE, fmt=capi.IMG_RGB_F32):
    dst.data, dst.format, dst.width, dst.height, dst.matrix9_host = data, fmt, w, h, matrix(*six)


def good_layers(jobs=1):
    """per job: a dissolving layer under a wiping one, every image 96 x 13 under the identity (2x across, 4x down)"""
    sets = []
    for j in range(jobs):
        arr = (capi.PhImageTransLayer * 2)()
        for i, kind in enumerate((capi.TRANSITION_DISSOLVE, capi.TRANSITION_WIPE)):
            image(arr[i].src, data=FAKE * (1 + 16 * j + 4 * i))
            image(arr[i].incoming, data=FAKE * (2 + 16 * j + 4 * i))
            arr[i].transition, arr[i].mix = kind, 0.25 + 0.5 * j
            if kind == capi.TRANSITION_WIPE:
                image(arr[i].mask, data=FAKE * (3 + 16 * j + 4 * i))
        sets.append(arr)
    return sets


def good_outputs(jobs=1, fmts=("v210", "rgba8")):
    outs = (capi.PhChanOutput * (jobs * len(fmts)))()
    for j in range(jobs):
        for k, f in enumerate(fmts):
            o = outs[j * len(fmts) + k]
            o.format, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut = capi.FORMATS[f], 0, FAKE * 100, FAKE * 101
            for p in range(3):
                o.planes[p] = FAKE * (200 + 16 * j + 4 * k + p)
    return outs


def answer(sets, outs, n_out=2, n=2, ow=OW, oh=OH, jobs=None):
    jobs = len(sets) if jobs is None else jobs
    arr = (C.POINTER(capi.PhImageTransLayer) * max(len(sets), 1))(*[C.cast(s, C.POINTER(capi.PhImageTransLayer)) for s in sets])
    rc = capi.lib().ph_compose_up_transition_multi(None, capi.QUEUE_PROCESS, jobs, n, arr, n_out, outs, ow, oh)
    return rc, capi.lib().ph_last_error(None).decode()


def test_good_arguments_get_as_far_as_the_missing_context():
    for jobs in (1, 2, 4):
        rc, text = answer(good_layers(jobs), good_outputs(jobs))
        assert rc == -1 and "ctx is NULL" in text, text  # every check of the arguments passed
    rc, text = answer(good_layers(), good_outputs(), oh=0)
    assert rc == -1 and "ctx is NULL" in text, text


def broken(change, jobs=1, fmts=("v210", "rgba8"), **kw):
    sets, outs = good_layers(jobs), good_outputs(jobs, fmts)
    change(sets, outs)
    rc, text = answer(sets, outs, n_out=len(fmts), **kw)
    assert rc == -1, text  # PH_E_INVALID
    assert "ph_compose_up_transition_multi" in text and "ctx is NULL" not in text, text
    return text


def test_every_refusal_names_its_cause():
    def setter(path, value, job=0):
        def change(sets, outs):
            obj = sets[job]
            *walk, last = path
            for step in walk:
                obj = obj[step] if isinstance(step, int) else getattr(obj, step)
            setattr(obj, last, value)
        return change

    assert "transition 3 is not" in broken(setter((0, "transition"), 3))
    assert "transition -1 is not" in broken(setter((1, "transition"), -1))
    assert "layer 0: the incoming image is missing" in broken(setter((0, "incoming", "data"), None))  # a NULL device pointer
    assert "layer 1: the mask image is missing" in broken(setter((1, "mask", "data"), None))
    assert "layer 1: the src image is missing" in broken(setter((1, "src", "data"), None))
    assert "layer 1: the incoming image is missing" in broken(setter((1, "incoming", "width"), 0))
    assert "job 1 layer 0: the incoming image is missing" in broken(setter((0, "incoming", "data"), None, job=1), jobs=2)
    assert "job 1 layer 1: another transition than job 0" in broken(setter((1, "transition"), capi.TRANSITION_DISSOLVE, job=1), jobs=2)
    assert "job 1 layer 0: the incoming image differs from job 0's" in broken(setter((0, "incoming", "width"), 48, job=1), jobs=2)
    assert "job 1 layer 1: the mask image differs from job 0's" in broken(lambda s, o: image(s[1][1].mask, six=(0.5, 0, 0, 0, 1, 0)), jobs=2)
    assert "job 1 layer 0: the src image differs from job 0's" in broken(setter((0, "src", "height"), 12, job=1), jobs=2)
    assert "another image format" in broken(setter((1, "mask", "format"), capi.IMG_RGBA_F32))
    assert "image format 7" in broken(setter((0, "src", "format"), 7))
    # a placement of any present image that does not qualify: rotated, mirrored, reduced, 2x down for a field's rows
    for six in ((1, 0.1, 0, -0.1, 1, 0), (-1, 0, 0, 0, 1, 0), (3, 0, 0, 0, 1, 0)):
        for which in ((0, "src"), (0, "incoming"), (1, "incoming"), (1, "mask")):
            assert "must be enlarged" in broken(lambda s, o: image(getattr(s[0][which[0]], which[1]), six=six))
    assert "must be enlarged" in broken(lambda s, o: (image(s[0][1].mask, h=27), [setattr(x, "interlace", 1) for x in o]))
    assert "must be enlarged" not in broken(lambda s, o: (image(s[0][0].mask, h=27, six=(1, 0.1, 0, 0, 1, 0)), setattr(o[0], "format", 99)))  # a dissolve's mask is not looked at
    # everything ph_compose_up_write_multi refuses, per job and output
    rc, text = answer(good_layers(), good_outputs(), jobs=5)
    assert rc == -1 and "1..4 jobs (5)" in text
    rc, text = answer(good_layers(), good_outputs(), n_out=5)
    assert rc == -1 and "1..4 outputs (5)" in text
    rc, text = answer(good_layers(), good_outputs(), n=9)
    assert rc == -1 and "1..8 layers" in text
    rc, text = answer(good_layers(), good_outputs(), ow=191)
    assert rc == -1 and "width 191 is odd" in text
    assert "does not write yuv420p10 frames" in broken(lambda s, o: setattr(o[1], "format", capi.FORMATS["yuv420p10"]))
    assert "does not write p010 frames" in broken(lambda s, o: setattr(o[0], "format", capi.FORMATS["p010"]))
    assert "format 99 is not a PH_FMT_" in broken(lambda s, o: setattr(o[1], "format", 99))
    assert "output 1: NULL argument" in broken(lambda s, o: o[1].planes.__setitem__(0, None))
    assert "matrix is missing" in broken(lambda s, o: setattr(o[0], "wr_col_matrix12", None))
    assert "interlace must be 0, 1 or 3" in broken(lambda s, o: setattr(o[1], "interlace", 2))
    assert "name the same plane" in broken(lambda s, o: o[1].planes.__setitem__(0, o[0].planes[0]))
    assert "output 0 of job 1 differs from job 0's" in broken(lambda s, o: setattr(o[2], "interlace", 1), jobs=2)
    assert "needs its three planes" in broken(lambda s, o: o[1].planes.__setitem__(2, None), fmts=("rgba8", "yuv422p8"))
    assert "multiple of 8" in broken(lambda s, o: None, fmts=("rgba8", "yuv422p8"), ow=100, oh=52)
    assert "even height" in broken(lambda s, o: None, fmts=("rgba8", "nv12"), oh=53)
    # a v210 output whose lines end in a tail quad, with a layer in a transition
    assert "tail quad" in broken(lambda s, o: None, ow=100, oh=52)
    assert "tail quad" not in broken(lambda s, o: setattr(s[0][0], "transition", 3), fmts=("rgba8", "bgra8"), ow=100, oh=52)
