"""The context option "fused_fields" without a GPU: the header documents it and the debug entry, the binding exports the entry, a field
quad's place in the frame - ph_debug_fused_field_quad, the inline function the field kernels use (phaneron_amd/csrc/ph_fused_field.h), run
on the host - against plain integer arithmetic for every quad of the small shapes, and node/defer.js sets the library option once in front
of the first launch (node/test/fused_fields_check.js, against a counting stand-in for the addon)."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from phaneron_amd import capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = [(48, 2), (96, 9), (384, 12), (1920, 16), (3840, 2160)]


def header():
    return re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "phaneron_hip.h")).read())


def comment_above(text, declaration):
    at = text.index(declaration)
    return text[text.rindex("/*", 0, at):at]


def test_the_header_lists_the_option_and_declares_the_debug_entry():
    text = header()
    at = text.index('"fused_fields" (default 0)')
    assert at < text.index("int ph_ctx_set_option(")
    item = text[at:text.index('"clip_batch" (default 0)')]
    for said in ("PH_E_INVALID", "The same bytes", "fused_v210_field_multi", "mixed field modes", "transition", "image_out"):
        assert said in item, said
    assert "int ph_debug_fused_field_quad(uint32_t width, uint32_t height, int interlace, uint32_t g, uint32_t *f, uint32_t *line, uint32_t *col);" in text
    assert "The whole frame is always composed; a field output (interlace 1 / 3) stores the quads of its lines" not in text


@pytest.mark.parametrize("declaration,name", [("int ph_fused_v210_combine_multi(", "fused_v210_field_multi x<outputs>f<interlace>"),
                                               ("int ph_fused_v210_combine_multi_batch(", "fused_v210_field_multi x<outputs>j<jobs>f<interlace>")])
def test_the_header_says_what_the_option_does_to_each_entry(declaration, name):
    doc = comment_above(header(), declaration)
    assert '"fused_fields"' in doc and name in doc and "same bytes" in doc


def test_the_binding_exports_the_entry_and_the_abi_stays_8():
    assert "ph_debug_fused_field_quad" in capi.EXPORTS
    l = capi.lib()
    assert l.ph_abi_version() == 8
    assert hasattr(l, "ph_debug_fused_field_quad")


def test_the_option_needs_a_context():
    l = capi.lib()
    assert l.ph_ctx_set_option(None, b"fused_fields", 1) == -1
    assert "NULL" in l.ph_last_error(None).decode()


def expected(width, height, interlace, g):
    """plain integer arithmetic (numpy int64, g an array): the field's line g // qpl is frame line 2 * that + (0 | 1)"""
    qpl = width // 6
    g = np.asarray(g, np.int64)
    fl, col = g // qpl, g % qpl
    line = 2 * fl + (1 if interlace == 3 else 0)
    return line * qpl + col, line, col


def quads_to_try(width, height):
    qpl, lines = width // 6, height // 2
    n = qpl * lines
    if n <= 4096:
        return np.arange(n, dtype=np.int64)
    # every line's first and last quad, and 10^4 seeded ones
    starts = np.arange(lines, dtype=np.int64) * qpl
    r = np.random.default_rng(20261021)
    return np.unique(np.concatenate([starts, starts + qpl - 1, r.integers(0, n, 10000)]))


@pytest.mark.parametrize("interlace", [1, 3])
@pytest.mark.parametrize("width,height", SHAPES)
def test_a_field_quads_place_in_the_frame(width, height, interlace):
    fn = capi.lib().ph_debug_fused_field_quad
    gs = quads_to_try(width, height)
    if width * height <= 1920 * 16:
        assert gs.size == (width // 6) * (height // 2), "every quad of the small shapes"
    want_f, want_line, want_col = expected(width, height, interlace, gs)
    f, line, col = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    got = np.empty((gs.size, 3), np.int64)
    for i, g in enumerate(gs):
        assert fn(width, height, interlace, int(g), ctypes.byref(f), ctypes.byref(line), ctypes.byref(col)) == 0, g
        got[i] = f.value, line.value, col.value
    assert np.array_equal(got[:, 0], want_f) and np.array_equal(got[:, 1], want_line) and np.array_equal(got[:, 2], want_col)
    assert (got[:, 1] % 2 == (1 if interlace == 3 else 0)).all(), "a line of the other parity"
    assert (got[:, 1] < 2 * (height // 2)).all(), "a line the field does not have"
    assert (got[:, 2] < width // 6).all() and (got[:, 0] < (width // 6) * height).all()
    # the binding's wrapper, and outputs that are not asked for
    assert capi.debug_fused_field_quad(width, height, interlace, int(gs[-1])) == (int(want_f[-1]), int(want_line[-1]), int(want_col[-1]))
    assert fn(width, height, interlace, 0, None, None, None) == 0


def test_the_debug_entry_refuses():
    fn = capi.lib().ph_debug_fused_field_quad
    f = ctypes.c_uint32(77)
    for args, needle in [((100, 8, 1, 0), "width 100"), ((0, 8, 1, 0), "width 0"), ((96, 8, 0, 0), "interlace 0"), ((96, 8, 2, 0), "interlace 2"),
                         ((96, 8, 1, 16 * 4), "outside the field"), ((96, 9, 3, 16 * 4), "outside the field"), ((96, 1, 1, 0), "outside the field")]:
        assert fn(*args, ctypes.byref(f), None, None) == -1, args
        assert needle in capi.lib().ph_last_error(None).decode(), (args, capi.lib().ph_last_error(None))
        assert f.value == 77, "a refused call wrote"
    with pytest.raises(capi.PhaneronError, match="ph_debug_fused_field_quad"):
        capi.debug_fused_field_quad(100, 8, 1, 0)


def test_the_binding_declares_fused_fields():
    text = open(os.path.join(ROOT, "node", "index.d.ts")).read()
    assert "fusedFields?: boolean" in text and "`fusedFields` (default false; PHANERON_FUSED_FIELDS=1)" in text and "`fused_fields`" in text
    assert "params.fusedFields" in open(os.path.join(ROOT, "node", "index.js")).read()
    assert "'fused_fields', 1" in open(os.path.join(ROOT, "node", "defer.js")).read()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_sets_the_option_once_before_the_first_launch():
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "node", "test", "fused_fields_check.js")], capture_output=True, text=True, timeout=120)
    assert r.stdout.strip(), r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 58  # (4 of the constructor, 18 + 17 + 17 per option value, 2 across them)
