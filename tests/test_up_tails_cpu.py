"""The context option "up_v210_tails" without a GPU: the header documents it and what it does to the three entries' routes, the node
binding declares `upTails`, and node/defer.js sets the library option once in front of the first launch (node/test/up_tails_check.js,
against a counting stand-in for the addon)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def header():
    return re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "phaneron_hip.h")).read())


def comment_above(text, declaration):
    """the comment that ends in front of `declaration`"""
    at = text.index(declaration)
    return text[text.rindex("/*", 0, at):at]


def test_the_header_lists_the_option():
    text = header()
    at = text.index('"up_v210_tails" (default 0)')
    assert at < text.index("int ph_ctx_set_option(")
    item = text[at:text.index("int ph_ctx_set_option(")]
    assert "PH_E_INVALID" in item and "out_width % 48 != 0" in item
    for left_alone in ("ph_compose_up_transition_multi", "ph_clip_compose_transition_multi", "ph_clip_compose_route_multi", "ph_fused_v210_", "the channel kernel"):
        assert left_alone in item, left_alone


@pytest.mark.parametrize("declaration,names", [("int ph_compose_up_write_multi(", ["compose_up_multi_t<rgb|rgba>x<outputs>j<jobs>", "alone with its table"]),
                                                ("int ph_clip_compose_multi(", ["clip_up_multi_t<rgb|rgba>x<outputs>", "compose_up_multi_t<rgba>x<outputs>j1", "n_out == 1"]),
                                                ("int ph_clip_compose_batch_out(", ["clip_up_multi_t<rgb|rgba>x<outputs>j<jobs>", "not a lone v210 output"])])
def test_the_header_says_what_the_option_does_to_each_entrys_routes(declaration, names):
    doc = comment_above(header(), declaration)
    assert '"up_v210_tails" = 1' in doc
    for n in names:
        assert n in doc, n


def test_the_binding_declares_up_tails():
    text = open(os.path.join(ROOT, "node", "index.d.ts")).read()
    assert "upTails?: boolean" in text and "`upTails` (default false" in text and "up_v210_tails" in text
    assert "params.upTails" in open(os.path.join(ROOT, "node", "index.js")).read()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_recording_context_sets_the_option_once_before_the_first_launch():
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "node", "test", "up_tails_check.js")], capture_output=True, text=True, timeout=120)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert r.returncode == 0 and res["checks"] >= 40
