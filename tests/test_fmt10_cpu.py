"""CPU-side checks of the 10-bit 4:2:0 decoder formats (yuv420p10le, p010le): their programs resolve by tag, their planes
are sized as DESIGN.md 2 defines them, odd frames are refused, and every binding knows them."""
import os
import re

import pytest

import fmt10
from phaneron_amd import capi

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
@pytest.mark.parametrize("name", ["read", "write"])
def test_tag_resolves_to_the_format_kernels(fmt, name):
    assert capi.resolve_program("phaneron:" + fmt, name) == ("%s_%s" % (fmt, name), fmt, "tag")


def test_other_tags_still_resolve_and_unknown_ones_are_refused():
    for fmt in ("v210", "yuv422p10", "yuv422p8", "yuv420p", "nv12", "rgba8", "bgra8"):
        assert capi.resolve_program("phaneron:" + fmt, "read")[1] == fmt
    for tag in ("phaneron:v211", "phaneron:p010le", "phaneron:yuv420p10le", "phaneron:p016"):
        with pytest.raises(capi.PhaneronError, match="cannot tell which pack format"):
            capi.resolve_program(tag, "read")


def test_plane_bytes():
    assert capi.pack_plane_bytes("yuv420p10", 1920, 1080) == [4147200, 1036800, 1036800]
    assert capi.pack_plane_bytes("p010", 1920, 1080) == [4147200, 2073600]
    assert capi.pack_plane_bytes("yuv420p10", 718, 480) == [691200, 172800, 172800]  # P = 720
    assert capi.pack_plane_bytes("p010", 718, 480) == [691200, 345600]
    for fmt in fmt10.FORMATS:
        for w, h in ((1920, 1080), (1280, 720), (718, 480), (3840, 2160), (2, 2)):
            assert capi.pack_plane_bytes(fmt, w, h) == fmt10.plane_bytes(fmt, w, h), (fmt, w, h)


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
def test_odd_frames_are_refused(fmt):
    for w, h in ((1920, 1081), (1919, 1080), (718, 479)):
        with pytest.raises(capi.PhaneronError, match="even width and height"):
            capi.pack_plane_bytes(fmt, w, h)
    assert capi.pack_plane_bytes("yuv420p", 1920, 1081)  # (the 8-bit 4:2:0 formats keep what they did)


def test_format_numbering_follows_the_header():
    hdr = open(os.path.join(ROOT, "include", "phaneron_hip.h")).read()
    assert re.search(r"PH_FMT_YUV420P10 = 7\b", hdr) and re.search(r"PH_FMT_P010 = 8\b", hdr)
    assert re.search(r"#define PH_SRC_YUV420P10 9\b", hdr) and re.search(r"#define PH_SRC_P010 10\b", hdr)
    assert capi.FORMATS["yuv420p10"] == 7 and capi.FORMATS["p010"] == 8
    assert capi.SRC_PLANAR["yuv420p10"] == 9 and capi.SRC_PLANAR["p010"] == 10
    assert capi.FORMAT_RANGE["yuv420p10"] == capi.FORMAT_RANGE["p010"] == (10, 64, 940, 896)  # the 10-bit Loader recipe
    assert capi.lib().ph_abi_version() == 8  # additive within 8


def test_node_binding_knows_the_formats():
    src = open(os.path.join(ROOT, "node", "index.js")).read()
    assert "'yuv420p10', 'p010']" in src
    napi = open(os.path.join(ROOT, "node", "ph_napi.c")).read()
    assert '"yuv420p10", "p010"}' in napi
