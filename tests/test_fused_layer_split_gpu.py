"""The fused v210 kernel's layer loop is split by a layer's place in the stack (ph_kernels_lds.hip fused_layer_combine):
the FIRST layer starts the accumulators without a combine, MIDDLE layers combine, the LAST layer combines and clamps.
Every case runs ph_fused_v210_combine and compares its v210 words bit for bit with orc.pipeline_v210_combine on the
same inputs.

v210 readers emit alpha = 1, so `combine` keeps only the top layer; where a lower layer has to show, the reader table
is the one of test_chains_gpu.py with entry 0 = +Inf (a lower-layer pixel that clamps to index 0 poisons the
accumulator: fma(Inf, 0, t) = NaN, and the writer maps NaN to index 0).
"""
import numpy as np
import pytest

import frames
from oracle import orc

pytestmark = pytest.mark.gpu

WR_O = (orc.rgb2ycbcr_matrix("2020"), orc.linear2gamma_lut("2020"))


def _bits_equal(got, want, what):
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %08x vs %08x" % (what, bad.size, w.size, bad[0], g[bad[0]], w[bad[0]])


def _poison_lut():
    lut = orc.gamma2linear_lut("709").copy()
    lut[0] = np.float32(np.inf)  # entry 0 is a block of its own in the LDS form (ph_lut.h), so it stays exact
    return lut


def _fused(layers, w, h, cm, lut, gm):
    """the kernel's words and the oracle's for one stack; cm (12), lut (65536), gm (9) as the oracle takes them"""
    import torch
    import hip_harness as hh
    k = hh.ctx()
    dlut = hh.dev(lut)
    assert k.register_lut(dlut, lut) == 1, "the reader table must keep its LDS form"
    try:
        wcm, wlut = hh.ColourParams.writer("2020")
        out = torch.full((frames.v210_pitch_bytes(w) * h // 4,), 0x2AAAAAAA, dtype=torch.int32, device="cuda")
        k.fused_v210_combine([hh.dev(l) for l in layers], out, w, h, hh.dev(cm), dlut,
                             hh.dev(np.concatenate([gm, np.zeros(3, np.float32)]).astype(np.float32)), wcm, wlut)
        got = hh.host(out, np.uint32)
    finally:
        k.unregister_lut(dlut)
    return got, orc.pipeline_v210_combine(layers, w, h, cm, lut, gm, *WR_O)


def _standard():
    return orc.ycbcr2rgb_matrix("709"), orc.rgb2rgb_matrix("709", "2020")


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_split_shape(n):
    """N = 1: first is last; 2: no middle; 3: one middle layer, written out; 5: the rolled loop of pairs and the odd one behind
    it.  (N = 4 and 8 are pinned by test_chains_gpu.py.)  The poisoned table makes every layer of the stack show."""
    w, h = 1920, 32
    cm, gm = _standard()
    layers = [frames.v210_random(w, h, frames.layer_seed(9, i), legal=False) for i in range(n)]
    got, want = _fused(layers, w, h, cm, _poison_lut(), gm)
    _bits_equal(got, want, "%d layers" % n)


@pytest.mark.parametrize("n", [1, 3])
def test_two_slices_per_workgroup(n):
    """1920 x 1080 is 345 600 quads over 256 workgroups, 1 350 each: one full slice of 1 024 and a second that only some waves
    hold - the smallest frame at which the prefetch chain crosses a slice boundary and a wave skips a slice."""
    w, h = 1920, 1080
    cm, gm = _standard()
    layers = [frames.v210_random(w, h, frames.layer_seed(10, i), legal=False) for i in range(n)]
    got, want = _fused(layers, w, h, cm, _poison_lut(), gm)
    _bits_equal(got, want, "%d layers, two slices" % n)


def test_poison_per_position():
    """Index 0 of the poisoned table hit in layer 0 only, in the middle layer only, in the last layer only (N = 3): an
    all-zero-code layer where the poison is wanted (R and B clamp to index 0), mid-grey layers elsewhere.
    In the last layer the Inf is the value that is clamped: white.  Below it the Inf meets a `* 0` on its way up and arrives as
    NaN: index 0, black - from layer 0 and from the middle layer alike, so those two stacks have the same picture in the
    oracle and cannot be told apart by it; each of them differs from the unpoisoned stack and from the poisoned top."""
    w, h = 1920, 32
    cm, gm = _standard()
    lut = _poison_lut()
    grey = frames.v210_pack_codes(np.full((h, w), 512, np.uint32), np.full((h, w // 2), 512, np.uint32), np.full((h, w // 2), 512, np.uint32), w, h)
    zero = frames.v210_pack_codes(np.zeros((h, w), np.uint32), np.zeros((h, w // 2), np.uint32), np.zeros((h, w // 2), np.uint32), w, h)
    wants = []
    for where in range(3):
        layers = [zero if l == where else grey for l in range(3)]
        got, want = _fused(layers, w, h, cm, lut, gm)
        _bits_equal(got, want, "poison in layer %d" % where)
        wants.append(want)
    clean = orc.pipeline_v210_combine([grey] * 3, w, h, cm, lut, gm, *WR_O)
    for where in range(3):
        assert not np.array_equal(wants[where], clean), "the poison of layer %d does not show" % where
    assert not np.array_equal(wants[0], wants[2]) and not np.array_equal(wants[1], wants[2])


@pytest.mark.parametrize("scale", [2.0, -1.0])
def test_clamp_on_both_sides(scale):
    """N = 2 with the gamut matrix scaled: by 2.0 the accumulators leave [0, 1] above, by -1.0 below, and the clamp that
    rides on the last layer's combine has to bring both back (writer index 65535 and index 0)."""
    w, h = 1920, 32
    cm, gm = _standard()
    gm = (gm * np.float32(scale)).astype(np.float32)
    lut = orc.gamma2linear_lut("709")
    layers = [frames.v210_random(w, h, frames.layer_seed(11, i), legal=False) for i in range(2)]
    got, want = _fused(layers, w, h, cm, lut, gm)
    top = np.asarray(orc.v210_read(layers[1], w, h, cm, lut, gm)).reshape(-1, 4)[:, :3]  # what the last layer leaves in the accumulators
    if scale > 0:
        assert (top > 1.0).any(), "nothing above 1 to clamp"
    else:
        assert (top < 0.0).any(), "nothing below 0 to clamp"
    _bits_equal(got, want, "gamut x %g" % scale)


def test_non_standard_matrix():
    """a near-miss of the standard matrix shape (Cb feeds R), as test_hip_parity.py builds one: the general dot-product copy
    of the three layer bodies"""
    w, h, n = 1920, 32, 3
    cm, gm = _standard()
    cm = cm.copy()
    cm[1] = np.float32(3.0e-4)
    layers = [frames.v210_random(w, h, frames.layer_seed(12, i), legal=False) for i in range(n)]
    got, want = _fused(layers, w, h, cm, _poison_lut(), gm)
    _bits_equal(got, want, "cb in red")


def test_ragged_lines():
    """1280 x 6: lines that end in a tail quad and two cleared slots, the kernel's other instantiation"""
    w, h, n = 1280, 6, 3
    cm, gm = _standard()
    layers = [frames.v210_random(w, h, frames.layer_seed(13, i), legal=False) for i in range(n)]
    got, want = _fused(layers, w, h, cm, _poison_lut(), gm)
    _bits_equal(got, want, "ragged lines")
