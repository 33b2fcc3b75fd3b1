"""GPU tests (-m gpu): every kernel family of the typed C ABI run between guard bands (tests/guard.py).

The callers' contract is the sizes of include/phaneron_hip.h - ph_pack_plane_bytes, ph_v210_pitch_bytes(w) * h, w * h * 16, w * h * 12 - and
a kernel that touches a byte more is wrong even when the picture is right.  Here every device buffer a call receives - sources, every
plane, masks, destinations, colour matrices, gamut blocks, flip vectors, device matrices and the gamma tables (registered, so the LDS
routes stay what they are) - sits between guards: a store outside damages a guard and guard.check() names it; a load outside brings a
NaN / code 1023 / opaque white where the border is transparent black into a result that is compared bit for bit with the oracle, as
the existing tests of the entry point compare it (their case builders and oracle chains are reused).

How a buffer cannot slip past: the fixture `gb` replaces hip_harness.dev, torch.zeros(device="cuda") and the cached colour parameters
with guarded ones for the test, and hip_harness.ctx() with a proxy that refuses any tensor that is not a guarded payload.  Each test
also counts the sources and destinations its cases have, from the cases' structure, and guard.check() must have seen exactly those.
Widths sit on both sides of each kernel's own unit (48-pixel v210 blocks, 8-sample octets, 58 / 250-column de-interlacer strips,
126-column wave steps, 192-pixel chunks); heights are tiny.  Nothing here provokes a fault: every access the controls at the end make
on purpose stays inside an allocation the test made."""
import numpy as np
import pytest

import cases
import frames
import guard
import packfmt
from oracle import orc

pytestmark = pytest.mark.gpu

H_ALL = [1, 2, 3, 5, 9, 17]
POISON_WORDS = (0xA5A5A5A5, 0x5A5A5A5A, 0x2AAAAAAA, cases.POISON)  # what the case builders pre-fill destinations with


def is_poison(a):
    """a destination as the reused case builders make them: one poison value throughout"""
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if b.size and b.size % 4 == 0:
        w = b.view("<u4")
        return bool((w == w[0]).all()) and int(w[0]) in POISON_WORDS
    return bool(b.size) and bool((b == b[0]).all()) and int(b[0]) in (0xA5, 0x5A)


class Session:
    """the guarded stand-ins of one test and its tally; as hip_harness.ctx() it hands every call on after looking at its tensors"""

    def __init__(self, mp):
        import torch
        import hip_harness as hh
        import test_chan_multi_gpu
        import test_pack_write_multi_gpu
        guard.reset()
        self._k, self._zeros, self._luts = hh.ctx(), torch.zeros, []
        self.tag, self.want = "", [0, 0]
        mp.setattr(hh, "dev", self.dev)
        mp.setattr(hh, "ctx", lambda: self)
        mp.setattr(hh.ColourParams, "_cache", {})
        mp.setattr(test_chan_multi_gpu, "_writers", {})
        mp.setattr(test_pack_write_multi_gpu, "_tables", {})
        mp.setattr(torch, "zeros", self.zeros)

    # ---- buffers -----------------------------------------------------------------------------------------------------------------
    def _make(self, a, role, pitch=None):
        a = np.ascontiguousarray(a)
        return guard.dev(a.reshape(-1), role, pitch=pitch, label="%s %s#%d" % (self.tag, role, len(guard.live())))

    def dev(self, a):
        """hip_harness.dev for the reused runners: a poisoned array is a destination, anything else a source (the runners count neither)"""
        return self._make(a, "dst" if is_poison(a) else "src")

    def zeros(self, *size, **kw):
        if not str(kw.get("device", "")).startswith("cuda"):
            return self._zeros(*size, **kw)
        import torch
        dt = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}[kw.get("dtype", torch.float32)]
        return self._make(np.zeros(int(np.prod(size)), dt), "dst")

    def src(self, a, pitch=None):
        self.want[0] += 1
        return self._make(a, "src", pitch)

    def dst(self, a, pitch=None):
        self.want[1] += 1
        return self._make(a, "dst", pitch)

    def poisoned_f32(self, n, pitch=None):
        return self.dst(np.full(n, 0xA5A5A5A5, np.uint32).view(np.float32), pitch)

    def expect(self, src=0, dst=0):
        """the buffers a reused runner is about to make, from the case's structure"""
        self.want[0] += src
        self.want[1] += dst

    def colour(self, fn, n):
        """colour parameters through the suite's own cache (emptied for the test, so they are uploaded between guards and their tables
        registered); n: how many buffers this recipe uploads now"""
        before = len(guard.live())
        self.tag = "colour"
        got = fn()
        assert len(guard.live()) - before == n, "the recipe uploaded %d buffers, not %d" % (len(guard.live()) - before, n)
        self.want[0] += n
        return got

    # ---- hip_harness.ctx() ---------------------------------------------------------------------------------------------------------
    def _see(self, name, x):
        import torch
        if isinstance(x, torch.Tensor):
            assert guard.owner(x) is not None, "%s: %s was handed a device buffer that is not between guards" % (self.tag, name)
        elif isinstance(x, (list, tuple)):
            for y in x:
                self._see(name, y)
        elif isinstance(x, dict):
            for y in x.values():
                self._see(name, y)

    def __getattr__(self, name):
        attr = getattr(self._k, name)
        if not callable(attr):
            return attr

        def looked_at(*args, **kw):
            self._see(name, (args, kw))
            if name == "register_lut":
                self._luts.append(args[0])
            return attr(*args, **kw)
        return looked_at

    def finish(self):
        """every guard intact, and exactly the buffers the cases have were guarded"""
        n = guard.check()
        assert n == tuple(self.want), "guard.check() saw %r (sources, destinations), the cases have %r" % (n, tuple(self.want))
        assert n[1]
        return n

    def teardown(self):
        for t in self._luts:
            self._k.unregister_lut(t)
        self._k.wait()
        guard.reset()


@pytest.fixture
def gb(monkeypatch):
    s = Session(monkeypatch)
    yield s
    s.teardown()


def bits_eq(got, want, what):
    g = np.ascontiguousarray(got).reshape(-1)
    g = g.view(np.uint32 if g.dtype.itemsize == 4 else g.dtype)
    w = np.ascontiguousarray(want).reshape(-1).view(g.dtype)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d differ, first at %d" % (what, bad.size, w.size, bad[0] if bad.size else -1)


def host(t, dtype=None):
    import hip_harness as hh
    return hh.host(t, dtype)


def reader(gb, rspec="709", wspec="2020"):
    import hip_harness as hh
    return gb.colour(lambda: hh.ColourParams.reader(rspec, wspec), 3), (orc.ycbcr2rgb_matrix(rspec), orc.gamma2linear_lut(rspec), orc.rgb2rgb_matrix(rspec, wspec))


def writer(gb, wspec="2020"):
    import hip_harness as hh
    return gb.colour(lambda: hh.ColourParams.writer(wspec), 2), (orc.rgb2ycbcr_matrix(wspec), orc.linear2gamma_lut(wspec))


def v210_poison(w, h):
    return np.full(frames.v210_pitch_bytes(w) * h // 4, 0xA5A5A5A5, np.uint32)


# ---- image operators ---------------------------------------------------------------------------------------------------------------
W_IMG = [1, 3, 63, 64, 65, 249, 250, 251, 257]
IMG_SIZES = [(w, H_ALL[i % len(H_ALL)]) for i, w in enumerate(W_IMG)] + [(250, 2), (251, 3), (65, 17)]  # (the first is 1 x 1)


def test_yadif_and_yadif_pair(gb):
    for i, (w, h) in enumerate(IMG_SIZES):
        gb.tag = "yadif %dx%d" % (w, h)
        p, c, n = (frames.rgba_random(w, h, 3000 + 7 * w + h + j) for j in range(3))
        dp, dc, dn = gb.src(p, w * 16), gb.src(c, w * 16), gb.src(n, w * 16)
        tff, skip = i & 1, bool(i & 2)
        pair = [gb.poisoned_f32(w * h * 4, w * 16) for _ in range(2)]
        gb.yadif_pair(dp, dc, dn, pair[0], pair[1], w, h, tff, skip)
        for parity in (0, 1):
            out = gb.poisoned_f32(w * h * 4, w * 16)
            gb.yadif(dp, dc, dn, out, w, h, parity, tff, skip)
            want = orc.yadif(p, c, n, parity, tff, skip)
            bits_eq(host(out), want, "%s p%d t%d s%d" % (gb.tag, parity, tff, skip))
            bits_eq(host(pair[parity]), want, "%s pair p%d t%d s%d" % (gb.tag, parity, tff, skip))
    assert gb.finish() == (3 * len(IMG_SIZES), 4 * len(IMG_SIZES))


# placements that put most taps outside a tiny source: shrunk into a corner, flipped, rotated, pushed off screen
OUTSIDE = [dict(scale_x=0.2, scale_y=0.3, offset_x=0.3, offset_y=-0.3, rotate=0.1), dict(flip_h=True, scale_x=0.15, scale_y=0.15, offset_x=-0.4),
           dict(flip_v=True, rotate=0.25, scale_x=0.5, scale_y=0.1), dict(offset_x=0.9, offset_y=0.9), dict(),
           dict(rotate=0.5, flip_h=True, flip_v=True, scale_x=0.3, scale_y=0.3, anchor_x=0.2), dict(scale_x=3.0, scale_y=3.0, rotate=-0.125)]


def test_transform_and_resize(gb):
    from phaneron_amd import capi
    shapes = [(iw, ih, ow, oh, kw) for (ow, oh) in ((65, 5), (3, 2)) for (iw, ih) in ((2, 2), (5, 3)) for kw in OUTSIDE]
    shapes += [((2, 5, ow)[i % 3], (2, 3, oh)[i % 3], ow, oh, OUTSIDE[i % len(OUTSIDE)]) for i, (ow, oh) in enumerate(IMG_SIZES)]
    for k, (iw, ih, ow, oh, kw) in enumerate(shapes):
        gb.tag = "transform %d: %dx%d -> %dx%d %r" % (k, iw, ih, ow, oh, kw)
        img = frames.rgba_random(iw, ih, 7000 + k)
        m = capi.transform_matrix(ow, oh, **kw)
        out = gb.poisoned_f32(ow * oh * 4, ow * 16)
        gb.transform(gb.src(img, iw * 16), iw, ih, gb.src(m), out, ow, oh)
        bits_eq(host(out), orc.transform(img, m, ow, oh), gb.tag)
        fh, fv = bool(k & 1), bool(k & 2)
        scale, ox, oy = (0.3, 1.0, 2.5, 7.0)[k % 4], (0.0, 0.4, -0.45, 0.9)[k % 4], (0.0, -0.4, 0.45, -0.9)[(k // 4) % 4]
        gb.tag = "resize %d: %dx%d -> %dx%d scale %g offset %g %g flips %d %d" % (k, iw, ih, ow, oh, scale, ox, oy, fh, fv)
        flip = np.array([1.0 if fh else 0.0, -1.0 if fh else 1.0, 1.0 if fv else 0.0, -1.0 if fv else 1.0], np.float32)
        out = gb.poisoned_f32(ow * oh * 4, ow * 16)
        gb.resize(gb.src(img, iw * 16), iw, ih, scale, ox, oy, gb.src(flip), out, ow, oh)
        bits_eq(host(out), orc.resize(img, scale, ox, oy, fh, fv, ow, oh), gb.tag)
    assert gb.finish() == (4 * len(shapes), 2 * len(shapes))


def test_combine_transitions_mixer_and_wipe(gb):
    for i, (w, h) in enumerate(IMG_SIZES):
        imgs = [frames.rgba_random(w, h, 7500 + 11 * i + j, -0.05, 1.05) for j in range(8)]
        gb.tag = "layers of %dx%d" % (w, h)
        d = [gb.src(x, w * 16) for x in imgs]
        mask = gb.src(frames.mask_ramp(w, h) if i & 1 else imgs[7], w * 16)
        mask_h = frames.mask_ramp(w, h) if i & 1 else imgs[7]
        mix = (0.0, 0.3, 1.0)[i % 3]
        for what, call, want in (
                ("combine 2", lambda o: gb.combine(d[:2], o, w, h), lambda: orc.combine(imgs[:2])),
                ("combine 8", lambda o: gb.combine(d, o, w, h), lambda: orc.combine(imgs)),
                ("dissolve", lambda o: gb.transition_dissolve(d[0], d[1], mix, o, w, h), lambda: orc.transition_dissolve(imgs[0], imgs[1], mix)),
                ("transition wipe", lambda o: gb.transition_wipe(d[2], d[3], mask, o, w, h), lambda: orc.transition_wipe(imgs[2], imgs[3], mask_h)),
                ("mixer", lambda o: gb.mixer(d[4], d[5], mix, o, w, h), lambda: orc.mixer(imgs[4], imgs[5], mix)),
                ("wipe", lambda o: gb.wipe(d[6], d[5], 0.4, o, w, h), lambda: orc.wipe(imgs[6], imgs[5], 0.4))):
            gb.tag = "%s %dx%d" % (what, w, h)
            out = gb.poisoned_f32(w * h * 4, w * 16)
            call(out)
            bits_eq(host(out), want(), gb.tag)
    assert gb.finish() == (9 * len(IMG_SIZES), 6 * len(IMG_SIZES))


def test_image_unpack_rgb_in_place(gb):
    """the one buffer is source and destination: w * h * 12 bytes of packed RGB at its start, sized w * h * 16, guards on both sides"""
    for w, h in IMG_SIZES:
        gb.tag = "rgb_unpack %dx%d" % (w, h)
        rgb = frames.uniform_f32(w * h * 3, 7700 + w, -0.05, 1.05)
        buf = gb.dst(np.concatenate([rgb, np.full(w * h, 0xA5A5A5A5, np.uint32).view(np.float32)]), w * 16)
        gb.image_unpack_rgb(buf, w, h)
        want = np.concatenate([rgb.reshape(-1, 3), np.ones((w * h, 1), np.float32)], axis=1)
        bits_eq(host(buf), want, gb.tag)
    assert gb.finish() == (0, len(IMG_SIZES))


# ---- v210 --------------------------------------------------------------------------------------------------------------------------
W_V210 = [2, 6, 46, 48, 50, 94, 96, 98]


def test_v210_read_batch_and_write(gb):
    (cm, lut, gm), rd_o = reader(gb)
    (wcm, wlut), wr_o = writer(gb)
    n_src, n_dst = 5, 0
    for i, w in enumerate(W_V210):
        for h in (H_ALL[i % 6], H_ALL[(i + 3) % 6]):
            gb.tag = "v210_read %dx%d" % (w, h)
            pitch = frames.v210_pitch_bytes(w)
            words = [frames.v210_random(w, h, 5000 + w + 100 * j, legal=bool((i + j) & 1)) for j in range(3)]
            d = [gb.src(x, pitch) for x in words]
            outs = [gb.poisoned_f32(w * h * 4, w * 16) for _ in range(4)]
            gb.v210_read(d[0], outs[3], w, h, cm, lut, gm)
            gb.v210_read_batch(d, outs[:3], w, h, cm, lut, gm)
            n_src, n_dst = n_src + 3, n_dst + 4
            for j in range(3):
                bits_eq(host(outs[j]), orc.v210_read(words[j], w, h, *rd_o), "%s, frame %d of a batch" % (gb.tag, j))
            bits_eq(host(outs[3]), orc.v210_read(words[0], w, h, *rd_o), gb.tag)
        # (the reference's writer overlaps the lines of a frame whose width is no multiple of 48 - test_hip_sweep.py: single lines there)
        for h in ((1,) if w % 48 else (1, 2, 3, 5, 9, 17)):
            for il in ((0,) if h < 2 else (0, 1, 3)):
                gb.tag = "v210_write %dx%d il%d" % (w, h, il)
                rgba = frames.rgba_random(w, h, 6000 + w + il, -0.1, 1.1)
                o = gb.dst(v210_poison(w, h), frames.v210_pitch_bytes(w))
                gb.v210_write(gb.src(rgba, w * 16), o, w, h, il, wcm, wlut)
                n_src, n_dst = n_src + 1, n_dst + 1
                bits_eq(host(o, np.uint32), orc.v210_write(rgba, w, h, il, *wr_o, out=v210_poison(w, h)), gb.tag)
    assert gb.finish() == (n_src, n_dst)


# ---- the pack formats ----------------------------------------------------------------------------------------------------------------
W_PLANAR = [2, 6, 8, 10, 14, 16, 18, 70, 250, 258]
W_RGB8 = [1, 3, 63, 64, 65]


def plane_pitches(f, w, h):
    """bytes per row of each plane (for the guards' size): a plane's bytes over the rows it has"""
    return [max(n // max(h, 1), 1) for n in f.plane_bytes(w, h)]


@pytest.mark.parametrize("fmt", packfmt.STANDALONE)
def test_pack_formats_between_guards(gb, fmt):
    import hip_harness as hh
    f = packfmt.get(fmt)
    ranged = f.code_range is not None
    cm, lut, gm = gb.colour(lambda: hh.ColourParams.fmt_reader(fmt, "709", "2020"), 4 + ranged)
    wcm, wlut = gb.colour(lambda: hh.ColourParams.fmt_writer(fmt, "2020"), 2 + ranged)
    rd_o, wr_o = f.oracle_reader("709", "2020"), f.oracle_writer("2020")
    n_src, n_dst = 6 + 2 * ranged, 0
    widths = W_RGB8 if fmt in packfmt.RGB8 else W_PLANAR
    sizes = [f.even(w, H_ALL[(i + k) % 6]) for i, w in enumerate(widths) for k in (0, 2)]
    assert len(set(sizes)) == len(sizes) and (f.v420 or any(h & 1 for _, h in sizes))
    for w, h in sizes:
        gb.tag = "%s read %dx%d" % (fmt, w, h)
        pitches = plane_pitches(f, w, h)
        planes = [f.random_planes(w, h, 9000 + w + 50 * j) for j in range(3)]
        d = [[gb.src(p, pt) for p, pt in zip(ps, pitches)] for ps in planes]
        outs = [gb.poisoned_f32(w * h * 4, w * 16) for _ in range(4)]
        gb.pack_read(fmt, d[0], outs[3], w, h, cm, lut, gm)
        gb.pack_read_batch(fmt, d, outs[:3], w, h, cm, lut, gm)
        n_src, n_dst = n_src + 3 * len(pitches), n_dst + 4
        for j in range(3):
            bits_eq(host(outs[j]), f.oracle_read(planes[j], w, h, *rd_o), "%s, frame %d of a batch" % (gb.tag, j))
        bits_eq(host(outs[3]), f.oracle_read(planes[0], w, h, *rd_o), gb.tag)
        for il in ((0,) if h < 2 else (0, 1, 3)):
            gb.tag = "%s write %dx%d il%d" % (fmt, w, h, il)
            rgba = frames.rgba_random(w, h, 9500 + w + il, -0.1, 1.1)
            dst = f.poisoned(w, h)
            dp = [gb.dst(p, pt) for p, pt in zip(dst, pitches)]
            gb.pack_write(fmt, gb.src(rgba, w * 16), dp, w, h, il, wcm, wlut)
            n_src, n_dst = n_src + 1, n_dst + len(dp)
            for pl, (g, wnt) in enumerate(zip(dp, f.oracle_write(rgba, w, h, il, *wr_o, dst))):
                bits_eq(host(g), wnt, "%s plane %d" % (gb.tag, pl))
    assert gb.finish() == (n_src, n_dst)


W_MULTI = [8, 48, 56, 96, 104]


def test_pack_write_multi_between_guards(gb):
    """1, 2 and 4 outputs, every format, every field mode - through test_pack_write_multi_gpu.run (the call, the separate ph_pack_write calls
    and the oracle over equally poisoned planes)"""
    import hip_harness as hh
    import test_pack_write_multi_gpu as t
    uploaded = set()

    def prime(fmts):  # the outputs' writers, uploaded once each
        for fmt in fmts:
            if fmt not in uploaded:
                ranged = packfmt.get(fmt).code_range is not None
                gb.colour(lambda: hh.ColourParams.fmt_writer(fmt, "709"), ranged + (2 if not uploaded else 0))
                uploaded.add(fmt)
    groups = [(f,) for f in t.ALL] + t.PAIRS + [t.QUAD_10, t.QUAD_8]
    seen = set()
    for i, fmts in enumerate(groups):
        w, h = W_MULTI[i % len(W_MULTI)], (2, 3, 5, 9, 17)[i % 5]
        for fmt in fmts:
            w, h = packfmt.get(fmt).even(w, h)
        modes = [(0, 1, 3, 1), (1, 1, 1, 1), (3, 3, 3, 3), (0, 0, 0, 0)]
        ils = modes[i % 4][:len(fmts)]
        prime(fmts)
        gb.tag = "pack_write_multi %r %dx%d fields %r" % (fmts, w, h, ils)
        outs = [t.O(fmt, il) for fmt, il in zip(fmts, ils)]
        assert t.defined(outs, w, h) == outs
        t.run(w, h, outs, t.image(w, h, 40 + i))
        gb.expect(src=1, dst=2 * sum(len(packfmt.get(fmt).plane_bytes(w, h)) for fmt in fmts))
        seen |= {(fmt, il) for fmt, il in zip(fmts, ils)}
    assert {fmt for fmt, _ in seen} == set(packfmt.NAMES) and {il for _, il in seen} == {0, 1, 3} and {len(g) for g in groups} == {1, 2, 4}
    gb.finish()


# ---- the de-interlacing reader ---------------------------------------------------------------------------------------------------------
W_DEINT = [2, 6, 56, 58, 60, 114, 116, 118]


@pytest.mark.parametrize("fmt", packfmt.names(deint=True))
def test_deinterlacing_reader_between_guards(gb, fmt):
    """ph_yadif_pair_packed with RGBA and packed-RGB fields, 1 and 3 sources: == the format's reader on the three window frames, then yadif"""
    from phaneron_amd import capi
    f = packfmt.get(fmt)
    (cm, lut, gm), _ = reader(gb)
    n_src, n_dst = 3, 0
    if f.code_range != packfmt.get("v210").code_range:  # an 8-bit packing: its own Loader matrix
        cm = gb.src(capi.ycbcr2rgb_matrix("709", *f.code_range))
        n_src += 1
    rd_o = f.oracle_reader("709", "2020")
    heights = [2, 4, 6, 10, 18] + ([] if f.v420 else [3, 5, 1])
    for i, w0 in enumerate(W_DEINT * 2):
        w = max(6, int(round(w0 / 6.0)) * 6) if fmt == "v210" else w0  # (v210 windows: whole quads - the nearest width the entry point takes)
        h = heights[(i + i // len(W_DEINT)) % len(heights)]
        n, rgb = [(1, False), (3, True), (1, True), (3, False)][(i + i // len(W_DEINT)) % 4]
        tff, skip = i & 1, i % 3 == 0
        gb.tag = "%s yadif pair %dx%d x%d %s t%d s%d" % (fmt, w, h, n, "rgb" if rgb else "rgba", tff, skip)
        pitches, px = plane_pitches(f, w, h), 3 if rgb else 4
        wins = [[f.random_planes(w, h, 9100 + 31 * l + 7 * j + w + i) for j in range(3)] for l in range(n)]
        dwin = [[[gb.src(p, pt) for p, pt in zip(fr, pitches)] for fr in win] for win in wins]
        outs = [[gb.poisoned_f32(w * h * px, w * 4 * px) for _ in range(2)] for _ in range(n)]
        n_src, n_dst = n_src + 3 * n * len(pitches), n_dst + 2 * n
        one = (lambda fr: fr[0]) if fmt == "v210" else tuple
        gb.v210_yadif_pair([(one(dwin[l][0]), one(dwin[l][1]), one(dwin[l][2]), outs[l][0], outs[l][1]) for l in range(n)], w, h, tff, skip, cm, lut, gm,
                           rgb=rgb, packing=fmt)
        for l in range(n):
            p, c, nx = (f.oracle_read(fr, w, h, *rd_o) for fr in wins[l])
            for parity in (0, 1):
                want = orc.yadif(p, c, nx, parity, tff, skip)
                bits_eq(host(outs[l][parity]), np.ascontiguousarray(want[..., :3]) if rgb else want, "%s source %d parity %d" % (gb.tag, l, parity))
    assert gb.finish() == (n_src, n_dst)


# ---- fused and layer compositors ----------------------------------------------------------------------------------------------------------
W_COMPOSE = [48, 96, 144, 192, 240, 384]
PLACED = [dict(rotate=0.07, scale_x=0.8, scale_y=0.9), dict(scale_x=0.3, scale_y=0.3, offset_x=-0.45, offset_y=0.4), dict(scale_x=2.0, scale_y=2.0, offset_x=0.6),
          dict(offset_x=1.5, offset_y=-1.2), dict(rotate=-0.25, scale_x=1.3, scale_y=0.6, offset_y=0.5), dict(scale_x=0.5, scale_y=1.7, offset_x=0.4, offset_y=-0.55, flip_h=True)]


def test_fused_v210_combine_and_batch(gb):
    (cm, lut, gm), rd_o = reader(gb)
    (wcm, wlut), wr_o = writer(gb)
    n_src, n_dst = 5, 0
    for i, w in enumerate(W_COMPOSE):
        for h in (H_ALL[i % 6], H_ALL[(i + 2) % 6]):
            n = 2 + (i + h) % 3
            gb.tag = "fused %dx%d, %d layers" % (w, h, n)
            pitch = frames.v210_pitch_bytes(w)
            jobs = [[frames.v210_random(w, h, frames.layer_seed(i + 10 * j, l), legal=bool(l & 1)) for l in range(n)] for j in range(3)]
            d = [[gb.src(x, pitch) for x in job] for job in jobs]
            outs = [gb.dst(v210_poison(w, h), pitch) for _ in range(3)]
            gb.fused_v210_combine(d[0], outs[0], w, h, cm, lut, gm, wcm, wlut)
            gb.fused_v210_combine_batch(d[1:], outs[1:], w, h, cm, lut, gm, wcm, wlut)
            n_src, n_dst = n_src + 3 * n, n_dst + 3
            for j in range(3):
                bits_eq(host(outs[j], np.uint32), orc.pipeline_v210_combine(jobs[j], w, h, rd_o[0], rd_o[1], rd_o[2], wr_o[0], wr_o[1]), "%s, job %d" % (gb.tag, j))
    assert gb.finish() == (n_src, n_dst)


def test_compose_write_and_compose_wipe_write(gb):
    from phaneron_amd import capi
    gb.set_option("lds_lut", True)
    (wcm, wlut), wr_o = writer(gb, "709")
    n_src, n_dst, refused = 2, 0, 0
    for i, ow in enumerate(W_COMPOSE):
        for oh, il in (((2, 3, 5, 9, 17)[i % 5], (0, 1, 3)[i % 3]), ((9, 17, 2, 3, 5)[i % 5], (1, 3, 0)[i % 3])):
            gb.tag = "compose %dx%d il%d" % (ow, oh, il)
            specs = [(2, 2, PLACED[i % 6]), (5, 3, PLACED[(i + 1) % 6]), (63, 7, PLACED[(i + 2) % 6]), (ow, oh, None), (5, 3, PLACED[(i + 3) % 6]), (ow, oh, PLACED[(i + 4) % 6])]
            imgs = [frames.rgba_random(w, h, 8000 + 10 * i + j + oh) for j, (w, h, _) in enumerate(specs)]
            mats = [None if kw is None else capi.transform_matrix(ow, oh, **kw) for (_, _, kw) in specs]
            pitch = frames.v210_pitch_bytes(ow)
            layers = [(gb.src(im, w * 16), w, h, None if m is None else gb.src(m)) for im, (w, h, _), m in zip(imgs, specs, mats)]
            out = gb.dst(v210_poison(ow, oh), pitch)
            gb.compose_write_v210(layers, out, ow, oh, il, wcm, wlut)
            n_src, n_dst = n_src + 11, n_dst + 1
            xf = [im if m is None else orc.transform(im, m, ow, oh) for im, m in zip(imgs, mats)]
            bits_eq(host(out, np.uint32), orc.v210_write(orc.combine(xf), ow, oh, il, *wr_o, out=v210_poison(ow, oh)), gb.tag)
            # wipes inside: on a sampled and on the 1:1 layer
            gb.tag = "compose with wipes %dx%d il%d" % (ow, oh, il)
            incoming = {j: frames.rgba_random(ow, oh, 8900 + 10 * i + j, -0.05, 1.05) for j in (1, 3)}
            masks = {j: frames.rgba_random(ow, oh, 8950 + 10 * i + j) for j in (1, 3)}
            dw = [(gb.src(incoming[j], ow * 16), gb.src(masks[j], ow * 16)) if j in incoming else None for j in range(len(layers))]
            out = gb.dst(v210_poison(ow, oh), pitch)
            n_src, n_dst = n_src + 4, n_dst + 1
            if ow % 192:  # the entry point takes whole 192-pixel chunks: a refusal, and nothing written
                with pytest.raises(capi.PhaneronError, match="192"):
                    gb.compose_wipe_write_v210(layers, dw, out, ow, oh, il, wcm, wlut)
                assert (host(out, np.uint32) == 0xA5A5A5A5).all(), gb.tag
                refused += 1
                continue
            gb.compose_wipe_write_v210(layers, dw, out, ow, oh, il, wcm, wlut)
            xw = [orc.transition_wipe(x, incoming[j], masks[j]) if j in incoming else x for j, x in enumerate(xf)]
            bits_eq(host(out, np.uint32), orc.v210_write(orc.combine(xw), ow, oh, il, *wr_o, out=v210_poison(ow, oh)), gb.tag)
    assert refused == 8
    assert gb.finish() == (n_src, n_dst)


# ---- the 2 x 2-block compositor ----------------------------------------------------------------------------------------------------------
W_UP = [2, 4, 124, 126, 128, 250, 252, 254]
UP_SOURCES = [(3, 3), (63, 5), (125, 9)]


def up_layers(ow, oh, i, factor, rgb, sets=1):
    """two layers of odd sizes enlarged `factor` times (the second partly off screen): per set [(h x w x 4 image, matrix)]"""
    from phaneron_amd import capi
    from test_up_gpu import opaque
    mk = opaque if rgb else (lambda w, h, s: frames.rgba_random(w, h, s, -0.05, 1.05).reshape(h, w, 4))
    out = [[] for _ in range(sets)]
    for l in range(2):
        sw, sh = UP_SOURCES[(i + l) % 3]
        kw = dict(scale_x=factor * sw / ow, scale_y=factor * sh / oh)
        if l:
            kw.update(offset_x=(0.45, -0.55)[i & 1], offset_y=(-0.5, 0.4)[(i >> 1) & 1])
        mat = capi.transform_matrix(ow, oh, **kw)
        for s in range(sets):
            out[s].append((mk(sw, sh, 300 + 10 * i + l + 100 * s), mat))
    return out


def up_device(gb, layers, rgb):
    return [(gb.src((np.ascontiguousarray(img[..., :3]) if rgb else img), img.shape[1] * (12 if rgb else 16)), img.shape[1], img.shape[0], mat) for img, mat in layers]


def up_oracle(layers, ow, oh, il, wr_o):
    placed = [orc.transform(img, mat, ow, oh) for img, mat in layers]
    return orc.v210_write(orc.combine(placed), ow, oh, il, *wr_o, out=v210_poison(ow, oh))


def test_compose_up_write_v210_pair_and_batch(gb):
    (wcm, wlut), wr_o = writer(gb)
    n_src, n_dst = 2, 0
    for i, ow in enumerate(W_UP):
        for factor, oh, il in ((2.0, (2, 3, 5, 9, 17)[i % 5], 0), (3.7, (9, 17, 2, 3, 5)[i % 5], (1, 3, 0)[i % 3])):
            rgb = bool((i + (factor > 2)) & 1)
            gb.tag = "compose_up %dx%d x%g il%d %s" % (ow, oh, factor, il, "rgb" if rgb else "rgba")
            sets = up_layers(ow, oh, i, factor, rgb, 6)
            d = [up_device(gb, s, rgb) for s in sets]
            pitch = frames.v210_pitch_bytes(ow)
            outs = [gb.dst(v210_poison(ow, oh), pitch) for _ in range(6)]
            gb.compose_up_write_v210(d[0], outs[0], ow, oh, il, wcm, wlut, rgb=rgb)
            gb.compose_up_write_v210_pair(d[1], d[2], outs[1], outs[2], ow, oh, il, wcm, wlut, rgb=rgb)
            gb.compose_up_write_v210_batch(d[3:], outs[3:], ow, oh, il, wcm, wlut, rgb=rgb)
            n_src, n_dst = n_src + 12, n_dst + 6
            for j in range(6):
                bits_eq(host(outs[j], np.uint32), up_oracle(sets[j], ow, oh, il, wr_o), "%s, set %d" % (gb.tag, j))
    assert gb.finish() == (n_src, n_dst)


def test_compose_up_write_multi_between_guards(gb):
    """each output format once (planar frames: widths in multiples of 8, 4:2:0 ones even heights), v210 and packed RGB at every width;
    through test_up_out_gpu.check (poisoned planes, the oracle's chain ending in the format's writer)"""
    import hip_harness as hh
    import test_chan_multi_gpu as tm
    import test_up_out_gpu as tu
    gb.colour(lambda: hh.ColourParams.writer("709"), 2)
    ranged = [f for f in tu.ALL_OUT if orc.FORMAT_RANGE[f] is not None]
    for f in tu.ALL_OUT:
        gb.colour(lambda: tm.writer(f, "709"), int(f in ranged))
    planes = lambda fmts, w, h: sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
    done = set()
    for i, ow in enumerate(W_UP):
        fmts = ["v210", ("rgba8", "bgra8")[i & 1]]
        oh, il, rgb = (2, 3, 5, 9, 17)[i % 5], 0, bool(i & 1)
        groups = [fmts]
        if ow % 8 == 0:
            oh = 10
            groups += [["yuv422p10", "yuv422p8", "yuv420p", "nv12"], ["yuv420p", "v210", "bgra8"]]
        for g, fm in enumerate(groups):
            gb.tag = "compose_up_multi %dx%d %r %s" % (ow, oh, fm, "rgb" if rgb else "rgba")
            jobs = 1 + (i + g) % 2
            sets = up_layers(ow, oh, i, 2.0 if g == 0 else 3.7, rgb, jobs)
            ils = [(0, 1, 3, 0)[k] if g == 2 else 0 for k in range(len(fm))]
            tu.check(sets, ow, oh, [tm.out(f, x) for f, x in zip(fm, ils)], gb.tag, rgb)
            gb.expect(src=2 * jobs, dst=jobs * planes(fm, ow, oh))
            done |= set(fm)
    assert done == set(tu.ALL_OUT)
    gb.finish()


# ---- the channel kernel ----------------------------------------------------------------------------------------------------------------
W_CHAN = [48, 192, 200, 240]
OVER_EDGES = [dict(scale_x=0.4, scale_y=0.5, offset_x=-0.45, rotate=0.1), dict(scale_x=0.4, scale_y=0.5, offset_x=0.45, rotate=-0.2),
              dict(scale_x=0.5, scale_y=0.4, offset_y=-0.45, rotate=0.3), dict(scale_x=0.5, scale_y=0.4, offset_y=0.45, rotate=-0.05)]


def n_buffers(layers):
    """the device buffers test_chan_gpu.Src.device() makes for a layer list: a tensor per plane, and an 8-bit planar source's own matrix"""
    n = 0
    for L in layers:
        for role in ("src", "incoming", "mask"):
            s = L.get(role)
            if s is not None:
                n += (len(s.data) if s.fmt in packfmt.BY_NAME and s.fmt != "v210" else 1) + (1 if s.fmt in packfmt.BY_NAME and s.own_matrix() else 0)
    return n


def n_planes(fmts, w, h):
    return sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)


@pytest.mark.parametrize("fmt", packfmt.names(chan_source=True))
def test_channel_kernel_between_guards(gb, fmt):
    """sources of one format - the channel's size taken 1:1, smaller ones as rotated insets hanging over each of the four edges, a larger one
    shrunk, one inside a wipe over a v210 clip by an f32 mask, one inside a dissolve with an f32 image - through all five entry points; the output formats rotate over v210 + packfmt.CHAN_OUT.  A
    frame of one enlarged clip goes by the clip route (reader + 2 x 2-block compositor) and by the one kernel, as the trace says."""
    import test_chan_batch_out_gpu as tb
    import test_chan_gpu as tc
    import test_chan_multi_gpu as tm
    from phaneron_amd import capi
    f = packfmt.get(fmt)
    all_out = ["v210"] + list(packfmt.CHAN_OUT)
    gb.colour(lambda: tc.colour("709", "709"), 5)
    for o in all_out:
        gb.colour(lambda: tm.writer(o, "709"), int(orc.FORMAT_RANGE[o] is not None))
    rd_o = tc.colour("709", "709")[0]
    routes = set()
    for i, ow in enumerate(W_CHAN):
        oh = (2, 6, 10, 18)[i] if f.v420 or i & 1 else (3, 6, 9, 17)[i]
        sw, sh = f.even(max(ow // 4 // 6 * 6, 6), 4)  # (whole v210 quads)
        bw, bh = f.even(ow + 48, oh + 3)
        assert (ow, oh) == f.even(ow, oh)
        layers = [dict(src=tc.Src.random(fmt, ow, oh, 100 + ow))] + [dict(src=tc.Src.random(fmt, sw, sh, 110 + ow + e, tc.m(ow, oh, **kw))) for e, kw in enumerate(OVER_EDGES)]
        layers.append(dict(src=tc.Src.random(fmt, bw, bh, 120 + ow, tc.m(ow, oh, scale_x=0.6, scale_y=0.7, offset_x=0.1, offset_y=-0.1))))
        layers.append(dict(src=tc.Src.random("v210", ow, oh, 130 + ow, tc.m(ow, oh, **tc.PIP[1])), transition="wipe",
                           incoming=tc.Src.random(fmt, sw, sh, 131 + ow, tc.m(ow, oh, scale_x=0.5, scale_y=0.5, offset_x=-0.25, offset_y=-0.25)),
                           mask=tc.Src(frames.mask_ramp(ow, oh), ow, oh, fmt="rgba")))
        layers.append(dict(src=tc.Src.random("rgba", 20, 5, 132 + ow, tc.m(ow, oh, scale_x=0.7, scale_y=0.6, offset_x=0.3, offset_y=0.35, rotate=-0.1)), transition="dissolve", mix=1.0 / 3.0,
                           incoming=tc.Src.random(fmt, sw, sh, 133 + ow, tc.m(ow, oh, scale_x=1.5, scale_y=1.5, offset_x=0.5, offset_y=0.5))))
        plain = layers[:6]  # (no transition: what check_format composes)
        ohc = oh if oh > 4 else oh + 4  # (the clip route wants the clip enlarged in both directions)
        small = [dict(src=tc.Src.random(fmt, sw, 2, 140 + ow, tc.m(ow, ohc)))]
        nl, npl, nsm = n_buffers(layers), n_buffers(plain), n_buffers(small)
        outs = [all_out[(i + k) % len(all_out)] for k in range(3)]
        if oh & 1:  # a 4:2:0 consumer's frame of an odd height is refused, and nothing is written; the other formats take its place
            outs = [o for o in outs if not packfmt.get(o).v420] + ["rgba8"]
            gb.tag = "chan_compose %s -> yuv420p %dx%d (refused)" % (fmt, ow, oh)
            rc = tm.writer("yuv420p", "709")
            dl = tc.device_layers(plain)
            refused = [gb.dst(p) for p in tm.poisoned("yuv420p", ow, oh + 1)]
            gb.expect(src=npl)
            with pytest.raises(capi.PhaneronError, match="even height"):
                gb.chan_compose_v210(dl, refused, ow, oh, 0, *tc.colour("709", "709")[2], rc[2], rc[3], out_fmt="yuv420p")
            assert all((host(p) == tm.POISON).all() for p in refused), gb.tag
        # ph_chan_compose_v210: frames and fields
        for il in ((0, 1, 3) if oh >= 2 else (0,)):
            gb.tag = "chan_compose_v210 %s %dx%d il%d" % (fmt, ow, oh, il)
            tc.check(layers, ow, oh, gb.tag, interlace=il, poison_dst=True)
            gb.expect(src=nl, dst=1)
        # ph_chan_compose: another consumer's frame
        for k, o in enumerate(outs):
            gb.tag = "chan_compose %s -> %s %dx%d" % (fmt, o, ow, oh)
            if o == "v210":
                tc.check(plain, ow, oh, gb.tag, poison_dst=True)
                gb.expect(src=npl, dst=1)
            else:
                tc.check_format(plain, ow, oh, o, gb.tag, interlace=(0, 1, 3)[k % 3])
                gb.expect(src=npl + int(orc.FORMAT_RANGE[o] is not None), dst=n_planes([o], ow, oh))
        # ph_chan_compose_batch: three jobs, two of them the fields of one frame
        gb.tag = "chan_compose_batch %s %dx%d" % (fmt, ow, oh)
        tc.check_batch([(layers, 0, 0), (plain, 1, 1), (layers, 3, 1)], ow, oh, gb.tag)
        gb.expect(src=2 * nl + npl, dst=4)
        # ph_chan_compose_multi (and the separate calls it must equal)
        gb.tag = "chan_compose_multi %s -> %r %dx%d" % (fmt, outs, ow, oh)
        tm.check_multi(layers, ow, oh, [tm.out(o, (0, 3, 1)[k % 3] if o != "v210" else 0) for k, o in enumerate(outs)], gb.tag)
        gb.expect(src=nl, dst=2 * n_planes(outs, ow, oh))
        # ph_chan_compose_batch_out: two jobs against the separate calls, and against the oracle
        gb.tag = "chan_compose_batch_out %s -> %r %dx%d" % (fmt, outs[:2], ow, oh)
        bo = [tm.out(o) for o in outs[:2]]
        _, planes, _ = tb.run_both([(layers, bo), (plain, bo)], ow, oh, gb.tag)
        gb.expect(src=nl + npl, dst=4 * n_planes(outs[:2], ow, oh))
        for j, ls in enumerate((layers, plain)):
            comp = tm.composite(ls, ow, oh, rd_o)
            for k, o in enumerate(bo):
                rc = tm.writer(o["fmt"], "709")
                for pl, wnt in enumerate(tm.oracle_frame(o["fmt"], comp, ow, oh, 0, rc[0], rc[1])):
                    bits_eq(host(planes[(j, k)][pl], np.uint8), wnt, "%s: job %d output %d plane %d" % (gb.tag, j, k, pl))
        # one enlarged clip: the clip route and the one kernel
        for option in (1, 2, 0):
            gb.tag = "enlarged %s clip %dx2 on %dx%d, chan_enlarged %d" % (fmt, sw, ow, ohc, option)
            try:
                gb.set_option("chan_enlarged", option)
                route = tc.dry_route(small, ow, ohc)
                tc.check(small, ow, ohc, gb.tag, poison_dst=True)
            finally:
                gb.set_option("chan_enlarged", 1)
            gb.expect(src=2 * nsm, dst=2)
            assert route and (option != 0 or route.startswith("chan_compose_v210<")), (gb.tag, route)
            routes.add((option, route.split("+")[-1].split("<")[0], "+" in route))
    assert any(o == 0 and name == "chan_compose_v210" for o, name, _ in routes), routes
    assert (2, "compose_up_write_v210", True) in routes, routes  # the reader, then the 2 x 2-block compositor
    assert any(o == 1 and name != "chan_compose_v210" for o, name, _ in routes), routes
    gb.finish()


# ---- the controls: these tests can fail -------------------------------------------------------------------------------------------------
def test_control_a_row_too_many_is_found_in_the_after_guard(gb):
    """ph_v210_write told h + 1 rows over a destination of h rows: the source honestly has h + 1 rows, the extra row lands in the guard
    behind the destination (two rows and more wide), and check() names it"""
    (wcm, wlut), wr_o = writer(gb)
    w, h = 48, 4
    pitch = frames.v210_pitch_bytes(w)
    assert guard.guard_bytes(pitch * h, pitch) >= 2 * pitch
    rgba = frames.rgba_random(w, h + 1, 77, -0.1, 1.1)
    gb.tag = "control"
    src = gb.src(rgba, w * 16)
    out = guard.dev(v210_poison(w, h), "dst", pitch=pitch, label="the short destination")
    gb.v210_write(src, out, w, h + 1, 0, wcm, wlut)
    with pytest.raises(AssertionError, match=r"'the short destination' \(dst, %d bytes\), side after: \d+ bytes differ, first at offset 0, last at offset %d" % (pitch * h, pitch - 1)):
        guard.check()
    bits_eq(host(out, np.uint32), np.asarray(orc.v210_write(rgba, w, h + 1, 0, *wr_o)).reshape(-1)[:pitch * h // 4], "the rows inside")


def test_control_a_row_read_from_the_guard_reaches_the_result(gb):
    """ph_transform under the identity placement on a source declared h rows whose payload holds h - 1: the last row is the NaN guard, the
    result holds NaN and differs from the oracle's on the honest image"""
    from phaneron_amd import capi
    w, h = 16, 5
    img = frames.rgba_random(w, h, 78)
    m = capi.transform_matrix(w, h)
    gb.tag = "control"
    short = gb.src(img[:h - 1], w * 16)
    out = gb.poisoned_f32(w * h * 4, w * 16)
    gb.transform(short, w, h, gb.src(m), out, w, h)
    got, want = host(out).reshape(h, w, 4), orc.transform(img, m, w, h)
    assert np.isnan(got).any() and not np.isnan(want).any()
    assert not np.array_equal(got.view(np.uint32), np.asarray(want).view(np.uint32))
    assert np.array_equal(got[:h - 2].view(np.uint32), np.asarray(want)[:h - 2].view(np.uint32)), "rows whose taps stay inside the payload"
    assert gb.finish() == (2, 1)  # (a load harms no guard)
