"""Every pack format (the names of capi.FORMATS) described once for the tests: random planes, plane sizes, poisoned destinations, the
oracle's read and write, the Loader / Saver code range and the constraints a sweep has to know.  The sweeps take their format
lists from here (the lists at the end), so a new format is swept once it has a row - and test_packfmt_cpu.py fails until it has.

Planes are lists of raw uint8 arrays, as the node Buffers are (v210: one array of uint32 words).  yuv420p10 / p010 have no
reference kernel: their read is the oracle's yuv422p10 Reader on the 4:2:2 frame F' (fmt10.to_422), their write its yuv422p10
Writer followed by fmt10.from_422_write - never the library's own output."""
import numpy as np

import fmt10
import frames
from oracle import orc
from phaneron_amd import capi

POISON = 0xA5


class PackFormat:
    def __init__(self, name, v420=False, even_size=False, chan_out=True, deint=True, planar=True, via422=False, sibling8=None):
        self.name = name
        self.v420 = v420            # 4:2:0: a chroma line serves two luma lines
        self.even_size = even_size  # defined for even widths and heights only (capi.pack_plane_bytes refuses the others)
        self.chan_source = True     # the channel kernel reads it as a source (every format so far)
        self.chan_out = chan_out    # the channel kernel writes it (ph_chan_compose)
        self.deint = deint          # the de-interlacing reader takes it
        self.planar = planar        # YCbCr in planes: a file decoder's frame
        self.via422 = via422        # defined through yuv422p10 and F'
        self.sibling8 = sibling8    # the 8-bit format of the same layout (it takes the same routes)
        self.code_range = capi.FORMAT_RANGE[name]  # (numBits, lumaBlack, lumaWhite, chromaRange); None: RGB

    def __repr__(self):
        return self.name

    # ---- geometry and data ------------------------------------------------------------------------------------------------------
    def plane_bytes(self, w, h):
        return fmt10.plane_bytes(self.name, w, h) if self.via422 else frames.pack_plane_bytes(self.name, w, h)

    def even(self, w, h):
        """the nearest size at or above w x h that the format is defined for (a stand-in, so that no case of a size list is dropped)"""
        return (w + (w & 1), h + (h & 1)) if self.even_size else (w, h + (h & 1)) if self.v420 else (w, h)

    def random_planes(self, w, h, seed, legal=True):
        """yuv420p10 / p010: all 16 bits of every word in use (p010 words with non-zero low bits); yuv422p10: every 10-bit code; 8-bit
        formats: every byte; v210: legal or all codes"""
        if self.name == "v210":
            return [frames.v210_random(w, h, seed, legal=legal)]
        if self.via422:
            return fmt10.as_bytes(fmt10.random_frame(self.name, w, h, seed))
        return frames.pack_random(self.name, w, h, seed)

    def poisoned(self, w, h, value=POISON):
        if self.name == "v210":
            return [np.full(frames.v210_pitch_bytes(w) * h // 4, value * 0x01010101, np.uint32)]
        return [np.full(n, value, np.uint8) for n in self.plane_bytes(w, h)]

    # ---- the oracle ---------------------------------------------------------------------------------------------------------------
    def reader_matrix(self, spec):
        return None if self.code_range is None else orc.ycbcr2rgb_matrix(spec, *self.code_range)

    def writer_matrix(self, spec):
        return None if self.code_range is None else orc.rgb2ycbcr_matrix(spec, *self.code_range)

    def oracle_reader(self, rspec, wspec):
        return self.reader_matrix(rspec), orc.gamma2linear_lut(rspec), orc.rgb2rgb_matrix(rspec, wspec)

    def oracle_writer(self, wspec):
        return self.writer_matrix(wspec), orc.linear2gamma_lut(wspec)

    def oracle_read(self, planes, w, h, cm, lut, gm):
        """the image [h][w][4] the reference's Reader makes of the planes"""
        if self.name == "v210":
            return orc.v210_read(planes[0], w, h, cm, lut, gm)
        planes = [np.ascontiguousarray(p).view(np.uint8) for p in planes]
        if self.via422:
            f422 = fmt10.to_422(self.name, [p.view(np.uint16) for p in planes], w, h)
            return orc.pack_read("yuv422p10", fmt10.as_bytes(f422), w, h, cm, lut, gm)
        return orc.pack_read(self.name, planes, w, h, cm, lut, gm)

    def oracle_write(self, rgba, w, h, interlace, cm, lut, planes):
        """the destination planes after the reference's Writer ran over them (interlace 0 / 1 / 3); `planes` is not changed.  For the
        10-bit 4:2:0 formats only the rows the call writes come from the definition: the luma rows of fmt10.rows_written and every
        chroma row (row g from line 2g, or 2g + 1 in field mode 3) - the other luma rows keep the destination's bytes, whatever they are
        (from_422_write shifts whole planes, so it must not see them)"""
        if self.name == "v210":
            return [np.asarray(orc.v210_write(rgba, w, h, interlace, cm, lut, out=planes[0].copy())).reshape(-1)]
        planes = [np.ascontiguousarray(p).view(np.uint8) for p in planes]
        if not self.via422:
            return orc.pack_write(self.name, rgba, w, h, interlace, cm, lut, planes=[p.copy() for p in planes])
        p422 = orc.pack_write("yuv422p10", rgba, w, h, interlace, cm, lut)
        made = fmt10.as_bytes(fmt10.from_422_write(self.name, [p.view(np.uint16) for p in p422], w, h, interlace))
        out = [p.copy() for p in planes]
        line = 2 * fmt10.pitch(w)
        rows = fmt10.rows_written(h, interlace)
        out[0].reshape(h, line)[rows] = made[0].reshape(h, line)[rows]
        for i in range(1, len(out)):
            out[i][:] = made[i]
        return out

    def rows_untouched(self, h, interlace):
        """the luma rows (every plane's rows for 4:2:2 and packed formats) a write call leaves alone"""
        return np.setdiff1d(np.arange(h), fmt10.rows_written(h, interlace))


_ROWS = [
    PackFormat("v210", planar=False),
    PackFormat("yuv422p10"),
    PackFormat("yuv422p8"),
    PackFormat("yuv420p", v420=True),
    PackFormat("nv12", v420=True),
    PackFormat("rgba8", deint=False, planar=False),
    PackFormat("bgra8", deint=False, planar=False),
    PackFormat("yuv420p10", v420=True, even_size=True, chan_out=False, deint=False, via422=True, sibling8="yuv420p"),
    PackFormat("p010", v420=True, even_size=True, chan_out=False, deint=False, via422=True, sibling8="nv12"),
]
BY_NAME = {f.name: f for f in _ROWS}
NAMES = [f.name for f in _ROWS]


def get(name):
    return BY_NAME[name]


def names(**traits):
    """the formats whose traits have these values, in capi.FORMATS order"""
    return [f.name for f in _ROWS if all(getattr(f, k) == v for k, v in traits.items())]


# ---- the lists the GPU sweeps are parametrised with (test_packfmt_cpu.py: together they hold every format) -----------------------
V210 = ["v210"]                          # the v210 kernels have sweeps of their own (test_hip_sweep.py, test_chan_gpu.py)
STANDALONE = [n for n in NAMES if n != "v210"]   # ph_pack_read / ph_pack_write
PLANAR = names(planar=True)              # file decoders' frames as channel sources
PLANAR_8 = [n for n in PLANAR if BY_NAME[n].code_range[0] == 8]
PLANAR_10_420 = names(via422=True)       # the 10-bit 4:2:0 decoder frames
RGB8 = [n for n in NAMES if BY_NAME[n].code_range is None]
CLIPS = PLANAR + RGB8                    # every wire format but v210 as an enlarged clip
CHAN_OUT = [n for n in names(chan_out=True) if n != "v210"]  # ph_chan_compose's other output formats
NOT_CHAN_OUT = names(chan_out=False)
NOT_DEINT = names(deint=False)
SWEPT = V210 + STANDALONE + PLANAR + CLIPS + CHAN_OUT + NOT_CHAN_OUT
