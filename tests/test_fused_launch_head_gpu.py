"""GPU tests (-m gpu) of the fused v210 kernel's launch head (phaneron_amd/csrc/ph_kernels_lds.hip, FusedLdsArgs in ph_kernels.h): the
host now computes what is uniform per launch - a workgroup's share, the reciprocal of the job division, both tables' lookup
constants - and the kernel reads the head of its arguments in one request by offset.  The shapes are the smallest at which that can
go wrong; every comparison is word for word against the oracle's chain read x n -> combine_n -> write."""
import contextlib
import functools

import numpy as np
import pytest

import frames
import luts
from oracle import orc

pytestmark = pytest.mark.gpu

RSPEC, WSPEC = "709", "2020"


def oracle_colour():
    return (orc.ycbcr2rgb_matrix(RSPEC), orc.gamma2linear_lut(RSPEC), orc.rgb2rgb_matrix(RSPEC, WSPEC),
            orc.rgb2ycbcr_matrix(WSPEC), orc.linear2gamma_lut(WSPEC))


def device_colour():
    import hip_harness as hh
    return hh.ColourParams.reader(RSPEC, WSPEC) + hh.ColourParams.writer(WSPEC)


@functools.lru_cache(maxsize=None)
def layers_of(w, h, n, job):
    """n v210 layers of job `job` (every other layer with illegal codes), and the oracle's frame for them - made once per shape"""
    layers = tuple(frames.v210_random(w, h, frames.layer_seed(70 + job, l), legal=(l % 2 == 0)) for l in range(n))
    return layers, orc.pipeline_v210_combine(list(layers), w, h, *oracle_colour())


def poisoned(w, h):
    import torch
    return torch.full((frames.v210_pitch_bytes(w) * h // 4,), 0x2AAAAAAA, dtype=torch.int32, device="cuda")


def same_words(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got %08x, want %08x" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def run_one(w, h, n, colour=None, want=None):
    import hip_harness as hh
    from phaneron_amd import capi
    layers, oracle_frame = layers_of(w, h, n, 0)
    out = poisoned(w, h)
    dl = [hh.dev(l) for l in layers]
    with capi.trace() as t:
        hh.ctx().fused_v210_combine(dl, out, w, h, *(colour or device_colour()))
    assert t.route == "fused_v210_combine_lds", t.route
    same_words(hh.host(out, np.uint32), oracle_frame if want is None else want, "fused_v210_combine %dx%d n=%d" % (w, h, n))


def run_batch(jobs, w, h, n, colour=None, want=None):
    import hip_harness as hh
    from phaneron_amd import capi
    cases = [layers_of(w, h, n, j) for j in range(jobs)]
    outs = [poisoned(w, h) for _ in range(jobs)]
    dl = [[hh.dev(l) for l in layers] for layers, _ in cases]
    with capi.trace() as t:
        hh.ctx().fused_v210_combine_batch(dl, outs, w, h, *(colour or device_colour()))
    assert set(t.kernels) == {"fused_v210_combine_lds"} and len(t.kernels) == 1, t.route  # ONE launch for all jobs
    for j in range(jobs):
        same_words(hh.host(outs[j], np.uint32), cases[j][1] if want is None else want[j], "fused_v210_combine_batch %dx%d n=%d job %d of %d" % (w, h, n, j, jobs))


@pytest.mark.parametrize("n", [1, 4])
def test_one_workgroup_one_partial_wave(n):
    """48 x 2: 16 quads - one workgroup whose share ends inside its first wave (per_wg, and the `wg_end - 1` clamp of the idle lanes)"""
    run_one(48, 2, n)


def test_more_workgroups_than_slices():
    """96 x 4: 64 quads, one slice - the launcher's cap wg_per_job <= slices with the reciprocal made for the capped value"""
    run_one(96, 4, 4)


@pytest.mark.parametrize("jobs", [2, 3, 4])
def test_batched_jobs_behind_the_moved_fields(jobs):
    """384 x 6 through ph_fused_v210_combine_batch: jobs >= 1 read their layers and output from the arrays behind the head"""
    run_batch(jobs, 384, 6, 3)


@pytest.mark.parametrize("jobs", [1, 2, 3, 4])
def test_job_division_at_the_launchers_group_sizes(jobs):
    """1920 x 408 is 130560 quads = 128 slices: on the MI355X's 256 CUs the launcher gives a job 128, 128, 85 and 64 workgroups, so
    blockIdx.x / wg_per_job runs over every group size it can produce for 2 .. 4 jobs, with real quotients.  (256 workgroups: the
    2160p tests.)  One layer per job keeps the oracle's share of the test short."""
    if jobs == 1:
        run_one(1920, 408, 1)
    else:
        run_batch(jobs, 1920, 408, 1)


def test_ragged_lines_share_the_head():
    """1280 x 4: the TAIL instantiation (lines of 213 quads and a 2-pixel tail in a pitch of 216 slots) has the same head"""
    run_one(1280, 4, 4)


# ---- the host-computed lookup constants under two registered tables of different layouts ------------------------------------------
@contextlib.contextmanager
def forced(layout, seed):
    """(host table, registered device table) that lut_compress can hold in `layout` only"""
    import hip_harness as hh
    tab = luts.layout_table(layout[0], layout[1], seed)
    with luts.register(tab) as dev:
        info = hh.ctx().lut_info(dev)
        assert info == dict(lds_bytes=luts.LDS_BYTES[layout], index_bias=layout[0], blocks_per_octave_log2=layout[1]), (layout, info)
        yield tab, dev


@pytest.mark.parametrize("rl,wl", [(luts.LARGEST, luts.SMALLEST), (luts.SMALLEST, luts.LARGEST)], ids=["rd-larger", "wr-larger"])
def test_two_tables_of_different_layouts(rl, wl):
    """reader table larger and writer table larger (bias 16 / 2^9 blocks per octave against bias 128 / 2^7): each table's a_scale,
    a_base, delta_base and a_shift differ, so a record that is wrong, or the reader's used for the writer, moves the frame.  One
    partial wave, ragged lines, and a batch of two."""
    import hip_harness as hh
    from phaneron_amd import capi
    gamut12 = np.concatenate([luts.IDENTITY, np.zeros(3, np.float32)])
    with forced(rl, 0xF00D) as (rtab, drtab), forced(wl, 0xF00D + 1000) as (wtab, dwtab):
        o_colour = (orc.ycbcr2rgb_matrix("709"), rtab, luts.IDENTITY, orc.rgb2ycbcr_matrix("709"), wtab)
        d_colour = (hh.dev(capi.ycbcr2rgb_matrix("709")), drtab, hh.dev(gamut12), hh.dev(capi.rgb2ycbcr_matrix("709")), dwtab)
        for w, h, n in ((48, 2, 4), (1280, 4, 4)):
            run_one(w, h, n, d_colour, orc.pipeline_v210_combine(list(layers_of(w, h, n, 0)[0]), w, h, *o_colour))
        w, h, n = 384, 6, 3
        run_batch(2, w, h, n, d_colour, [orc.pipeline_v210_combine(list(layers_of(w, h, n, j)[0]), w, h, *o_colour) for j in range(2)])
