"""phaneron_amd/csrc/ph_spans.h on its own: the byte ranges a job reads and writes and the one hazard test that decides where a shared
launch ends (ph_run_programs' groups, ph_chan_compose_batch_out, ph_clip_compose_batch_out).  The header is host-only C++17, so the
checks are a stand-alone program, tests/native/spans_check.cpp, built here with the host compiler: no GPU, no HIP.

What the header cannot show - that each planner asks it the right question - the GPU tests pin, per site and hazard (a dropped
hazard fails the test named):
  site                                RAW / WAR / WAW                                                     the site's exception
  ph_run_programs kind 1 (chan)       test_call_order_gpu cells chan-RAW, chan-RAW-chroma / chan-WAR /    two fields of one frame stay in one launch:
                                      (WAW is ph_chan_compose_batch's: cell chan-WAW)                     test_call_order_gpu ..two_fields_of_one_frame_from_the_channel_kernel_stay_in_one_launch
  kind 2 (fused)                      cells fused-RAW / fused-WAR / fused-WAW
  kind 3 (compose_up)                 cells up_*-RAW* / up_*-WAR* / up_*-WAW
  kind 5 (fused multi)                test_fused_multi_batch_gpu test_by_name_a_job_that_reads_an_earlier_output.. / ..writes_an_earlier_layer.. /
                                      ..writes_an_earlier_output_splits_the_group
  ph_chan_compose_batch_out           test_chan_batch_out_gpu test_a_job_reading_an_earlier_jobs_output / test_a_job_writing_what_an_earlier_job_reads /
                                      test_two_jobs_writing_one_plane_the_later_wins                      4:2:2 fields share, 4:2:0 do not: test_the_two_fields_of_one_frame_as_two_jobs
  ph_clip_compose_batch_out           test_clip_batch_gpu test_a_job_that_reads_an_earlier_jobs_output.. / ..writes_what_an_earlier_job_reads.. /
                                      ..writes_what_an_earlier_job_writes_starts_the_next_launch          two fields are two launches: test_the_two_fields_of_one_frame_are_two_launches
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "spans_check.cpp")


def host_compiler():
    for cc in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        exe = shutil.which(cc)
        if exe:
            return exe
    pytest.fail("no host C++ compiler (g++, c++ or clang++) to build tests/native/spans_check.cpp with")


def test_the_header_alone_keeps_its_promises(tmp_path):
    exe = str(tmp_path / "spans_check")
    built = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", SOURCE, "-o", exe], capture_output=True, text=True, timeout=120)
    assert built.returncode == 0, built.stderr
    assert not built.stderr.strip(), built.stderr  # (the header compiles without a warning from a plain host compiler)
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.strip().endswith("0 failed checks")
