"""CPU-side checks of icpk_align_frames_batch's ABI: the layout of icpk_frame_job as a C compiler sees it in
include/icpk.h equals binding.FrameJob's, and the library exports the new entry points."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from icp_slam_prototype_amd import binding, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["stream", "depth_source", "depth_target", "R", "t", "last_rotation", "last_translation"]

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "icpk.h"
int main(void) {
  printf("sizeof %zu\n", sizeof(icpk_frame_job));
#define F(name) printf("%s %zu %zu\n", #name, offsetof(icpk_frame_job, name), sizeof(((icpk_frame_job*)0)->name));
  F(stream) F(depth_source) F(depth_target) F(R) F(t) F(last_rotation) F(last_translation)
  printf("max_streams %d\n", ICPK_MAX_FRAME_STREAMS);
  return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.fail("gcc is needed to compile the layout probe")
    d = tmp_path_factory.mktemp("probe")
    src, exe = d / "probe.c", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        k, *v = line.split()
        out[k] = tuple(int(x) for x in v)
    return out


def test_frame_job_layout_matches_header(layout):
    assert layout["sizeof"] == (C.sizeof(binding.FrameJob),)
    for name in FIELDS:
        f = getattr(binding.FrameJob, name)
        assert layout[name] == (f.offset, f.size), name
    assert layout["max_streams"] == (binding.MAX_FRAME_STREAMS,)


def test_frame_batch_symbols_exported():
    lib = C.CDLL(build.build())
    for s in ("icpk_align_frames_batch", "icpk_get_frames_trace", "icpk_release_frame_streams"):
        assert hasattr(lib, s), s
        assert s in binding.SYMBOLS


def test_frame_batch_refuses_null_context():
    lib = binding.load()
    assert lib.icpk_align_frames_batch(None, 0, None, 1, 1, 1.0, 0.0, None, 0, 0, 0, 0, 0, 0, None, None, None) == binding.E_ARG
    n = C.c_int32(0)
    assert lib.icpk_get_frames_trace(None, 0, C.byref(n), None, None, None, None) == binding.E_ARG
    assert lib.icpk_release_frame_streams(None) == binding.E_ARG
