"""The sanitized row of K34 in build.LATER_PROGRAMS, built and run: tests/cpp/plane_host_main.cpp, a stand-alone program
with its own main and no GPU, over icpk_plane.cpp (and so csrc/plane_rule.h) compiled under -fsanitize=address,undefined.
Nothing is preloaded: the program is run directly.  It must exit 0, report no sanitizer finding and end on its closing
line."""
import subprocess

from icp_slam_prototype_amd import build


def test_plane_host_program_runs_clean_under_the_sanitizers():
    assert build.LATER_PROGRAMS["plane_host_sanitized"]["kind"] == "sanitized"
    assert build.LATER_PROGRAMS["plane_host_sanitized"]["csrc"] == ["icpk_plane.cpp"]
    exe = build.program("plane_host_sanitized")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert r.stdout.splitlines()[-1] == "plane host: ok"
