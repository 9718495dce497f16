"""Every sanitized row of build.PROGRAMS, built and run: a stand-alone program with its own main and no GPU, host code of
the library compiled under -fsanitize=address,undefined.  Each must exit 0, report no failure and no sanitizer finding,
and end on its own closing line."""
import re
import subprocess

import pytest

from icp_slam_prototype_amd import build

# what the last line of each program's stdout holds when everything held (see the end of its tests/cpp/*_host_main.cpp)
CLOSING = {
    "tsdf_apply_host_sanitized": r"refusals",
    "bilateral_host_sanitized": r"bilateral host: ok",
    "pyramid_host_sanitized": r"pyramid host: ok",
    "projective_host_sanitized": r"projective host: ok",
    "projective_color_host_sanitized": r"projective colour host: ok",
    "sdf_track_host_sanitized": r"sdf track host: ok",
    "fern_host_sanitized": r"fern host: ok",
    "tsdf_shift_host_sanitized": r"clean",
    "tsdf_mesh_host_sanitized": r"^\d+ x \d+ x \d+: \d+ vertices, ",
}

SANITIZED = [name for name, row in build.PROGRAMS.items() if row["kind"].startswith("sanitized")]


@pytest.mark.parametrize("name", SANITIZED)
def test_sanitized_host_program_exits_clean(name):
    exe = build.program(name)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "FAILED" not in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert re.search(CLOSING[name], r.stdout.splitlines()[-1])
