"""The one way the tests run a C++ mirror program (a "mirror" row of build.PROGRAMS): bytes in, bytes out."""
import os
import subprocess
import tempfile

from icp_slam_prototype_amd import build


def run(name, blob, *args, timeout=120):
    """Build the program, hand it `blob` as in.bin, run [exe, in.bin, *args, out.bin] and return (out.bin's bytes, the
    program's stdout).  Anything but exit status 0 fails the test."""
    exe = build.program(name)
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        out = subprocess.run([exe, fin, *args, fout], capture_output=True, text=True, timeout=timeout)
        assert out.returncode == 0, (out.returncode, out.stderr)
        with open(fout, "rb") as f:
            return f.read(), out.stdout
