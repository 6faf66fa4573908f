"""The launch-side dispatch of the last-axis passes (csrc/mvn_pass_bodies.hpp: mvn_epi_dispatch, the one table of
which pass takes which epilogue mode, and the helpers beside it) and the direct dim0 leg's shared launch check
(csrc/mvn_dim0_direct.hpp: mvn_dim0_check) in a stand-alone program: tools/epi_dispatch_standalone.cpp walks every
pass kind and every integer mode from -1 to one past the last enumerator and exits non-zero on a mismatch.  Headers
only, nothing is loaded into Python, no GPU: the program is built here and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_every_kind_and_mode_is_dispatched_once_or_refused(tmp_path):
    exe = str(tmp_path / "epi_dispatch_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fno-fast-math", "-ffp-contract=off",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "epi_dispatch_standalone.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
