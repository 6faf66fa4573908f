"""The passes behind mvn_extract_psf of the host emulation (csrc/mvn_beads.hpp) in a stand-alone program under
AddressSanitizer + UBSan: tools/beads_standalone.cpp runs the gather, the sum over the groups, the minimum and the score
bodies on exactly sized heap blocks - beads in the corners of the stack, windows of (3, 5, 7), (5, 3, 67) and, wider
than the stack, (7, 9, 11) in (6, 7, 40), both element types - against a plain loop over the definition and exits
non-zero on a mismatch.  The sanitizer runtimes are linked statically, the environment is passed on as it is, and
nothing is loaded into Python: the program is built here and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_passes_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "beads_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "beads_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for case in ("uint16, stack (6, 7, 40), window (7, 9, 11), 70 beads", "float32, stack (9, 11, 70), window (5, 3, 67), 33",
                 "float32, stack (6, 7, 40), window (3, 5, 7), 4 beads"):
        assert case in r.stdout, case
    assert r.stdout.count(": 0 mismatches") == 36
