"""The passes behind mvn_register_beads of the host emulation (csrc/mvn_register.hpp) in a stand-alone program under
AddressSanitizer + UBSan: tools/register_standalone.cpp runs the neighbour and descriptor pass, the match pass with its
fold - B in chunks whose last one is partial - and the RANSAC pass on exactly sized heap blocks, sets of 5, 65 and 257
beads, 1 and 257 hypotheses, exactly four candidates, against a plain loop over the definition, and exits non-zero on
a mismatch.  The sanitizer runtimes are linked statically, the environment is passed on as it is, and nothing is
loaded into Python: the program is built here and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_passes_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "register_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "register_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for case in ("neighbours and descriptors, 257 beads", "match, 65 x 257 beads in 3 chunks of 128",
                 "ransac, 4 candidates, 257 hypotheses: best score 4 at h = 0", "ransac, 257 candidates, 1 hypotheses"):
        assert case in r.stdout, case
    assert r.stdout.count(" 0 mismatches") == 6 + 18 + 6
