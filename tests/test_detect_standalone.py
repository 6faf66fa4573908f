"""The passes behind mvn_detect_beads of the host emulation (csrc/mvn_detect.hpp) in a stand-alone program under
AddressSanitizer + UBSan: tools/detect_standalone.cpp runs the row, column and plane blurs, the extremum pass - into a
list of exactly the candidates' number, and into one that is an entry short - and the fit on exactly sized heap blocks,
both element types, maxima and minima, candidates next to the faces, a stack narrower than the radius, against a plain
loop over the definition, and exits non-zero on a mismatch.  The sanitizer runtimes are linked statically, the
environment is passed on as it is, and nothing is loaded into Python: the program is built here and run as a child
process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_passes_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "detect_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "detect_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for case in ("uint16, stack (5, 6, 40), sigma (1.5, 1.5, 1.5)", "float32, stack (34, 37, 70), sigma (2.5, 2.5, 2.5)",
                 "uint16, stack (9, 11, 70), sigma (0, 1.5, 1.5) / (0, 1.8, 1.8), minima"):
        assert case in r.stdout, case
    assert r.stdout.count(", 0 mismatches") == 36
