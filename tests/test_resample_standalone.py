"""The resample pass and the weights normalisation of the host emulation (csrc/mvn_resample.hpp) in a stand-alone program
under AddressSanitizer + UBSan: tools/resample_standalone.cpp runs the pass bodies on (3, 5, 7), (4, 6, 10), (2, 3, 20),
a block with tile seams on all three axes and a raw stack of one plane, from uint16 and float32 raw stacks, against a
plain triple loop over the definition and exits non-zero on a mismatch.  The sanitizer runtimes are linked statically,
the environment is passed on as it is, and nothing is loaded into Python: the program is built here and run as a child
process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_pass_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resample_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "resample_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for shape in ("(3, 5, 7) in", "(4, 6, 10) in", "(2, 3, 20) in", "(10, 14, 70) in", "(1, 6, 7)"):
        assert shape in r.stdout, shape
    assert r.stdout.count("uint16") == r.stdout.count("float32") == 6
