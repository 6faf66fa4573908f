"""The total-variation pass of the host emulation (csrc/mvn_tv.hpp) in a stand-alone program under AddressSanitizer +
UBSan: tools/tv_standalone.cpp runs the pass body on (3, 5, 2), (1, 3, 5), (10, 14, 45) and a volume with tile and
segment seams on every axis against a plain triple loop and exits non-zero on a mismatch.  The sanitizer runtimes are
linked statically, the environment is passed on as it is, and nothing is loaded into Python: the program is built
here and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_pass_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tv_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "tv_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for shape in ("(3, 5, 2)", "(1, 3, 5)", "(10, 14, 45)"):
        assert shape in r.stdout
