"""The passes behind mvn_derive_kernels of the host emulation (csrc/mvn_psf.hpp) in a stand-alone program under
AddressSanitizer + UBSan: tools/psf_standalone.cpp runs the correlation, normalisation and pointwise bodies on exactly
sized heap blocks - kernels of (1, 3, 5), (33, 7, 11) with and without exact zeros, and one view of (3, 3, 3) - against a
plain loop over the definition and exits non-zero on a mismatch.  The sanitizer runtimes are linked statically, the
environment is passed on as it is, and nothing is loaded into Python: the program is built here and run as a child
process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_passes_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "psf_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "psf_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for shape in ("(1, 3, 5) x 3 views", "(33, 7, 11) x 2 views:", "(33, 7, 11) x 2 views with zeros",
                  "autocorrelation (65, 13, 21)", "(3, 3, 3) x 1 views"):
        assert shape in r.stdout, shape
    assert r.stdout.count("0 mismatches") == 4
