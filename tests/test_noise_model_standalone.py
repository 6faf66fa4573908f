"""The noise-model divide epilogues of the host emulation (MVN_EPI_DIVIDE_NM, MVN_EPI_DIVIDE_NM_U16) in a stand-alone
program under AddressSanitizer + UBSan: tools/noise_model_standalone.cpp runs the last-axis pass bodies with the
epilogue, plain and fused, on float32 and uint16 views, and the reduce, on (3, 5, 2), (10, 14, 45) with a window
strictly inside the volume, and (6, 8, 512), against a plain triple loop, and exits non-zero on a mismatch.  The
sanitizer runtimes are linked statically, the environment is passed on as it is, and nothing is loaded into Python: the
program is built here and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmultiviewnative_amd", "csrc")


def test_epilogue_bodies_against_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "noise_model_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DMVN_HOST_EMU", "-fopenmp", "-pthread", "-fno-fast-math",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wno-unknown-pragmas", "-I", CSRC,
                           os.path.join(ROOT, "tools", "noise_model_standalone.cpp"), "-o", exe])
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    for shape in ("(3, 5, 2)", "(10, 14, 45) window (2, 2, 3)", "(6, 8, 512)"):
        assert shape in r.stdout
    assert "wave rows 1" in r.stdout and "MISMATCH" not in r.stdout
