"""Cost of bead detection (mvn_detect_beads, csrc/mvn_detect.hpp) on the MI355X.
  mvn_detect_time for uint16 and float32 raw stacks of 128 x 512 x 512 and 320 x 1920 x 1920 at sigma1 = 1.5 and 2.5
  (sigma2 = 2^(1/4) sigma1): milliseconds per detection (the three blur passes, the extremum pass and the fit: all its
  device work), for the blur passes alone, and for a plain copy of one float32 volume.  From the copy follows the rate
  at which this device streams; from the volumes the passes move by construction - the raw stack read once, 2 + 2
  volumes written and read twice, D written and read once: 10 float32 volumes and the raw stack - the time that traffic
  costs at that rate, and the ratio of the measured detection to it.
    python tools/detect_bench.py [out.json] [--small]      (--small: the 128 x 512 x 512 stack only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libmultiviewnative_amd import native

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
STACKS = ((128, 512, 512),) if "--small" in sys.argv else ((128, 512, 512), (320, 1920, 1920))
Q = 2.0 ** 0.25
lib = native.lib()
res = {"rows": []}
for stack in STACKS:
    n = stack[0] * stack[1] * stack[2]
    for u16 in (True, False):
        for sigma in (1.5, 2.5):
            # a threshold far above the random values' D: the candidates stay rare, as they are in a real stack
            runs = [lib.detect_time(stack, sigma, sigma * Q, 400.0, u16=u16, reps=3) for _ in range(3)]
            detect, blur, copy = (min(x[i] for x in runs) for i in range(3))
            rate = 2 * 4 * n / copy / 1e6  # GB/s of the copy: one volume read, one written
            blur_bytes = (2 if u16 else 4) * n + 9 * 4 * n   # raw once; 2 + 2 volumes out and in again; D out
            detect_bytes = blur_bytes + 4 * n                # D in again
            row = {"stack": stack, "dtype": "uint16" if u16 else "float32", "sigma1": sigma, "detect_ms": detect,
                   "blur_ms": blur, "copy_ms": copy, "copy_gb_per_s": rate,
                   "blur_streaming_ms": blur_bytes / rate / 1e6, "detect_streaming_ms": detect_bytes / rate / 1e6,
                   "blur_over_streaming": blur / (blur_bytes / rate / 1e6),
                   "detect_over_streaming": detect / (detect_bytes / rate / 1e6), "all_ms": runs}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
