"""Cost of bead registration (mvn_register_beads, csrc/mvn_register.hpp) on the MI355X.
  mvn_register_time at (n_A, n_B, H) = (2000, 2000, 10^4), (10000, 10000, 10^5) and (50000, 50000, 10^5): milliseconds
  for the neighbour and descriptor pass of both sets, for the match pass with its fold, and for the RANSAC pass over
  min(n_A, n_B) candidate records.  From the match pass follows its rate in descriptor comparisons per second
  (n_A n_B 16 per launch); a comparison is 9 subtractions, 9 products and 8 sums in float32, none of them fused, so the
  rate times 26 is set beside the float32 vector peak of the device, which counts a fused multiply-add as two.
    python tools/register_bench.py [out.json] [--small]      (--small: the first size only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libmultiviewnative_amd import native

PEAK_FP32_VECTOR_TFLOPS = 157.3  # MI355X, spec; a fused multiply-add counts as two
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else None
CASES = ((2000, 2000, 10 ** 4), (10000, 10000, 10 ** 5), (50000, 50000, 10 ** 5))
if "--small" in sys.argv:
    CASES = CASES[:1]
lib = native.lib()
res = {"rows": []}
for na, nb, hyps in CASES:
    runs = [lib.register_time(na, nb, hyps, reps=3) for _ in range(3)]
    neigh, match, ransac = (min(x[i] for x in runs) for i in range(3))
    comparisons = 16.0 * na * nb
    rate = comparisons / match / 1e-3
    row = {"num_a": na, "num_b": nb, "hypotheses": hyps, "neighbours_ms": neigh, "match_ms": match, "ransac_ms": ransac,
           "match_comparisons_per_s": rate, "match_tflops_unfused": 26.0 * rate / 1e12,
           "match_over_fp32_vector_peak": 26.0 * rate / 1e12 / PEAK_FP32_VECTOR_TFLOPS,
           "ransac_residuals_per_s": float(hyps) * min(na, nb) / ransac / 1e-3,
           "device_bytes": lib.register_memory(na, nb, hyps), "all_ms": runs}
    res["rows"].append(row)
    print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
