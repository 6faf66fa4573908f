"""Cost of bead PSFs (mvn_extract_psf, csrc/mvn_beads.hpp) on the MI355X.
  mvn_extract_time for windows of 15^3 .. 31^3, 256 .. 4096 beads, a uint16 and a float32 raw stack of 128 x 512 x 512:
  milliseconds per extraction (the gather and the sum over the groups: all its device work), the same for the route a
  caller had until now - one launch of the resample pass per bead, image only, nothing summed -, and a plain copy of
  beads x window floats; the samples per second the extraction reaches (8 loads and one trilinear sample each), and
  the bar of the record: extraction <= per-bead resampling at every row.
    python tools/beads_bench.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libmultiviewnative_amd import native

out_path = sys.argv[1] if len(sys.argv) > 1 else None
STACK = (128, 512, 512)
lib = native.lib()
res = {"stack": STACK, "rows": []}
for u16 in (True, False):
    for edge in (15, 23, 31):
        for beads in (256, 1024, 4096):
            r = (edge,) * 3
            runs = [lib.extract_time(STACK, beads, r, u16=u16, reps=3) for _ in range(3)]
            extract, per_bead, copy = (min(x[i] for x in runs) for i in range(3))
            row = {"dtype": "uint16" if u16 else "float32", "window": r, "beads": beads, "extract_ms": extract,
                   "per_bead_resample_ms": per_bead, "copy_ms": copy, "resample_over_extract": per_bead / extract,
                   "extract_over_copy": extract / copy, "gsamples_per_s": beads * edge ** 3 / extract / 1e6,
                   "meets_bar": extract <= per_bead, "all_ms": runs}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
missed = [(x["dtype"], x["window"], x["beads"]) for x in res["rows"] if not x["meets_bar"]]
print(json.dumps({"rows_that_miss_the_bar": missed}), flush=True)
