"""Records the results that tests/test_emu_mid_fused_phase.py and tests/test_gpu_mid_fused_phase.py pin bit for bit: for the
cases of tests/mid_fused_phase_util.py a seeded sample of 4096 voxels of the blocking ABI call's result and their
indices.  Run on the build whose arithmetic is to be kept:
    python tools/mid_fused_phase_golden.py emu [out.npz]     (the host emulation, lib/libmvn_emu.so; EMU_CASES)
    python tools/mid_fused_phase_golden.py gpu [out.npz]     (the product library, on the GPU box; CASES)
Default output: tests/golden/mid_fused_phase_<emu|gpu>.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MVN_MID_FUSED"] = "2"
os.environ["MVN_PAD_MODE"] = "none"
import numpy as np  # noqa: E402
from libmultiviewnative_amd import native  # noqa: E402
import mid_fused_phase_util as mu  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "emu"
assert tag in ("emu", "gpu"), tag
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(mu.GOLDEN_DIR, "mid_fused_phase_%s.npz" % tag)
binding = native.Binding(native.EMU_SO) if tag == "emu" else native.lib()
rec = {}
for k0, d0 in (mu.EMU_CASES if tag == "emu" else mu.CASES):
    got, _, _ = mu.run_case(binding, k0, d0)
    idx = mu.sample_index(k0, d0)
    rec[mu.golden_key(k0, d0) + "_idx"] = idx.astype(np.int32)
    rec[mu.golden_key(k0, d0) + "_val"] = got.reshape(-1)[idx].astype(np.float32)
    print("K %2d d0 %2d: %d voxels, sum %.9g" % (k0, d0, idx.size, float(got.reshape(-1)[idx].astype(np.float64).sum())), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
np.savez_compressed(out, **rec)
print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))
