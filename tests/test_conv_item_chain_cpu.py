"""CPU check of the item-walking G = 64 conv kernels (csrc/conv_split.h, no GPU): with their item loops k_conv12_fwd_split<false>,
k_conv12_fwd_split<true> and k_conv2_wgrad_split_dma keep 0 bytes of scratch and at most 128 VGPRs -- four waves per SIMD at 1 024 threads.
(The data-gradient kernel lost 10 us to a spill when it was given an item loop: profiles/r06_notes.md, section 8.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
KERNELS = ("_Z18k_conv12_fwd_splitILb0EE", "_Z18k_conv12_fwd_splitILb1EE", "_Z23k_conv2_wgrad_split_dma")


@pytest.mark.skipif(HIPCC is None, reason="hipcc needed to compile the gfx950 kernels")
def test_item_walking_kernels_have_no_scratch_and_four_waves_per_simd():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c", os.path.join(ROOT, "gennbv_amd", "csrc", "encoder.hip"),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        for k in KERNELS:
            if name.startswith(k):
                get = lambda key: int(re.search(re.escape(key) + r"\s*(\d+)", blk).group(1))
                found[k] = (get("VGPRs:"), get("ScratchSize [bytes/lane]:"), get("VGPRs Spill:"), get("Occupancy [waves/SIMD]:"))
    assert sorted(found) == sorted(KERNELS), list(found)
    for k, (vgpr, scratch, spill, occ) in found.items():
        print(k, "VGPRs", vgpr, "scratch", scratch, "VGPR spill", spill, "waves/SIMD", occ)
        assert scratch == 0 and spill == 0 and vgpr <= 128 and occ >= 4, (k, vgpr, scratch, spill, occ)
