"""CPU: the candidate-view kernels and k_frontview keep 0 bytes of scratch and the occupancy they had before their shared pieces
moved into ray_walk.h, view_kernels.h and common.h (block_sum, xcd_env).  A kernel may use fewer registers; a VGPR count that
crosses an occupancy step downward fails.  k_view_gain<true> and k_view_cover<0, 1> sit right below the step from 5 to 4 waves,
k_frontview two registers below the step from 6 to 5 (DESIGN.md has the rows).
"""
import os
import re
import shutil
import subprocess

import pytest

from gennbv_amd.csrc import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# waves per SIMD of the kernels before the refactor, by a distinctive piece of the mangled name
WAVES = {
    "viewgain.hip": {"k_view_gainILb0E": 5, "k_view_gainILb1E": 5, "k_vg_prepILb0E": 8, "k_vg_prepILb1E": 8, "k_vg_fateE": 8,
                     "k_vg_slabILb0E": 7, "k_vg_slabILb1E": 7},
    "viewcover.hip": {"k_view_coverILb0ELb0E": 5, "k_view_coverILb0ELb1E": 5, "k_view_coverILb1ELb0E": 4, "k_view_coverILb1ELb1E": 4},
    "frontview.hip": {"k_frontviewILb0ELb0E": 6, "k_frontviewILb0ELb1E": 6, "k_frontviewILb1ELb0E": 6, "k_frontviewILb1ELb1E": 6},
}


@pytest.mark.skipif(HIPCC is None, reason="hipcc needed to compile the gfx950 kernels")
@pytest.mark.parametrize("unit", sorted(WAVES))
def test_kernels_have_no_scratch_and_keep_their_occupancy(unit):
    cmd = [HIPCC] + B.flags() + ["--cuda-device-only", "-c", os.path.join(ROOT, "gennbv_amd", "csrc", unit), "-o", os.devnull,
                                 "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    # remarks per kernel: "Function Name: <mangled>", then "VGPRs: n", "ScratchSize [bytes/lane]: n", "Occupancy [waves/SIMD]: n"
    rows = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        get = lambda key: int(re.search(re.escape(key) + r"\s*(\d+)", b).group(1))
        rows[b.split()[0]] = (get("VGPRs:"), get("SGPRs Spill:"), get("ScratchSize [bytes/lane]:"), get("Occupancy [waves/SIMD]:"))
    for piece, waves in WAVES[unit].items():
        mine = [(name, row) for name, row in rows.items() if piece in name]
        assert len(mine) == 1, (piece, list(rows))
        vgpr, spill, scratch, occ = mine[0][1]
        print(unit, piece, "VGPRs", vgpr, "SGPR spills", spill, "scratch", scratch, "waves/SIMD", occ)
        assert scratch == 0 and occ >= waves, (piece, vgpr, scratch, occ, waves)
