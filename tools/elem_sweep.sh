#!/bin/bash
# Round-3 experiments on the N = 32 element-view kernel (run on the GPU box via gpurun):
#   1. FETCH_SIZE / WRITE_SIZE calibrated on known byte counts in this kernel's access shapes (tools/micro/fetchcal)
#   2. residency sweep 8 / 6 / 5 / 4 / 3 gaits per CU (WG_TICK_LDS_PAD): ticks/s, and the traffic per gait-tick at 8, 4, 3
# These rows were measured with round 2's 256-register build of the element view (make ... EXTRA="-DWG_TICK32_WPE=2
# -DWG_ELEM_GRP=8" reproduces it).  The round's third leg -- a build with the Z stream marked non-temporal (its row is in
# docs/HISTORY.md 3.2) -- needs the sources of commit 80f27a6, the last to carry that build switch, and is not run here.
set -eu
R=${GRAFT_REPO_ROOT:?run this on the GPU box (gpurun sets GRAFT_REPO_ROOT)}
mkdir -p $R/gpurun_out
cd "$R"
./tools/micro/fetchcal > gpurun_out/fetchcal.txt 2>&1
bash tools/pmc_traffic.sh fetchcal $R/tools/micro/fetchcal > gpurun_out/fetchcal_pmc.txt 2>&1
echo "calibration done"
export PN=32 PB=8192 PT=50 PR=3
for pad in 0 6400 11000 20000 33000; do
  WG_TICK_LDS_PAD=$pad python3 tools/probe_elem.py 2>&1 | { grep -v amdgpu.ids || true; }
done > gpurun_out/elem_residency.txt
echo "residency sweep done"
for pad in 0 20000 33000; do
  export WG_TICK_LDS_PAD=$pad
  bash tools/pmc_traffic.sh elem_pad$pad python3 $R/tools/probe_elem.py > gpurun_out/elem_pad${pad}_pmc.txt 2>&1
done
unset WG_TICK_LDS_PAD
echo "traffic passes done"
