#!/bin/bash
# Registers, spills, scratch and LDS of the GICP / fused / cloud / planar ICP / point-to-plane ICP / top-K kernels as the compiler
# reports them (no GPU needed), over every source of build.SOURCES:
#   tools/resource_usage.sh [extra hipcc flags, e.g. -DPCORE_GICP_LDS_ROUNDS=1]
# (tools/isa_diff.py prints the same figures for every kernel beside a comparison with another tree.)
cd "$(dirname "$0")/.."
FLAGS=$(python -c "from perception_amd import build; print(' '.join(f for f in build.flags() if f not in ('-shared','-fPIC')))")
for SRC in $(python -c "from perception_amd import build; print(' '.join(build.SOURCES))"); do
  /opt/rocm/bin/hipcc $FLAGS "$@" --offload-device-only -S perception_amd/csrc/$SRC -o /dev/null \
    -Rpass-analysis=kernel-resource-usage 2>&1 | python -c "
import re, sys
cur = None
KERNELS = ('gicp_kernel', 'fused_cost', 'render_cloud_kernel', 'window_probe_kernel', 'covariance_kernel', 'planar_icp', 'p2p_icp', 'scene_kernel', 'scene_finalize', 'topk_', 'state_cost')
for l in sys.stdin:
    m = re.search(r'remark: Function Name: (\S+)', l)
    if m:
        cur = m.group(1); continue
    m = re.search(r'remark:\s+(VGPRs|TotalSGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', l)
    if m and cur and any(k in cur for k in KERNELS):
        print(f'{cur[:60]:60s} {m.group(1):28s} {m.group(2)}')
"
done
