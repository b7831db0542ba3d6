#!/bin/bash
# usage: bash tools/spills_report.sh > profiles/rNN_spills.txt  -- registers, scratch and spills of the hot kernels from the compiler
# (make resources) and, per kernel, the basic blocks that touch scratch (tools/asm_spills.py over make asm's output).  No GPU needed.
#        bash tools/spills_report.sh FILE.hip [FILE.hip ...]  -- the compiler's figures for every kernel of the given
# files of blurrily_amd/csrc (the library's flags, -Rpass-analysis=kernel-resource-usage), and how many instructions
# of each file's device assembly touch scratch.
cd "$(dirname "$0")/.."
if [ $# -gt 0 ]; then
  FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC"
  for f in "$@"; do
    echo "# $f: hipcc $FLAGS -c -Rpass-analysis=kernel-resource-usage"
    (cd blurrily_amd/csrc && /opt/rocm/bin/hipcc $FLAGS -c -Rpass-analysis=kernel-resource-usage -o /dev/null "$f" 2>&1) | python3 -c "
import sys,re
cur=None
keys=(('TotalSGPRs',r'TotalSGPRs: (\d+)'),('VGPRs',r' VGPRs: (\d+)'),('ScratchSize [bytes/lane]',r'ScratchSize \[bytes/lane\]: (\d+)'),('Occupancy [waves/SIMD]',r'Occupancy \[waves/SIMD\]: (\d+)'),('SGPRs Spill',r'SGPRs Spill: (\d+)'),('VGPRs Spill',r'VGPRs Spill: (\d+)'),('LDS Size [bytes/block]',r'LDS Size \[bytes/block\]: (\d+)'))
out={};order=[]
for l in sys.stdin:
    m=re.search(r'Function Name: (\S+)',l)
    if m:
        cur=m.group(1)
        if cur not in out: out[cur]={}; order.append(cur)
    for k,pat in keys:
        m=re.search(pat,l)
        if m and cur: out[cur][k]=m.group(1)
for f in order:
    print(f); print(' '+' '.join(f'{k}: {out[f].get(k)}' for k,_ in keys))
"
    (cd blurrily_amd/csrc && /opt/rocm/bin/hipcc $FLAGS -S --cuda-device-only -o - "$f" 2>/dev/null) | python3 -c "
import sys,re
t=sys.stdin.read()
n=lambda p: len(re.findall('^[ \t]+'+p,t,re.M))
print('# device assembly: %d scratch_ instructions, %d global atomics, %d v_readlane / v_writelane, %d ds_bpermute'
      % (n('scratch_'), n('global_atomic_'), n('v_(readlane|writelane)'), n('ds_bpermute')))
"
  done
  exit 0
fi
echo "# register spills of the hot kernels at commit $(git rev-parse --short HEAD) (+ working tree)"
echo "# (make -C blurrily_amd/csrc resources: the compiler's own figures; tools/asm_spills.py: where the scratch accesses sit --"
echo "#  basic blocks with a barrier, >= 8 LDS atomics or a scratch access; 'scratch [...]' lists the accesses of the block)"
echo
make -s -C blurrily_amd/csrc resources 2>&1 | python3 -c "
import sys,re
cur=None;d={};order=[]
for l in sys.stdin:
    m=re.search(r'Function Name: (\S+)',l)
    if m: cur=m.group(1); d[cur]={}; order.append(cur)
    for k,pat in (('VGPRs',r' VGPRs: (\d+)'),('scratch',r'ScratchSize \[bytes/lane\]: (\d+)'),('occ',r'Occupancy \[waves/SIMD\]: (\d+)'),('sgpr_sp',r'SGPRs Spill: (\d+)'),('vgpr_sp',r'VGPRs Spill: (\d+)')):
        m=re.search(pat,l)
        if m and cur: d[cur][k]=m.group(1)
for k in order:
    if any(x in k for x in ('wsweep_kernel','find_small_kernel','find_one_kernel','find_kernelIh')) and 'counted' not in k:
        v=d[k]; print(f\"{k}  VGPRs {v.get('VGPRs')}  scratch {v.get('scratch')} B/lane  occupancy {v.get('occ')}  SGPR spills {v.get('sgpr_sp')}  VGPR spills {v.get('vgpr_sp')}\")
"
make -s -C blurrily_amd/csrc asm 2>&1 | grep -i error
for k in find_kernelIhLi1024ELb0ELb1E find_kernelIhLi1024ELb1ELb1E find_small_kernel find_one_kernel wsweep_kernel; do
  echo; echo "## $k: blocks with scratch accesses"
  python3 tools/asm_spills.py $k | grep -E "scratch \['|totals"
done
