#!/bin/bash
# Timing-only ablation builds of the hand-scheduled global attention backward (results are wrong by construction; run from the
# repo root on the GPU box).  One library per ablation mask, each timed by tools/attn_bwd_ab.py through CM3P_HIP_LIB.
#   bash tools/ubench/attn_bwd_ablate.sh "1 2 4 8 16 32"     (attention_bwd_fused.hip, -DCM3P_FABL=mask)
set -e
R=$(pwd)
C=$R/cm3p_amd/csrc
O=$R/gpurun_out/ablate
mkdir -p $O
SRC=attention_bwd_fused
OBJS=$(ls $C/*.o | grep -v "/$SRC.o")
for m in ${1:-1 2 4 8}; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -DCM3P_FABL=$m -c $C/$SRC.hip -o $O/${SRC}_$m.o 2>/dev/null
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $O/lib_$m.so $OBJS $O/${SRC}_$m.o
  echo "== fused ablation mask $m"
  CM3P_ALLOW_ABLATED_LIB=1 CM3P_HIP_LIB=$O/lib_$m.so timeout -k 10 120 python3 tools/attn_bwd_ab.py --rounds 3 --arms fused 2>&1 | grep -E "^fused "
done
