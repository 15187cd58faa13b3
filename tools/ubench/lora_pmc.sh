#!/bin/bash
# HBM traffic of cm3p_lora_grad from the L2's memory-side counters, one counter per pass (they do not fit one), no tracing beside them.
#   bash tools/ubench/lora_pmc.sh [OUT_DIR]      (GPU box, repository root)  -> OUT_DIR/lora_pmc.txt (default: a fresh temporary directory)
R=$(pwd); O=${1:-$(mktemp -d)}; mkdir -p $O
for c in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 200 rocprofv3 --pmc $c --output-format csv -d $O/$c -o out -- python $R/tools/ubench/lora_pmc.py > $O/$c.log 2>&1 || { echo "$c pass failed: $?"; tail -5 $O/$c.log; exit 1; }
done
python $R/tools/ubench/lora_pmc.py --read $O | tee $O/lora_pmc.txt
