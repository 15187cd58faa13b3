"""One cm3p_lora_grad call per adapted projection shape of a 768-wide layer at T = 32 x 4096, r = 16, for a counter run:
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -o out -- python tools/ubench/lora_pmc.py          (WRITE_SIZE: a second run)
    python tools/ubench/lora_pmc.py --read DIR      sums the counter per kernel of lora.hip (KiB as reported)
No tracing in the same run; tools/ubench/lora_pmc.sh does both passes."""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
T, R = 32 * 4096, 16
SHAPES = (("Wqkv", 768, 2304), ("attn.Wo", 768, 768), ("Wi", 768, 2304), ("mlp.Wo", 1152, 768))  # (name, K, N)


def read(d):
    tot = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            m = re.search(r"lora_\w+_kernel(<\d+>)?", row["Kernel_Name"])
            if m:
                key = (m.group(0), row["Counter_Name"])
                tot[key] = tot.get(key, 0.0) + float(row["Counter_Value"])
    algo = sum(4 * T * (K + N) for _, K, N in SHAPES)
    print(f"algorithmic operand bytes of the {len(SHAPES)} calls (X and DY twice): {algo / 1e9:.3f} GB")
    for (k, c), v in sorted(tot.items()):
        print(f"{c:11s} {k:40s} {v:14.0f} KiB = {v * 1024 / 1e9:.3f} GB")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--read":
        return read(sys.argv[2])
    import torch

    from cm3p_amd import kernels as K

    for _, Kd, N in SHAPES:
        x = torch.randn(T, Kd, device="cuda").to(torch.bfloat16)
        dy = torch.randn(T, N, device="cuda").to(torch.bfloat16)
        A, B = torch.randn(R, Kd, device="cuda"), torch.randn(N, R, device="cuda")
        K.lora_grad(x, dy, A, B, 2.0)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
