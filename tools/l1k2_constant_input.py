"""Worst case of the dim-128 bound path: all rows equal, nothing can be ruled out.  Prints the time of
the l1k2_tile scope at 256k x 256k.  Usage: python tools/l1k2_constant_input.py [rows]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from spectavi_amd import device as spv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
x = torch.full((n, 128), 93, dtype=torch.uint8, device="cuda")
spv.l1k2(x, x)
torch.cuda.synchronize()
spv.profile_enable(True)
spv.profile_reset()
for _ in range(3):
    spv.l1k2(x, x)
torch.cuda.synchronize()
k, ms = spv.profile_read("l1k2_tile")
print(json.dumps({"rows": n, "input": "constant", "l1k2_tile_ms": ms / k}))
