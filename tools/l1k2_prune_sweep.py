"""Times the L1 2-NN at dim 128 with the matrix-core bound off and on (spv_l1k2_set_prune) over a list of
shapes on one GPU; the `auto` rule of l1k2_prune.hip is read off the result.
Usage: python tools/l1k2_prune_sweep.py [xrows x yrows ...]   (default: squares 16k .. 1M)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from spectavi_amd import device as spv
    shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(n, n) for n in
                                                                             (16384, 32768, 65536, 131072, 262144, 524288, 1048576)]
    for m, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randint(0, 256, (m, 128), dtype=torch.uint8, device="cuda", generator=g)
        y = torch.randint(0, 256, (n, 128), dtype=torch.uint8, device="cuda", generator=g)
        rec = {"xrows": m, "yrows": n}
        for mode in (0, 1):
            spv.l1k2_set_prune(mode)
            spv.l1k2(x, y)
            torch.cuda.synchronize()
            spv.profile_enable(True)
            spv.profile_reset()
            reps = 3 if m * n <= 1 << 36 else 1
            for _ in range(reps):
                spv.l1k2(x, y)
            torch.cuda.synchronize()
            k, ms = spv.profile_read("l1k2_tile")
            spv.profile_enable(False)
            rec["ms_prune%d" % mode] = ms / k
        spv.l1k2_set_prune("auto")
        rec["speedup"] = rec["ms_prune0"] / rec["ms_prune1"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
