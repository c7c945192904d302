"""Break-even survivor share of the dim-128 bound path (l1k2_prune.hip): for inputs whose survivor share
ranges from a few percent to nearly all pairs, the time of the `l1k2_tile` scope with the bound off,
with the bound on and the fallback disabled (SPECTAVI_L1K2_PRUNE_SHARE=1024), with every wave falling
back after the warm-up tiles (=0), and with the shipped rule (unset).  One child process per setting: the
library reads the knob once.
Usage: python tools/l1k2_prune_breakeven.py [rows] [input ...]   (inputs: u256 u128 u64 u32 u16 u8 sift)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys
sys.path.insert(0, %r)
import numpy as np, torch
from spectavi_amd import device as spv
n, kind = int(sys.argv[1]), sys.argv[2]
if kind == "sift":   # the golden table's descriptor columns, tiled, every other row perturbed by a few units
    t = np.load(os.path.join(%r, "tests", "golden", "sift_sur_ogre_table.npz"))["table"][:, -128:]
    u = np.clip(np.rint(t), 0, 255).astype(np.int16)
    rng = np.random.default_rng(3)
    def make():
        out = u[rng.permutation(len(u))][np.arange(n) %% len(u)]
        noisy = rng.random(n) < 0.5
        out[noisy] += rng.integers(-3, 4, (int(noisy.sum()), 128)).astype(np.int16)
        return torch.from_numpy(np.clip(out, 0, 255).astype(np.uint8)).cuda()
    x, y = make(), make()
else:
    g = torch.Generator(device="cuda").manual_seed(1)
    hi = int(kind[1:])
    x = torch.randint(0, hi, (n, 128), dtype=torch.uint8, device="cuda", generator=g)
    y = torch.randint(0, hi, (n, 128), dtype=torch.uint8, device="cuda", generator=g)
rec = {}
for mode in (0, 1):
    spv.l1k2_set_prune(mode)
    spv.l1k2(x, y); torch.cuda.synchronize()
    spv.profile_enable(True); spv.profile_reset()
    for _ in range(2): spv.l1k2(x, y)
    torch.cuda.synchronize()
    k, ms = spv.profile_read("l1k2_tile")
    spv.profile_enable(False)
    rec["ms_prune%%d" %% mode] = ms / k
    if mode == 1:
        b, s, e = spv.l1k2_prune_stats()
        rec["survivor_share"] = s / max(b, 1)
        rec["fallback_share"] = e / float(n) / n
print(json.dumps(rec))
''' % (ROOT, ROOT)


def main():
    args = sys.argv[1:]
    rows = int(args[0]) if args and args[0].isdigit() else 262144
    kinds = [a for a in args if not a.isdigit()] or ["u256", "u128", "u64", "u32", "u16", "u8", "sift"]
    for kind in kinds:
        for share in [None if k == "shipped" else k for k in os.environ.get("BREAKEVEN_KNOBS", "1024,0,shipped").split(",")]:
            env = dict(os.environ)
            env.pop("SPECTAVI_L1K2_PRUNE_SHARE", None)
            if share is not None:
                env["SPECTAVI_L1K2_PRUNE_SHARE"] = share
            out = subprocess.run([sys.executable, "-c", CHILD, str(rows), kind], env=env, capture_output=True, text=True,
                                 timeout=300)
            lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
            rec = json.loads(lines[-1]) if lines else {"error": out.stderr[-300:]}
            rec.update(rows=rows, input=kind, share_knob=share or "shipped")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
