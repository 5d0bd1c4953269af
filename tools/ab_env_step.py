"""Interleaved A/B of the whole C2 forward step under different library environment settings (the tuning flags are read when a
context is created, i.e. per mgunet.UNet): prints ms per step for every setting and round, and whether the outputs are bitwise equal
to the first setting's.
  python tools/ab_env_step.py [--graph] ROUNDS NAME=VALUE[,NAME=VALUE...] [NAME=VALUE...] ...     ("-" = no override)
  e.g.  python tools/ab_env_step.py 3 - MGU_WINO_ASM=0
--graph: the headline step as bench.py runs it (U-Net + patch means + the patch GAT through mgunet.MinGraphUNet), which is what
the switches of the head / patch-mean path act on, e.g.  python tools/ab_env_step.py --graph 4 MGU_HEAD_FUSED=0 MGU_HEAD_FUSED=1
"""
import os
import sys

from benchkit import emit, timed  # first: benchkit sets the import path
import torch

import mgunet

graph = len(sys.argv) > 1 and sys.argv[1] == "--graph"
if graph:
    del sys.argv[1]
rounds = int(sys.argv[1])
settings = sys.argv[2:] or ["-"]
dev = torch.device("cuda:0")
torch.manual_seed(0)
x = torch.randn(8, 3, 512, 512, device=dev)
touched = sorted({kv.split("=")[0] for s in settings if s != "-" for kv in s.split(",")})
first = None
for r in range(rounds):
    for s in settings:
        for k in touched:
            os.environ.pop(k, None)
        if s != "-":
            for kv in s.split(","):
                k, v = kv.split("=")
                os.environ[k] = v
        torch.manual_seed(1)
        unet = mgunet.UNet(3, 2, 32, 4).to(dev).eval()
        if graph:
            unet = mgunet.MinGraphUNet(unet, mgunet.GATNetwork(32, 128, 64, 4, 1).to(dev).eval(), 16).eval()
        ms = timed(lambda: unet(x), 20, 3, park=False)   # the step as a caller paces it, as bench.py runs it
        lg, sk, ft = unet(x)[:3]
        outs = [lg.clone()] + [t.clone() for t in ft]
        if first is None:
            first = outs
        same = all(torch.equal(a, b) for a, b in zip(first, outs))
        emit(round=r, env=s, ms_per_step=round(ms, 4), bitwise_equal_to_first=same)
        del unet
