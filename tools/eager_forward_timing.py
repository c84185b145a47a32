#!/usr/bin/env python3
"""Host cost of the eager path: wall time of one eager one-scene UNet forward (graph_forward = False, fp16, the benchmark's
models and inputs), forward + synchronise, median of 20 calls after 5 warm-up calls.  Prints `EAGER_MS <median>`.

    python tools/eager_forward_timing.py

A host-side change is judged by alternating this between a checkout of the parent and one of the change, five pairs in one
session, each run a process of its own (profiles/derived_weights_eager.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench


def main():
    dev, dt = torch.device("cuda:0"), torch.float16
    with torch.no_grad():
        unet, cns = bench.build_models(dt, dev, dual=False)
        unet.graph_forward = cns[0].graph_forward = False
        lat, prompt, cam, boxes, conds = bench.synthetic_inputs(1, dt, dev, 0)
        b, n = lat.shape[:2]
        t = torch.tensor(481, device=dev)
        lmi = torch.cat([lat] * 2)
        down, mid, ctx = cns[0](lmi, t.expand(2 * b), cam, boxes[0], prompt, conds[0], conditioning_scale=1.0,
                                guess_mode=False, return_dict=False, use_aug_text=False)
        x = lmi.reshape(2 * b * n, *lmi.shape[2:])

        def forward():
            t0 = time.perf_counter()
            unet(x, t, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        for _ in range(5):
            forward()
        ts = sorted(forward() for _ in range(20))
    print("EAGER_MS %.4f" % (1e3 * 0.5 * (ts[9] + ts[10])))


if __name__ == "__main__":
    main()
