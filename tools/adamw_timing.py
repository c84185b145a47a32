"""The fused optimizer step (`FusedAdamW`: dd_adamw_step's three launches): what it costs on the GPU, beside torch's chain
on the same tensors and beside the streaming floor.

    python tools/adamw_timing.py                           # one and two branches -> profiles/adamw.txt (and stdout)
    python tools/adamw_timing.py --branches 1 --out -      # one branch, stdout only

The parameter set is that of `BEVControlNetModel(cross_attention_dim=768)` as bench.py builds it, once and twice (the
reference trains one or two branches): fp32 masters of the module's parameter shapes, the module's own fp16 Parameters as
shadows, fp32 gradients.  Per set:
  * each of the three launches alone (`ops.adamw_step(launches=1 / 2 / 4)`) and the whole `FusedAdamW.step()` with
    max_grad_norm=1 and a grad_scale, between a pair of device events, median of N, three rounds;
  * torch on the same GPU, same parameter and gradient tensors: GradScaler.unscale_ + clip_grad_norm_(foreach=True) +
    GradScaler.step(AdamW(fused=True)) + GradScaler.update() + torch._foreach_copy_ into the shadows, the same way;
  * the streaming floor: the bytes each launch must move (4 per element for the norm; p, g, m, v read, p, m, v and the
    16-bit shadow written: 30 for the update) over the 6.29 TB/s a float4 copy reaches on this part;
  * the memory the optimizer adds.
DD_ADAMW_CHUNK_AB=<n>: the chunk size of an alternative build of the library (DD_HIP_LIB) under A/B."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12                     # bytes / s, float4 copy


def device_events(torch, launch, n):
    rounds = []
    for _ in range(3):
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        rounds.append(statistics.median(ts))
    return rounds


def fmt(rounds):
    return " / ".join("%.0f" % r for r in rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--branches", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw.txt"))
    ap.add_argument("-n", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import torch
    from dualdiff_amd import _build, ops
    from dualdiff_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from dualdiff_amd.pipeline.optim import FusedAdamW
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    if os.environ.get("DD_ADAMW_CHUNK_AB"):
        ops.ADAMW_CHUNK = int(os.environ["DD_ADAMW_CHUNK_AB"])
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("# %s, torch %s, library %s, chunk %d" % (torch.cuda.get_device_name(0), torch.__version__,
                                                os.path.relpath(_build.lib_path(), ROOT), ops.adamw_chunk()))
    dev = torch.device("cuda:0")
    for branches in args.branches:
        with torch.device(dev):
            mods = [BEVControlNetModel(cross_attention_dim=768).to(torch.float16) for _ in range(branches)]
        shadows = [p for m in mods for p in m.parameters()]
        g = torch.Generator(device=dev).manual_seed(1)
        params = [torch.randn(s.shape, generator=g, device=dev) * 0.02 for s in shadows]
        for p in params:
            p.grad = torch.randn(p.shape, generator=g, device=dev) * (65536.0 * 1e-3)
        numel = sum(p.numel() for p in params)
        sizes = sorted(p.numel() for p in params)
        say("")
        say("%d branch(es): %d tensors, %.1f M parameters (smallest %d, median %d, largest %.1f M elements)"
            % (branches, len(params), numel / 1e6, sizes[0], sizes[len(sizes) // 2], sizes[-1] / 1e6))
        opt = FusedAdamW(params, max_grad_norm=1.0, shadows=dict(zip(params, shadows)))
        scale = torch.full((1,), 65536.0, device=dev)
        for _ in range(3):
            opt.step(grad_scale=scale)
        torch.cuda.synchronize()
        say("   after 3 steps: steps_taken %d, skipped %d, grad_norm %.6g, clip_coef %.6g; shadows equal p.half(): %s"
            % (int(opt.steps_taken), int(opt.skipped), float(opt.grad_norm), float(opt.clip_coef),
               all(torch.equal(s, p.half()) for p, s in zip(params, shadows))))
        group = opt.param_groups[0]

        def launch(mask):
            ops.adamw_step(opt._table, opt._chunks, opt._state_block, opt._lr_table, betas=group["betas"], eps=group["eps"],
                           weight_decay=group["weight_decay"], max_grad_norm=1.0, grad_scale=scale, workspace=opt._workspace,
                           launches=mask)
        floors = {1: 4 * numel / COPY_RATE * 1e6, 2: 12 * opt._chunks.shape[0] / COPY_RATE * 1e6, 4: 30 * numel / COPY_RATE * 1e6}
        total = 0.0
        for mask, name in ((1, "launch 1, norm partials"), (2, "launch 2, scalars      "), (4, "launch 3, update       ")):
            r = device_events(torch, lambda: launch(mask), args.n)
            total += statistics.median(r)
            say("   %s  %s us  (floor %.0f us: %.2f of the copy rate)"
                % (name, fmt(r), floors[mask], floors[mask] / statistics.median(r)))
        whole = device_events(torch, lambda: opt.step(grad_scale=scale), args.n)
        floor = 34 * numel / COPY_RATE * 1e6
        say("   FusedAdamW.step()         %s us  (floor at 34 bytes per parameter %.0f us: %.2f of the copy rate; the three "
            "launches alone sum to %.0f us)" % (fmt(whole), floor, floor / statistics.median(whole), total))
        say("   memory added: m and v %.2f GB, table %.1f KB, chunk list %.1f KB, partials and marks %.1f KB, state 96 bytes"
            % (8 * numel / 1e9, 48 * len(params) / 1e3, 8 * opt._chunks.shape[0] / 1e3, opt._workspace.numel() / 1e3))
        del opt
        if not args.no_torch:
            ref = torch.optim.AdamW(params, lr=8e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, fused=True)
            scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
            scaler.scale(torch.zeros((), device=dev))

            def chain():
                with torch.no_grad():
                    scaler.unscale_(ref)
                    torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
                    scaler.step(ref)
                    scaler.update()
                    torch._foreach_copy_(shadows, params)
            for _ in range(3):
                chain()
            torch.cuda.synchronize()
            r = device_events(torch, chain, args.n)
            say("   torch's chain             %s us  (unscale_, clip_grad_norm_(foreach), AdamW(fused) under the scaler, "
                "_foreach_copy_ to the shadows)" % fmt(r))
            say("   FusedAdamW.step() / torch's chain = %.2f" % (statistics.median(whole) / statistics.median(r)))
            del ref, scaler
        for p in params:
            p.grad = None
        del params, shadows, mods
        torch.cuda.empty_cache()
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
