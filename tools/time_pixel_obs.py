#!/usr/bin/env python3
"""What pixel observations cost (diagnostic): pz_render_gray per scale, with and without the grey-background fast path,
against the only route without it -- render() in chunks plus torch ops for grey and the box filter.

    python tools/time_pixel_obs.py [--n 65536 4096] [--rounds 7] [--min-time 0.1] [--baseline-games 4096]

Per batch size: an env of n games (human vs human, synthetic sprites) is played for 96 random frames, then for every scale
in 1 / 2 / 4 / 8 two variants draw its state through the C ABI into their own output buffer: `fast` (background_gray
given) and `composed` (NULL: every pixel composed).  Each variant has a captured hipGraph of 4 launches; before it is
timed its frames are compared with the other variant's, and 8 lanes of them with render()'s frames reduced in numpy on the
host by the definition.  The graphs are replayed in interleaved rounds, the order rotating, each timed batch at least --min-time
seconds between HIP events.  Printed per variant: us per launch of the whole batch, median / min / max over the rounds,
and the output bytes per second of the median.
The baseline is a COST baseline only (it is not held to the definition bit for bit):
`render(lanes=chunk)` in chunks below 1 GiB, then `(77 R + 150 G + 29 B + 128) >> 8` and the block mean in torch ops, timed
eagerly between HIP events over --baseline-games games and scaled linearly to n (EXTRAPOLATED, said so in the line).
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "pika-zoo_amd"))
from pikazoo_amd import _native, pikazoo_v0  # noqa: E402
from pikazoo_amd import render as R  # noqa: E402

LAUNCHES = 4  # per captured graph
SCALES = (1, 2, 4, 8)


def judge(env, scale, lanes):
    """The frames of `lanes` by the other route: render() (held to the frame definition by the test suite) and the
    definition's reduction in numpy on the host."""
    return R.gray_downsample(env.render(lanes=lanes).cpu().numpy(), scale)


def played_env(n, dev, sprites):
    env = pikazoo_v0.env(num_envs=n, device=dev, seed=0, render_mode="rgb_array", sprites=sprites)
    env.reset()
    for t in range(3):
        env.step_random(1, k=32)
    return env


def time_fused(lib, dev, n, sprites, args):
    env = played_env(n, dev, sprites)
    side = torch.cuda.Stream()
    lanes = [0, 1, 63, 64, n // 2, n - 66, n - 2, n - 1]
    runs = {}
    for scale in SCALES:
        h, w = R.HEIGHT // scale, R.WIDTH // scale
        for name, fast in ((f"scale {scale} fast", True), (f"scale {scale} composed", False)):
            out = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)

            def body(stream, out=out, fast=fast, scale=scale):
                for _ in range(LAUNCHES):
                    R.render_gray(lib, env._state_buf.data_ptr(), dev, n, env._stride, sprites, None, stream, scale, out=out,
                                  fast_path=fast)

            body(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    body(torch.cuda.current_stream().cuda_stream)
            runs[name] = dict(graph=g, out=out, scale=scale, bytes=n * h * w)
        a, b = runs[f"scale {scale} fast"]["out"], runs[f"scale {scale} composed"]["out"]
        ok = torch.equal(a, b) and np.array_equal(a[lanes].cpu().numpy(), judge(env, scale, lanes))
        runs[f"scale {scale} fast"]["ok"] = runs[f"scale {scale} composed"]["ok"] = ok
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = {}
    for name, r in runs.items():
        with torch.cuda.stream(side):
            e0.record()
            r["graph"].replay()
            e1.record()
        torch.cuda.synchronize()
        reps[name] = max(2, int(args.min_time * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    times = {name: [] for name in runs}
    names = list(runs)
    for rnd in range(args.rounds):
        for name in names[rnd % len(names):] + names[:rnd % len(names)]:
            r = runs[name]
            with torch.cuda.stream(side):
                r["graph"].replay()  # untimed lead-in behind the previous variant
                e0.record()
                for _ in range(reps[name]):
                    r["graph"].replay()
                e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / (reps[name] * LAUNCHES))
    print(f"\n== {n} games: us per launch of the whole batch over {args.rounds} interleaved rounds (each >= {args.min_time} s of "
          f"graph replays)", flush=True)
    med = {}
    for name in names:
        med[name] = statistics.median(times[name])
        print(f"  {name:18s} median {med[name]:10.2f}  min {min(times[name]):10.2f}  max {max(times[name]):10.2f}  "
              f"{med[name] * 1e3 / n:8.2f} ns per game  output {runs[name]['bytes'] / med[name] / 1e3:8.1f} GB/s  "
              f"judged {'ok' if runs[name]['ok'] else 'MISMATCH'}", flush=True)
    assert all(r["ok"] for r in runs.values())
    del runs, env
    torch.cuda.empty_cache()
    return med


def baseline(dev, n_base, sprites, args):
    """us per game of render() in chunks + torch ops, per scale (eager, HIP events, median of the rounds)."""
    env = played_env(n_base, dev, sprites)
    chunk = (1 << 30) // (R.HEIGHT * R.WIDTH * 3)
    chunks = [torch.arange(i, min(i + chunk, n_base), device=dev, dtype=torch.int32) for i in range(0, n_base, chunk)]
    weights = torch.tensor([77, 150, 29], dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def route(scale):
        outs = []
        for lanes in chunks:
            rgb = env.render(lanes=lanes)
            y = ((rgb.to(torch.int32) * weights).sum(dim=-1) + 128) >> 8
            m = y.shape[0]
            s = y.view(m, R.HEIGHT // scale, scale, R.WIDTH // scale, scale).sum(dim=(2, 4))
            outs.append(((s + scale * scale // 2) >> (2 * (scale.bit_length() - 1))).to(torch.uint8))
        return outs

    per_game = {}
    for scale in SCALES:
        route(scale)  # warm up (allocator)
        ts = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            e0.record()
            route(scale)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / n_base)
        per_game[scale] = (statistics.median(ts), min(ts), max(ts))
    del env
    torch.cuda.empty_cache()
    return per_game, len(chunks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.1)
    ap.add_argument("--baseline-games", type=int, default=4096)
    args = ap.parse_args()
    lib = _native.load()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; library build {lib.pz_build_id().decode()}", flush=True)
    sprites = R.synthetic_sprites(0, dev)
    fused = {n: time_fused(lib, dev, n, sprites, args) for n in args.n}
    per_game, n_chunks = baseline(dev, args.baseline_games, sprites, args)
    print(f"\n== baseline: render(lanes=chunk) in {n_chunks} chunks below 1 GiB + torch ops (luma, block mean), eagerly, "
          f"{args.baseline_games} games, {args.rounds} rounds; a cost baseline only", flush=True)
    for scale, (med, lo, hi) in per_game.items():
        print(f"  scale {scale}: median {med:8.3f}  min {lo:8.3f}  max {hi:8.3f} us per game", flush=True)
    for n in args.n:
        print(f"\n== {n} games: fused launch against the baseline scaled linearly from {args.baseline_games} games "
              f"({'measured at this size' if n == args.baseline_games else 'EXTRAPOLATED'})", flush=True)
        for scale in SCALES:
            base = per_game[scale][0] * n
            f = fused[n][f"scale {scale} fast"]
            print(f"  scale {scale}: fused {f:10.2f} us, baseline {base:12.2f} us: {base / f:7.1f} x"
                  f"{'' if f < base else '  ** the fused launch is NOT faster **'}", flush=True)


if __name__ == "__main__":
    main()
