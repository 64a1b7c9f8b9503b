#!/usr/bin/env python3
"""What an action repeat costs (diagnostic): pz_step_held(k) against the two ways to hold an action without it.

    python tools/time_frame_skip.py [--n 65536 524288] [--k 1 2 4 8] [--rounds 7] [--min-time 0.15] [--no-eager]

Per batch size, player mix (human vs human; config 3: player 2 the computer, both flight tables) and state format, for
every k three variants run one POLICY STEP -- the same two action vectors for k frames -- through the C ABI:
  held   pz_step_held(k): one launch, one set of outputs (the rewards summed);
  steps  k launches of pz_step on the same actions: the only way to get these outputs without pz_step_held;
  many   pz_step_many on a tape of k identical slices: one launch that writes all k output sets (NOT equivalent: it is
         the bandwidth yardstick).
Each variant has its own state and buffers and a captured hipGraph of 32 policy steps (actions cycled from 64 slices);
the graphs of one k are replayed in interleaved rounds, the order rotating, each timed batch at least --min-time
seconds between HIP events.  Printed per variant: us per policy step, median / min / max over the rounds; `held` passes
when its median is below the `steps` median by more than that figure's own run-to-run spread (max - min).
Then, through the env API without a graph: env.step() with frame_skip=4 against four eager step() calls on a twin env.
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "pika-zoo_amd"))
from pikazoo_amd import _native, pikazoo_v0  # noqa: E402
from pikazoo_amd import env as pz_env  # noqa: E402

POLICY_STEPS = 32  # per captured graph
MIXES = (("human vs human", False), ("config 3 (player 2 computer, both tables)", True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 524288])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.15)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    lib = _native.load()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; library build {lib.pz_build_id().decode()}", flush=True)
    failed = []
    for n in args.n:
        for mix, computer in MIXES:
            for state_format in ("int32", "packed"):
                for k in args.k:
                    ok = time_one(lib, dev, n, mix, computer, state_format, k, args)
                    if k >= 2 and not ok:
                        failed.append((n, mix, state_format, k))
    print(f"\nrows where pz_step_held(k >= 2) is NOT faster than k pz_step launches by more than their spread: {failed or 'none'}",
          flush=True)
    if not args.no_eager:
        eager(dev, args)


def time_one(lib, dev, n, mix, computer, state_format, k, args):
    packed = state_format == "packed"
    side = torch.cuda.Stream()
    slices = torch.randint(0, 18, (64, 2, n), dtype=torch.int32, device=dev)
    tapes = slices[:, None].expand(64, k, 2, n).contiguous() if k * n <= 8 * 524288 else None
    tables = pz_env.flight_tables(dev) if computer else None
    tref = C.byref(tables[0]) if computer else None
    runs = {}
    for name in ("held", "steps", "many"):
        cfg = _native.PzConfig()
        cfg.winning_score, cfg.auto_reset, cfg.seed, cfg.x_line, cfg.y_line = 15, 1, 0, 216, 176
        cfg.packed_state, cfg.p2_computer = int(packed), int(computer)
        state = (torch.zeros(36 * n, dtype=torch.uint8, device=dev) if packed
                 else torch.zeros((44, n), dtype=torch.int32, device=dev))
        frames = k if name == "many" else 1
        obs = [torch.zeros((frames, n, 35), dtype=torch.int32, device=dev) for _ in range(2)]
        rew = [torch.zeros((frames, n), dtype=torch.int32, device=dev) for _ in range(2)]
        term = torch.zeros((frames, n), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        assert lib.pz_init(state.data_ptr(), n, n, C.byref(cfg), stream) == 0
        assert lib.pz_reset(state.data_ptr(), n, n, C.byref(cfg), None, obs[0].data_ptr(), obs[1].data_ptr(), None,
                            stream) == 0
        r = dict(cfg=cfg, state=state, obs=obs, rew=rew, term=term)

        def body(stream, r=r, name=name):
            cfg, st = C.byref(r["cfg"]), r["state"].data_ptr()
            out = (r["obs"][0].data_ptr(), r["obs"][1].data_ptr(), r["rew"][0].data_ptr(), r["rew"][1].data_ptr(),
                   r["term"].data_ptr())
            for t in range(POLICY_STEPS):
                a = slices[t % 64]
                if name == "held":
                    rc = lib.pz_step_held(st, n, n, cfg, a[0].data_ptr(), a[1].data_ptr(), k, *out, None, None, tref, stream)
                elif name == "steps":
                    rc = 0
                    for _ in range(k):
                        rc = rc or lib.pz_step(st, n, n, cfg, a[0].data_ptr(), a[1].data_ptr(), *out, None, tref, stream)
                else:
                    rc = lib.pz_step_many(st, n, n, cfg, tapes[t % 64].data_ptr(), k, *out, None, None, tref, stream)
                assert rc == 0, (name, rc)

        for _ in range(3):
            body(torch.cuda.current_stream().cuda_stream)  # warm up (and settle the games past their opening)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                body(torch.cuda.current_stream().cuda_stream)
        r["graph"] = g
        runs[name] = r
    torch.cuda.synchronize()

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = {}
    for name, r in runs.items():  # replays per timed batch: at least min_time seconds
        with torch.cuda.stream(side):
            e0.record()
            r["graph"].replay()
            e1.record()
        torch.cuda.synchronize()
        reps[name] = max(2, int(args.min_time * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    times = {name: [] for name in runs}
    names = list(runs)
    for rnd in range(args.rounds):
        order = names[rnd % len(names):] + names[:rnd % len(names)]
        for name in order:
            r = runs[name]
            with torch.cuda.stream(side):
                r["graph"].replay()  # untimed lead-in behind the previous variant
                e0.record()
                for _ in range(reps[name]):
                    r["graph"].replay()
                e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / (reps[name] * POLICY_STEPS))
    print(f"\n== {n} games, {mix}, {state_format} state, k = {k}: us per policy step ({k} frames) over {args.rounds} "
          f"interleaved rounds (each >= {args.min_time} s of graph replays)", flush=True)
    med = {name: statistics.median(times[name]) for name in names}
    for name in names:
        lo, hi = min(times[name]), max(times[name])
        print(f"  {name:5s} median {med[name]:8.3f}  min {lo:8.3f}  max {hi:8.3f}  vs steps {med[name] / med['steps']:6.3f}"
              f"  per frame {med[name] / k:7.3f}", flush=True)
    spread = max(times["steps"]) - min(times["steps"])
    ok = med["held"] < med["steps"] - spread
    print(f"  held vs steps: {med['steps'] - med['held']:+.3f} us saved, spread of steps {spread:.3f} us -> "
          f"{'faster' if ok else 'NOT faster by more than the spread'}", flush=True)
    del runs
    torch.cuda.empty_cache()
    return ok


def eager(dev, args, n=65536, k=4, steps=1500):
    print(f"\n== env.step() eagerly, {n} games, int32 state: frame_skip={k} against {k} step() calls per policy step "
          f"(host clock around {steps} policy steps ending in a synchronise), {args.rounds} interleaved rounds", flush=True)
    for mix, computer in MIXES:
        envs = {"frame_skip": pikazoo_v0.env(num_envs=n, device=dev, is_player2_computer=computer, frame_skip=k),
                "k calls": pikazoo_v0.env(num_envs=n, device=dev, is_player2_computer=computer)}
        acts = [{"player_1": torch.randint(0, 18, (n,), dtype=torch.int32, device=dev),
                 "player_2": torch.randint(0, 18, (n,), dtype=torch.int32, device=dev)} for _ in range(16)]
        times = {name: [] for name in envs}
        for name, env in envs.items():
            env.reset()
        for rnd in range(args.rounds + 1):  # (round 0 warms up)
            for name in (list(envs) if rnd % 2 else list(envs)[::-1]):
                env = envs[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(steps):
                    for _ in range(1 if name == "frame_skip" else k):
                        env.step(acts[t % 16])
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e6 / steps)
        for name in envs:
            print(f"  {mix:42s} {name:10s} median {statistics.median(times[name]):8.3f}  min {min(times[name]):8.3f}  "
                  f"max {max(times[name]):8.3f} us per policy step", flush=True)


if __name__ == "__main__":
    main()
