#!/usr/bin/env python3
"""Launch time per observation row format (diagnostic): the seven formats of include/pikazoo_hip.h enum pz_obs_format.

    python tools/time_obs_formats.py [--n 65536 524288] [--rounds 7] [--min-time 0.25]

Human vs human on the on-device random policy's actions, through the C ABI: for every batch size, state format (int32
columns / packed) and launch (`step`: pz_step, one frame per launch, actions cycled from 64 slices; `rollout`:
pz_rollout_random with k = 32, the two trajectory tensors placed like the env places them) each format gets its own
state, buffers and a captured hipGraph of its launches; then the formats' graphs are replayed in interleaved rounds (the
order rotates every round), each replay batch timed with HIP events around at least --min-time seconds.  Printed: us per
frame, median and min over the rounds, and the ratio to int32.  The fused NormalizeObservation formats run with no other
wrapper (normalize_obs alone).
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "pika-zoo_amd"))
from pikazoo_amd import _native, placement  # noqa: E402

FORMATS = (("int32", 0), ("float32-norm", 1), ("int16", 2), ("f16", 3), ("bf16", 4), ("f16-norm", 5), ("bf16-norm", 6))
K = 32
STEP_LAUNCHES = 256   # pz_step launches per captured graph
ROLLOUT_LAUNCHES = 8  # pz_rollout_random launches (of K frames) per captured graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 524288])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.25)
    ap.add_argument("--launch", nargs="+", default=["step", "rollout"], choices=["step", "rollout"])
    ap.add_argument("--state", nargs="+", default=["int32", "packed"], choices=["int32", "packed"])
    args = ap.parse_args()
    lib = _native.load()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; library build {lib.pz_build_id().decode()}", flush=True)
    for n in args.n:
        for state_format in args.state:
            for launch in args.launch:
                time_one(lib, dev, n, state_format, launch, args)


def time_one(lib, dev, n, state_format, launch, args):
    packed = state_format == "packed"
    side = torch.cuda.Stream()
    slices = torch.randint(0, 18, (64, 2, n), dtype=torch.int32, device=dev)
    runs = {}
    for name, fmt in FORMATS:
        cfg = _native.PzConfig()
        cfg.winning_score, cfg.auto_reset, cfg.seed, cfg.x_line, cfg.y_line = 15, 1, 0, 216, 176
        cfg.packed_state, cfg.normalize_obs = int(packed), fmt
        state = (torch.zeros(36 * n, dtype=torch.uint8, device=dev) if packed
                 else torch.zeros((44, n), dtype=torch.int32, device=dev))
        rows = n if fmt < 2 else (n + 1) // 2 * 2
        odt = torch.int32 if fmt < 2 else torch.int16
        obs = [torch.zeros((rows, 35), dtype=odt, device=dev) for _ in range(2)]
        rew = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
        term = torch.zeros(n, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        assert lib.pz_init(state.data_ptr(), n, n, C.byref(cfg), stream) == 0
        assert lib.pz_reset(state.data_ptr(), n, n, C.byref(cfg), None, obs[0].data_ptr(), obs[1].data_ptr(), None,
                            stream) == 0
        r = dict(cfg=cfg, state=state, obs=obs, rew=rew, term=term)
        if launch == "rollout":
            r["t_obs"] = list(placement.alloc_pair((K, n, 35), odt, dev))
            r["t_rew"] = [torch.zeros((K, n), dtype=torch.int32, device=dev) for _ in range(2)]
            r["t_term"] = torch.zeros((K, n), dtype=torch.uint8, device=dev)
            r["t_act"] = torch.zeros((K, 2, n), dtype=torch.int32, device=dev)

        def body(stream, r=r):
            cfg, st = C.byref(r["cfg"]), r["state"].data_ptr()
            if launch == "step":
                for t in range(STEP_LAUNCHES):
                    a = slices[t % 64]
                    rc = lib.pz_step(st, n, n, cfg, a[0].data_ptr(), a[1].data_ptr(), r["obs"][0].data_ptr(),
                                     r["obs"][1].data_ptr(), r["rew"][0].data_ptr(), r["rew"][1].data_ptr(),
                                     r["term"].data_ptr(), None, None, stream)
                    assert rc == 0, rc
                return STEP_LAUNCHES
            for j in range(ROLLOUT_LAUNCHES):
                rc = lib.pz_rollout_random(st, n, n, cfg, 7, j * K, K, r["t_act"].data_ptr(), r["t_obs"][0].data_ptr(),
                                           r["t_obs"][1].data_ptr(), r["t_rew"][0].data_ptr(), r["t_rew"][1].data_ptr(),
                                           r["t_term"].data_ptr(), None, None, None, stream)
                assert rc == 0, rc
            return ROLLOUT_LAUNCHES * K

        body(torch.cuda.current_stream().cuda_stream)  # warm up (and settle the games past their opening)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                r["frames"] = body(torch.cuda.current_stream().cuda_stream)
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
                r["graph"].replay()  # untimed lead-in behind the previous format
                e0.record()
                for _ in range(reps[name]):
                    r["graph"].replay()
                e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / (reps[name] * r["frames"]))
    what = f"pz_step (1 frame per launch)" if launch == "step" else f"pz_rollout_random k={K}"
    print(f"\n== {n} games, {state_format} state, human vs human, {what}: us per frame over {args.rounds} interleaved "
          f"rounds (each >= {args.min_time} s of graph replays)", flush=True)
    base = statistics.median(times["int32"])
    for name in names:
        med, lo = statistics.median(times[name]), min(times[name])
        print(f"  {name:13s} median {med:7.3f}  min {lo:7.3f}  vs int32 {med / base:6.3f}", flush=True)
    del runs
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
