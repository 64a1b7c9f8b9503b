#!/usr/bin/env python3
"""What per-game computer players cost (diagnostic): pz_step_mixed against pz_step and against the sorted-batch split.

    python tools/time_mixed_step.py [--n 65536 524288] [--rounds 7] [--min-time 0.15] [--no-eager]

Per batch size and state format, both flight tables, one frame per launch through the C ABI:
  mixed 0 / 2 / 3   pz_step_mixed with every role code 0 (nobody) / 2 (player 2) / 3 (both) the computer;
  mixed 50%         pz_step_mixed, bit 1 set on a random half of the games;
  step hvh / cfg3 / both   pz_step with cfg's flags: human vs human, player 2 the computer, both;
  split             what a caller can do today for that half-and-half batch: the batch sorted by opponent in two state
                    tensors of n / 2 games, one pz_step launch each (human vs human, config 3).
Each variant has its own state and buffers and a captured hipGraph of 32 frames (actions cycled from 64 slices), all on the
same seed, game ids and action slices.  Before it is timed, every variant's first 32 frames are judged in the run against
the pz_step runs (the test suite holds those to the CPU oracle): the whole state and the last frame's outputs of mixed 0 /
2 / 3 equal step hvh / cfg3 / both; of mixed 50% lane by lane step hvh (role code 0) or step cfg3 (role code 2); of the
split's two halves the same lanes of step hvh and step cfg3.  The graphs are then replayed in interleaved rounds, the order
rotating, each timed batch at least --min-time seconds between HIP events.  Printed per variant: us per launch, median /
min / max over the rounds, and the ratio to the pz_step figure it is judged against with that figure's spread (max - min).
Then, through the env API without a graph: env.step() on a mixed env (50 % mask) against a uniform config-3 env and a
uniform human-vs-human env.
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "pika-zoo_amd"))
from pikazoo_amd import _native, pikazoo_v0  # noqa: E402
from pikazoo_amd import env as pz_env  # noqa: E402

FRAMES = 32  # per captured graph
SLICE = 512
# variant -> (entry, role code of every game or None, the pz_step variant it is judged against)
VARIANTS = {"mixed 0": ("mixed", 0, "step hvh"), "mixed 2": ("mixed", 2, "step cfg3"), "mixed 3": ("mixed", 3, "step both"),
            "mixed 50%": ("mixed", None, "split"), "step hvh": ("step", 0, None), "step cfg3": ("step", 2, None),
            "step both": ("step", 3, None), "split": ("split", None, None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 524288])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.15)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    lib = _native.load()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; library build {lib.pz_build_id().decode()}", flush=True)
    for n in args.n:
        for state_format in ("int32", "packed"):
            time_one(lib, dev, n, state_format, args)
    if not args.no_eager:
        eager(dev, args)


def make_state(lib, dev, n, packed, code, base, stream):
    cfg = _native.PzConfig()
    cfg.winning_score, cfg.auto_reset, cfg.seed, cfg.x_line, cfg.y_line = 15, 1, 0, 216, 176
    cfg.packed_state, cfg.env_id_base = int(packed), base
    cfg.p1_computer, cfg.p2_computer = code & 1, (code >> 1) & 1
    state = (torch.zeros(36 * n, dtype=torch.uint8, device=dev) if packed else torch.zeros((44, n), dtype=torch.int32, device=dev))
    obs = [torch.zeros((n, 35), dtype=torch.int32, device=dev) for _ in range(2)]
    rew = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
    term = torch.zeros(n, dtype=torch.uint8, device=dev)
    assert lib.pz_init(state.data_ptr(), n, n, C.byref(cfg), stream) == 0
    assert lib.pz_reset(state.data_ptr(), n, n, C.byref(cfg), None, obs[0].data_ptr(), obs[1].data_ptr(), None, stream) == 0
    return dict(cfg=cfg, state=state, out=(obs[0], obs[1], rew[0], rew[1], term), n=n)


def snapshot(lib, dev, parts, packed, stream):
    """What a variant holds after its first FRAMES frames, by global lane: the state as int32[44, n] and the last frame's
    five outputs (a split's two halves side by side)."""
    states = []
    for p in parts:
        state = p["state"]
        if packed:
            flat = torch.zeros((44, p["n"]), dtype=torch.int32, device=dev)
            flagged = torch.zeros(1, dtype=torch.int64, device=dev)
            assert lib.pz_unpack_state(state.data_ptr(), p["n"], p["n"], flat.data_ptr(), p["n"], flagged.data_ptr(), stream) == 0
            state = flat
        states.append(state.clone())
    return [torch.cat(states, dim=1)] + [torch.cat([p["out"][k] for p in parts], dim=0).clone() for k in range(5)]


def judge(snaps, name, codes):
    """Variant `name` against the pz_step runs: lane l equals the run with the flags of its role code codes[l]."""
    ref = {0: snaps["step hvh"], 2: snaps["step cfg3"], 3: snaps["step both"]}
    ok = True
    for code in np.unique(codes):
        lanes = torch.from_numpy(codes == code).to(snaps[name][0].device)
        ok &= bool((snaps[name][0][:, lanes] == ref[int(code)][0][:, lanes]).all())
        ok &= all(bool((got[lanes] == want[lanes]).all()) for got, want in zip(snaps[name][1:], ref[int(code)][1:]))
    return ok


def time_one(lib, dev, n, state_format, args):
    packed = state_format == "packed"
    half = n // 2
    side = torch.cuda.Stream()
    stream0 = torch.cuda.current_stream().cuda_stream
    slices = torch.randint(0, 18, (64, 2, n), dtype=torch.int32, device=dev)
    tables = pz_env.flight_tables(dev)
    tref = C.byref(tables[0])
    rng = np.random.default_rng(n)
    runs, snaps, codes_of = {}, {}, {}
    for name, (entry, code, _) in VARIANTS.items():
        if entry == "split":  # the sorted batch: games [0, n/2) human vs human, [n/2, n) against the computer
            parts = [dict(make_state(lib, dev, half, packed, 0, 0, stream0), lane0=0, codes=np.zeros(half, np.uint8)),
                     dict(make_state(lib, dev, half, packed, 2, half, stream0), lane0=half, codes=np.full(half, 2, np.uint8))]
        else:
            codes = np.full(n, code, np.uint8) if code is not None else (rng.permutation(n) < half).astype(np.uint8) * 2
            part = dict(make_state(lib, dev, n, packed, code if entry == "step" else 0, 0, stream0), lane0=0, codes=codes)
            part["mask"] = torch.from_numpy(codes).to(dev)
            parts = [part]

        def body(stream, parts=parts, entry=entry):
            for t in range(FRAMES):
                for p in parts:
                    a = slices[t % 64][:, p["lane0"]:p["lane0"] + p["n"]]
                    out = [o.data_ptr() for o in p["out"]]
                    if entry == "mixed":
                        rc = lib.pz_step_mixed(p["state"].data_ptr(), p["n"], p["n"], C.byref(p["cfg"]), p["mask"].data_ptr(),
                                               a[0].data_ptr(), a[1].data_ptr(), *out, None, tref, stream)
                    else:
                        rc = lib.pz_step(p["state"].data_ptr(), p["n"], p["n"], C.byref(p["cfg"]), a[0].data_ptr(),
                                         a[1].data_ptr(), *out, None, tref, stream)
                    assert rc == 0, (entry, rc)

        body(stream0)  # the first FRAMES frames: judged below, once the pz_step runs are there
        snaps[name] = snapshot(lib, dev, parts, packed, stream0)
        codes_of[name] = np.concatenate([p["codes"] for p in parts])
        for _ in range(2):
            body(stream0)  # warm up (and settle the games past their opening)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                body(torch.cuda.current_stream().cuda_stream)
        runs[name] = dict(parts=parts, graph=g)
    torch.cuda.synchronize()
    judged = {name: judge(snaps, name, codes_of[name]) for name in runs if VARIANTS[name][0] != "step"}
    del snaps

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
            times[name].append(e0.elapsed_time(e1) * 1e3 / (reps[name] * FRAMES))
    print(f"\n== {n} games, {state_format} state, both flight tables: us per frame of the whole batch over {args.rounds} interleaved "
          f"rounds (each >= {args.min_time} s of graph replays)", flush=True)
    med = {name: statistics.median(times[name]) for name in names}
    for name in names:
        lo, hi = min(times[name]), max(times[name])
        against = VARIANTS[name][2]
        ratio = ""
        if against is not None:
            spread = max(times[against]) - min(times[against])
            ratio = f"  vs {against:9s} {med[name] / med[against]:6.3f} ({med[name] - med[against]:+.3f} us; its spread {spread:.3f})"
        verdict = "the reference " if name not in judged else f"judged {'ok' if judged[name] else 'MISMATCH'}"
        print(f"  {name:10s} median {med[name]:8.3f}  min {lo:8.3f}  max {hi:8.3f}  {verdict}{ratio}",
              flush=True)
    assert all(judged.values()), judged
    del runs
    torch.cuda.empty_cache()


def eager(dev, args, n=65536, steps=1500):
    print(f"\n== env.step() eagerly, {n} games, int32 state (host clock around {steps} steps ending in a synchronise), "
          f"{args.rounds} interleaved rounds", flush=True)
    half = (np.random.default_rng(n).permutation(n) < n // 2)
    envs = {"mixed env, 50 % mask": pikazoo_v0.env(num_envs=n, device=dev, is_player2_computer=half),
            "uniform env, config 3": pikazoo_v0.env(num_envs=n, device=dev, is_player2_computer=True),
            "uniform env, human vs human": pikazoo_v0.env(num_envs=n, device=dev)}
    acts = [{"player_1": torch.randint(0, 18, (n,), dtype=torch.int32, device=dev),
             "player_2": torch.randint(0, 18, (n,), dtype=torch.int32, device=dev)} for _ in range(16)]
    times = {name: [] for name in envs}
    for env in envs.values():
        env.reset()
    for rnd in range(args.rounds + 1):  # (round 0 warms up)
        for name in (list(envs) if rnd % 2 else list(envs)[::-1]):
            env = envs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(steps):
                env.step(acts[t % 16])
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e6 / steps)
    for name in envs:
        print(f"  {name:28s} median {statistics.median(times[name]):8.3f}  min {min(times[name]):8.3f}  "
              f"max {max(times[name]):8.3f} us per step", flush=True)


if __name__ == "__main__":
    main()
