#!/usr/bin/env python3
"""What a trajectory of held actions costs (diagnostic): pz_rollout_random_held / pz_step_many_held against k launches
of pz_step_held, the only way to get such a trajectory without them.

    python tools/time_held_rollout.py [--n 65536 524288] [--hold 2 4 8] [--k 32] [--rounds 7] [--min-time 0.1]

Per batch size, player mix (human vs human; config 3: player 2 the computer, both flight tables) and state format:
  rollout / many            pz_rollout_random / pz_step_many at k: us per FRAME, the ceiling of a frame_skip=1 user;
and for every hold, us per POLICY STEP (hold frames on one pair of actions):
  held x k                  k launches of pz_step_held(hold), one set of outputs each;
  rollout_held / many_held  ONE launch of pz_rollout_random_held / pz_step_many_held(k, hold), k slabs of outputs.
Each variant has its own state and buffers and a captured hipGraph of one k-step trajectory; the graphs of one row are
replayed in interleaved rounds, the order rotating, each timed batch at least --min-time seconds between HIP events.
Before it is timed every variant runs its trajectory once from reset and is compared with the judge of the tests on the
first 256 games (tests/frame_skip_judge.py through tests/held_timing_judge.py: every slab it writes, the final state); a
variant that fails is not timed.
A new launch passes when its median is below the `held x k` median by more than that figure's own spread (max - min).
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests"):
    sys.path.insert(0, str(p))
from held_timing_judge import timing_judge  # noqa: E402  (tests/: the tools never link the judge themselves)
from pikazoo_amd import _native  # noqa: E402
from pikazoo_amd import env as pz_env  # noqa: E402

MIXES = (("human vs human", False), ("config 3 (player 2 computer, both tables)", True))
CHECKED = 256  # games compared with the oracle
SEED = 5       # of the on-device policy


class Variant:
    def __init__(self, lib, dev, name, n, k, hold, computer, packed, slices, tref):
        self.lib, self.name, self.n, self.k, self.hold, self.packed, self.tref = lib, name, n, k, hold, packed, tref
        self.traj = name != "held x k"
        self.frames = hold if name in ("held x k", "rollout_held", "many_held") else 1  # per policy step
        self.slices = slices  # int32[k][2][n]: the tape / the action vectors of the k policy steps
        cfg = self.cfg = _native.PzConfig()
        cfg.winning_score, cfg.auto_reset, cfg.seed, cfg.x_line, cfg.y_line = 15, 1, 0, 216, 176
        cfg.packed_state, cfg.p2_computer = int(packed), int(computer)
        self.state = (torch.zeros(36 * n, dtype=torch.uint8, device=dev) if packed
                      else torch.zeros((44, n), dtype=torch.int32, device=dev))
        slabs = k if self.traj else 1
        self.obs = [torch.zeros((slabs, n, 35), dtype=torch.int32, device=dev) for _ in range(2)]
        self.rew = [torch.zeros((slabs, n), dtype=torch.int32, device=dev) for _ in range(2)]
        self.term = torch.zeros((slabs, n), dtype=torch.uint8, device=dev)
        self.act = torch.zeros((k, 2, n), dtype=torch.int32, device=dev) if name.startswith("rollout") else None
        self.unpacked = torch.zeros((44, CHECKED), dtype=torch.int32, device=dev)

    def reset(self, stream):
        st, cfg = self.state.data_ptr(), C.byref(self.cfg)
        assert self.lib.pz_init(st, self.n, self.n, cfg, stream) == 0
        assert self.lib.pz_reset(st, self.n, self.n, cfg, None, self.obs[0].data_ptr(), self.obs[1].data_ptr(), None,
                                 stream) == 0

    def body(self, stream):
        lib, n, k, cfg, st = self.lib, self.n, self.k, C.byref(self.cfg), self.state.data_ptr()
        out = (self.obs[0].data_ptr(), self.obs[1].data_ptr(), self.rew[0].data_ptr(), self.rew[1].data_ptr(),
               self.term.data_ptr())
        tail = (None, None, self.tref, stream)
        if self.name == "held x k":
            rc = 0
            for t in range(k):
                a = self.slices[t]
                rc = rc or lib.pz_step_held(st, n, n, cfg, a[0].data_ptr(), a[1].data_ptr(), self.hold, *out, *tail)
        elif self.name == "rollout_held":
            rc = lib.pz_rollout_random_held(st, n, n, cfg, SEED, 0, k, self.hold, self.act.data_ptr(), *out, *tail)
        elif self.name == "many_held":
            rc = lib.pz_step_many_held(st, n, n, cfg, self.slices.data_ptr(), k, self.hold, *out, *tail)
        elif self.name == "rollout":
            rc = lib.pz_rollout_random(st, n, n, cfg, SEED, 0, k, self.act.data_ptr(), *out, *tail)
        else:
            rc = lib.pz_step_many(st, n, n, cfg, self.slices.data_ptr(), k, *out, *tail)
        assert rc == 0, (self.name, rc)

    def first_games(self, stream):
        """the int32 columns of the first CHECKED games"""
        if not self.packed:
            return self.state[:, :CHECKED].cpu().numpy()
        flagged = torch.zeros(1, dtype=torch.int64, device=self.state.device)
        assert self.lib.pz_unpack_state(self.state.data_ptr(), CHECKED, self.n, self.unpacked.data_ptr(), CHECKED,
                                        flagged.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert int(flagged.item()) == 0
        return self.unpacked.cpu().numpy()

    def check(self, stream):
        """one trajectory from reset against the judge on the first CHECKED games"""
        m, k = CHECKED, self.k
        judge, policy = timing_judge(m, self.frames, bool(self.cfg.p2_computer), SEED)
        self.reset(stream)
        torch.cuda.synchronize()
        assert np.array_equal(self.first_games(stream), judge.state), (self.name, "state after reset")
        self.body(stream)
        torch.cuda.synchronize()
        tape = self.slices[:, :, :m].cpu().numpy()
        for t in range(k):
            a1, a2 = policy(t) if self.act is not None else (tape[t, 0], tape[t, 1])
            robs, rrew, rterm = judge.step(a1, a2)
            if self.traj or t == k - 1:
                s = t if self.traj else 0
                for p in range(2):
                    assert np.array_equal(self.obs[p][s, :m].cpu().numpy(), robs[p]), (self.name, t, "observations")
                    assert np.array_equal(self.rew[p][s, :m].cpu().numpy(), rrew[p]), (self.name, t, "rewards")
                assert np.array_equal(self.term[s, :m].cpu().numpy(), rterm), (self.name, t, "terminated")
            if self.act is not None:
                assert np.array_equal(self.act[t, 0, :m].cpu().numpy(), a1), (self.name, t, "actions")
        assert np.array_equal(self.first_games(stream), judge.state), (self.name, "final state")


def time_row(lib, dev, n, mix, computer, state_format, holds, args):
    packed, k = state_format == "packed", args.k
    side = torch.cuda.Stream()
    slices = torch.randint(0, 18, (k, 2, n), dtype=torch.int32, device=dev)
    tables = pz_env.flight_tables(dev) if computer else None
    tref = C.byref(tables[0]) if computer else None
    names = [("rollout", 1), ("many", 1)] + [(v, h) for h in holds for v in ("held x k", "rollout_held", "many_held")]
    runs = {}
    for name, hold in names:
        v = Variant(lib, dev, name, n, k, hold, computer, packed, slices, tref)
        stream = torch.cuda.current_stream().cuda_stream
        v.check(stream)
        for _ in range(2):
            v.body(stream)  # warm up (and settle the games past their opening)
        torch.cuda.synchronize()
        v.graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(v.graph, stream=side):
                v.body(torch.cuda.current_stream().cuda_stream)
        runs[(name, hold)] = v
    torch.cuda.synchronize()
    print(f"\n== {n} games, {mix}, {state_format} state, k = {k}: every variant below matched the oracle on its first "
          f"{CHECKED} games; {args.rounds} interleaved rounds (each >= {args.min_time} s of graph replays)", flush=True)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = {}
    for key, v in runs.items():
        with torch.cuda.stream(side):
            e0.record()
            v.graph.replay()
            e1.record()
        torch.cuda.synchronize()
        reps[key] = max(2, int(args.min_time * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    times = {key: [] for key in runs}
    keys = list(runs)
    for rnd in range(args.rounds):
        for key in keys[rnd % len(keys):] + keys[:rnd % len(keys)]:
            v = runs[key]
            with torch.cuda.stream(side):
                v.graph.replay()  # untimed lead-in behind the previous variant
                e0.record()
                for _ in range(reps[key]):
                    v.graph.replay()
                e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e3 / (reps[key] * k))
    med = {key: statistics.median(times[key]) for key in keys}
    failed = []
    for (name, hold) in keys:
        ts = times[(name, hold)]
        unit = "frame" if hold == 1 and name in ("rollout", "many") else f"policy step of {hold} frames"
        line = f"  {name:12s} hold {hold}: median {med[(name, hold)]:8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f} us per {unit}"
        if name in ("rollout_held", "many_held"):
            base = times[("held x k", hold)]
            spread = max(base) - min(base)
            saved = med[("held x k", hold)] - med[(name, hold)]
            ok = saved > spread
            line += (f"; per frame {med[(name, hold)] / hold:6.3f}; vs held x k {saved:+.3f} us saved, its spread {spread:.3f} -> "
                     f"{'faster' if ok else 'NOT faster by more than the spread'}")
            if not ok:
                failed.append((n, mix, state_format, name, hold))
        print(line, flush=True)
    del runs
    torch.cuda.empty_cache()
    return failed


def registers(lib_path):
    """what the two held kernel families occupy (code-object notes; skipped where the ROCm LLVM tools are missing)"""
    try:
        sys.path.insert(0, str(REPO / "tools"))
        import kernel_notes

        rows = [(name.split("(")[0].replace("void pz::", ""), r) for name, r in kernel_notes.notes(Path(lib_path))]
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
        return
    for family in ("hold_kernel<", "held_traj_kernel<false, false, 2", "held_traj_kernel<false, false, 3",
                   "held_traj_kernel<false, true, 2", "held_traj_kernel<false, true, 3", "held_traj_kernel<"):
        mine = [r for name, r in rows if name.startswith(family)]
        span = lambda key: f"{min(r[key] for r in mine)}-{max(r[key] for r in mine)}"  # noqa: E731
        print(f"  {family + '...>':36s} {len(mine):2d} kernels: VGPRs {span('.vgpr_count')}, spilled SGPRs "
              f"{span('.sgpr_spill_count')}, spilled VGPRs {span('.vgpr_spill_count')}, scratch bytes "
              f"{span('.private_segment_fixed_size')}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 524288])
    ap.add_argument("--hold", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.1)
    args = ap.parse_args()
    lib = _native.load()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(dev)}; library build {lib.pz_build_id().decode()}", flush=True)
    registers(_native.LIB_PATH)
    failed = []
    for n in args.n:
        for mix, computer in MIXES:
            for state_format in ("int32", "packed"):
                failed += time_row(lib, dev, n, mix, computer, state_format, args.hold, args)
    print(f"\nrows where a held trajectory launch is NOT faster than k pz_step_held launches by more than their spread: "
          f"{failed or 'none'}", flush=True)


if __name__ == "__main__":
    main()
