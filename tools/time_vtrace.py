#!/usr/bin/env python3
"""What V-trace targets over the trajectory tensors cost (diagnostic): pz_vtrace against the torch loop it replaces, pz_gae
on the same rewards and values, and a copy.

    python tools/time_vtrace.py [--rounds 7] [--min-time 0.05] [--cells 65536x32 65536x128 524288x32 4096x128]

Per cell (games x rows; both agents; float32 rewards and values, plus one row each with int32 rewards and with bfloat16
values at the first cell), five variants, interleaved in one process over --rounds rounds, the order rotating:
  pz_vtrace     ONE launch (pikazoo_amd.vtrace.targets into its previous result), replayed as a hipGraph;
  torch eager   the straightforward loop of torch operations (an exp, three clamps and k dependent iterations of two
                recurrences per agent) into preallocated outputs;
  torch graph   the same loop captured into a hipGraph: its best case, no host in the way;
  pz_gae        pikazoo_amd.learn.gae on the same rewards, values and flags, as a hipGraph: what the on-policy targets cost;
  copy          a device-to-device copy moving the same number of bytes (half read, half written): the streaming floor.
Every tensor a graph reads or writes stays alive until the cell is done.  Before it is timed every variant is compared with the
judge of the tests (tests/vtrace_judge.py) on the first and the last 2 048 games: pz_vtrace and the torch loop against the
float64 formula within the tolerance derived there per element (the torch loop's order of operations is not the header's, so
its bound is taken twice), pz_gae bit for bit against its own judge.  A variant that fails is not timed.  Reported: median and
spread (max - min) in us per call, the algorithmic bytes (every input and output element once: 49 per game-step for both
agents at float32, against GAE's 33.25) over the median in GB/s, that rate as a share of the 6.3 TB/s a streaming kernel
achieves on the MI355X, and pz_vtrace's time over the copy's and over pz_gae's.  A cell where pz_vtrace's median is not below
the captured torch loop's is marked *slower*.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
import gae_judge as GJ  # noqa: E402
import vtrace_judge as J  # noqa: E402  (tests/: the definition in numpy)
from pikazoo_amd import learn, vtrace  # noqa: E402

GAMMA, LAM = 0.99, 0.95
CLIPS = (1.0, 1.0, 1.0)
ACHIEVABLE = 6.3e12  # bytes per second of a streaming kernel on the MI355X
CHECKED = 2048
AGENTS = ("player_1", "player_2")
TORCH_VALUE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def torch_loop(rew, val, notdone, lpb, lpt, pg_adv, vs):
    """the loop a trainer would carry: per agent an exp, three clamps and k dependent iterations of small elementwise launches"""
    gl = GAMMA * LAM
    for a in AGENTS:
        r, v = rew[a].float(), val[a].float()  # (no-ops on float32)
        w = torch.exp(lpt[a] - lpb[a])
        rho, c, pg = w.clamp(max=CLIPS[0]), w.clamp(max=CLIPS[1]), w.clamp(max=CLIPS[2])
        acc = torch.zeros_like(r[0])
        for t in range(r.shape[0] - 1, -1, -1):
            m = notdone[t]
            delta = r[t] + GAMMA * v[t + 1] * m - v[t]
            pg_adv[a][t] = pg[t] * (delta + gl * m * acc)
            acc = rho[t] * delta + gl * c[t] * m * acc
            vs[a][t] = acc
        vs[a].add_(v[:-1])


def time_cell(n, k, reward_dtype, value_dtype, args):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng([n, k])
    d_h = (rng.random((k, n)) < 0.02).astype(np.uint8)
    rew_h, val_h, lpb_h, lpt_h = {}, {}, {}, {}
    for a in AGENTS:
        r = rng.integers(-1, 2, size=(k, n)).astype(np.int32)
        rew_h[a] = r if reward_dtype == "int32" else (r + rng.choice(np.array([0.0, 0.01, -0.01], np.float32), size=(k, n))).astype(np.float32)
        val_h[a] = GJ.as_value_dtype(rng.normal(0.0, 1.5, size=(k + 1, n)).astype(np.float32), value_dtype)
        lpb_h[a] = (-rng.uniform(0.05, 5.0, size=(k, n))).astype(np.float32)
        lpt_h[a] = (lpb_h[a] + rng.normal(0.0, 0.5, size=(k, n)).astype(np.float32)).astype(np.float32)
    rew = {a: torch.from_numpy(rew_h[a]).to(dev) for a in AGENTS}
    val = {a: torch.from_numpy(val_h[a]).to(dev).to(TORCH_VALUE[value_dtype]) for a in AGENTS}
    lpb = {a: torch.from_numpy(lpb_h[a]).to(dev) for a in AGENTS}
    lpt = {a: torch.from_numpy(lpt_h[a]).to(dev) for a in AGENTS}
    done = torch.from_numpy(d_h).to(dev).view(torch.bool)
    notdone = (~done).float()
    outs = {name: {key: {a: torch.empty((k, n), dtype=torch.float32, device=dev) for a in AGENTS} for key in ("advantages", "returns")}
            for name in ("pz_vtrace", "torch eager", "torch graph", "pz_gae")}
    value_bytes = 4 if value_dtype == "float32" else 2
    total = 2 * (k * n * 4 + (k + 1) * n * value_bytes + 2 * k * n * 4 + 2 * k * n * 4) + k * n  # both agents + the shared flags
    total_gae = total - 2 * 2 * k * n * 4
    src, dst = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)

    bodies = {
        "pz_vtrace": lambda: vtrace.targets(rew, val, done, lpb, lpt, GAMMA, LAM, *CLIPS, out=outs["pz_vtrace"]),
        "torch eager": lambda: torch_loop(rew, val, notdone, lpb, lpt, outs["torch eager"]["advantages"], outs["torch eager"]["returns"]),
        "torch graph": lambda: torch_loop(rew, val, notdone, lpb, lpt, outs["torch graph"]["advantages"], outs["torch graph"]["returns"]),
        "pz_gae": lambda: learn.gae(rew, val, done, GAMMA, LAM, out=outs["pz_gae"]),
        "copy": lambda: dst.copy_(src),
    }
    # every variant against the judge before it is timed
    games = np.r_[0:min(CHECKED, n), max(n - CHECKED, 0):n]
    pick = torch.from_numpy(games).to(dev)
    want64 = {a: J.judge64(rew_h[a][:, games], d_h[:, games], val_h[a][:, games], lpb_h[a][:, games], lpt_h[a][:, games], GAMMA, LAM, CLIPS) for a in AGENTS}
    want_gae = {a: GJ.judge(rew_h[a][:, games], d_h[:, games], val_h[a][:, games], GAMMA, LAM) for a in AGENTS}
    used = {}
    side = torch.cuda.Stream()
    graphs = {}
    for name, body in bodies.items():
        body()
        torch.cuda.synchronize()
        if name != "copy":
            for a in AGENTS:
                for i, key in enumerate(("advantages", "returns")):
                    got = outs[name][key][a][:, pick].cpu().numpy()
                    if name == "pz_gae":
                        assert np.array_equal(got.view(np.uint32), want_gae[a][i].view(np.uint32)), (name, a, key, "bits")
                    else:
                        share = J.worst_share(got, want64[a][i], want64[a][2 + i])
                        used[name] = max(used.get(name, 0.0), share)
                        assert share <= (1 if name == "pz_vtrace" else 2), (name, a, key, share)
        if name != "torch eager":
            body()  # warm up
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graphs[name], stream=side):
                    body()
    torch.cuda.synchronize()

    def run(name):
        if name == "torch eager":
            bodies[name]()
        else:
            graphs[name].replay()

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    names, reps = list(bodies), {}
    for name in names:
        with torch.cuda.stream(side):
            run(name)
            e0.record()
            run(name)
            e1.record()
        torch.cuda.synchronize()
        reps[name] = max(2, min(2000, int(args.min_time * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1))
    times = {name: [] for name in names}
    for rnd in range(args.rounds):
        for name in names[rnd % len(names):] + names[:rnd % len(names)]:
            with torch.cuda.stream(side):
                run(name)  # untimed lead-in behind the previous variant
                e0.record()
                for _ in range(reps[name]):
                    run(name)
                e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps[name])
    med = {name: statistics.median(times[name]) for name in names}
    print(f"\n== {n} games x {k} rows, both agents, {reward_dtype} rewards, {value_dtype} values: {total} algorithmic bytes "
          f"({total / (k * n):.2f} per game-step; pz_gae {total_gae / (k * n):.2f}); pz_vtrace used {used['pz_vtrace']:.3f} of the derived tolerance, "
          f"the torch loop {used['torch eager']:.3f}, pz_gae matched its judge bit for bit; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        ts = times[name]
        rate = (total_gae if name == "pz_gae" else total) / (med[name] * 1e-6)
        print(f"  {name:12s} median {med[name]:10.2f} us per call  spread {max(ts) - min(ts):8.2f}  ({reps[name]:4d} calls per sample)  "
              f"{rate / 1e9:8.1f} GB/s  {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s", flush=True)
    beats = med["pz_vtrace"] < med["torch graph"]
    print(f"  pz_vtrace vs torch eager {med['torch eager'] / med['pz_vtrace']:.1f}x, vs torch graph {med['torch graph'] / med['pz_vtrace']:.1f}x, "
          f"{med['pz_vtrace'] / med['copy']:.2f}x the copy's time, {med['pz_vtrace'] / med['pz_gae']:.2f}x pz_gae's -> "
          f"{'faster than the captured torch loop' if beats else '*slower*'}", flush=True)
    del graphs
    torch.cuda.empty_cache()
    return beats


def registers():
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(vtrace.LIB_PATH):
            print(f"  {name.split('(')[0].replace('void ', ''):32s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch "
                  f"{r['.private_segment_fixed_size']}  spilled VGPRs {r['.vgpr_spill_count']}  LDS {r['.group_segment_fixed_size']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=["65536x32", "65536x128", "524288x32", "4096x128"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = vtrace.load()
    learn.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_vtrace_build_id().decode()}", flush=True)
    registers()
    cells = [tuple(int(x) for x in c.split("x")) for c in args.cells]
    slower = []
    for i, (n, k) in enumerate(cells):
        rows = [("float32", "float32")] + ([("int32", "float32"), ("float32", "bfloat16")] if i == 0 else [])
        for rf, vf in rows:
            if not time_cell(n, k, rf, vf, args):
                slower.append((n, k, rf, vf))
    print(f"\ncells where pz_vtrace is not faster than the captured torch loop: {slower or 'none'}", flush=True)


if __name__ == "__main__":
    main()
