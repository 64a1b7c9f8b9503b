#!/usr/bin/env python3
"""What the egocentric mirror costs (diagnostic): pz_ego_rows against the torch route it replaces and against a device copy of
the same bytes, and the league example's policy step with and without the wrapper.

    python tools/time_ego.py [--rounds 7] [--min-time 0.05] [--cells 4096 65536 524288]

Per cell (rows x row format: float32-normalised, bfloat16-normalised, int32), interleaved in one process over --rounds rounds,
the order rotating, 16 calls per hipGraph replay, reported per call:
    mirror             ego.mirror(rows, out=slot): ONE launch into a separate buffer (a slot of a rollout buffer);
    mirror, in place   ego.mirror(rows, out=rows);
    torch              what it replaces: slot.copy_(rows); slot[:, cols] = c - slot[:, cols]  (captured);
    copy               slot.copy_(rows): the bytes moved and nothing else -- the floor, and what the examples issue for that
                       tensor anyway.
Before anything is timed the mirror is compared bit for bit with the judge of the tests (tests/ego_judge.py) on the first and
the last 2 048 rows.  Reported: median and spread (max - min) in us per call, the ratio to the copy and to the torch route.  A
cell where the launch is not faster than the torch route is marked *slower*.

Then, per batch size, the league example's policy step -- Snapshots.act, policy.sample, env.step -- captured on
NormalizeObservation(SimplifyAction(env)) with and without EgocentricObservation around it.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
import ego_judge as EJ  # noqa: E402  (tests/: the header in numpy)
from pikazoo_amd import ego, net, pikazoo_v0, policy, pool  # noqa: E402
from pikazoo_amd.wrappers import EgocentricObservation, NormalizeObservation, SimplifyAction  # noqa: E402
from time_policy_head import CHECKED, INNER, measure  # noqa: E402
from time_policy_net import capture  # noqa: E402

FORMS = (("float32 normalised", 1, torch.float32, None), ("bfloat16 normalised", 6, torch.bfloat16, True), ("int32", 0, torch.int32, None))
COLS = list(EJ.COURT + EJ.SIGN)


def stored(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


def time_cell(n, form, args):
    label, fmt, dtype, normalized = form
    dev = torch.device("cuda:0")
    rng = np.random.default_rng([n, fmt])
    host = EJ.encode(rng.integers(EJ.LOW, EJ.HIGH + 1, (n, EJ.DIM)), fmt)
    rows = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
    rows = rows.view(torch.bfloat16) if dtype == torch.bfloat16 else rows
    buf = torch.zeros((2, n, EJ.DIM), dtype=dtype, device=dev)
    slot = buf[1]
    scratch = rows.clone()
    side = torch.cuda.Stream()

    # ---- judged before it is timed
    ego.mirror(rows, normalized, out=slot)
    torch.cuda.synchronize()
    for lo, hi in ((0, min(CHECKED, n)), (max(n - CHECKED, 0), n)):
        assert np.array_equal(EJ.bits(stored(slot[lo:hi])), EJ.bits(EJ.mirror(host[lo:hi], fmt))), (n, label)
    if fmt == 0:
        c = torch.tensor([EJ.WIDTH if j in EJ.COURT else 0 for j in COLS], dtype=dtype, device=dev)
    else:
        c = torch.tensor([float(EJ.C26) if j == 26 else 1.0 for j in COLS], dtype=torch.float32, device=dev)
    cols = torch.tensor(COLS, device=dev)

    def torch_route():
        slot.copy_(rows)
        slot[:, cols] = (c - slot[:, cols]).to(dtype)

    torch_route()
    torch.cuda.synchronize()
    assert np.array_equal(EJ.bits(stored(slot[:CHECKED])), EJ.bits(EJ.mirror(host[:CHECKED], fmt))), "the torch route and the judge disagree"

    bodies = {
        "mirror": lambda: ego.mirror(rows, normalized, out=slot),
        "mirror, in place": lambda: ego.mirror(scratch, normalized, out=scratch),
        "torch": torch_route,
        "copy": lambda: slot.copy_(rows),
    }
    names = list(bodies)
    graphs = {name: capture(bodies[name], INNER, side) for name in names}
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side, graphed=tuple(names))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    moved = 2 * n * EJ.DIM * rows.element_size()
    print(f"\n== ego: {n} rows, {label} ({moved / 1e6:.2f} MB read + written); the mirror equal to the judge; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        print(f"  {name:18s} median {med[name]:10.2f} us per call  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)  "
              f"{moved / med[name] / 1e3:8.1f} GB/s", flush=True)
    slower = []
    for ours in ("mirror", "mirror, in place"):
        lost = not med[ours] < med["torch"]
        print(f"  {ours}: {med[ours] / med['copy']:.2f}x the copy's time, torch route {med['torch'] / med[ours]:.2f}x{' *slower*' if lost else ''}", flush=True)
        if lost:
            slower.append((n, label, ours, round(med[ours], 2), round(spread[ours], 2)))
    del graphs
    torch.cuda.empty_cache()
    return slower


def time_policy_step(n, args):
    """the league example's policy step, captured, with and without EgocentricObservation"""
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    graphs, names = {}, ["policy step", "policy step, egocentric"]
    alive = []   # every tensor a captured graph reads or writes has to outlive its replays: both envs, nets, plans and results
    for name in names:
        env = NormalizeObservation(SimplifyAction(pikazoo_v0.env(num_envs=n, device=dev, seed=3, validate_actions=False)))
        if name.endswith("egocentric"):
            env = EgocentricObservation(env)
        learner, opponent = env.agents
        A = env.action_space(learner).n
        obs, _ = env.reset()
        torch.manual_seed(1)
        model = net.ActorCritic(in_features=obs[learner].shape[1], hidden=64, num_actions=A).to(dev)
        snapshots = pool.Snapshots(model, 4)
        for _ in range(3):
            snapshots.push()
        plan = pool.plan(torch.randint(4, (n,), device=dev), 4)
        sides = {learner: None, opponent: plan}
        state = {"head": None, "picked": None, "obs": obs}

        def step(env=env, snapshots=snapshots, sides=sides, state=state, A=A):
            state["head"] = snapshots.act(state["obs"], sides, out=state["head"])
            state["picked"] = policy.sample({a: state["head"][a][:, :A] for a in env.agents}, seed=7, step=0, out=state["picked"])
            state["obs"] = env.step(state["picked"]["actions"])[0]

        graphs[name] = capture(step, INNER, side)
        alive.append((env, model, snapshots, plan, sides, state, step))
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side, graphed=tuple(names))
    med = {name: statistics.median(times[name]) for name in names}
    print(f"\n== the league example's policy step at {n} games, 4 members, 13 actions (act, sample, env.step), captured", flush=True)
    for name in names:
        print(f"  {name:26s} median {med[name]:10.2f} us per call  spread {max(times[name]) - min(times[name]):8.2f}  ({reps[name]:4d} runs per sample)",
              flush=True)
    print(f"  the wrapper adds {med[names[1]] - med[names[0]]:+.2f} us ({med[names[1]] / med[names[0]]:.3f}x)", flush=True)
    del graphs, alive
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = ego.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_ego_build_id().decode()}", flush=True)
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(ego.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:36s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                  f"spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  static LDS {r['.group_segment_fixed_size']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    slower = []
    for n in args.cells:
        for form in FORMS:
            slower += time_cell(n, form, args)
    print(f"\ncells where the launch is not faster than the torch route it replaces: {slower or 'none'}", flush=True)
    for n in args.cells:
        time_policy_step(n, args)


if __name__ == "__main__":
    main()
