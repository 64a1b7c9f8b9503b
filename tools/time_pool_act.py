#!/usr/bin/env python3
"""What the pool-act launch saves (diagnostic): pz_mlp_act_pool against the two launches it replaces, and the league's policy
step around it.

    python tools/time_pool_act.py [--rounds 7] [--min-time 0.05] [--cells 4096 65536 524288] [--members 1 4 16]

Per cell (rows x pool members P; two agents, 35 -> 64 -> 64 -> 19, tanh, 18 actions, float32-normalised observations; player_1
on member 0 without a plan, player_2 planned over the members a ``league.Matchmaker`` drew), interleaved in one process over
--rounds rounds, the order rotating, every variant captured into a hipGraph of 16 calls per replay and reported per call:
    two launches         Snapshots.act(out=) + policy.sample(out=) on its logits: THE BASELINE of this tool, what the launch
                         replaces, never the code under test;
    pool act             Snapshots.act_sample(out=), statistics of both agents: ONE launch, no head stored;
    pool act, learner    the same with stats={player_1}: the league's call (the opponents' side stores its actions only);
    pool act + head      statistics of both agents and head=True;
    learner + head       stats={player_1} and head=True;
    three-launch step    two launches + env.step + Matchmaker.record: the league example's policy step as it was;
    two-launch step      pool act, learner + env.step + Matchmaker.record: the same with --fused-act.
Before anything is timed every pool-act variant is held to the two launches bit for bit (actions, log-probs, entropy, values,
head) on all rows.  Reported: median and spread (max - min) in us per call.  A cell where the pool-act route is not faster than
the route it replaces by more than the sum of both spreads is marked: *slower* when its median is above the baseline's,
*level* otherwise.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
from pikazoo_amd import league as matchmaking  # noqa: E402
from pikazoo_amd import net, pikazoo_v0, policy, pool, pool_act  # noqa: E402
from pikazoo_amd.wrappers import NormalizeObservation  # noqa: E402
from time_policy_head import AGENTS, INNER, measure  # noqa: E402
from time_policy_net import capture  # noqa: E402

K, H, O, A = 35, 64, 19, 18
PAIRS = (("pool act", "two launches"), ("pool act, learner", "two launches"), ("pool act + head", "two launches"),
         ("learner + head", "two launches"), ("two-launch step", "three-launch step"))


def same_bits(x, y):
    return torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def time_cell(n, P, args):
    dev = torch.device("cuda:0")
    env = NormalizeObservation(pikazoo_v0.env(num_envs=n, device=dev, seed=3, validate_actions=False))
    obs, _ = env.reset()
    for t in range(24):  # (observations of games under way, not of the serve)
        obs, *_ = env.step(env.unwrapped.random_actions(5, t))
    learner, opponent = AGENTS
    torch.manual_seed(1)
    model = net.ActorCritic(K, H, A).to(dev)
    league = pool.Snapshots(model, max(P, 1))
    matchmaker = matchmaking.Matchmaker(league, n, seed=2)
    with torch.no_grad():
        for _ in range(P - 1):  # P - 1 snapshots, the learner moving between them
            for p in model.parameters():
                p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
            matchmaker.push()
        for p in model.parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
    assert len(league) == P
    plan = matchmaker.rematch()
    matchmaker.check()
    sides = {learner: None, opponent: plan}
    side = torch.cuda.Stream()
    kw = dict(seed=3, step=5)
    # ---- held to the two launches before it is timed
    head = league.act(obs, sides)
    picked = policy.sample({a: head[a][:, :A] for a in AGENTS}, **kw)
    outs = {
        "pool act": league.act_sample(obs, sides, **kw),
        "pool act, learner": league.act_sample(obs, sides, stats={learner}, **kw),
        "pool act + head": league.act_sample(obs, sides, head=True, **kw),
        "learner + head": league.act_sample(obs, sides, stats={learner}, head=True, **kw),
    }
    torch.cuda.synchronize()
    for name, got in outs.items():
        for a in AGENTS:
            assert same_bits(got["actions"][a], picked["actions"][a]), (name, a, "actions")
            for key in ("log_probs", "entropy"):
                assert a not in got[key] or same_bits(got[key][a], picked[key][a]), (name, a, key)
            assert a not in got["values"] or same_bits(got["values"][a], head[a][:, A].contiguous()), (name, a, "values")
            assert "head" not in got or same_bits(got["head"][a], head[a]), (name, a, "head")
        assert list(got["log_probs"]) == ([learner] if "learner" in name else list(AGENTS)), name

    def two_launches():
        league.act(obs, sides, out=head)
        policy.sample({a: head[a][:, :A] for a in AGENTS}, out=picked, **kw)

    def three_launch_step():
        two_launches()
        _, _, terminations, _, _ = env.step(picked["actions"])
        matchmaker.record(terminations[learner], env.scores)

    def two_launch_step():
        league.act_sample(obs, sides, stats={learner}, out=outs["pool act, learner"], **kw)
        _, _, terminations, _, _ = env.step(outs["pool act, learner"]["actions"])
        matchmaker.record(terminations[learner], env.scores)

    bodies = {
        "two launches": two_launches,
        "pool act": lambda: league.act_sample(obs, sides, out=outs["pool act"], **kw),
        "pool act, learner": lambda: league.act_sample(obs, sides, stats={learner}, out=outs["pool act, learner"], **kw),
        "pool act + head": lambda: league.act_sample(obs, sides, head=True, out=outs["pool act + head"], **kw),
        "learner + head": lambda: league.act_sample(obs, sides, stats={learner}, head=True, out=outs["learner + head"], **kw),
        "three-launch step": three_launch_step,
        "two-launch step": two_launch_step,
    }
    names = list(bodies)
    graphs = {name: capture(bodies[name], INNER, side) for name in names}
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side, graphed=tuple(graphs))
    matchmaker.check()
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    groups = int(plan.first[P]) // pool.GROUP_ROWS
    print(f"\n== pool act: {n} rows x {P} members, two agents ({learner} on member 0, {opponent} planned: {groups} groups of {pool.GROUP_ROWS} "
          f"slots), {K}-{H}-{H}-{O} tanh, {A} actions, float32 normalised observations; equal to the two launches bit for bit on all rows; "
          f"{args.rounds} interleaved rounds", flush=True)
    for name in names:
        print(f"  {name:18s} median {med[name]:10.2f} us per call  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)", flush=True)
    marks = []
    for ours, base in PAIRS:
        both = spread[ours] + spread[base]
        mark = "faster by more than both spreads" if med[ours] < med[base] - both else ("*slower*" if med[ours] > med[base] else "*level*")
        marks.append((ours, mark))
        print(f"  {ours} vs {base}: {med[base] - med[ours]:+.2f} us saved ({med[base] / med[ours]:.2f}x), spreads {both:.2f} -> {mark}", flush=True)
    del graphs
    torch.cuda.empty_cache()
    return [(n, P, ours, mark) for ours, mark in marks if mark.startswith("*")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--members", nargs="+", type=int, default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = pool_act.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_pool_act_build_id().decode()}", flush=True)
    try:
        import kernel_digest
        import kernel_notes

        counts = kernel_digest.kernels(pool_act.LIB_PATH) if kernel_digest.available() else {}
        for name, r in kernel_notes.notes(pool_act.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:44s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                  f"spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  static LDS {r['.group_segment_fixed_size']}  "
                  f"instructions {counts.get(short, ('', '?'))[1]}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    marked = []
    for n in args.cells:
        for P in args.members:
            marked += time_cell(n, P, args)
    print(f"\ncells where the pool-act route is not faster than the route it replaces by more than both spreads: {marked or 'none'}", flush=True)


if __name__ == "__main__":
    main()
