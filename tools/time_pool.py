#!/usr/bin/env python3
"""What the opponent-pool forward costs (diagnostic): pz_mlp_forward_pool against the route it replaces, against the plain
net launch on one parameter set, and the plan on its own.

    python tools/time_pool.py [--rounds 7] [--min-time 0.05] [--cells 4096 65536 524288] [--members 1 4 16]

Per cell (rows x pool members P; two agents, 35 -> 64 -> 64 -> 19, tanh, float32-normalised observations; player_1 on member
0 without a plan, player_2 on uniformly random members), interleaved in one process over --rounds rounds, the order
rotating, 16 calls per hipGraph replay, reported per call:
    pool            pool.forward(out=previous result): ONE launch;
    per member (a)  what it replaces: net.forward of player_1, then per member a precomputed index list, index_select into a
                    preallocated buffer, net.forward, index_copy_ into the head -- 1 + 3 P launches, captured in one graph;
    one net (b)     what the capability costs: net.forward of both agents on ONE parameter set at the same rows (the kernels
                    of libpikazoo_net.so; their instruction streams are the parent commit's, profiles/pool_ab.log);
    pool, no plan   pool.forward of both agents WITHOUT a plan on member 0: the pool kernel doing exactly (b)'s work, which
                    separates what the kernel around the tile costs from what the plan's indirection costs;
    plan            pool.plan(out=previous plan) on its own: once per re-assignment of opponents, not per policy step.
Before it is timed, `pool` is compared bit for bit with route (a)'s result and with the judge of the tests (tests/pool_judge.py)
on the first and the last 2 048 rows of each agent.  Reported: median and spread (max - min) in us per call.  A cell where
`pool` is not faster than (a) by more than the sum of both spreads is marked *slower*; so is a P = 1 cell where `pool` is slower
than (b) by more than (b)'s own spread.
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
import net_judge as N  # noqa: E402,F401  (tests/: the definition in numpy float64)
import pool_judge as PJ  # noqa: E402
from pikazoo_amd import net, pikazoo_v0, pool  # noqa: E402
from pikazoo_amd.wrappers import NormalizeObservation  # noqa: E402
from time_policy_head import AGENTS, CHECKED, INNER, measure  # noqa: E402
from time_policy_net import capture  # noqa: E402

K, H, O, A = 35, 64, 19, 18


def time_cell(n, P, args):
    dev = torch.device("cuda:0")
    env = NormalizeObservation(pikazoo_v0.env(num_envs=n, device=dev, seed=3, validate_actions=False))
    obs, _ = env.reset()
    for t in range(24):  # (observations of games under way, not of the serve)
        obs, *_ = env.step(env.unwrapped.random_actions(5, t))
    learner, opponent = AGENTS
    torch.manual_seed(1)
    models = [net.ActorCritic(K, H, A).to(dev) for _ in range(P)]
    with torch.no_grad():
        for model in models:
            for p in model.parameters():
                p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
    member_params = [m.parameter_tensors() for m in models]
    members = torch.randint(P, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    plan = pool.plan(members, P).check()
    sides = {learner: None, opponent: plan}
    side = torch.cuda.Stream()
    # ---- route (a)'s fixtures: an index list, a gathered input and an output per member
    index = [torch.nonzero(members == p).flatten() for p in range(P)]
    gathered = [torch.empty((len(i), K), dtype=torch.float32, device=dev) for i in index]
    partial = [torch.empty((len(i), O), dtype=torch.float32, device=dev) for i in index]
    theirs = {a: torch.empty((n, O), dtype=torch.float32, device=dev) for a in AGENTS}

    def per_member():
        net.forward(obs[learner], member_params[0], out=theirs[learner])
        for p in range(P):
            if len(index[p]):
                torch.index_select(obs[opponent], 0, index[p], out=gathered[p])
                net.forward(gathered[p], member_params[p], out=partial[p])
                theirs[opponent].index_copy_(0, index[p], partial[p])

    # ---- judged before it is timed
    head = pool.forward(obs, member_params, sides)
    per_member()
    torch.cuda.synchronize()
    assert all(torch.equal(head[a], theirs[a]) for a in AGENTS), "pool.forward and the per-member route disagree"
    rows = np.r_[0:min(CHECKED, n), max(n - CHECKED, 0):n]
    host = [[p.detach().cpu().numpy() for p in ps] for ps in member_params]
    worst = 0.0
    for a, eff in ((learner, None), (opponent, members.cpu().numpy()[rows])):
        ref, tol = PJ.judge(obs[a][rows].cpu().numpy(), host, eff, "tanh")
        share, _ = N.worst_share(head[a][rows].cpu().numpy(), ref, tol)
        assert share <= 1, (n, P, a, share)
        worst = max(worst, share)
    groups = int(plan.first[P]) // pool.GROUP_ROWS
    plain = {a: torch.empty((n, O), dtype=torch.float32, device=dev) for a in AGENTS}
    bare = {a: torch.empty((n, O), dtype=torch.float32, device=dev) for a in AGENTS}
    unplanned = {a: None for a in AGENTS}
    bodies = {
        "pool": lambda: pool.forward(obs, member_params, sides, out=head),
        "per member (a)": per_member,
        "one net (b)": lambda: net.forward(obs, member_params[0], out=plain),
        "pool, no plan": lambda: pool.forward(obs, member_params[:1], unplanned, out=bare),
        "plan": lambda: pool.plan(members, P, out=plan),
    }
    names = list(bodies)
    graphs = {name: capture(bodies[name], INNER, side) for name in names}
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side, graphed=tuple(graphs))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    print(f"\n== pool forward: {n} rows x {P} members, two agents ({learner} on member 0, {opponent} planned: {groups} groups of "
          f"{pool.GROUP_ROWS} slots for {n} rows), {K}-{H}-{H}-{O} tanh, float32 normalised observations; pool within {worst:.4f} of the judge's "
          f"tolerance and bit-equal to the per-member route; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        print(f"  {name:15s} median {med[name]:10.2f} us per call  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)", flush=True)
    faster = med["pool"] < med["per member (a)"] - (spread["pool"] + spread["per member (a)"])
    over_b = med["pool"] - med["one net (b)"]
    verdict = "faster than (a) by more than both spreads" if faster else "*slower* than (a), or within the spreads"
    if P == 1 and over_b > spread["one net (b)"]:
        verdict += "; *slower* than (b) at P = 1 by more than (b)'s spread"
    print(f"  pool vs (a) {med['per member (a)'] / med['pool']:.2f}x; pool - (b) = {over_b:+.2f} us ({med['pool'] / med['one net (b)']:.2f}x): {verdict}",
          flush=True)
    del graphs
    torch.cuda.empty_cache()
    return faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--members", nargs="+", type=int, default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = pool.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_pool_build_id().decode()}", flush=True)
    try:
        import kernel_notes

        for path in (pool.LIB_PATH, net.LIB_PATH):
            for name, r in kernel_notes.notes(path):
                short = name.split("(")[0].replace("void ", "")
                print(f"  {short:44s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                      f"spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  static LDS {r['.group_segment_fixed_size']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    slower = []
    for n in args.cells:
        for P in args.members:
            if not time_cell(n, P, args):
                slower.append((n, P))
    print(f"\ncells where pool is not faster than the per-member route by more than both spreads: {slower or 'none'}", flush=True)


if __name__ == "__main__":
    main()
