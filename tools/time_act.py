#!/usr/bin/env python3
"""What the act launch saves (diagnostic): pz_mlp_act against the two launches it replaces, and the rollout step around it.

    python tools/time_act.py [--rounds 7] [--min-time 0.05] [--cells 4096 65536 131072 262144 524288]

(131 072 and 262 144 rows are there to place the size at which the fused launch stops paying.)
Per cell (rows; both agents on shared weights, 35 -> 64 -> 64 -> 19 tanh, 18 actions; float32-normalised, bfloat16-normalised
and raw int32 observations), interleaved in one process over --rounds rounds, the order rotating, every variant captured into a
hipGraph of 16 calls per replay (a replay costs the host some 10 us) and reported per call:
    two launches    net.forward(out=) + policy.sample(out=) on its logits: THE BASELINE of this tool, never the code under test;
    act             act.sample(out=): ONE launch, no head stored;
    act + head      the same with head=True (what the native_batch route of examples/ppo_selfplay.py asks for);
    three-launch step   two launches + env.step on the sampled actions: the rollout step as it was;
    act step        act + env.step.
Before anything is timed the act launch is held to the two launches bit for bit (actions, log-probs, entropy, values, head) on
all rows.  Reported: median and spread (max - min) in us per call.  A cell where the act route is not faster than the route it
replaces by more than the sum of both spreads is marked: *slower* when its median is above the baseline's, *level* otherwise.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
from pikazoo_amd import act, net, pikazoo_v0, policy  # noqa: E402
from pikazoo_amd.wrappers import NormalizeObservation  # noqa: E402
from time_policy_head import AGENTS, INNER, measure  # noqa: E402
from time_policy_net import FORMS, A, H, K, O, capture  # noqa: E402

PAIRS = (("act", "two launches"), ("act + head", "two launches"), ("act step", "three-launch step"))


def time_cell(n, form, args):
    label, dtype, normalise = form
    dev = torch.device("cuda:0")
    env = pikazoo_v0.env(num_envs=n, device=dev, seed=3, validate_actions=False,
                         observation_dtype=dtype if dtype != torch.float32 else torch.int32)
    if normalise:
        env = NormalizeObservation(env)
    obs, _ = env.reset()
    for t in range(24):  # (observations of games under way, not of the serve)
        obs, *_ = env.step(env.unwrapped.random_actions(5, t))
    assert all(obs[a].dtype == dtype and tuple(obs[a].shape) == (n, K) for a in AGENTS)
    torch.manual_seed(1)
    model = net.ActorCritic(K, H, A).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
        if not normalise:
            model.fc1.weight.mul_(1.0 / 432)
    side = torch.cuda.Stream()
    # ---- held to the two launches before it is timed
    head = model.act(obs)
    picked = policy.sample({a: head[a][:, :A] for a in AGENTS}, seed=3, step=5)
    fused = model.act_sample(obs, seed=3, step=5)
    fused_head = model.act_sample(obs, seed=3, step=5, head=True)
    torch.cuda.synchronize()
    for a in AGENTS:
        for got in (fused, fused_head):
            for key in ("actions", "log_probs", "entropy"):
                assert torch.equal(got[key][a].view(torch.int32) if key != "actions" else got[key][a],
                                   picked[key][a].view(torch.int32) if key != "actions" else picked[key][a]), (label, a, key)
            assert torch.equal(got["values"][a].view(torch.int32), head[a][:, A].contiguous().view(torch.int32)), (label, a)
        assert torch.equal(fused_head["head"][a].view(torch.int32), head[a].view(torch.int32)), (label, a)

    def two_launches():
        model.act(obs, out=head)
        policy.sample({a: head[a][:, :A] for a in AGENTS}, seed=3, step=5, out=picked)

    def three_launch_step():
        two_launches()
        env.step(picked["actions"])

    def act_step():
        model.act_sample(obs, seed=3, step=5, out=fused)
        env.step(fused["actions"])

    bodies = {
        "two launches": two_launches,
        "act": lambda: model.act_sample(obs, seed=3, step=5, out=fused),
        "act + head": lambda: model.act_sample(obs, seed=3, step=5, head=True, out=fused_head),
        "three-launch step": three_launch_step,
        "act step": act_step,
    }
    names = list(bodies)
    graphs = {name: capture(bodies[name], INNER, side) for name in names}
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side, graphed=tuple(graphs))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    print(f"\n== act: {n} rows, both agents, shared weights, {K}-{H}-{H}-{O} tanh, {A} actions, {label} observations; equal to the two launches "
          f"bit for bit on all rows; {args.rounds} interleaved rounds", flush=True)
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
    return [(n, label, ours, mark) for ours, mark in marks if mark.startswith("*")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 131072, 262144, 524288])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = act.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_act_build_id().decode()}", flush=True)
    try:
        import kernel_digest
        import kernel_notes

        counts = kernel_digest.kernels(act.LIB_PATH) if kernel_digest.available() else {}
        for name, r in kernel_notes.notes(act.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:32s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                  f"spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  static LDS {r['.group_segment_fixed_size']}  "
                  f"instructions {counts.get(short, ('', '?'))[1]}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    marked = []
    for n in args.cells:
        for form in FORMS:
            marked += time_cell(n, form, args)
    print(f"\ncells where the act route is not faster than the route it replaces by more than both spreads: {marked or 'none'}", flush=True)


if __name__ == "__main__":
    main()
