#!/usr/bin/env python3
"""What the policy-rollout launch costs per policy step (diagnostic): pz_rollout_policy against the launches it replaces.

    python tools/time_policy_rollout.py [--rounds 7] [--min-time 0.05] [--k 32] [--cells 4096 65536 524288]

Per cell (games; both agents on shared weights, 35 -> 64 -> 64 -> 19 tanh, 18 actions, float32-normalised rows), interleaved in
one process over --rounds rounds, the order rotating, every route captured into ONE hipGraph of k policy steps and reported per
policy step (a replay's time / k):
    act_sample + step       k x (model.act_sample(out=); env.step): two launches per step -- a BASELINE, never the code under test;
    act + sample + step     k x (model.act(out=); policy.sample(out=); env.step): three launches per step -- a BASELINE;
    rollout_random          env.rollout_random(k, out=): the env alone under the random policy, for scale;
    rollout_policy          env.rollout_policy(model, k, out=): ONE launch.
Every route steps an env of its own from the same seed.  Before anything is timed the launch is held to the two-launch route bit
for bit over its k steps (every output and the final state).  Reported: median and spread (max - min) in us per policy step.  The
better baseline is the one with the lower median; a cell in which the launch is slower than it by more than that baseline's
spread is marked *slower*.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
from pikazoo_amd import net, pikazoo_v0, policy, rollout  # noqa: E402
from pikazoo_amd.wrappers import NormalizeObservation  # noqa: E402
from time_policy_head import AGENTS, measure  # noqa: E402
from time_policy_net import A, H, K, O, capture  # noqa: E402

BASELINES = ("act_sample + step", "act + sample + step")


def make_env(n, dev):
    env = NormalizeObservation(pikazoo_v0.env(num_envs=n, device=dev, seed=3, validate_actions=False))
    obs, _ = env.reset()
    for t in range(24):  # (games under way, not the serve)
        obs, *_ = env.step(env.unwrapped.random_actions(5, t))
    return env, obs


def time_cell(n, args):
    dev, k = torch.device("cuda:0"), args.k
    torch.manual_seed(1)
    model = net.ActorCritic(K, H, A).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
    side = torch.cuda.Stream()
    # ---- held to the two-launch route before it is timed
    (ea, _), (eb, obs_b) = make_env(n, dev), make_env(n, dev)
    got = ea.unwrapped.rollout_policy(model, k, 3, step=5)
    for t in range(k):
        picked = model.act_sample(obs_b, seed=3, step=5 + t)
        for a in AGENTS:
            for key in ("actions", "log_probs", "values"):
                assert torch.equal(got[key][a][t], picked[key][a]), (n, t, a, key)
            assert torch.equal(got["obs"][a][t], obs_b[a]), (n, t, a, "obs")
        obs_b, rew, term, _, _ = eb.step(picked["actions"])
        assert all(torch.equal(got["rewards"][a][t], rew[a]) for a in AGENTS) and torch.equal(got["terminations"][t], term[AGENTS[0]]), (n, t)
    assert torch.equal(ea.unwrapped.read_state(), eb.unwrapped.read_state()), n
    del ea, eb, got
    # ---- the routes, each on an env of its own
    envs = {name: make_env(n, dev) for name in (*BASELINES, "rollout_random", "rollout_policy")}
    state = {}

    def two_launch_steps():
        env, obs = envs["act_sample + step"]
        for t in range(k):
            state["picked2"] = model.act_sample(obs, seed=3, step=t, out=state.get("picked2"))
            env.step(state["picked2"]["actions"])

    def three_launch_steps():
        env, obs = envs["act + sample + step"]
        for t in range(k):
            state["head"] = model.act(obs, out=state.get("head"))
            state["picked3"] = policy.sample({a: state["head"][a][:, :A] for a in AGENTS}, seed=3, step=t, out=state.get("picked3"))
            env.step(state["picked3"]["actions"])

    def random_rollout():
        state["traj"] = envs["rollout_random"][0].unwrapped.rollout_random(3, k, t0=0, out=state.get("traj"))

    def policy_rollout():
        state["buf"] = envs["rollout_policy"][0].unwrapped.rollout_policy(model, k, 3, step=0, out=state.get("buf"))

    bodies = {"act_sample + step": two_launch_steps, "act + sample + step": three_launch_steps, "rollout_random": random_rollout,
              "rollout_policy": policy_rollout}
    names = list(bodies)
    graphs = {name: capture(bodies[name], 1, side) for name in names}
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side)
    per_step = {name: [x / k for x in times[name]] for name in names}
    med = {name: statistics.median(per_step[name]) for name in names}
    spread = {name: max(per_step[name]) - min(per_step[name]) for name in names}
    print(f"\n== policy rollout: {n} games, k = {k}, both agents, shared weights, {K}-{H}-{H}-{O} tanh, {A} actions, float32 normalised rows; equal "
          f"to the two-launch route bit for bit over {k} steps; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        print(f"  {name:22s} median {med[name]:9.2f} us per policy step  spread {spread[name]:7.2f}  ({reps[name]:4d} replays per sample)", flush=True)
    base = min(BASELINES, key=lambda name: med[name])
    gap = med["rollout_policy"] - med[base]
    mark = "*slower*" if gap > spread[base] else ("faster" if -gap > spread[base] else "*level*")
    print(f"  rollout_policy vs {base} (the better baseline): {-gap:+.2f} us saved per step ({med[base] / med['rollout_policy']:.2f}x), "
          f"baseline spread {spread[base]:.2f} -> {mark}; the env alone (rollout_random) takes {med['rollout_random']:.2f}", flush=True)
    del graphs, state, envs
    torch.cuda.empty_cache()
    return (n, mark, round(med["rollout_policy"], 2), round(med[base], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = rollout.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_rollout_build_id().decode()}", flush=True)
    try:
        import kernel_digest
        import kernel_notes

        counts = kernel_digest.kernels(rollout.LIB_PATH) if kernel_digest.available() else {}
        for name, r in kernel_notes.notes(rollout.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:44s} VGPRs {r['.vgpr_count']:3d}  AGPRs {r.get('.agpr_count', 0):3d}  SGPRs {r['.sgpr_count']:3d}  scratch "
                  f"{r['.private_segment_fixed_size']}  spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  "
                  f"instructions {counts.get(short, ('', '?'))[1]}", flush=True)
        print(f"  dynamic LDS at {K}-{H}-{H}-{O}, shared weights: {rollout.lds_bytes(H, O, 1)} B", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    cells = [time_cell(n, args) for n in args.cells]
    print(f"\ncells (games, mark, rollout_policy, better baseline; us per policy step): {cells}", flush=True)


if __name__ == "__main__":
    main()
