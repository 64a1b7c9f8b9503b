#!/usr/bin/env python3
"""League PPO on the project's own pieces: the learner plays a pool of its own frozen snapshots, a different one per game.

    python pika-zoo_amd/build.py        # once: hipcc --offload-arch=gfx950
    python examples/ppo_league.py --num-envs 4096 --iters 20 --steps 32 --pool 8 --snapshot-every 2

``player_1`` of every game is the learner (pool member 0, the live ``net.ActorCritic``).  ``player_2`` of every game is a
member drawn for that game with ``torch.randint`` over the current pool -- the learner itself or one of its snapshots -- and
the draw is renewed once per iteration: ``pool.plan`` groups the games by member (one launch), and every policy step is then
``pool.Snapshots.act`` (ONE launch for both sides, each row through its own member's net) -> ``policy.sample`` -> ``env.step``.
Every ``--snapshot-every`` iterations ``push()`` freezes the learner's parameters into the next slot of the ring.  The update
uses ``player_1``'s samples only, through ``ActorCritic.evaluate`` -> ``ppo.loss`` -> ``backward`` -> ``optim.Adam.step``; the
snapshots have no gradients.

``--pfsp`` turns the pool into a league (``pikazoo_amd.league``): a ``Matchmaker`` records every finished game against the
member it was played against (``record`` after every ``env.step``, one launch), draws the opponents by prioritised fictitious
self-play -- members the learner loses to more often -- once per iteration (``rematch()``: the weights, one draw launch, the
plan), pushes the snapshots through it so that an overwritten slot does not inherit results, and the log shows the learner's
win rate against each member.  Without the flag the opponents are drawn uniformly with ``torch.randint`` and nobody keeps
score: the loop launches what it launched before the flag existed.

``--fused-act`` makes the policy step TWO launches instead of three: ``pool.Snapshots.act_sample`` (``pikazoo_amd.pool_act``:
the net over the pool and the draw in one launch, the learner's log-probabilities and values only, the opponents' side its
actions alone) -> ``env.step``.  It returns the bits of the two launches it replaces, so the losses are the same floats.

``--egocentric`` makes the interface side-symmetric: ``EgocentricObservation(NormalizeObservation(SimplifyAction(env)))``.  The
snapshots are copies of a net that only ever played ``player_1``; as ``player_2`` they otherwise sit on rows they were never
trained on, with left and right reversed.  With the flag ``player_2``'s rows are what ``player_1`` would see in the mirrored
game (``pikazoo_amd.ego``, one launch behind the step) and the 13 relative actions mean the same on both sides.  Whether that
trains better is what the flag is there to find out; without it nothing changes.
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "pika-zoo_amd"))

from pikazoo_amd import league as matchmaking  # noqa: E402
from pikazoo_amd import learn, net, optim, pikazoo_v0, policy, pool, ppo  # noqa: E402
from pikazoo_amd.wrappers import EgocentricObservation, NormalizeObservation, SimplifyAction  # noqa: E402


def main(num_envs=1024, iters=4, steps=16, epochs=2, minibatches=4, lr=3e-4, seed=0, device="cuda:0", log=print, pool_size=8,
         snapshot_every=2, pfsp=False, fused_act=False, egocentric=False):
    """Returns the loss of every minibatch update, as floats."""
    torch.manual_seed(seed)
    env = pikazoo_v0.env(num_envs=num_envs, device=device, seed=seed, validate_actions=False)
    # egocentric: relative actions and player_2's rows mirrored -- both sides are ONE task for a net
    env = EgocentricObservation(NormalizeObservation(SimplifyAction(env))) if egocentric else NormalizeObservation(env)
    learner, opponent = env.agents
    A = env.action_space(learner).n
    obs, _ = env.reset()
    K = obs[learner].shape[1]
    model = net.ActorCritic(in_features=K, hidden=64, num_actions=A).to(device)
    optimizer = optim.Adam(model.parameters(), lr=lr, eps=1e-5, max_grad_norm=0.5)
    league = pool.Snapshots(model, pool_size)
    matchmaker = matchmaking.Matchmaker(league, num_envs, seed=seed) if pfsp else None

    n, k = num_envs, steps
    buf_obs = torch.empty((k, n, K), dtype=obs[learner].dtype, device=device)
    buf_act = torch.empty((k, n), dtype=torch.int64, device=device)
    buf_logp = torch.empty((k, n), dtype=torch.float32, device=device)
    buf_val = torch.empty((k + 1, n), dtype=torch.float32, device=device)
    buf_rew = torch.empty((k, n), dtype=torch.float32, device=device)
    buf_term = torch.empty((k, n), dtype=torch.bool, device=device)
    head = picked = targets = None
    plans = {}                                                    # {pool size: Plan}: a plan is re-used while the pool keeps its size
    losses, policy_step = [], 0

    for it in range(iters):
        if it % snapshot_every == 0 and pool_size > 1:
            matchmaker.push() if pfsp else league.push()
        # ---- every game draws its opponent; the games are grouped by member once per iteration -------------------------------
        if pfsp:
            plan = matchmaker.rematch()                           # PFSP weights from the results so far, one draw, the plan
        else:
            members = torch.randint(len(league), (n,), device=device)
            plan = plans[len(league)] = pool.plan(members, len(league), out=plans.get(len(league)))
        sides = {learner: None, opponent: plan}                   # the learner's side needs no plan: member 0 everywhere

        # ---- rollout: k policy steps, three launches each (net over the pool, head, step), two with fused_act -------------
        for t in range(k):
            if fused_act:                                         # the learner's statistics only: the update reads no others
                picked = league.act_sample(obs, sides, seed=seed, step=policy_step, stats={learner}, out=picked)
                values = picked["values"][learner]
            else:
                head = league.act(obs, sides, out=head)           # {agent: [n, A + 1]}: each row under its own member
                picked = policy.sample({a: head[a][:, :A] for a in env.agents}, seed=seed, step=policy_step, out=picked)
                values = head[learner][:, A]
            buf_obs[t].copy_(obs[learner])
            buf_act[t].copy_(picked["actions"][learner])
            buf_logp[t].copy_(picked["log_probs"][learner])
            buf_val[t].copy_(values)
            obs, rewards, terminations, _, _ = env.step(picked["actions"])
            if pfsp:
                matchmaker.record(terminations[learner], env.scores)   # the terminal frame's scores: the reset comes with the next step
            buf_rew[t].copy_(rewards[learner])
            buf_term[t].copy_(terminations[learner])
            policy_step += 1
        head = league.act(obs, sides, out=head)                   # the bootstrap value
        buf_val[k].copy_(head[learner][:, A])
        targets = learn.gae({learner: buf_rew}, {learner: buf_val}, buf_term, gamma=0.99, lam=0.95, out=targets)

        # ---- update: the learner's samples only --------------------------------------------------------------------------------
        flat = lambda t: t[:k].reshape(k * n, *t.shape[2:])  # noqa: E731
        f_obs, f_act, f_logp = flat(buf_obs), flat(buf_act), flat(buf_logp)
        f_adv, f_ret = flat(targets["advantages"][learner]), flat(targets["returns"][learner])
        size = k * n // minibatches
        for epoch in range(epochs):
            order = torch.randperm(k * n, device=device)
            for m in range(minibatches):
                idx = order[m * size:(m + 1) * size]
                out = model.evaluate({learner: f_obs[idx]})
                loss, stats = ppo.loss(head=out, num_actions=A, actions={learner: f_act[idx]}, old_log_probs={learner: f_logp[idx]},
                                       advantages={learner: f_adv[idx]}, returns={learner: f_ret[idx]}, clip=0.2, vf_coef=0.5, ent_coef=0.01)
                optimizer.zero_grad(set_to_none=True)
                loss[learner].backward()
                optimizer.step()
                losses.append(loss[learner].detach())
        line = (f"iter {it}: pool {len(league)} | loss {float(losses[-1]):+.4f} | entropy {float(stats['entropy'][learner]):.3f} | "
                f"approx_kl {float(stats['approx_kl'][learner]):.5f} | mean reward {float(buf_rew.mean()):+.5f}")
        if pfsp:
            matchmaker.check()
            rates, games = matchmaker.win_rates().tolist(), matchmaker.table[0, :, 0].tolist()
            line += " | win rate " + " ".join(f"{m}:{rates[m]:.2f}/{games[m]}" if games[m] else f"{m}:-" for m in range(len(league)))
        log(line)
    return [float(x) for x in losses]


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--num-envs", type=int, default=1024)
    p.add_argument("--iters", type=int, default=4)
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--pool", type=int, default=8, help="pool members: the learner and pool - 1 snapshots (at most 16)")
    p.add_argument("--snapshot-every", type=int, default=2, help="iterations between two snapshots of the learner")
    p.add_argument("--pfsp", action="store_true", help="a league: record results per member and draw opponents by prioritised fictitious self-play")
    p.add_argument("--fused-act", action="store_true", help="the net over the pool and the action draw in one launch (pikazoo_amd.pool_act)")
    p.add_argument("--egocentric", action="store_true", help="relative actions and player_2's rows mirrored: one net, either side")
    args = p.parse_args()
    main(num_envs=args.num_envs, iters=args.iters, steps=args.steps, pool_size=args.pool, snapshot_every=args.snapshot_every, pfsp=args.pfsp,
         fused_act=args.fused_act, egocentric=args.egocentric)
