#!/usr/bin/env python3
"""Self-play PPO on the project's own pieces: one shared actor-critic plays both sides.

    python pika-zoo_amd/build.py        # once: hipcc --offload-arch=gfx950
    python examples/ppo_selfplay.py --num-envs 4096 --iters 20 --steps 32

Per policy step: ``ActorCritic.act`` (the net's forward, both agents, one launch) -> ``policy.sample`` (action, log-prob
and entropy, one launch) -> ``env.step``.  Per iteration: ``learn.gae`` (one launch), then minibatches through
``ActorCritic.evaluate`` (the same forward launch, differentiable, both agents at once) -> ``ppo.loss(head=...)`` (loss and
gradients in one pass) -> ``backward`` (``netgrad.backward``: the six parameter gradients in one call) ->
``optim.Adam.step`` (the gradient clip and Adam in one launch).  ``--torch-update`` (``native_update=False``) keeps the update
on ``ActorCritic.forward`` and torch autograd; ``--torch-optimizer`` (``native_optimizer=False``) keeps
``clip_grad_norm_`` and ``torch.optim.Adam``.  The rollout net reads the parameters in place: nothing to copy after a step
of the optimizer.  ``native_batch=True`` moves the data between these stages with ``batch.RolloutBuffer``: one ``store`` per
policy step instead of eleven ``copy_`` calls, and one ``minibatch`` per minibatch instead of ``randperm`` and ten index
gathers.  It is off by default, because what it costs against the torch route is not measured yet:
``--native-batch`` turns it on.  ``fused_act=True`` (``--fused-act``) makes the rollout's first two launches one:
``ActorCritic.act_sample`` goes from the observations to action, log-prob, entropy and value (``act.sample``), returns the
bits of the two launches and draws from the same stream, so the losses are the same numbers; it stores the head only on the
``native_batch`` route, whose ``store`` takes it.  Off by default; which route is faster at which batch: README.
``egocentric=True`` (``--egocentric``) makes the env ``EgocentricObservation(NormalizeObservation(SimplifyAction(env)))``:
``player_2``'s rows are what ``player_1`` would see in the mirrored game and the 13 relative actions mean the same on both
sides, so the shared weights learn one task instead of two.  Whether that trains better is what the flag is there to find out.
``vtrace=True`` (``--vtrace``) recomputes the targets at the start of every epoch after the first: by then the parameters have
moved and the rollout is off-policy.  One ``model.act`` over all ``(k + 1) * n`` stored observations gives the current values
and logits, ``policy.log_probs`` the current log-probs of the stored actions, and ``vtrace.targets`` (one launch, into the
tensors ``learn.gae`` wrote) the V-trace returns and advantages with the stored log-probs as behaviour.  The first epoch keeps
``learn.gae`` -- there the two are the same bits -- and ``ppo.loss`` keeps the stored log-probs as ``old_log_probs``.  Not with
``native_batch``, whose buffer keeps no bootstrap observations.
``fused_rollout=True`` (``--fused-rollout``) makes the whole rollout loop ONE launch per iteration: ``ActorCritic.rollout``
(``env.rollout_policy``) runs the ``k`` policy steps -- net, draw and frame -- and the bootstrap value inside one kernel and
returns the rollout buffer itself, which ``learn.gae`` reads as it is.  It returns the bits of the loop it replaces and draws
from the same stream, so the losses are the same numbers.  Off by default; not with ``native_batch`` or ``egocentric``.
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "pika-zoo_amd"))

from pikazoo_amd import batch, learn, net, optim, pikazoo_v0, policy, ppo  # noqa: E402
from pikazoo_amd import vtrace as vtrace_targets  # noqa: E402  (the module alone: its library loads on the first call)
from pikazoo_amd.wrappers import EgocentricObservation, NormalizeObservation, SimplifyAction  # noqa: E402


def main(num_envs=1024, iters=4, steps=16, epochs=2, minibatches=4, lr=3e-4, seed=0, device="cuda:0", log=print,
         native_update=True, native_optimizer=True, native_batch=False, fused_act=False, egocentric=False, vtrace=False,
         fused_rollout=False):
    """Returns the loss of every minibatch update, as floats."""
    if fused_rollout and (native_batch or egocentric):
        raise ValueError("fused_rollout=True returns the rollout buffer itself (no batch.RolloutBuffer: native_batch=False) and takes "
                         "wrappers the step kernel fuses (EgocentricObservation mirrors outside it: egocentric=False)")
    if vtrace and native_batch:
        raise ValueError("vtrace=True needs the bootstrap observations, which batch.RolloutBuffer (native_batch=True) does not keep")
    torch.manual_seed(seed)
    env = pikazoo_v0.env(num_envs=num_envs, device=device, seed=seed, validate_actions=False)
    # egocentric: relative actions and player_2's rows mirrored -- both sides are ONE task for a net
    env = EgocentricObservation(NormalizeObservation(SimplifyAction(env))) if egocentric else NormalizeObservation(env)
    agents = env.agents
    A = env.action_space(agents[0]).n
    obs, _ = env.reset()
    K = obs[agents[0]].shape[1]
    model = net.ActorCritic(in_features=K, hidden=64, num_actions=A).to(device)
    if native_optimizer:
        optimizer = optim.Adam(model.parameters(), lr=lr, eps=1e-5, max_grad_norm=0.5)   # the clip is part of its launch
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=lr, eps=1e-5)

    n, k = num_envs, steps
    buf = gathered = rewards = terminations = None   # native_batch: the buffers take their shapes from the first policy step
    if not native_batch and not fused_rollout:
        buf_obs = {a: torch.empty((k + 1 if vtrace else k, n, K), dtype=obs[a].dtype, device=device) for a in agents}   # vtrace: and the bootstrap's
        buf_act = {a: torch.empty((k, n), dtype=torch.int64, device=device) for a in agents}
        buf_logp = {a: torch.empty((k, n), dtype=torch.float32, device=device) for a in agents}
        buf_val = {a: torch.empty((k + 1, n), dtype=torch.float32, device=device) for a in agents}
        buf_rew = {a: torch.empty((k, n), dtype=torch.float32, device=device) for a in agents}
        buf_term = torch.empty((k, n), dtype=torch.bool, device=device)
    head = picked = targets = now = roll = None
    if vtrace:
        now_val = {a: torch.empty((k + 1, n), dtype=torch.float32, device=device) for a in agents}
    losses, policy_step = [], 0

    for it in range(iters):
        # ---- rollout: k policy steps, three launches each (net, head, step), two with fused_act ------------------------------
        if fused_rollout:
            # ONE launch: k x (net, draw, frame) and the bootstrap value; what it returns IS the rollout buffer
            roll = model.rollout(env, k, seed=seed, step=policy_step, out=roll)
            policy_step += k
            buf_obs, buf_act, buf_logp, buf_val = roll["obs"], roll["actions"], roll["log_probs"], roll["values"]
            buf_rew, buf_term = roll["rewards"], roll["terminations"]
            targets = learn.gae(buf_rew, buf_val, buf_term, gamma=0.99, lam=0.95, out=targets)
        else:
            for t in range(k):
                if fused_act:                                         # one launch: the head only where the buffer stores it
                    picked = model.act_sample(obs, seed=seed, step=policy_step, head=native_batch, out=picked)
                    values = picked["values"]
                    if native_batch:
                        head = picked["head"]
                else:
                    head = model.act(obs, out=head)                   # {agent: [n, A + 1]}: logits and value
                    picked = policy.sample({a: head[a][:, :A] for a in agents}, seed=seed, step=policy_step, out=picked)
                    values = {a: head[a][:, A] for a in agents}
                if native_batch:
                    if buf is None:
                        buf = batch.RolloutBuffer(k, n, dict(obs=obs, actions=picked["actions"], log_probs=picked["log_probs"], head=head),
                                                  minibatches=minibatches, seed=seed)
                    # one launch: this step's records to row t, the outcome of the previous step (what came with obs) to row t - 1
                    buf.store(t, obs=obs, actions=picked["actions"], log_probs=picked["log_probs"], head=head,
                              rewards=rewards if t else None, terminations=terminations if t else None)
                else:
                    for a in agents:
                        buf_obs[a][t].copy_(obs[a])
                        buf_act[a][t].copy_(picked["actions"][a])
                        buf_logp[a][t].copy_(picked["log_probs"][a])
                        buf_val[a][t].copy_(values[a])
                obs, rewards, terminations, _, _ = env.step(picked["actions"])
                if not native_batch:
                    for a in agents:
                        buf_rew[a][t].copy_(rewards[a])
                    buf_term[t].copy_(terminations[agents[0]])
                policy_step += 1
            head = model.act(obs, out=head)                           # the bootstrap value
            if native_batch:
                buf.store(k, head=head, rewards=rewards, terminations=terminations)
                targets = learn.gae(buf.rewards, buf.values, buf.terminations, gamma=0.99, lam=0.95, out=targets)
                buf.set_targets(targets)
            else:
                for a in agents:
                    buf_val[a][k].copy_(head[a][:, A])
                    if vtrace:
                        buf_obs[a][k].copy_(obs[a])
                targets = learn.gae(buf_rew, buf_val, buf_term, gamma=0.99, lam=0.95, out=targets)

        # ---- update: both agents' samples through the one net ----------------------------------------------------------------
        flat = lambda d: {a: d[a][:k].reshape(k * n, *d[a].shape[2:]) for a in agents}  # noqa: E731
        if not native_batch:
            f_obs, f_act, f_logp = flat(buf_obs), flat(buf_act), flat(buf_logp)
            f_adv, f_ret = flat(targets["advantages"]), flat(targets["returns"])
        size = k * n // minibatches
        for epoch in range(epochs):
            if vtrace and epoch > 0:
                # off-policy by now: values and log-probs of the CURRENT parameters over the whole buffer (one net launch, one head
                # launch), then V-trace into the tensors learn.gae wrote -- f_adv and f_ret are views of them
                now = model.act({a: buf_obs[a].reshape((k + 1) * n, K) for a in agents}, out=now)
                logp_now, _ = policy.log_probs({a: now[a][:k * n, :A] for a in agents}, f_act)
                for a in agents:
                    now_val[a].view(-1).copy_(now[a][:, A])
                targets = vtrace_targets.targets(buf_rew, now_val, buf_term, buf_logp, {a: logp_now[a].view(k, n) for a in agents},
                                                 gamma=0.99, lam=0.95, out=targets)
            if not native_batch:
                order = torch.randperm(k * n, device=device)
            for m in range(minibatches):
                if native_batch:
                    # one launch: minibatch m of the epoch's shuffle, every tensor of both agents (no randperm, no index tensor)
                    gathered = buf.minibatch(counter=(it * epochs + epoch) * minibatches + m, out=gathered)
                    pick = lambda d: d  # noqa: E731
                    f_obs, f_act, f_logp = gathered["obs"], gathered["actions"], gathered["log_probs"]
                    f_adv, f_ret = gathered["advantages"], gathered["returns"]
                else:
                    idx = order[m * size:(m + 1) * size]
                    pick = lambda d: {a: d[a][idx] for a in agents}  # noqa: E731
                if native_update:
                    out = model.evaluate(pick(f_obs))             # one forward launch; its backward is one call
                else:
                    out = {a: model(pick(f_obs)[a]) for a in agents}   # the torch route: differentiable
                loss, stats = ppo.loss(head=out, num_actions=A, actions=pick(f_act), old_log_probs=pick(f_logp),
                                       advantages=pick(f_adv), returns=pick(f_ret), clip=0.2, vf_coef=0.5, ent_coef=0.01)
                optimizer.zero_grad(set_to_none=True)
                sum(loss.values()).backward()
                if not native_optimizer:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), 0.5)
                optimizer.step()
                losses.append(sum(loss.values()).detach())
        log(f"iter {it}: loss {float(losses[-1]):+.4f} | entropy {float(stats['entropy'][agents[0]]):.3f} | "
            f"approx_kl {float(stats['approx_kl'][agents[0]]):.5f} | mean reward {float((buf.rewards if native_batch else buf_rew)[agents[0]].float().mean()):+.5f}")
    return [float(x) for x in losses]


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--num-envs", type=int, default=1024)
    p.add_argument("--iters", type=int, default=4)
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--torch-update", action="store_true", help="update through ActorCritic.forward and torch autograd")
    p.add_argument("--torch-optimizer", action="store_true", help="clip_grad_norm_ and torch.optim.Adam instead of optim.Adam")
    p.add_argument("--native-batch", action="store_true", help="batch.RolloutBuffer: one store per policy step, one gather per minibatch")
    p.add_argument("--fused-act", action="store_true", help="ActorCritic.act_sample: the net's forward and the sampling in one launch")
    p.add_argument("--egocentric", action="store_true", help="relative actions and player_2's rows mirrored: one net, either side")
    p.add_argument("--vtrace", action="store_true", help="V-trace targets under the current parameters from the second epoch on")
    p.add_argument("--fused-rollout", action="store_true", help="ActorCritic.rollout: the k policy steps of an iteration in one launch")
    args = p.parse_args()
    main(num_envs=args.num_envs, iters=args.iters, steps=args.steps, native_update=not args.torch_update,
         native_optimizer=not args.torch_optimizer, native_batch=args.native_batch, fused_act=args.fused_act,
         egocentric=args.egocentric, vtrace=args.vtrace, fused_rollout=args.fused_rollout)
