"""pikazoo_amd -- MI355X-native batched Pikachu Volleyball (drop-in for pika-zoo's step path).

    from pikazoo_amd import pikazoo_v0
    env = pikazoo_v0.env(num_envs=65536, device="cuda:0", is_player2_computer=True)

    from pikazoo_amd import learn                      # GAE over the trajectory tensors of a k-step launch, one launch
    out = learn.gae(traj["rewards"], values, traj["terminations"])

    from pikazoo_amd import policy                     # the categorical head: sample + log-prob + entropy, one launch
    out = policy.sample(logits, seed=7, step=env.steps_done)

    from pikazoo_amd import ppo                        # the PPO update loss: loss, statistics and gradients, one pass
    loss, stats = ppo.loss(logits, values, actions, old_log_probs, advantages, returns)

    from pikazoo_amd import net                        # the policy net's forward: observations -> [N, A + 1] head, one launch
    head = net.ActorCritic().to("cuda").act(obs)

    from pikazoo_amd import netgrad                    # the policy net's backward: d loss / d head -> six parameter gradients
    grads = netgrad.backward(obs, params, grad_head)   # (or model.evaluate(obs) and torch's own .backward())

    from pikazoo_amd import optim                      # the optimizer step: gradient clip + Adam / AdamW, one launch
    optimizer = optim.Adam(model.parameters(), lr=3e-4, max_grad_norm=0.5)

    from pikazoo_amd import batch                      # rollout-buffer stores and shuffled minibatch gathers, one launch each
    minibatch = batch.gather(sources, minibatches=4, seed=0, counter=c)

    from pikazoo_amd import pool                       # the net's forward for a pool of snapshots: each row its own member's net
    head = pool.Snapshots(model, capacity=8).act(obs, {"player_1": None, "player_2": pool.plan(members, 8)})

    from pikazoo_amd import league                     # league matchmaking: per-member results and weighted draws, one launch each
    table = league.tally(terminations, env.scores, members, 8); members = league.draw(league.pfsp_weights(table, 8), n, seed=0)

    from pikazoo_amd import act                        # net forward + action sampling: observations -> action, log-prob, entropy, value
    out = model.act_sample(obs, seed=7, step=env.steps_done)      # one launch; the bits of model.act + policy.sample

    from pikazoo_amd import pool_act                   # the same over a pool: each row its own member's net, then the draw
    out = snapshots.act_sample(obs, plans, seed=7, step=env.steps_done, stats={"player_1"})   # one launch; pool.forward + policy.sample

    from pikazoo_amd import ego                        # egocentric rows: player_2 sees the court as player_1 does, one launch
    ego.mirror(obs["player_2"], out=buf_obs[t])        # (wrappers.EgocentricObservation does it behind reset and step)

    from pikazoo_amd import vtrace                     # V-trace targets for off-policy samples (learn.gae's bits on-policy), one launch
    out = vtrace.targets(rewards, values_now, terminations, stored_log_probs, log_probs_now, gamma=0.99, lam=0.95)

    from pikazoo_amd import rollout                    # k policy steps -- net, draw and frame -- in one launch: the rollout buffer
    buf = env.rollout_policy(model, k=32, seed=7, step=env.steps_done)    # the bits of k x (model.act_sample + env.step)
"""
from ._version import VERSION, __version__  # noqa: F401

__all__ = ["VERSION", "__version__", "learn", "policy", "ppo", "net", "netgrad", "optim", "batch", "pool", "league", "act", "pool_act", "ego", "vtrace", "rollout"]


def __getattr__(name):
    # `pikazoo_amd.learn` / `pikazoo_amd.policy` / `pikazoo_amd.ppo` / `pikazoo_amd.net` / `pikazoo_amd.netgrad` / `pikazoo_amd.optim` / `pikazoo_amd.batch` / `pikazoo_amd.pool` / `pikazoo_amd.league` / `pikazoo_amd.act` / `pikazoo_amd.pool_act` / `pikazoo_amd.ego` / `pikazoo_amd.vtrace` / `pikazoo_amd.rollout` on first use:
    # importing the package (and with it the step path) never loads those libraries
    if name in ("learn", "policy", "ppo", "net", "netgrad", "optim", "batch", "pool", "league", "act", "pool_act", "ego", "vtrace", "rollout"):
        import importlib

        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
