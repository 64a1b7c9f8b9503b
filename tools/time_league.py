#!/usr/bin/env python3
"""What league matchmaking costs (diagnostic): pz_league_draw and pz_league_tally against the sync-free torch routes they
replace, and the league example's policy step with and without the tally.

    python tools/time_league.py [--rounds 7] [--min-time 0.05] [--cells 4096 65536 524288] [--members 1 4 16]

Per cell (games x pool members P x share of games that ended on the step: none, 1 in 64), interleaved in one process over
--rounds rounds, the order rotating, 16 calls per hipGraph replay, reported per call:
    draw               league.draw(weights, n, seed, counter on the device, out=members): ONE launch;
    multinomial        what it replaces: members.copy_(torch.multinomial(weights.double(), n, replacement=True));
    draw, masked       league.draw(..., mask=terminations, out=members): only the games that ended are re-drawn;
    multinomial, masked   the same through torch.where(terminations, multinomial, members);
    tally              league.tally(terminations, scores, members, P, table=, errors=): ONE launch;
    index_add_         what it replaces without a synchronisation: masks, a stack of the four int64 words per game, one
                       index_add_ into the [P * P, 4] view of the table, and the count of invalid members.
A torch route that cannot be captured is timed eagerly, one call per run, and says so.  Before anything is timed, `draw` is
compared word for word with the judge of the tests (tests/league_judge.py) on the first and the last 2 048 games, masked and
not, and `tally` cell for cell on the whole batch, as is the index_add_ route.  Reported: median and spread (max - min) in us
per call.  A cell where the new launch is not faster than the torch route is marked *slower*.

Then, per batch size, the league example's policy step -- Snapshots.act, policy.sample, env.step -- captured with and without
Matchmaker.record behind it (4 members, opponents from one rematch()).
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
import league_judge as LJ  # noqa: E402  (tests/: the header in integers)
from pikazoo_amd import league, net, pikazoo_v0, policy, pool  # noqa: E402
from pikazoo_amd.wrappers import NormalizeObservation  # noqa: E402
from time_policy_head import CHECKED, INNER, measure  # noqa: E402
from time_policy_net import capture  # noqa: E402

SEED = 7


def capture_or_eager(body, side):
    """(callable, calls per run, note): the body as a graph of INNER calls, or -- where torch refuses the capture -- itself"""
    try:
        graph = capture(body, INNER, side)
        return graph.replay, True, ""
    except Exception as exc:  # noqa: BLE001
        torch.cuda.synchronize()
        return body, False, f" (eager: capture refused, {type(exc).__name__})"


def time_cell(n, P, one_in, args):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng([n, P, one_in])
    w = rng.integers(1, 1 << 20, P).astype(np.int64)
    weights = torch.from_numpy(w).to(dev)
    t = np.zeros(n, bool) if not one_in else rng.random(n) < 1.0 / one_in
    term = torch.from_numpy(t).to(dev)
    s = rng.integers(0, 16, (2, n)).astype(np.int32)
    scores = torch.from_numpy(s).to(dev).t()                      # the int32 state's layout: two rows at stride 1
    m = rng.integers(0, P, n).astype(np.int64)
    members = torch.from_numpy(m).to(dev)
    counter = torch.tensor([3], dtype=torch.int64, device=dev)
    draw_errors = torch.zeros(1, dtype=torch.int32, device=dev)
    table = torch.zeros((P, P, 4), dtype=torch.int64, device=dev)
    errors = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()

    # ---- judged before it is timed
    rows = np.r_[0:min(CHECKED, n), max(n - CHECKED, 0):n]
    for mask, host_mask in ((None, None), (term, t)):
        got = league.draw(weights, n, SEED, counter=counter, mask=mask, out=members.clone(), errors=draw_errors).cpu().numpy()
        for lo, hi in ((0, min(CHECKED, n)), (max(n - CHECKED, 0), n)):
            want, _ = LJ.draw(w, hi - lo, SEED, 3, lo, None if host_mask is None else host_mask[lo:hi], prior=m[lo:hi])
            assert np.array_equal(got[lo:hi], want), (n, P, one_in, "draw")
    league.tally(term, scores, members, P, table=table, errors=errors)
    want_table, want_errors = LJ.tally(t, s[0], s[1], 1, None, m, P)
    assert np.array_equal(table.cpu().numpy(), want_table) and int(errors.item()) == want_errors == 0 and int(draw_errors.item()) == 0

    flat = torch.zeros((P * P, 4), dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)

    def index_add():
        valid = (members >= 0) & (members < P)
        live = term & valid
        s1, s2 = scores[:, 0].to(torch.int64), scores[:, 1].to(torch.int64)
        words = torch.stack([live.to(torch.int64), (live & (s1 > s2)).to(torch.int64), s1 * live, s2 * live], 1)
        flat.index_add_(0, members.clamp(0, P - 1), words)        # player_1 is member 0: cell (0, b) is row b
        bad.add_((term & ~valid).sum())

    index_add()
    torch.cuda.synchronize()
    assert np.array_equal(flat.view(P, P, 4).cpu().numpy(), want_table), "the index_add_ route and the judge disagree"

    def multinomial():
        members.copy_(torch.multinomial(weights.double(), n, replacement=True))

    def multinomial_masked():
        members.copy_(torch.where(term, torch.multinomial(weights.double(), n, replacement=True), members))

    bodies = {
        "draw": lambda: league.draw(weights, n, SEED, counter=counter, out=members, errors=draw_errors),
        "multinomial": multinomial,
        "draw, masked": lambda: league.draw(weights, n, SEED, counter=counter, mask=term, out=members, errors=draw_errors),
        "multinomial, masked": multinomial_masked,
        "tally": lambda: league.tally(term, scores, members, P, table=table, errors=errors),
        "index_add_": index_add,
    }
    names = list(bodies)
    runs, graphed, notes = {}, [], {}
    for name in names:
        runs[name], is_graph, notes[name] = capture_or_eager(bodies[name], side)
        if is_graph:
            graphed.append(name)
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: runs[name](), args, side, graphed=tuple(graphed))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    print(f"\n== league: {n} games x {P} members, {'no game ended' if not one_in else f'1 game in {one_in} ended ({int(t.sum())})'}; draw and tally equal "
          f"to the judge; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        print(f"  {name:20s} median {med[name]:10.2f} us per call  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample){notes[name]}", flush=True)
    slower = []
    for ours, theirs in (("draw", "multinomial"), ("draw, masked", "multinomial, masked"), ("tally", "index_add_")):
        lost = not med[ours] < med[theirs]
        print(f"  {ours} vs {theirs}: {med[theirs] / med[ours]:.2f}x{' *slower*' if lost else ''}", flush=True)
        if lost:
            slower.append((n, P, one_in, ours))
    del runs
    torch.cuda.empty_cache()
    return slower


def time_policy_step(n, args):
    """the league example's policy step, captured, with and without Matchmaker.record"""
    dev = torch.device("cuda:0")
    env = NormalizeObservation(pikazoo_v0.env(num_envs=n, device=dev, seed=3, validate_actions=False))
    learner, opponent = env.agents
    A = env.action_space(learner).n
    obs, _ = env.reset()
    torch.manual_seed(1)
    model = net.ActorCritic(in_features=obs[learner].shape[1], hidden=64, num_actions=A).to(dev)
    snapshots = pool.Snapshots(model, 4)
    mm = league.Matchmaker(snapshots, n, seed=SEED)
    for _ in range(3):
        mm.push()
    sides = {learner: None, opponent: mm.rematch()}
    state = {"head": None, "picked": None}

    def step(record):
        state["head"] = snapshots.act(obs, sides, out=state["head"])
        state["picked"] = policy.sample({a: state["head"][a][:, :A] for a in env.agents}, seed=SEED, step=0, out=state["picked"])
        _, _, terminations, _, _ = env.step(state["picked"]["actions"])
        if record:
            mm.record(terminations[learner], env.unwrapped.scores)

    side = torch.cuda.Stream()
    names = ["policy step", "policy step + record"]
    graphs = {"policy step": capture(lambda: step(False), INNER, side), "policy step + record": capture(lambda: step(True), INNER, side)}
    torch.cuda.synchronize()
    times, reps = measure(names, lambda name: graphs[name].replay(), args, side, graphed=tuple(names))
    mm.check()
    med = {name: statistics.median(times[name]) for name in names}
    print(f"\n== the league example's policy step at {n} games, 4 members (act, sample, env.step), captured; {int(mm.table[0, :, 0].sum())} games recorded "
          f"while it was timed", flush=True)
    for name in names:
        print(f"  {name:20s} median {med[name]:10.2f} us per call  spread {max(times[name]) - min(times[name]):8.2f}  ({reps[name]:4d} runs per sample)",
              flush=True)
    print(f"  record adds {med[names[1]] - med[names[0]]:+.2f} us ({med[names[1]] / med[names[0]]:.3f}x)", flush=True)
    del graphs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--members", nargs="+", type=int, default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = league.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_league_build_id().decode()}", flush=True)
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(league.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:28s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                  f"spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  static LDS {r['.group_segment_fixed_size']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    slower = []
    for n in args.cells:
        for P in args.members:
            for one_in in (0, 64):
                slower += time_cell(n, P, one_in, args)
    print(f"\ncells where the new launch is not faster than the torch route it replaces: {slower or 'none'}", flush=True)
    for n in args.cells:
        time_policy_step(n, args)


if __name__ == "__main__":
    main()
