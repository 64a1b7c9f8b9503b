#!/usr/bin/env python3
"""What the categorical policy head costs (diagnostic): pz_sample_actions and the log_probs pair against the torch
operations they replace and a copy.

    python tools/time_policy_head.py [--rounds 7] [--min-time 0.05] [--cells 65536 524288 4096]

Per cell (games; A = 18, both agents; float32 and bfloat16 logits), interleaved in one process over --rounds rounds, the
order rotating:
  sampling
    pz_sample       ONE launch (pikazoo_amd.policy.sample into its previous result, the step read from a device counter
                    that the graph increments: its one-element add is part of the figure), 16 calls per hipGraph replay
                    (a replay costs the host some 10 us, more than a launch timed here), reported per call;
    torch eager     torch.distributions.Categorical(logits=...): sample() + log_prob() + entropy() per agent, eagerly;
    torch graph     the same captured into a hipGraph where torch allows it (multinomial under capture needs a
                    graph-safe generator: if the capture raises, the row says so and the variant is not timed);
    copy            a device-to-device copy moving the same number of bytes (half read, half written), 16 per replay;
  update side (forward + backward of log-prob and entropy of given actions, a scalar loss, gradient w.r.t. the logits)
    pz_log_probs    pikazoo_amd.policy.log_probs under autograd: two launches and autograd's own bookkeeping, eagerly;
    pz fwd+bwd      the two C-ABI launches alone (pz_action_log_probs, pz_action_log_probs_backward), 16 pairs per hipGraph replay;
    torch fwd+bwd   Categorical(logits=...).log_prob(a) / .entropy() and .backward(), eagerly.
Before it is timed every pz variant is compared with the judge of the tests (tests/policy_judge.py) on the first and the
last 2 048 games, and the torch log-prob with the judge within 1e-5 (bfloat16 logits: computed by torch in bfloat16, not
compared).  Reported: median and spread (max - min) in us per call, the algorithmic bytes (every input and output
element once) over the median in GB/s and as a share of the 6.3 TB/s a streaming kernel achieves on the MI355X.  A cell
where the pz median is not below every torch median of its group is marked *slower*.
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
import policy_judge as J  # noqa: E402  (tests/: the definition in numpy float64)
from pikazoo_amd import policy  # noqa: E402

ACHIEVABLE = 6.3e12  # bytes per second of a streaming kernel on the MI355X
INNER = 16           # calls per captured graph: one replay costs the host ~10 us, more than the launches timed here
CHECKED = 2048
A = 18
AGENTS = ("player_1", "player_2")
SEED, FIRST = 7, 0


def torch_sample(logits, out):
    for a in AGENTS:
        dist = torch.distributions.Categorical(logits=logits[a].float())
        act = dist.sample()
        out["actions"][a].copy_(act)
        out["log_probs"][a].copy_(dist.log_prob(act))
        out["entropy"][a].copy_(dist.entropy())


def torch_update(leaves, actions, w_logp, w_ent):
    loss = 0
    for a in AGENTS:
        dist = torch.distributions.Categorical(logits=leaves[a])
        loss = loss + (dist.log_prob(actions[a]).float() * w_logp[a]).sum() + (dist.entropy().float() * w_ent[a]).sum()
    for a in AGENTS:
        leaves[a].grad = None
    loss.backward()


def pz_update(leaves, actions, w_logp, w_ent):
    logp, ent = policy.log_probs(leaves, actions)
    loss = sum((logp[a] * w_logp[a]).sum() + (ent[a] * w_ent[a]).sum() for a in AGENTS)
    for a in AGENTS:
        leaves[a].grad = None
    loss.backward()


def measure(names, run, args, side, graphed=()):
    """median material: us per CALL of every variant; a variant in `graphed` runs INNER calls per run()"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = {}
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
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps[name] / (INNER if name in graphed else 1))
    return times, reps


def report(title, names, times, reps, total, ours, theirs):
    med = {name: statistics.median(times[name]) for name in names}
    print(title, flush=True)
    for name in names:
        ts = times[name]
        rate = total / (med[name] * 1e-6)
        print(f"  {name:14s} median {med[name]:10.2f} us per call  spread {max(ts) - min(ts):8.2f}  ({reps[name]:4d} runs per sample)  "
              f"{rate / 1e9:8.1f} GB/s  {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s", flush=True)
    beats = all(med[ours] < med[t] for t in theirs if t in med)
    ratios = ", ".join(f"vs {t} {med[t] / med[ours]:.1f}x" for t in theirs if t in med)
    tail = f", {med[ours] / med['copy']:.2f}x the copy's time" if "copy" in med else ""
    print(f"  {ours} {ratios}{tail} -> {'faster than every torch form' if beats else '*slower*'}", flush=True)
    return beats


def time_cell(n, dtype, args):
    dev = torch.device("cuda:0")
    tdtype = {"float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    esize = 4 if dtype == "float32" else 2
    rng = np.random.default_rng([n, esize])
    host = {a: J.as_logit_dtype(rng.normal(0.0, 2.0, size=(n, A)).astype(np.float32), dtype) for a in AGENTS}
    logits = {a: torch.from_numpy(host[a]).to(dev).to(tdtype) for a in AGENTS}
    games = np.r_[0:min(CHECKED, n), max(n - CHECKED, 0):n]
    side = torch.cuda.Stream()

    # ---- sampling -------------------------------------------------------------------------------------------------------
    def outputs():
        return {"actions": {a: torch.empty(n, dtype=torch.int64, device=dev) for a in AGENTS},
                "log_probs": {a: torch.empty(n, dtype=torch.float32, device=dev) for a in AGENTS},
                "entropy": {a: torch.empty(n, dtype=torch.float32, device=dev) for a in AGENTS}}

    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = {name: outputs() for name in ("pz_sample", "torch eager", "torch graph")}
    total = 2 * n * (A * esize + 8 + 4 + 4)
    src, dst = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)

    def pz_body():
        policy.sample(logits, SEED, counter, FIRST, out=outs["pz_sample"])
        counter.add_(1)

    bodies = {"pz_sample": pz_body, "torch eager": lambda: torch_sample(logits, outs["torch eager"]),
              "torch graph": lambda: torch_sample(logits, outs["torch graph"]), "copy": lambda: dst.copy_(src)}
    counter.fill_(5)
    pz_body()
    torch.cuda.synchronize()
    us = J.uniforms(SEED, FIRST, 5, None, n)
    for s, a in enumerate(AGENTS):
        act, amb, nb, st = J.sample(host[a][games], us[s][games])
        got = outs["pz_sample"]["actions"][a].cpu().numpy()[games]
        assert np.array_equal(got[~amb], act[~amb]) and ((got >= nb[:, 0]) & (got <= nb[:, 1])).all(), ("pz_sample", a)
        want, tol = J.log_prob(st, got)
        assert (np.abs(outs["pz_sample"]["log_probs"][a].cpu().numpy()[games] - want) <= tol).all()
        assert (np.abs(outs["pz_sample"]["entropy"][a].cpu().numpy()[games] - st["H"]) <= J.entropy_tolerance(st)).all()
    graphs, notes = {}, []
    for name, body in bodies.items():
        if name == "torch eager":
            body()
            continue
        try:
            body()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    for _ in range(INNER):
                        body()
            graphs[name] = g
        except Exception as exc:  # noqa: BLE001  (torch refuses the capture: say so, do not time it)
            torch.cuda.synchronize()
            notes.append(f"  ({name}: torch did not allow the capture: {type(exc).__name__}: {str(exc).splitlines()[0][:160]})")
    torch.cuda.synchronize()
    assert "pz_sample" in graphs and "copy" in graphs
    names = [name for name in bodies if name == "torch eager" or name in graphs]
    times, reps = measure(names, lambda name: bodies[name]() if name == "torch eager" else graphs[name].replay(), args, side,
                          graphed=tuple(graphs))
    ok = report(f"\n== sampling: {n} games, A = {A}, both agents, {dtype} logits, int64 actions: {total} algorithmic bytes "
                f"({total / (2 * n):.0f} per game and agent); pz_sample within the judge's tolerances; {args.rounds} interleaved rounds",
                names, times, reps, total, "pz_sample", ("torch eager", "torch graph"))
    for note in notes:
        print(note, flush=True)
    del graphs

    # ---- the update side -----------------------------------------------------------------------------------------------
    actions = {a: torch.from_numpy(rng.integers(0, A, n)).to(dev) for a in AGENTS}
    w_logp = {a: torch.from_numpy(rng.normal(size=n).astype(np.float32)).to(dev) for a in AGENTS}
    w_ent = {a: torch.from_numpy(rng.normal(size=n).astype(np.float32)).to(dev) for a in AGENTS}
    leaves = {name: {a: logits[a].clone().requires_grad_(True) for a in AGENTS} for name in ("pz_log_probs", "torch fwd+bwd")}
    lib = policy.load()
    fwd = {a: (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)) for a in AGENTS}
    grad = {a: torch.empty((n, A), dtype=tdtype, device=dev) for a in AGENTS}
    fmt = policy.LOGIT_FORMATS[tdtype]

    def cabi():
        stream = torch.cuda.current_stream().cuda_stream
        p = lambda d, i=None: [(d[a] if i is None else d[a][i]).data_ptr() for a in AGENTS]  # noqa: E731
        assert lib.pz_action_log_probs(*p(logits), fmt, A, n, A, 1, *p(actions), *p(fwd, 0), *p(fwd, 1), stream) == 0
        assert lib.pz_action_log_probs_backward(*p(logits), fmt, A, n, A, 1, *p(actions), *p(w_logp), *p(w_ent), *p(grad), A, stream) == 0

    update = {"pz_log_probs": lambda: pz_update(leaves["pz_log_probs"], actions, w_logp, w_ent), "pz fwd+bwd": cabi,
              "torch fwd+bwd": lambda: torch_update(leaves["torch fwd+bwd"], actions, w_logp, w_ent)}
    for body in update.values():
        body()
    torch.cuda.synchronize()
    for a in AGENTS:
        st = J.stats(host[a][games])
        acts = actions[a].cpu().numpy()[games]
        want, tol = J.gradient(st, acts, w_logp[a].cpu().numpy()[games], w_ent[a].cpu().numpy()[games])
        rounded, ulp = J.round_to(want, dtype)
        for name, got in (("pz_log_probs", leaves["pz_log_probs"][a].grad), ("pz fwd+bwd", grad[a])):
            err = np.abs(got.float().cpu().numpy()[games].astype(np.float64) - rounded)
            assert (err <= tol + (ulp if dtype != "float32" else 0)).all(), (name, a, float(err.max()))
        if dtype == "float32":
            assert np.abs(leaves["torch fwd+bwd"][a].grad.cpu().numpy()[games] - want).max() <= 1e-5
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(INNER):
                cabi()
    torch.cuda.synchronize()
    names = list(update)
    times, reps = measure(names, lambda name: g.replay() if name == "pz fwd+bwd" else update[name](), args, side,
                          graphed=("pz fwd+bwd",))
    total_u = 2 * n * (2 * A * esize + 8 + 4 + 4 + A * esize + 8 + 4 + 4)  # forward reads + writes, backward reads + the gradient
    ok2 = report(f"\n== update side: forward + backward of log-prob and entropy of given actions, {n} games, both agents, {dtype} logits: "
                 f"{total_u} algorithmic bytes of the two launches; both pz forms within the judge's gradient tolerance",
                 names, times, reps, total_u, "pz_log_probs", ("torch fwd+bwd",))
    del g
    torch.cuda.empty_cache()
    return ok, ok2


def registers():
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(policy.LIB_PATH):
            print(f"  {name.split('(')[0].replace('void ', ''):36s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch "
                  f"{r['.private_segment_fixed_size']}  spilled VGPRs {r['.vgpr_spill_count']}  LDS {r['.group_segment_fixed_size']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[65536, 524288, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = policy.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_policy_build_id().decode()}", flush=True)
    registers()
    slower = []
    for n in args.cells:
        for dtype in ("float32", "bfloat16"):
            ok, ok2 = time_cell(n, dtype, args)
            if not ok:
                slower.append((n, dtype, "sampling"))
            if not ok2:
                slower.append((n, dtype, "update"))
    print(f"\ncells where the pz form is not faster than every torch form: {slower or 'none'}", flush=True)


if __name__ == "__main__":
    main()
