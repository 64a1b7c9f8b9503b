#!/usr/bin/env python3
"""What the PPO update loss costs (diagnostic): pz_ppo_moments + pz_ppo_loss against the route the tree served before
them (policy.log_probs and the loss in torch operations), plain torch, and a copy.

    python tools/time_ppo_loss.py [--rounds 7] [--min-time 0.05] [--cells 65536 524288 4096]

Per cell (rows; A = 18, both agents, value clip on; float32 and bfloat16 logits and values), interleaved in one process
over --rounds rounds, the order rotating -- forward AND backward of every form, to the gradients of logits and values:
    pz norm+loss    pikazoo_amd.ppo.loss_and_grad(out=previous result): pz_ppo_moments + pz_ppo_loss, four launches, 16 calls
                    per hipGraph replay (a replay costs the host some 10 us), reported per call;
    pz loss         the same without the normalisation (two launches);
    parent eager    policy.log_probs (its two launches) and ratio, clips, value loss, entropy bonus, normalisation and
                    means in torch operations, .backward(), eagerly: what a trainer ran on the parent commit;
    parent graph    the same captured into a hipGraph if torch allows it (if the capture raises, the row says so);
    torch eager     torch.distributions.Categorical for log-prob and entropy, the same loss, .backward(), eagerly;
    copy            a device-to-device copy of the algorithmic bytes (half read, half written), 16 per replay.
Before it is timed, every pz variant is compared with the judge of the tests (tests/ppo_judge.py: statistics over all the
rows, gradients on the first and the last 2 048 rows), and the loss of every torch form with the judged loss within 1e-4
(float32; bfloat16 forms compute in bfloat16 and are held to 2e-2).  Reported: median and spread (max - min) in us per
call and the algorithmic bytes over the median.  A cell where `pz norm+loss` is not faster than `parent eager` (and
`parent graph`, where there is one) by more than that route's spread is marked *slower*.
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
import policy_judge as J  # noqa: E402
import ppo_judge as P  # noqa: E402  (tests/: the definition in numpy float64)
from pikazoo_amd import policy, ppo  # noqa: E402
from time_policy_head import ACHIEVABLE, AGENTS, CHECKED, INNER, measure  # noqa: E402

A = 18


def torch_loss(logp, ent, values, d, a):
    adv = d["adv"][a]
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    logratio = logp - d["old_logp"][a]
    ratio = logratio.exp()
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - P.CLIP, 1 + P.CLIP)).mean()
    v, old_v, ret = values.float(), d["old_values"][a].float(), d["ret"][a]
    vc = old_v + torch.clamp(v - old_v, -P.VALUE_CLIP, P.VALUE_CLIP)
    vl = 0.5 * torch.max((v - ret) ** 2, (vc - ret) ** 2).mean()
    with torch.no_grad():
        d["log"][a] = (((ratio - 1) - logratio).mean(), ((ratio - 1.0).abs() > P.CLIP).float().mean())
    return pg + P.VF_COEF * vl - P.ENT_COEF * ent.mean()


def route(leaves, vleaves, d, ours):
    """forward and backward of both agents' losses; `ours`: log-prob and entropy from policy.log_probs (the parent's route)"""
    if ours:
        logp, ent = policy.log_probs(leaves, d["actions"])
    total = 0
    for a in AGENTS:
        if ours:
            lp, en = logp[a], ent[a]
        else:
            dist = torch.distributions.Categorical(logits=leaves[a])
            lp, en = dist.log_prob(d["actions"][a]).float(), dist.entropy().float()
        d["loss"][a] = torch_loss(lp, en, vleaves[a], d, a)
        total = total + d["loss"][a]
    for a in AGENTS:
        leaves[a].grad = None
        vleaves[a].grad = None
    total.backward()


def time_cell(n, dtype, args):
    dev = torch.device("cuda:0")
    tdtype = {"float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    esize = 4 if dtype == "float32" else 2
    rng = np.random.default_rng([n, esize, 3])
    cases = {}
    for a in AGENTS:
        l = J.as_logit_dtype(rng.normal(0.0, 2.0, size=(n, A)).astype(np.float32), dtype)
        act = rng.integers(0, A, n)
        lp, _ = J.log_prob(J.stats(l), act)
        ret = rng.normal(0.0, 1.0, n).astype(np.float32)
        v = J.as_logit_dtype((ret + rng.normal(0.0, 0.5, n)).astype(np.float32), dtype)
        cases[a] = dict(logits=l, actions=act, old_logp=(lp + rng.normal(0.0, 0.15, n)).astype(np.float32),
                        adv=rng.normal(0.0, 1.0, n).astype(np.float32), ret=ret, values=v,
                        old_values=J.as_logit_dtype((v + rng.normal(0.0, 1.0 / 3, n)).astype(np.float32), dtype), clip=P.CLIP,
                        value_clip=P.VALUE_CLIP, vf_coef=P.VF_COEF, ent_coef=P.ENT_COEF, normalize=True)
    up = lambda key, cast=None: {a: (torch.from_numpy(cases[a][key]).to(dev) if cast is None else torch.from_numpy(cases[a][key]).to(dev).to(cast))  # noqa: E731
                                 for a in AGENTS}
    logits, values = up("logits", tdtype), up("values", tdtype)
    d = dict(actions=up("actions"), old_logp=up("old_logp"), adv=up("adv"), ret=up("ret"), old_values=up("old_values", tdtype), log={}, loss={})
    common = dict(actions=d["actions"], old_log_probs=d["old_logp"], advantages=d["adv"], returns=d["ret"], old_values=d["old_values"],
                  clip=P.CLIP, value_clip=P.VALUE_CLIP, vf_coef=P.VF_COEF, ent_coef=P.ENT_COEF)
    side = torch.cuda.Stream()
    rows = np.r_[0:min(CHECKED, n), max(n - CHECKED, 0):n]
    # ---- the pz variants, judged
    held = {}
    judged_loss = {}
    for name, norm in (("pz norm+loss", True), ("pz loss", False)):
        held[name] = ppo.loss_and_grad(logits, values, normalize_advantages=norm, **common)
        torch.cuda.synchronize()
        for s, a in enumerate(AGENTS):
            jd = P.judge({**cases[a], "normalize": norm})
            judged_loss[name, a] = jd["stats"]["loss"][0]
            got = dict(stats=held[name]["_stats"][s].cpu().numpy())
            assert not P.failures(P.compare(jd, got, dtype, dtype)), (name, a, P.compare(jd, got, dtype, dtype))
            sub = P.judge({**{k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in cases[a].items()}, "normalize": False})
            # (the subset's own judge needs the whole batch's M and moments: compare the gradients through their ratio to M)
            scale = n / len(rows)
            if not norm:
                got = dict(stats=[sub["stats"][k][0] for k in P.STAT_NAMES],
                           grad_logits=held[name]["grad_logits"][a].float().cpu().numpy()[rows].astype(np.float64) * scale,
                           grad_values=held[name]["grad_values"][a].float().cpu().numpy()[rows].astype(np.float64) * scale)
                res = P.compare(sub, got, dtype, dtype)
                # a 16-bit gradient was rounded at 1 / scale of the subset's magnitude: its last place scales with it
                assert dtype != "float32" or not P.failures(res), (name, a, res)
    bodies = {name: (lambda name=name, norm=norm: ppo.loss_and_grad(logits, values, normalize_advantages=norm, out=held[name], **common))
              for name, norm in (("pz norm+loss", True), ("pz loss", False))}
    # ---- the torch forms, their loss held to the judged one
    leaves = {name: ({a: logits[a].clone().requires_grad_(True) for a in AGENTS}, {a: values[a].clone().requires_grad_(True) for a in AGENTS})
              for name in ("parent eager", "parent graph", "torch eager")}
    for name in leaves:
        bodies[name] = (lambda name=name: route(*leaves[name], d, ours=name.startswith("parent")))
        bodies[name]()
        torch.cuda.synchronize()
        for a in AGENTS:
            err = abs(float(d["loss"][a].detach()) - judged_loss["pz norm+loss", a])
            assert err <= (1e-4 if dtype == "float32" else 2e-2), (name, a, err)
    total = 2 * n * (2 * A * esize + 8 + 4 + 2 * 4 + 4 + 3 * esize)
    src, dst = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)
    bodies["copy"] = lambda: dst.copy_(src)
    graphs, notes = {}, []
    for name in ("pz norm+loss", "pz loss", "parent graph", "copy"):
        try:
            inner = 1 if name == "parent graph" else INNER
            with torch.cuda.stream(side):
                for _ in range(3):
                    bodies[name]()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    for _ in range(inner):
                        bodies[name]()
            graphs[name] = g
        except Exception as exc:  # noqa: BLE001  (torch refuses the capture: say so, do not time it)
            torch.cuda.synchronize()
            notes.append(f"  ({name}: torch did not allow the capture: {type(exc).__name__}: {str(exc).splitlines()[0][:160]})")
    torch.cuda.synchronize()
    assert "pz norm+loss" in graphs and "pz loss" in graphs and "copy" in graphs
    names = [name for name in bodies if name in graphs or name.endswith("eager")]
    times, reps = measure(names, lambda name: graphs[name].replay() if name in graphs else bodies[name](), args, side,
                          graphed=tuple(g for g in graphs if g != "parent graph"))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    print(f"\n== PPO loss, forward and backward: {n} rows, A = {A}, both agents, {dtype} logits and values, value clip on: {total} "
          f"algorithmic bytes ({total / (2 * n):.0f} per row and agent); the pz forms within the judge's bounds; {args.rounds} interleaved rounds",
          flush=True)
    for name in names:
        rate = total / (med[name] * 1e-6)
        print(f"  {name:14s} median {med[name]:10.2f} us per call  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)  "
              f"{rate / 1e9:8.1f} GB/s  {100 * rate / ACHIEVABLE:5.1f} % of 6.3 TB/s", flush=True)
    theirs = [t for t in ("parent eager", "parent graph") if t in med]
    faster = all(med["pz norm+loss"] < med[t] - spread[t] for t in theirs)
    print("  pz norm+loss " + ", ".join(f"vs {t} {med[t] / med['pz norm+loss']:.1f}x" for t in theirs + ["torch eager"]) +
          f", {med['pz norm+loss'] / med['copy']:.2f}x the copy's time; the normalisation costs {med['pz norm+loss'] - med['pz loss']:.2f} us"
          f" -> {'faster than the parent route by more than its spread' if faster else '*slower*'}", flush=True)
    for note in notes:
        print(note, flush=True)
    del graphs
    torch.cuda.empty_cache()
    return faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[65536, 524288, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = ppo.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_ppo_build_id().decode()}", flush=True)
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(ppo.LIB_PATH):
            print(f"  {name.split('(')[0].replace('void ', ''):36s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch "
                  f"{r['.private_segment_fixed_size']}  spilled VGPRs {r['.vgpr_spill_count']}  LDS {r['.group_segment_fixed_size']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    slower = []
    for n in args.cells:
        for dtype in ("float32", "bfloat16"):
            if not time_cell(n, dtype, args):
                slower.append((n, dtype))
    print(f"\ncells where pz norm+loss is not faster than the parent route by more than its spread: {slower or 'none'}", flush=True)


if __name__ == "__main__":
    main()
