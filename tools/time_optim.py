#!/usr/bin/env python3
"""What the optimizer step costs (diagnostic): pz_adam_step -- the gradient clip and Adam in one launch -- against the torch
route it replaces in each of its forms, and a whole captured minibatch update with either optimizer behind it.

    python tools/time_optim.py [--rounds 7] [--min-time 0.05] [--rows 4096 65536 524288]

Part 1, per cell (the default net 35-64-64-19 with 7 571 parameters and the largest box 72-128-128-40 with 31 016; one group
and two), interleaved in one process over --rounds rounds, the order rotating:
    pz step           optim.adam_step(max_grad_norm=0.5), 16 per hipGraph replay, reported per step;
    pz eager          optim.Adam.step(), eagerly (the launch behind its cached plan);
    torch eager       clip_grad_norm_(..., 0.5) + torch.optim.Adam.step() (foreach), eagerly: what examples/ppo_selfplay.py ran;
    torch capturable  the same with capturable=True, captured, 16 per replay;
    torch fused       the same with fused=True, capturable=True, captured, 16 per replay;
    copy              a device-to-device copy of the step's bytes (4 tensors read, 3 written: half read, half written), 16 per replay.
With two groups the torch route clips and steps each net on its own, as two nets are trained.  Before it is timed, one
optim.adam_step is held to the judge of the tests (tests/optim_judge.py).  A capture that torch refuses is recorded, not timed.
Part 2: net.forward -> ppo.loss_and_grad(head=) -> netgrad.backward -> the optimizer, both agents on shared weights, one captured
graph per optimizer, 16 updates per replay.
Reported: median and spread (max - min) in us.  `pz step` counts as faster than a torch form only when it wins by more than the
sum of both spreads; otherwise the cell is printed as *slower*.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
import optim_judge as J  # noqa: E402  (tests/: the definition in numpy float64)
from pikazoo_amd import net, netgrad, optim, ppo  # noqa: E402
from time_policy_head import AGENTS, INNER, measure  # noqa: E402
from time_policy_net import capture  # noqa: E402

NETS = (("default net 35-64-64-19", J.DEFAULT_NET), ("largest box 72-128-128-40", J.LARGEST_BOX))
CLIP, LR, EPS = 0.5, 3e-4, 1e-5
TORCH_FORMS = (("torch eager", dict()), ("torch capturable", dict(capturable=True)), ("torch fused", dict(fused=True, capturable=True)))


def verdict_lines(med, spread, ours, refs):
    """[(reference, faster by more than both spreads?)] and the printed lines"""
    out = []
    for ref in refs:
        if ref in med:
            faster = med[ours] < med[ref] - (spread[ours] + spread[ref])
            out.append((ref, faster))
            print(f"  {ours} vs {ref} {med[ref] / med[ours]:.2f}x -> {'faster by more than both spreads' if faster else '*slower* (or within the spreads)'}",
                  flush=True)
    return out


def run_variants(title, bodies, captured, args, side):
    graphs, notes = {}, []
    for name in captured:
        try:
            graphs[name] = capture(bodies[name], INNER, side)
        except Exception as exc:  # noqa: BLE001  (torch refuses the capture: say so, do not time it)
            torch.cuda.synchronize()
            notes.append(f"  ({name}: torch did not allow the capture: {type(exc).__name__}: {str(exc).splitlines()[0][:160]})")
    torch.cuda.synchronize()
    names = [name for name in bodies if name in graphs or name not in captured]
    times, reps = measure(names, lambda name: graphs[name].replay() if name in graphs else bodies[name](), args, side, graphed=tuple(graphs))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    print(title, flush=True)
    for name in names:
        print(f"  {name:18s} median {med[name]:10.2f} us  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)", flush=True)
    for note in notes:
        print(note, flush=True)
    del graphs
    return med, spread


def torch_nets(shapes, n_groups, dev, form):
    """[(parameters, optimizer)] per net, gradients in place"""
    out = []
    for a in range(n_groups):
        grp = J.make_group(20 + a, shapes, J.GRAD_SCALE)
        ps = [torch.nn.Parameter(torch.from_numpy(p).to(dev)) for p in grp["p"]]
        for p, g in zip(ps, grp["g"]):
            p.grad = torch.from_numpy(g).to(dev)
        out.append((ps, torch.optim.Adam(ps, lr=LR, eps=EPS, **form)))
    return out


def torch_step(nets):
    for ps, opt in nets:
        torch.nn.utils.clip_grad_norm_(ps, CLIP)
        opt.step()


def time_step_cell(label, shapes, n_groups, args):
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    hosts = [J.make_group(20 + a, shapes, J.GRAD_SCALE) for a in range(n_groups)]
    state = [{k: [torch.from_numpy(x).to(dev) for x in h[k]] for k in "pgmv"} for h in hosts]
    words = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in hosts]
    stats = [torch.zeros(2, dtype=torch.float32, device=dev) for _ in hosts]

    def keyed(seqs):
        return seqs[0] if n_groups == 1 else {a: s for a, s in zip(AGENTS, seqs)}

    call = dict(lr=LR, eps=EPS, max_grad_norm=CLIP)

    def pz_step():
        optim.adam_step(keyed([s["p"] for s in state]), keyed([s["g"] for s in state]), keyed([s["m"] for s in state]),
                        keyed([s["v"] for s in state]), keyed(words), stats=keyed(stats), **call)

    # ---- judged before it is timed
    pz_step()
    torch.cuda.synchronize()
    worst = 0.0
    for h, s, w in zip(hosts, state, words):
        verdict = J.judge(h, J.options(**call))
        share, beyond = J.check_group({k: [x.cpu().numpy() for x in s[k]] for k in "pmv"}, verdict)
        assert not beyond and w.tolist() == [1, 0], (label, share, beyond)
        worst = max(worst, share)
    ours_nets = []
    for h in hosts:
        ps = [torch.nn.Parameter(torch.from_numpy(p).to(dev)) for p in h["p"]]
        for p, g in zip(ps, h["g"]):
            p.grad = torch.from_numpy(g).to(dev)
        ours_nets.append(ps)
    adam = optim.Adam([{"params": ps} for ps in ours_nets], lr=LR, eps=EPS, max_grad_norm=CLIP)
    total = 7 * 4 * n_groups * sum(x.size for x in hosts[0]["p"])
    src, dst = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)
    bodies = {"pz step": pz_step, "pz eager": adam.step}
    for name, form in TORCH_FORMS:
        nets = torch_nets(shapes, n_groups, dev, form)
        bodies[name] = lambda nets=nets: torch_step(nets)
    bodies["copy"] = lambda: dst.copy_(src)
    med, spread = run_variants(
        f"\n== optimizer step: {label}, {n_groups} group{'s' if n_groups > 1 else ''}: {total} bytes; optim.adam_step within {worst:.2g} of the "
        f"judge's tolerance; {args.rounds} interleaved rounds", bodies, ("pz step", "torch capturable", "torch fused", "copy"), args, side)
    print(f"  pz step is {med['pz step'] / med['copy']:.2f}x the copy's time", flush=True)
    verdicts = verdict_lines(med, spread, "pz step", [name for name, _ in TORCH_FORMS])
    torch.cuda.empty_cache()
    return bool(verdicts) and all(f for _, f in verdicts)


def time_update_cell(n, args):
    """the whole minibatch update in one captured graph, both agents on shared weights"""
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    K, H, A = 35, 64, 18
    gen = torch.Generator(device=dev).manual_seed(5)
    obs = {a: torch.rand((n, K), generator=gen, device=dev) for a in AGENTS}
    act = {a: torch.randint(0, A, (n,), generator=gen, device=dev, dtype=torch.int32) for a in AGENTS}
    old = {a: torch.full((n,), -2.9, device=dev) for a in AGENTS}
    adv = {a: torch.randn((n,), generator=gen, device=dev) for a in AGENTS}
    ret = {a: torch.randn((n,), generator=gen, device=dev) for a in AGENTS}

    def learner(make_optimizer):
        torch.manual_seed(1)
        model = net.ActorCritic(K, H, A).to(dev)
        P = [p.detach() for p in model.parameter_tensors()]
        ws = netgrad.workspace(n, K, H, A + 1, dev)
        box = dict(head=None, loss=None, grads=None)

        def gradients():
            box["head"] = net.forward(obs, P, out=box["head"])
            box["loss"] = ppo.loss_and_grad(actions=act, old_log_probs=old, advantages=adv, returns=ret, head=box["head"], num_actions=A,
                                            out=box["loss"])
            box["grads"] = netgrad.backward(obs, P, box["loss"]["grad_head"], out=box["grads"], workspace=ws)

        gradients()
        step = make_optimizer(model, P, box["grads"])

        def update():
            gradients()
            step()
        return update

    def pz(model, P, grads):
        m, v = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
        words = torch.zeros(2, dtype=torch.int64, device=dev)
        return lambda: optim.adam_step(P, list(grads), m, v, words, lr=LR, eps=EPS, max_grad_norm=CLIP)

    def torch_form(form):
        def make(model, P, grads):
            ps = list(model.parameter_tensors())
            for p, g in zip(ps, grads):
                p.grad = g  # (netgrad.backward writes into these tensors on every update)
            opt = torch.optim.Adam(ps, lr=LR, eps=EPS, **form)
            return lambda: torch_step([(ps, opt)])
        return make

    bodies = {"pz update": learner(pz)}
    for name, form in TORCH_FORMS[1:]:
        bodies[name.replace("torch", "torch update,")] = learner(torch_form(form))
    med, spread = run_variants(f"\n== whole minibatch update in one captured graph: {n} rows x 2 agents, shared weights, 35-64-64-19; "
                               f"{args.rounds} interleaved rounds", bodies, tuple(bodies), args, side)
    refs = [name for name in bodies if name != "pz update" and name in med]
    if not refs:
        return None
    best = min(refs, key=lambda name: med[name])
    not_slower = med["pz update"] <= med[best] + (spread["pz update"] + spread[best])
    faster = med["pz update"] < med[best] - (spread["pz update"] + spread[best])
    print(f"  pz update vs the best torch form ({best}) {med[best] / med['pz update']:.3f}x -> "
          f"{'faster by more than both spreads' if faster else ('within the spreads: not slower' if not_slower else '*slower*')}", flush=True)
    torch.cuda.empty_cache()
    return not_slower


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = optim.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_optim_build_id().decode()}; torch {torch.__version__}", flush=True)
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(optim.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:32s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  LDS {r['.group_segment_fixed_size']}  scratch "
                  f"{r['.private_segment_fixed_size']}  spilled VGPRs {r['.vgpr_spill_count']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    lost = []
    for label, shapes in NETS:
        for n_groups in (1, 2):
            if not time_step_cell(label, shapes, n_groups, args):
                lost.append(f"step: {label}, {n_groups} group(s)")
    for n in args.rows:
        verdict = time_update_cell(n, args)
        if verdict is not True:
            lost.append(f"update: {n} rows" + (" (no torch form was captured)" if verdict is None else ""))
    print(f"\ncells where the launch does not beat every torch form by more than both spreads, or the whole update is slower: {lost or 'none'}",
          flush=True)


if __name__ == "__main__":
    main()
