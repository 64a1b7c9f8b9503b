#!/usr/bin/env python3
"""What the policy net's update side costs (diagnostic): ActorCritic.evaluate + backward(grad) -- net.forward and
netgrad.backward behind torch autograd -- against the torch route it replaces, and pz_mlp_backward alone against a copy.

    python tools/time_policy_net_backward.py [--rounds 7] [--min-time 0.05] [--cells 4096 65536 524288]

Per cell (rows; both agents on shared weights, 35 -> 64 -> 64 -> 19, tanh; float32-normalised and raw int32 observations),
interleaved in one process over --rounds rounds, the order rotating; every variant sets the six .grad anew:
    pz update       model.evaluate(obs) for both agents, then backward(grad_head): one forward launch and one pz_mlp_backward
                    call, 16 updates per hipGraph replay, reported per update;
    pz eager        the same, eagerly;
    torch graph     model.forward(obs) + head.backward(grad_head) per agent, torch autograd, captured into a hipGraph, 16 per
                    replay: THE REFERENCE POINT of this tool;
    torch eager     the same, eagerly: what examples/ppo_selfplay.py ran before;
    pz backward     netgrad.backward(out=, workspace=) alone, 16 per replay;
    copy            a device-to-device copy of pz_mlp_backward's algorithmic bytes (half read, half written), 16 per replay.
Before it is timed, netgrad.backward is compared with the judge of the tests (tests/netgrad_judge.py) where the batch is small
enough for the float64 judge (<= 65 536 rows per agent), and the torch route's gradients are held to twice its tolerance.
Reported: median and spread (max - min) in us, and the floors of pz_mlp_backward: the arithmetic at 157 TFLOPS (three times the
forward's 7 552 multiply-adds per row) and the bytes at 6.3 TB/s.  A cell where `pz update` is not faster than `torch graph` by
more than the sum of both spreads is marked *slower*.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
import netgrad_judge as G  # noqa: E402  (tests/: the definition in numpy float64)
from pikazoo_amd import net, netgrad  # noqa: E402
from time_policy_head import ACHIEVABLE, AGENTS, INNER, measure  # noqa: E402
from time_policy_net import MATRIX_RATE, capture  # noqa: E402

K, H, O, A = 35, 64, 19, 18
JUDGED_ROWS = 65536
FORMS = (("float32 normalised", torch.float32), ("int32 raw", torch.int32))


def time_cell(n, form, args):
    label, dtype = form
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    if dtype == torch.float32:
        obs = {a: torch.rand((n, K), generator=gen, device=dev) for a in AGENTS}
    else:
        obs = {a: torch.randint(-20, 433, (n, K), generator=gen, device=dev, dtype=torch.int32) for a in AGENTS}
    grad = {a: (torch.rand((n, O), generator=gen, device=dev) * 2 - 1) / n for a in AGENTS}
    torch.manual_seed(1)
    model = net.ActorCritic(K, H, A).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
        if dtype == torch.int32:
            model.fc1.weight.mul_(1.0 / 432)
    params = model.parameter_tensors()
    raw = [p.detach() for p in params]
    side = torch.cuda.Stream()
    ws = netgrad.workspace(n, K, H, O, dev)
    out = netgrad.backward(obs, raw, grad, workspace=ws)

    def pz_update():
        for p in params:
            p.grad = None
        head = model.evaluate(obs)
        torch.autograd.backward([head[a] for a in AGENTS], [grad[a] for a in AGENTS])

    def torch_update():
        for p in params:
            p.grad = None
        for a in AGENTS:
            model(obs[a]).backward(grad[a])

    # ---- judged before it is timed
    torch_update()
    theirs = [p.grad.clone() for p in params]
    pz_update()
    assert all(torch.equal(p.grad, o) for p, o in zip(params, out)), "evaluate + backward is not netgrad.backward"
    torch.cuda.synchronize()
    worst = None
    if n <= JUDGED_ROWS:
        host = [p.cpu().numpy() for p in raw]
        refs, tols, _ = G.judge([(obs[a].cpu().numpy(), grad[a].cpu().numpy()) for a in AGENTS], host, "tanh")
        worst, beyond = G.worst_share([o.cpu().numpy() for o in out], refs, tols)
        assert not beyond, (label, n, worst, beyond)
        assert not G.worst_share([t.cpu().numpy() for t in theirs], refs, [2 * t for t in tols])[1], (label, n)
    # ---- the variants
    esize = obs[AGENTS[0]].element_size()
    total = 2 * n * (K * esize + O * 4) + 4 * sum(p.numel() for p in raw)
    src, dst = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)
    bodies = {
        "pz update": pz_update,
        "pz eager": pz_update,
        "torch graph": torch_update,
        "torch eager": torch_update,
        "pz backward": lambda: netgrad.backward(obs, raw, grad, out=out, workspace=ws),
        "copy": lambda: dst.copy_(src),
    }
    graphs, notes = {}, []
    for name in ("pz update", "torch graph", "pz backward", "copy"):
        try:
            graphs[name] = capture(bodies[name], INNER, side)
        except Exception as exc:  # noqa: BLE001  (torch refuses the capture: say so, do not time it)
            torch.cuda.synchronize()
            notes.append(f"  ({name}: torch did not allow the capture: {type(exc).__name__}: {str(exc).splitlines()[0][:160]})")
    torch.cuda.synchronize()
    assert "pz backward" in graphs and "copy" in graphs, notes
    names = [name for name in bodies if name in graphs or name.endswith("eager")]
    times, reps = measure(names, lambda name: graphs[name].replay() if name in graphs else bodies[name](), args, side, graphed=tuple(graphs))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    flops_floor = 3 * 2 * n * 2 * (K * H + H * H + H * O) / MATRIX_RATE * 1e6
    bytes_floor = total / ACHIEVABLE * 1e6
    judged = f"netgrad.backward within {worst:.2g} of the judge's tolerance" if worst is not None else "too many rows for the float64 judge"
    print(f"\n== policy net update: {n} rows, both agents, shared weights, {K}-{H}-{H}-{O} tanh, {label} observations: {total} algorithmic "
          f"bytes of the backward; {judged}; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        print(f"  {name:12s} median {med[name]:10.2f} us  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)", flush=True)
    print(f"  floors of pz backward: arithmetic {flops_floor:.2f} us at 157 TFLOPS, bytes {bytes_floor:.2f} us at 6.3 TB/s; pz backward is at "
          f"{med['pz backward'] / max(flops_floor, bytes_floor):.1f}x of the larger and {med['pz backward'] / med['copy']:.2f}x the copy's time",
          flush=True)
    ours = "pz update" if "pz update" in med else "pz eager"
    verdicts = []
    for ref in ("torch graph", "torch eager"):
        if ref in med:
            faster = med[ours] < med[ref] - (spread[ours] + spread[ref])
            verdicts.append((ref, faster))
            print(f"  {ours} vs {ref} {med[ref] / med[ours]:.2f}x -> "
                  f"{'faster by more than both spreads' if faster else '*slower* (or within the spreads)'}", flush=True)
    for note in notes:
        print(note, flush=True)
    del graphs
    torch.cuda.empty_cache()
    return dict(verdicts).get("torch graph")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", type=int, default=[4096, 65536, 524288])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-time", type=float, default=0.05)
    args = ap.parse_args()
    lib = netgrad.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_netgrad_build_id().decode()}", flush=True)
    try:
        import kernel_notes

        for name, r in kernel_notes.notes(netgrad.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:44s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                  f"spilled VGPRs {r['.vgpr_spill_count']}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    slower = []
    for n in args.cells:
        for form in FORMS:
            verdict = time_cell(n, form, args)
            if verdict is not True:
                slower.append((n, form[0], "not captured" if verdict is None else "slower"))
    print(f"\ncells where pz update is not faster than the captured torch route by more than both spreads: {slower or 'none'}", flush=True)


if __name__ == "__main__":
    main()
