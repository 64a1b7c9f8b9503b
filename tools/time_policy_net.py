#!/usr/bin/env python3
"""What the policy net's forward costs (diagnostic): pz_mlp_forward against the torch route it replaces on the rollout side,
a copy, and the rollout step as a whole.

    python tools/time_policy_net.py [--rounds 7] [--min-time 0.05] [--cells 65536 524288 4096]

Per cell (rows; both agents on shared weights, 35 -> 64 -> 64 -> 19, tanh; float32-normalised, bfloat16-normalised and raw
int32 observations), interleaved in one process over --rounds rounds, the order rotating:
    pz net          net.forward(out=previous result): ONE launch, 16 calls per hipGraph replay (a replay costs the host some
                    10 us), reported per call;
    torch graph     the torch route under no_grad -- the cast where the dtype needs one, F.linear x 3 and tanh x 2 per agent --
                    captured into a hipGraph, 16 calls per replay: THE REFERENCE POINT of this tool;
    torch eager     the same, eagerly;
    copy            a device-to-device copy of the algorithmic bytes (half read, half written), 16 per replay;
    pz step         the rollout step as a whole: pz net + pz_sample_actions + pz_step in one captured graph (env.step's own
                    launch on the observations it wrote the step before);
    torch step      the torch route + the same two.
Before it is timed the pz net is compared with the judge of the tests (tests/net_judge.py) on the first and the last
2 048 rows of each agent, and the torch route is held to twice the judge's tolerance of it.  Reported: median and spread
(max - min) in us per call, the algorithmic bytes over the median, and the two floors of the launch: the arithmetic at
157 TFLOPS (exact-float32 matrix rate; 7 552 multiply-adds per row) and the bytes at 6.3 TB/s.  A cell where `pz net` is
not faster than `torch graph` by more than the sum of both spreads is marked *slower*.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd", REPO / "tests", REPO / "tools"):
    sys.path.insert(0, str(p))
import net_judge as N  # noqa: E402  (tests/: the definition in numpy float64)
from pikazoo_amd import net, pikazoo_v0, policy  # noqa: E402
from pikazoo_amd.wrappers import NormalizeObservation  # noqa: E402
from time_policy_head import ACHIEVABLE, AGENTS, CHECKED, INNER, measure  # noqa: E402

K, H, O, A = 35, 64, 19, 18
MATRIX_RATE = 157e12  # FLOP per second of v_mfma_f32_32x32x2_f32 over the chip
FORMS = (("float32 normalised", torch.float32, True), ("bfloat16 normalised", torch.bfloat16, True), ("int32 raw", torch.int32, False))


def torch_route(obs, params, out):
    W1, b1, W2, b2, W3, b3 = params
    with torch.no_grad():
        for a in AGENTS:
            x = obs[a] if obs[a].dtype == torch.float32 else obs[a].to(torch.float32)
            out[a].copy_(F.linear(torch.tanh(F.linear(torch.tanh(F.linear(x, W1, b1)), W2, b2)), W3, b3))


def capture(body, inner, side):
    with torch.cuda.stream(side):
        for _ in range(3):
            body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(inner):
                body()
    return g


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
    assert all(obs[a].dtype == dtype and tuple(obs[a].shape) == (n, K) for a in AGENTS), (obs[AGENTS[0]].dtype, obs[AGENTS[0]].shape)
    torch.manual_seed(1)
    model = net.ActorCritic(K, H, A).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1))
        if not normalise:
            model.fc1.weight.mul_(1.0 / 432)
    params = model.parameter_tensors()
    side = torch.cuda.Stream()
    # ---- judged before it is timed
    head = model.act(obs)
    theirs = {a: torch.empty((n, O), dtype=torch.float32, device=dev) for a in AGENTS}
    torch_route(obs, params, theirs)
    torch.cuda.synchronize()
    rows = np.r_[0:min(CHECKED, n), max(n - CHECKED, 0):n]
    host = [p.detach().cpu().numpy() for p in params]
    worst = 0.0
    for a in AGENTS:
        x = obs[a][rows]
        x = (x.float() if dtype == torch.bfloat16 else x).cpu().numpy()
        ref, tol = N.judge(x, host, "tanh")
        share, _ = N.worst_share(head[a][rows].cpu().numpy(), ref, tol)
        assert share <= 1, (label, a, share)
        worst = max(worst, share)
        assert N.worst_share(theirs[a][rows].cpu().numpy(), ref, 2 * tol)[0] <= 1, (label, a)
    # ---- the variants
    picked = policy.sample({a: head[a][:, :A] for a in AGENTS}, seed=3, step=0)
    esize = obs[AGENTS[0]].element_size()
    total = 2 * n * (K * esize + O * 4)
    src, dst = torch.empty(total // 2, dtype=torch.uint8, device=dev), torch.empty(total // 2, dtype=torch.uint8, device=dev)

    def rollout(forward):
        forward()
        policy.sample({a: head[a][:, :A] for a in AGENTS}, seed=3, step=0, out=picked)
        env.step(picked["actions"])

    bodies = {
        "pz net": lambda: model.act(obs, out=head),
        "torch graph": lambda: torch_route(obs, params, theirs),
        "torch eager": lambda: torch_route(obs, params, theirs),
        "copy": lambda: dst.copy_(src),
        "pz step": lambda: rollout(lambda: model.act(obs, out=head)),
        "torch step": lambda: rollout(lambda: torch_route(obs, params, head)),
    }
    graphs, notes = {}, []
    for name in ("pz net", "torch graph", "copy", "pz step", "torch step"):
        try:
            graphs[name] = capture(bodies[name], INNER, side)
        except Exception as exc:  # noqa: BLE001  (torch refuses the capture: say so, do not time it)
            torch.cuda.synchronize()
            notes.append(f"  ({name}: torch did not allow the capture: {type(exc).__name__}: {str(exc).splitlines()[0][:160]})")
    torch.cuda.synchronize()
    assert "pz net" in graphs and "torch graph" in graphs and "copy" in graphs, notes
    names = [name for name in bodies if name in graphs or name == "torch eager"]
    times, reps = measure(names, lambda name: graphs[name].replay() if name in graphs else bodies[name](), args, side, graphed=tuple(graphs))
    med = {name: statistics.median(times[name]) for name in names}
    spread = {name: max(times[name]) - min(times[name]) for name in names}
    flops_floor = 2 * n * 2 * (K * H + H * H + H * O) / MATRIX_RATE * 1e6
    bytes_floor = total / ACHIEVABLE * 1e6
    print(f"\n== policy net forward: {n} rows, both agents, shared weights, {K}-{H}-{H}-{O} tanh, {label} observations: {total} algorithmic "
          f"bytes; pz net within {worst:.4f} of the judge's tolerance; {args.rounds} interleaved rounds", flush=True)
    for name in names:
        rate = total / (med[name] * 1e-6)
        print(f"  {name:12s} median {med[name]:10.2f} us per call  spread {spread[name]:8.2f}  ({reps[name]:4d} runs per sample)  "
              f"{rate / 1e9:8.1f} GB/s", flush=True)
    faster = med["pz net"] < med["torch graph"] - (spread["pz net"] + spread["torch graph"])
    binds = "arithmetic" if flops_floor > bytes_floor else "bytes"
    print(f"  floors: arithmetic {flops_floor:.2f} us at 157 TFLOPS, bytes {bytes_floor:.2f} us at 6.3 TB/s: the {binds} floor binds; pz net is at "
          f"{med['pz net'] / max(flops_floor, bytes_floor):.1f}x of it and {med['pz net'] / med['copy']:.2f}x the copy's time", flush=True)
    step = (f"; the rollout step {med['pz step']:.2f} us against {med['torch step']:.2f} us ({med['torch step'] / med['pz step']:.1f}x)"
            if "pz step" in med and "torch step" in med else "")
    print(f"  pz net vs torch graph {med['torch graph'] / med['pz net']:.1f}x, vs torch eager {med['torch eager'] / med['pz net']:.1f}x{step}"
          f" -> {'faster than the captured torch route by more than both spreads' if faster else '*slower*'}", flush=True)
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
    lib = net.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library build {lib.pz_net_build_id().decode()}", flush=True)
    try:
        import kernel_digest
        import kernel_notes

        counts = kernel_digest.kernels(net.LIB_PATH) if kernel_digest.available() else {}
        for name, r in kernel_notes.notes(net.LIB_PATH):
            short = name.split("(")[0].replace("void ", "")
            print(f"  {short:36s} VGPRs {r['.vgpr_count']:3d}  SGPRs {r['.sgpr_count']:3d}  scratch {r['.private_segment_fixed_size']}  "
                  f"spilled VGPRs {r['.vgpr_spill_count']}  spilled SGPRs {r['.sgpr_spill_count']}  static LDS {r['.group_segment_fixed_size']}  "
                  f"instructions {counts.get(short, ('', '?'))[1]}", flush=True)
    except Exception as exc:  # noqa: BLE001
        print(f"(no code-object notes: {exc})", flush=True)
    slower = []
    for n in args.cells:
        for form in FORMS:
            if not time_cell(n, form, args):
                slower.append((n, form[0]))
    print(f"\ncells where pz net is not faster than the captured torch route by more than both spreads: {slower or 'none'}", flush=True)


if __name__ == "__main__":
    main()
