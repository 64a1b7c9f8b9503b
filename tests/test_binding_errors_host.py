"""CPU tests (no GPU needed) of what the learner's bindings SAY when they refuse a call: a table of bad calls on CPU tensors
through the public functions alone, each compared -- exception type and whole text -- with tests/golden/binding_errors.json.

The file was recorded before the bindings shared ``_launch`` and ``net``'s argument check: every sentence a moved helper
raises is pinned here through every function that reaches it without a GPU, and every function has one fully valid call,
which must end in the function's own "... on the GPU" ``ValueError`` -- so nothing in front of that check fires, and the
order of the checks is the recorded one.  (In ``policy``, ``ppo``, ``learn.gae`` and ``ppo.moments`` the GPU check comes
before the workspace and the overlap checks, in ``net.forward``, ``pool.forward`` and ``netgrad.backward`` before the
overlap check: those raises need a GPU and are not in this table.)

``python tests/test_binding_errors_host.py OUT.json COMMIT`` records the file from the tree it stands in."""
import json
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "binding_errors.json"
if __name__ == "__main__":  # the recorder; under pytest the conftest has put the package on the path
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def net_params(K=5, H=32, O=3):
    return [z(H, K), z(H), z(H, H), z(H), z(O, H), z(O)]


def put(ps, i, t):
    ps = list(ps)
    ps[i] = t
    return ps


# ---- the MLP argument check, through its three callers -----------------------------------------------------------------------
def mlp_callers():
    """{caller: f(obs, first, second, **kw)}: `first` and `second` are the parameter sets of agent / member 0 and 1"""
    from pikazoo_amd import net, netgrad, pool

    def per_agent(obs, first, second):
        return dict(zip(obs, (first, second))) if isinstance(obs, dict) and len(obs) == 2 else first

    def head_like(obs):
        like = lambda x: z(x.shape[0], 3) if isinstance(x, torch.Tensor) and x.dim() == 2 else None  # noqa: E731
        return {a: like(x) for a, x in obs.items()} if isinstance(obs, dict) else like(obs)

    def forward(obs, first, second, **kw):
        return net.forward(obs, per_agent(obs, first, second), **kw)

    def pool_forward(obs, first, second, plans="none", **kw):
        if plans == "none":
            plans = {a: None for a in obs} if isinstance(obs, dict) else None
        return pool.forward(obs, [first, second], plans, **kw)

    def backward(obs, first, second, grad_head="like", **kw):
        return netgrad.backward(obs, per_agent(obs, first, second), head_like(obs) if isinstance(grad_head, str) else grad_head, **kw)

    return {"net.forward": forward, "pool.forward": pool_forward, "netgrad.backward": backward}


def mlp_cases():
    from pikazoo_amd import pool

    good, two = z(4, 5), {"a": z(4, 5), "b": z(4, 5)}
    ps = net_params()
    shared = {   # name: (obs, first, second, kw) -- the observation geometry and the net's box, the same for all three callers
        "obs: three agents": ({"a": good, "b": good, "c": good}, ps, ps, {}),
        "obs: no agent": ({}, ps, ps, {}),
        "obs: not a tensor": ([good], ps, ps, {}),
        "obs: not a tensor in a dict": ({"a": good, "b": 1.5}, ps, ps, {}),
        "obs: one dimension": (z(4), ps, ps, {}),
        "obs: no feature": (z(4, 0), ps, ps, {}),
        "obs: 73 features": (z(4, 73), ps, ps, {}),
        "obs: more than 2^30 rows": (z(1, 5).expand((1 << 30) + 1, 5), ps, ps, {}),
        "obs: uint8": (z(4, 5, dtype=torch.uint8), ps, ps, {}),
        "rows: the agents differ in shape": ({"a": good, "b": z(3, 5)}, ps, ps, {}),
        "rows: the agents differ in dtype": ({"a": good, "b": z(4, 5, dtype=torch.int32)}, ps, ps, {}),
        "rows: last dimension strided": (z(4, 10)[:, ::2], ps, ps, {}),
        "rows: rows overlap": (z(1, 5).expand(4, 5), ps, ps, {}),
        "rows: two row strides": ({"a": good, "b": z(4, 10)[:, :5]}, ps, ps, {}),
        "activation": (good, ps, ps, {"activation": "gelu"}),
        "W1: one dimension": (good, put(ps, 0, z(32)), ps, {}),
        "hidden: 48": (good, net_params(H=48), ps, {}),
        "W3: one dimension": (good, put(ps, 4, z(3)), ps, {}),
        "out_features: 41": (good, net_params(O=41), ps, {}),
        "shape: b1 of set 0": (two, put(ps, 1, z(31)), ps, {}),
        "shape: W2 of set 1 is float64": (two, ps, put(ps, 2, z(32, 32, dtype=torch.float64)), {}),
        "shape: W1 of set 1 for other features": (two, ps, net_params(K=6), {}),
        "shape: W2 of set 1 not contiguous": (two, ps, put(ps, 2, z(32, 64)[:, ::2]), {}),
        "valid": (good, ps, ps, {}),
        "valid: two agents at a row stride": ({"a": z(4, 8)[:, :5], "b": z(4, 8)[:, :5]}, ps, ps, {}),
    }
    forwards = {  # the out / out_dtype block of the two forwards
        "out: a dict for a tensor obs": (good, ps, ps, {"out": {"a": z(4, 3)}}),
        "out: other agents": (two, ps, ps, {"out": {"a": z(4, 3), "c": z(4, 3)}}),
        "out: three agents": (two, ps, ps, {"out": {"a": z(4, 3), "b": z(4, 3), "c": z(4, 3)}}),
        "out: not a tensor": (good, ps, ps, {"out": "head"}),
        "out: float64": (good, ps, ps, {"out": z(4, 3, dtype=torch.float64)}),
        "out: rows: wrong width": (good, ps, ps, {"out": z(4, 4)}),
        "out: rows: last dimension strided": (good, ps, ps, {"out": z(4, 6)[:, ::2]}),
        "out: rows: rows overlap": (good, ps, ps, {"out": z(1, 3).expand(4, 3)}),
        "out: rows: two row strides": (two, ps, ps, {"out": {"a": z(4, 3), "b": z(4, 6)[:, :3]}}),
        "out_dtype: float64": (good, ps, ps, {"out_dtype": torch.float64}),
        "valid: out given": (two, ps, ps, {"out": {"a": z(4, 8)[:, :3], "b": z(4, 8)[:, :3]}, "out_dtype": None}),
    }
    plan = pool.Plan(z(pool.capacity(4, 2), dtype=torch.int32), z(3, dtype=torch.int32), z(1, dtype=torch.int32), 4, 2)
    of_three = pool.Plan(plan.order, plan.first, plan.errors, 3, 2)
    pools = {     # the plan check sits between the parameter shapes and out
        "plans: a bad shape comes first": (good, ps, put(ps, 5, z(4)), {"plans": of_three, "out": z(4, 4)}),
        "plans: then the plan, then out": (good, ps, ps, {"plans": of_three, "out": z(4, 4)}),
        "plans: not a plan": (good, ps, ps, {"plans": "plan"}),
        "plans: a dict for a tensor obs": (good, ps, ps, {"plans": {"a": None}}),
        "valid: a plan": (good, ps, ps, {"plans": plan}),
    }
    grads = {     # netgrad.backward: grad_head through the same helpers, and the workspace
        "grad_head: three agents": (good, ps, ps, {"grad_head": {"a": good, "b": good, "c": good}}),
        "grad_head: not a tensor": (good, ps, ps, {"grad_head": None}),
        "grad_head: a dict for a tensor obs": (good, ps, ps, {"grad_head": {"a": z(4, 3)}}),
        "grad_head: int32": (good, ps, ps, {"grad_head": z(4, 3, dtype=torch.int32)}),
        "grad_head: rows: wrong width": (good, ps, ps, {"grad_head": z(4, 4)}),
        "grad_head: rows: last dimension strided": (good, ps, ps, {"grad_head": z(4, 6)[:, ::2]}),
        "grad_head: rows: rows overlap": (good, ps, ps, {"grad_head": z(1, 3).expand(4, 3)}),
        "grad_head: rows: two row strides": (two, ps, ps, {"grad_head": {"a": z(4, 3), "b": z(4, 6)[:, :3]}}),
        "workspace: too small": (good, ps, ps, {"workspace": z(16, dtype=torch.uint8)}),
        "workspace: not a tensor": (good, ps, ps, {"workspace": 4096}),
        "workspace: float32": (good, ps, ps, {"workspace": z(1 << 16)}),
        "workspace: not aligned": (good, ps, ps, {"workspace": z(1 << 16, dtype=torch.uint8)[1:]}),
        "valid: out and workspace given": (good, ps, ps, {"out": [torch.zeros_like(p) for p in ps], "workspace": z(1 << 16, dtype=torch.uint8)}),
    }
    cases = {}
    for caller, f in mlp_callers().items():
        extra = {"net.forward": forwards, "pool.forward": {**forwards, **pools}, "netgrad.backward": grads}[caller]
        for name, (obs, first, second, kw) in {**shared, **extra}.items():
            cases[f"{caller}: {name}"] = lambda f=f, obs=obs, first=first, second=second, kw=kw: f(obs, first, second, **kw)
    return cases


# ---- the other functions -----------------------------------------------------------------------------------------------------
def sides_cases(call):
    """both raises of ``sides`` through `call`, a function of the argument that is a tensor or a dict of them"""
    t = z(4)
    return {"three agents": lambda: call({"a": t, "b": t, "c": t}), "no agent": lambda: call({}), "not a tensor": lambda: call([t]),
            "not a tensor in a dict": lambda: call({"a": 3})}


def other_cases():
    from pikazoo_amd import batch, league, learn, optim, policy, pool, ppo

    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    groups = {}
    # learn.gae
    rew, val, term = z(3, 4), z(4, 4), z(3, 4, dtype=torch.bool)
    groups["learn.gae"] = {
        **{f"rewards: {k}": v for k, v in sides_cases(lambda x: learn.gae(x, val, term)).items()},
        **{f"values: {k}": v for k, v in sides_cases(lambda x: learn.gae(rew, x, term)).items()},
        "valid": lambda: learn.gae(rew, val, term),
        "valid: two agents": lambda: learn.gae({"a": rew, "b": rew}, {"a": val, "b": val}, {"a": term, "b": term}),
    }
    # policy
    logits, actions = z(4, 6), z(4, dtype=i64)
    groups["policy.sample"] = {**{f"logits: {k}": v for k, v in sides_cases(lambda x: policy.sample(x, seed=0)).items()},
                               "valid": lambda: policy.sample(logits, seed=0),
                               "valid: two agents": lambda: policy.sample({"a": logits, "b": logits}, seed=0)}
    groups["policy.log_probs"] = {**{f"logits: {k}": v for k, v in sides_cases(lambda x: policy.log_probs(x, actions)).items()},
                                  "valid": lambda: policy.log_probs(logits, actions)}
    # ppo
    vec = z(4)
    rest = dict(actions=actions, old_log_probs=vec, advantages=vec, returns=vec)
    groups["ppo.moments"] = {**{f"advantages: {k}": v for k, v in sides_cases(ppo.moments).items()},
                             "valid": lambda: ppo.moments(vec), "valid: out and workspace given":
                             lambda: ppo.moments({"a": vec, "b": vec}, out=z(2, 2), workspace=z(64, dtype=u8))}
    for name, f in (("ppo.loss_and_grad", ppo.loss_and_grad), ("ppo.loss", ppo.loss)):
        groups[name] = {
            **{f"head: {k}": v for k, v in sides_cases(lambda x, f=f: f(head=x, num_actions=5, **rest)).items()},
            **{f"logits: {k}": v for k, v in sides_cases(lambda x, f=f: f(logits=x, values=vec, **rest)).items()},
            "valid": lambda f=f: f(logits=logits, values=vec, **rest),
            "valid: head": lambda f=f: f(head=z(4, 7), num_actions=6, **rest),
        }
    groups["ppo.loss"].update({f"values: {k}": v for k, v in sides_cases(lambda x: ppo.loss(logits=logits, values=x, **rest)).items()})
    # optim.adam_step
    p, g, m, v, step = [z(3), z(2, 2)], [z(3), z(2, 2)], [z(3), z(2, 2)], [z(3), z(2, 2)], z(2, dtype=i64)
    adam = lambda *a, **kw: optim.adam_step(*a, lr=1e-3, **kw)  # noqa: E731
    groups["optim.adam_step"] = {
        "step: not a tensor": lambda: adam(p, g, m, v, 5),
        "step: a tensor of three": lambda: adam(p, g, m, v, z(3, dtype=i64)),
        "stats: not a tensor": lambda: adam(p, g, m, v, step, stats=[0.0, 0.0]),
        "stats: int64": lambda: adam(p, g, m, v, step, stats=z(2, dtype=i64)),
        "overlap: a moment is its gradient": lambda: adam(p, g, [g[0], m[1]], v, step),
        "overlap: a parameter inside its gradient": lambda: adam([p[0], g[0][:2]], [g[0], z(2)], [m[0], z(2)], [v[0], z(2)], step),
        "overlap: both moments are one tensor": lambda: adam(p, g, m, [v[0], m[1]], step),
        "overlap: the statistics in a moment": lambda: adam(p, g, m, v, step, stats=m[0][:2]),
        "valid": lambda: adam(p, g, m, v, step),
        "valid: two nets, statistics": lambda: adam({"a": p, "b": [z(3)]}, {"a": g, "b": [z(3)]}, {"a": m, "b": [z(3)]}, {"a": v, "b": [z(3)]},
                                                    {"a": step, "b": z(2, dtype=i64)}, stats={"a": z(2), "b": z(2)}),
    }
    # batch
    src, dst, wide = z(4, 3), z(4, 3), z(4, 8)
    groups["batch.copy"] = {
        "overlap: a dst is its src": lambda: batch.copy([(src, src)]),
        "overlap: a dst inside another pair's src": lambda: batch.copy([(wide[:, :3], dst), (src, wide[:, 2:5])]),
        "overlap: two dst are one tensor": lambda: batch.copy([(src, dst), (z(4, 3), dst)]),
        "overlap: two dst interleave": lambda: batch.copy([(src, wide[:, :3]), (src, wide[:, 2:5])]),
        "valid": lambda: batch.copy([(src, dst), (wide[:, 7], z(4))]),
    }
    sources = {"x": z(2, 4, 3), "y": {"a": z(2, 4, dtype=i64)}}
    outs = {"x": z(4, 3), "y": {"a": z(4, dtype=i64)}}
    gather = lambda **kw: batch.gather(sources, 2, 0, **kw)  # noqa: E731
    groups["batch.gather"] = {
        "counter_dev: not a tensor": lambda: gather(counter_dev=3),
        "counter_dev: a tensor of two": lambda: gather(counter_dev=z(2, dtype=i64)),
        "counter_dev: int32": lambda: gather(counter_dev=z(1, dtype=i32)),
        "overlap: an output inside a source": lambda: gather(out={"x": sources["x"][0], "y": outs["y"]}),
        "overlap: index_out is the index": lambda: gather(index=outs["y"]["a"], out={"x": outs["x"], "y": {"a": z(4, dtype=i64)}},
                                                         index_out=outs["y"]["a"]),
        "overlap: two outputs are one tensor": lambda: batch.gather({"a": sources["x"], "b": sources["x"]}, 2, 0, out={"a": outs["x"], "b": outs["x"]}),
        "overlap: index_out inside an output": lambda: gather(out=outs, index_out=outs["y"]["a"]),
        "valid": lambda: gather(),
        "valid: everything given": lambda: gather(counter=3, counter_dev=z(1, dtype=i64), out=outs, index_out=z(4, dtype=i64),
                                                  errors=z(1, dtype=i32)),
    }
    # pool.plan
    cap = pool.capacity(5, 4)
    base = z(cap, dtype=i32)
    members = z(5, dtype=i64)
    plan_of = lambda order, first, errors: pool.Plan(order, first, errors, 5, 4)  # noqa: E731
    groups["pool.plan"] = {
        "overlap: the members inside out.order": lambda: pool.plan(base[:5], 4, out=plan_of(base, z(5, dtype=i32), z(1, dtype=i32))),
        "overlap: the members inside out.errors": lambda: pool.plan(base[:5], 4, out=plan_of(z(cap, dtype=i32), z(5, dtype=i32), base[4:5])),
        "overlap: out.first inside out.order": lambda: pool.plan(members, 4, out=plan_of(base, base[8:13], z(1, dtype=i32))),
        "overlap: out.errors inside out.first": lambda: pool.plan(members, 4, out=plan_of(z(cap, dtype=i32), base[:5], base[4:5])),
        "valid": lambda: pool.plan(members, 4),
        "valid: out given": lambda: pool.plan(members, 4, out=plan_of(base, z(5, dtype=i32), z(1, dtype=i32))),
    }
    # league
    term1, scores, mem = z(4, dtype=torch.bool), z(4, 2, dtype=i32), z(4, dtype=i64)
    table = z(1, 1, 4, dtype=i64)
    groups["league.tally"] = {
        "terminations: not a tensor": lambda: league.tally(3, scores, mem, 2),
        "terminations: float32": lambda: league.tally(z(4), scores, mem, 2),
        "scores: not a tensor": lambda: league.tally(term1, None, mem, 2),
        "scores: one column": lambda: league.tally(term1, z(4, 1, dtype=i32), mem, 2),
        "members: not a tensor": lambda: league.tally(term1, scores, [0, 0, 0, 0], 2),
        "members: two dimensions": lambda: league.tally(term1, scores, z(4, 1, dtype=i64), 2),
        "table: not a tensor": lambda: league.tally(term1, scores, mem, 2, table="table"),
        "table: int32": lambda: league.tally(term1, scores, mem, 2, table=z(2, 2, 4, dtype=i32)),
        "errors: not a tensor": lambda: league.tally(term1, scores, mem, 2, errors=0),
        "errors: two elements": lambda: league.tally(term1, scores, mem, 2, errors=z(2, dtype=i64)),
        "overlap: the members inside the table": lambda: league.tally(term1, scores, table.view(-1), 1, table=table),
        "overlap: the members_p1 inside errors": lambda: league.tally(z(1, dtype=torch.bool), z(1, 2, dtype=i32), z(1, dtype=i64), 1,
                                                                      members_p1=table.view(-1)[:1], errors=table.view(-1)[:1]),
        "overlap: errors inside the table": lambda: league.tally(term1, scores, mem, 1, table=table, errors=table.view(-1)[3:]),
        "valid": lambda: league.tally(term1, scores, mem, 2),
        "valid: everything given": lambda: league.tally(term1, scores, mem, 2, table=z(2, 2, 4, dtype=i64), members_p1=z(4, dtype=i64),
                                                        errors=z(1, dtype=i64)),
    }
    weights = torch.ones(4, dtype=i64)
    drawn, counter = z(4, dtype=i32), z(1, dtype=i64)
    groups["league.draw"] = {
        "weights: not a tensor": lambda: league.draw([1, 1], 4, 0),
        "weights: float32": lambda: league.draw(z(4), 4, 0),
        "counter: int32": lambda: league.draw(weights, 4, 0, counter=z(1, dtype=i32)),
        "mask: not a tensor": lambda: league.draw(weights, 4, 0, mask=True),
        "mask: int64": lambda: league.draw(weights, 4, 0, mask=z(4, dtype=i64)),
        "out: not a tensor": lambda: league.draw(weights, 4, 0, out=4),
        "out: float32": lambda: league.draw(weights, 4, 0, out=z(4)),
        "errors: not a tensor": lambda: league.draw(weights, 4, 0, errors=0),
        "errors: int64": lambda: league.draw(weights, 4, 0, errors=z(1, dtype=i64)),
        "overlap: out is the weights": lambda: league.draw(weights, 4, 0, out=weights),
        "overlap: errors inside the counter": lambda: league.draw(weights, 4, 0, counter=counter, errors=counter.view(i32)[1:]),
        "overlap: errors inside out": lambda: league.draw(weights, 4, 0, out=drawn, errors=drawn[3:]),
        "valid": lambda: league.draw(weights, 4, 0),
        "valid: everything given": lambda: league.draw(weights, 4, 0, counter=z(1, dtype=i64), mask=z(4, dtype=torch.bool), out=drawn,
                                                       errors=z(1, dtype=i32)),
    }
    return {f"{group}: {name}": f for group, cases in groups.items() for name, f in cases.items()}


ON_THE_GPU = {  # every function's own last check without a GPU: what its valid calls must end in
    "learn.gae": "gae() runs on the GPU: ", "policy.sample": "the policy head runs on the GPU: ", "policy.log_probs": "the policy head runs on the GPU: ",
    "ppo.moments": "the moments run on the GPU: ", "ppo.loss_and_grad": "the policy head runs on the GPU: ", "ppo.loss": "the policy head runs on the GPU: ",
    "net.forward": "the policy net runs on the GPU: ", "pool.forward": "the policy net runs on the GPU: ", "netgrad.backward": "the policy net runs on the GPU: ",
    "optim.adam_step": "the optimizer step runs on the GPU: ", "batch.copy": "the batch launches run on the GPU: ",
    "batch.gather": "the batch launches run on the GPU: ", "pool.plan": "the plan is built on the GPU: ",
    "league.tally": "the league launches run on the GPU: ", "league.draw": "the league launches run on the GPU: ",
}


def all_cases():
    return {**mlp_cases(), **other_cases()}


def outcome(f):
    """{"type", "text"} of the exception `f` raises; a call that raises nothing is an error of the table"""
    try:
        f()
    except Exception as e:  # noqa: BLE001 (the type is what is recorded)
        return {"type": type(e).__name__, "text": str(e)}
    raise AssertionError("the call raised nothing")


CASES = all_cases()


def test_the_table_covers_every_function_and_the_golden_file_every_case():
    golden = json.loads(GOLDEN.read_text())
    assert sorted(golden["cases"]) == sorted(CASES)
    assert len(golden["commit"]) == 40
    for function, words in ON_THE_GPU.items():
        valid = [name for name in CASES if name.startswith(f"{function}: valid")]
        assert valid, function
        for name in valid:
            got = golden["cases"][name]
            assert got["type"] == "ValueError" and got["text"].startswith(words) and got["text"].endswith(" on cpu"), (name, got)
    texts = " | ".join(c["text"] for c in golden["cases"].values())
    for sentence in ("a dict of one or two agents, got 3", "must be a tensor or a dict of tensors, got list", "outputs must not alias an input or each other",
                     "member 1: W2 must be a contiguous float32", "the workspace must be a contiguous uint8 tensor of at least",
                     "the last dimension must be contiguous (stride 2)", "rows overlap (row stride 0 < 5)", "must have the same row stride, got [5, 10]",
                     "got int", "got torch.float32 [4] on cpu"):
        assert sentence in texts, sentence


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_message_is_the_recorded_one(name):
    golden = json.loads(GOLDEN.read_text())["cases"]
    assert name in golden, f"{name} is not in {GOLDEN.name}: record it from the commit the file names"
    assert outcome(CASES[name]) == golden[name]


if __name__ == "__main__":
    out, commit = Path(sys.argv[1]), sys.argv[2]
    record = {"commit": commit, "cases": {name: outcome(f) for name, f in sorted(all_cases().items())}}
    out.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")
    print(f"{len(record['cases'])} cases recorded from {commit} into {out}")
